"""tests/trim_spec.py against cutadapt's documented example, its loop against the closed form a parallel kernel computes, and hand
cases for each step and for the order of the steps.  No device."""
import numpy as np

import trim_spec as ts
from trim_spec import DEFAULTS, Opts


def _q(vals, base=33):
    return bytes(v + base for v in vals)


def test_cutadapt_documented_example():
    """qualities 42 40 26 27 8 7 11 4 2 3 at cutoff 10: the partial sums from the end are (70) (38) 8 8 25 23 20 21 15 7, the
    largest is at the fifth base: four bases stay"""
    q = _q([42, 40, 26, 27, 8, 7, 11, 4, 2, 3])
    assert ts.quality_stop(b"A" * 10, q, 10, 33) == 4
    assert ts.quality_stop_closed(b"A" * 10, q, 10, 33) == 4


def test_loop_equals_closed_form():
    rng = np.random.default_rng(5)
    for _ in range(20_000):
        L = int(rng.integers(1, 40))
        base = 33 if rng.random() < 0.7 else 64
        kind = rng.integers(0, 3)
        vals = rng.integers(0, 42, L) if kind == 0 else rng.choice([2, 19, 20, 21, 40], L) if kind == 1 else np.full(L, 20)
        q = bytes(int(v) + base for v in vals)[:int(rng.integers(0, L + 1)) if rng.random() < 0.1 else L]
        c = int(rng.choice([1, 10, 20, 21, 30]))
        assert ts.quality_stop(b"A" * L, q, c, base) == ts.quality_stop_closed(b"A" * L, q, c, base), (vals, q, c, base)


def test_quality_hand_cases():
    s = b"A" * 8
    assert ts.quality_stop(s, _q([40] * 8), 20, 33) == 8                       # all high: untouched
    assert ts.quality_stop(s, _q([2] * 8), 20, 33) == 0                        # all low: nothing stays
    assert ts.quality_stop(s, _q([40] * 8), 0, 33) == 8                        # cutoff 0: the step is off
    assert ts.quality_stop(s, _q([40, 40, 40, 40, 40, 2, 2, 2]), 20, 33) == 5
    # good - bad - good: the good tail makes the sum negative before the bad stretch is reached -- the early break, nothing is cut
    assert ts.quality_stop(s, _q([40, 40, 2, 2, 2, 40, 40, 40]), 20, 33) == 8
    # ... and a single last base above the cutoff is enough for that; one AT the cutoff leaves the sum at 0 and the walk goes on
    assert ts.quality_stop(b"A" * 10, _q([40, 40, 2, 2, 2, 2, 2, 2, 2, 21]), 20, 33) == 10
    assert ts.quality_stop(b"A" * 10, _q([40, 40, 2, 2, 2, 2, 2, 2, 2, 20]), 20, 33) == 2
    # equal maxima: the rightmost one wins (the loop only moves on a larger sum)
    assert ts.quality_stop(b"A" * 6, _q([40, 40, 10, 20, 20, 10]), 20, 33) == 2
    assert ts.quality_stop(b"A" * 6, _q([40, 10, 30, 10, 30, 10]), 20, 33) == 5
    # Phred+64, and what a Phred+33 line looks like under it
    assert ts.quality_stop(s, _q([40, 40, 40, 40, 40, 2, 2, 2], 64), 20, 64) == 5
    assert ts.quality_stop(s, _q([40] * 8, 33), 20, 64) == 0
    # a short quality line: the missing characters are ' ' (below any Phred+33 quality)
    assert ts.quality_stop(s, _q([40] * 5), 20, 33) == 5


def test_adapter_hand_cases():
    A = "AGATCGGAAGAGC"
    read = b"ACGTTGCAACGTTGCAACGT"
    for i in range(len(read)):
        # (the insert has no chance hit that an overlap of 3 accepts)
        assert ts.adapter_start(read[:i] + A.encode(), i + 13, A, 3, 100) == i, i
    assert ts.adapter_start(A.encode() + read, 33, A, 1, 100) == 0
    # partial overlaps at the end: every length down to min_overlap
    for o in range(1, 13):
        s = read + A[:o].encode()
        assert ts.adapter_start(s, len(s), A, o, 0) == len(read)
        assert ts.adapter_start(s, len(s), A, o + 1, 0) == len(s)
    # one mismatch in 13 is within 13 * 100 // 1000 = 1, two are not; below ten letters of overlap nothing is allowed
    one = read + b"AGATCGGTAGAGC"
    two = read + b"AGTTCGGTAGAGC"
    assert ts.adapter_start(one, len(one), A, 5, 100) == len(read)
    assert ts.adapter_start(two, len(two), A, 5, 100) == len(two)
    assert ts.adapter_start(read + b"AGATCGGTA", 29, A, 5, 100) == 29
    # lower case compares as upper case; N matches nothing
    assert ts.adapter_start(read.lower() + A.lower().encode(), 33, A, 5, 0) == len(read)
    assert ts.adapter_start(read + b"AGATCGGNAGAGC", 33, A, 5, 0) == 33
    assert ts.adapter_start(read + b"AGATCGGNAGAGC", 33, A, 5, 100) == len(read)
    # the leftmost accepted start, not the best one: a chance 'A' in front of a full copy
    s = b"CCCCCCA" + b"CC" + A.encode()
    assert ts.adapter_start(s, len(s), A, 1, 100) == 9                        # ('A' + 'CC...' has too many mismatches for its overlap)
    assert ts.adapter_start(b"CCCCCCA", 7, A, 1, 100) == 6
    assert ts.adapter_start(read, len(read), "", 1, 100) == len(read)


def test_order_of_the_steps():
    A = "AGATCGGAAGAGC"
    o = Opts(20, (A, A), 1, 100, 20, (0, 0), (0, 0), 33)
    ins = b"ACGTTGCAACGTTGCAACGTTGCAACGTTGCC"
    # quality first: an adapter in the low-quality tail is gone before the adapter step looks
    s = ins + A.encode()
    t = ts.trim_record(s, _q([40] * 32 + [2] * 13), 0, o)
    assert (t.after_quality, t.after_adapter, t.L, t.k) == (32, 32, 32, 0)
    t = ts.trim_record(s, _q([40] * 45), 0, o)
    assert (t.after_quality, t.after_adapter, t.L) == (45, 32, 32)
    # clips come after both, the 3' clip before the 5' clip; the quality line follows the sequence
    o2 = o._replace(clip_5p=(3, 30), clip_3p=(4, 10))
    t = ts.trim_record(s, _q([40] * 45), 0, o2)
    assert (t.k, t.L, t.qual_len) == (3, 25, 25)
    t = ts.trim_record(s, _q([40] * 45), 1, o2)
    assert (t.k, t.L, t.qual_len) == (22, 0, 0)                               # 32 - 10 = 22 left, all of it clipped at the 5' end
    t = ts.trim_record(s, _q([40] * 2), 0, o2._replace(quality=0))
    assert (t.k, t.L, t.qual_len) == (3, 25, 0)                               # a quality line shorter than the clip
    t = ts.trim_record(s, _q([40] * 10), 0, o2._replace(quality=0))
    assert (t.k, t.L, t.qual_len) == (3, 25, 7)


def test_trim_fastq_filters_templates_and_counts():
    A = "AGATCGGAAGAGC"
    o = DEFAULTS
    good = b"ACGTTGCAACGTTGCAACGTTGCAACGTTGCC"
    hi = _q([40] * 32)
    t1 = b"@a/1\n" + good + b"\n+\n" + hi + b"\n@b/1\n" + good[:10] + A.encode() + good[:9] + b"\n+\n" + hi + b"\n@c/1\n" + good + b"\n+\n" + hi + b"\n"
    t2 = b"@a/2\n" + good + b"\n+\n" + hi + b"\n@b/2\n" + good + b"\n+\n" + hi + b"\n@c/2\n" + good + b"\n+\n" + _q([40] * 12 + [2] * 20) + b"\n"
    o1, o2, kept, cnt = ts.trim_fastq(t1, t2, o)
    assert kept == 1 and cnt["templates_dropped"] == 2
    assert o1 == b"@a/1\n" + good + b"\n+\n" + hi + b"\n" and o2 == b"@a/2\n" + good + b"\n+\n" + hi + b"\n"
    assert cnt["records_in"] == [3, 3] and cnt["bases_in"] == [96, 96] and cnt["bases_out"] == [32, 32]
    assert cnt["adapter_records"] == [1, 0] and cnt["adapter_bases"] == [22, 0]
    assert cnt["quality_records"] == [0, 1] and cnt["quality_bases"] == [0, 20]
    # single end: the same file alone keeps two
    o1, none, kept, cnt = ts.trim_fastq(t1, None, o)
    assert none is None and kept == 2 and o1.count(b"\n") == 8 and cnt["templates_dropped"] == 1
