"""tests/nonconv_spec.py on hand-made records with known answers (no GPU), and a look at the random records tests/test_nonconv.py
feeds the device: they are not trivial for this rule."""
import numpy as np
import pytest

import methyl_spec as spec
import nonconv_spec as nc
from nonconv_spec import Params

# sequence 0: forward C in CHH context at 2, 5, ..., 29 (C A A), a CpG at 32, a CHG at 35; sequence 1: forward G in CHH context (a
# cytosine of the reverse strand) at 4, 7, ..., 31 (T T G)
TEXT = ("TT" + "CAA" * 10 + "CGT" + "CAG" + "TT", "AA" + "TTG" * 10 + "AA")
SEQS = [bytes("ACGT".index(c) for c in t) for t in TEXT]
CHH0 = list(range(2, 32, 3))
CHH1 = list(range(4, 34, 3))


def test_the_tiny_genome_is_what_the_comments_say():
    assert [p for p in range(len(SEQS[0])) if spec.context(SEQS[0], p) == (spec.CHH, 0)] == CHH0
    assert spec.context(SEQS[0], 32) == (spec.CPG, 0) and spec.context(SEQS[0], 33) == (spec.CPG, 1)
    assert spec.context(SEQS[0], 35) == (spec.CHG, 0) and spec.context(SEQS[0], 37) == (spec.CHG, 1)
    assert [p for p in range(len(SEQS[1])) if spec.context(SEQS[1], p) == (spec.CHH, 1)] == CHH1
    assert not any(c == 1 for c in SEQS[1])


def read(ref, pos, length, keep, flag=0, quals=None, mapq=30, cigar=None, low=()):
    """a record that shows reference bases pos .. pos + length - 1 of sequence ref under one M (or `cigar`, whose read-consuming
    operations are filled from the reference in order): the cytosines of its strand (C for OT, G for OB) at the positions in `keep`
    stay, every other one reads T (A); quality 30, 19 at the reference positions in `low`"""
    ob = spec.is_ob(flag)
    a, b = ("G", "A") if ob else ("C", "T")
    text = TEXT[ref]
    shown = [(p, b if text[p] == a and p not in keep else text[p]) for p in range(pos, pos + length)]
    if cigar is None:
        cigar = [("M", length)]
    seq, q, at = [], [], 0
    for op, ln in cigar:
        if op in "M=X":
            seq += [c for _p, c in shown[at:at + ln]]
            q += [19 if p in low else 30 for p, _c in shown[at:at + ln]]
            at += ln
        elif op in "DN":
            at += ln
        elif op in "IS":
            seq += [a] * ln                                                      # an unconverted cytosine that is no call
            q += [30] * ln
    return spec.make_record(ref, pos, flag, cigar, seq, q if quals is None else quals, mapq=mapq)


def test_threshold_exactly_and_one_below():
    two, three = read(0, 0, 32, CHH0[:2]), read(0, 0, 32, CHH0[:3])
    assert nc.counts(two, SEQS) == (2, 8) and nc.counts(three, SEQS) == (3, 7)
    assert nc.templates(SEQS, [two, three], False) == [0, 1]
    assert nc.templates(SEQS, [two, three], False, Params(2, 0, 5, 0)) == [1, 1]
    assert nc.templates(SEQS, [two, three], False, Params(0, 0, 5, 0)) == [0, 0]                    # both switches off: nothing fails
    assert nc.totals(SEQS, [two, three]) == [[[0, 0], [0, 0], [15, 5]], [[0, 0]] * 3]


def test_cpg_calls_count_for_the_totals_only():
    r = read(0, 0, 40, CHH0[:2] + [32, 35])
    assert nc.tally(r, SEQS) == [[0, 1], [0, 1], [8, 2]] and nc.counts(r, SEQS) == (3, 8)
    r = read(0, 0, 40, CHH0[:2] + [32])
    assert nc.counts(r, SEQS) == (2, 9) and nc.templates(SEQS, [r], False) == [0]


def test_percent_rule_at_equality_one_below_and_below_min_count():
    p = Params(0, 50, 5, 0)
    half, below, few = read(0, 2, 18, CHH0[:3]), read(0, 2, 18, CHH0[:2]), read(0, 2, 12, CHH0[:4])
    assert nc.counts(half, SEQS) == (3, 3) and nc.counts(below, SEQS) == (2, 4) and nc.counts(few, SEQS) == (4, 0)
    assert nc.templates(SEQS, [half, below, few], False, p) == [1, 0, 0]
    assert nc.templates(SEQS, [few], False, Params(0, 50, 4, 0)) == [1]
    assert nc.fails(1, 1, Params(0, 50, 0, 0)) and not nc.fails(0, 0, Params(0, 0, 0, 0)) and nc.fails(0, 0, Params(0, 100, 0, 0)) is True
    assert nc.fails(2 ** 31, 2 ** 31, Params(0, 50, 5, 0)) and not nc.fails(2 ** 31 - 1, 2 ** 31, Params(0, 50, 5, 0))
    with pytest.raises(ValueError):
        nc.templates(SEQS, [half], False, Params(0, 101, 5, 0))
    with pytest.raises(ValueError):
        nc.templates(SEQS, [half], False, Params(-1, 0, 5, 0))
    with pytest.raises(ValueError):
        nc.templates(SEQS, [half], False, Params(3, 0, 5, 256))


def test_a_methylated_call_taken_away():
    base = read(0, 0, 32, CHH0[:3])
    assert nc.templates(SEQS, [base], False) == [1]
    # an unconverted cytosine inside an insertion or a soft clip is a read base without a reference position
    ins = read(0, 0, 32, CHH0[:2], cigar=[("M", 4), ("I", 1), ("M", 28)])
    soft = read(0, 0, 32, CHH0[:2], cigar=[("S", 2), ("M", 32), ("S", 1)])
    assert spec.fields(ins)[5].count(spec.SEQ_C) == 3 and spec.fields(soft)[5].count(spec.SEQ_C) == 5
    assert nc.counts(ins, SEQS) == (2, 8) and nc.counts(soft, SEQS) == (2, 8)
    # the third methylated position lies in a deletion: no read base stands against it
    dele = read(0, 0, 32, CHH0[:3], cigar=[("M", 7), ("D", 3), ("M", 22)])
    assert nc.counts(dele, SEQS) == (2, 7)
    # a quality below min_phred
    low = read(0, 0, 32, CHH0[:3], low=(CHH0[2],))
    assert nc.counts(low, SEQS, 19) == (3, 7) and nc.counts(low, SEQS, 20) == (2, 7)
    assert nc.templates(SEQS, [ins, soft, dele, low], False) == [0, 0, 0, 1]
    assert nc.templates(SEQS, [low], False, Params(3, 0, 5, 20)) == [0]


def test_an_ob_record():
    two, three = read(1, 0, 34, CHH1[:2], flag=16), read(1, 0, 34, CHH1[:3], flag=16)
    assert nc.counts(two, SEQS) == (2, 8) and nc.counts(three, SEQS) == (3, 7)
    assert nc.templates(SEQS, [two, three], False) == [0, 1]
    assert nc.totals(SEQS, [two, three]) == [[[0, 0]] * 3, [[0, 0], [0, 0], [15, 5]]]
    # the same bases read as OT call nothing: sequence 1 has no forward C
    assert nc.counts(read(1, 0, 34, CHH1[:3], flag=0), SEQS) == (0, 0)


def test_a_pair_failed_by_read_2_alone_whose_read_1_is_unmapped():
    r1 = spec.make_record(-1, -1, 0x45, [], "ACGT", [30] * 4)
    r2 = read(1, 0, 34, CHH1[:3], flag=0x89)                                      # read 2 forward: OB
    good = [read(0, 0, 32, CHH0[:1], flag=0x63), read(0, 2, 32, CHH0[:2], flag=0x93)]
    recs = [r1, r2] + good
    assert nc.counts(r1, SEQS) == (0, 0) and nc.counts(r2, SEQS) == (3, 7)
    failed = nc.templates(SEQS, recs, True)
    assert failed == [1, 0]
    marked = nc.mark(recs, True, failed)
    assert [spec.fields(r)[3] for r in marked] == [0x245, 0x289, 0x63, 0x93]
    assert all(len(a) == len(b) and sum(x != y for x, y in zip(a, b)) == (1 if i < 2 else 0) for i, (a, b) in enumerate(zip(recs, marked)))
    # holes: a template without records does not fail; a record beside a hole decides alone
    assert nc.templates(SEQS, [b"", b"", r2, b""], True) == [0, 1]


def test_secondary_and_supplementary_are_not_examined_but_duplicates_qc_fails_and_low_mapq_are():
    for flag in (0x100, 0x800, 0x900):
        r = read(0, 0, 32, CHH0, flag=flag)
        assert not nc.examined(r) and nc.counts(r, SEQS) == (0, 0) and nc.templates(SEQS, [r], False) == [0]
        assert nc.totals(SEQS, [r]) == [[[0, 0]] * 3] * 2
    for flag, mapq in ((0x400, 30), (0x200, 30), (0, 0), (0x41, 30), (0x1, 30)):
        r = read(0, 0, 32, CHH0[:3], flag=flag, mapq=mapq)
        assert nc.examined(r) and nc.templates(SEQS, [r], False) == [1], (flag, mapq)
    assert not nc.examined(spec.make_record(0, 0, 4, [("M", 4)], "CCCC", [30] * 4)) and not nc.examined(spec.make_record(0, 0, 0, [], "CCCC", [30] * 4))
    assert not nc.examined(b"") and not nc.examined(None)


def test_report_text():
    tot = [[[1, 3], [0, 0], [199, 1]], [[5, 5], [2, 0], [98, 0]]]
    assert nc.report_text(tot, 10, 2) == (
        b"#strand\tcontext\tmethylated\tunmethylated\tpercent\n"
        b"OT\tCpG\t3\t1\t75\nOT\tCHG\t0\t0\tNA\nOT\tCHH\t1\t199\t1\n"
        b"OB\tCpG\t5\t5\t50\nOB\tCHG\t0\t2\t0\nOB\tCHH\t0\t98\t0\n"
        b"non-CpG conversion rate\t299\t300\t99.67\ntemplates\t10\tfailed\t2\n")
    assert nc.report_text([[[0, 0]] * 3] * 2, 0, 0).endswith(b"non-CpG conversion rate\t0\t0\tNA\ntemplates\t0\tfailed\t0\n")
    assert b"\t1\t8\t12.50\n" in nc.report_text([[[0, 0], [1, 7], [0, 0]], [[0, 0]] * 3], 1, 1)          # 12.5 exactly
    assert b"\t1\t3\t33.33\n" in nc.report_text([[[0, 0], [1, 2], [0, 0]], [[0, 0]] * 3], 1, 1)
    assert b"\t2\t3\t66.67\n" in nc.report_text([[[0, 0], [2, 1], [0, 0]], [[0, 0]] * 3], 1, 1)


def test_the_random_records_of_the_device_tests_are_not_trivial():
    """test_mbias_spec.random_records with the lengths of tests/test_mbias.py, as tests/test_nonconv.py makes them"""
    import test_mbias
    from test_mbias_spec import golden_seqs, random_records
    seqs = golden_seqs()
    recs = random_records(np.random.default_rng(23), seqs, 4000, test_mbias.L_SEQS)
    tallies = [nc.tally(r, seqs) for r in recs]
    seen = [t for t in tallies if t is not None]
    assert 100 < len(seen) < len(recs) - 100
    nm = [nc.counts_of(t)[0] for t in seen]
    for k in range(5):
        assert nm.count(k) > 20, k                                              # none, below, at and above the threshold of 3
    p50 = Params(0, 50, 5, 0)
    at_half = [t for t in seen if sum(nc.counts_of(t)) >= 5 and 2 * nc.counts_of(t)[0] == sum(nc.counts_of(t))]
    assert len(at_half) > 20 and all(nc.fails(*nc.counts_of(t), p50) for t in at_half)
    assert any(sum(nc.counts_of(t)) == 4 and nc.counts_of(t)[0] >= 2 for t in seen)                   # min_count - 1 calls, above the percent
    assert any(nc.fails(*nc.counts_of(t), p50) != nc.fails(*nc.counts_of(t)) for t in seen)
    # taken as pairs: every combination of {fails, passes, not examined} x 2
    kind = [2 if t is None else int(nc.fails(*nc.counts_of(t))) for t in tallies]
    pairs = {(kind[i], kind[i + 1]) for i in range(0, len(kind), 2)}
    assert pairs == {(a, b) for a in range(3) for b in range(3)}
    assert 0 < sum(nc.verdicts(tallies, True)) < len(recs) // 2
    # all twelve totals are fed
    assert all(x > 100 for s in nc.totals_of(recs, tallies) for ctx in s for x in ctx)
