"""Trimming in the text calls on the device (bmbs_set_trim, bmbs_text_trim_counts, bmbs_trim_text, `bmbs_search --trim`) against
tests/trim_spec.py.  The stage is compared field for field; a call with trimming on the raw text is compared byte for byte with the same
call, trimming off, on the text the spec trims.  Everything is integers and bytes: every comparison here is exact."""
import json
import os
import subprocess

import numpy as np
import pytest

import trim_spec as ts
from common import GOLD, bam_payload, bgzf_blocks, golden_args, write_bgzf
from test_methyl import _driver, _fastq_records, gold  # noqa: F401  (fixture)
from test_sorted_bam import split_records
from trim_spec import DEFAULTS, Opts

pytestmark = pytest.mark.gpu

A13 = "AGATCGGAAGAGC"
A32 = "AGATCGGAAGAGCACACGTCTGAACTCCAGTC"
LENGTHS = (1, 15, 16, 17, 31, 32, 33, 150, 255, 256, 257, 998)


def _set(m, o: Opts):
    m.set_trim(quality=o.quality, adapter=o.adapter[0], adapter2=o.adapter[1], min_overlap=o.min_overlap, error_permille=o.error_permille,
               min_length=o.min_length, clip_5p=o.clip_5p, clip_3p=o.clip_3p)


def _text(recs):
    """records (name without '@', sequence, quality) -> the FASTQ text, and where each sequence and quality line begins"""
    out = bytearray()
    so, qo = [], []
    for name, s, q in recs:
        out += b"@" + name + b"\n"
        so.append(len(out)); out += s + b"\n+\n"
        qo.append(len(out)); out += q + b"\n"
    return bytes(out), so, qo


def _check_stage(m, recs, o: Opts, mate=0):
    text, so, qo = _text(recs)
    _set(m, o)
    got = m.trim_text(text, len(recs), mate)
    want = [ts.trim_record(s, q, mate, o) for _, s, q in recs]
    assert got[0].tolist() == [a + t.k for a, t in zip(so, want)]
    assert got[1].tolist() == [a + t.k for a, t in zip(qo, want)]
    assert got[2].tolist() == [t.L for t in want]
    assert got[3].tolist() == [t.qual_len for t in want]
    return want


def _q(vals, base=33):
    return bytes(int(v) + base for v in vals)


def _mut(a: str, where):
    """the adapter with the letters at `where` replaced by ones that differ"""
    b = bytearray(a.encode())
    for j in where:
        b[j] = ord("C") if b[j] != ord("C") else ord("T")
    return bytes(b)


def _crafted():
    """the records of the stage tests, by family; names of varying length put the lines at every byte alignment.  No GPU."""
    rng = np.random.default_rng(11)
    fam = {}

    def ins(n, letters=b"CGT"):
        return bytes(rng.choice(list(letters), n).astype(np.uint8))

    def quals(n, kind, base=33):
        if kind == 0:
            v = rng.integers(2, 42, n)
        elif kind == 1:                                # a good read with a bad tail
            v = np.full(n, 38); v[n - int(rng.integers(0, n + 1)):] = rng.integers(2, 25, 1)[0]
        elif kind == 2:                                # good - bad - good
            v = np.full(n, 38); a = int(rng.integers(0, n)); b = int(rng.integers(a, n)); v[a:b] = 2
            v[b:] = rng.choice([19, 20, 21, 38])
        else:                                          # at the cutoff and one beside it: equal maxima
            v = rng.choice([19, 20, 21], n)
        return _q(v, base)

    recs = []
    for L in LENGTHS:
        for kind in range(4):
            for rep in range(3):
                s = ins(L, b"ACGT")
                if L > 40 and rep:
                    at = int(rng.integers(0, L - 5)); s = (s[:at] + A13.encode() + ins(L))[:L]
                recs.append((s, quals(L, kind)))
    fam["lengths"] = recs
    fam["all_high"] = [(ins(L, b"ACGT"), _q([40] * L)) for L in LENGTHS]
    fam["all_low"] = [(ins(L, b"ACGT"), _q([2] * L)) for L in LENGTHS]
    fam["short_quality"] = [(ins(L, b"ACGT"), quals(L, k)[:int(rng.integers(0, L))]) for L in LENGTHS for k in range(4)]
    fam["lower_and_n"] = [((ins(20) + A13.lower().encode() + ins(7)), _q([38] * 40)), ((ins(20) + b"AGATCGGNAGAGC" + ins(7)), _q([38] * 40)),
                          ((ins(20).lower() + b"AgAtCgGaAgAgC" + ins(7)), _q([38] * 40)), (b"N" * 40, _q([38] * 40)), (b"n" * 17 + A13.encode(), _q([38] * 30))]
    fam["break"] = [(ins(8, b"ACGT"), _q(v)) for v in ([40, 40, 2, 2, 2, 40, 40, 40], [40, 40, 2, 2, 2, 2, 2, 21], [40, 40, 2, 2, 2, 2, 2, 20], [2, 2, 2, 2, 2, 2, 2, 40])]
    fam["equal_maxima"] = [(ins(6, b"ACGT"), _q(v)) for v in ([40, 40, 10, 20, 20, 10], [40, 10, 30, 10, 30, 10], [20] * 6, [10, 30, 10, 30, 10, 30])]
    # the adapter at every start of a 40-base read (the rest of the read: letters the adapter does not begin with)
    fam["every_start"] = [((ins(i) + A13.encode() + ins(40))[:40], _q([38] * 40)) for i in range(40)]
    fam["every_start_32"] = [((ins(i) + A32.encode() + ins(40))[:40], _q([38] * 40)) for i in range(40)]
    fam["partial"] = [(ins(30) + A13[:o].encode(), _q([38] * (30 + o))) for o in range(1, 13)] + [(ins(30) + A32[:o].encode(), _q([38] * (30 + o))) for o in range(1, 32)]
    fam["at_zero"] = [(A13.encode() + ins(27), _q([38] * 40)), (A32.encode() + ins(8), _q([38] * 40)), (A13.encode(), _q([38] * 13)), (b"A", _q([38]))]
    # mismatches at the bound (13 * 100 // 1000 = 1, 32 * 100 // 1000 = 3) and one above it
    fam["mismatches_13"] = [(ins(20) + _mut(A13, w) + ins(7), _q([38] * 40)) for w in ((), (6,), (0,), (12,), (3, 9), (0, 12))]
    fam["mismatches_32"] = [(ins(20) + _mut(A32, w) + ins(8), _q([38] * 60)) for w in ((), (5, 15, 25), (0, 16, 31), (5, 15, 25, 30), (0, 1, 2, 3))]
    for k, v in fam.items():
        fam[k] = [(b"%s%d%s" % (k.encode(), i, b"x" * int(rng.integers(0, 16))), s, q) for i, (s, q) in enumerate(v)]
    return fam


@pytest.fixture(scope="module")
def crafted():
    return _crafted()


@pytest.fixture(scope="module")
def stage_mapper():
    """a context without an index: the stage needs none"""
    from bitmapperbs_amd import mapper
    m = mapper.Mapper(None, 0)
    yield m
    m.close()


OPTS = {
    "defaults": DEFAULTS,
    "overlap5": DEFAULTS._replace(min_overlap=5),
    "a32": DEFAULTS._replace(adapter=(A32, A32), min_overlap=5),
    "exact": DEFAULTS._replace(error_permille=0, min_overlap=3),
    "loose": DEFAULTS._replace(error_permille=1000),
    "no_quality": DEFAULTS._replace(quality=0),
    "no_adapter": DEFAULTS._replace(adapter=("", "")),
    "q30": DEFAULTS._replace(quality=30, adapter=("", "")),
    "clips": DEFAULTS._replace(clip_5p=(3, 0), clip_3p=(4, 0)),
    "big_clips": DEFAULTS._replace(clip_5p=(20, 0), clip_3p=(14, 0), quality=0),
    "huge_clips": DEFAULTS._replace(clip_5p=(1000, 0), clip_3p=(0, 0), quality=0, adapter=("", "")),
    "huge_3p": DEFAULTS._replace(clip_5p=(5, 0), clip_3p=(2000, 0)),
}


@pytest.mark.parametrize("name", sorted(OPTS))
def test_stage_equals_the_spec_field_for_field(crafted, stage_mapper, name):
    o = OPTS[name]
    recs = [r for k in sorted(crafted) for r in crafted[k]]
    text, so, qo = _text(recs)
    assert {a % 16 for a in so} == set(range(16)) and {a % 16 for a in qo} == set(range(16))      # every alignment of both lines
    want = _check_stage(stage_mapper, recs, o)
    if name == "defaults":
        assert any(t.after_quality < len(r[1]) for t, r in zip(want, recs)) and any(t.after_adapter < t.after_quality for t in want)
        assert any(t.L == 0 for t in want) and any(t.L > 900 for t in want)
    if name == "clips":
        assert any(t.k == 3 for t in want) and any(t.L > 100 for t in want)
    if name == "big_clips":                            # (no quality step: a short quality line stays short; reads shorter than the clips)
        assert any(0 < t.qual_len < t.L for t in want) and any(0 < t.k < 20 for t in want) and any(t.k == 20 and t.qual_len == 0 and t.L for t in want)


def test_stage_families_do_what_they_are_for(crafted, stage_mapper):
    """the spec's own answers on the crafted families: the cases are the cases they claim to be (and the device agrees)"""
    o5 = DEFAULTS._replace(min_overlap=5)
    want = _check_stage(stage_mapper, crafted["every_start"], o5)
    assert [t.L for t in want] == [i if 40 - i >= 5 else 40 for i in range(40)]
    want = _check_stage(stage_mapper, crafted["every_start_32"], OPTS["a32"])
    assert [t.L for t in want] == [i if 40 - i >= 5 else 40 for i in range(40)]
    want = _check_stage(stage_mapper, crafted["partial"], DEFAULTS)
    assert all(t.L == 30 for t in want)
    want = _check_stage(stage_mapper, crafted["partial"], o5)
    assert [t.L for t in want[:12]] == [30 + o if o < 5 else 30 for o in range(1, 13)]
    want = _check_stage(stage_mapper, crafted["at_zero"], DEFAULTS)
    assert all(t.L == 0 for t in want)
    want = _check_stage(stage_mapper, crafted["mismatches_13"], o5)
    assert [t.L for t in want] == [20, 20, 20, 20, 40, 40]
    want = _check_stage(stage_mapper, crafted["mismatches_32"], OPTS["a32"])
    assert [t.L for t in want] == [20, 20, 20, 60, 60]
    want = _check_stage(stage_mapper, crafted["all_high"], DEFAULTS._replace(adapter=("", "")))
    assert [t.L for t in want] == list(LENGTHS)
    want = _check_stage(stage_mapper, crafted["all_low"], DEFAULTS)
    assert all(t.L == 0 for t in want)
    want = _check_stage(stage_mapper, crafted["break"], DEFAULTS._replace(adapter=("", "")))
    assert [t.L for t in want] == [8, 8, 2, 8]
    want = _check_stage(stage_mapper, crafted["equal_maxima"], DEFAULTS._replace(adapter=("", "")))
    assert [t.L for t in want] == [2, 5, 6, 6]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 16, 17])
def test_stage_with_a_wave_or_block_that_is_not_full(crafted, stage_mapper, n):
    _check_stage(stage_mapper, crafted["lengths"][40:40 + n], DEFAULTS)


def test_stage_second_mate_and_phred64(crafted):
    """mate 1's adapter and clips differ from mate 0's; a context with Phred+64 reads the same bytes 31 lower"""
    from bitmapperbs_amd import mapper
    o = DEFAULTS._replace(adapter=(A13, A32), clip_5p=(0, 2), clip_3p=(0, 1), min_overlap=3)
    m = mapper.Mapper(None, 0)
    recs = crafted["every_start"] + crafted["every_start_32"] + crafted["lengths"][:60]
    w0 = _check_stage(m, recs, o, mate=0)
    w1 = _check_stage(m, recs, o, mate=1)
    assert [t.L for t in w0] != [t.L for t in w1]
    m.close()
    m = mapper.Mapper(None, 0, q_base=64)
    rng = np.random.default_rng(3)
    r64 = [(b"p%d" % i, s, _q(rng.integers(2, 42, len(s)), 64)) for i, (_, s, _) in enumerate(crafted["lengths"])]
    o64 = DEFAULTS._replace(base=64)
    w = _check_stage(m, r64, o64)
    assert any(0 < t.after_quality < len(r[1]) for t, r in zip(w, r64))
    w33 = _check_stage(m, crafted["all_high"], o64._replace(adapter=("", "")))        # Phred+33 bytes under Phred+64: all below the cutoff
    assert all(t.L == 0 for t in w33)
    m.close()


def test_refusals(stage_mapper):
    m = stage_mapper
    for kw, what in ((dict(adapter="ACGN"), "ACGT"), (dict(adapter2="AC-T"), "ACGT"), (dict(min_length=0), "min_length"), (dict(error_permille=1001), "error_permille"),
                     (dict(error_permille=-1), "negative"), (dict(quality=-1), "negative"), (dict(min_overlap=-2), "negative"), (dict(clip_5p=(0, -1)), "negative"),
                     (dict(clip_3p=-3), "negative")):
        with pytest.raises(RuntimeError, match=r"bmbs error -22: .*" + what):
            m.set_trim(**kw)
    with pytest.raises(ValueError, match="32"):
        m.set_trim(adapter="A" * 33)
    m.set_trim(off=True)
    with pytest.raises(RuntimeError, match="bmbs error -1: .*off"):
        m.trim_text(b"@a\nACGT\n+\nIIII\n", 1)
    with pytest.raises(RuntimeError, match="bmbs error -1: "):
        m.trim_counts()
    m.set_trim()
    with pytest.raises(RuntimeError, match="bmbs error -22: .*fewer than 4 lines"):
        m.trim_text(b"@a\nACGT\n+\nIIII\n", 2)
    assert [a.tolist() for a in m.trim_text(b"@a\nACGT\n+\nIIII\n", 1)] == [[3], [10], [4], [4]]


# ---- equivalence: a call with trimming on the raw text == the call without on the spec's text -------------------------------------------
def _raw_records(recs, rng, drop, mate="", clean=False):
    """golden reads made raw: adapter read-through behind a shortened insert, low-quality tails, lower case; `drop`[i]: record i is left
    with an insert below the minimum length; clean: the golden qualities (random ones) give way to high ones first"""
    out = []
    for i, r in enumerate(recs):
        s, q = r[1].encode(), bytearray(r[3].encode())
        L = len(s)
        if clean:
            q[:] = b"F" * L
        u = rng.random()
        if drop[i]:
            keep = int(rng.integers(0, 20))
            s = (s[:keep] + A13.encode() + bytes(rng.choice(list(b"ACGT"), L).astype(np.uint8)))[:L]
        elif u < 0.3:
            keep = int(rng.integers(25, L))
            s = (s[:keep] + A13.encode() + bytes(rng.choice(list(b"ACGT"), L).astype(np.uint8)))[:L]
        elif u < 0.5:
            t = int(rng.integers(1, L - 30))
            q[L - t:] = bytes([35]) * t                                    # '#': Phred 2
        elif u < 0.55:
            s = s.lower()
        out.append("@t%d%s\n%s\n+\n%s\n" % (i, mate, s.decode(), bytes(q).decode()))
    return "".join(out).encode()


def _drops(n, rng, kind):
    d = np.zeros(n, dtype=bool)
    if kind == "mixed":
        d[rng.random(n) < 0.1] = True
        d[0] = d[n - 1] = True
    elif kind == "all":
        d[:] = True
    return d


def _batches():
    """raw FASTQ texts and what the spec makes of them, by (pairs?, kind of drops); the first and the last record of a `mixed` batch are
    dropped, a pair loses each mate in turn, `all` loses everything, `none` nothing.  No GPU."""
    rng = np.random.default_rng(21)
    se = _fastq_records(os.path.join(GOLD, "se_b150.fq.gz"))
    p1 = _fastq_records(os.path.join(GOLD, "pe_p100_1.fq.gz")); p2 = _fastq_records(os.path.join(GOLD, "pe_p100_2.fq.gz"))
    out = {}
    for kind, n in (("mixed", 1500), ("all", 700), ("none", 400)):
        raw = _raw_records(se[:n], rng, _drops(n, rng, kind), clean=kind == "none")
        out[False, kind] = (raw, None, n) + ts.trim_fastq(raw, None, DEFAULTS)
        n = min(n, len(p1))
        d1 = _drops(n, rng, kind); d2 = _drops(n, rng, kind)
        if kind == "mixed":
            d1[1] = True; d2[1] = False; d1[2] = False; d2[2] = True
        r1, r2 = _raw_records(p1[:n], rng, d1, "/1", kind == "none"), _raw_records(p2[:n], rng, d2, "/2", kind == "none")
        out[True, kind] = (r1, r2, n) + ts.trim_fastq(r1, r2, DEFAULTS)
    for (pe, kind), b in out.items():
        assert b[5] == {"mixed": b[5], "all": 0, "none": b[2]}[kind]
        if kind == "mixed":
            assert 0.5 * b[2] < b[5] < 0.95 * b[2] and b[6]["quality_records"][0] > 100 and b[6]["adapter_records"][0] > 100
        if kind == "none":
            assert b[6]["adapter_bases"][0] > 1000                                   # nothing dropped, much trimmed
    return out


@pytest.fixture(scope="module")
def batches():
    return _batches()


@pytest.fixture(scope="module")
def mappers(gold):
    from bitmapperbs_amd import mapper
    ms = {False: mapper.Mapper(gold["index"], 0), True: mapper.Mapper(gold["index"], 0, max_ins=520)}
    yield ms
    for m in ms.values():
        m.close()


def _payload(out, flags, M):
    if flags & M.TEXT_BAM and not flags & M.TEXT_BAM_SORTED:
        return b"".join(raw for _, raw in bgzf_blocks(out))
    return out


def _counts(m):
    c, kept = m.trim_counts()
    return {k: list(v) if isinstance(v, tuple) else v for k, v in c.items()}, kept


FLAGS = {"sam": 0, "unmapped": 2, "bam": 16, "sorted": 16 | 32, "sorted_unmapped": 2 | 16 | 32}


@pytest.mark.parametrize("kind", ["mixed", "all", "none"])
@pytest.mark.parametrize("out", sorted(FLAGS))
@pytest.mark.parametrize("pe", [False, True])
def test_trimmed_call_equals_the_call_on_the_trimmed_text(batches, mappers, pe, out, kind):
    m = mappers[pe]
    M = type(m)
    flags = FLAGS[out]
    raw1, raw2, n, t1, t2, kept, cnt = batches[pe, kind]
    m.set_trim(off=True); m.reset_stats()
    want = _payload(m.map_text(t1, kept, t2, flags=flags), flags, M)
    st = m.stats().copy()
    extra_want = (m.sorted_index(), m.sorted_dup(), m.sorted_clip()) if flags & M.TEXT_BAM_SORTED else None
    m.set_trim(); m.reset_stats()
    got = _payload(m.map_text(raw1, n, raw2, flags=flags), flags, M)
    assert got == want
    assert (m.stats() == st).all()
    assert _counts(m) == (cnt, kept)
    if kind != "all":
        assert len(want) > 10_000
    if extra_want is not None:
        (key, ln), (sig, tmpl), clip = m.sorted_index(), m.sorted_dup(), m.sorted_clip()
        assert key.tolist() == extra_want[0][0].tolist() and ln.tolist() == extra_want[0][1].tolist()
        assert len(sig) == kept and sig.tobytes() == extra_want[1][0].tobytes() and tmpl.tolist() == extra_want[1][1].tolist()
        assert clip.tolist() == extra_want[2].tolist()
    m.set_trim(off=True)


@pytest.mark.parametrize("pe", [False, True])
def test_clips_behind_a_short_quality_line(batches, mappers, pe):
    """a 5' clip longer than a record's quality line moves its quality offset behind that line's end, the LAST record's behind the text:
    rows, SAM and BAM lines are made from such records (what the text buffers' extra padding under trimming is for)"""
    m = mappers[pe]
    rng = np.random.default_rng(31)
    o = DEFAULTS._replace(quality=0, clip_5p=(25, 40), clip_3p=(3, 0), min_length=20)

    def cut(text):
        recs = ts.records_of(text)[:400]
        for i, r in enumerate(recs):
            if i % 3 == 0 or i == len(recs) - 1:
                r[3] = r[3][:int(rng.integers(0, 50))]                       # shorter than the clip, as often as not
        return b"".join(l + b"\n" for r in recs for l in r)
    src = batches[pe, "none"]
    raw1, raw2 = cut(src[0]), cut(src[1]) if pe else None
    t1, t2, kept, cnt = ts.trim_fastq(raw1, raw2, o)
    assert kept > 300 and cnt["clip_records"][0] == 400
    for flags in (m.TEXT_UNMAPPED, m.TEXT_UNMAPPED | m.TEXT_BAM):
        m.set_trim(off=True)
        want = _payload(m.map_text(t1, kept, t2, flags=flags), flags, type(m))
        _set(m, o)
        assert _payload(m.map_text(raw1, 400, raw2, flags=flags), flags, type(m)) == want and len(want) > 10_000
        assert _counts(m) == (cnt, kept)
    m.set_trim(off=True)


def test_pbat(batches, mappers):
    m = mappers[False]
    raw1, _, n, t1, _, kept, cnt = batches[False, "mixed"]
    m.set_trim(off=True)
    want = m.map_text(t1, kept, None, flags=m.TEXT_PBAT | m.TEXT_UNMAPPED)
    m.set_trim()
    assert m.map_text(raw1, n, None, flags=m.TEXT_PBAT | m.TEXT_UNMAPPED) == want and len(want) > 10_000
    m.set_trim(off=True)


def test_trimming_off_counts_nothing(batches, mappers):
    m = mappers[False]
    raw1, _, n = batches[False, "none"][:3]
    m.set_trim()
    m.map_text(raw1, n)
    assert m.trim_counts()[1] == n
    m.set_trim(off=True)
    m.map_text(raw1, n)
    with pytest.raises(RuntimeError, match="bmbs error -1: "):
        m.trim_counts()
    # a call without records is the last text call too: nothing stale is reported for it
    m.set_trim()
    m.map_text(raw1, n)
    assert m.trim_counts()[1] == n
    assert m.map_text(b"", 0) == b""
    with pytest.raises(RuntimeError, match="bmbs error -1: "):
        m.trim_counts()
    m.set_trim(off=True)


@pytest.mark.parametrize("pe", [False, True])
def test_retry_after_no_room(batches, mappers, pe):
    """a buffer that is too small: the library's no-room error; the call repeated with room gives the same bytes and the same counts, and
    the statistics count the batch once"""
    m = mappers[pe]
    raw1, raw2, n, t1, t2, kept, cnt = batches[pe, "mixed"]
    m.set_trim(); m.reset_stats()
    want = m.map_text(raw1, n, raw2)
    st = m.stats().copy()
    m.reset_stats()
    with pytest.raises(RuntimeError, match="bmbs error -12"):
        m.map_text(raw1, n, raw2, cap=4096)
    assert m.map_text(raw1, n, raw2, cap=len(want)) == want
    assert (m.stats() == st).all() and st[0] == kept                                 # (the statistics count templates)
    assert _counts(m) == (cnt, kept)
    m.set_trim(off=True)


@pytest.mark.parametrize("pe", [False, True])
def test_open_bgzf_then_map(batches, mappers, tmp_path, pe):
    """the same through compressed input that stays on the device, with a retry in between"""
    m = mappers[pe]
    raw1, raw2, n, t1, t2, kept, cnt = batches[pe, "mixed"]
    m.set_trim(off=True)
    want = m.map_text(t1, kept, t2, flags=m.TEXT_UNMAPPED)
    z = []
    for f, raw in enumerate((raw1, raw2) if pe else (raw1,)):
        write_bgzf(str(tmp_path / ("%d.gz" % f)), raw)
        z.append(open(tmp_path / ("%d.gz" % f), "rb").read()[:-28])           # (without the empty end-of-file block)
    m.set_trim()
    got_n, tail1, tail2 = m.text_open_bgzf((b"", z[0]), (b"", z[1]) if pe else None, last=(True, True))
    assert (got_n, tail1, tail2) == (n, b"", b"")
    with pytest.raises(RuntimeError, match="bmbs error -12"):
        m.text_map_open(flags=m.TEXT_UNMAPPED, cap=4096)
    assert m.text_map_open(flags=m.TEXT_UNMAPPED) == want
    assert _counts(m) == (cnt, kept)
    m.set_trim(off=True)


# ---- the driver -------------------------------------------------------------------------------------------------------------------------
def _run(index, inputs, args, out):
    p = subprocess.run([_driver(), "--search", index] + inputs + ["-o", out] + args, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return p.stderr


def _body(path):
    return b"".join(l for l in open(path, "rb").read().splitlines(True) if not l.startswith(b"@"))


@pytest.fixture(scope="module")
def driver_files(batches, tmp_path_factory):
    """raw and spec-trimmed FASTQ files: 300 templates of the mixed batch, 700 that are all dropped, 300 of which none is: with --batch 300
    the second and the third batch keep nothing"""
    wd = tmp_path_factory.mktemp("trim_driver")
    files = {}
    for pe in (False, True):
        parts = [batches[pe, "mixed"], batches[pe, "all"], batches[pe, "none"]]

        def cut(text, n):
            return b"".join(text.splitlines(True)[:4 * n]) if text is not None else None
        raw = [[cut(b[0], k) for b, k in zip(parts, (300, 700, 300))], [cut(b[1], k) for b, k in zip(parts, (300, 700, 300))]]
        r1 = b"".join(raw[0]); r2 = b"".join(raw[1]) if pe else None
        n = r1.count(b"\n") // 4
        t1, t2, kept, cnt = ts.trim_fastq(r1, r2, DEFAULTS)
        names = {}
        for tag, a, b in (("raw", r1, r2), ("trimmed", t1, t2)):
            open(wd / ("%s_%d_1.fq" % (tag, pe)), "wb").write(a)
            if pe:
                open(wd / ("%s_%d_2.fq" % (tag, pe)), "wb").write(b)
            names[tag] = (["--seq1", str(wd / ("%s_%d_1.fq" % (tag, pe))), "--seq2", str(wd / ("%s_%d_2.fq" % (tag, pe)))] if pe
                          else ["--seq", str(wd / ("%s_%d_1.fq" % (tag, pe)))])
        files[pe] = dict(names, n=n, kept=kept, cnt=cnt, wd=wd)
    return files


def _args(pe):
    return json.load(open(os.path.join(GOLD, "pe_args.json")))["p100"] if pe else golden_args()["b150"]


@pytest.mark.parametrize("pe", [False, True])
def test_driver_sam_and_reports(gold, driver_files, tmp_path, pe):
    F = driver_files[pe]
    args = _args(pe) + ["--batch", "300", "--unmapped_out"]
    _run(gold["fa"], F["trimmed"], args + ["--mapstats", str(tmp_path / "want.stats")], str(tmp_path / "want.sam"))
    err = _run(gold["fa"], F["raw"], args + ["--trim", "--mapstats", str(tmp_path / "got.stats"), "--trim-report", str(tmp_path / "trim.tsv")], str(tmp_path / "got.sam"))
    assert _body(tmp_path / "got.sam") == _body(tmp_path / "want.sam") and len(_body(tmp_path / "want.sam")) > 100_000
    hdr = [l for l in open(tmp_path / "got.sam") if l.startswith("@PG")]
    assert len(hdr) == 1 and "--trim" not in hdr[0]
    got, want = open(tmp_path / "got.stats").read().splitlines(), open(tmp_path / "want.stats").read().splitlines()
    removed = "%-48s%d" % ("No. of Reads Removed by Trimming:", (F["n"] - F["kept"]) * (2 if pe else 1))
    assert got == want + [removed] and removed in err
    rep = [l.split("\t") for l in open(tmp_path / "trim.tsv").read().splitlines()]
    cnt = F["cnt"]
    want_rep = [[k, str(m + 1), str(cnt[k][m])] for k in ts.COUNTERS for m in range(2 if pe else 1)]
    want_rep += [["templates_in", "0", str(F["n"])], ["templates_kept", "0", str(F["kept"])], ["templates_dropped", "0", str(F["n"] - F["kept"])]]
    assert rep == want_rep


@pytest.mark.parametrize("pe", [False, True])
def test_driver_sorted_bam_with_everything(gold, driver_files, tmp_path, pe):
    """BAM records, .bai and bedGraphs.  The .bai holds virtual offsets, which begin behind the header block, and the header's @PG line
    holds the command line: the two runs get the same one (--trim stays out of it) -- each in a directory of its own, with the same
    relative file names"""
    import shutil
    F = driver_files[pe]
    args = _args(pe) + ["--batch", "300", "--bam", "--sort", "--markdup", "--bai", "--methyl", "m", "--CpG", "--CHG"]
    outs = {}
    for tag, extra in (("want", []), ("got", ["--trim"])):
        wd = tmp_path / tag
        wd.mkdir()
        src = F["trimmed" if tag == "want" else "raw"]
        inputs = []
        for k in range(0, len(src), 2):
            shutil.copy(src[k + 1], wd / ("r_%d.fq" % (k // 2 + 1)))
            inputs += [src[k], "r_%d.fq" % (k // 2 + 1)]
        p = subprocess.run([_driver(), "--search", gold["fa"]] + inputs + ["-o", "o.bam"] + args + extra, capture_output=True, text=True, cwd=str(wd))
        assert p.returncode == 0, p.stderr
        outs[tag] = (bam_payload(str(wd / "o.bam")), open(wd / "o.bam.bai", "rb").read(), [open(wd / ("m_%s.bedGraph" % c), "rb").read() for c in ("CpG", "CHG")])
    assert outs["got"][0] == outs["want"][0] and len(split_records(outs["want"][0][1])) > 200
    assert outs["got"][1] == outs["want"][1]
    assert outs["got"][2] == outs["want"][2] and len(outs["want"][2][0]) > 1000


def test_driver_refusals(gold, driver_files, tmp_path):
    """every refusal is the new options' own: exit status 2 AND their message (an unknown option would give the status alone)"""
    F = driver_files[False]
    base = [_driver(), "--search", gold["fa"]] + F["raw"] + ["-o", str(tmp_path / "x.sam")]
    need, letters = "need --trim", "takes letters of ACGT"
    for bad, msg in ((["--trim-quality", "20"], need), (["--trim-adapter", "ACGT"], need), (["--trim-report", str(tmp_path / "r")], need), (["--trim-clip-r1", "2"], need),
                     (["--trim-adapter2", "ACGT"], need), (["--trim-stringency", "3"], need), (["--trim-error-rate", "0.1"], need), (["--trim-min-length", "30"], need),
                     (["--trim", "--trim-adapter", "ACGU"], "--trim-adapter " + letters), (["--trim", "--trim-adapter2", "ACNT"], "--trim-adapter2 " + letters),
                     (["--trim", "--trim-adapter2", "A" * 33], "--trim-adapter2 takes at most 32 letters"), (["--trim", "--trim-min-length", "0"], "--trim-min-length takes 1..65535"),
                     (["--trim", "--trim-error-rate", "1.5"], "--trim-error-rate takes a plain decimal in 0..1"), (["--trim", "--trim-error-rate", "0.1234"], "at most 3 digits"),
                     (["--trim", "--trim-quality", "-1"], "--trim-quality takes 0..255"), (["--trim", "--trim-quality", "256"], "--trim-quality takes 0..255"),
                     (["--trim", "--trim-stringency", "0"], "--trim-stringency takes 1..65535"), (["--trim", "--trim-three-prime-clip-r2", "x"], "--trim-three-prime-clip-r2 takes 0..65535"),
                     (["--trim", "--trim-clip-r2", "65536"], "--trim-clip-r2 takes 0..65535")):
        p = subprocess.run(base + bad, capture_output=True, text=True)
        assert p.returncode == 2 and msg in p.stderr and "unsupported option" not in p.stderr, (bad, p.stderr)
    assert not os.path.exists(tmp_path / "x.sam") or os.path.getsize(tmp_path / "x.sam") == 0


def test_driver_refinements(gold, driver_files, tmp_path):
    """the options reach the device: another adapter for mate 2, clips, a cutoff, a stringency, an error rate and a length"""
    F = driver_files[True]
    o = Opts(25, (A13, A32), 3, 200, 30, (2, 1), (1, 3), 33)
    r1, r2 = open(F["raw"][1], "rb").read(), open(F["raw"][3], "rb").read()
    t1, t2, kept, cnt = ts.trim_fastq(r1, r2, o)
    open(tmp_path / "1.fq", "wb").write(t1); open(tmp_path / "2.fq", "wb").write(t2)
    args = _args(True) + ["--unmapped_out"]
    _run(gold["fa"], ["--seq1", str(tmp_path / "1.fq"), "--seq2", str(tmp_path / "2.fq")], args, str(tmp_path / "want.sam"))
    _run(gold["fa"], F["raw"], args + ["--trim", "--trim-quality", "25", "--trim-adapter", A13, "--trim-adapter2", A32, "--trim-stringency", "3", "--trim-error-rate", "0.2",
                                       "--trim-min-length", "30", "--trim-clip-r1", "2", "--trim-clip-r2", "1", "--trim-three-prime-clip-r1", "1",
                                       "--trim-three-prime-clip-r2", "3"], str(tmp_path / "got.sam"))
    assert _body(tmp_path / "got.sam") == _body(tmp_path / "want.sam") and len(_body(tmp_path / "want.sam")) > 100_000
