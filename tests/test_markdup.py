"""Duplicate marking on the device (`bmbs_search --bam --sort --markdup`, bmbs_bam_dup_sigs, bmbs_text_sorted_dup, bmbs_dup_select) against
tests/markdup_spec.py.  Signatures and marks are integers and bytes: every comparison here is exact."""
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bai_spec
import markdup_spec as spec
from common import GOLD, ROOT, bam_payload, bgzf_blocks, golden_args, gunzip_to
from test_sorted_bam import _bam_header_text, split_records, stable_sorted

pytestmark = pytest.mark.gpu


def _sig_array(sigs):
    from bitmapperbs_amd import capi
    a = np.zeros(len(sigs), dtype=capi.DUP_SIG_DTYPE)
    for i, s in enumerate(sigs):
        a[i] = s
    return a


def _sig_tuples(a):
    return [tuple(int(x) for x in r) for r in a.tolist()]


# ---- bmbs_bam_dup_sigs ------------------------------------------------------------------------------------------------------------------
L_SEQS = (0, 1, 15, 16, 17, 151, 998)
COUNTS = (1, 63, 64, 65, 257, 20_000)


def _random_records(n, seed=21):
    """names of 1..40 characters (records start at every alignment mod 16), l_seq of L_SEQS, every CIGAR operation anywhere (0..6
    operations, now and then 40), both strands and reads, some unmapped / secondary / supplementary records, qualities 0..60 with 14,
    15 and 0xff among them; every ninth entry is a hole, and so is every 23rd pair of entries as a whole"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i % 9 == 4 or (i // 2) % 23 == 7:
            out.append(b"")
            continue
        l_seq = L_SEQS[int(rng.integers(0, len(L_SEQS)))]
        n_ops = 40 if rng.random() < 0.02 else int(rng.integers(0, 7))
        cigar = [(int(rng.integers(0, 9)), int(rng.integers(1, 300))) for _ in range(n_ops)]
        flag = int(rng.choice([0, 16])) | int(rng.choice([0, 0x40, 0x80])) | 1
        r = rng.random()
        flag |= 4 if r < 0.05 else 0x100 if r < 0.08 else 0x800 if r < 0.11 else 0
        q = rng.integers(0, 61, l_seq).astype(np.uint8)
        q[rng.random(l_seq) < 0.05] = 0xff
        q[rng.random(l_seq) < 0.1] = 14
        q[rng.random(l_seq) < 0.1] = 15
        name = bytes(rng.integers(97, 123, int(rng.integers(1, 41))).astype(np.uint8))
        out.append(spec.make_record(int(rng.integers(0, 4)), int(rng.integers(0, 5000)), flag, cigar, q.tobytes(), name))
    return out


@pytest.fixture(scope="module")
def sig_case():
    """the records and what the spec says of them, computed once: single end over the first 20 000 entries, paired over all 40 000"""
    recs = _random_records(2 * COUNTS[-1])
    starts = np.cumsum([0] + [len(r) for r in recs[:-1]])
    assert len({int(s) % 16 for s, r in zip(starts, recs) if r}) == 16
    return dict(recs=recs, se=spec.signatures(recs[:COUNTS[-1]], False), pe=spec.signatures(recs, True))


@pytest.fixture(scope="module")
def bare():
    """a context without an index"""
    from bitmapperbs_amd import mapper
    m = mapper.Mapper(None, 0)
    yield m
    m.close()


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("count", COUNTS)
def test_dup_sigs_equal_the_spec(sig_case, bare, count, paired):
    n = 2 * count if paired else count
    recs = sig_case["recs"][:n]
    want = sig_case["pe" if paired else "se"][:count]
    got = bare.dup_sigs(b"".join(recs), [len(r) for r in recs], paired)
    assert got.size == count
    assert _sig_tuples(got) == [tuple(s) for s in want]
    if count == COUNTS[-1]:
        none = sum(1 for s in want if s[4] & spec.DUP_NONE)
        assert 0 < none < count // 2 and any(s[4] & 8 for s in want) == paired


def test_dup_sigs_refusals_are_those_of_bam_sort(sig_case, bare):
    recs = [r for r in sig_case["recs"][:400] if r][:100]
    lens = np.array([len(r) for r in recs], dtype=np.uint32)
    stream = b"".join(recs)
    assert bare.dup_sigs(stream, lens).size == 100
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 41\b.*36"):
        bad = lens.copy(); bad[42] += bad[41] - 20; bad[41] = 20
        bare.dup_sigs(stream, bad)
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 12\b"):
        bad = lens.copy(); bad[12] += 4; bad[13] -= 4                       # not block_size + 4 (the sum still matches)
        bare.dup_sigs(stream, bad)
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*add up"):
        bare.dup_sigs(stream[:-1], lens)
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*odd"):
        bare.dup_sigs(b"".join(recs[:99]), lens[:99], True)
    # a record whose fields reach behind its length: named, nothing is read behind it
    r = bytearray(recs[5]); struct.pack_into("<I", r, 20, len(r))            # l_seq = the whole record's size
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 5\b.*do not fit"):
        bare.dup_sigs(b"".join(recs[:5]) + bytes(r) + b"".join(recs[6:]), lens)
    assert bare.dup_sigs(b"", np.zeros(0, dtype=np.uint32)).size == 0
    assert bare.dup_sigs(b"", np.zeros(6, dtype=np.uint32), True)["orient"].tolist() == [spec.DUP_NONE] * 3


# ---- bmbs_dup_select ----------------------------------------------------------------------------------------------------------------------
def _check_select(m, sigs):
    dup, nd = m.dup_select(_sig_array(sigs))
    want = spec.select(sigs)
    assert dup.tolist() == want
    assert nd == sum(want)
    return want


def test_dup_select_small_and_degenerate_inputs(bare):
    assert bare.dup_select(_sig_array([]))[1] == 0
    assert _check_select(bare, [(0, 5, -1, -1, 0, 100)]) == [0]
    assert _check_select(bare, [spec.NO_SIG]) == [0]
    # all equal, n = 300 (the group spans a workgroup boundary): one survivor, the best score, earliest among equals
    rng = np.random.default_rng(3)
    sc = rng.integers(100, 104, 300).tolist()
    want = _check_select(bare, [(1, 777, 2, 888, 9, s) for s in sc])
    assert sum(want) == 299 and want.index(0) == sc.index(103) and sc.count(103) > 1
    # all distinct; all without a signature (whatever their other fields hold)
    assert sum(_check_select(bare, [(0, i, -1, -1, i & 1, 50) for i in range(1000)])) == 0
    assert sum(_check_select(bare, [(0, 5, 0, 9, spec.DUP_NONE | 8, 50 + i % 3) for i in range(500)])) == 0
    # negative coordinates and the largest score
    _check_select(bare, [(0, -7, 0, -3, 8, 0xffffffff), (0, -7, 0, -3, 8, 0xffffffff), (0, -7, 0, -3, 8, 5), (0, -7, 1, -3, 8, 0), (-1, -7, 0, -3, 8, 0)])


def test_dup_select_of_random_signatures_whole_and_in_three_parts(bare):
    """100 000 signatures over 2 000 sites (half of them over the first 100: groups of hundreds) and 8 scores, some without a signature
    at the coordinates of real ones; the same set split by a function of pos_lo into three calls gives the same marks"""
    rng = np.random.default_rng(17)
    sites = [(int(rng.integers(0, 3)), int(rng.integers(-5, 3000)), int(rng.integers(-1, 3)), int(rng.integers(-1, 3000)), int(rng.integers(0, 16)))
             for _ in range(2000)]
    n = 100_000
    pick = np.where(rng.random(n) < 0.5, rng.integers(0, 100, n), rng.integers(0, 2000, n))
    score = rng.integers(0, 8, n) * 37
    none = rng.random(n) < 0.03
    sigs = [sites[p][:4] + (sites[p][4] | (spec.DUP_NONE if z else 0), int(s)) for p, s, z in zip(pick.tolist(), score.tolist(), none.tolist())]
    want = _check_select(bare, sigs)
    # the test saw what it is about: groups larger than a wave, and ties for the best score inside groups
    groups = {}
    for i, s in enumerate(sigs):
        if not s[4] & spec.DUP_NONE:
            groups.setdefault(s[:5], []).append(s[5])
    assert max(len(g) for g in groups.values()) > 64
    assert any(g.count(max(g)) > 1 for g in groups.values())
    assert 0 < sum(want) < n and not any(w for w, z in zip(want, none.tolist()) if z)
    got = [None] * n
    for part in range(3):
        idx = [i for i, s in enumerate(sigs) if s[1] % 3 == part]
        dup, _ = bare.dup_select(_sig_array([sigs[i] for i in idx]))
        for i, d in zip(idx, dup.tolist()):
            got[i] = d
    assert got == want


# ---- bmbs_text_sorted_dup -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    """the golden genome's index, built once"""
    from bitmapperbs_amd import mapper
    wd = tmp_path_factory.mktemp("markdup_gold")
    fa = str(wd / "genome.fa")
    gunzip_to(os.path.join(GOLD, "genome.fa.gz"), fa)
    mapper.Index.build(fa, fa, threads=4)
    return fa


def _fastq_records(path):
    lines = gzip.open(path, "rt").read().split("\n")
    return [lines[i:i + 4] for i in range(0, len(lines) - 3, 4)]


def _with_copies(recs, tag, mate=""):
    """every fifth read three times under new names: as it is, with lowered qualities, with 7 bases trimmed from its 3' end; names are
    `<tag><serial>` (+ /1, /2), the serial counts output records"""
    out = []
    def put(seq, qual):
        out.append("@%s%d%s\n%s\n+\n%s" % (tag, len(out), mate, seq, qual))
    for i, r in enumerate(recs):
        put(r[1], r[3])
        if i % 5 == 0:
            put(r[1], "".join(chr(max(35, ord(c) - 4)) for c in r[3]))
            put(r[1][:-7], r[3][:-7])
    return "\n".join(out) + "\n", len(out)


def _name(rec):
    return rec[36:36 + rec[12] - 1]


def _by_template(records, n_tmpl, paired, tag):
    """the records of a run's unsorted output, in order -> 1 or 2 entries per template, b"" where a template's line printed nothing"""
    out = []
    at = 0
    for t in range(n_tmpl):
        nm = b"%s%d" % (tag.encode(), t)
        for _ in range(2 if paired else 1):
            if at < len(records) and _name(records[at]) == nm:
                out.append(records[at]); at += 1
            else:
                out.append(b"")
    assert at == len(records)
    return out


@pytest.mark.parametrize("kind", ["pe_p100", "se_b150"])
def test_sorted_dup_of_a_text_call_equals_dup_sigs_of_its_unsorted_records(gold, kind):
    from bitmapperbs_amd import mapper
    M = mapper.Mapper
    paired = kind.startswith("pe")
    if paired:
        t1, n = _with_copies(_fastq_records(os.path.join(GOLD, "pe_p100_1.fq.gz")), "t", "/1")
        t2, _ = _with_copies(_fastq_records(os.path.join(GOLD, "pe_p100_2.fq.gz")), "t", "/2")
        t1, t2 = t1.encode(), t2.encode()
        kw = dict(e_f=0.04, max_ins=520)
    else:
        t1, n = _with_copies(_fastq_records(os.path.join(GOLD, "se_b150.fq.gz")), "t")
        t1, t2 = t1.encode(), None
        kw = dict(e_f=0.04)
    m = M(mapper.Index(gold), 0, **kw)
    with pytest.raises(RuntimeError, match="bmbs error -1:"):
        m.sorted_dup()                                                       # no sorted call yet
    unsorted = split_records(b"".join(raw for _, raw in bgzf_blocks(m.map_text(t1, n, t2, flags=M.TEXT_BAM))))
    entries = _by_template(unsorted, n, paired, "t")
    assert entries.count(b"") > 0                                            # some lines printed nothing
    got = split_records(m.map_text(t1, n, t2, flags=M.TEXT_BAM | M.TEXT_BAM_SORTED))
    sig, tmpl = m.sorted_dup()
    sig2, tmpl2 = m.sorted_dup()                                             # (kept behind the size query: the same again)
    assert sig.tobytes() == sig2.tobytes() and tmpl.tobytes() == tmpl2.tobytes()
    bare = M(None, 0)
    want = bare.dup_sigs(b"".join(entries), [len(e) for e in entries], paired)
    bare.close()
    assert sig.size == n and sig.tobytes() == want.tobytes()
    assert _sig_tuples(sig) == [tuple(s) for s in spec.signatures(entries, paired)]
    assert tmpl.size == len(got) and [_name(r) for r in got] == [b"t%d" % t for t in tmpl.tolist()]
    dup, nd = m.dup_select(sig)
    assert nd > n // 10 and dup.tolist() == spec.select(_sig_tuples(sig))
    # another call has rewritten the buffers: BMBS_ESTATE
    m.map_text(t1, n, t2, flags=M.TEXT_BAM | M.TEXT_BAM_SORTED)
    m.bam_sort(b"".join(unsorted[:10]), [len(r) for r in unsorted[:10]], raw=True)
    with pytest.raises(RuntimeError, match="bmbs error -1:"):
        m.sorted_dup()
    m.map_text(t1, n, t2, flags=M.TEXT_BAM | M.TEXT_BAM_SORTED)
    assert m.sorted_dup()[0].tobytes() == sig.tobytes()
    m.map_text(t1, n, t2, flags=M.TEXT_BAM)
    with pytest.raises(RuntimeError, match="bmbs error -1:"):
        m.sorted_dup()
    m.close()


# ---- the driver -------------------------------------------------------------------------------------------------------------------------------
def _driver():
    p = os.path.join(ROOT, "bitmapperbs_amd", "bmbs_search")
    assert os.path.exists(p), "bmbs_search not built (make -C bitmapperbs_amd/csrc)"
    return p


def _run(gold, inputs, args, out, env=None):
    cmd = [_driver(), "--search", gold] + inputs + ["-o", out, "--verbose", "--bam"] + args
    p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stderr
    return p.stderr


@pytest.fixture(scope="module")
def runs(gold, tmp_path_factory):
    """per kind: the FASTQ with copies, the plain --bam run, the --sort run, what the spec makes of the plain run -- made once"""
    pe_args = __import__("json").load(open(os.path.join(GOLD, "pe_args.json")))
    made = {}

    def get(kind):
        if kind in made:
            return made[kind]
        wd = tmp_path_factory.mktemp("markdup_" + kind)
        paired = kind == "pe"
        if paired:
            t1, n = _with_copies(_fastq_records(os.path.join(GOLD, "pe_p100_1.fq.gz")), "d", "/1")
            t2, _ = _with_copies(_fastq_records(os.path.join(GOLD, "pe_p100_2.fq.gz")), "d", "/2")
            open(wd / "1.fq", "w").write(t1); open(wd / "2.fq", "w").write(t2)
            inputs, args = ["--seq1", str(wd / "1.fq"), "--seq2", str(wd / "2.fq")], pe_args["p100"]
        else:
            t1, n = _with_copies(_fastq_records(os.path.join(GOLD, "se_b150.fq.gz")), "d")
            open(wd / "r.fq", "w").write(t1)
            inputs, args = ["--seq", str(wd / "r.fq")], golden_args()["b150"]
        _run(gold, inputs, args, str(wd / "plain.bam"))
        _run(gold, inputs, args + ["--sort"], str(wd / "sorted.bam"))
        entries = _by_template(split_records(bam_payload(str(wd / "plain.bam"))[1]), n, paired, "d")
        marked = spec.mark(entries, paired)
        made[kind] = dict(wd=wd, inputs=inputs, args=args, n=n, paired=paired, entries=entries, marked=marked,
                          want=stable_sorted(b"".join(marked)), sorted=bam_payload(str(wd / "sorted.bam")))
        return made[kind]
    return get


def _markdup_counts(err):
    m = re.search(r"markdup: templates (\d+), with signature (\d+), duplicates (\d+) \(select calls (\d+)", err)
    assert m, err
    return tuple(int(x) for x in m.groups())


@pytest.mark.parametrize("kind", ["se", "pe"])
def test_driver_marks_what_the_spec_marks(gold, runs, kind):
    """the payload of --bam --sort --markdup = the plain --bam output of the same build, marked by the spec, stably sorted -- byte for
    byte; with 0x400 cleared it is the --sort output; the header is --sort's"""
    R = runs(kind)
    out = str(R["wd"] / "md.bam")
    err = _run(gold, R["inputs"], R["args"] + ["--sort", "--markdup"], out)
    ref_dict, got = bam_payload(out)
    assert (ref_dict, got) == (R["sorted"][0], R["want"])
    recs = split_records(got)
    flags = [struct.unpack_from("<H", r, 18)[0] for r in recs]
    assert any(f & 0x400 for f in flags)
    assert b"".join(r[:19] + bytes([r[19] & ~0x04]) + r[20:] for r in recs) == R["sorted"][1]
    hdr = lambda p: [l for l in _bam_header_text(p).split("\n") if not l.startswith("@PG")]
    assert hdr(out) == hdr(str(R["wd"] / "sorted.bam")) and hdr(out)[0] == "@HD\tVN:1.4\tSO:coordinate"
    # the counts of the --verbose line
    sigs = spec.signatures(R["entries"], R["paired"])
    dup = spec.select(sigs)
    assert _markdup_counts(err)[:3] == (R["n"], sum(1 for s in sigs if not s[4] & spec.DUP_NONE), sum(dup))
    # a marked reverse-strand record whose pos is not its kept representative's (its 3' end was trimmed: only the 5' end counts)
    per = 2 if R["paired"] else 1
    keeper = {s[:5]: t for t, s in enumerate(sigs) if not dup[t] and not s[4] & spec.DUP_NONE}
    moved = 0
    for t, s in enumerate(sigs):
        if not dup[t]:
            continue
        mine = R["marked"][per * t:per * t + per]; theirs = R["marked"][per * keeper[s[:5]]:per * keeper[s[:5]] + per]
        for a in mine:
            for b in theirs:
                fa, fb = struct.unpack_from("<H", a, 18)[0], struct.unpack_from("<H", b, 18)[0]
                if (fa & 16) and (fa & 0xd0) == (fb & 0xd0) and a[8:12] != b[8:12]:
                    moved += 1
        if R["paired"]:                                                       # the mates of a template always agree
            assert all(struct.unpack_from("<H", a, 18)[0] & 0x400 for a in mine if a)
    assert moved > 0
    if R["paired"]:
        by_name = {}
        for r, f in zip(recs, flags):
            by_name.setdefault(_name(r), set()).add(f & 0x400)
        assert all(len(v) == 1 for v in by_name.values())


@pytest.mark.parametrize("kind", ["se", "pe"])
def test_driver_payload_under_another_store_and_call_geometry(gold, runs, kind):
    """small pass-2 calls and few bins (a call budget of 8 000 bytes = 333 signatures per select group, below the 800 pairs and the
    1 500 reads of the goldens: several select groups), batches so small that copies fall into different batches, two contexts: the
    same payload every time"""
    R = runs(kind)
    cases = [(dict(BMBS_SORT_CALL_BYTES="8000", BMBS_SORT_BINS="7"), []),
             (dict(BMBS_SORT_CALL_BYTES="8000"), ["--batch", "50"]),
             (dict(BMBS_SORT_BINS="1"), ["--batch", "31", "--contexts", "2"])]
    for i, (env, more) in enumerate(cases):
        out = str(R["wd"] / ("geo%d.bam" % i))
        err = _run(gold, R["inputs"], R["args"] + ["--sort", "--markdup"] + more, out, env)
        assert bam_payload(out) == (R["sorted"][0], R["want"]), (env, more)
        if "BMBS_SORT_CALL_BYTES" in env:
            assert _markdup_counts(err)[3] > 1 and int(re.search(r"pass-2 calls (\d+)", err).group(1)) > 1


def test_driver_markdup_with_bai(gold, runs):
    R = runs("pe")
    out = str(R["wd"] / "ix.bam")
    _run(gold, R["inputs"], R["args"] + ["--sort", "--markdup", "--bai"], out, dict(BMBS_SORT_CALL_BYTES="100000"))
    assert bam_payload(out) == (R["sorted"][0], R["want"])
    assert open(out + ".bai", "rb").read() == bai_spec.spec_bai(out)
