"""Read-end trimming and the M-bias table on the device (bmbs_bam_methyl_opts, bmbs_bam_sort_methyl_opts, bmbs_methyl_mbias,
`bmbs_search --methyl ... --methyl-ignore* --mbias`) against tests/mbias_spec.py.  Sites, counters and files: every comparison is exact.

A trim is written (ignore_5p, ignore_3p), each (read 1 or single end, read 2); the tuples of four below are in the order
(ignore_5p[0], ignore_5p[1], ignore_3p[0], ignore_3p[1])."""
import bisect
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import bai_spec
import markdup_spec
import mbias_spec
import methyl_spec as spec
import test_methyl as tm
from common import GOLD, ROOT, bam_payload, golden_args
from test_mbias_spec import golden_seqs, random_records
from test_methyl import gold, mapper_on_gold, runs  # noqa: F401  (fixtures)
from test_sorted_bam import split_records

gpu = pytest.mark.gpu

MIN_MAPQ, MIN_PHRED = tm.MIN_MAPQ, tm.MIN_PHRED
# the 32-base word borders, the border between the block's table and the global one at 256, the clamp at 1024
L_SEQS = (1, 2, 31, 32, 33, 63, 64, 65, 151, 255, 256, 257, 998, 1023, 1024, 1025, 1100)
COUNTS = (1, 63, 64, 65, 257, 20_000)
TRIMS = ((0, 0, 0, 0), (5, 0, 0, 0), (0, 3, 0, 0), (2, 1, 7, 4), (40, 40, 0, 0), (65535, 0, 0, 65535))


def _trim(t):
    return (t[0], t[1]), (t[2], t[3])


def _site_tuples(a):
    return [(int(r["ref"]), int(r["pos"]), int(r["meth"]), int(r["unmeth"]), int(r["kind"])) for r in a]


def _table(walked, contexts=7):
    return np.array(mbias_spec.table_of(walked, contexts), dtype=np.uint64)


def _upto(walked, count):
    """the calls of records 0 .. count - 1 (the list is in record order)"""
    return walked[:bisect.bisect_left(walked, (count,))]


# ---- 1. crafted records -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crafted():
    """20 000 random records (every 11th entry a hole) with their clips and 20 000 stacked on 200 bases, and every call the spec finds in
    them, every context -- walked once; sites and tables of any count, trim and selection are sums over that list.  No GPU."""
    rng = np.random.default_rng(23)
    seqs = golden_seqs()
    recs = [b"" if i % 11 == 6 else r for i, r in enumerate(random_records(rng, seqs, COUNTS[-1], L_SEQS))]
    clip = [tm._random_clip(rng, r) if r else 0 for r in recs]
    stack = random_records(rng, seqs, COUNTS[-1], L_SEQS, stack=True)
    return dict(seqs=seqs, recs=recs, clip=clip, stack=stack, walked=mbias_spec.walk(seqs, recs, clip, MIN_MAPQ, MIN_PHRED),
                stack_walked=mbias_spec.walk(seqs, stack, None, MIN_MAPQ, MIN_PHRED))


def test_the_crafted_records_are_not_trivial(crafted):
    """on the spec alone (no GPU)"""
    walked, recs = crafted["walked"], crafted["recs"]
    t = _table(walked)
    assert t.shape == mbias_spec.SHAPE
    # every one of the 24 rows has calls in more than 100 cycles; both tables of the kernel and the clamped bin are hit
    assert ((t > 0).sum(axis=-1) > 100).all()
    assert t[..., :256].any() and t[..., 256:1023].any() and t[..., 1023].any()
    assert any(c[8] > 1023 for c in walked) and any(c[8] == 1023 for c in walked)
    # each non-zero trim removes calls, and keeps some -- but the last, which ignores every cycle of either mate: it keeps none
    n_all = len(walked)
    for trim in TRIMS[1:]:
        i5, i3 = _trim(trim)
        kept = sum(1 for c in walked if mbias_spec.keeps(c[8], c[2], c[1], i5, i3))
        assert kept < n_all and (kept > 0) == (trim != TRIMS[-1]), trim
    # (40, 40, 0, 0) ignores whole records that call something
    assert any(c[2] <= 40 for c in walked)
    # both orientations, both mates and single end, every CIGAR operation, S, I and H in front and behind, holes, clips that take calls away
    flags = {spec.fields(r)[3] & 0xd1 for r in recs if r and not spec.skip_reason(r, MIN_MAPQ)}
    assert flags >= {0, 0x10, 0x41, 0x51, 0x81, 0x91}
    cigars = [spec.fields(r)[4] for r in recs if r and not spec.skip_reason(r, MIN_MAPQ)]
    assert {op for c in cigars for op, _ in c} == set(range(9))
    assert {c[0][0] for c in cigars} >= {1, 4, 5} and {c[-1][0] for c in cigars} >= {1, 4, 5}
    assert sum(1 for r in recs if not r) > 1000
    assert len(mbias_spec.walk(crafted["seqs"], recs[:3000], None, MIN_MAPQ, MIN_PHRED)) > len(_upto(walked, 3000))
    # the stack: 32 cycles only, so every counter in use is fed by far more records than the 16 a block holds at a time.  (A record
    # adds at most 1 to any one counter: no counter of 20 000 records can pass 20 000, let alone 65 536.)
    ts = _table(crafted["stack_walked"])
    assert not ts[..., 32:].any() and ts[..., :32].max() > 100 and ts.sum() > 20_000
    assert max(s[2] + s[3] for s in mbias_spec.sites_of(crafted["stack_walked"], 7)) > 2 * 256


@gpu
@pytest.mark.parametrize("trim", TRIMS)
@pytest.mark.parametrize("count", COUNTS)
def test_sites_and_table_equal_the_spec(crafted, mapper_on_gold, count, trim):
    recs, i53 = crafted["recs"][:count], _trim(trim)
    got = mapper_on_gold.bam_methyl(b"".join(recs), [len(r) for r in recs], crafted["clip"][:count], contexts=7, min_mapq=MIN_MAPQ, min_phred=MIN_PHRED,
                                    ignore_5p=i53[0], ignore_3p=i53[1], mbias=True)
    walked = _upto(crafted["walked"], count)
    assert _site_tuples(got) == mbias_spec.sites_of(walked, 7, *i53)
    assert not got["pad"].any()
    t = mapper_on_gold.methyl_mbias()
    assert t.dtype == np.uint64 and t.shape == mbias_spec.SHAPE
    assert (t == _table(walked)).all()                                                # the table does not look at the trim


@gpu
@pytest.mark.parametrize("contexts", [1, 2, 4, 5])
def test_rows_of_contexts_that_are_not_selected_stay_zero(crafted, mapper_on_gold, contexts):
    recs = crafted["recs"][:3000]
    got = mapper_on_gold.bam_methyl(b"".join(recs), [len(r) for r in recs], None, contexts=contexts, min_mapq=MIN_MAPQ, min_phred=MIN_PHRED, ignore_3p=(4, 9), mbias=True)
    walked = mbias_spec.walk(crafted["seqs"], recs, None, MIN_MAPQ, MIN_PHRED)
    assert _site_tuples(got) == mbias_spec.sites_of(walked, contexts, (0, 0), (4, 9))
    t = mapper_on_gold.methyl_mbias()
    assert (t == _table(walked, contexts)).all()
    for ctx in range(3):
        assert t[:, :, ctx].any() == bool(contexts >> ctx & 1)


@gpu
def test_a_stack_of_records_on_200_bases(crafted, mapper_on_gold):
    """20 000 records of 32 bases on the same 200 bases: many lanes of a block add to one word of its table at once, and every
    counter is the sum over all blocks"""
    recs = crafted["stack"]
    got = mapper_on_gold.bam_methyl(b"".join(recs), [len(r) for r in recs], None, contexts=7, min_mapq=MIN_MAPQ, min_phred=MIN_PHRED, ignore_5p=(2, 1), ignore_3p=(7, 4),
                                    mbias=True)
    assert _site_tuples(got) == mbias_spec.sites_of(crafted["stack_walked"], 7, (2, 1), (7, 4))
    assert (mapper_on_gold.methyl_mbias() == _table(crafted["stack_walked"])).all()


SLICE_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from bitmapperbs_amd import mapper
d = np.load(sys.argv[3], allow_pickle=False)
m = mapper.Mapper(mapper.Index(sys.argv[2]), 0)
got = m.bam_methyl(d["stream"].tobytes(), d["lens"], d["clip"], contexts=7, min_mapq=int(sys.argv[5]), min_phred=int(sys.argv[6]), ignore_5p=(2, 1), ignore_3p=(7, 4), mbias=True)
np.savez(sys.argv[4], sites=got, table=m.methyl_mbias())
m.close()
"""


@gpu
def test_slices_of_records_give_the_same_table_and_sites(crafted, gold, tmp_path):
    """BMBS_METHYL_EVENTS (read once: a child process) cuts the events into slices; the table is made once over all records"""
    recs = crafted["recs"][:5000] + crafted["stack"][:5000]
    clip = crafted["clip"][:5000] + [0] * 5000
    np.savez(tmp_path / "in.npz", stream=np.frombuffer(b"".join(recs), dtype=np.uint8), lens=np.array([len(r) for r in recs], dtype=np.uint32),
             clip=np.array(clip, dtype=np.uint32))
    open(tmp_path / "child.py", "w").write(SLICE_CHILD)
    p = subprocess.run([os.sys.executable, str(tmp_path / "child.py"), ROOT, gold["fa"], str(tmp_path / "in.npz"), str(tmp_path / "out.npz"), str(MIN_MAPQ), str(MIN_PHRED)],
                       capture_output=True, text=True, env=dict(os.environ, BMBS_METHYL_EVENTS="5000"))
    assert p.returncode == 0, p.stderr
    walked = _upto(crafted["walked"], 5000) + [(c[0] + 5000,) + c[1:] for c in crafted["stack_walked"] if c[0] < 5000]
    assert len(walked) > 10 * 5000                                                     # more than ten slices
    out = np.load(tmp_path / "out.npz")
    assert _site_tuples(out["sites"]) == mbias_spec.sites_of(walked, 7, (2, 1), (7, 4))
    assert (out["table"] == _table(walked)).all()


@gpu
@pytest.mark.parametrize("raw", [True, False])
def test_bam_sort_methyl_with_options_equals_bam_methyl(crafted, mapper_on_gold, raw):
    m = mapper_on_gold
    some, clip = crafted["recs"][:5000], crafted["clip"][:5000]
    keep = [i for i, r in enumerate(some) if r]
    kw = dict(contexts=7, min_mapq=MIN_MAPQ, min_phred=MIN_PHRED, ignore_5p=(2, 1), ignore_3p=(7, 4), mbias=True)
    want = m.bam_methyl(b"".join(some), [len(r) for r in some], clip, **kw).tobytes()
    want_t = m.methyl_mbias()
    m.bam_sort(b"".join(some[i] for i in keep), [len(some[i]) for i in keep], raw=raw)
    assert m.bam_sort_methyl([clip[i] for i in keep], **kw).tobytes() == want
    assert (m.methyl_mbias() == want_t).all() and want_t.any()
    assert _site_tuples(np.frombuffer(want, dtype=m.methyl_sites().dtype)) == mbias_spec.sites_of(_upto(crafted["walked"], 5000), 7, (2, 1), (7, 4))


# ---- 2. defaults and refusals ---------------------------------------------------------------------------------------------------------------
def _opts_call(m, recs, opts):
    from bitmapperbs_amd import capi
    stream = np.frombuffer(b"".join(recs), dtype=np.uint8)
    lens = np.array([len(r) for r in recs], dtype=np.uint32)
    n = ctypes.c_int64(0)
    return m._lib.bmbs_bam_methyl_opts(m._ctx, capi.ptr(stream), stream.size, capi.ptr(lens), lens.size, None, ctypes.byref(opts), ctypes.byref(n))


@gpu
def test_defaults_are_the_old_calls_and_leave_no_table(crafted, mapper_on_gold):
    from bitmapperbs_amd import capi
    m = mapper_on_gold
    recs = [r for r in crafted["recs"][:3000] if r]
    lens = [len(r) for r in recs]
    old = m.bam_methyl(b"".join(recs), lens, None, contexts=7)                        # default keywords: bmbs_bam_methyl
    assert len(old) > 1000
    with pytest.raises(RuntimeError, match="bmbs error -1:"):
        m.methyl_mbias()                                                               # that call did not ask for the table
    assert m.bam_methyl(b"".join(recs), lens, None, contexts=7, mbias=True).tobytes() == old.tobytes()
    assert m.methyl_mbias().any()
    # the _opts entry point with flags 0 and no trim: the same sites, no table
    assert _opts_call(m, recs, capi.MethylOpts(7, 10, 5, 0, (ctypes.c_int32 * 2)(0, 0), (ctypes.c_int32 * 2)(0, 0))) == 0
    assert m.methyl_sites().tobytes() == old.tobytes()
    with pytest.raises(RuntimeError, match="bmbs error -1:"):
        m.methyl_mbias()
    m.bam_sort(b"".join(recs), lens)
    assert m.bam_sort_methyl(None, contexts=7).tobytes() == old.tobytes() == m.bam_sort_methyl(None, contexts=7, mbias=True).tobytes()
    # a failed call leaves no table either
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*parameters"):
        m.bam_methyl(b"".join(recs), lens, None, contexts=8, mbias=True)
    with pytest.raises(RuntimeError, match="bmbs error -1:"):
        m.methyl_mbias()
    # n = 0 is valid and leaves an all-zero table
    assert len(m.bam_methyl(b"", np.zeros(0, dtype=np.uint32), mbias=True)) == 0
    t = m.methyl_mbias()
    assert t.shape == mbias_spec.SHAPE and not t.any()


@gpu
def test_refusals(crafted, mapper_on_gold):
    from bitmapperbs_amd import capi
    m = mapper_on_gold
    recs = [r for r in crafted["recs"][:400] if r][:100]
    lens = [len(r) for r in recs]
    for kw in (dict(ignore_5p=(-1, 0)), dict(ignore_5p=(0, 65536)), dict(ignore_3p=(65536, 0)), dict(ignore_3p=(0, -1))):
        with pytest.raises(RuntimeError, match=r"bmbs error -22: .*parameters"):
            m.bam_methyl(b"".join(recs), lens, **kw)
    assert len(m.bam_methyl(b"".join(recs), lens, ignore_5p=(65535, 65535), ignore_3p=(65535, 65535))) == 0     # every cycle ignored: no error
    assert _opts_call(m, recs, capi.MethylOpts(1, 10, 5, 2, (ctypes.c_int32 * 2)(0, 0), (ctypes.c_int32 * 2)(0, 0))) == -22
    assert re.search("parameters", m._lib.bmbs_last_error(m._ctx).decode())
    m.bam_sort(b"".join(recs), lens, raw=True)
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*parameters"):
        m.bam_sort_methyl(None, ignore_5p=(0, 65536))
    # a cap that is too small: BMBS_ENOMEM with n set
    m.bam_methyl(b"".join(recs), lens, mbias=True)
    n = ctypes.c_int64(0)
    small = np.zeros(100, dtype=np.uint64)
    assert m._lib.bmbs_methyl_mbias(m._ctx, capi.ptr(small), 100, ctypes.byref(n)) == -12 and n.value == 24 * capi.MBIAS_CYCLES == 24 * 1024
    assert not small.any()
    assert m._lib.bmbs_methyl_mbias(m._ctx, None, 0, ctypes.byref(n)) == -12 and n.value == 24 * 1024            # the size query


# ---- the driver -------------------------------------------------------------------------------------------------------------------------------
ALL = tm.ALL_CONTEXTS
TRIM_ARGS = ["--methyl-ignore", "3", "--methyl-ignore-3prime", "2", "--methyl-ignore-r2", "6", "--methyl-ignore-3prime-r2", "1"]
TRIM = ((3, 6), (2, 1))


def _tsv_table(data):
    """<prefix>_mbias.tsv -> the table"""
    lines = data.decode().split("\n")
    assert lines[0] == "#context\tstrand\tread\tcycle\tmethylated\tunmethylated\tpercent" and lines[-1] == ""
    t = np.zeros(mbias_spec.SHAPE, dtype=np.uint64)
    for line in lines[1:-1]:
        c, s, r, cy, me, un, _pct = line.split("\t")
        t[int(r) - 1, ("OT", "OB").index(s), spec.CONTEXT_NAMES.index(c), :, int(cy) - 1] = (int(un), int(me))
    return t


# ---- 3. planted bias ------------------------------------------------------------------------------------------------------------------------------
def _biased_pairs(fa, n_pe, L=100, bias=5):
    """test_methyl.py's planted pairs (a cytosine of the pair's strand stays exactly when its position is a multiple of 3) whose read 2
    has the first `bias` cycles unconverted, as end repair leaves them: there it shows the genome's own letters"""
    rng = np.random.default_rng(12)
    texts = [t.encode() for t in ("".join(b.split("\n")[1:]).upper() for b in open(fa).read().split(">")[1:])]
    q = "I" * L
    pe1, pe2 = [], []
    for i in range(n_pe):
        ref = int(rng.integers(0, len(texts))); F = int(rng.integers(120, 321)); p = int(rng.integers(0, len(texts[ref]) - F)); ob = bool(rng.integers(0, 2))
        T = texts[ref]
        if ob:            # read 1 reverse at the right end, read 2 forward at the left end: its first cycles are the fragment's first bases
            r1 = tm._planted(T, p + F - L, p + F, ob).translate(tm._COMP)[::-1]
            r2 = T[p:p + bias] + tm._planted(T, p + bias, p + L, ob)
            p1, p2 = p + F - L, p
        else:             # read 1 forward at the left end, read 2 reverse at the right end: its first cycles are the fragment's last bases
            r1 = tm._planted(T, p, p + L, ob)
            r2 = (tm._planted(T, p + F - L, p + F - bias, ob) + T[p + F - bias:p + F]).translate(tm._COMP)[::-1]
            p1, p2 = p, p + F - L
        nm = "p%d_%d_%d_%d_%d" % (i, ref, p1, p2, ob)
        pe1.append("@%s/1\n%s\n+\n%s\n" % (nm, r1.decode(), q)); pe2.append("@%s/2\n%s\n+\n%s\n" % (nm, r2.decode(), q))
    return "".join(pe1), "".join(pe2)


@gpu
def test_planted_read_2_bias_shows_in_the_table_and_the_trim_removes_it(gold, tmp_path):
    n_pe = 400
    pe1, pe2 = _biased_pairs(gold["fa"], n_pe)
    open(tmp_path / "1.fq", "w").write(pe1); open(tmp_path / "2.fq", "w").write(pe2)
    inputs, args = ["--seq1", str(tmp_path / "1.fq"), "--seq2", str(tmp_path / "2.fq")], json.load(open(os.path.join(GOLD, "pe_args.json")))["p100"]
    out, pre, pre5 = str(tmp_path / "o.bam"), str(tmp_path / "m"), str(tmp_path / "t")
    tm._run(gold["fa"], inputs, args + ["--sort", "--methyl", pre, "--mbias"] + ALL, out)
    recs = split_records(bam_payload(out)[1])
    tm._run(gold["fa"], inputs, args + ["--sort", "--methyl", pre5, "--methyl-ignore-r2", "5"] + ALL, out)
    assert split_records(bam_payload(out)[1]) == recs
    # the records at home: where they were made, one M operation
    is_home = []
    for r in recs:
        ref, pos, _mq, flag, cigar, _b, _q = spec.fields(r)
        f = tm._name(r).decode().split("_")
        is_home.append((ref, pos) == (int(f[1]), int(f[3] if flag & 0x80 else f[2])) and len(cigar) == 1 and cigar[0][0] == 0 and not flag & 4)
    assert 2 * sum(is_home) >= 2 * n_pe, (sum(is_home), 2 * n_pe)
    # the spec's calls of the file's records, with the clips of their pairs
    by_name = {(tm._name(r), spec.fields(r)[3] & 0xc0): r for r in recs}
    clip = [spec.clip_of(r, by_name.get((tm._name(r), spec.fields(r)[3] & 0xc0 ^ 0xc0))) for r in recs]
    assert sum(1 for c in clip if c) > 50
    walked = mbias_spec.walk(gold["seqs"], recs, clip)
    t = _tsv_table(open(pre + "_mbias.tsv", "rb").read())
    assert (t == _table(walked)).all()
    # read 2, cycles 1-5: every row and cycle whose calls all come from records at home is 100 % methylated in the file's table; and so
    # is every row of the table without the calls of the other records (the file's table is the spec's, just shown).  Read 1 shows the
    # planted third
    foreign = {(c[1], c[7], c[6], c[8]) for c in walked if not is_home[c[0]]}
    t_home = _table([c for c in walked if is_home[c[0]]])
    checked = 0
    for strand in range(2):
        for ctx in range(3):
            for cy in range(5):
                if (1, strand, ctx, cy) not in foreign and t[1, strand, ctx, :, cy].any():
                    assert t[1, strand, ctx, 0, cy] == 0 and t[1, strand, ctx, 1, cy] > 0
                    checked += 1
        assert not t_home[1, strand, :, 0, :5].any() and t_home[1, strand, :, 1, :5].all()
        assert t_home[0, strand, :, 0, :5].sum() > t_home[0, strand, :, 1, :5].sum() > 0
        assert t_home[1, strand, :, 0, 5:].sum() > t_home[1, strand, :, 1, 5:].sum() > 0
    assert checked >= 1
    assert all(bool(c[5]) == (c[4] % 3 == 0) for c in walked if is_home[c[0]] and (c[1] == 0 or c[8] >= 5))
    # the bedGraph lines at sites that only records at home call: with --methyl-ignore-r2 5 they follow the planted pattern, without it
    # some do not
    names = {n: i for i, n in enumerate(gold["names"])}
    mixed = {(c[3], c[4]) for c in walked if not is_home[c[0]]}

    def off_pattern(prefix):
        bad = seen = 0
        for f in tm._files(prefix):
            for line in f.decode().split("\n")[1:-1]:
                c, p, _e, pct, me, un = line.split("\t")
                if (names[c], int(p)) not in mixed:
                    seen += 1
                    bad += not ((int(un) == 0 and pct == "100") if int(p) % 3 == 0 else (int(me) == 0 and pct == "0"))
        assert seen > 1000
        return bad
    assert off_pattern(pre5) == 0 and off_pattern(pre) > 0


# ---- 4. the driver against the spec -----------------------------------------------------------------------------------------------------------------
def _entries(R):
    """what test_methyl.py's `runs` made its sites from: the plain run's records per template (b"" where a line printed nothing)"""
    fq = R["inputs"][1]
    n = sum(1 for _ in open(fq)) // 4
    return tm._by_template(split_records(bam_payload(str(R["wd"] / "plain.bam"))[1]), n, R["paired"], "d")


def _check_run(gold, R, entries, pre, err):
    walked = mbias_spec.walk(gold["seqs"], entries, R["clip"])
    want_sites = mbias_spec.sites_of(walked, 7, *TRIM)
    assert tm._files(pre) == tm._spec_files(pre, gold["names"], want_sites)
    want_t = mbias_spec.table_of(walked, 7)
    assert open(pre + "_mbias.tsv", "rb").read() == mbias_spec.tsv(want_t)
    assert int(re.search(r"methyl: sites .*, mbias calls (\d+)", err).group(1)) == mbias_spec.total(want_t) > sum(s[2] + s[3] for s in want_sites) > 1000
    return want_sites


@gpu
@pytest.mark.parametrize("kind", ["se", "pe"])
def test_driver_files_equal_the_spec(gold, runs, kind):
    R = runs(kind)
    wd = R["wd"]
    pre = str(wd / "mb")
    base = R["args"] + ["--sort", "--bai", "--methyl", pre] + ALL
    tm._run(gold["fa"], R["inputs"], base, str(wd / "mb.bam"))
    without = (open(wd / "mb.bam", "rb").read(), open(str(wd / "mb.bam") + ".bai", "rb").read())
    plain_files = tm._files(pre)
    assert plain_files == tm._spec_files(pre, gold["names"], R["sites"]) and not os.path.exists(pre + "_mbias.tsv")
    err = tm._run(gold["fa"], R["inputs"], base + ["--mbias"] + TRIM_ARGS, str(wd / "mb.bam"))
    want_sites = _check_run(gold, R, _entries(R), pre, err)
    assert want_sites != R["sites"] and tm._files(pre) != plain_files                 # the trim took calls away
    # the BAM and its index are those of the run without the new options into the same file, byte for byte (the header names none of them)
    assert (open(wd / "mb.bam", "rb").read(), open(str(wd / "mb.bam") + ".bai", "rb").read()) == without
    assert without[1] == bai_spec.spec_bai(str(wd / "mb.bam"))


@gpu
@pytest.mark.parametrize("geometry", range(len(tm.GEOMETRIES)))
@pytest.mark.parametrize("kind", ["se", "pe"])
def test_driver_files_with_markdup_under_other_geometries(gold, runs, kind, geometry):
    """small pass-2 calls, few bins, small batches and two contexts: the calls' tables add up to the same table"""
    R = runs(kind)
    env, more = tm.GEOMETRIES[geometry]
    pre = str(R["wd"] / ("mg%d" % geometry))
    err = tm._run(gold["fa"], R["inputs"], R["args"] + ["--sort", "--bai", "--markdup", "--methyl", pre, "--mbias"] + TRIM_ARGS + ALL + more, pre + ".bam", env)
    _check_run(gold, R, markdup_spec.mark(_entries(R), R["paired"]), pre, err)
    if "BMBS_SORT_CALL_BYTES" in env:
        assert int(re.search(r"pass-2 calls (\d+)", err).group(1)) > 1


@gpu
def test_driver_refusals(gold, runs, tmp_path):
    R = runs("se")
    pre = str(tmp_path / "t")
    for bad, named in ((["--sort", "--mbias"], "--mbias needs --methyl"), (["--sort", "--methyl-ignore", "5"], "--methyl-ignore"),
                       (["--sort", "--methyl", pre, "--methyl-ignore", "-1"], "--methyl-ignore takes 0..65535"),
                       (["--sort", "--methyl", pre, "--methyl-ignore-3prime-r2", "65536"], "--methyl-ignore-3prime-r2 takes 0..65535")):
        p = subprocess.run([tm._driver(), "--search", gold["fa"]] + R["inputs"] + ["-o", str(tmp_path / "x.bam"), "--bam"] + bad, capture_output=True, text=True)
        assert p.returncode == 2 and named in p.stderr, p.stderr
    assert not os.path.exists(pre + "_mbias.tsv") and not os.path.exists(str(tmp_path / "x.bam"))
