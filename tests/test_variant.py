"""The opposite-strand observation on the device (bmbs_bam_methyl_opposite, bmbs_bam_sort_methyl_opposite, bmbs_methyl_opposite), the
variant filter (bmbs_methyl_drop_variants) and `bmbs_search --methyl ... --methyl-min-opposite-depth --methyl-max-variant-frac
--methyl-merge-context --methyl-min-depth` against tests/variant_spec.py.  Entries, sites and files: every comparison is exact.

The shapes are those of test_mbias.py: record lengths across the 32-base word borders, record counts across group, wave and block
borders, holes, clips, trims, a stack of records on 200 bases, slices of events."""
import bisect
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bai_spec
import mbias_spec
import methyl_spec as spec
import test_mbias as tmb
import test_methyl as tm
import variant_spec as vs
from common import GOLD, ROOT, bam_payload
from test_mbias_spec import golden_seqs, random_records
from test_methyl import gold, mapper_on_gold, runs  # noqa: F401  (fixtures)
from test_sorted_bam import split_records

gpu = pytest.mark.gpu

MIN_MAPQ, MIN_PHRED = tm.MIN_MAPQ, tm.MIN_PHRED
L_SEQS, COUNTS, TRIMS = tmb.L_SEQS, (1, 63, 64, 65, 257, 20_000), tmb.TRIMS
# (min_opposite_depth, max_variant_ppm) of the filter tests.  About one observed base in nine of the crafted records is a variant (12 %
# mutated and 3 % errors, three of four of them to another letter), and most positions are covered once or twice, the sequences' ends
# ten times and more: bounds at which some sites go and most stay
FILTERS = ((1, 0), (2, 500_000), (3, 333_333), (5, 200_000), (8, 125_000))
N_FILTER = 5000                                       # the records whose sites are filtered


def _trim(t):
    return (t[0], t[1]), (t[2], t[3])


def _tuples(a):
    return [(int(r["ref"]), int(r["pos"]), int(r["meth"]), int(r["unmeth"]), int(r["kind"])) for r in a]


def _upto(walked, count):
    """the observations of records 0 .. count - 1 (the list is in record order)"""
    return walked[:bisect.bisect_left(walked, (count,))]


def _mutated(rng, rec, share=0.12):
    """the record with that share of its bases replaced by a random one of A C G T: the records of test_methyl.py's generator show the
    genome's letter at nearly every position of the OTHER strand's cytosines, which would leave the variant counts almost empty"""
    if not rec:
        return rec
    l_name, n_cig, l_seq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<I", rec, 20)[0]
    s_at = 36 + l_name + 4 * n_cig
    out = bytearray(rec)
    for i in np.nonzero(rng.random(l_seq) < share)[0].tolist():
        code = (1, 2, 4, 8)[int(rng.integers(0, 4))]
        b = out[s_at + (i >> 1)]
        out[s_at + (i >> 1)] = (b & 0xf0 | code) if i & 1 else (b & 0x0f | code << 4)
    return bytes(out)


# ---- 1. crafted records -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crafted():
    """20 000 random records (every 11th entry a hole) with their clips and 20 000 stacked on 200 bases, and every observation the spec
    finds in them, every context -- walked once; the entries of any count, trim and selection are sums over that list.  The calls of the
    first N_FILTER records too, for the filter.  No GPU."""
    rng = np.random.default_rng(29)
    seqs = golden_seqs()
    recs = [b"" if i % 11 == 6 else _mutated(rng, r) for i, r in enumerate(random_records(rng, seqs, COUNTS[-1], L_SEQS))]
    clip = [tm._random_clip(rng, r) if r else 0 for r in recs]
    stack = [_mutated(rng, r) for r in random_records(rng, seqs, COUNTS[-1], L_SEQS, stack=True)]
    return dict(seqs=seqs, recs=recs, clip=clip, stack=stack, walked=vs.walk(seqs, recs, clip, MIN_MAPQ, MIN_PHRED),
                stack_walked=vs.walk(seqs, stack, None, MIN_MAPQ, MIN_PHRED),
                calls=mbias_spec.walk(seqs, recs[:N_FILTER], clip[:N_FILTER], MIN_MAPQ, MIN_PHRED))


def test_the_crafted_records_are_not_trivial(crafted):
    """on the spec alone (no GPU)"""
    walked, recs = crafted["walked"], crafted["recs"]
    entries = vs.entries_of(walked, 7)
    # entries of every kind, with matches, with variants and with both; observations of both record strands
    for kind in (0, 1, 2, 4, 5, 6):
        of = [e for e in entries if e[4] == kind]
        assert len(of) > 1000 and sum(1 for e in of if e[2]) > 100 and sum(1 for e in of if e[3]) > 100 and sum(1 for e in of if e[2] and e[3]) > 100, kind
    counting = [r for r in recs if r and not spec.skip_reason(r, MIN_MAPQ)]
    assert {spec.is_ob(spec.fields(r)[3]) for r in counting} == {False, True}
    assert {c[7] for c in walked} == {0, 1}                                            # (strand 0: seen on an OB record)
    assert {spec.fields(r)[3] & 0xd1 for r in counting} >= {0, 0x10, 0x41, 0x51, 0x81, 0x91}
    # every CIGAR operation, holes, records that do not count, clips and trims that take observations away
    assert {op for r in counting for op, _ in spec.fields(r)[4]} == set(range(9))
    assert sum(1 for r in recs if not r) > 1000 and sum(1 for r in recs if r and spec.skip_reason(r, MIN_MAPQ)) > 1000
    assert len(vs.walk(crafted["seqs"], recs[:3000], None, MIN_MAPQ, MIN_PHRED)) > len(_upto(walked, 3000))
    for trim in TRIMS[1:]:
        kept = sum(1 for c in walked if mbias_spec.keeps(c[8], c[2], c[1], *_trim(trim)))
        assert kept < len(walked) and (kept > 0) == (trim != TRIMS[-1]), trim
    # the codes that are nothing do occur where a record is looked at: more positions are looked at than observed
    assert any(15 in spec.fields(r)[5] for r in counting)
    # the filter: entries with depth on both sides of every tested bound; every tested pair drops some sites and keeps some; some sites
    # have no entry, some entries no site
    sites = mbias_spec.sites_of(crafted["calls"], 7)
    opp = vs.entries_of(_upto(walked, N_FILTER), 7)
    assert len(sites) > 10_000
    for depth, ppm in FILTERS:
        assert sum(1 for e in opp if e[2] + e[3] == depth - 1) > 10 or depth == 1
        assert sum(1 for e in opp if e[2] + e[3] == depth) > 10 and sum(1 for e in opp if e[2] + e[3] > depth) > 10
        left = vs.drop_variants(sites, opp, depth, ppm)
        assert 100 < len(left) < len(sites) - 100, (depth, ppm, len(left), len(sites))
    keys_s, keys_o = {s[:2] for s in sites}, {e[:2] for e in opp}
    assert len(keys_s - keys_o) > 100 and len(keys_o - keys_s) > 100 and len(keys_s & keys_o) > 1000
    # the stack: some position is observed by more records than two blocks of the reduction hold
    stack = vs.entries_of(crafted["stack_walked"], 7)
    assert max(e[2] + e[3] for e in stack) > 2 * 256 and all(e[0] == 0 and e[1] < 200 for e in stack)
    assert sum(1 for e in stack if e[2] > 20 and e[3] > 20) > 10


@gpu
@pytest.mark.parametrize("trim", TRIMS)
@pytest.mark.parametrize("count", COUNTS)
def test_entries_equal_the_spec(crafted, mapper_on_gold, count, trim):
    recs, i53 = crafted["recs"][:count], _trim(trim)
    got = mapper_on_gold.bam_methyl_opposite(b"".join(recs), [len(r) for r in recs], crafted["clip"][:count], contexts=7, min_mapq=MIN_MAPQ, min_phred=MIN_PHRED,
                                             ignore_5p=i53[0], ignore_3p=i53[1])
    assert _tuples(got) == vs.entries_of(_upto(crafted["walked"], count), 7, *i53)
    assert not got["pad"].any()


@gpu
@pytest.mark.parametrize("contexts", [1, 2, 4, 5])
def test_context_selections(crafted, mapper_on_gold, contexts):
    recs = crafted["recs"][:3000]
    got = mapper_on_gold.bam_methyl_opposite(b"".join(recs), [len(r) for r in recs], None, contexts=contexts, min_mapq=MIN_MAPQ, min_phred=MIN_PHRED, ignore_3p=(4, 9))
    walked = vs.walk(crafted["seqs"], recs, None, MIN_MAPQ, MIN_PHRED)
    want = vs.entries_of(walked, contexts, (0, 0), (4, 9))
    assert _tuples(got) == want and 0 < len(want) < len(vs.entries_of(walked, 7, (0, 0), (4, 9)))
    assert {e[4] & 3 for e in want} == {c for c in range(3) if contexts >> c & 1}


@gpu
def test_a_stack_of_records_on_200_bases(crafted, mapper_on_gold):
    """20 000 records of 32 bases on the same 200 bases: a position's run of events crosses waves and blocks of the reduction"""
    recs = crafted["stack"]
    got = mapper_on_gold.bam_methyl_opposite(b"".join(recs), [len(r) for r in recs], None, contexts=7, min_mapq=MIN_MAPQ, min_phred=MIN_PHRED, ignore_5p=(2, 1), ignore_3p=(7, 4))
    assert _tuples(got) == vs.entries_of(crafted["stack_walked"], 7, (2, 1), (7, 4))


@gpu
@pytest.mark.parametrize("depth,ppm", FILTERS)
def test_the_filter_on_the_device_results(crafted, mapper_on_gold, depth, ppm):
    from bitmapperbs_amd import mapper
    m = mapper_on_gold
    recs, clip = crafted["recs"][:N_FILTER], crafted["clip"][:N_FILTER]
    kw = dict(contexts=7, min_mapq=MIN_MAPQ, min_phred=MIN_PHRED)
    sites = m.bam_methyl(b"".join(recs), [len(r) for r in recs], clip, **kw)
    opp = m.bam_methyl_opposite(b"".join(recs), [len(r) for r in recs], clip, **kw)
    want_sites = mbias_spec.sites_of(crafted["calls"], 7)
    assert _tuples(sites) == want_sites
    assert _tuples(mapper.drop_variants(sites, opp, depth, ppm)) == vs.drop_variants(want_sites, vs.entries_of(_upto(crafted["walked"], N_FILTER), 7), depth, ppm)


SLICE_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from bitmapperbs_amd import mapper
d = np.load(sys.argv[3], allow_pickle=False)
m = mapper.Mapper(mapper.Index(sys.argv[2]), 0)
got = m.bam_methyl_opposite(d["stream"].tobytes(), d["lens"], d["clip"], contexts=7, min_mapq=int(sys.argv[5]), min_phred=int(sys.argv[6]), ignore_5p=(2, 1), ignore_3p=(7, 4))
np.save(sys.argv[4], got)
m.close()
"""


@gpu
def test_slices_of_records_give_the_same_entries(crafted, gold, tmp_path):
    """BMBS_METHYL_EVENTS (read once: a child process) cuts the events into slices whose entries are merged"""
    recs = crafted["recs"][:5000] + crafted["stack"][:5000]
    clip = crafted["clip"][:5000] + [0] * 5000
    np.savez(tmp_path / "in.npz", stream=np.frombuffer(b"".join(recs), dtype=np.uint8), lens=np.array([len(r) for r in recs], dtype=np.uint32),
             clip=np.array(clip, dtype=np.uint32))
    open(tmp_path / "child.py", "w").write(SLICE_CHILD)
    p = subprocess.run([os.sys.executable, str(tmp_path / "child.py"), ROOT, gold["fa"], str(tmp_path / "in.npz"), str(tmp_path / "out.npy"), str(MIN_MAPQ), str(MIN_PHRED)],
                       capture_output=True, text=True, env=dict(os.environ, BMBS_METHYL_EVENTS="5000"))
    assert p.returncode == 0, p.stderr
    walked = _upto(crafted["walked"], 5000) + [(c[0] + 5000,) + c[1:] for c in crafted["stack_walked"] if c[0] < 5000]
    want = vs.entries_of(walked, 7, (2, 1), (7, 4))
    assert sum(e[2] + e[3] for e in want) > 10 * 5000                                  # more than ten slices
    assert _tuples(np.load(tmp_path / "out.npy")) == want


@gpu
@pytest.mark.parametrize("raw", [True, False])
def test_bam_sort_methyl_opposite_between_two_bam_sort_methyl_calls(crafted, mapper_on_gold, raw):
    m = mapper_on_gold
    some, clip = crafted["recs"][:5000], crafted["clip"][:5000]
    keep = [i for i, r in enumerate(some) if r]
    kw = dict(contexts=7, min_mapq=MIN_MAPQ, min_phred=MIN_PHRED, ignore_5p=(2, 1), ignore_3p=(7, 4))
    want_sites = m.bam_methyl(b"".join(some), [len(r) for r in some], clip, **kw).tobytes()
    want_opp = m.bam_methyl_opposite(b"".join(some), [len(r) for r in some], clip, **kw)
    assert _tuples(want_opp) == vs.entries_of(_upto(crafted["walked"], 5000), 7, (2, 1), (7, 4)) and len(want_opp) > 1000
    m.bam_sort(b"".join(some[i] for i in keep), [len(some[i]) for i in keep], raw=raw)
    k_clip = [clip[i] for i in keep]
    first = m.bam_sort_methyl(k_clip, **kw).tobytes()
    second = m.bam_sort_methyl_opposite(k_clip, **kw).tobytes()
    third = m.bam_sort_methyl(k_clip, **kw).tobytes()
    assert first == want_sites and second == want_opp.tobytes() and third == first
    # ... and before one: a fresh sort, the opposite call first
    m.bam_sort(b"".join(some[i] for i in keep), [len(some[i]) for i in keep], raw=raw)
    assert m.bam_sort_methyl_opposite(k_clip, **kw).tobytes() == second and m.bam_sort_methyl(k_clip, **kw).tobytes() == first


# ---- 2. one result at a time, refusals --------------------------------------------------------------------------------------------------------
def _opposite_call(m, recs, opts):
    from bitmapperbs_amd import capi
    stream = np.frombuffer(b"".join(recs), dtype=np.uint8)
    lens = np.array([len(r) for r in recs], dtype=np.uint32)
    n = ctypes.c_int64(0)
    return m._lib.bmbs_bam_methyl_opposite(m._ctx, capi.ptr(stream), stream.size, capi.ptr(lens), lens.size, None, ctypes.byref(opts) if opts is not None else None, ctypes.byref(n)), n.value


@gpu
def test_state_rules_and_refusals(crafted, mapper_on_gold, gold):
    from bitmapperbs_amd import capi, mapper
    m = mapper_on_gold
    recs = [r for r in crafted["recs"][:400] if r][:100]
    lens = [len(r) for r in recs]
    stream = b"".join(recs)
    zero2 = (ctypes.c_int32 * 2)(0, 0)
    # a context holds one result: each kind of call ends the other's, and the fetch of the wrong kind says so
    sites = m.bam_methyl(stream, lens, contexts=7)
    assert len(sites) > 100
    with pytest.raises(RuntimeError, match=r"bmbs error -1: .*not an opposite call.*bmbs_methyl_sites"):
        m.methyl_opposite()
    opp = m.bam_methyl_opposite(stream, lens, contexts=7)
    assert len(opp) > 100 and m.methyl_opposite().tobytes() == opp.tobytes()
    with pytest.raises(RuntimeError, match=r"bmbs error -1: .*opposite call.*bmbs_methyl_opposite"):
        m.methyl_sites()
    with pytest.raises(RuntimeError, match="bmbs error -1:"):
        m.methyl_mbias()
    assert m.bam_methyl(stream, lens, contexts=7, mbias=True).tobytes() == sites.tobytes()
    with pytest.raises(RuntimeError, match="bmbs error -1:"):
        m.methyl_opposite()
    # opts NULL: the defaults (CpG, MAPQ 10, quality 5, no trim)
    rc, n = _opposite_call(m, recs, None)
    assert rc == 0 and n > 0 and m.methyl_opposite().tobytes() == m.bam_methyl_opposite(stream, lens).tobytes()
    assert _tuples(m.methyl_opposite()) == vs.entries(crafted["seqs"], recs)
    # flags must be 0
    for flags in (capi.METHYL_MBIAS, 2):
        rc, n = _opposite_call(m, recs, capi.MethylOpts(1, 10, 5, flags, zero2, zero2))
        assert rc == -22 and n == 0 and re.search("parameters", m._lib.bmbs_last_error(m._ctx).decode())
        with pytest.raises(RuntimeError, match="bmbs error -1:"):
            m.methyl_opposite()                                                        # the failed call left no result
    assert _opposite_call(m, [], capi.MethylOpts(1, 10, 5, capi.METHYL_MBIAS, zero2, zero2))[0] == -22
    # every other check is that of the _opts call
    for kw in (dict(contexts=8), dict(contexts=0), dict(min_mapq=256), dict(min_phred=-1), dict(ignore_5p=(0, 65536)), dict(ignore_3p=(-1, 0))):
        with pytest.raises(RuntimeError, match=r"bmbs error -22: .*parameters"):
            m.bam_methyl_opposite(stream, lens, **kw)
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 12\b.*block_size"):
        bad = np.array(lens, dtype=np.uint32); bad[12] += 4; bad[13] -= 4
        m.bam_methyl_opposite(stream, bad)
    off_end = spec.make_record(1, len(gold["seqs"][1]) - 9, 16, [("M", 10)], "ACGTACGTAC", [30] * 10)
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 3\b.*runs off"):
        m.bam_methyl_opposite(b"".join(recs[:3]) + off_end, lens[:3] + [len(off_end)])
    assert len(m.bam_methyl_opposite(stream, lens, ignore_5p=(65535, 65535))) == 0     # every cycle ignored: no error
    # n = 0 is valid, holes only too
    assert len(m.bam_methyl_opposite(b"", np.zeros(0, dtype=np.uint32))) == 0 and len(m.bam_methyl_opposite(b"", np.zeros(5, dtype=np.uint32))) == 0
    with pytest.raises(RuntimeError, match="bmbs error -1:"):
        m.methyl_sites()
    # the fetch: BMBS_ENOMEM with n set when the array is too small, a cap of 0 is the size query
    opp = m.bam_methyl_opposite(stream, lens, contexts=7)
    n = ctypes.c_int64(0)
    small = np.zeros(10, dtype=capi.METHYL_SITE_DTYPE)
    assert m._lib.bmbs_methyl_opposite(m._ctx, capi.ptr(small), 10, ctypes.byref(n)) == -12 and n.value == len(opp) > 10
    assert not small["meth"].any() and not small["unmeth"].any()
    assert m._lib.bmbs_methyl_opposite(m._ctx, None, 0, ctypes.byref(n)) == -12 and n.value == len(opp)
    big = np.zeros(len(opp) + 3, dtype=capi.METHYL_SITE_DTYPE)
    assert m._lib.bmbs_methyl_opposite(m._ctx, capi.ptr(big), big.size, ctypes.byref(n)) == 0 and n.value == len(opp) and big[:len(opp)].tobytes() == opp.tobytes()
    # no index, no resident sort
    bare = mapper.Mapper(None, 0)
    with pytest.raises(RuntimeError, match="bmbs error -1: .*no index"):
        bare.bam_methyl_opposite(stream, lens)
    bare.close()
    m2 = mapper.Mapper(gold["index"], 0)
    with pytest.raises(RuntimeError, match="bmbs error -1: .*resident"):
        m2.bam_sort_methyl_opposite()
    m2.bam_sort(stream, lens)
    assert m2.bam_sort_methyl_opposite(contexts=7).tobytes() == opp.tobytes()
    m2.close()


# ---- 3. the driver against the spec ---------------------------------------------------------------------------------------------------------------
ALL = tm.ALL_CONTEXTS
FILTER_ARGS = ["--methyl-min-opposite-depth", "1", "--methyl-max-variant-frac", "0.333333"]
FILTER = (1, 333_333)
MERGE_ARGS, DEPTH_ARGS = ["--methyl-merge-context"], ["--methyl-min-depth", "3"]


def _records_and_clips(bam, paired):
    """the records of the file a run wrote, and the clips of their pairs as the spec gives them"""
    recs = split_records(bam_payload(bam)[1])
    if not paired:
        return recs, None
    by_name = {(tm._name(r), spec.fields(r)[3] & 0xc0): r for r in recs}
    return recs, [spec.clip_of(r, by_name.get((tm._name(r), spec.fields(r)[3] & 0xc0 ^ 0xc0))) for r in recs]


def _spec_of(gold, bam, paired):
    """sites and opposite entries of the file's records, every context"""
    recs, clip = _records_and_clips(bam, paired)
    return mbias_spec.sites_of(mbias_spec.walk(gold["seqs"], recs, clip), 7), vs.entries_of(vs.walk(gold["seqs"], recs, clip), 7)


def _want_files(pre, names, sites, opp, filt, merge, depth):
    left = vs.drop_variants(sites, opp, *FILTER) if filt else sites
    return [vs.bedgraph(pre, c, names, left, merge, 3 if depth else 1) for c in range(3)], len(sites) - len(left), \
        len(vs.lines(left, merge)) - len(vs.lines(left, merge, 3 if depth else 1))


COMBOS = [(True, False, False), (False, True, False), (False, False, True), (True, True, True)]


@pytest.fixture(scope="module")
def plain_runs(gold, runs):
    """per kind: the run without any of the new options (with --markdup, --bai and --mbias) -- the bytes of its BAM, index and M-bias table,
    its bedGraphs, and the spec's sites and opposite entries of the records of its BAM; made once"""
    made = {}

    def get(kind):
        if kind not in made:
            R = runs(kind)
            pre, bam = str(R["wd"] / "v"), str(R["wd"] / "v.bam")
            base = R["args"] + ["--sort", "--bai", "--markdup", "--methyl", pre, "--mbias"] + ALL
            tm._run(gold["fa"], R["inputs"], base, bam)
            sites, opp = _spec_of(gold, bam, R["paired"])
            made[kind] = dict(R=R, pre=pre, bam=bam, base=base, files=tm._files(pre), sites=sites, opp=opp,
                              without=(open(bam, "rb").read(), open(bam + ".bai", "rb").read(), open(pre + "_mbias.tsv", "rb").read()))
        return made[kind]
    return get


@gpu
@pytest.mark.parametrize("kind", ["se", "pe"])
def test_driver_without_the_options_writes_what_it_wrote(gold, plain_runs, kind):
    P = plain_runs(kind)
    assert P["files"] == tm._spec_files(P["pre"], gold["names"], P["sites"]) and len(P["sites"]) > 1000
    assert P["without"][1] == bai_spec.spec_bai(P["bam"])
    # what the options will find to do: sites the filter drops, lines below the depth bound, CpG and CHG partners to merge
    want, n_variants, n_shallow = _want_files(P["pre"], gold["names"], P["sites"], P["opp"], True, True, True)
    assert n_variants > 0 and n_shallow > 0
    assert len(vs.lines(P["sites"], True)) < len(vs.lines(P["sites"], False))


@gpu
@pytest.mark.parametrize("combo", range(len(COMBOS)))
@pytest.mark.parametrize("kind", ["se", "pe"])
def test_driver_files_equal_the_spec(gold, plain_runs, kind, combo):
    """the filter, --methyl-merge-context and --methyl-min-depth 3, singly and together, into the files of the run without them"""
    P = plain_runs(kind)
    filt, merge, depth = COMBOS[combo]
    pre, bam = P["pre"], P["bam"]
    err = tm._run(gold["fa"], P["R"]["inputs"], P["base"] + (FILTER_ARGS if filt else []) + (MERGE_ARGS if merge else []) + (DEPTH_ARGS if depth else []), bam)
    want, n_variants, n_shallow = _want_files(pre, gold["names"], P["sites"], P["opp"], filt, merge, depth)
    assert tm._files(pre) == want
    assert tm._files(pre) != P["files"] and (n_variants > 0) == filt and (n_shallow > 0) == depth
    # (the pairs' mates are clipped where they overlap and duplicates do not count: few of their positions are called three times)
    assert depth and kind == "pe" or sum(f.count(b"\n") - 1 for f in want) > 10
    m = re.search(r"sites dropped as variants (\d+), lines left out below the minimum depth (\d+)", err)
    assert m and (int(m.group(1)), int(m.group(2))) == (n_variants, n_shallow), err
    # the BAM, its index and the M-bias table do not depend on any of this (the header names none of the options)
    assert (open(bam, "rb").read(), open(bam + ".bai", "rb").read(), open(pre + "_mbias.tsv", "rb").read()) == P["without"]


@gpu
@pytest.mark.parametrize("geometry", range(len(tm.GEOMETRIES)))
@pytest.mark.parametrize("kind", ["se", "pe"])
def test_driver_files_under_other_geometries(gold, runs, kind, geometry):
    """small pass-2 calls, few bins, small batches and two contexts: a site's calls and its opposite evidence arrive in different pass-2
    calls, and the merged lists give the same files"""
    R = runs(kind)
    env, more = tm.GEOMETRIES[geometry]
    pre = str(R["wd"] / ("vg%d" % geometry))
    base = R["args"] + ["--sort", "--bai", "--markdup", "--methyl", pre, "--mbias"] + ALL + more
    tm._run(gold["fa"], R["inputs"], base, pre + ".bam", env)
    without = (open(pre + ".bam", "rb").read(), open(pre + ".bam.bai", "rb").read(), open(pre + "_mbias.tsv", "rb").read())
    err = tm._run(gold["fa"], R["inputs"], base + FILTER_ARGS + MERGE_ARGS + DEPTH_ARGS, pre + ".bam", env)
    sites, opp = _spec_of(gold, pre + ".bam", R["paired"])
    want, n_variants, n_shallow = _want_files(pre, gold["names"], sites, opp, True, True, True)
    assert tm._files(pre) == want and n_variants > 0 and n_shallow > 0
    assert (open(pre + ".bam", "rb").read(), open(pre + ".bam.bai", "rb").read(), open(pre + "_mbias.tsv", "rb").read()) == without
    if "BMBS_SORT_CALL_BYTES" in env:
        assert int(re.search(r"pass-2 calls (\d+)", err).group(1)) > 1


# ---- 4. planted polymorphisms ---------------------------------------------------------------------------------------------------------------------
N_PLANTED, PLANTED_COVER, PLANTED_L = 12, 16, 100


def _planted_variants(fa):
    """a sample whose genome has T where the golden genome has the C of a CpG, at N_PLANTED places; error-free single-end reads of both
    bisulfite strands of THAT genome, PLANTED_COVER of each strand over every place and as many over N_PLANTED control CpGs that the
    sample shares with the genome.  No cytosine is methylated: every C of an OT read reads T, every G of an OB read A.  The reads of
    the C's own strand (OT) show T at a planted place as at every unmethylated C; the OB records show T there as well (SEQ is written
    on the forward strand) -- the sample's T:A pair, which no conversion makes of a C:G pair -- and C at the controls.
    -> the FASTQ text, the planted places, the controls, and the records the reads give when each maps where it was made"""
    rng = np.random.default_rng(31)
    texts = [t.encode() for t in ("".join(b.split("\n")[1:]).upper() for b in open(fa).read().split(">")[1:])]
    L = PLANTED_L
    places, controls = [], []
    for k in range(2 * N_PLANTED):
        ref = k % len(texts)
        lo = 2000 + 5000 * (k // len(texts))
        p = texts[ref].index(b"CG", lo)
        (places if k % 2 == 0 else controls).append((ref, p))
    sample = [bytearray(t) for t in texts]
    for ref, p in places:
        sample[ref][p] = ord("T")
    reads, home = [], []
    for ref, p in places + controls:
        for ob in (False, True):
            for _ in range(PLANTED_COVER):
                a = p - int(rng.integers(10, L - 10))
                fwd = bytes(sample[ref][a:a + L])
                fwd = fwd.replace(b"G", b"A") if ob else fwd.replace(b"C", b"T")
                s = fwd.translate(tm._COMP)[::-1] if ob else fwd
                reads.append("@v%d_%d_%d_%d\n%s\n+\n%s\n" % (len(reads), ref, a, ob, s.decode(), "I" * L))
                home.append(spec.make_record(ref, a, 16 if ob else 0, [("M", L)], fwd.decode(), [40] * L))
    return "".join(reads), places, controls, home


def _check_planted_on_the_spec(seqs, recs, places, controls):
    """the spec on the records: the planted places are unmethylated cytosines without the filter and gone with it (depth 3, fraction
    0.5), the controls stay as they are -> the sites without and with the filter"""
    sites = spec.sites(seqs, recs, None, contexts=1)
    opp = vs.entries(seqs, recs, None, contexts=1)
    left = vs.drop_variants(sites, opp, 3, 500_000)
    by_pos, left_pos, opp_pos = {s[:2]: s for s in sites}, {s[:2]: s for s in left}, {e[:2]: e for e in opp}
    for key in places:
        assert by_pos[key][2] == 0 and by_pos[key][3] >= 3 and key not in left_pos, key
        assert opp_pos[key][2] >= 3 and opp_pos[key][3] == 0
    for key in controls:
        assert left_pos[key] == by_pos[key] and by_pos[key][2] == 0 and by_pos[key][3] >= 3
        assert opp_pos[key][3] >= 3 and opp_pos[key][2] == 0
    return sites, left


def test_the_planted_reads_separate_on_the_spec(tmp_path):
    """no GPU: with every read mapped where it was made, the coverage tells the planted places from the controls, and nothing else is
    dropped"""
    import gzip
    fa = tmp_path / "g.fa"
    fa.write_text(gzip.open(os.path.join(GOLD, "genome.fa.gz"), "rt").read())
    _fq, places, controls, home = _planted_variants(str(fa))
    assert len(set(places)) == N_PLANTED == len(set(controls)) and not set(places) & set(controls)
    sites, left = _check_planted_on_the_spec(golden_seqs(), home, places, controls)
    assert {s[:2] for s in sites} - {s[:2] for s in left} == set(places) and len(left) > 100


@gpu
def test_planted_polymorphisms_are_filtered_and_true_sites_stay(gold, tmp_path):
    from common import golden_args
    fq, places, controls, _home = _planted_variants(gold["fa"])
    open(tmp_path / "r.fq", "w").write(fq)
    inputs, args = ["--seq", str(tmp_path / "r.fq")], golden_args()["b150"]
    out, pre, pre_f = str(tmp_path / "o.bam"), str(tmp_path / "m"), str(tmp_path / "f")
    tm._run(gold["fa"], inputs, args + ["--sort", "--methyl", pre, "--CpG"], out)
    recs = split_records(bam_payload(out)[1])
    tm._run(gold["fa"], inputs, args + ["--sort", "--methyl", pre_f, "--CpG", "--methyl-min-opposite-depth", "3", "--methyl-max-variant-frac", "0.5"], out)
    assert split_records(bam_payload(out)[1]) == recs
    # the places whose reads all came home: mapped where they were made, one M operation, MAPQ as the calls ask (a place in a stretch
    # that the three-letter alphabet makes ambiguous says nothing about the filter)
    home = {}
    for r in recs:
        ref, pos, mapq, flag, cigar, _b, _q = spec.fields(r)
        f = tm._name(r).decode().split("_")
        home[int(f[0][1:])] = (ref, pos) == (int(f[1]), int(f[2])) and len(cigar) == 1 and cigar[0][0] == 0 and not flag & 4 and mapq >= 10 and spec.is_ob(flag) == bool(int(f[3]))
    usable = [all(home.get(2 * PLANTED_COVER * k + i, False) for i in range(2 * PLANTED_COVER)) for k in range(2 * N_PLANTED)]
    places = [key for k, key in enumerate(places) if usable[k]]
    controls = [key for k, key in enumerate(controls) if usable[N_PLANTED + k]]
    assert len(places) >= N_PLANTED // 2 and len(controls) >= N_PLANTED // 2, (len(places), len(controls))
    # the spec on the records of the file (test_the_planted_reads_separate_on_the_spec has shown it on the reads as they were made)
    sites, left = _check_planted_on_the_spec(gold["seqs"], recs, places, controls)
    dropped = {s[:2] for s in sites} - {s[:2] for s in left}
    assert set(places) <= dropped
    names = {n: i for i, n in enumerate(gold["names"])}

    def lines_of(prefix):
        out = {}
        for line in open(prefix + "_CpG.bedGraph").read().split("\n")[1:-1]:
            c, p, _e, pct, me, un = line.split("\t")
            out[names[c], int(p)] = (int(pct), int(me), int(un))
        return out
    plain, filtered = lines_of(pre), lines_of(pre_f)
    # without the filter the planted places stand in the file at 0 %; with it they are gone and every other site is there, unchanged
    for key in places:
        assert plain[key][0] == 0 and plain[key][2] >= 3 and key not in filtered
    assert filtered == {k: v for k, v in plain.items() if k not in dropped} and len(filtered) > 100
    for key in controls:
        assert filtered[key] == plain[key] and plain[key][0] == 0
    assert open(pre_f + "_CpG.bedGraph", "rb").read() == vs.bedgraph(pre_f, 0, gold["names"], left)


# ---- 5. what the driver refuses (the command line alone: no GPU) ----------------------------------------------------------------------------------
def test_driver_refusals(tmp_path):
    pre = str(tmp_path / "t")
    head = [tm._driver(), "--search", str(tmp_path / "none"), "--seq", str(tmp_path / "none.fq"), "-o", str(tmp_path / "x.bam"), "--bam", "--sort"]
    needs = "--methyl-min-opposite-depth, --methyl-max-variant-frac, --methyl-min-depth and --methyl-merge-context need --methyl"
    frac = "--methyl-max-variant-frac takes a plain decimal in 0..1 with at most 6 digits behind the point"
    cases = [(["--methyl-min-opposite-depth", "3"], needs), (["--methyl-max-variant-frac", "0.5"], needs), (["--methyl-min-depth", "2"], needs),
             (["--methyl-merge-context"], needs),
             (["--methyl", pre, "--methyl-min-opposite-depth", "-1"], "--methyl-min-opposite-depth takes 0..65535"),
             (["--methyl", pre, "--methyl-min-opposite-depth", "65536"], "--methyl-min-opposite-depth takes 0..65535"),
             (["--methyl", pre, "--methyl-min-opposite-depth", "3x"], "--methyl-min-opposite-depth takes 0..65535"),
             (["--methyl", pre, "--methyl-max-variant-frac", "0.5"], "--methyl-max-variant-frac needs --methyl-min-opposite-depth above 0"),
             (["--methyl", pre, "--methyl-min-opposite-depth", "0", "--methyl-max-variant-frac", "0.5"], "--methyl-max-variant-frac needs --methyl-min-opposite-depth above 0"),
             (["--methyl", pre, "--methyl-min-depth", "0"], "--methyl-min-depth takes 1.."),
             (["--methyl", pre, "--methyl-min-depth", "two"], "--methyl-min-depth takes 1.."),
             (["--methyl", pre, "--CHH", "--methyl-merge-context"], "--methyl-merge-context needs --CpG or --CHG")]
    cases += [(["--methyl", pre, "--methyl-min-opposite-depth", "3", "--methyl-max-variant-frac", bad], frac) for bad in ("1.0000001", "1.1", "-0", "1e-3", "", ".", "1.", "2")]
    for bad, named in cases:
        p = subprocess.run(head + bad, capture_output=True, text=True)
        assert p.returncode == 2 and named in p.stderr, (bad, p.stderr)
    # what the spec's parse_frac takes, the driver takes: --print-parts ends such a run before it needs a device or its input
    for good in ("0", "1", "1.0", "0.000001", ".5"):
        assert vs.parse_frac(good) >= 0
        p = subprocess.run(head + ["--methyl", pre, "--methyl-min-opposite-depth", "3", "--methyl-max-variant-frac", good, "--methyl-merge-context", "--methyl-min-depth", "3", "--print-parts"],
                           capture_output=True, text=True)
        assert "--methyl-max-variant-frac" not in p.stderr and "need --methyl" not in p.stderr, (good, p.stderr)
    assert not os.path.exists(str(tmp_path / "x.bam")) and not os.path.exists(pre + "_CpG.bedGraph")
