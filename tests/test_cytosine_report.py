"""The genome-wide cytosine report on the device (bmbs_methyl_report, `bmbs_search --methyl <prefix> --cytosine-report`) against
tests/cytosine_spec.py.  The report is text made of integers and letters: every comparison here is exact bytes."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cytosine_spec as cs
import methyl_spec as spec
import test_methyl as tm
import test_variant as tv
from common import bam_payload
from test_methyl import gold, mapper_on_gold, runs  # noqa: F401  (fixtures)
from test_sorted_bam import split_records
from test_variant import plain_runs  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM, ESTATE = -22, -12, -1
COUNTS = (0, 1, 9, 10, 99, 100, 999999999, 1000000000, 2 ** 32 - 1)
LONG_NAME = "c" + "x" * 199
# k_cytosine.hip: a block of k_cyt_emit owns CYT_WPB = 64 genome words = 2048 positions and formats into an LDS image of CYT_LDS bytes
CYT_WPB, CYT_LDS = 64, 49152


# ---- the fixture genome ---------------------------------------------------------------------------------------------------------------------
def _fixture_fasta():
    """[(name, letters)]: sequences of 1, 2, 3, 31, 32, 33, 63, 64, 65 and 130 bases, 3000 random bases under a name of one character,
    4000 C under a name of 200 characters, 4000 G, CG repeated; runs of N at a sequence's first base, at its last base, across a border
    of the genome's 32-base words (the words count the concatenated sequences), over a whole word, and single N two bases in front of
    and two bases behind a cytosine"""
    rng = np.random.default_rng(7)
    rnd = lambda n: "".join("ACGT"[x] for x in rng.integers(0, 4, n))
    seqs = [("s%d" % n, rnd(n)) for n in (1, 2, 3, 31, 32, 33, 63, 64, 65, 130)]
    seqs[2] = ("s3", "CAG")
    seqs[1] = ("s2", "CG")
    start = sum(len(s) for _, s in seqs)
    r = list(rnd(3000))
    r[0] = "N"; r[2999] = "N"
    border = 32 * ((start + 1000) // 32 + 1) - start                  # the first position of a genome word
    r[border - 2:border + 3] = "NNNNN"
    r[border + 320:border + 400] = "N" * 80
    clear = lambda p: not set("Nn") & set(r[p - 6:p + 7])
    c_at = next(p for p in range(1500, 2900) if r[p] == "C" and r[p + 1] == "G" and clear(p))
    r[c_at + 2] = "N"; r[c_at - 1] = "N"                                # two behind the C of a CpG, two in front of its G: both lines end in N
    h_at = next(p for p in range(1800, 2900) if r[p] == "C" and r[p + 1] != "G" and clear(p))
    r[h_at + 2] = "N"; r[h_at - 2] = "n"                                # two behind a C that is no CpG (its line goes), two in front of it
    g_at = next(p for p in range(2200, 2900) if r[p] == "G" and r[p - 1] != "C" and clear(p))
    r[g_at - 2] = "N"; r[g_at + 2] = "N"                                # the same for a cytosine of the other strand
    s33 = list(seqs[5][1]); s33[32] = "N"; seqs[5] = ("s33", "".join(s33))
    s65 = list(seqs[8][1]); s65[0] = "N"; seqs[8] = ("s65", "".join(s65))
    seqs += [("r", "".join(r)), (LONG_NAME, "C" * 4000), ("allG", "G" * 4000), ("cg", "CG" * 1000)]
    return seqs


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    """the fixture genome's index (the host builder), its sequences as the index holds them, the runs, a mapper on it"""
    from bitmapperbs_amd import mapper
    wd = tmp_path_factory.mktemp("cyt")
    fa = str(wd / "f.fa")
    seqs = _fixture_fasta()
    text = "".join(">%s\n%s\n" % (n, "\n".join(s[k:k + 60] for k in range(0, len(s), 60))) for n, s in seqs)
    open(fa, "w").write(text)
    mapper.Index.build(fa, fa, threads=4)
    ix = mapper.Index(fa)
    assert ix.chrom_names == [n for n, _ in seqs] and ix.chrom_len.tolist() == [len(s) for _, s in seqs]
    held = spec.genome_of_pac(ctypes.string_at(ix.view.pac, int(ix.view.pac_bytes)), ix.chrom_len)
    runs = spec.non_acgt_runs(text)
    ref_of = {n: i for i, n in enumerate(ix.chrom_names)}
    assert len(runs[ref_of["r"]]) >= 9 and runs[ref_of["r"]][0] == (0, 1) and runs[ref_of["r"]][-1] == (2999, 3000)
    assert runs[ref_of["s33"]] == [(32, 33)] and runs[ref_of["s65"]] == [(0, 1)]
    m = mapper.Mapper(ix, 0)
    yield dict(fa=fa, index=ix, seqs=held, names=ix.chrom_names, runs=runs, m=m, ref_of=ref_of)
    m.close()
    ix.close()


def cytosines(seqs, runs, ref, contexts=7, beg=0, end=None):
    """[(pos, kind)] of the cytosines of a window that have a line"""
    seq, rs = seqs[ref], (runs[ref] if runs else [])
    out = []
    for p in range(beg, len(seq) if end is None else end):
        c = spec.context(seq, p)
        if c is not None and contexts >> c[0] & 1 and not cs.touches(rs, *spec.window((ref, p, 0, 0, c[0] | c[1] << 2))):
            out.append((p, c[0] | c[1] << 2))
    return out


def random_sites(rng, cyt, ref, share, omit=0.1, counts=COUNTS):
    """sites on `share` of the cytosines, counts drawn from COUNTS, one in ten omitted"""
    out = []
    for p, kind in cyt:
        if rng.random() < share:
            out.append((ref, p, int(rng.choice(counts)), int(rng.choice(counts)), kind | (cs.REPORT_OMIT if rng.random() < omit else 0)))
    return out


def as_array(sites):
    from bitmapperbs_amd import capi
    a = np.zeros(len(sites), dtype=capi.METHYL_SITE_DTYPE)
    for i, (r, p, me, un, kind) in enumerate(sites):
        a[i] = (r, p, me, un, kind, 0)
    return a


def device(F, ref, beg, end, sites, contexts, runs="own"):
    if runs == "own":
        runs = F["runs"][ref] if 0 <= ref < len(F["runs"]) else None
    return F["m"].methyl_report(ref, beg, end, as_array(sites), runs, contexts)


def want(F, ref, beg, end, sites, contexts):
    return cs.report(F["seqs"], F["names"], F["runs"], sites, contexts, ref, beg, end)


# ---- 1., 2. whole sequences -------------------------------------------------------------------------------------------------------------------
def test_the_fixture_genome_is_not_trivial(fx):
    F = fx
    kinds = set()
    for ref in range(len(F["seqs"])):
        kinds |= {k for _p, k in cytosines(F["seqs"], F["runs"], ref)}
    assert kinds == {0, 1, 2, 4, 5, 6}
    r = F["ref_of"]["r"]
    whole = want(F, r, 0, 3000, [], 7).decode().split("\n")[:-1]
    assert any(l.endswith("\tCG\tCGN") for l in whole)                                # a CpG directly in front of a run
    assert len(whole) < len(cytosines(F["seqs"], None, r)) - 20                        # cytosines the runs take away
    assert want(F, F["ref_of"]["s2"], 0, 2, [], 1) == b"s2\t1\t+\t0\t0\tCG\tCGN\n" b"s2\t2\t-\t0\t0\tCG\tCGN\n"
    assert want(F, F["ref_of"]["s1"], 0, 1, [], 7) == b""


@pytest.mark.parametrize("contexts", [1, 2, 3, 4, 5, 6, 7])
def test_no_sites_every_sequence_whole(fx, contexts):
    F = fx
    total = 0
    for ref, seq in enumerate(F["seqs"]):
        got = device(F, ref, 0, len(seq), [], contexts)
        assert got == want(F, ref, 0, len(seq), [], contexts), (F["names"][ref][:10], contexts)
        total += got.count(b"\n")
    assert total > 300


@pytest.mark.parametrize("share", [1.0, 1 / 3, 0.0])
def test_random_sites_every_sequence_whole(fx, share):
    F = fx
    rng = np.random.default_rng(int(share * 100))
    n_sites = n_omit = 0
    for contexts in (7, 5):
        for ref, seq in enumerate(F["seqs"]):
            sites = random_sites(rng, cytosines(F["seqs"], F["runs"], ref, contexts), ref, share)
            n_sites += len(sites); n_omit += sum(1 for s in sites if s[4] & cs.REPORT_OMIT)
            got = device(F, ref, 0, len(seq), sites, contexts)
            assert got == want(F, ref, 0, len(seq), sites, contexts), (F["names"][ref][:10], contexts)
            assert F["m"].report_lines == got.count(b"\n")
    assert (n_sites > 5000 and n_omit > 300) if share else n_sites == 0


# ---- 3. windows -------------------------------------------------------------------------------------------------------------------------------
EDGES = [0, 1, 2, 30, 31, 32, 33, 34, 62, 63, 64, 65, 66, 128, 129, 130]


@pytest.fixture(scope="module")
def s130(fx):
    """the 130-base sequence: its random sites, and the spec's line of every position (b"" where it has none), worked out once"""
    F = fx
    ref = F["ref_of"]["s130"]
    sites = random_sites(np.random.default_rng(130), cytosines(F["seqs"], F["runs"], ref), ref, 0.6)
    by_pos = [want(F, ref, p, p + 1, [s for s in sites if s[1] == p], 7) for p in range(130)]
    assert b"".join(by_pos) == want(F, ref, 0, 130, sites, 7) and sum(1 for l in by_pos if l) > 40
    return dict(ref=ref, sites=sites, by_pos=by_pos)


def test_every_window_between_the_edges_of_the_130_base_sequence(fx, s130):
    ref, sites, by_pos = s130["ref"], s130["sites"], s130["by_pos"]
    for beg in EDGES:
        for end in EDGES:
            if beg <= end:
                got = device(fx, ref, beg, end, [s for s in sites if beg <= s[1] < end], 7)
                assert got == b"".join(by_pos[beg:end]), (beg, end)


@pytest.mark.parametrize("size", [1, 31, 32, 33, 64])
def test_consecutive_windows_add_up_to_the_whole_sequence(fx, s130, size):
    F = fx
    cases = [(s130["ref"], s130["sites"])]
    if size > 1:
        r = F["ref_of"]["r"]
        cases.append((r, random_sites(np.random.default_rng(size), cytosines(F["seqs"], F["runs"], r), r, 0.5)))
    for ref, sites in cases:
        n = len(F["seqs"][ref])
        parts = [device(F, ref, beg, min(n, beg + size), [s for s in sites if beg <= s[1] < beg + size], 7) for beg in range(0, n, size)]
        assert b"".join(parts) == want(F, ref, 0, n, sites, 7), (ref, size)


def test_runs_may_be_cut_to_those_near_the_window(fx):
    """what the driver does: only the runs that reach into [beg - 2, end + 2) travel with a window"""
    F = fx
    r = F["ref_of"]["r"]
    rs = F["runs"][r]
    for beg, end in ((0, 1000), (1000, 2000), (2000, 3000), (1, 2999)):
        near = [(b, e) for b, e in rs if e > beg - 2 and b < end + 2]
        assert device(F, r, beg, end, [], 7, near) == want(F, r, beg, end, [], 7)
    assert device(F, r, 0, 3000, [], 7, None) != want(F, r, 0, 3000, [], 7)              # (without them the runs' cytosines are there)


# ---- 4. the cap protocol -------------------------------------------------------------------------------------------------------------------------
def _raw_call(F, ref, beg, end, sites, contexts, cap, guard=64):
    from bitmapperbs_amd import capi
    m = F["m"]
    m._set_refs()
    st = as_array(sites)
    rn = np.ascontiguousarray(F["runs"][ref], dtype=np.int64).reshape(-1, 2)
    out = np.full(cap + guard, 0xAA, dtype=np.uint8)
    used = ctypes.c_uint64(12345); lines = ctypes.c_int64(12345)
    rc = m._lib.bmbs_methyl_report(m._ctx, ref, beg, end, capi.ptr(st) if st.size else None, st.size, capi.ptr(rn) if rn.size else None, rn.shape[0], contexts,
                                   capi.ptr(out), cap, ctypes.byref(used), ctypes.byref(lines))
    return rc, used.value, lines.value, out


def test_the_cap_protocol(fx):
    F = fx
    r = F["ref_of"]["r"]
    sites = random_sites(np.random.default_rng(4), cytosines(F["seqs"], F["runs"], r), r, 0.5)
    text = want(F, r, 0, 3000, sites, 7)
    n_lines = text.count(b"\n")
    assert len(text) > 10000
    for cap in (0, len(text) - 1):
        rc, used, lines, out = _raw_call(F, r, 0, 3000, sites, 7, cap)
        assert (rc, used, lines) == (ENOMEM, len(text), n_lines)
        assert (out == 0xAA).all()                                                    # nothing is written when the text does not fit
    rc, used, lines, out = _raw_call(F, r, 0, 3000, sites, 7, len(text))
    assert (rc, used, lines) == (0, len(text), n_lines)
    assert out[:len(text)].tobytes() == text and (out[len(text):] == 0xAA).all() and out.size == len(text) + 64
    # a larger buffer: nothing behind the text either; an empty window: 0 bytes, and NULL will do
    rc, used, lines, out = _raw_call(F, r, 0, 3000, sites, 7, len(text) + 1000)
    assert (rc, used, lines) == (0, len(text), n_lines) and (out[len(text):] == 0xAA).all()
    for beg in (0, 17, 3000):
        rc, used, lines, out = _raw_call(F, r, beg, beg, [], 7, 0, guard=64)
        assert (rc, used, lines) == (0, 0, 0) and (out == 0xAA).all()
    assert device(F, r, 5, 5, [], 7) == b""


# ---- 5. the LDS fall-back --------------------------------------------------------------------------------------------------------------------------
def test_a_block_whose_text_does_not_fit_its_lds_image(fx):
    """k_cyt_emit formats a block's text -- that of CYT_WPB = 64 consecutive genome words, 2048 positions -- into an LDS image of CYT_LDS =
    49 152 bytes, and writes straight to memory when the text is longer.  Here: the sequence of 4000 C under the name of 200 characters,
    every cytosine with ten-digit counts.  Every C at p <= 3997 is a CHH, so 3998 lines; a line is 200 (name) + 11 (six tabs, strand,
    three letters, newline) + 3 (CHH) + 10 + 10 (counts) + at least 1 (position) = at least 235 bytes.  The sequence's positions lie in
    at most ceil((4000 + 31) / 32) = 126 genome words, that is in two blocks; the first block holds at least 2048 - 31 = 2017 of the
    positions, the second what is left of 3998, at least 3998 - 2048 = 1950: at least 1950 * 235 = 458 250 bytes each, nine times the
    image.  No block of this call can take the LDS path.  (Every other test here stays below the image size in most of its blocks: the
    3000 random bases give about 1500 lines of about 20 bytes.)"""
    F = fx
    ref = F["ref_of"][LONG_NAME]
    assert len(F["names"][ref]) == 200 and F["seqs"][ref] == bytes([spec.C]) * 4000
    cyt = cytosines(F["seqs"], F["runs"], ref)
    assert len(cyt) == 3998 and {k for _p, k in cyt} == {2}
    rng = np.random.default_rng(5)
    sites = [(ref, p, int(rng.integers(10 ** 9, 2 ** 32)), int(rng.integers(10 ** 9, 2 ** 32)), k) for p, k in cyt]
    text = want(F, ref, 0, 4000, sites, 7)
    assert min(len(l) + 1 for l in text.split(b"\n")[:-1]) >= 235 and 1950 * 235 > CYT_LDS
    assert device(F, ref, 0, 4000, sites, 7) == text
    # ... and a window of it that begins and ends inside a word, with one line in four taken away
    sites = [s[:4] + (s[4] | (cs.REPORT_OMIT if i % 4 == 0 else 0),) for i, s in enumerate(sites)]
    assert device(F, ref, 17, 3990, [s for s in sites if 17 <= s[1] < 3990], 4) == want(F, ref, 17, 3990, [s for s in sites if 17 <= s[1] < 3990], 4)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_first_offender(fx):
    F = fx
    r = F["ref_of"]["r"]
    cyt = cytosines(F["seqs"], F["runs"], r)
    good = [(r, p, 1, 2, k) for p, k in cyt]
    assert len(good) > 1000
    rs = F["runs"][r]

    def refused(what, sites=(), ref=r, beg=0, end=3000, contexts=7, runs="own"):
        with pytest.raises(RuntimeError, match=r"bmbs error -22: methyl report: .*" + what):
            device(F, ref, beg, end, list(sites), contexts, runs)

    refused("ref %d is outside" % len(F["seqs"]), ref=len(F["seqs"]))
    refused("ref -1 is outside", ref=-1)
    refused(r"window \[-1, 10\)", beg=-1, end=10)
    refused(r"window \[11, 10\)", beg=11, end=10)
    refused(r"window \[0, 3001\)", end=3001)
    refused("contexts 0", contexts=0)
    refused("contexts 8", contexts=8)
    refused("run 1 ", runs=[(5, 9), (2, 3)])
    refused("run 1 ", runs=[(5, 9), (8, 12)])
    refused("run 0 ", runs=[(5, 5)])
    # sites: the offender sits behind 700 good ones; a later offender of another kind does not hide it
    i = next(j for j in range(700, len(cyt)) if any(F["seqs"][r][q] in (spec.A, spec.T) for q in range(cyt[j][0] + 1, cyt[j + 1][0])))
    def with_(j, s):
        return good[:j] + [s] + good[j + 1:]
    p, k = cyt[i]
    site_i, site_i1 = "site %d " % i, "site %d " % (i + 1)
    refused(site_i + "has another ref", with_(i, (r + 1, p, 1, 2, k)))
    refused("site 0 lies outside the window", good[i:], beg=p + 1)
    refused("site %d lies outside the window" % i, good[:i + 1], end=p)
    refused(site_i1 + "does not sit at a larger pos", good[:i + 1] + [good[i]] + good[i + 1:])
    refused(site_i1 + "does not sit at a larger pos", good[:i] + [good[i + 1], good[i]] + good[i + 2:])
    refused(site_i + "has a kind that is not what the genome says", with_(i, (r, p, 1, 2, k ^ 4)))
    refused(site_i + "has a kind that is not what the genome says", with_(i, (r, p, 1, 2, (k + 1) % 3 | k & 4)))
    refused(site_i + "has a kind that is not what the genome says", with_(i, (r, p, 1, 2, k | 16)))
    no_c = next(q for q in range(p + 1, cyt[i + 1][0]) if F["seqs"][r][q] in (spec.A, spec.T))
    refused(site_i1 + "has a kind that is not what the genome says", good[:i + 1] + [(r, no_c, 1, 2, 0)] + good[i + 1:])
    refused(site_i + "has a kind that is not what the genome says", with_(i, (r, p, 1, 2, k ^ 4)) [:900] + [(r + 1, 2990, 0, 0, 0)])
    late = [s for j, s in enumerate(good) if j >= 100 or s[4] & 3 != 2]                   # no CHH site among the first hundred cytosines
    other = next(j for j, s in enumerate(late) if s[4] & 3 == 2)
    assert other > 50
    refused("site %d is of a context that is not selected" % other, late, contexts=3)
    # a site whose window touches a run: a cytosine the runs took away, put back
    gone = [(q, kk) for q, kk in cytosines(F["seqs"], None, r) if (q, kk) not in set(cyt)]
    assert len(gone) > 20
    q, kk = gone[len(gone) // 2]
    j = sum(1 for s in good if s[1] < q)
    refused("site %d has a window that touches a run" % j, good[:j] + [(r, q, 1, 2, kk)] + good[j:])
    assert device(F, r, 0, 3000, good, 7) == want(F, r, 0, 3000, good, 7)                 # (the good ones alone are fine)


def test_without_an_index_the_call_is_refused(fx):
    from bitmapperbs_amd import mapper
    m = mapper.Mapper(None, 0)
    used = ctypes.c_uint64(0); lines = ctypes.c_int64(0)
    assert m._lib.bmbs_methyl_report(m._ctx, 0, 0, 0, None, 0, None, 0, 1, None, 0, ctypes.byref(used), ctypes.byref(lines)) == ESTATE
    assert b"no index attached" in m._lib.bmbs_last_error(m._ctx)
    m.close()


# ---- 7., 8. the golden genome; the methylation result stays ---------------------------------------------------------------------------------------
def test_the_golden_genome_whole_with_20000_sites(gold, mapper_on_gold):
    rng = np.random.default_rng(20000)
    seqs, names = gold["seqs"], gold["names"]
    cyt = [(ref, p, k) for ref in range(len(seqs)) for p, k in cytosines(seqs, None, ref)]
    pick = sorted(rng.choice(len(cyt), 20000, replace=False).tolist())
    sites = [(cyt[i][0], cyt[i][1], int(rng.choice(COUNTS)), int(rng.choice(COUNTS)), cyt[i][2] | (cs.REPORT_OMIT if rng.random() < 0.1 else 0)) for i in pick]
    got = b"".join(mapper_on_gold.methyl_report(ref, 0, len(seqs[ref]), as_array([s for s in sites if s[0] == ref]), None, 7) for ref in range(len(seqs)))
    assert got == cs.report_all(seqs, names, None, sites, 7)
    assert got.count(b"\n") == len(cyt) - sum(1 for s in sites if s[4] & cs.REPORT_OMIT) and len(cyt) > 100000


def test_a_report_leaves_the_methylation_result_alone(gold, mapper_on_gold):
    m = mapper_on_gold
    rng = np.random.default_rng(8)
    recs = [tm._random_record(rng, gold["seqs"]) for _ in range(2000)]
    before = m.bam_methyl(b"".join(recs), [len(r) for r in recs], None, contexts=7, mbias=True).copy()
    table = m.methyl_mbias().copy()
    assert len(before) > 1000
    sites = [s for s in tm._site_tuples(before) if s[0] == 0]
    text = m.methyl_report(0, 0, len(gold["seqs"][0]), as_array(sites), None, 7)
    assert text == cs.report(gold["seqs"], gold["names"], None, sites, 7, 0, 0, len(gold["seqs"][0]))
    assert m.methyl_sites().tobytes() == before.tobytes() and m.methyl_mbias().tobytes() == table.tobytes()
    opp = m.bam_methyl_opposite(b"".join(recs), [len(r) for r in recs], None, contexts=7).copy()
    m.methyl_report(1, 100, 5000, [], None, 1)
    assert m.methyl_opposite().tobytes() == opp.tobytes() and len(opp) > 100


# ---- the driver -------------------------------------------------------------------------------------------------------------------------------------
REPORT = ".cytosine_report.txt"


def _side_files(pre, bam):
    return [open(bam, "rb").read(), open(bam + ".bai", "rb").read(), open(pre + "_mbias.tsv", "rb").read()] + tm._files(pre)


def _bedgraph_sites(files):
    """(name, pos) of every line of the three bedGraphs"""
    out = set()
    for f in files:
        for line in f.decode().split("\n")[1:-1]:
            c, p = line.split("\t")[:2]
            out.add((c, int(p)))
    return out


@pytest.mark.parametrize("window", [None, 64, 1000])
@pytest.mark.parametrize("kind", ["se", "pe"])
def test_driver_report_equals_the_spec_whatever_the_window(gold, plain_runs, kind, window):
    """the file = cytosine_spec applied to methyl_spec's sites of the BAM's own records, with the default window and with windows of 64
    and 1000 bases; BAM, .bai, bedGraphs and M-bias table are the bytes of the run without the option.  The run with 1000 has
    --methyl-merge-context and --methyl-min-depth 3 too: they shape the bedGraphs, not the report"""
    P = plain_runs(kind)
    pre, bam = P["pre"], P["bam"]
    want_text = cs.report_all(gold["seqs"], gold["names"], None, P["sites"], 7)
    more = [] if window is None else ["--methyl-report-window", str(window)] + (tv.MERGE_ARGS + tv.DEPTH_ARGS if window == 1000 else [])
    if os.path.exists(pre + REPORT):
        os.unlink(pre + REPORT)
    err = tm._run(gold["fa"], P["R"]["inputs"], P["base"] + ["--cytosine-report"] + more, bam)
    assert open(pre + REPORT, "rb").read() == want_text
    if window == 1000:
        assert _side_files(pre, bam)[:3] == list(P["without"]) and tm._files(pre) != P["files"]
    else:
        assert _side_files(pre, bam) == list(P["without"]) + P["files"]
    m = re.search(r"report lines (\d+) bytes (\d+)", err)
    assert m and (int(m.group(1)), int(m.group(2))) == (want_text.count(b"\n"), len(want_text)), err
    if window is None:
        # the lines with calls are exactly the sites of the per-strand bedGraphs
        covered = set()
        for line in want_text.decode().split("\n")[:-1]:
            c, p, _s, me, un = line.split("\t")[:5]
            if int(me) + int(un):
                covered.add((c, int(p) - 1))
        assert covered == _bedgraph_sites(P["files"]) and len(covered) == len(P["sites"]) > 1000


@pytest.mark.parametrize("kind", ["se", "pe"])
def test_driver_report_with_the_variant_filter(gold, plain_runs, kind):
    """the sites the filter drops have no line; every other cytosine has one"""
    P = plain_runs(kind)
    pre, bam = P["pre"], P["bam"]
    left = tv.vs.drop_variants(P["sites"], P["opp"], *tv.FILTER)
    dropped = sorted(set(P["sites"]) - set(left))
    assert len(dropped) > 0
    marked = sorted(left + [s[:4] + (s[4] | cs.REPORT_OMIT,) for s in dropped])
    want_text = cs.report_all(gold["seqs"], gold["names"], None, marked, 7)
    tm._run(gold["fa"], P["R"]["inputs"], P["base"] + tv.FILTER_ARGS + ["--cytosine-report", "--methyl-report-window", "777"], bam)
    got = open(pre + REPORT, "rb").read()
    assert got == want_text
    assert got.count(b"\n") == cs.report_all(gold["seqs"], gold["names"], None, [], 7).count(b"\n") - len(dropped)
    for ref, p, _m, _u, _k in dropped:
        assert ("\n%s\t%d\t" % (gold["names"][ref], p + 1)).encode() not in b"\n" + got
    assert [open(bam, "rb").read(), open(bam + ".bai", "rb").read(), open(pre + "_mbias.tsv", "rb").read()] == list(P["without"])


def test_driver_report_on_a_genome_with_runs(tmp_path):
    """the genome of test_methyl's test_sites_at_bases_the_fasta_does_not_spell_are_left_out (runs of N of 1..60 bases and two other
    letters in both sequences), reads across the runs' borders: the report equals the spec on the sites the bedGraphs start from"""
    from bitmapperbs_amd import mapper
    rng = np.random.default_rng(3)
    seqs = ["".join("ACGT"[x] for x in rng.integers(0, 4, 6000)) for _ in range(2)]
    runs_in = [(300, 301), (700, 702), (1100, 1103), (1500, 1560), (2500, 2501), (3000, 3060), (4000, 4002)]
    mut = []
    for s in seqs:
        b = list(s)
        for lo, hi in runs_in:
            b[lo:hi] = "N" * (hi - lo)
        b[5000] = "R"; b[5003] = "n"
        mut.append("".join(b))
    fa = str(tmp_path / "n.fa")
    open(fa, "w").write("".join(">c%d some text\n%s\n" % (i, "\n".join(s[k:k + 70] for k in range(0, len(s), 70))) for i, s in enumerate(mut)))
    mapper.Index.build(fa, fa, threads=4)
    ix = mapper.Index(fa)
    held = spec.genome_of_pac(ctypes.string_at(ix.view.pac, int(ix.view.pac_bytes)), ix.chrom_len)
    n_runs = spec.non_acgt_runs(open(fa).read())
    reads = []
    for ref, s in enumerate(mut):
        for p in range(0, 5900, 37):
            seq = "".join("T" if c not in "ACGT" else ("C" if c == "C" and p % 2 else "T" if c == "C" else c) for c in s[p:p + 100].upper())
            reads.append("@r%d_%d_%d\n%s\n+\n%s\n" % (len(reads), ref, p, seq, "I" * 100))
    open(tmp_path / "r.fq", "w").write("".join(reads))
    pre = str(tmp_path / "m")
    for args, contexts in ((["--CHG", "--CpG"], 3),):
        tm._run(fa, ["--seq", str(tmp_path / "r.fq")], ["--sort", "--methyl", pre, "--cytosine-report", "--methyl-report-window", "500"] + args, pre + ".bam")
        recs = split_records(bam_payload(pre + ".bam")[1])
        sites = spec.drop_non_acgt(spec.sites(held, recs, None, contexts=contexts), n_runs)
        got = open(pre + REPORT, "rb").read()
        assert got == cs.report_all(held, ix.chrom_names, n_runs, sites, contexts)
        assert len(sites) > 300 and got.count(b"\n") > len(sites)
    ix.close()


def test_driver_refusals(gold, tmp_path):
    pre = str(tmp_path / "p")
    head = [tm._driver(), "--search", gold["fa"], "--seq", str(tmp_path / "none.fq"), "-o", str(tmp_path / "x.bam"), "--bam", "--sort"]
    needs = "--cytosine-report and --methyl-report-window need --methyl"
    cases = [(["--cytosine-report"], needs), (["--methyl-report-window", "64"], needs), (["--cytosine-report", "--methyl-report-window", "64"], needs),
             (["--methyl", pre, "--methyl-report-window", "64"], "--methyl-report-window needs --cytosine-report"),
             (["--methyl", pre, "--cytosine-report", "--methyl-report-window", "0"], "--methyl-report-window takes 1..2147483647"),
             (["--methyl", pre, "--cytosine-report", "--methyl-report-window", "64k"], "--methyl-report-window takes 1..2147483647"),
             (["--methyl", pre, "--cytosine-report", "--methyl-report-window"], "missing value")]
    for more, msg in cases:
        p = subprocess.run(head + more, capture_output=True, text=True)
        assert p.returncode == 2 and msg in p.stderr, (more, p.stderr)
    assert not os.path.exists(pre + REPORT)
    # --help says what the report is and that the two bedGraph options do not shape it
    p = subprocess.run([tm._driver(), "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and "--cytosine-report [--methyl-report-window bases]" in p.stdout and "the report stays per strand and includes depth 0" in p.stdout
