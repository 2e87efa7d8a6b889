"""The balanced outcome table (k_attach.hip: entry index = the first B bits of the code T -> 0, G -> 10, A -> 11 of the letters behind
a seed start, depth 16 .. 32 letters; the default of GRCh38-size texts, forced here with BMBS_TDEPTH=h32).

CPU: the index / depth function the seeding kernels use (bmbs_outcome_index) against a restatement in Python.
GPU: every mapping mode with the table against the oracle and against the same call without a table (BMBS_T20=0) and with the
ternary 21-mer table (BMBS_TDEPTH=21); the seeding stage on a genome whose T runs, G/A stretches and repeat families reach the
table's corners."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import orc
from common import GOLD

SETTINGS = (("BMBS_TDEPTH", "h32"), ("BMBS_T20", "0"), ("BMBS_TDEPTH", "21"))


# ---- the index / depth function ------------------------------------------------------------------------------------------------------
def restated(letters, n, bits):
    """index and depth of the seed start `letters` (a str; n = how many of them the seed has), or -1: the 16-mer path"""
    code, depth = "", 0
    for ch in letters[:32]:
        c = "0" if ch in "TC" else "10" if ch == "G" else "11"          # (a letter outside ACGT is packed like A)
        if len(code) + len(c) > bits:
            if len(code) < bits:
                code += "1"                                                # half a G/A code: belongs to no letter
            break
        code += c
        depth += 1
    index = int(code.ljust(bits, "0"), 2)
    if n < depth or any(ch not in "ACGT" for ch in letters[:depth]):
        return -1, depth
    return index, depth


def library(letters, n, bits):
    from bitmapperbs_amd import capi
    bases = bad = 0
    for j, ch in enumerate(letters[:32]):
        if ch in "ACGT":
            bases |= "ACGT".index(ch) << (2 * j)
        else:
            bad |= 1 << j
    d = C.c_int32(-1)
    idx = capi.lib().bmbs_outcome_index(bases, bad, n, bits, C.byref(d))
    return int(idx), int(d.value)


@pytest.mark.parametrize("bits", [32, 33])
def test_index_and_depth_match_the_restatement(bits):
    rng = np.random.default_rng(bits)
    cases = []
    for p in ((0.25, 0.25, 0.25, 0.25), (0.05, 0.45, 0.05, 0.45), (0.4, 0.1, 0.4, 0.1), (0.02, 0.49, 0.0, 0.49)):
        for _ in range(1500):
            cases.append(("".join("ACGT"[i] for i in rng.choice(4, 34, p=p)), int(rng.integers(16, 60))))
    cases += [("T" * 34, 34), ("C" * 34, 34), ("TC" * 17, 32), ("T" * 34, 31),                   # all T: depth 32, the bits behind stay 0
              ("GA" * 17, 34), ("G" * 34, 16), ("A" * 34, 17), ("A" * 34, 15)]                   # all G/A: depth 16 (B = 33: and half a code)
    for t in range(0, 34):                                                                        # the last bit straddled by G and by A
        for tail in ("G", "A", "T"):
            ga = (bits - 1 - t) // 2
            s = "T" * t + "GA" * (ga // 2) + "G" * (ga % 2) + tail
            cases.append(((s + "T" * 34)[:34], 40))
    for pos in range(0, 34):                                                                      # a letter outside ACGT at every position
        for base in ("T" * 34, "G" * 34, "TGACTTAG" * 5, "ACGT" * 9):
            s = base[:34]
            cases.append((s[:pos] + "N" + s[pos + 1:], 40))
    depths = set()
    for letters, n in cases:
        want = restated(letters, n, bits)
        got = library(letters, n, bits)
        assert got == want, (letters, n, bits, got, want)
        assert 16 <= got[1] <= 32 and got[0] < (1 << bits)
        depths.add(got[1])
    assert depths == set(range(16, 33))
    assert library("T" * 34, 40, 31)[0] == -2


# ---- the mapping modes ---------------------------------------------------------------------------------------------------------------
def _make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    """the 300 kb test genome and the 5 Mb repeat-rich one (tests/golden/make_golden.py), indexed on the device; the oracle's
    results are computed once per (genome, mode, length) and shared by the packed-row and the ASCII-row case"""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bitmapperbs_amd import synth, mapper
    mg = _make_golden()
    out = {}
    for name, (names, chroms) in (("small", mg.genome()), ("big", mg.big_genome())):
        fa = str(tmp_path_factory.mktemp(name) / "g.fa")
        synth.write_fasta(fa, names, chroms)
        mapper.Index.build(fa, fa, threads=8, device=0)
        out[name] = dict(chroms=chroms, ix=mapper.Index(fa), oix=orc.OrcIndex(fa), cache={})
    return out


def _spoil(seq, rng, L):
    """letters outside ACGT at positions 16 .. 33 behind the first seed start of every third read, and a few anywhere"""
    n = seq.shape[0]
    rows = np.arange(0, n, 3)
    cols = 16 + (rows // 3) % 18
    keep = cols < L
    seq[rows[keep], cols[keep]] = np.frombuffer(b"NRNY", dtype=np.uint8)[(rows[keep] // 3) % 4]
    pos = rng.random(seq.shape) < 0.002
    seq[pos] = ord("N")


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["packed", "ascii"])               # ascii = BMBS_LEGACY=1
@pytest.mark.parametrize("L", [40, 150, 251])                       # 40: seeds that end with fewer letters than the table is deep
@pytest.mark.parametrize("mode", ["se", "pe", "pe_sensitive"])
@pytest.mark.parametrize("genome", ["small", "big"])
def test_mapping_with_the_balanced_table(genomes, monkeypatch, genome, mode, L, rows):
    from bitmapperbs_amd import synth, mapper
    from test_gpu_parity import compare_records, compare_pe
    g = genomes[genome]
    sens = 1 if mode == "pe_sensitive" else 0
    prm = dict(e_f=0.08) if mode == "se" else dict(e_f=0.08, sensitive=sens, max_ins=max(500, 2 * L + 50))
    key = (mode, L)
    if key not in g["cache"]:
        rng = np.random.default_rng(1000 + L)
        if mode == "se":
            r = synth.make_reads_se(g["chroms"], n=3000, L=L, seed=500 + L, sub=0.03, indel=0.002, qual="random")
            _spoil(r["seq"], rng, L)
            inp = (r["seq"], r["qual"])
            want = g["oix"].map_se(orc.params(**prm), r["seq"], r["qual"], L)
        else:
            m1, m2 = synth.make_reads_pe(g["chroms"], n=2000, L=L, seed=600 + L + sens, sub=0.05 if sens else 0.02, indel=0.002, qual="random",
                                         ins_hi=max(500, 2 * L + 50))
            _spoil(m1["seq"], rng, L); _spoil(m2["seq"], rng, L)
            inp = (m1["seq"], m1["qual"], m2["seq"], m2["qual"])
            want = g["oix"].map_pe(orc.params(**prm), *inp, L)
        for a in inp:
            a.setflags(write=False)
        g["cache"][key] = (inp, want)
    inp, (recs, ost, ocnt) = g["cache"][key]
    if rows == "ascii":
        monkeypatch.setenv("BMBS_LEGACY", "1")
    got = []
    for name, val in SETTINGS:
        monkeypatch.delenv("BMBS_TDEPTH", raising=False); monkeypatch.delenv("BMBS_T20", raising=False)
        monkeypatch.setenv(name, val)
        m = mapper.Mapper(g["ix"], 0, **prm)
        res, pool = m.map_se(*inp, L) if mode == "se" else m.map_pe(*inp, L)
        cnt = m.counters()
        got.append((res.tobytes(), pool.tobytes(), m.stats().tolist(), cnt["n_hash"], cnt["n_ext"]))
        if val == "h32":
            assert not (compare_records(res, pool, recs, L) if mode == "se" else compare_pe(res, pool, recs, L))
            assert (m.stats() == ost).all()
            if mode == "se":
                assert cnt["n_hash"] == ocnt["n_hash"]
        m.close()
    assert got[0][:4] == got[1][:4] and got[0][:4] == got[2][:4]
    assert got[0][4] <= got[1][4]                                   # the table only ever saves extensions


# ---- the seeding stage on a genome that reaches the table's corners ---------------------------------------------------------------------
def corner_genome():
    """two chromosomes of 0.5 Mb with T / C runs of 40 .. 200 bases (their reverse strand: G / A runs), G/A-only stretches and families
    of near-identical copies, and a third that is one T / C run of 1.15 Mb: a T-only pattern of any length has more than 2^20
    occurrences, which do not fit the entry's hits field (tag 14, the 16-mer path)"""
    from bitmapperbs_amd import synth
    names, chroms = synth.make_genome(1_000_000, 2, seed=611)
    names, chroms = list(names), list(chroms)
    rng = np.random.default_rng(612)

    def plant(e):
        ch = chroms[rng.integers(0, len(chroms))]
        p = int(rng.integers(0, ch.size - e.size))
        ch[p:p + e.size] = e if rng.random() < 0.5 else synth.revcomp(e)
        return ch, p

    tc, ga = np.frombuffer(b"TC", dtype=np.uint8), np.frombuffer(b"GA", dtype=np.uint8)
    for _ in range(300):
        plant(tc[rng.integers(0, 2, int(rng.integers(40, 201)))])
    for _ in range(300):
        plant(ga[rng.integers(0, 2, int(rng.integers(40, 201)))])
    for (elen, copies, div) in [(600, 120, 0.01), (1500, 40, 0.004), (300, 200, 0.03), (2000, 30, 0.0)]:
        el = synth._ACGT[rng.integers(0, 4, elen)]
        for _ in range(copies):
            e = el.copy(); mm = rng.random(elen) < div
            e[mm] = synth._ACGT[rng.integers(0, 4, int(mm.sum()))]
            plant(e)
    return names + ["tc_run"], chroms + [tc[rng.integers(0, 2, 1_150_000)]]


@pytest.mark.gpu
def test_seed_stage_on_t_runs_ga_stretches_and_families(tmp_path, monkeypatch):
    """bmbs_seed_batch: verdicts, exit sites and vote lists are the same bytes under the three table settings and equal the
    oracle's; n_hash equals the oracle's.  (n_ext and n_sa count the steps and locates really taken: the tables exist to lower
    them, so they are compared as <= the table-less run's.)"""
    from bitmapperbs_amd import synth, mapper
    names, chroms = corner_genome()
    fa = str(tmp_path / "g.fa")
    synth.write_fasta(fa, names, chroms)
    mapper.Index.build(fa, fa, threads=8, device=0)
    ix = mapper.Index(fa); oix = orc.OrcIndex(fa)
    L = 150
    r = synth.make_reads_se(chroms[:2], n=18000, L=L, seed=613, sub=0.02, indel=0.001, qual="const", n_rate=0.001)
    r2 = synth.make_reads_se(chroms[2:], n=2000, L=L, seed=614, sub=0.02, indel=0.001, qual="const")
    r = dict(seq=np.concatenate([r["seq"], r2["seq"]]), qual=np.concatenate([r["qual"], r2["qual"]]))
    # the table's corners must really occur among the first seed starts: depth 32 (T / C only), depth 16 (G / A only)
    first32 = r["seq"][:, :32]
    assert (np.isin(first32, np.frombuffer(b"TC", dtype=np.uint8)).all(axis=1)).sum() > 20
    assert (np.isin(first32[:, :17], np.frombuffer(b"GA", dtype=np.uint8)).all(axis=1)).sum() > 20
    recs, ovs, ovc, ovo = oix.map_se_votes(orc.params(e_f=0.08), r["seq"], r["qual"], L)
    _, _, ocnt = oix.map_se(orc.params(e_f=0.08), r["seq"], r["qual"], L)
    got = []
    for name, val in SETTINGS:
        monkeypatch.delenv("BMBS_TDEPTH", raising=False); monkeypatch.delenv("BMBS_T20", raising=False)
        monkeypatch.setenv(name, val)
        m = mapper.Mapper(ix, 0, e_f=0.08)
        s = m.seed(r["seq"], L, vote_cap=4096 * 1024)
        cnt = m.counters()
        m.close()
        got.append((tuple(s[k].tobytes() for k in ("verdict", "exit_site", "seg_off", "n_votes", "vote_site", "vote_cnt")), cnt))
        assert cnt["n_hash"] == ocnt["n_hash"], (val, cnt["n_hash"], ocnt["n_hash"])
        if val != "h32":
            continue
        v = s["verdict"].astype(np.int64); op = recs["path"].astype(np.int64)
        gen = (op == 3) | ((op == 0) & (recs["n_cand"] > 0))
        assert (v[op == 1] == 1).all() and (v[op == 2] == 2).all() and (v[op == 4] == 4).all() and (v[gen] == 3).all()
        assert (s["n_votes"][gen].astype(np.int64) == recs["n_votes"][gen]).all()
        for i in np.nonzero(gen)[0]:
            a = int(s["seg_off"][i]); nv = int(s["n_votes"][i]); oa, ob = int(ovo[i]), int(ovo[i + 1])
            assert ob - oa == nv, i
            assert (s["vote_site"][a:a + nv] == ovs[oa:ob]).all() and (s["vote_cnt"][a:a + nv] == ovc[oa:ob]).all(), i
        assert gen.sum() > 500
    assert got[0][0] == got[1][0] and got[0][0] == got[2][0]
    h32, off = got[0][1], got[1][1]
    assert h32["n_ext"] < off["n_ext"] and h32["n_sa"] <= off["n_sa"], (h32, off)
