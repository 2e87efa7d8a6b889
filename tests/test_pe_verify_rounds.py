"""The two verification rounds of paired-end fast mode with per-pair counts from the kernels before them, a scan that writes the work
list and one compaction lane per pair (BMBS_PE_ROUNDS=1, the default; verify_round_pairs in bmbs_api.hip, k_scan_expand in k_scan.hip)
against the form that counts, scans and scatters over all 2n reads (BMBS_PE_ROUNDS=0) and the oracle.

Every case maps the same pairs under both settings and asserts that records, CIGAR pool, stats() and counters() are the same, and that
the new form equals the oracle (orc.OrcIndex.map_pe).  The cases aim at what the new form adds: which kernel writes a pair's count
(k_pe_filter_pairs, lane 0 or the serial loop of k_pe_filter_pairs_long, the lane or the wave of k_pe_prune), which mate of a pair a
round takes, the scan's tile of 256 threads x 8 pairs, lists of more than 64 entries, and the launch sequence around the rounds."""
import re

import numpy as np
import pytest

import orc
from test_vote_dense import (ELEN, _clean_pairs, _compose, _freeze, _index, _layout, _other_letter, _pairs_from, _spoil_n,    # noqa: F401
                             block_pairs, families, family_genome, genomes)

FORMS = ("1", "0")


def both_rounds(monkeypatch, g, prm, batches, L, env=None, want_retries=False, want_same_stages=False):
    """maps `batches` (a list of (inp, oracle result); one context per setting, the calls in order) under BMBS_PE_ROUNDS=1 and =0: the
    same records, pool, stats() and counters() from both, the new form equal to the oracle.  -> the counters"""
    from bitmapperbs_amd import mapper
    from test_gpu_parity import compare_pe
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    got, cnts, stages = [], [], []
    for form in FORMS:
        monkeypatch.setenv("BMBS_PE_ROUNDS", form)
        m = mapper.Mapper(g["ix"], 0, **prm)
        out = []
        tot = np.zeros(5, dtype=np.int64)
        for inp, (recs, ost, _) in batches:
            res, pool = m.map_pe(*inp, L)
            tot += ost
            if form == "1":
                bad = compare_pe(res, pool, recs, L)
                assert not bad, bad[:5]
                assert (m.stats() == tot).all(), (m.stats(), tot)
            out.append((res.tobytes(), pool.tobytes(), m.stats().tolist()))
        if want_retries:
            assert m.retries() > 0
        cnts.append(m.counters())
        stages.append([name for name, _ in m.profile()])
        m.close()
        got.append(out)
    assert got[0] == got[1]
    assert cnts[0] == cnts[1], {k: (cnts[0][k], cnts[1].get(k)) for k in cnts[0] if cnts[0][k] != cnts[1].get(k)}
    if want_same_stages:
        assert stages[0] == stages[1]
    return cnts[0]


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L", [150, 251])
@pytest.mark.parametrize("genome", ["small", "big"])
def test_parity_with_rounds_over_all_reads_and_oracle(genomes, monkeypatch, genome, L):
    from bitmapperbs_amd import synth
    g = genomes[genome]
    prm = dict(e_f=0.08, max_ins=max(500, 2 * L + 50))
    m1, m2 = synth.make_reads_pe(g["chroms"], n=2000, L=L, seed=1200 + L, sub=0.02 + 0.01 * (L == 251), indel=0.002, qual="random",
                                 ins_hi=max(500, 2 * L + 50))
    rng = np.random.default_rng(79 + L)
    _spoil_n(m1["seq"], rng); _spoil_n(m2["seq"], rng)
    inp = _freeze((m1["seq"], m1["qual"], m2["seq"], m2["qual"]))
    want = g["oix"].map_pe(orc.params(**prm), *inp, L)
    cnt = both_rounds(monkeypatch, g, prm, [(inp, want)], L)
    assert cnt["n_filter"] > 0


# ---- 2. the classes of pairs in one block ------------------------------------------------------------------------------------------------
def _chrom_of(names):
    return np.array([int(re.match(rb"p\d+_chr(\d+)_", nm).group(1)) for nm in names])


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["front", "back", "strided"])
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 256])
def test_pair_classes_in_one_block(block_pairs, monkeypatch, count, where):
    """256 pairs, `count` of them with both mates spoiled (both verified: round 1 takes one mate, round 2 the other); of the others
    every fourth has mate 1 alone spoiled (one-sided: round 1 only), every fourth both mates spoiled and mate 2 taken from a pair of
    another chromosome (no partner: dead), the rest are clean (settled before the rounds)"""
    from bitmapperbs_amd import synth
    g, clean, spoiled, q1, q2 = block_pairs
    both = _layout(count, where)
    rest = np.setdiff1d(np.arange(256), both)
    one_sided, dead = rest[0::4], rest[1::4]
    h1 = np.concatenate([both, one_sided, dead]).astype(np.int64)
    h2 = np.concatenate([both, dead]).astype(np.int64)
    s1, s2 = _compose(clean, spoiled, h1, h2)
    # the pairs' chromosomes, from the names make_reads_pe gives them (the same call as _clean_pairs makes)
    m1, _ = synth.make_reads_pe(g["chroms"], n=256, L=150, seed=4242, sub=0.0, indel=0.0, qual="const")
    chrom = _chrom_of([nm[:-2] for nm in m1["names"]])
    assert (chrom == 1).any() and (chrom == 2).any()
    for p in dead:
        other = np.nonzero(chrom != chrom[p])[0]
        s2[p] = spoiled[1][other[p % other.size]]
    inp = _freeze((s1, q1, s2, q2))
    prm = dict(e_f=0.08)
    want = g["oix"].map_pe(orc.params(**prm), *inp, 150)
    cnt = both_rounds(monkeypatch, g, prm, [(inp, want)], 150)
    assert (cnt["n_filter"] > 0) == (count > 0 or one_sided.size > 0)


# ---- 3. sizes around the scan's tile (256 threads x 8 pairs) ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 31, 33, 63, 65, 2047, 2048, 2049, 4097])
def test_sizes_around_the_scan_tile(genomes, monkeypatch, n):
    """the last pair and every third one have lists: mate 1 of all of those, mate 2 of every second of them (one-sided and both)"""
    g = genomes["small"]
    clean, spoiled, q1, q2 = _clean_pairs(g, n, 7000 + n)
    h1 = np.union1d(np.arange(0, n, 3), [n - 1])
    h2 = np.union1d(np.arange(0, n, 6), [n - 1])
    s1, s2 = _compose(clean, spoiled, h1, h2)
    inp = _freeze((s1, q1, s2, q2))
    prm = dict(e_f=0.08)
    want = g["oix"].map_pe(orc.params(**prm), *inp, 150)
    both_rounds(monkeypatch, g, prm, [(inp, want)], 150)


# ---- 4. / 5. long lists, and the rule that depends on the order of discovery ------------------------------------------------------------------
def _family_pairs(g, L, seed):
    """pairs from the four-letter elements of every copy count, two substitutions per mate (verdict 3: lists of every class, the 300
    copies past the 64 entries a lane walks alone); per element a third of the pairs as they are (the two filtered lists are equally
    long: a tie), a third with a base inserted into mate 1 (its seeds vote for two sites per copy: mate 2's list is the shorter one and
    is verified first), a third with the base inserted into mate 2"""
    rng = np.random.default_rng(seed)
    s1s, s2s = [], []
    for (kind, copies), e in g["els"].items():
        if kind != "acgt":
            continue
        s1, s2 = _pairs_from(e, 12, L, rng)
        for s in (s1, s2):
            for p in (L // 3, 2 * L // 3):
                s[:, p] = _other_letter(s[:, p])
        for s, rows in ((s1, slice(4, 8)), (s2, slice(8, 12))):
            at = L // 2
            s[rows, at + 1:] = s[rows, at:-1].copy()
            s[rows, at] = _other_letter(s[rows, at + 1])
        s1s.append(s1); s2s.append(s2)
    s1 = np.concatenate(s1s); s2 = np.concatenate(s2s)
    q = np.full_like(s1, ord("I"))
    return _freeze((s1, q, s2, q.copy()))


@pytest.mark.gpu
@pytest.mark.parametrize("L", [150, 251])
def test_long_lists(families, monkeypatch, L):
    g = families
    inp = _family_pairs(g, L, 913 + L)
    prm = dict(e_f=0.08, max_ins=ELEN + 50)
    want = g["oix"].map_pe(orc.params(**prm), *inp, L)
    cnt = both_rounds(monkeypatch, g, prm, [(inp, want)], L)
    assert cnt["n_cand_big"] > 0 and cnt["n_filter"] > 64 and cnt["n_pef_entries"] > 0


@pytest.mark.gpu
def test_order_dependent_rule_on_the_long_list_kernel(families, monkeypatch):
    """BMBS_PEF_LONG=2 hands every pair of more than 24 entries to k_pe_filter_pairs_long; a minimum insert above read + 2k (150 + 24)
    makes the lower distance bound positive, where lane 0 runs the reference's loop (pe_filter_serial) and writes the pair's count"""
    g = families
    L = 150
    inp = _family_pairs(g, L, 931)
    prm = dict(e_f=0.08, min_ins=200, max_ins=ELEN + 50)
    want = g["oix"].map_pe(orc.params(**prm), *inp, L)
    cnt = both_rounds(monkeypatch, g, prm, [(inp, want)], L, env={"BMBS_PEF_LONG": "2"})
    assert cnt["n_filter"] > 0


# ---- 6. the start of the text ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def start_genome(tmp_path_factory):
    """the family genome with one more copy of the 300-copy four-letter element at the very start of the first chromosome"""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    names, chroms, els = family_genome()
    chroms[0][:ELEN] = els[("acgt", 300)]
    g = _index(tmp_path_factory, "start", names, chroms)
    g["els"] = els
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("min_ins", [0, 200])
def test_mates_at_the_start_of_the_text(start_genome, monkeypatch, min_ins):
    """mate 1 begins 0 .. 14 bases (k = 12) into the element whose first copy opens the text: of its 300 and more sites the one of that
    copy lies below zero, and the pair takes the serial loops (k_pe_filter_pairs_long, k_pe_prune) whatever the distance bounds"""
    from bitmapperbs_amd import synth
    g = start_genome
    L = 150
    e = g["els"][("acgt", 300)]
    a = np.repeat(np.arange(15), 2)
    ins = np.where(np.arange(a.size) % 2 == 0, 300, 420)
    s1 = np.stack([e[x:x + L] for x in a])
    s2 = np.stack([synth.revcomp(e[x + i - L:x + i]) for x, i in zip(a, ins)])
    for s in (s1, s2):
        for p in (L // 3, 2 * L // 3):
            s[:, p] = _other_letter(s[:, p])
    q = np.full_like(s1, ord("I"))
    inp = _freeze((s1, q, s2, q.copy()))
    prm = dict(e_f=0.08, min_ins=min_ins, max_ins=ELEN + 50)
    want = g["oix"].map_pe(orc.params(**prm), *inp, L)
    for pef in ("1", "2"):
        cnt = both_rounds(monkeypatch, g, prm, [(inp, want)], L, env={"BMBS_PEF_LONG": pef})
        assert cnt["n_filter"] > 64


# ---- 7. the launch sequence around the rounds ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_capacity_guard_repeats_the_call(genomes, monkeypatch):
    """the first call of a fresh context waits for its counts (exact); BMBS_CAP_SCALE shrinks the learned capacities, so the later
    calls' candidates do not fit and the calls run again with exact sizes -- on two lanes, under both settings"""
    from bitmapperbs_amd import synth
    g = genomes["small"]
    batches = []
    for seed, sub in [(711, 0.005), (712, 0.05), (713, 0.06)]:
        m1, m2 = synth.make_reads_pe(g["chroms"], n=9000, L=100, seed=seed, sub=sub, indel=0.002, qual="random")
        inp = _freeze((m1["seq"], m1["qual"], m2["seq"], m2["qual"]))
        batches.append((inp, g["oix"].map_pe(orc.params(), *inp, 100)))
    both_rounds(monkeypatch, g, {}, batches, 100, env={"BMBS_CAP_SCALE": "0.02", "BMBS_LANES": "2", "BMBS_SPLIT_MIN": "3000"}, want_retries=True)


@pytest.mark.gpu
def test_chunks_on_three_lanes(genomes, monkeypatch):
    """2000 pairs as five chunks of 400 dealt to three lanes"""
    from bitmapperbs_amd import synth
    g = genomes["big"]
    m1, m2 = synth.make_reads_pe(g["chroms"], n=2000, L=150, seed=721, sub=0.03, indel=0.002, qual="random")
    inp = _freeze((m1["seq"], m1["qual"], m2["seq"], m2["qual"]))
    want = g["oix"].map_pe(orc.params(e_f=0.08), *inp, 150)
    both_rounds(monkeypatch, g, dict(e_f=0.08), [(inp, want)], 150, env={"BMBS_LANES": "3", "BMBS_SPLIT_MIN": "200", "BMBS_CHUNK": "400"})


# ---- 8. --sensitive is not touched -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sensitive_runs_the_same_kernels_under_both_settings(genomes, monkeypatch):
    from bitmapperbs_amd import synth
    g = genomes["big"]
    prm = dict(e_f=0.08, sensitive=1, max_ins=500)
    m1, m2 = synth.make_reads_pe(g["chroms"], n=2000, L=150, seed=731, sub=0.05, indel=0.002, qual="random", ins_hi=500)
    inp = _freeze((m1["seq"], m1["qual"], m2["seq"], m2["qual"]))
    want = g["oix"].map_pe(orc.params(**prm), *inp, 150)
    both_rounds(monkeypatch, g, prm, [(inp, want)], 150, want_same_stages=True)
