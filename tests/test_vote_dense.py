"""The paired-end vote stage on block-compacted lanes (k_vote_pe_dense, k_pe_fast.hip; BMBS_VOTE_DENSE=1, the default) against the
one-lane-per-read form (BMBS_VOTE_DENSE=0) and the oracle.

Every case maps the same pairs under both settings and asserts that records, CIGAR pool and stats() are the same bytes, and that the
dense form equals the oracle (orc.OrcIndex.map_pe).  The cases aim at what the compaction adds: the number of reads with lists in a
block (none, one, a wave's worth +- 1, all), where in the block they sit, blocks that the batch does not fill, the hand-over of
longer lists to the mid / long / block kernels, and the launch sequence around the stage (capacity guard, chunks on three lanes)."""
import importlib.util
import os

import numpy as np
import pytest

import orc
from common import GOLD

FORMS = ("1", "0")


def _make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def _index(tmp_path_factory, name, names, chroms):
    from bitmapperbs_amd import synth, mapper
    fa = str(tmp_path_factory.mktemp(name) / "g.fa")
    synth.write_fasta(fa, names, chroms)
    mapper.Index.build(fa, fa, threads=8, device=0)
    return dict(chroms=chroms, ix=mapper.Index(fa), oix=orc.OrcIndex(fa), cache={})


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    """the 300 kb test genome and the 5 Mb repeat-rich one (tests/golden/make_golden.py) and a plain random one, indexed on the device"""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    mg = _make_golden()
    from bitmapperbs_amd import synth
    # ("plain": 200 kb without a repeat, so that an error-free read has exactly one place)
    return {name: _index(tmp_path_factory, name, *g)
            for name, g in (("small", mg.genome()), ("big", mg.big_genome()), ("plain", synth.make_genome(200_000, 2, seed=911)))}


def both_forms(monkeypatch, g, prm, batches, L, env=None, want_retries=False):
    """maps `batches` (a list of (inp, oracle result); one context per form, the calls in order) under BMBS_VOTE_DENSE=1 and =0:
    the same bytes from both, the dense form equal to the oracle.  -> the counters of (dense, one lane per read)"""
    from bitmapperbs_amd import mapper
    from test_gpu_parity import compare_pe
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    got, cnts = [], []
    for form in FORMS:
        monkeypatch.setenv("BMBS_VOTE_DENSE", form)
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
        m.close()
        got.append(out)
    assert got[0] == got[1]
    return cnts


def _freeze(inp):
    for a in inp:
        a.setflags(write=False)
    return inp


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------------
def _spoil_n(seq, rng):
    pos = rng.random(seq.shape) < 0.002
    seq[pos] = np.frombuffer(b"NRYN", dtype=np.uint8)[rng.integers(0, 4, int(pos.sum()))]


@pytest.mark.gpu
@pytest.mark.parametrize("sens", [0, 1])
@pytest.mark.parametrize("L", [150, 251])                         # 251: lists of 17..32 are the rule, k_vote_pe_mid takes them
@pytest.mark.parametrize("genome", ["small", "big"])
def test_parity_with_one_lane_per_read_and_oracle(genomes, monkeypatch, genome, L, sens):
    from bitmapperbs_amd import synth
    g = genomes[genome]
    prm = dict(e_f=0.08, sensitive=sens, max_ins=max(500, 2 * L + 50))
    sub = 0.05 if sens else 0.02 + 0.01 * (L == 251)
    m1, m2 = synth.make_reads_pe(g["chroms"], n=2000, L=L, seed=900 + L + sens, sub=sub, indel=0.002, qual="random", ins_hi=max(500, 2 * L + 50))
    rng = np.random.default_rng(77 + L)
    _spoil_n(m1["seq"], rng); _spoil_n(m2["seq"], rng)
    inp = _freeze((m1["seq"], m1["qual"], m2["seq"], m2["qual"]))
    want = g["oix"].map_pe(orc.params(**prm), *inp, L)
    both_forms(monkeypatch, g, prm, [(inp, want)], L)


# ---- 2. / 3. how many reads of a block have lists, where they sit, blocks the batch does not fill ------------------------------------------
SPOIL_AT = (40, 80, 120)


def _other_letter(b):
    """a letter that differs from b in the three-letter alphabet as well (T and C are one letter there)"""
    out = np.full(b.shape, ord("A"), dtype=np.uint8)
    out[b == ord("A")] = ord("G")
    return out


def _clean_pairs(g, n, seed):
    """error-free pairs (every mate has an exact match), and the same pairs with three substitutions per mate, at positions SPOIL_AT
    of the row the seeding kernels see (mate 2: the reverse complement of its FASTQ text, where the read's C -> T conversion cannot
    hide them)"""
    from bitmapperbs_amd import synth
    m1, m2 = synth.make_reads_pe(g["chroms"], n=n, L=150, seed=seed, sub=0.0, indel=0.0, qual="const")
    clean = (m1["seq"], m2["seq"])
    r1, r2 = clean[0].copy(), synth.revcomp(clean[1])
    for s in (r1, r2):
        for p in SPOIL_AT:
            s[:, p] = _other_letter(s[:, p])
    return clean, (r1, synth.revcomp(r2)), m1["qual"], m2["qual"]


def _compose(clean, spoiled, h1, h2):
    """mate 1 of the pairs in h1 and mate 2 of the pairs in h2 spoiled"""
    s1 = clean[0].copy(); s2 = clean[1].copy()
    s1[h1] = spoiled[0][h1]; s2[h2] = spoiled[1][h2]
    return s1, s2


def _rows_as_seeded(s1, s2):
    """the rows the seeding kernels see: mate 1, and the reverse complement of mate 2's FASTQ text"""
    from bitmapperbs_amd import synth
    return np.concatenate([s1, synth.revcomp(s2)])


@pytest.fixture(scope="module")
def block_pairs(genomes):
    """256 pairs -- mate 1 fills block 0 of the vote kernel, mate 2 block 1 -- and the premise the cases stand on, by the oracle's
    single-end counters on the mates: a clean mate ends at its first table lookup (exit A), a spoiled one seeds on (verdict 3)"""
    g = genomes["plain"]
    clean, spoiled, q1, q2 = _clean_pairs(g, 256, 4242)
    q = np.concatenate([q1, q2])
    for rows, is_clean in ((_rows_as_seeded(*clean), True), (_rows_as_seeded(*spoiled), False)):
        recs, _, cnt = g["oix"].map_se(orc.params(e_f=0.08), rows, q, 150)
        if is_clean:
            assert cnt["n_hash"] == rows.shape[0], cnt
        else:
            assert cnt["n_hash"] > 2 * rows.shape[0], cnt
            assert (recs["n_cand"] > 0).all() and (recs["path"] == 3).all(), (recs["path"], recs["n_cand"])
    return g, clean, spoiled, q1, q2


def _layout(count, where, size=256):
    if where == "front":
        return np.arange(count)
    if where == "back":
        return np.arange(size - count, size)
    return (np.arange(count) * size) // max(count, 1)             # every k-th lane


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["front", "back", "strided"])
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 128, 255, 256])
def test_heavy_reads_per_block(block_pairs, monkeypatch, count, where):
    """exactly `count` reads with lists in block 0 (mate 1) and 256 - count in block 1 (mate 2)"""
    g, clean, spoiled, q1, q2 = block_pairs
    h1 = _layout(count, where)
    h2 = _layout(256 - count, where)
    s1, s2 = _compose(clean, spoiled, h1, h2)
    inp = _freeze((s1, q1, s2, q2))
    prm = dict(e_f=0.08)
    want = g["oix"].map_pe(orc.params(**prm), *inp, 150)
    both_forms(monkeypatch, g, prm, [(inp, want)], 150)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 31, 33, 127, 129, 2049])
def test_tail_blocks(genomes, monkeypatch, n):
    """2n reads are no multiple of 64 or 256; the last block holds reads with lists (the last pair and every third one)"""
    g = genomes["small"]
    clean, spoiled, q1, q2 = _clean_pairs(g, n, 5000 + n)
    h = np.union1d(np.arange(0, n, 3), [n - 1])
    s1, s2 = _compose(clean, spoiled, h, h)
    inp = _freeze((s1, q1, s2, q2))
    prm = dict(e_f=0.08)
    want = g["oix"].map_pe(orc.params(**prm), *inp, 150)
    both_forms(monkeypatch, g, prm, [(inp, want)], 150)


# ---- 4. hand-over classes -----------------------------------------------------------------------------------------------------------------
COPIES = (2, 15, 16, 17, 32, 33, 300)
ELEN = 600


def family_genome():
    """1 Mb in two chromosomes; per copy count one element of G/A/T letters only and one of all four letters, each planted in exactly
    that many identical copies (forward, 1000 bases apart or more, so no two copies touch).  -> names, chroms, {(kind, copies): element}"""
    from bitmapperbs_amd import synth
    names, chroms = synth.make_genome(1_000_000, 2, seed=811)
    rng = np.random.default_rng(812)
    slots = [(c, p) for c in range(2) for p in range(0, 499_000, 1000)]
    order = rng.permutation(len(slots))
    gat = np.frombuffer(b"GAT", dtype=np.uint8)
    els, at = {}, 0
    for kind in ("gat", "acgt"):
        for copies in COPIES:
            e = gat[rng.integers(0, 3, ELEN)] if kind == "gat" else synth._ACGT[rng.integers(0, 4, ELEN)]
            els[(kind, copies)] = e
            for _ in range(copies):
                c, p = slots[order[at]]; at += 1
                chroms[c][p:p + ELEN] = e
    assert at <= len(slots)
    return names, chroms, els


def _pairs_from(e, n, L, rng):
    """n error-free pairs whose fragments lie inside the element e"""
    from bitmapperbs_amd import synth
    ins = rng.integers(L + 20, ELEN - 10, n)
    a = (rng.random(n) * (ELEN - ins)).astype(np.int64)
    s1 = np.stack([e[x:x + L] for x in a])
    s2 = np.stack([synth.revcomp(e[x + i - L:x + i]) for x, i in zip(a, ins)])
    return s1, s2


@pytest.fixture(scope="module")
def families(tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    names, chroms, els = family_genome()
    g = _index(tmp_path_factory, "families", names, chroms)
    g["els"] = els
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("L", [150, 251])
def test_hand_over_classes(families, monkeypatch, L):
    """exact reads from G/A/T elements: verdict 4 with as many candidates as the element has copies -- 16 stay in registers, 17 and 32
    go to the mid kernel (L = 251) or the wave form, 33 to the wave form, 300 to the block form; reads with two substitutions from
    the four-letter elements: verdict 3 with lists of every class"""
    g = families
    rng = np.random.default_rng(813 + L)
    s1s, s2s = [], []
    for (kind, copies), e in g["els"].items():
        s1, s2 = _pairs_from(e, 12, L, rng)
        if kind == "gat":
            # the premise, by the oracle on mate 1: exact and ambiguous (every copy is a hit, and every hit a candidate)
            recs, _, _ = g["oix"].map_se(orc.params(e_f=0.08), s1, np.full_like(s1, ord("I")), L)
            assert (recs["path"] == 4).all(), (copies, recs["path"])
        else:
            for s in (s1, s2):
                for p in (L // 3, 2 * L // 3):
                    s[:, p] = _other_letter(s[:, p])
            recs, _, _ = g["oix"].map_se(orc.params(e_f=0.08), s1, np.full_like(s1, ord("I")), L)
            assert (recs["path"] == 3).all() and (recs["n_cand"] >= 3 * copies).all(), (copies, recs["path"], recs["n_cand"])
        s1s.append(s1); s2s.append(s2)
    s1 = np.concatenate(s1s); s2 = np.concatenate(s2s)
    q = np.full_like(s1, ord("I"))
    inp = _freeze((s1, q, s2, q.copy()))
    prm = dict(e_f=0.08, max_ins=ELEN + 50)
    want = g["oix"].map_pe(orc.params(**prm), *inp, L)
    dense, sparse = both_forms(monkeypatch, g, prm, [(inp, want)], L)
    for k in ("n_cand_mid", "n_cand_long", "n_cand_big", "n_lists_long"):
        assert dense[k] == sparse[k], k
    assert dense["n_cand_long"] > 0 and dense["n_cand_big"] > 0 and dense["n_lists_long"] > 0
    if L == 251:
        assert dense["n_cand_mid"] > 0


# ---- 5. the launch sequence around the stage ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_capacity_guard_repeats_the_call(genomes, monkeypatch):
    """BMBS_CAP_SCALE shrinks the learned capacities: the later calls' candidates do not fit, the guard takes the work away and the call
    runs again with exact sizes -- results as if nothing had happened, under both forms"""
    from bitmapperbs_amd import synth
    g = genomes["small"]
    batches = []
    for seed, sub in [(611, 0.005), (612, 0.05), (613, 0.06)]:
        m1, m2 = synth.make_reads_pe(g["chroms"], n=9000, L=100, seed=seed, sub=sub, indel=0.002, qual="random")
        inp = _freeze((m1["seq"], m1["qual"], m2["seq"], m2["qual"]))
        batches.append((inp, g["oix"].map_pe(orc.params(), *inp, 100)))
    both_forms(monkeypatch, g, {}, batches, 100, env={"BMBS_CAP_SCALE": "0.02", "BMBS_LANES": "2", "BMBS_SPLIT_MIN": "3000"}, want_retries=True)


@pytest.mark.gpu
def test_chunks_on_three_lanes(genomes, monkeypatch):
    """2000 pairs as five chunks of 400 dealt to three lanes"""
    from bitmapperbs_amd import synth
    g = genomes["big"]
    m1, m2 = synth.make_reads_pe(g["chroms"], n=2000, L=150, seed=621, sub=0.03, indel=0.002, qual="random")
    inp = _freeze((m1["seq"], m1["qual"], m2["seq"], m2["qual"]))
    want = g["oix"].map_pe(orc.params(e_f=0.08), *inp, 150)
    both_forms(monkeypatch, g, dict(e_f=0.08), [(inp, want)], 150, env={"BMBS_LANES": "3", "BMBS_SPLIT_MIN": "200", "BMBS_CHUNK": "400"})

