"""BMBS_SEED_STAGE: k_seed_first writes each chunk's first-seed results coalesced out of LDS, and k_seed_decide_p keeps back the
exit-A record nobody reads (not under --sensitive).  Both forms map exactly like the oracle and like each other: single-end,
paired-end fast and --sensitive, on inputs that reach every booking path."""
import numpy as np
import pytest

import orc
from test_gpu_parity import _trim, compare_pe, compare_records

pytestmark = pytest.mark.gpu

FORMS = ("0", "1")


@pytest.fixture(scope="module")
def genv(tmp_path_factory):
    """a genome with repeat families (seeds with many hits: records with hits > 1, reads that run every seed)"""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bitmapperbs_amd import synth, mapper
    from common import plant_repeats
    wd = tmp_path_factory.mktemp("stage")
    names, chroms = synth.make_genome(1_000_000, 2, seed=171)
    plant_repeats(chroms, seed=172)
    fa = str(wd / "g.fa")
    synth.write_fasta(fa, names, chroms)
    mapper.Index.build(fa, fa, threads=8)
    return dict(chroms=chroms, ix=mapper.Index(fa), oix=orc.OrcIndex(fa))


def _se_batch(chroms):
    """12 345 reads (not a multiple of 64 or of a chunk): exact reads (exit A / B), 1-mismatch reads (exit C), heavily
    substituted reads that run all max_seed seeds and book many records, reads with N, and lengths
    from 17 to 250 (reads shorter than 18 bases after their first seed)"""
    from bitmapperbs_amd import synth
    parts = [synth.make_reads_se(chroms, n=3000, L=250, seed=181, sub=0.0, indel=0.0, qual="const", conv=0.0),
             synth.make_reads_se(chroms, n=3000, L=250, seed=182, sub=0.004, indel=0.0, qual="random"),
             synth.make_reads_se(chroms, n=3000, L=250, seed=183, sub=0.06, indel=0.003, qual="random", n_rate=0.004),
             synth.make_reads_se(chroms, n=3345, L=250, seed=184, sub=0.02, indel=0.002, qual="random", n_rate=0.002)]
    seq = np.concatenate([p["seq"] for p in parts]); qual = np.concatenate([p["qual"] for p in parts])
    rng = np.random.default_rng(185)
    lens = rng.integers(17, 251, seq.shape[0]).astype(np.uint16)
    lens[::5] = 250; lens[1::11] = 30; lens[2::13] = 20
    return _trim(seq, lens), _trim(qual, lens), lens


def _run_se(genv, monkeypatch, form, seq, qual, lens):
    from bitmapperbs_amd import mapper
    monkeypatch.setenv("BMBS_SEED_STAGE", form)
    m = mapper.Mapper(genv["ix"], 0, e_f=0.08)
    res, pool = m.map_se_var(seq, qual, lens)
    stats = m.stats().copy()
    m.close()
    return res, pool, stats


def test_seed_stage_forms_se(genv, monkeypatch):
    seq, qual, lens = _se_batch(genv["chroms"])
    recs, ost, _ = genv["oix"].map_se_var(orc.params(e_f=0.08), seq, qual, lens)
    assert (recs["status"] == 1).sum() > 6000
    out = {f: _run_se(genv, monkeypatch, f, seq, qual, lens) for f in FORMS}
    for f, (res, pool, stats) in out.items():
        bad = compare_records(res, pool, recs, lens)
        assert not bad, (f, bad[:10])
        assert (stats == ost).all(), (f, stats, ost)
    res0, pool0, _ = out["0"]
    for f in FORMS[1:]:
        assert out[f][0].tobytes() == res0.tobytes(), f
        assert np.array_equal(out[f][1], pool0), f


@pytest.mark.parametrize("sensitive", [0, 1], ids=["fast", "sensitive"])
def test_seed_stage_forms_pe(genv, monkeypatch, sensitive):
    """pairs of different mate lengths, N in some mates, exact and heavily substituted pairs, 9 001 pairs"""
    from bitmapperbs_amd import synth, mapper
    n = 9001
    m1, m2 = synth.make_reads_pe(genv["chroms"], n=n, L=150, seed=191 + sensitive, sub=0.03, indel=0.002, qual="random", ins_hi=500)
    rng = np.random.default_rng(193)
    ex1, ex2 = synth.make_reads_pe(genv["chroms"], n=2000, L=150, seed=194, sub=0.0, indel=0.0, qual="const", conv=0.0, ins_hi=500)
    for mm, ex in ((m1, ex1), (m2, ex2)):
        mm["seq"][:2000] = ex["seq"]; mm["qual"][:2000] = ex["qual"]
        pos = rng.random(mm["seq"].shape) < 0.003
        pos[:4000] = False
        mm["seq"][pos] = ord("N")
    l1 = rng.integers(30, 151, n).astype(np.uint16); l2 = rng.integers(30, 151, n).astype(np.uint16)
    l1[:3000] = 150; l2[:3000] = 150
    s1, q1, s2, q2 = _trim(m1["seq"], l1), _trim(m1["qual"], l1), _trim(m2["seq"], l2), _trim(m2["qual"], l2)
    prm = dict(sensitive=sensitive, max_ins=500)
    recs, ost, _ = genv["oix"].map_pe_var(orc.params(**prm), s1, q1, s2, q2, l1, l2)
    assert (recs["status"] == 1).sum() > 3000
    out = {}
    for f in FORMS:
        monkeypatch.setenv("BMBS_SEED_STAGE", f)
        m = mapper.Mapper(genv["ix"], 0, **prm)
        res, pool = m.map_pe_var(s1, q1, s2, q2, l1, l2)
        bad = compare_pe(res, pool, recs, l1, l2)
        assert not bad, (f, bad[:5])
        assert (m.stats() == ost).all(), (f, m.stats(), ost)
        out[f] = res.copy()
        m.close()
    for f in FORMS[1:]:
        assert out[f].tobytes() == out["0"].tobytes(), f
