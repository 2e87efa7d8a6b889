"""-m gpu: the alignment stage on crafted jobs (tests/align_cases.py), every form of the DP -- BMBS_SW = reg2 (k_align_sw2, two jobs
per lane in 16 bits, where run_align admits it), reg (k_align_sw) and wave (k_align_sw_wave) -- on the ASCII rows
(bmbs_align_batch: k_align_ungapped, k_align_sw2<KB, false, false>) and on the packed rows the mapping calls run
(bmbs_align_batch_packed: k_align_ungapped_p, k_align_sw2<KB, EXACT, true>), the latter also with half of the reads reading their
qualities mirrored.  (start, end, NM, score, CIGAR) against orc.align, exactly: integers and text, no tolerance.

What makes the jobs worth running -- every job accepted by the filter, every edit class really showing its operation, the tie set
really scoring differently, the two host references agreeing -- is asserted on the host by tests/test_align_spec.py."""
import numpy as np
import pytest

import align_cases as ac
import align_spec
import orc
from test_gpu_parity import compare_records, env          # noqa: F401  (env: the module-scoped fixture, built once for this module too)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(env, tmp_path_factory):
    """the two genomes with their device index and oracle index; the jobs and oracle results of a case are computed once"""
    from bitmapperbs_amd import mapper
    _, chroms = ac.make_env_genome()
    assert all(np.array_equal(a, b) for a, b in zip(chroms, env["chroms"])), "align_cases.GENOME no longer describes the env fixture"
    fa, hp_oix = ac.build_index(tmp_path_factory.mktemp("align_hp"), *ac.make_homopolymer_genome(), "hp")
    return dict(env=dict(ix=env["ix"], oix=env["oix"]), hp=dict(ix=mapper.Index(fa), oix=hp_oix), cache={})


def case_data(world, name):
    if name not in world["cache"]:
        case = ac.CASE_BY_NAME[name]
        jobs = ac.build_jobs(case, world[case["genome"]]["oix"])
        n = len(jobs["pattern"])
        rq = np.arange(n) >= n // 2
        world["cache"][name] = dict(case=case, jobs=jobs, rev_from=n // 2, orc=ac.reference_results(case, jobs),
                                    orc_rev=ac.reference_results(case, jobs, rq))
    return world["cache"][name]


def device_results(out, L):
    res = []
    for j in range(out["n_ops"].size):
        n_ops = int(out["n_ops"][j])
        assert n_ops >= 0, "job %d overflowed its CIGAR slots" % j
        cg = "%dM" % L if n_ops == 0 else "".join("%d%s" % (int(x) >> 4, "MDISH"[int(x) & 15]) for x in out["ops"][j][:n_ops])
        res.append((int(out["start"][j]), int(out["end"][j]), int(out["nm"][j]), int(out["score"][j]), cg))
    return res


@pytest.mark.parametrize("form", ["reg2", "reg", "wave"])
@pytest.mark.parametrize("name", [c["name"] for c in ac.CASES])
def test_align_forms_match_oracle(world, monkeypatch, name, form):
    from bitmapperbs_amd import mapper
    monkeypatch.setenv("BMBS_SW", form)
    d = case_data(world, name)
    case, jobs = d["case"], d["jobs"]
    L, k = case["L"], case["k"]
    assert jobs["accepted"].all() and int(jobs["dp"].sum()) == case["n"]          # n = the jobs that reach the DP kernels
    if name == "inverted40000":
        # the case is about scores that 16 bits cannot hold: it proves something only if the jobs really have them
        prm = orc.params(**ac.params_of(case["scoring"], L, k))
        spec = align_spec.align_batch(prm, jobs["windows"], jobs["seq"][:, :L], jobs["qual"][:, :L], k, jobs["end"], jobs["err"], jobs["forward"])
        assert sum(s["raw"] is not None and s["lo"] < -32768 for s in spec) >= 30
    m = mapper.Mapper(world[case["genome"]]["ix"], 0, **ac.params_of(case["scoring"], L, k))
    assert m.threshold(L) == k
    read_of = np.arange(len(jobs["pattern"]), dtype=np.uint32)
    for rows, rev_from, want in (("ascii", None, d["orc"]), ("packed", None, d["orc"]), ("packed_mirrored", d["rev_from"], d["orc_rev"])):
        out = m.align(jobs["seq"], jobs["qual"], L, read_of, jobs["site"], jobs["end"], jobs["err"], packed=rows != "ascii", rev_from=rev_from)
        got = device_results(out, L)
        for j, (g, o) in enumerate(zip(got, want)):
            assert g == (o["start"], o["end"], o["nm"], o["score"], o["cigar"]), (rows, j, jobs["pattern"][j], int(jobs["site"][j]))
    m.close()


def test_map_se_with_phred64_on_phred33_qualities(env):
    """--phred64 on Phred+33 data: quality bytes below q_base take the penalty formula below zero, mismatches raise the score, and a
    score above 0 has a MAPQ of its own (not `perfect`, though every rank cut is reached): whole mapping against the oracle, MAPQ included"""
    from bitmapperbs_amd import synth, mapper
    n, L = 3000, 100
    r = synth.make_reads_se(env["chroms"], n=n, L=L, seed=64, sub=0.03, indel=0.002, qual="random")
    qual = r["qual"].copy()
    qual[:, :L] = np.random.default_rng(65).integers(33, 38, (n, L))          # '!' .. '%': penalties -1 and 0
    m = mapper.Mapper(env["ix"], 0, q_base=64)
    res, pool = m.map_se(r["seq"], qual, L)
    recs, ost, _ = env["oix"].map_se(orc.params(q_base=64), r["seq"], qual, L)
    assert ((recs["status"] == 1) & (recs["score"] > 0)).sum() >= 20
    bad = compare_records(res, pool, recs, L)
    assert not bad, bad[:10]
    assert (m.stats() == ost).all()
    m.close()
