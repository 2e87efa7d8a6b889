"""The dispatch layer of bmbs_api.hip -- the chunk plan, the host-buffer calls' upload / kernels / download per lane, the device
calls' dealing of chunks -- pinned at a shape where every lane takes more than one chunk: 6 000 units cut into chunks of 700 (eight
of them and one of 400) over four host lanes / three device lanes.  Bit-exact everywhere."""
import ctypes as C

import numpy as np
import pytest

import orc
from test_gpu_parity import _sprinkle_n, _trim, compare_pe, compare_records, env  # noqa: F401  (env: the module's fixture)

pytestmark = pytest.mark.gpu

N, CHUNK = 6000, 700
SPLIT = {"BMBS_SPLIT_MIN": "500", "BMBS_CHUNK": str(CHUNK)}
EINVAL, ENOMEM = -22, -12
FIELDS = ("status", "chrom", "pos", "flag", "mapq", "nm", "score", "n_cigar", "tlen", "path", "n_cand")


@pytest.fixture(scope="module")
def D(env):
    """one single-end batch (L = 150) and one of pairs (L = 100): full-length rows for the uniform calls; trimmed ones (20 or 30 .. L,
    the first rows at L, a sprinkle of 'N') with their packed rows and packed quality classes for the others; the oracle's records of
    the trimmed batches; results of earlier runs by (form, switches)"""
    from bitmapperbs_amd import synth, mapper
    P, Q = mapper.Mapper.pack_rows, mapper.pack_quals
    rng = np.random.default_rng(907)
    r = synth.make_reads_se(env["chroms"], n=N, L=150, seed=901, sub=0.02, indel=0.002, qual="random", n_rate=0.002)
    ln = rng.integers(20, 151, N).astype(np.uint16); ln[:300] = 150
    seq, qual = _trim(r["seq"], ln), _trim(r["qual"], ln)
    se = dict(L=150, full=(r["seq"], r["qual"]), seq=seq, qual=qual, len=ln, rows=P(seq, 150, ln), qrows=Q(None, qual, 150, ln))
    m1, m2 = synth.make_reads_pe(env["chroms"], n=N, L=100, seed=902, sub=0.02, indel=0.002, qual="random", ins_hi=480)
    l1 = rng.integers(30, 101, N).astype(np.uint16); l2 = rng.integers(30, 101, N).astype(np.uint16)
    l1[:300] = 100; l2[:300] = 100
    s1, q1, s2, q2 = _trim(m1["seq"], l1), _trim(m1["qual"], l1), _trim(m2["seq"], l2), _trim(m2["qual"], l2)
    s1 = _sprinkle_n(rng, s1, l1); s2 = _sprinkle_n(rng, s2, l2)
    pe = dict(L=100, full=(m1["seq"], m1["qual"], m2["seq"], m2["qual"]), seq=(s1, s2), qual=(q1, q2), len=(l1, l2),
              rows=(P(s1, 100, l1), P(s2, 100, l2)), qrows=(Q(None, q1, 100, l1), Q(None, q2, 100, l2)))
    se["oracle"] = env["oix"].map_se_var(orc.params(), seq, qual, ln)[:2]
    pe["oracle"] = env["oix"].map_pe_var(orc.params(), s1, q1, s2, q2, l1, l2)[:2]
    assert (se["oracle"][0]["status"] == 1).sum() > N // 2 and (pe["oracle"][0]["status"] == 1).sum() > N // 3
    return dict(se=se, pe=pe, runs={})


def _c(a):
    return np.ascontiguousarray(a)


def _ops(L):
    """CIGAR slots per read under the default parameters"""
    from bitmapperbs_amd import capi
    return int(capi.lib().bmbs_max_cigar_ops(C.byref(capi.default_params()), L))


# the eight host-buffer forms on the rows `sl` of the batch
FORMS = {
    "se": lambda m, d, sl: m.map_se(d["full"][0][sl], d["full"][1][sl], d["L"]),
    "se_var": lambda m, d, sl: m.map_se_var(d["seq"][sl], d["qual"][sl], d["len"][sl]),
    "se_packed": lambda m, d, sl: m.map_se_packed(_c(d["rows"][sl]), d["qual"][sl], d["L"], d["len"][sl]),
    "se_packedq": lambda m, d, sl: m.map_se_packedq(_c(d["rows"][sl]), _c(d["qrows"][sl]), d["L"], d["len"][sl]),
    "pe": lambda m, d, sl: m.map_pe(*[a[sl] for a in d["full"]], d["L"]),
    "pe_var": lambda m, d, sl: m.map_pe_var(d["seq"][0][sl], d["qual"][0][sl], d["seq"][1][sl], d["qual"][1][sl], d["len"][0][sl], d["len"][1][sl]),
    "pe_packed": lambda m, d, sl: m.map_pe_packed(_c(d["rows"][0][sl]), _c(d["rows"][1][sl]), d["qual"][0][sl], d["qual"][1][sl], d["L"],
                                                  d["len"][0][sl], d["len"][1][sl]),
    "pe_packedq": lambda m, d, sl: m.map_pe_packedq(_c(d["rows"][0][sl]), _c(d["rows"][1][sl]), _c(d["qrows"][0][sl]), _c(d["qrows"][1][sl]), d["L"],
                                                    d["len"][0][sl], d["len"][1][sl]),
}


def _mapper(env, switches, **prm):
    """the switches are read when a context is created, and only then"""
    from bitmapperbs_amd import mapper
    with pytest.MonkeyPatch.context() as mp:
        for k, v in switches.items():
            mp.setenv(k, v)
        return mapper.Mapper(env["ix"], 0, **prm)


def _run(env, D, form, switches, sl=slice(None)):
    """(records, CIGAR pool cut at n_cigar_used, statistics) of one call on a fresh context; kept for the tests that share it"""
    key = (form, tuple(sorted(switches.items())), sl.start, sl.stop)
    if key not in D["runs"]:
        m = _mapper(env, switches)
        res, pool = FORMS[form](m, D[form[:2]], sl)
        D["runs"][key] = (res, pool, m.stats().copy())
        m.close()
    return D["runs"][key]


def _differences(a, pa, b, pb, offsets):
    """every field of every record (cigar_off only with `offsets`), and every record's CIGAR words read through its own cigar_off"""
    bad = []
    assert a.size == b.size
    for f in FIELDS + (("cigar_off",) if offsets else ()):
        d = np.nonzero(a[f] != b[f])[0]
        if d.size:
            bad.append((f, int(d[0]), int(a[f][d[0]]), int(b[f][d[0]])))
    for i in np.nonzero((a["n_cigar"] > 0) & (a["n_cigar"] < 255) & (a["n_cigar"] == b["n_cigar"]))[0]:
        k, oa, ob = int(a[i]["n_cigar"]), int(a[i]["cigar_off"]), int(b[i]["cigar_off"])
        if oa + k > pa.size or ob + k > pb.size or not (pa[oa:oa + k] == pb[ob:ob + k]).all():
            bad.append(("cigar", int(i)))
            break
    return bad


# ---- 1. split invariance, every form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(FORMS))
def test_nine_chunks_on_four_lanes_give_the_records_of_the_whole_call(form, env, D):
    """every lane takes a second chunk (lane 0 a third) and the last chunk is ragged: every field but cigar_off, every record's CIGAR
    words and the statistics are those of the call that runs whole; the two var-length forms also against the oracle"""
    res, pool, st = _run(env, D, form, SPLIT)
    res1, pool1, st1 = _run(env, D, form, {})
    assert (res["n_cigar"] > 0).sum() > 200
    base_last = (N // CHUNK) * CHUNK * (2 if form.startswith("pe") else 1) * _ops(D[form[:2]]["L"])
    assert res["cigar_off"].max() >= base_last > res1["cigar_off"].max()          # (the chunks did have bases of their own)
    bad = _differences(res, pool, res1, pool1, offsets=False)
    assert not bad, bad
    assert (st == st1).all(), (st, st1)
    if form == "se_var":
        recs, ost = D["se"]["oracle"]
        bad = compare_records(res, pool, recs, D["se"]["len"])
        assert not bad, bad[:5]
        assert (st == ost).all(), (st, ost)
    if form == "pe_var":
        recs, ost = D["pe"]["oracle"]
        bad = compare_pe(res, pool, recs, *D["pe"]["len"])
        assert not bad, bad[:5]
        assert (st == ost).all(), (st, ost)


# ---- 2. n_cigar_used ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["se", "pe_packed"])
def test_n_cigar_used_is_the_end_of_the_last_job_of_the_last_chunk_that_has_one(form, env, D):
    """k_finalize / k_finalize_pe give a record whose read has an alignment job `cigar_off = cigar_base + job * max_ops`, the jobs of a
    chunk being numbered 0 .. jobs - 1 by align_jobs' scan, and the dispatcher returns the largest `cigar_base + jobs * max_ops` over
    the chunks that had a job.  A job need not end in a record with a CIGAR (an ambiguous read's does not), so from the records alone
    the count is pinned from below: a multiple of max_ops, at or above `cigar_off + max_ops` of every record with a CIGAR, at most the
    capacity.  From above it is pinned by the jobs themselves: the whole call's count over max_ops is its number of jobs, a read's
    having one does not depend on the batch around it, so the last chunk mapped alone returns jobs_last * max_ops and the split call
    exactly `base of the last chunk + that`."""
    d = D[form[:2]]
    rpu = 2 if form.startswith("pe") else 1
    ops = _ops(d["L"])
    last = slice((N // CHUNK) * CHUNK, N)
    base_last = last.start * rpu * ops
    got = {}
    for tag, sw in (("whole", {}), ("split", SPLIT)):
        res, pool, _ = _run(env, D, form, sw)
        used = pool.size                                     # (the Mapper cuts the pool at the count the call returned)
        has = res["n_cigar"] > 0
        ends = res["cigar_off"][has].astype(np.int64) + ops
        print(form, tag, "n_cigar_used", used, "max_ops", ops, "capacity", N * rpu * ops, "largest cigar_off + max_ops", int(ends.max()))
        assert used % ops == 0 and int(ends.max()) <= used <= N * rpu * ops
        assert ((res["cigar_off"][has].astype(np.int64) + res["n_cigar"][has]) <= used).all()
        assert (res["cigar_off"][has] % ops == 0).all()
        got[tag] = (res, used)
    res, used = got["split"]
    assert (res["n_cigar"][last.start * rpu:] > 0).any() and used >= base_last
    m = _mapper(env, {})
    each = [FORMS[form](m, d, slice(a, min(a + CHUNK, N)))[1].size for a in range(0, N, CHUNK)]
    m.close()
    alone, total = each[-1], sum(each)
    print(form, "last chunk alone", alone, "its base", base_last, "sum over the chunks alone", total)
    assert alone > 0 and used == base_last + alone
    assert got["whole"][1] == total


# ---- 3. a repeated chunk on a reused lane -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["pe_packed", "se_packedq"])
def test_chunks_repeated_with_exact_sizes_on_lanes_that_take_several(form, env):
    """BMBS_CAP_SCALE shrinks the learned capacities: chunks of the second and third call are issued again, on lanes that then go on
    to their next chunk -- the records behind the first attempt are copied again, the packed quality classes are still expanded"""
    from bitmapperbs_amd import synth, mapper
    M = mapper.Mapper
    m = _mapper(env, dict(SPLIT, BMBS_CAP_SCALE="0.02"))
    tot = np.zeros(5, dtype=np.int64)
    for seed, sub in [(921, 0.005), (922, 0.05), (923, 0.05)]:
        if form == "se_packedq":
            r = synth.make_reads_se(env["chroms"], n=N, L=150, seed=seed, sub=sub, indel=0.002, qual="random", n_rate=0.002)
            res, pool = m.map_se_packedq(M.pack_rows(r["seq"], 150), m.pack_quals(r["qual"], 150), 150)
            recs, ost, _ = env["oix"].map_se(orc.params(), r["seq"], r["qual"], 150)
            bad = compare_records(res, pool, recs, 150)
        else:
            m1, m2 = synth.make_reads_pe(env["chroms"], n=N, L=100, seed=seed, sub=sub, indel=0.002, qual="random")
            res, pool = m.map_pe_packed(M.pack_rows(m1["seq"], 100), M.pack_rows(m2["seq"], 100), m1["qual"], m2["qual"], 100)
            recs, ost, _ = env["oix"].map_pe(orc.params(), m1["seq"], m1["qual"], m2["seq"], m2["qual"], 100)
            bad = compare_pe(res, pool, recs, 100)
        assert (recs["status"] == 1).sum() > N // 3
        assert not bad, bad[:5]
        tot += ost
        assert (m.stats() == tot).all(), (m.stats(), tot)
    assert m.retries() > 0
    m.close()


# ---- 4. the switches of the layer ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["BMBS_UP_TURNS=0", "BMBS_HOST_LANES=1", "BMBS_HOST_LANES=2", "BMBS_HOST_LANES=8", "BMBS_HOST_LANES=2 BMBS_LANES=2",
                                    "BMBS_HOST_LANES=1 BMBS_LANES=1"])
@pytest.mark.parametrize("form", ["se_var", "pe_packedq"])
def test_upload_turns_and_the_number_of_host_lanes_change_nothing(form, switch, env, D):
    """chunk k's place in the caller's buffers does not depend on the lane that takes it or on who uploads when: records byte for
    byte, cigar_off included, and the same CIGAR words as with the defaults.  A context has at least BMBS_LANES (three) host lanes,
    so BMBS_HOST_LANES below that takes effect only with BMBS_LANES lowered too.  One lane is the path without threads and, like
    every context with fewer than two lanes, runs the call whole: the whole call's records"""
    sw = dict(SPLIT, **dict(s.split("=") for s in switch.split()))
    res, pool, st = _run(env, D, form, sw)
    res0, pool0, st0 = _run(env, D, form, {} if sw.get("BMBS_LANES") == "1" else SPLIT)
    bad = _differences(res, pool, res0, pool0, offsets=True)
    assert not bad, bad
    assert pool.size == pool0.size and (st == st0).all()


# ---- 5. a failure in a later chunk ----------------------------------------------------------------------------------------------------------
def test_a_bad_length_in_the_sixth_chunk_fails_the_call_and_leaves_the_context_usable(env, D):
    """the host-side check of a chunk's lengths (upload_lens) fails on one lane while others are at work: BMBS_EINVAL with its
    message, every lane drained; the same context then maps the good batch to the oracle's records and statistics"""
    d = D["pe"]
    (s1, s2), (q1, q2), (l1, l2) = d["seq"], d["qual"], d["len"]
    bad_l2 = l2.copy(); bad_l2[5 * CHUNK + 100] = 0
    m = _mapper(env, SPLIT)
    with pytest.raises(RuntimeError) as e:
        m.map_pe_var(s1, q1, s2, q2, l1, bad_l2)
    assert "bmbs error %d: " % EINVAL in str(e.value) and "read length 0 or longer than L_max" in str(e.value)
    m.reset_stats()
    res, pool = m.map_pe_var(s1, q1, s2, q2, l1, l2)
    recs, ost = d["oracle"]
    bad = compare_pe(res, pool, recs, l1, l2)
    assert not bad, bad[:5]
    assert (m.stats() == ost).all(), (m.stats(), ost)
    m.close()


# ---- 6. the host pool bound ----------------------------------------------------------------------------------------------------------------
def test_host_cigar_pool_of_exactly_the_words_used_is_enough_and_one_less_is_not(env, D):
    """a call that runs whole: U = n_cigar_used of a call with a full pool; a pool of U words gives the same records, one of U - 1
    BMBS_ENOMEM "host cigar pool too small" (the device writes into the lane's own worst-case pool either way).  A context that
    would split finds that a pool of U words cannot hold every chunk's worst case and runs the call whole: the same records,
    cigar_off included"""
    from bitmapperbs_amd import capi
    lib = capi.lib()
    seq, qual = (_c(a) for a in D["se"]["full"])
    res0, pool0, _ = _run(env, D, "se", {})
    U = pool0.size
    assert 0 < U < N * 40

    def call(m, cap):
        res = np.zeros(N, dtype=capi.RESULT_DTYPE); pool = np.zeros(U + 1, dtype=np.uint32); used = C.c_int64(-1)
        rc = lib.bmbs_map_se(m._ctx, capi.ptr(seq), capi.ptr(qual), 150, 150, N, capi.ptr(res), capi.ptr(pool), cap, C.byref(used))
        return rc, res, pool, used.value
    for sw in ({}, SPLIT):
        m = _mapper(env, sw)
        rc, res, pool, used = call(m, U)
        assert rc == 0 and used == U and pool[U] == 0
        assert not _differences(res, pool, res0, pool0, offsets=True)
        m.close()
    m = _mapper(env, {})
    rc, res, pool, used = call(m, U - 1)
    assert rc == ENOMEM and b"host cigar pool too small" in lib.bmbs_last_error(m._ctx)
    m.close()


# ---- 7. edges --------------------------------------------------------------------------------------------------------------------------------
def test_empty_and_negative_counts_and_bad_geometry(env):
    """host calls: n <= 0 is BMBS_OK with a count of 0, before the geometry is looked at; device calls: the geometry comes first and
    n < 0 is part of it"""
    import torch
    from bitmapperbs_amd import capi, mapper
    lib = capi.lib()
    m = mapper.Mapper(env["ix"], 0)
    seq = np.full((4, 64), ord("A"), dtype=np.uint8); qual = np.full((4, 64), ord("I"), dtype=np.uint8)
    res = np.zeros(8, dtype=capi.RESULT_DTYPE); pool = np.zeros(4096, dtype=np.uint32)
    a = (capi.ptr(res), capi.ptr(pool), 4096)
    for n in (0, -1):
        used = C.c_int64(99)
        assert lib.bmbs_map_se(m._ctx, capi.ptr(seq), capi.ptr(qual), 50, 64, n, *a, C.byref(used)) == 0 and used.value == 0
        used = C.c_int64(99)
        assert lib.bmbs_map_pe(m._ctx, capi.ptr(seq), capi.ptr(qual), capi.ptr(seq), capi.ptr(qual), 0, 64, n, *a, C.byref(used)) == 0 and used.value == 0
    used = C.c_int64(99)
    for L, stride in ((0, 64), (50, 49)):
        assert lib.bmbs_map_se(m._ctx, capi.ptr(seq), capi.ptr(qual), L, stride, 4, *a, C.byref(used)) == EINVAL
        assert lib.bmbs_last_error(m._ctx) == b"bad read geometry" and used.value == 0
    t = torch.zeros(4 * 64 * 2 + 8 * 32 + 4096 * 4, dtype=torch.uint8, device="cuda")
    p = t.data_ptr()
    dev = (p + 512, p + 512 + 256, 4096)
    for L, stride, n in ((0, 64, 4), (50, 49, 4), (50, 64, -1)):
        assert lib.bmbs_map_se_device(m._ctx, p, p + 256, L, stride, n, *dev) == EINVAL
        assert lib.bmbs_last_error(m._ctx) == b"bad read geometry"
    assert lib.bmbs_map_se_device(m._ctx, p, p + 256, 50, 64, 0, *dev) == 0
    m.sync()
    m.close()


# ---- 8. one split device call with lengths ----------------------------------------------------------------------------------------------------
def test_split_device_call_of_pairs_with_lengths_matches_oracle(env, D):
    """bmbs_map_pe_var_device, nine chunks on three lanes: each chunk's lengths are re-laid into its lane's own array as [m first
    mates][m second mates] behind the lane's previous chunk"""
    import torch
    from bitmapperbs_amd import capi
    d = D["pe"]
    L, stride = 100, 112

    def dev(a):
        t = torch.zeros((N, stride), dtype=torch.uint8, device="cuda")
        t[:, :a.shape[1]] = torch.from_numpy(_c(a)).cuda()
        return t
    rows = [dev(x) for x in (d["seq"][0], d["qual"][0], d["seq"][1], d["qual"][1])]
    d_len = torch.from_numpy(np.concatenate(d["len"]).view(np.int16)).cuda()
    m = _mapper(env, SPLIT)
    ops = m.max_cigar_ops(L)
    res = torch.zeros((2 * N, 32), dtype=torch.uint8, device="cuda")
    cig = torch.zeros((2 * N * ops,), dtype=torch.int32, device="cuda")
    rc = capi.lib().bmbs_map_pe_var_device(m._ctx, *[r.data_ptr() for r in rows], d_len.data_ptr(), L, stride, N, res.data_ptr(), cig.data_ptr(), 2 * N * ops)
    assert rc == 0
    m.sync()
    got = res.cpu().numpy().view(capi.RESULT_DTYPE).reshape(-1)
    recs, ost = d["oracle"]
    bad = compare_pe(got, cig.cpu().numpy().view(np.uint32), recs, *d["len"])
    assert not bad, bad[:5]
    assert got["cigar_off"].max() >= (N - CHUNK) * 2 * ops
    assert (m.stats() == ost).all(), (m.stats(), ost)
    m.close()
