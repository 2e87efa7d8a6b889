"""Packed quality classes (bmbs_qual_classes, bmbs_pack_quals, bmbs_map_{se,pe}_packedq): a 4-bit penalty class per base goes over
the link instead of the quality byte.  Host arithmetic (class table, packer) without a GPU; on the MI355X the new entry points against
the oracle on the original bytes and against bmbs_map_*_packed, field by field."""
import ctypes as C

import numpy as np
import pytest

import orc

EINVAL = -22
MAX_READ = 998

# (mp_max, mp_min, q_base) -> (distinct penalties over all 256 bytes, over the bytes >= q_base): evaluated on the CPU with the reference's
# formula (MismatchPenaltyByQuality, ksw.h:148-161)
PARAM_SETS = {
    "defaults": ((6, 2, 33), (8, 5)),
    "phred64": ((6, 2, 64), (11, 5)),
    "mp_max10": ((10, 2, 33), (15, 9)),
    "mp_max11": ((11, 2, 33), (17, 10)),
    "mp_max17": ((17, 2, 33), (28, 16)),
    "mp_max17_phred64": ((17, 2, 64), (40, 16)),
    "mp_max20_min0": ((20, 0, 33), (37, 21)),
    "flat": ((4, 4, 33), (1, 1)),
    "inverted": ((2, 6, 33), (8, 5)),
}


def penalty(mp_max, mp_min, q_base, b):
    """MismatchPenaltyByQuality restated: every step in IEEE double, the product truncated toward zero"""
    phred = min(float(b - q_base), 40.0) / 40
    return int(phred * (mp_max - mp_min)) + mp_min


def pen_table(mp_max, mp_min, q_base):
    return np.array([penalty(mp_max, mp_min, q_base, b) for b in range(256)], dtype=np.int64)


def prm(mp_max=6, mp_min=2, q_base=33):
    from bitmapperbs_amd import capi
    return capi.default_params(mp_max=mp_max, mp_min=mp_min, q_base=q_base)


def unpack(qrows, L):
    """class of base j of every row: bits 4 (j % 16) .. 4 (j % 16) + 3 of word j / 16"""
    sh = (np.arange(16, dtype=np.uint64) * np.uint64(4))[None, None, :]
    nib = (qrows[:, :, None] >> sh) & np.uint64(15)
    return nib.reshape(qrows.shape[0], -1)[:, :L].astype(np.uint8)


# ---- 1. the class table against the reference's formula -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PARAM_SETS))
def test_class_table_follows_the_reference_formula(name):
    from bitmapperbs_amd import mapper
    (mp_max, mp_min, q_base), (n_all, n_ord) = PARAM_SETS[name]
    pen = pen_table(mp_max, mp_min, q_base)
    distinct = sorted(set(pen.tolist()), reverse=True)
    assert (len(distinct), len(set(pen[q_base:].tolist()))) == (n_all, n_ord)
    class_of, penalty_of = mapper.qual_classes(prm(mp_max, mp_min, q_base))
    assert penalty_of.size == min(16, n_all)
    assert (np.diff(penalty_of) < 0).all()                       # strictly descending: class 0 is the largest penalty
    assert penalty_of.tolist() == distinct[:16]
    packable = np.isin(pen, distinct[:16])
    assert ((class_of != 0xFF) == packable).all()
    assert (penalty_of[class_of[packable]] == pen[packable]).all()
    assert bool(packable.all()) == (n_all <= 16)
    # every ordinary quality (byte >= q_base) has a class exactly when the penalties span at most 15
    assert bool((class_of[q_base:] != 0xFF).all()) == (abs(mp_max - mp_min) <= 15)


def test_class_table_defaults_when_params_is_null():
    from bitmapperbs_amd import mapper
    a, pa = mapper.qual_classes(None)
    b, pb = mapper.qual_classes(prm())
    assert (a == b).all() and (pa == pb).all() and pa.tolist() == [6, 5, 4, 3, 2, 1, 0, -1]


# ---- 2. the packer: layout and errors -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 15, 16, 17, 150, 998])
def test_packer_layout(L):
    from bitmapperbs_amd import mapper
    rng = np.random.default_rng(L)
    n = 9000                                                      # more than 4096 rows: several threads really run
    stride = L + int(rng.integers(0, 20))
    qual = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    class_of, _ = mapper.qual_classes(None)
    Wq = (L + 15) // 16
    # uniform lengths, rows exactly Wq words apart
    q = mapper.pack_quals(None, qual, L)
    assert q.shape == (n, Wq) and q.dtype == np.uint64
    assert (unpack(q, L) == class_of[qual[:, :L]]).all()
    assert (unpack(q, Wq * 16)[:, L:] == 0).all()                 # nibbles past the length
    # per-read lengths, rows further apart than needed, 1 thread and 8 threads
    lens = rng.integers(1, L + 1, n).astype(np.uint16)
    lens[:10] = L; lens[10:20] = 1
    q1 = mapper.pack_quals(None, qual, L, lens, qwords=Wq + 3, threads=1)
    q8 = mapper.pack_quals(None, qual, L, lens, qwords=Wq + 3, threads=8)
    assert q1.shape == (n, Wq + 3) and (q1 == q8).all()
    want = class_of[qual[:, :L]].copy()
    want[np.arange(L)[None, :] >= lens[:, None]] = 0
    full = unpack(q1, (Wq + 3) * 16)
    assert (full[:, :L] == want).all() and (full[:, L:] == 0).all()


def test_packer_reports_the_first_row_that_cannot_be_packed():
    from bitmapperbs_amd import capi, mapper
    lib = capi.lib()
    rng = np.random.default_rng(3)
    n, L = 20000, 100
    wide = prm(mp_max=20, mp_min=0)                               # Phred 0..40 takes 21 penalties here: the five smallest have no class
    class_of, _ = mapper.qual_classes(wide)
    ok_bytes = np.nonzero(class_of != 0xFF)[0].astype(np.uint8)
    bad_bytes = np.nonzero(class_of[33:74] == 0xFF)[0] + 33
    assert len(set(pen_table(20, 0, 33)[bad_bytes].tolist())) == 21 - 16 and ok_bytes.size > 16
    qual = ok_bytes[rng.integers(0, ok_bytes.size, (n, L))]
    mapper.pack_quals(wide, qual, L)                              # packs
    qual[17003, 99] = bad_bytes[0]; qual[9111, 0] = bad_bytes[-1]; qual[9111, 57] = bad_bytes[1]
    for threads in (1, 8):
        with pytest.raises(ValueError, match="row 9111 "):
            mapper.pack_quals(wide, qual, L, threads=threads)
    mapper.pack_quals(None, qual, L)                              # the same bytes under the defaults: every byte has a class
    # a byte past a read's length is not looked at
    lens = np.full(n, L, dtype=np.uint16); lens[9111] = 0; lens[17003] = 99
    qual[9111] = ok_bytes[0]
    with pytest.raises(ValueError, match="row 9111 "):            # ... and a length of 0 makes the row the bad row
        mapper.pack_quals(wide, qual, L, lens)
    lens[9111] = 5; lens[12000] = L + 1
    with pytest.raises(ValueError, match="row 12000 "):
        mapper.pack_quals(wide, qual, L, lens)
    lens[12000] = L
    mapper.pack_quals(wide, qual, L, lens)
    # argument checks
    q = np.zeros((4, 8), dtype=np.uint64); a = np.full((4, 120), 70, dtype=np.uint8)
    bad = C.c_int64(7)
    call = lambda qp, op, L_, stride, qw: lib.bmbs_pack_quals(None, qp, L_, stride, 4, None, op, qw, 1, C.byref(bad))
    assert call(capi.ptr(a), capi.ptr(q), 100, 120, 8) == 0 and bad.value == -1
    assert call(None, capi.ptr(q), 100, 120, 8) == EINVAL
    assert call(capi.ptr(a), None, 100, 120, 8) == EINVAL
    assert call(capi.ptr(a), capi.ptr(q), 100, 120, 6) == EINVAL          # qwords < Wq = 7
    assert call(capi.ptr(a), capi.ptr(q), 120, 119, 8) == EINVAL          # stride < L_max
    assert call(capi.ptr(a), capi.ptr(q), MAX_READ + 1, 2000, 80) == EINVAL
    assert call(capi.ptr(a), capi.ptr(q), 0, 120, 8) == EINVAL
    assert lib.bmbs_pack_quals(None, capi.ptr(a), 100, 120, 4, None, capi.ptr(q), 8, 1, None) == 0        # bad_row may be NULL
    assert lib.bmbs_qual_classes(None, None, None, None) == EINVAL


# ---- 3. the classes lose nothing the mapping path reads ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lo,hi", [("defaults", 0, 256), ("phred64", 66, 105), ("mp_max10", 35, 74), ("mp_max17", 35, 74), ("inverted", 35, 74)])
def test_expanded_classes_give_the_penalties_of_the_original_bytes(name, lo, hi):
    """what k_qual_expand writes for class c is rep[c], the smallest byte with that penalty: expanding the packed words that way and
    looking the bytes up in the penalty table gives the penalty of every original byte"""
    from bitmapperbs_amd import mapper
    (mp_max, mp_min, q_base), _ = PARAM_SETS[name]
    p = prm(mp_max, mp_min, q_base)
    pen = pen_table(mp_max, mp_min, q_base)
    class_of, penalty_of = mapper.qual_classes(p)
    rep = np.array([int(np.nonzero(pen == v)[0][0]) for v in penalty_of], dtype=np.uint8)
    rng = np.random.default_rng(11)
    L = 151
    qual = rng.integers(lo, hi, (5000, L), dtype=np.uint8)
    q = mapper.pack_quals(p, qual, L, qwords=12)
    expanded = rep[unpack(q, L)]
    assert (pen[expanded] == pen[qual]).all()
    assert (expanded <= qual).all()


# ---- on the MI355X ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env(tmp_path_factory):
    """a repeat-rich 3-chromosome genome + product-built index + both handles (the recipe of test_gpu_parity's fixture)"""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bitmapperbs_amd import synth, mapper
    from common import plant_repeats
    wd = tmp_path_factory.mktemp("gpuq")
    names, chroms = synth.make_genome(1_500_000, 3, seed=77)
    plant_repeats(chroms, seed=78)
    fa = str(wd / "g.fa")
    synth.write_fasta(fa, names, chroms)
    mapper.Index.build(fa, fa, threads=8)
    return dict(fa=fa, chroms=chroms, ix=mapper.Index(fa), oix=orc.OrcIndex(fa), wd=str(wd))


FIELDS = ("status", "chrom", "pos", "flag", "mapq", "nm", "score", "n_cigar", "tlen", "path", "n_cand")


def same_records(res, pool, res2, pool2):
    """every field of every record, and the CIGAR operations of every record that has some"""
    bad = []
    assert res.size == res2.size
    for f in FIELDS:
        d = np.nonzero(res[f] != res2[f])[0]
        if d.size:
            bad.append((f, int(d[0]), int(res[f][d[0]]), int(res2[f][d[0]])))
    has = np.nonzero(res["n_cigar"] > 0)[0]
    d = has[res["cigar_off"][has] != res2["cigar_off"][has]]
    if d.size:
        bad.append(("cigar_off", int(d[0])))
    if not bad:
        for i in has:
            a, k = int(res[i]["cigar_off"]), int(res[i]["n_cigar"])
            if not (pool[a:a + k] == pool2[a:a + k]).all():
                bad.append(("cigar", int(i)))
                break
    return bad


def run_se(env, m, oprm, seq, qual, L, lens, qwords=None, oracle=True, min_mapped=None):
    """the batch through bmbs_map_se_packedq; against the oracle on the original bytes (oracle=True) and against bmbs_map_se_packed"""
    from bitmapperbs_amd import mapper
    from test_gpu_parity import compare_records
    n = seq.shape[0]
    rows = mapper.Mapper.pack_rows(seq, L, lens)
    qrows = m.pack_quals(qual, L, lens, qwords=qwords)
    m.reset_stats()
    res, pool = m.map_se_packedq(rows, qrows, L, lens)
    st = m.stats().copy()
    if oracle:
        if lens is None:
            recs, ost, _ = env["oix"].map_se(oprm, seq, qual, L)
        else:
            recs, ost, _ = env["oix"].map_se_var(oprm, seq, qual, lens)
        assert (recs["status"] == 1).sum() > (n // 2 if min_mapped is None else min_mapped)
        bad = compare_records(res, pool, recs, L if lens is None else lens)
        assert not bad, bad[:5]
        assert (st == ost).all(), (st, ost)
    m.reset_stats()
    res2, pool2 = m.map_se_packed(rows, qual, L, lens)
    assert (res2["status"] == 1).sum() > (n // 2 if min_mapped is None else min_mapped)
    bad = same_records(res, pool, res2, pool2)
    assert not bad, bad
    assert (st == m.stats()).all(), (st, m.stats())
    return res, pool


def run_pe(env, m, oprm, s1, q1, s2, q2, L, l1, l2, qwords=None, pwords=None, oracle=True):
    from bitmapperbs_amd import mapper
    from test_gpu_parity import compare_pe
    n = s1.shape[0]
    r1 = mapper.Mapper.pack_rows(s1, L, l1, pwords=pwords); r2 = mapper.Mapper.pack_rows(s2, L, l2, pwords=pwords)
    k1 = m.pack_quals(q1, L, l1, qwords=qwords); k2 = m.pack_quals(q2, L, l2, qwords=qwords)
    m.reset_stats()
    res, pool = m.map_pe_packedq(r1, r2, k1, k2, L, l1, l2)
    st = m.stats().copy()
    if oracle:
        if l1 is None:
            recs, ost, _ = env["oix"].map_pe(oprm, s1, q1, s2, q2, L)
            bad = compare_pe(res, pool, recs, L, L)
        else:
            recs, ost, _ = env["oix"].map_pe_var(oprm, s1, q1, s2, q2, l1, l2)
            bad = compare_pe(res, pool, recs, l1, l2)
        assert (recs["status"] == 1).sum() > n // 2
        assert not bad, bad[:5]
        assert (st == ost).all(), (st, ost)
    m.reset_stats()
    res2, pool2 = m.map_pe_packed(r1, r2, q1, q2, L, l1, l2)
    assert (res2["status"] == 1).sum() > n // 2                  # (two records per pair: more than a quarter of the pairs)
    bad = same_records(res, pool, res2, pool2)
    assert not bad, bad
    assert (st == m.stats()).all(), (st, m.stats())
    return res, pool


# ---- 4. / 8. the seven cases of the packed-rows test through the new entry points -----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["se150", "se_mixed", "se998", "pe100_fast", "pe150_sensitive", "pe_mixed", "pe_chunks"])
def test_packed_quality_classes_match_oracle(case, env, monkeypatch):
    """bmbs_map_se_packedq / bmbs_map_pe_packedq on random Phred 2..40 qualities: the oracle's records, CIGARs and mapstats on the
    original bytes, and every field and CIGAR of bmbs_map_*_packed on the same rows.  Lengths that are no multiple of 16 (150, 100,
    125, 998 and the mixed ones); se_mixed and the pairs of up to 150 bases hand their class rows over two words further apart than
    they need to be"""
    from bitmapperbs_amd import synth, mapper
    from test_gpu_parity import _trim, _sprinkle_n
    rng = np.random.default_rng(5)
    if case.startswith("se"):
        L = 998 if case == "se998" else 150
        n = 1500 if case == "se998" else 20000
        r = synth.make_reads_se(env["chroms"], n=n, L=L, seed=51, sub=0.02, indel=0.002, qual="random", n_rate=0.002)
        lens = None
        seq, qual = r["seq"], r["qual"]
        if case == "se_mixed":
            lens = rng.integers(20, L + 1, n).astype(np.uint16); lens[:500] = L
            seq, qual = _trim(seq, lens), _trim(qual, lens)
        m = mapper.Mapper(env["ix"], 0, e_f=0.08)
        run_se(env, m, orc.params(e_f=0.08), seq, qual, L, lens, qwords=(L + 15) // 16 + 2 if case == "se_mixed" else None)
        m.close()
        return
    p = dict(sensitive=1) if case == "pe150_sensitive" else dict()
    L = 150 if case in ("pe150_sensitive", "pe_chunks") else 100 if case == "pe100_fast" else 125
    n = 12000
    if case == "pe_chunks":
        monkeypatch.setenv("BMBS_LANES", "3"); monkeypatch.setenv("BMBS_SPLIT_MIN", "1000")
    m1, m2 = synth.make_reads_pe(env["chroms"], n=n, L=L, seed=52, sub=0.02, indel=0.002, qual="random", ins_hi=480)
    l1 = l2 = None
    s1, q1, s2, q2 = m1["seq"], m1["qual"], m2["seq"], m2["qual"]
    if case == "pe_mixed":
        l1 = rng.integers(30, L + 1, n).astype(np.uint16); l2 = rng.integers(30, L + 1, n).astype(np.uint16)
        l1[:2000] = L; l2[:2000] = L
        s1, q1, s2, q2 = _trim(s1, l1), _trim(q1, l1), _trim(s2, l2), _trim(q2, l2)
    s1 = _sprinkle_n(rng, s1, l1); s2 = _sprinkle_n(rng, s2, l2)
    m = mapper.Mapper(env["ix"], 0, **p)
    run_pe(env, m, orc.params(**p), s1, q1, s2, q2, L, l1, l2, qwords=(L + 15) // 16 + 2, pwords=12)
    m.close()


# ---- 5. other parameter sets against the oracle --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["phred64", "mp_max10_min1"])
def test_packed_quality_classes_under_other_parameters(name, env):
    from bitmapperbs_amd import synth, mapper
    p = dict(q_base=64) if name == "phred64" else dict(mp_max=10, mp_min=1)
    shift = 31 if name == "phred64" else 0                       # Phred 2..40 as Phred+64 characters
    r = synth.make_reads_se(env["chroms"], n=20000, L=150, seed=61, sub=0.03, indel=0.002, qual="random", n_rate=0.002)
    m = mapper.Mapper(env["ix"], 0, **p)
    _, pen = m.qual_classes()
    assert pen.size == min(16, len(set(pen_table(m.params.mp_max, m.params.mp_min, m.params.q_base).tolist())))
    run_se(env, m, orc.params(**p), r["seq"], (r["qual"] + shift).astype(np.uint8), 150, None)
    m1, m2 = synth.make_reads_pe(env["chroms"], n=12000, L=100, seed=62, sub=0.03, indel=0.002, qual="random", ins_hi=480)
    run_pe(env, m, orc.params(**p), m1["seq"], (m1["qual"] + shift).astype(np.uint8), m2["seq"], (m2["qual"] + shift).astype(np.uint8), 100, None, None)
    m.close()


# ---- 6. bytes a FASTQ file does not hold: the unchanged byte path is the reference ---------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["all_bytes", "phred33_read_as_phred64"])
def test_packed_quality_classes_on_bytes_outside_the_ordinary_range(name, env):
    """qualities drawn from all of 0..255 under the defaults (' ' = 32, the reader's padding of a short quality line, and bytes below
    q_base, whose classes carry penalties below mp_min), and Phred+33 data mapped with q_base = 64: every field and CIGAR of
    bmbs_map_*_packed on the bytes"""
    from bitmapperbs_amd import synth, mapper
    rng = np.random.default_rng(71)
    p = dict() if name == "all_bytes" else dict(q_base=64)
    r = synth.make_reads_se(env["chroms"], n=20000, L=150, seed=72, sub=0.03, indel=0.002, qual="random", n_rate=0.002)
    m1, m2 = synth.make_reads_pe(env["chroms"], n=12000, L=100, seed=73, sub=0.03, indel=0.002, qual="random", ins_hi=480)
    q, q1, q2 = r["qual"], m1["qual"], m2["qual"]
    if name == "all_bytes":
        q, q1, q2 = (rng.integers(0, 256, a.shape, dtype=np.uint8) for a in (q, q1, q2))
        q[:, 140:] = 32                                           # a padded quality line
    m = mapper.Mapper(env["ix"], 0, **p)
    class_of, _ = m.qual_classes()
    assert (class_of != 0xFF).all()
    run_se(env, m, None, r["seq"], q, 150, None, oracle=False)
    run_pe(env, m, None, m1["seq"], q1, m2["seq"], q2, 100, None, None, oracle=False)
    m.close()


# ---- 7. a chunk issued again with exact sizes finds its byte rows in place ----------------------------------------------------------
@pytest.mark.gpu
def test_packed_quality_classes_survive_the_repeat_with_exact_sizes(env, monkeypatch):
    from bitmapperbs_amd import synth, mapper
    from test_gpu_parity import compare_records, compare_pe, _se_reads
    monkeypatch.setenv("BMBS_CAP_SCALE", "0.02")
    monkeypatch.setenv("BMBS_LANES", "2")
    monkeypatch.setenv("BMBS_SPLIT_MIN", "3000")
    m = mapper.Mapper(env["ix"], 0, e_f=0.08)
    tot = np.zeros(5, dtype=np.int64)
    for seed, sub in [(601, 0.005), (602, 0.05), (603, 0.05)]:
        r = _se_reads(env, seed, sub)
        res, pool = m.map_se_packedq(mapper.Mapper.pack_rows(r["seq"], 150), m.pack_quals(r["qual"], 150), 150)
        recs, ost, _ = env["oix"].map_se(orc.params(e_f=0.08), r["seq"], r["qual"], 150)
        assert (recs["status"] == 1).sum() > 12000
        assert not compare_records(res, pool, recs, 150)
        tot += ost
        assert (m.stats() == tot).all()
    assert m.retries() > 0
    m.close()
    for sensitive in (0, 1):
        m = mapper.Mapper(env["ix"], 0, sensitive=sensitive)
        tot = np.zeros(5, dtype=np.int64)
        for seed, sub in [(611, 0.005), (612, 0.05), (613, 0.06)]:
            m1, m2 = synth.make_reads_pe(env["chroms"], n=9000, L=100, seed=seed + sensitive, sub=sub, indel=0.002, qual="random")
            P = mapper.Mapper.pack_rows
            res, pool = m.map_pe_packedq(P(m1["seq"], 100), P(m2["seq"], 100), m.pack_quals(m1["qual"], 100), m.pack_quals(m2["qual"], 100), 100)
            recs, ost, _ = env["oix"].map_pe(orc.params(sensitive=sensitive), m1["seq"], m1["qual"], m2["seq"], m2["qual"], 100)
            assert (recs["status"] == 1).sum() > 4500
            assert not compare_pe(res, pool, recs, 100)
            tot += ost
            assert (m.stats() == tot).all()
        assert m.retries() > 0
        m.close()


@pytest.mark.gpu
def test_packedq_entry_points_refuse_bad_arguments(env):
    from bitmapperbs_amd import capi, mapper
    m = mapper.Mapper(env["ix"], 0)
    lib = capi.lib()
    rows = np.zeros((4, 8), dtype=np.uint64); q = np.zeros((4, 10), dtype=np.uint64)
    res = np.zeros(8, dtype=capi.RESULT_DTYPE); pool = np.zeros(4096, dtype=np.uint32); used = C.c_int64(0)
    a = (capi.ptr(res), capi.ptr(pool), 4096, C.byref(used))
    assert lib.bmbs_map_se_packedq(m._ctx, capi.ptr(rows), 8, None, 10, None, 150, 4, *a) == EINVAL
    assert lib.bmbs_map_se_packedq(m._ctx, capi.ptr(rows), 8, capi.ptr(q), 9, None, 150, 4, *a) == EINVAL          # qwords < Wq = 10
    assert b"qwords" in lib.bmbs_last_error(m._ctx)
    assert lib.bmbs_map_pe_packedq(m._ctx, capi.ptr(rows), capi.ptr(rows), 8, capi.ptr(q), None, 10, None, None, 150, 4, *a) == EINVAL
    assert lib.bmbs_map_pe_packedq(m._ctx, capi.ptr(rows), capi.ptr(rows), 8, capi.ptr(q), capi.ptr(q), 10, None, None, 999, 4, *a) == EINVAL
    assert lib.bmbs_map_se_packedq(m._ctx, capi.ptr(rows), 8, capi.ptr(q), 10, None, 150, 0, *a) == 0 and used.value == 0
    m.close()
