"""-m gpu: bmbs_map_se_fastq / bmbs_map_pe_fastq (include/bmbs.h): the host hands over FASTQ text and where its
sequence and quality lines are, the device cuts the rows.  Records and CIGAR words are those of the row calls on the same reads
(upper-cased bases, qualities padded with blanks); refusals, the empty batch and a CIGAR pool one word too small."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import env        # noqa: F401  (the module's genome and index)

pytestmark = pytest.mark.gpu

OK, EINVAL, ENOMEM = 0, -22, -12
L_MAX = 120


def _records(r, n, mixed, seed, mate):
    """n FASTQ records the way _odd_fastq (test_gpu_parity.py) writes them: lower-case bases in some, a quality line shorter than its
    sequence in some; mixed: lengths 30..120"""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        Li = int(rng.integers(30, L_MAX + 1)) if mixed and i else L_MAX          # (record 0: L_max, so that the row calls see the same longest read)
        s = r["seq"][i, :Li].tobytes(); q = r["qual"][i, :Li].tobytes()
        if mixed and i % 7 == 0: s = s.lower()
        if mixed and i % 11 == 0: q = q[:max(1, Li - 5)]
        nm = b"@read%d" % i + (b" extra/%d" % mate if i % 3 == 0 else b"/%d" % mate if i % 3 == 1 else b"")
        recs.append((nm, s, q))
    return recs


class View:
    """the text of the records, its line index computed on the host, and the rows a row call takes for the same reads"""

    def __init__(self, recs):
        from bitmapperbs_amd import capi
        n = len(recs)
        self.n = n
        self.seq_off = np.zeros(n, dtype=np.uint32); self.qual_off = np.zeros(n, dtype=np.uint32)
        self.seq_len = np.zeros(n, dtype=np.uint16); self.qual_len = np.zeros(n, dtype=np.uint16)
        self.seq = np.zeros((n, L_MAX), dtype=np.uint8); self.qual = np.zeros((n, L_MAX), dtype=np.uint8)
        parts = []; at = 0
        for i, (nm, s, q) in enumerate(recs):
            self.seq_off[i] = at + len(nm) + 1; self.qual_off[i] = at + len(nm) + 1 + len(s) + 3
            self.seq_len[i] = len(s); self.qual_len[i] = len(q)
            self.seq[i, :len(s)] = np.frombuffer(s.upper(), dtype=np.uint8)
            self.qual[i, :len(s)] = np.frombuffer(q + b" " * (len(s) - len(q)), dtype=np.uint8)
            rec = nm + b"\n" + s + b"\n+\n" + q + b"\n"
            parts.append(rec); at += len(rec)
        self.raw = b"".join(parts)
        self.text = np.frombuffer(self.raw, dtype=np.uint8)
        self.names = [nm for nm, _, _ in recs]
        self.c = capi.FastqView(capi.ptr(self.text), self.text.size, capi.ptr(self.seq_off), capi.ptr(self.qual_off), capi.ptr(self.seq_len),
                                capi.ptr(self.qual_len))


def _call(m, views, n, L_max, uniform, pbat=0, cap=None):
    """-> (rc, results, pool, used) of bmbs_map_se_fastq (one view) / bmbs_map_pe_fastq (two)"""
    from bitmapperbs_amd import capi
    n2 = n * len(views)
    res = np.zeros(max(n2, 1), dtype=capi.RESULT_DTYPE)
    cap = max(1, n2 * m.max_cigar_ops(min(L_max, 998))) if cap is None else cap
    pool = np.zeros(max(cap, 1), dtype=np.uint32)
    used = C.c_int64(-1)
    v = [C.byref(x) if x is not None else None for x in views]
    if len(views) == 1:
        rc = m._lib.bmbs_map_se_fastq(m._ctx, v[0], n, L_max, uniform, pbat, capi.ptr(res), capi.ptr(pool), cap, C.byref(used))
    else:
        rc = m._lib.bmbs_map_pe_fastq(m._ctx, v[0], v[1], n, L_max, uniform, capi.ptr(res), capi.ptr(pool), cap, C.byref(used))
    return rc, res[:n2], pool, used.value


def _same(got, want):
    rc, res, pool, used = got
    eres, epool = want
    assert rc == OK
    assert (eres["status"] == 1).sum() > res.size // 4                  # the batch really maps
    assert res.tobytes() == eres.tobytes()
    assert used == epool.size and used > 0
    assert np.array_equal(pool[:used], epool)


@pytest.fixture(scope="module")
def se(env):
    from bitmapperbs_amd import synth
    r = synth.make_reads_se(env["chroms"], n=600, L=L_MAX, seed=41, sub=0.03, indel=0.002, qual="random", n_rate=0.002)
    return dict(r=r, mixed=View(_records(r, 600, True, 6, 1)), uniform=View(_records(r, 600, False, 6, 1)))


@pytest.fixture(scope="module")
def pe(env):
    from bitmapperbs_amd import synth
    m1, m2 = synth.make_reads_pe(env["chroms"], n=400, L=L_MAX, seed=5, sub=0.03, indel=0.003, qual="random")
    return dict(mixed=(View(_records(m1, 400, True, 7, 1)), View(_records(m2, 400, True, 8, 2))),
                uniform=(View(_records(m1, 400, False, 7, 1)), View(_records(m2, 400, False, 8, 2))))


@pytest.fixture()
def m(env):
    from bitmapperbs_amd import mapper
    mm = mapper.Mapper(env["ix"], 0)
    yield mm
    mm.close()


def test_se_view_equals_the_row_calls(env, se, m):
    v = se["mixed"]
    assert len({int(x) % 16 for x in v.seq_len}) == 16 and (v.qual_len < v.seq_len).any()
    _same(_call(m, [v.c], 600, L_MAX, 0), m.map_se_var(v.seq, v.qual, v.seq_len))
    u = se["uniform"]
    _same(_call(m, [u.c], 600, L_MAX, 1), m.map_se(u.seq, u.qual, L_MAX))


def _rc_rows(v):
    """the rows of a --pbat library: every read reverse-complemented, its padded qualities mirrored"""
    from bitmapperbs_amd import synth
    seq = np.zeros_like(v.seq); qual = np.zeros_like(v.qual)
    for i in range(v.n):
        Li = int(v.seq_len[i])
        seq[i, :Li] = synth.revcomp(v.seq[i, :Li]); qual[i, :Li] = v.qual[i, :Li][::-1]
    return seq, qual


def test_se_view_pbat_equals_the_text_call(env, se, m):
    """pbat=1 against the text call with BMBS_TEXT_PBAT: the SAM lines the host formatter makes of the view call's records are the
    ones the text call prints.  The reads are written reverse-complemented, as a --pbat library has them, so that they map"""
    from bitmapperbs_amd import mapper, synth
    recs = [(nm, synth.revcomp(np.frombuffer(s.upper(), dtype=np.uint8)).tobytes(), q) for nm, s, q in _records(se["r"], 600, True, 6, 1)]
    v = View(recs)
    rc, res, pool, used = _call(m, [v.c], 600, L_MAX, 0, pbat=1)
    assert rc == OK
    _same((rc, res, pool, used), m.map_se_var(*_rc_rows(v), v.seq_len))          # (the rows the device cut are the mirrored ones)
    M = mapper.Mapper
    got = m.map_text(v.raw, 600, flags=M.TEXT_PBAT | M.TEXT_UNMAPPED).decode().splitlines()
    exp = []
    for i in range(600):
        x = res[i]; Li = int(v.seq_len[i])
        nm = v.names[i][1:].decode().split(" ")[0].split("/")[0]
        s = v.seq[i, :Li]; q = v.qual[i, :Li]
        if int(x["status"]) == 1:
            if not int(x["flag"]) & 16:                       # mapped as the reverse complement of the text: flag 16 prints the text as it is
                s = mapper._COMP[s][::-1]; q = q[::-1]
            exp.append("%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\tNM:i:%d" % (nm, int(x["flag"]), env["ix"].chrom_names[int(x["chrom"])], int(x["pos"]),
                       int(x["mapq"]), mapper.cigar_text(x, pool, Li), s.tobytes().decode(), q.tobytes().decode(), int(x["nm"])))
        elif int(x["status"]) != 2:
            exp.append("%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s" % (nm, s.tobytes().decode(), q.tobytes().decode()))
    assert got == exp


def test_pe_view_equals_the_row_calls(env, pe, m):
    a, b = pe["mixed"]
    _same(_call(m, [a.c, b.c], 400, L_MAX, 0), m.map_pe_var(a.seq, a.qual, b.seq, b.qual, a.seq_len, b.seq_len))
    a, b = pe["uniform"]
    _same(_call(m, [a.c, b.c], 400, L_MAX, 1), m.map_pe(a.seq, a.qual, b.seq, b.qual, L_MAX))


def test_view_refusals_empty_batch_and_small_pool(env, se, pe, m):
    from bitmapperbs_amd import capi
    v = se["mixed"]
    assert int(v.seq_len[:8].max()) > 100

    def refused(what, n=8, L_max=L_MAX, **change):
        """one field of a copy of the view (or one element of one of its arrays) changed"""
        arrs = {k: getattr(v, k).copy() for k in ("seq_off", "qual_off", "seq_len", "qual_len")}
        text_bytes = v.text.size
        for k, val in change.items():
            if k == "text": continue
            if val is None: arrs[k] = None
            else: arrs[k][3] = val
        c = capi.FastqView(capi.ptr(v.text) if change.get("text", 1) else None, text_bytes,
                           *[capi.ptr(arrs[k]) if arrs[k] is not None else None for k in ("seq_off", "qual_off", "seq_len", "qual_len")])
        for views in ([c], [v.c, c], [c, v.c]):
            rc = _call(m, views, n, L_max, 0)[0]
            assert rc == EINVAL, (what, len(views), rc)
            assert m._lib.bmbs_last_error(m._ctx)
    refused("NULL text", text=0)
    refused("NULL seq_off", seq_off=None)
    refused("NULL qual_len", qual_len=None)
    refused("sequence line beyond the text", seq_off=v.text.size - int(v.seq_len[3]) + 1)
    refused("quality line beyond the text", qual_off=v.text.size - int(v.qual_len[3]) + 1)
    refused("seq_len 0", seq_len=0, qual_len=0)
    refused("seq_len > L_max", L_max=100)
    refused("qual_len > seq_len", qual_len=int(v.seq_len[3]) + 1)
    refused("L_max 999", L_max=999)
    assert _call(m, [None], 8, L_MAX, 0)[0] == EINVAL and _call(m, [v.c, None], 8, L_MAX, 0)[0] == EINVAL
    # n = 0: nothing to do, nothing used
    for views in ([v.c], [v.c, v.c]):
        rc, _, _, used = _call(m, views, 0, L_MAX, 0)
        assert (rc, used) == (OK, 0)
    # a pool one word too small
    for views, n in (([v.c], 600), ([x.c for x in pe["mixed"]], 400)):
        rc, _, _, used = _call(m, views, n, L_MAX, 0)
        assert rc == OK and used > 1
        assert _call(m, views, n, L_MAX, 0, cap=used)[0] == OK
        rc, _, _, got = _call(m, views, n, L_MAX, 0, cap=used - 1)
        assert rc == ENOMEM and got == 0
        assert b"host cigar pool too small" in m._lib.bmbs_last_error(m._ctx)
