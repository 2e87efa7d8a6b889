"""The gapped alignment stage restated in plain numpy, for a batch of jobs of one read length and one threshold:
fast_recalculate_bs_Cigar (ksw.cpp:2578-2876) = the err == 0 exit, try_cigar_without_path (:2515-2570), else
ksw_semi_global_quality_back (:1850-2045) followed by the leading / trailing I -> M rewrite and the NM recount.

Written from ksw.cpp and the scoring matrix of Schema.cpp:830-850, cell by cell in the order the reference visits them; the one
liberty is that every scalar of the reference is a vector over the jobs of the batch here (all jobs share L and k, so they share
the loop bounds).  All arithmetic is 64-bit.  The reference stores its matrix in int8_t; this keeps the penalties as they are
given, as the oracle and the device do.

Besides the results it returns, per job, the smallest and the largest H / E / F value the band ever forms (`lo`, `hi`), the diagonal
candidate M = H(i-1, j-1) + S(i, j) included (the kernels form it in the same width): what decides whether the job fits a narrower
integer.  Values that descend from the "minus infinity" the band is fenced with are not counted."""
import numpy as np

MINUS_INF = -0x40000000
_FENCE = MINUS_INF // 2          # anything below descends from MINUS_INF, not from a score

NT4 = np.full(256, 4, dtype=np.int64)
for _i, _c in enumerate(b"ACGT"):
    NT4[_c] = _i
    NT4[_c + 32] = _i


def score_matrix(mp_max, mp_min, np_pen):
    """mat / mat_diff of Schema.cpp:830-850 as [read base][window base]: row 4 and column 4 are N, read T over window C is a match"""
    mat = np.zeros((5, 5), dtype=np.int64)
    diff = np.zeros((5, 5), dtype=np.int64)
    for i in range(4):
        for j in range(4):
            diff[i, j] = 0 if i == j else mp_max - mp_min
            mat[i, j] = 0 if i == j else -mp_min
        mat[i, 4] = -np_pen
    mat[4, :] = -np_pen
    diff[3, 1] = 0
    mat[3, 1] = 0
    return mat, diff


def mismatch_penalty(mp_max, mp_min, q_base, q):
    """MismatchPenaltyByQuality (ksw.h:148-161), q an array of quality bytes"""
    phred = np.minimum(q.astype(np.float64) - q_base, 40.0) / 40
    return (phred * (mp_max - mp_min)).astype(np.int64) + mp_min          # astype truncates toward zero, as (int) does


def _ops_text(ops):
    return "".join("%d%s" % (n, "MDISH"[op]) for op, n in ops)


def align_batch(prm, windows, reads, quals, k, end_in, err_in, forward, reverse_quality=None):
    """prm: anything with mp_max, mp_min, np, gap_open, gap_ext, q_base.  windows u8 [n, L + 2k] (ASCII), reads / quals u8 [n, L],
    end_in / err_in: what the filter found, forward[n]: the strand, reverse_quality[n] (or None): the quality row is read mirrored.
    -> list of dicts: start, end, nm, score, cigar (as the reference prints it), raw (the CIGAR before the I -> M rewrite; None when
    no DP ran), lo, hi (the range tracker; 0, 0 when no DP ran)"""
    windows = np.asarray(windows, dtype=np.uint8); reads = np.asarray(reads, dtype=np.uint8)
    quals = np.asarray(quals, dtype=np.uint8).copy()
    n, tlen = reads.shape
    qlen = windows.shape[1]
    w = int(k)
    assert qlen == tlen + 2 * w
    if reverse_quality is not None:
        rq = np.asarray(reverse_quality, dtype=bool)
        quals[rq] = quals[rq, ::-1]
    out = [None] * n
    need = []
    for j in range(n):
        e = int(end_in[j])
        if int(err_in[j]) == 0:
            out[j] = dict(start=e - tlen + 1, end=e, nm=0, score=0, cigar="%dM" % tlen, raw=None, lo=0, hi=0)
            continue
        # try_cigar_without_path
        start = e - tlen + 1
        done = False
        if start >= 0:
            pat = windows[j, start:start + tlen]; txt = reads[j]
            mm = (txt != pat) & ~((txt == ord("T")) & (pat == ord("C")))
            if int(mm.sum()) == int(err_in[j]):
                isn = (txt == ord("N")) | (pat == ord("N"))
                pen = mismatch_penalty(prm.mp_max, prm.mp_min, prm.q_base, quals[j])
                sc = -int(np.where(isn, prm.np, pen)[mm].sum())
                out[j] = dict(start=start, end=e, nm=int(err_in[j]), score=sc, cigar="%dM" % tlen, raw=None, lo=0, hi=0)
                done = True
        if not done:
            need.append(j)
    if need:
        sel = np.array(need)
        res = _semi_global_back(prm, windows[sel], reads[sel], quals[sel], w)
        for t, j in enumerate(need):
            out[j] = _post(windows[j], reads[j], bool(forward[j]), *[r[t] for r in res])
    return out


def _semi_global_back(prm, query, target, qual, w):
    """ksw_semi_global_quality_back over a batch: query = the windows (columns), target = the reads (rows)"""
    n, tlen = target.shape
    qlen = query.shape[1]
    gapoe, gape = int(prm.gap_open) + int(prm.gap_ext), int(prm.gap_ext)
    band = 2 * w + 1
    mat, diff = score_matrix(prm.mp_max, prm.mp_min, prm.np)
    qc = NT4[query]; tc = NT4[target]
    H = np.full((qlen + 2, n), MINUS_INF, dtype=np.int64)
    E = np.full((qlen + 2, n), MINUS_INF, dtype=np.int64)
    H[:band] = 0
    E[:band] = -gapoe
    z = np.zeros((tlen, band, n), dtype=np.uint8)
    lo = np.zeros(n, dtype=np.int64); hi = np.zeros(n, dtype=np.int64)

    def track(v):
        real = v > _FENCE
        np.minimum(lo, np.where(real, v, lo), out=lo)
        np.maximum(hi, np.where(real, v, hi), out=hi)

    beg = end = 0
    for i in range(tlen):
        f = np.full(n, MINUS_INF, dtype=np.int64)
        h1 = np.full(n, MINUS_INF, dtype=np.int64)
        phred = np.minimum(qual[:, i].astype(np.float64) - prm.q_base, 40.0) / 40
        beg, end = i, i + band
        for j in range(beg, end):
            m = H[j].copy(); e = E[j].copy()
            H[j] = h1
            m = m + mat[tc[:, i], qc[:, j]] - (diff[tc[:, i], qc[:, j]] * phred).astype(np.int64)
            d = np.where(m >= e, 0, 1)
            h = np.where(m >= e, m, e)
            d = np.where(h >= f, d, 2)
            h = np.where(h >= f, h, f)
            h1 = h
            t = m - gapoe
            e = e - gape
            d = d | np.where(e > t, 1 << 2, 0)
            e = np.where(e > t, e, t)
            E[j] = e
            f = f - gape
            d = d | np.where(f > t, 2 << 4, 0)
            f = np.where(f > t, f, t)
            z[i, j - beg] = d
            track(m); track(h); track(e); track(f)
        H[end] = h1
        E[end] = MINUS_INF
    max_i = np.full(n, tlen + w, dtype=np.int64)
    score = H[tlen + w].copy()
    for i in range(end, beg, -1):
        better = H[i] > score
        score = np.where(better, H[i], score)
        max_i = np.where(better, i, max_i)
    qe = max_i - 1
    # backtrack, job by job
    raws, qbs = [], []
    for t in range(n):
        ops = []          # [op, len] with op 0 M, 1 D (window only), 2 I (read only), last cell first

        def push(op, ln):
            if ops and ops[-1][0] == op:
                ops[-1][1] += ln
            else:
                ops.append([op, ln])
        i, kk, which = tlen - 1, int(max_i[t]) - 1, 0
        while i >= 0 and kk >= 0:
            which = (int(z[i, kk - i, t]) >> (which << 1)) & 3
            if which == 0:
                push(0, 1); i -= 1; kk -= 1
            elif which == 1:
                push(2, 1); i -= 1
            else:
                push(1, 1); kk -= 1
        if i >= 0:
            push(2, i + 1)
        ops.reverse()
        raws.append(ops); qbs.append(kk + 1)
    return score.tolist(), qbs, qe.tolist(), raws, lo.tolist(), hi.tolist()


def _post(pattern, text, forward, score, qb, qe, raw, lo, hi):
    """fast_recalculate_bs_Cigar after the DP: I runs at either end become M, NM is recounted, the minus strand prints backwards"""
    cg = [list(o) for o in raw]
    n_cigar = len(cg)
    cg.append([0, 0])          # the reference may look one slot past the end
    ins = 0
    i = 0
    while i < n_cigar and cg[i][0] == 2:
        ins += cg[i][1]; i += 1
    if i != 0:
        if cg[i][0] == 0:
            cg[i][1] += ins
        else:
            i -= 1
            cg[i] = [0, ins]
        qb -= ins
    cigar_b = i
    ins = 0
    i = n_cigar - 1
    while i >= cigar_b and cg[i][0] == 2:
        ins += cg[i][1]; i -= 1
    if i != n_cigar - 1:
        if cg[i][0] == 0:
            cg[i][1] += ins
        else:
            i += 1
            cg[i] = [0, ins]
        qe += ins
    cigar_e = i

    def mism(p, t):
        return p != t and not (p == ord("C") and t == ord("T"))
    nm = 0
    printed = []
    if forward:
        qs, ts = qb, 0
        for op, ln in cg[cigar_b:cigar_e + 1]:
            printed.append((op, ln))
            if op == 0:
                nm += sum(mism(int(pattern[qs + x]), int(text[ts + x])) for x in range(ln))
                qs += ln; ts += ln
            elif op == 1:
                qs += ln; nm += ln
            else:
                ts += ln; nm += ln
    else:
        qx, te = qe, len(text) - 1
        for op, ln in reversed(cg[cigar_b:cigar_e + 1]):
            printed.append((op, ln))
            if op == 0:
                nm += sum(mism(int(pattern[qx - x]), int(text[te - x])) for x in range(ln))
                qx -= ln; te -= ln
            elif op == 1:
                qx -= ln; nm += ln
            else:
                te -= ln; nm += ln
    return dict(start=qb, end=qe, nm=nm, score=int(score), cigar=_ops_text(printed), raw=_ops_text(raw), lo=int(lo), hi=int(hi))
