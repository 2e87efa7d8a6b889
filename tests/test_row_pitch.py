"""The device's packed read rows on whole 64-byte lines (pack_words in k_rows.hip: W + M words rounded up to a multiple of 8) with no
spare word behind a row: where W + M is a multiple of 8 already (129-160 bases, 481-512) the word after a row's last mask word is the
next row's first base word, or the slack behind the buffer.

1. every mapping mode at the lengths where the layout can go wrong, against the oracle (every record and CIGAR word);
2. neighbour independence: what stands in the rows next to a read cannot reach its records;
3. one context used at 250, 150 and 100 bases in turn equals a fresh context at each length (stale words of a reused row buffer);
4. the pitch rule itself for 1 .. 1000 bases, by a stand-alone host program compiled from the header k_rows.hip includes (CPU).

The packed rows themselves are not handed out by any entry point (bmbs_filter_batch_packed packs on the device and returns the filter's
results only), so the layout on the device is pinned through 2. and 3. and not by reading the buffer.  What no case here can see:
whether the writers zero the mask plane's bits beyond the last 16-character piece and the words up to the pitch -- every reader masks
by the read's length, so those words reach no record either way; that part rests on reading pack_row_tail and its three callers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import orc
from common import ROOT
from test_vote_dense import _freeze, _index, _make_golden, _other_letter

LENGTHS = [100, 128, 129, 150, 160, 161, 250, 500]         # 129 / 150 / 160 / 500: no word between W + M and the pitch
N_SE, N_PE = 3000, 2000


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """the 300 kb test genome of the GPU suite (tests/golden/make_golden.py)"""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return _index(tmp_path_factory, "small", *_make_golden().genome())


def _plant(rows, exact, rng):
    """the special reads, written over the first rows of `rows` (as the seeding kernels see them) from error-free reads `exact`:
    a mismatch in the last base alone (exit C: k_seed_second walks to the row's end), an 'N' as the first / the last character, both,
    all-'N' reads, and a deleted / an inserted base a few positions before the 3' end (k_align_sw2 and its recount read the row's end)"""
    n, L = rows.shape
    k = 0

    def take(cnt):
        nonlocal k
        sl = slice(k, k + cnt)
        rows[sl] = exact[sl]
        k += cnt
        return sl
    sl = take(100); rows[sl, L - 1] = _other_letter(rows[sl, L - 1])
    sl = take(40); rows[sl, 0] = ord("N")
    sl = take(40); rows[sl, L - 1] = ord("N")
    sl = take(20); rows[sl, 0] = ord("N"); rows[sl, L - 1] = ord("N")
    sl = take(20); rows[sl, :] = ord("N")
    for back in (6, 9, 14):
        sl = take(30)                                                     # deletion: the tail moves up, a new last base
        rows[sl, L - back:L - 1] = rows[sl, L - back + 1:L].copy()
        rows[sl, L - 1] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 30)]
        sl = take(30)                                                     # insertion: the tail moves down, the last base drops out
        rows[sl, L - back + 1:L] = rows[sl, L - back:L - 1].copy()
        rows[sl, L - back] = _other_letter(rows[sl, L - back + 1])
    assert k <= n
    return rows


def se_batch(g, L, n=N_SE, seed=0):
    from bitmapperbs_amd import synth
    r = synth.make_reads_se(g["chroms"], n=n, L=L, seed=1300 + L + seed, sub=0.02, indel=0.002, qual="random", n_rate=0.002)
    x = synth.make_reads_se(g["chroms"], n=400, L=L, seed=1400 + L + seed, sub=0.0, indel=0.0, qual="const")
    seq = _plant(r["seq"].copy(), x["seq"], np.random.default_rng(L + seed))
    return _freeze((seq, r["qual"]))


def pe_batch(g, L, n=N_PE, seed=0):
    """mate 2 is planted on the row the kernels see (the reverse complement of its FASTQ text) and turned back"""
    from bitmapperbs_amd import synth
    hi = max(500, 2 * L + 50)
    m1, m2 = synth.make_reads_pe(g["chroms"], n=n, L=L, seed=1500 + L + seed, sub=0.02, indel=0.002, qual="random", ins_hi=hi)
    x1, x2 = synth.make_reads_pe(g["chroms"], n=800, L=L, seed=1600 + L + seed, sub=0.0, indel=0.0, qual="const", ins_hi=hi)
    rng = np.random.default_rng(7 * L + seed)
    s1, r2, rx2 = m1["seq"].copy(), synth.revcomp(m2["seq"]), synth.revcomp(x2["seq"])
    # pairs 0 .. 399: mate 1 special beside its error-free mate 2; pairs 400 .. 799 the other way round
    s1[:400] = _plant(s1[:400].copy(), x1["seq"][:400], rng); r2[:400] = rx2[:400]
    s1[400:800] = x1["seq"][400:800]; r2[400:800] = _plant(r2[400:800].copy(), rx2[400:800], rng)
    return _freeze((s1, m1["qual"], synth.revcomp(r2), m2["qual"]))


def _se(g, prm, inp, L):
    from bitmapperbs_amd import mapper
    from test_gpu_parity import compare_records
    m = mapper.Mapper(g["ix"], 0, **prm)
    res, pool = m.map_se(*inp, L)
    st = m.stats()
    m.close()
    recs, ost, _ = g["oix"].map_se(orc.params(**prm), *inp, L)
    bad = compare_records(res, pool, recs, L)
    assert not bad, bad[:5]
    assert (st == ost).all(), (st, ost)
    return recs


def _pe(g, prm, inp, L):
    from bitmapperbs_amd import mapper
    from test_gpu_parity import compare_pe
    m = mapper.Mapper(g["ix"], 0, **prm)
    res, pool = m.map_pe(*inp, L)
    st = m.stats()
    m.close()
    recs, ost, _ = g["oix"].map_pe(orc.params(**prm), *inp, L)
    bad = compare_pe(res, pool, recs, L)
    assert not bad, bad[:5]
    assert (st == ost).all(), (st, ost)
    return recs


# ---- 1. the lengths where the layout can go wrong ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L", LENGTHS)
def test_single_end_matches_oracle(small, L):
    recs = _se(small, dict(e_f=0.08), se_batch(small, L), L)
    assert (recs["status"] == 1).sum() > N_SE // 2


@pytest.mark.gpu
@pytest.mark.parametrize("sens", [0, 1], ids=["fast", "sensitive"])
@pytest.mark.parametrize("L", LENGTHS)
def test_paired_end_matches_oracle(small, L, sens):
    prm = dict(e_f=0.08, sensitive=sens, max_ins=max(500, 2 * L + 50))
    recs = _pe(small, prm, pe_batch(small, L), L)
    assert (recs["status"] == 1).sum() > N_PE // 2


def _trim(rows, lens):
    out = rows.copy()
    out[np.arange(rows.shape[1])[None, :] >= lens[:, None]] = 0
    return out


def _lens(rng, n):
    """30 .. 150, the longest (the row's last position) in front and the lengths around the planes' word boundaries among them"""
    lens = rng.integers(30, 151, n).astype(np.uint16)
    lens[:600] = 150
    lens[600:660] = np.repeat(np.array([30, 32, 33, 64, 65, 96, 97, 128, 129, 144, 145, 149], dtype=np.uint16), 5)
    return lens


@pytest.mark.gpu
def test_single_end_mixed_lengths_match_oracle(small):
    from bitmapperbs_amd import mapper
    from test_gpu_parity import compare_records
    g = small
    seq, qual = se_batch(g, 150, seed=1)
    lens = _lens(np.random.default_rng(41), N_SE)
    seq, qual = _trim(seq, lens), _trim(qual, lens)
    m = mapper.Mapper(g["ix"], 0, e_f=0.08)
    res, pool = m.map_se_var(seq, qual, lens)
    recs, ost, _ = g["oix"].map_se_var(orc.params(e_f=0.08), seq, qual, lens)
    bad = compare_records(res, pool, recs, lens)
    assert not bad, bad[:5]
    assert (m.stats() == ost).all(), (m.stats(), ost)
    assert (recs["status"] == 1).sum() > N_SE // 2
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sens", [0, 1], ids=["fast", "sensitive"])
def test_paired_end_mixed_lengths_match_oracle(small, sens):
    from bitmapperbs_amd import mapper
    from test_gpu_parity import compare_pe
    g = small
    s1, q1, s2, q2 = pe_batch(g, 150, seed=1)
    rng = np.random.default_rng(43)
    l1, l2 = _lens(rng, N_PE), _lens(rng, N_PE)[::-1].copy()
    s1, q1, s2, q2 = _trim(s1, l1), _trim(q1, l1), _trim(s2, l2), _trim(q2, l2)
    prm = dict(e_f=0.08, sensitive=sens, max_ins=500)
    m = mapper.Mapper(g["ix"], 0, **prm)
    res, pool = m.map_pe_var(s1, q1, s2, q2, l1, l2)
    recs, ost, _ = g["oix"].map_pe_var(orc.params(**prm), s1, q1, s2, q2, l1, l2)
    bad = compare_pe(res, pool, recs, l1, l2)
    assert not bad, bad[:5]
    assert (m.stats() == ost).all(), (m.stats(), ost)
    assert (recs["status"] == 1).sum() > N_PE // 3
    m.close()


# ---- 2. neighbour independence ------------------------------------------------------------------------------------------------------------------
def _fields(res, pool, L):
    """a record without its place in the CIGAR pool (that depends on the records before it): every field, and the CIGAR's text"""
    from bitmapperbs_amd import mapper
    out = []
    for a in res:
        rec = tuple(int(a[f]) for f in ("status", "chrom", "pos", "flag", "mapq", "nm", "score", "path", "tlen", "n_cigar", "n_cand"))
        out.append(rec + (mapper.cigar_text(a, pool, L) if int(a["status"]) == 1 else "",))
    return out


def _others(seq, rng):
    """the rows of another batch, with all-T, all-'N', all-A and all-G rows among them (every bit of both planes set somewhere)"""
    out = seq[rng.permutation(seq.shape[0])].copy()
    for i, c in enumerate(b"TNAG"):
        out[i::16] = c
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("L", [129, 150, 160, 500])
def test_single_end_records_do_not_depend_on_the_neighbouring_rows(small, L):
    from bitmapperbs_amd import mapper
    g = small
    seq, qual = se_batch(g, L, n=2001, seed=2)                 # odd: the last row is an even one, in front of the slack behind the buffer
    other = _others(se_batch(g, L, n=2001, seed=3)[0], np.random.default_rng(L))
    seq2 = seq.copy(); seq2[1::2] = other[1::2]
    m = mapper.Mapper(g["ix"], 0, e_f=0.08)
    a = m.map_se(seq, qual, L); b = m.map_se(seq2, qual, L)
    one = m.map_se(seq[-1:], qual[-1:], L)                     # a one-row batch: nothing but the slack behind it
    m.close()
    fa, fb = _fields(*a, L), _fields(*b, L)
    assert fa[0::2] == fb[0::2]
    assert _fields(*one, L)[0] == fa[-1]
    assert sum(r[0] == 1 for r in fa[0::2]) > 500


@pytest.mark.gpu
@pytest.mark.parametrize("sens", [0, 1], ids=["fast", "sensitive"])
@pytest.mark.parametrize("L", [129, 150, 160, 500])
def test_paired_end_records_do_not_depend_on_the_neighbouring_rows(small, L, sens):
    """rows [0, n) are mate 1 and [n, 2n) mate 2: with n odd, the pairs at even places keep both their rows' neighbours changing, and
    mate 1 of the last pair stands in front of mate 2 of the first"""
    from bitmapperbs_amd import mapper
    g = small
    n = 1501
    s1, q1, s2, q2 = pe_batch(g, L, n=n, seed=2)
    o1, _, o2, _ = pe_batch(g, L, n=n, seed=3)
    rng = np.random.default_rng(3 * L)
    o1, o2 = _others(o1, rng), _others(o2, rng)
    t1, t2 = s1.copy(), s2.copy()
    t1[1::2] = o1[1::2]; t2[1::2] = o2[1::2]
    prm = dict(e_f=0.08, sensitive=sens, max_ins=max(500, 2 * L + 50))
    m = mapper.Mapper(g["ix"], 0, **prm)
    a = m.map_pe(s1, q1, s2, q2, L); b = m.map_pe(t1, q1, t2, q2, L)
    one = m.map_pe(s1[-1:], q1[-1:], s2[-1:], q2[-1:], L)
    m.close()
    fa, fb = _fields(*a, L), _fields(*b, L)
    even = [i for p in range(0, n, 2) for i in (2 * p, 2 * p + 1)]
    assert [fa[i] for i in even] == [fb[i] for i in even]
    assert _fields(*one, L) == fa[-2:]
    assert sum(fa[i][0] == 1 for i in even) > 500


# ---- 3. one row buffer, three lengths --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["se", "pe", "pe_sensitive"])
def test_a_context_used_at_another_length_before_equals_a_fresh_one(small, mode):
    """250 bases (16-word rows), then 150 (8 words, no word to spare), then 100 (8 words, two of them beyond W + M): every word of the
    shorter rows stood inside a longer row before"""
    from bitmapperbs_amd import mapper
    g = small
    prm = dict(e_f=0.08) if mode == "se" else dict(e_f=0.08, sensitive=int(mode == "pe_sensitive"), max_ins=600)
    make = se_batch if mode == "se" else pe_batch

    def run(m, inp, L):
        """the records' bytes and every CIGAR word a record points at (the pool's words between them belong to no record: alignment
        jobs that lost, whose slots keep what an earlier call left there)"""
        res, pool = (m.map_se if mode == "se" else m.map_pe)(*inp, L)
        used = [pool[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["n_cigar"])].tobytes() for a in res if int(a["n_cigar"])]
        assert len(used) > 20
        return res.tobytes(), used
    batches = [(L, make(g, L, n=1500, seed=4)) for L in (250, 150, 100)]
    m = mapper.Mapper(g["ix"], 0, **prm)
    reused = [run(m, inp, L) for L, inp in batches]
    m.close()
    for (L, inp), got in zip(batches, reused):
        f = mapper.Mapper(g["ix"], 0, **prm)
        assert run(f, inp, L) == got, L
        f.close()


# ---- 4. the pitch rule (CPU) -------------------------------------------------------------------------------------------------------------------------
def test_pitch_rule_for_every_length(tmp_path):
    """pack_words(L) for L = 1 .. 1000, computed by the header k_rows.hip includes (csrc/bmbs_rowpitch.h): a multiple of 8 words, at
    least W + M, less than W + M + 8; 150 and 100 bases take one line, 250 two"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is part of the build"
    csrc = os.path.join(ROOT, "bitmapperbs_amd", "csrc")
    assert '#include "bmbs_rowpitch.h"' in open(os.path.join(csrc, "k_rows.hip")).read()
    prog = tmp_path / "pitch.cpp"
    prog.write_text("#include <cstdio>\n#define __host__\n#define __device__\n#include \"bmbs_rowpitch.h\"\n"
                    "int main() { for (int L = 1; L <= 1000; L++) std::printf(\"%d %d %d\\n\", L, pack_base_words(L), pack_words(L)); return 0; }\n")
    exe = tmp_path / "pitch"
    subprocess.run([cxx, "-O1", "-I", csrc, "-o", str(exe), str(prog)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    rows = [tuple(map(int, ln.split())) for ln in out if ln]
    assert [r[0] for r in rows] == list(range(1, 1001))
    for L, W, pw in rows:
        M = (L + 63) // 64
        assert W == (L + 31) // 32
        assert pw % 8 == 0 and W + M <= pw < W + M + 8, (L, W, M, pw)
    pitch = {L: pw for L, _, pw in rows}
    assert (pitch[100], pitch[150], pitch[160], pitch[161], pitch[250], pitch[500]) == (8, 8, 8, 16, 16, 24)
