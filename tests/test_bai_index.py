"""The .bai index of a sorted BAM, written in the same run (`bmbs_search --bam --sort --bai`, bmbs_bam_sort_index, csrc/k_bai.hip).
The yardstick is tests/bai_spec.py: a plain-Python BAI builder and reader written from the SAM specification.  Every comparison is
exact: an index is a table of integers."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import bai_spec
from common import GOLD, ROOT, bgzf_blocks, golden_args, gunzip_to, write_bgzf

HERE = os.path.dirname(os.path.abspath(__file__))
BLK = 0xff00
OPS = "MIDNSHP=X"


def make_rec(ref, pos, flag, name=b"r", cigar=((10, "M"),), l_seq=10, fill=0x5a):
    """one BAM record (block_size word included); cigar: (length, op) pairs"""
    cig = b"".join(struct.pack("<I", (n << 4) | OPS.index(op)) for n, op in cigar)
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name) + 1, 30, 4680, len(cigar), flag, l_seq, -1, -1, 0) + name + b"\0" + cig + \
        bytes([fill & 0xff]) * ((l_seq + 1) // 2) + bytes([(fill >> 1) & 0x3f]) * l_seq
    return struct.pack("<I", len(body)) + body


def bam_bytes(refs, records):
    text = b"@HD\tVN:1.4\tSO:coordinate\n"
    h = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, ln in refs:
        h += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", ln)
    return h + b"".join(records)


def _driver():
    p = os.path.join(ROOT, "bitmapperbs_amd", "bmbs_search")
    assert os.path.exists(p), "bmbs_search not built (make -C bitmapperbs_amd/csrc)"
    return p


# ---- no GPU: the yardstick itself ------------------------------------------------------------------------------------------------------
def test_spec_against_a_hand_written_index(tmp_path):
    """six records in two BGZF blocks (stored, so that the block sizes do not depend on the deflater): one crosses a 16 kb boundary and
    lies in a bin of the level above, one is unmapped with a coordinate, one has no coordinate.  The expected index, byte by byte:
    the header takes bytes 0..69 of the inflated stream, the records 57 bytes each (the last, without a CIGAR, 53); blocks of 250 data
    bytes are 281 in the file, so block 2 (158 data bytes, 189 in the file) starts at file offset 281 and the end-of-file block at 470.
      record   stream offset   virtual offset    ref  [beg, end)       bin    windows
      a        70              70                0    [100, 110)       4681   0
      b        127             127               0    [16380, 16390)   585    0, 1      (crosses 16384: one level up)
      c        184             184               0    [16400, 16401)   4682   -         (flag 4, placed)
      d        241             241               0    [16400, 16410)   4682   1         (9 bytes in block 1, the rest in block 2)
      e        298             281 << 16 | 48    1    [0, 10)          4681   0
      f        355             281 << 16 | 105   -1
      end      408             470 << 16"""
    recs = [make_rec(0, 100, 0, b"a"), make_rec(0, 16380, 16, b"b"), make_rec(0, 16400, 4 | 1 | 8, b"c"), make_rec(0, 16400, 0, b"d"),
            make_rec(1, 0, 0, b"e"), make_rec(-1, -1, 4, b"f", cigar=(), l_seq=10)]
    data = bam_bytes([(b"c1", 100000), (b"c2", 50000), (b"c3", 7)], recs)
    assert [len(r) for r in recs] == [57] * 5 + [53] and len(data) == 70 + 5 * 57 + 53
    path = str(tmp_path / "h.bam")
    write_bgzf(path, data, block=250, level=0)
    raw = open(path, "rb").read()
    assert [(b, len(r)) for b, r in bgzf_blocks(raw)] == [(281, 250), (189, 158), (31, 0)]
    B2, END = 281 << 16, 470 << 16
    q = lambda *v: struct.pack("<%dQ" % len(v), *v)
    want = b"BAI\x01" + struct.pack("<i", 3) + \
        struct.pack("<i", 4) + \
        struct.pack("<Ii", 585, 1) + q(127, 184) + \
        struct.pack("<Ii", 4681, 1) + q(70, 127) + \
        struct.pack("<Ii", 4682, 1) + q(184, B2 | 48) + \
        struct.pack("<Ii", 37450, 2) + q(70, B2 | 48, 3, 1) + \
        struct.pack("<i", 2) + q(70, 127) + \
        struct.pack("<i", 2) + \
        struct.pack("<Ii", 4681, 1) + q(B2 | 48, B2 | 105) + \
        struct.pack("<Ii", 37450, 2) + q(B2 | 48, B2 | 105, 1, 0) + \
        struct.pack("<i", 1) + q(B2 | 48) + \
        struct.pack("<ii", 0, 0) + \
        q(1)
    got = bai_spec.spec_bai(path)
    assert got == want
    ix = bai_spec.parse_bai(got)
    assert ix["n_no_coor"] == 1 and ix["refs"][2] == dict(bins={}, meta=None, lin=[])
    assert ix["refs"][0]["meta"] == (70, B2 | 48, 3, 1) and ix["refs"][0]["lin"] == [70, 127]
    # the pieces of the record blocks alone (offsets relative to their first byte): what bmbs_bam_sort_index returns for one call.
    # 338 bytes in blocks of 200: block 2 at 231, e at its byte 28, f at 85, the end at 231 + 169 = 400
    recs_only = str(tmp_path / "r.bgzf")
    write_bgzf(recs_only, b"".join(recs), block=200, level=0)
    z = open(recs_only, "rb").read()[:400]                                          # (without the empty last block)
    b2 = 231 << 16
    chunks, wins, refs, nnc = bai_spec.spec_pieces(z)
    assert chunks == [(0, 585, 57, 114), (0, 4681, 0, 57), (0, 4682, 114, b2 | 28), (1, 4681, b2 | 28, b2 | 85)]
    assert wins == [(0, 0, 0), (0, 1, 57), (1, 0, b2 | 28)]
    assert refs == [(0, 0, b2 | 28, 3, 1), (1, b2 | 28, b2 | 85, 1, 0)] and nnc == 1
    assert bai_spec._Stream(z).voff(338) == 400 << 16
    # the lookup: b reaches into window 1, c is found although only mapped records enter the linear index, nothing on c3
    assert bai_spec.query(got, raw, 0, 16384, 16385) == [127]
    assert bai_spec.query(got, raw, 0, 16400, 16401) == [184, 241]
    assert bai_spec.query(got, raw, 0, 0, 100000) == [70, 127, 184, 241]
    assert bai_spec.query(got, raw, 1, 0, 1) == [B2 | 48] and bai_spec.query(got, raw, 2, 0, 7) == []
    assert END == bai_spec._Stream(raw).voff(408)


def _random_sorted_bam(path, n=2000, seed=5):
    """n records on three references (one of them long enough for the upper bin levels), sorted; flag-4 records with a coordinate sit
    behind a mapped record of the same position, as placed mates do"""
    rng = np.random.default_rng(seed)
    lens = [300_000, 70_000_000, 90_000]
    rows = []
    for i in range(n):
        ref = int(rng.integers(0, 3))
        pos = int(rng.integers(0, lens[ref] - 40_000)) if rng.random() < 0.5 else int(rng.integers(0, 30_000))
        span = int(rng.choice([30, 100, 150, 5_000, 20_000, 35_000], p=[.3, .3, .2, .1, .05, .05]))
        rows.append((ref, pos, 0, 0, span, i))
        if i % 17 == 0:
            rows.append((ref, pos, 1, 4, 0, i))
    rows += [(-1, -1, 0, 4, 0, n + k) for k in range(25)]
    rows.sort(key=lambda r: (r[0] & 0xffffffff, r[1], r[2]))
    recs = [make_rec(ref, pos, flag | (16 if i % 2 else 0), b"n%d" % i, ((20, "M"), (span - 20, "N")) if span > 150 else ((span, "M"),) if span else (), 20 + i % 50, i)
            for ref, pos, _, flag, span, i in rows]
    write_bgzf(path, bam_bytes([(b"a", lens[0]), (b"b", lens[1]), (b"c", lens[2])], recs), block=50_000)
    return lens


def test_spec_query_against_brute_force_overlap(tmp_path):
    """the yardstick's index + lookup return exactly the overlapping records: 2 000 random records on three references, 200 random
    regions and every reference's whole span"""
    path = str(tmp_path / "r.bam")
    lens = _random_sorted_bam(path)
    raw = open(path, "rb").read()
    st = bai_spec._Stream(raw)
    ix = bai_spec.parse_bai(bai_spec.spec_bai(path))
    assert sum(r["meta"][2] + r["meta"][3] for r in ix["refs"]) + ix["n_no_coor"] == 2000 + 118 + 25
    assert any(b < 585 for r in ix["refs"] for b in r["bins"])                      # bins of the upper levels
    rng = np.random.default_rng(6)
    regions = [(r, 0, lens[r]) for r in range(3)]
    for _ in range(200):
        r = int(rng.integers(0, 3))
        b = int(rng.integers(0, lens[r] if rng.random() < 0.5 else 60_000))
        regions.append((r, b, b + int(rng.choice([1, 100, 20_000, 3_000_000]))))
    hits = 0
    for r, b, e in regions:
        want = bai_spec.brute_force(st, r, b, e)
        assert bai_spec.query(ix, st, r, b, e) == want, (r, b, e)
        hits += len(want)
    assert hits > 5000


# ---- no GPU: the command line and the interface ---------------------------------------------------------------------------------------------
def test_bai_without_sort_is_refused_by_name():
    p = subprocess.run([_driver(), "--search", "nowhere", "--seq", "none.fq", "--bam", "--bai"], capture_output=True, text=True)
    assert p.returncode == 2
    assert "bmbs_search: --bai needs --sort" in p.stderr


def test_bai_with_an_output_that_is_no_regular_file_is_refused_by_name():
    p = subprocess.run([_driver(), "--search", "nowhere", "--seq", "none.fq", "--bam", "--sort", "--bai", "-o", "/dev/null"], capture_output=True, text=True)
    assert p.returncode == 2
    assert "bmbs_search: --bai needs a regular output file (-o /dev/null is none)" in p.stderr


def test_bam_sort_index_is_declared_and_listed():
    from bitmapperbs_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmbs.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+bmbs_bam_sort_index\s*\(\s*bmbs_ctx\s*\*", hdr)
    for t in ("bmbs_bai_chunk", "bmbs_bai_win", "bmbs_bai_ref"):
        assert re.search(r"typedef\s+struct\s+%s\b" % t, hdr), t
    assert "bmbs_bam_sort_index" in capi.SYMBOLS
    assert hasattr(capi.lib(), "bmbs_bam_sort_index")


def test_several_units_budget_forces_a_run_across_a_unit_boundary():
    """the choice of test_driver_index_over_several_units, checked on the unsorted golden: with calls of at most UNIT_BUDGET bytes the
    sorted records of se_b150 need more calls than they have runs of one (ref, bin) -- so some run goes on across a call boundary"""
    import gzip
    from common import sam_to_bam_records
    sam = gzip.open(os.path.join(GOLD, "se_b150.ref.sam.gz"), "rb").read()
    names = [l.split(b"\t")[1][3:].decode() for l in sam.split(b"\n") if l.startswith(b"@SQ")]
    recs = sam_to_bam_records(sam, names)
    keys = []
    at = 0
    while at < len(recs):
        size, ref, beg, end, _ = bai_spec.record_fields(recs, at)
        keys.append((ref & 0xffffffff, beg, bai_spec._reg2bin(beg, end)))
        at += size
    keys.sort()
    runs = 1 + sum(1 for a, b in zip(keys, keys[1:]) if (a[0], a[2]) != (b[0], b[2]))
    assert len(recs) // UNIT_BUDGET >= max(4, runs + 1)


UNIT_BUDGET = 8000


# ---- GPU: the library ----------------------------------------------------------------------------------------------------------------------
def _synthetic_records(seed=3):
    """about 3 000 records, in no order, that take every branch of k_bai_records and its successors (see the list in the test)"""
    rng = np.random.default_rng(seed)
    recs = []
    name = lambda i: b"abcdefghijklmnopqrstuvwxyz0123456789ABCD"[:i % 40 + 1]      # 1 .. 40 characters: CIGARs at every alignment
    for i in range(2900):
        ref = int(rng.choice([0, 1, 2, 4, 5]))                                     # reference 3 has no records
        pos = int(rng.integers(0, 40_000)) if i % 2 else int(rng.integers(0, 3_000_000))
        n_ops = int(rng.integers(1, 8))
        cigar = tuple((int(rng.integers(1, 60)), OPS[int(rng.integers(0, 9))]) for _ in range(n_ops))
        flag = (16 if rng.random() < 0.5 else 0) | (4 if i % 23 == 0 else 0)       # flag 4 with a position (and a CIGAR that must not count)
        if i % 29 == 0:
            cigar = ()                                                             # n_cigar_op 0, mapped or not
        recs.append(make_rec(ref, pos, flag, name(i), cigar, 20 + int(rng.integers(0, 260)), i))
    for k in range(60):
        recs.append(make_rec(-1, -1, 4, b"u%d" % k, (), 50, k))                    # refID -1
    W = 1 << 14
    special = [
        (0, 0, ((50, "M"),)), (1, 0, ()),                                          # pos 0
        (5, (1 << 29) - 100, ((100, "M"),)),                                       # ends exactly at 2^29
        (5, (1 << 29) - 1, ()),
        (2, 10 * W + 5, ((100, "M"),)),                                            # one window
        (2, 11 * W - 5, ((100, "M"),)),                                            # two windows: a level-5 bin boundary
        (2, 20 * W + 5, ((10, "M"), (8 * W, "N"), (10, "M"))),                     # nine windows
        (4, (1 << 17) - 5, ((10, "="), (10, "X"))),                                # a level-4 bin boundary
        (4, (1 << 26) - 5, ((10, "M"), (3, "D"), (10, "M"))),                      # a level-1 bin boundary: bin 0
        (4, (1 << 20) - 1, ((1, "M"), (5, "I"), (1, "M"))),
        (0, 7 * W - 1, ((5, "S"), (1, "M"), (5, "H"))),                            # ends exactly at a window edge
        (0, 7 * W - 1, ((5, "I"), (3, "P"))),                                      # a CIGAR without reference length: end = pos + 1
    ]
    for j, (ref, pos, cigar) in enumerate(special):
        recs.append(make_rec(ref, pos, 0, b"s%d" % j, cigar, 30, j))
    order = rng.permutation(len(recs))
    return [recs[i] for i in order]


def _index_equals_spec(m, recs):
    """bam_sort + bam_sort_index of the records against the yardstick's pieces of the blocks returned, entry for entry"""
    z = m.bam_sort(b"".join(recs), np.array([len(r) for r in recs], dtype=np.uint32))
    ch, wi, rf, nnc = m.bam_sort_index()
    chunks, wins, refs, want_nnc = bai_spec.spec_pieces(z)
    assert [tuple(x) for x in ch.tolist()] == chunks
    assert [tuple(x) for x in wi.tolist()] == wins
    assert [(r, b, e, nm, nu) for r, _, b, e, nm, nu in rf.tolist()] == refs
    assert nnc == want_nnc
    return z, chunks, wins, refs, nnc


def _synthetic_check():
    from bitmapperbs_amd import mapper
    recs = _synthetic_records()
    m = mapper.Mapper(None, 0)
    z, chunks, wins, refs, nnc = _index_equals_spec(m, recs)
    m.close()
    blocks = bgzf_blocks(z)
    assert len(blocks) >= 4 and sum(len(r) for r in recs) % BLK                    # several blocks; records straddle their edges
    assert nnc == 60 and [r[0] for r in refs] == [0, 1, 2, 4, 5]
    bins = {b for _, b, _, _ in chunks}
    assert 0 in bins and any(1 <= b < 4681 for b in bins) and any(b >= 4681 for b in bins)
    assert (5, ((1 << 29) - 1) >> 14) in {(r, w) for r, w, _ in wins}
    assert len([1 for r, w, _ in wins if r == 2 and 20 <= w <= 28]) == 9
    print("chunks %d windows %d refs %d" % (len(chunks), len(wins), len(refs)))


@pytest.mark.gpu
def test_index_of_synthetic_records_is_the_spec():
    """every CIGAR operation, no CIGAR, flag 4 with a position, refID -1, pos 0, an end at exactly 2^29, records over one, two and nine
    windows, over a level-5, a level-4 and a level-1 bin boundary, a reference without records between two that have some, read names
    of 1 to 40 characters, several BGZF blocks with records across their edges"""
    _synthetic_check()


def _sized(size, ref, pos, tag):
    """a mapped record of exactly `size` bytes"""
    for extra in range(1, 4):
        rem = size - 36 - (extra + 1) - 4
        for l_seq in range(max(0, 2 * rem // 3 - 2), 2 * rem // 3 + 3):
            if (l_seq + 1) // 2 + l_seq == rem:
                r = make_rec(ref, pos, 0, b"xyz"[:extra], ((min(l_seq, 100) or 1, "M"),), l_seq, tag)
                assert len(r) == size
                return r
    raise AssertionError(size)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["two_blocks_exactly", "one_block_and_a_byte", "one_record"])
def test_index_of_streams_that_end_at_block_edges_is_the_spec(case):
    """a stream of exactly 2 x 0xff00 bytes whose first block ends with a record (the next one starts at in-block offset 0 and the
    call's end is a block's end), one of 0xff00 + 1 bytes, a single record"""
    from bitmapperbs_amd import mapper
    if case == "one_record":
        recs = [make_rec(3, 12345, 0, b"only", ((40, "M"),), 40)]
    else:
        total = 2 * BLK if case == "two_blocks_exactly" else BLK + 1
        recs, used = [], 0
        while BLK - used > 700:
            recs.append(make_rec(len(recs) % 2, 100 * len(recs), 0, b"r%d" % len(recs), ((75, "M"),), 150 + 7 * (len(recs) % 9), len(recs)))
            used += len(recs[-1])
        recs.append(_sized(BLK - used, 1, 1_000_000, 1))                              # the first block ends with this record
        used = BLK
        while total - used > 700:
            recs.append(make_rec(1, 2_000_000 + 100 * len(recs), 0, b"t%d" % len(recs), ((75, "M"),), 150, len(recs)))
            used += len(recs[-1])
        if total - used >= 60:
            recs.append(_sized(total - used, 1, 3_000_000, 2))
        else:                                                                           # (0xff00 + 1: the record that ends block 1 grows by a byte)
            recs[-1] = _sized(len(recs[-1]) + total - used, 1, 1_000_000, 1)
        assert sum(len(r) for r in recs) == total
    m = mapper.Mapper(None, 0)
    z, chunks, _, refs, _ = _index_equals_spec(m, recs[::-1])
    m.close()
    assert max(e for _, _, _, e in chunks) == len(z) << 16 == refs[-1][2]
    if case == "two_blocks_exactly":
        second = bgzf_blocks(z)[0][0] << 16
        assert any(b == second for _, _, b, _ in chunks) or any(b < second < e for _, _, b, e in chunks)


@pytest.mark.gpu
def test_index_errors_and_size_query():
    import ctypes as C
    from bitmapperbs_amd import capi, mapper
    m = mapper.Mapper(None, 0)
    with pytest.raises(RuntimeError, match="bmbs error -1: "):                       # BMBS_ESTATE: no call yet
        m.bam_sort_index()
    good = [make_rec(0, 20_000 * i, 0, b"g%d" % i, ((100, "M"),), 100, i) for i in range(9)] + [make_rec(-1, -1, 4, b"n", (), 30)]
    far = make_rec(0, (1 << 29) - 99, 0, b"far", ((100, "M"),), 100)                # end = 2^29 + 1
    lens = lambda rs: np.array([len(r) for r in rs], dtype=np.uint32)
    m.bam_sort(b"".join([far] + good), lens([far] + good))
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 9 .*BAI"):     # named by its place in the sorted order
        m.bam_sort_index()
    m.bam_sort(b"".join(good), lens(good), raw=True)
    with pytest.raises(RuntimeError, match="bmbs error -1: "):                       # BMBS_ESTATE: the last call was RAW
        m.bam_sort_index()
    z = m.bam_sort(b"".join(good), lens(good))
    nc = C.c_int64(-1); nw = C.c_int64(-1); nr = C.c_int64(-1); nn = C.c_uint64(99)
    lib = capi.lib()
    assert lib.bmbs_bam_sort_index(m._ctx, None, 0, C.byref(nc), None, 0, C.byref(nw), None, 0, C.byref(nr), C.byref(nn)) == -12
    chunks, wins, refs, nnc = bai_spec.spec_pieces(z)
    assert (nc.value, nw.value, nr.value, nn.value) == (len(chunks), len(wins), len(refs), nnc) == (9, 9, 1, 1)
    ch = np.zeros(nc.value, dtype=capi.BAI_CHUNK_DTYPE); wi = np.zeros(nw.value, dtype=capi.BAI_WIN_DTYPE); rf = np.zeros(nr.value, dtype=capi.BAI_REF_DTYPE)
    assert lib.bmbs_bam_sort_index(m._ctx, capi.ptr(ch), nc.value, C.byref(nc), capi.ptr(wi), nw.value - 1, C.byref(nw), capi.ptr(rf), nr.value, C.byref(nr), C.byref(nn)) == -12
    assert lib.bmbs_bam_sort_index(m._ctx, capi.ptr(ch), nc.value, C.byref(nc), capi.ptr(wi), nw.value, C.byref(nw), capi.ptr(rf), nr.value, C.byref(nr), C.byref(nn)) == 0
    assert [tuple(x) for x in ch.tolist()] == chunks and [tuple(x) for x in wi.tolist()] == wins
    m.bam_sort(b"", np.zeros(0, dtype=np.uint32))                                    # a call that returned no blocks
    with pytest.raises(RuntimeError, match="bmbs error -1: "):
        m.bam_sort_index()
    m.close()


@pytest.mark.gpu
def test_index_of_synthetic_records_on_the_plain_gather_path():
    """the same with BMBS_BSG_TINY=1 (every workgroup of k_bam_gather takes its plain path), in a process of its own"""
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]; import test_bai_index as t; t._synthetic_check()" % (ROOT, HERE)],
                       capture_output=True, text=True, env=dict(os.environ, BMBS_BSG_TINY="1"))
    assert p.returncode == 0 and "chunks " in p.stdout, p.stderr[-2000:]


# ---- GPU: the driver -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    """the golden genome's index, built once"""
    from bitmapperbs_amd import mapper
    wd = tmp_path_factory.mktemp("bai_gold")
    fa = str(wd / "genome.fa")
    gunzip_to(os.path.join(GOLD, "genome.fa.gz"), fa)
    mapper.Index.build(fa, fa, threads=4)
    return fa


def _inputs(kind, name, tmp_path):
    if kind == "se":
        fq = str(tmp_path / "r.fq")
        gunzip_to(os.path.join(GOLD, "se_%s.fq.gz" % name), fq)
        return ["--seq", fq]
    f1 = str(tmp_path / "1.fq"); f2 = str(tmp_path / "2.fq")
    gunzip_to(os.path.join(GOLD, "pe_%s_1.fq.gz" % name), f1)
    gunzip_to(os.path.join(GOLD, "pe_%s_2.fq.gz" % name), f2)
    return ["--seq1", f1, "--seq2", f2]


def _run(gold, inputs, args, out, env=None):
    cmd = [_driver(), "--search", gold] + inputs + ["-o", out, "--verbose", "--bam", "--sort"] + args
    p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stderr
    return p.stderr


def _payload(path):
    """the blocks of a BAM file without the header's (it holds the command line, which names the output file)"""
    raw = open(path, "rb").read()
    st = bai_spec._Stream(raw)
    _, skip = bai_spec._header_end(st.raw)
    return raw[st.voff(skip) >> 16:]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["se_e75", "pe_p75", "se_e75_unmapped"])
def test_driver_index_is_the_spec_and_finds_every_record(case, gold, tmp_path):
    """--bam --sort --bai: the index is the normal form of the file's, byte for byte; the file is the one the command writes without
    --bai; the lookup through the product's index returns exactly the overlapping records for 50 random regions and every reference's
    whole span; the counts of the index add up to the file's records"""
    pe_args = __import__("json").load(open(os.path.join(GOLD, "pe_args.json")))
    if case == "pe_p75":
        inputs, args = _inputs("pe", "p75", tmp_path), pe_args["p75"]
    else:
        inputs, args = _inputs("se", "e75", tmp_path), golden_args()["e75"] + (["--unmapped_out"] if case.endswith("unmapped") else [])
    out = str(tmp_path / "x.bam"); plain = str(tmp_path / "p.bam")
    err = _run(gold, inputs, args + ["--bai"], out)
    _run(gold, inputs, args, plain)
    assert not os.path.exists(plain + ".bai")
    bai = open(out + ".bai", "rb").read()
    assert bai == bai_spec.spec_bai(out)
    assert _payload(out) == _payload(plain)
    m = re.search(r"sort: .*index: chunks (\d+), windows (\d+), (\d+) bytes", err)
    assert m and int(m.group(3)) == len(bai), err
    raw = open(out, "rb").read()
    st = bai_spec._Stream(raw)
    ix = bai_spec.parse_bai(bai)
    assert int(m.group(1)) == sum(len(c) for r in ix["refs"] for c in r["bins"].values())
    n_ref, skip = bai_spec._header_end(st.raw)
    ref_len = []
    p = 12 + struct.unpack_from("<i", st.raw, 4)[0]
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", st.raw, p)[0]
        ref_len.append(struct.unpack_from("<i", st.raw, p + 4 + l_name)[0]); p += 8 + l_name
    n_records = len(list(bai_spec._walk(st, skip)))
    assert n_records > 500
    assert sum(r["meta"][2] + r["meta"][3] for r in ix["refs"] if r["meta"]) + ix["n_no_coor"] == n_records
    if case.endswith("unmapped"):
        assert ix["n_no_coor"] > 0
    rng = np.random.default_rng(12)
    regions = [(r, 0, ref_len[r]) for r in range(n_ref)]
    for _ in range(50):
        r = int(rng.integers(0, n_ref)); b = int(rng.integers(0, ref_len[r]))
        regions.append((r, b, min(ref_len[r], b + int(rng.choice([1, 200, 20_000])))))
    hits = 0
    for r, b, e in regions:
        want = bai_spec.brute_force(st, r, b, e)
        assert bai_spec.query(ix, st, r, b, e) == want, (r, b, e)
        hits += len(want)
    assert hits >= n_records - ix["n_no_coor"]


@pytest.mark.gpu
@pytest.mark.parametrize("bins", [None, "1"])
def test_driver_index_over_several_units(bins, gold, tmp_path):
    """pass-2 calls of at most UNIT_BUDGET bytes (and, with one sort bin, that bin cut into sub-units): the pieces of many calls,
    shifted and merged, are the normal form of the file's index; some chunk spans a call boundary, so the join is exercised"""
    inputs, args = _inputs("se", "b150", tmp_path), golden_args()["b150"]
    env = {"BMBS_SORT_CALL_BYTES": str(UNIT_BUDGET)}
    if bins:
        env["BMBS_SORT_BINS"] = bins
    out = str(tmp_path / "u.bam")
    err = _run(gold, inputs, args + ["--bai"], out, env)
    calls = int(re.search(r"pass-2 calls (\d+)", err).group(1))
    assert calls >= 4, err
    bai = open(out + ".bai", "rb").read()
    assert bai == bai_spec.spec_bai(out)
    # a call's last block is the only one of its blocks below 0xff00 bytes: the call boundaries of the file
    raw = open(out, "rb").read()
    blocks = bgzf_blocks(raw)
    st = bai_spec._Stream(raw)
    first = st.voff(bai_spec._header_end(st.raw)[1]) >> 16
    at, bounds = 0, []
    for bsize, data in blocks:
        at += bsize
        if at > first and 0 < len(data) < BLK:
            bounds.append(at << 16)
    bounds = bounds[:-1]                                                              # (the last call ends the records)
    assert UNIT_BUDGET < BLK and len(bounds) == calls - 1                             # (one block per call)
    ix = bai_spec.parse_bai(bai)
    spanning = [(b, e) for r in ix["refs"] for cl in r["bins"].values() for b, e in cl if any(b < x < e for x in bounds)]
    assert spanning, err
