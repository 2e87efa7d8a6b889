"""The BAI index of a BAM file in plain Python, written from the SAM specification (section 5.2 "The BAI index format for BAM files",
reg2bin / reg2bins of section 5.3) and the push rules of htslib's hts_idx_push: the yardstick of tests/test_bai_index.py.  It uses none
of the product's code.

Per record: beg = pos (below 0: 0), end = pos + the reference length of its CIGAR (M D N = X), pos + 1 when flag 4 is set, there is no
CIGAR or that length is 0; bin = reg2bin(beg, end); a virtual offset is (file offset of the BGZF block) << 16 | offset inside the block's
data, and the offset "just behind" the last byte of a block is that of the next block's first byte.
  chunks  one per maximal run of consecutive records with equal (ref, bin): (ref, bin, offset of its first record, offset of the record
          behind it or of the end), ordered by (ref, bin, beg)
  wins    one per (ref, 16 kb window) a MAPPED record overlaps: the smallest offset among those records, ordered by (ref, win)
  refs    one per refID >= 0 with records: (ref, offset of its first record, offset behind its last, mapped, unmapped)
The normal form of the file (one index per BAM): n_ref of the header; per reference its bins in ascending number with the chunks in file
order (two of one bin joined when they touch), the pseudo-bin 37450, a linear index of 1 + the last window touched with empty windows
filled from the left (leading ones: the reference's first offset); then the count of records without a reference.  No compress_binning.
(A known property of BAI, not of this file: only mapped records enter the linear index, so a flag-4 record that has a coordinate and
lies in front of every mapped record of its window, in a chunk of its own, can be dropped by the linear-index cut.)"""
import struct

from common import _reg2bin, bgzf_blocks

PSEUDO_BIN = 37450
_REF_OPS = (0, 2, 3, 7, 8)                      # M D N = X


class _Stream:
    """the BGZF blocks of a byte string: the inflated stream and the virtual offset of each of its bytes"""

    def __init__(self, data: bytes):
        self.coff, self.ustart, raws = [], [], []
        at = u = 0
        for bsize, raw in bgzf_blocks(data):
            if raw:
                self.coff.append(at); self.ustart.append(u); raws.append(raw)
                u += len(raw)
            at += bsize
            if raw:
                self.behind = at                 # the first byte behind the last block that holds data
        self.raw = b"".join(raws)
        self.total = u
        self._blk = 0

    def voff(self, u: int) -> int:
        if u >= self.total:
            return self.behind << 16
        import bisect
        i = bisect.bisect_right(self.ustart, u) - 1
        return (self.coff[i] << 16) | (u - self.ustart[i])

    def tell_u(self, voff: int) -> int:
        import bisect
        c, o = voff >> 16, voff & 0xffff
        i = bisect.bisect_left(self.coff, c)
        if i >= len(self.coff) or self.coff[i] != c:
            assert c == self.behind and o == 0, voff
            return self.total
        return self.ustart[i] + o


def record_fields(raw: bytes, at: int):
    """-> (size with the block_size word, ref, beg, end, mapped) of the record at byte `at` of an inflated stream"""
    bs, ref, pos, l_name, _mapq, _bin, n_cig, flag = struct.unpack_from("<iiiBBHHH", raw, at)
    rl = 0
    if not flag & 4:
        for k in range(n_cig):
            c = struct.unpack_from("<I", raw, at + 36 + l_name + 4 * k)[0]
            if c & 15 in _REF_OPS:
                rl += c >> 4
    beg = max(pos, 0)
    return bs + 4, ref, beg, beg + (rl or 1), not flag & 4


def _walk(st: _Stream, skip: int):
    at = skip
    while at < st.total:
        size, ref, beg, end, mapped = record_fields(st.raw, at)
        yield at, ref, beg, end, mapped
        at += size
    assert at == st.total


def _pieces(st: _Stream, skip: int):
    recs = list(_walk(st, skip))
    offs = [st.voff(r[0]) for r in recs] + [st.voff(st.total)]
    chunks, wins, refs, n_no_coor = [], {}, {}, 0
    prev = None
    for i, (_, ref, beg, end, mapped) in enumerate(recs):
        if ref < 0:
            n_no_coor += 1
            prev = None
            continue
        assert end <= 1 << 29, "record %d: BAI cannot hold it" % i
        key = (ref, _reg2bin(beg, end))
        if key == prev:
            chunks[-1][3] = offs[i + 1]
        else:
            chunks.append([ref, key[1], offs[i], offs[i + 1]])
        prev = key
        if mapped:
            for w in range(beg >> 14, ((end - 1) >> 14) + 1):
                wins[(ref, w)] = min(wins.get((ref, w), offs[i]), offs[i])
        r = refs.setdefault(ref, [ref, offs[i], 0, 0, 0])
        r[2] = offs[i + 1]
        r[3 if mapped else 4] += 1
    chunks = sorted(tuple(c) for c in chunks)
    return chunks, [(r, w, o) for (r, w), o in sorted(wins.items())], [tuple(refs[r]) for r in sorted(refs)], n_no_coor


def spec_pieces(blocks_bytes: bytes):
    """BGZF blocks that hold records only (what bmbs_bam_sort returns) -> (chunks, wins, refs, n_no_coor), offsets relative to the
    first byte of the string"""
    return _pieces(_Stream(blocks_bytes), 0)


def _header_end(raw: bytes):
    assert raw[:4] == b"BAM\x01"
    p = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", raw, p)[0]
    return n_ref, p


def normal_form(n_ref: int, chunks, wins, refs, n_no_coor) -> bytes:
    out = [b"BAI\x01", struct.pack("<i", n_ref)]
    by_ref = {r[0]: r for r in refs}
    for ref in range(n_ref):
        if ref not in by_ref:
            out.append(struct.pack("<ii", 0, 0))
            continue
        bins = {}
        for r, b, beg, end in chunks:                      # (ordered by (ref, bin, beg): file order inside a bin)
            if r != ref:
                continue
            cl = bins.setdefault(b, [])
            if cl and cl[-1][1] == beg:
                cl[-1][1] = end
            else:
                cl.append([beg, end])
        out.append(struct.pack("<i", len(bins) + 1))
        for b in sorted(bins):
            out.append(struct.pack("<Ii", b, len(bins[b])))
            out += [struct.pack("<QQ", beg, end) for beg, end in bins[b]]
        _, rbeg, rend, n_mapped, n_unmapped = by_ref[ref]
        out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, rbeg, rend, n_mapped, n_unmapped))
        lin = {w: o for r, w, o in wins if r == ref}
        n_intv = max(lin) + 1 if lin else 0
        out.append(struct.pack("<i", n_intv))
        prev = rbeg
        for w in range(n_intv):
            prev = lin.get(w, prev)
            out.append(struct.pack("<Q", prev))
    out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


def spec_bai(bam_path: str) -> bytes:
    """the normal form of the index of a BAM file"""
    st = _Stream(open(bam_path, "rb").read())
    n_ref, skip = _header_end(st.raw)
    return normal_form(n_ref, *_pieces(st, skip))


def parse_bai(data: bytes):
    """-> {"refs": [{"bins": {bin: [(beg, end), ...]}, "meta": (beg, end, n_mapped, n_unmapped) or None, "lin": [...]}, ...],
    "n_no_coor": int or None}; every byte has to be used"""
    assert data[:4] == b"BAI\x01"
    n_ref = struct.unpack_from("<i", data, 4)[0]
    p = 8
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", data, p)[0]; p += 4
        bins, meta = {}, None
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", data, p); p += 8
            cl = [struct.unpack_from("<QQ", data, p + 16 * k) for k in range(n_chunk)]; p += 16 * n_chunk
            if b == PSEUDO_BIN:
                assert n_chunk == 2 and meta is None
                meta = cl[0] + cl[1]
            else:
                assert b not in bins and b < PSEUDO_BIN
                bins[b] = cl
        n_intv = struct.unpack_from("<i", data, p)[0]; p += 4
        lin = list(struct.unpack_from("<%dQ" % n_intv, data, p)); p += 8 * n_intv
        refs.append(dict(bins=bins, meta=meta, lin=lin))
    n_no_coor = None
    if p < len(data):
        n_no_coor = struct.unpack_from("<Q", data, p)[0]; p += 8
    assert p == len(data)
    return dict(refs=refs, n_no_coor=n_no_coor)


def reg2bins(beg: int, end: int):
    end -= 1
    out = [0]
    for sh, off in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(off + (beg >> sh), off + (end >> sh) + 1)
    return out


def query(bai, bam: bytes, ref: int, beg: int, end: int):
    """the standard lookup: the bins of reg2bins(beg, end), chunks that end at or before the linear offset of beg's window dropped, the
    records between the remaining chunks' offsets tested for overlap -> the sorted virtual offsets of the records found.
    bai: an index (bytes or parsed); bam: the whole file"""
    ix = parse_bai(bai) if isinstance(bai, (bytes, bytearray)) else bai
    st = bam if isinstance(bam, _Stream) else _Stream(bam)
    r = ix["refs"][ref]
    lin = r["lin"]
    min_off = lin[min(beg >> 14, len(lin) - 1)] if lin else 0
    chunks = sorted(c for b in reg2bins(beg, end) for c in r["bins"].get(b, ()) if c[1] > min_off)
    found = set()
    for cb, ce in chunks:
        at, stop = st.tell_u(cb), st.tell_u(ce)
        while at < stop:
            size, rref, rbeg, rend, _ = record_fields(st.raw, at)
            if rref == ref and rbeg < end and rend > beg:
                found.add(st.voff(at))
            at += size
        assert at == stop
    return sorted(found)


def brute_force(bam: bytes, ref: int, beg: int, end: int):
    """every record of the file on `ref` that overlaps [beg, end), by its virtual offset"""
    st = bam if isinstance(bam, _Stream) else _Stream(bam)
    _, skip = _header_end(st.raw)
    return sorted(st.voff(at) for at, rref, rbeg, rend, _ in _walk(st, skip) if rref == ref and rbeg < end and rend > beg)
