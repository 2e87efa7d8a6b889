"""A yardstick for deflate streams, written from RFC 1951 / RFC 1952 / the BGZF section of the SAM specification: plain Python, no GPU,
no project code, no zlib.  inflate() decodes a raw deflate stream and keeps a trace of what it read -- per deflate block the BTYPE, the
code lengths and the token list -- so that a test can say WHICH forms of the format a compressor used, not only that its output
inflates.  It refuses what zlib's inflate refuses (tests/test_bgzf_deflate.py holds the differential against zlib)."""
import struct


class DeflateError(ValueError):
    pass


# RFC 1951 3.2.5: length symbols 257..285 and distance symbols 0..29 as (base, extra bits)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def length_symbol(length):
    """the symbol 257..285 that codes a match length 3..258"""
    assert 3 <= length <= 258
    if length == 258:
        return 285
    return 257 + max(i for i in range(28) if LEN_BASE[i] <= length)


def kraft(lens):
    """the Kraft sum of a list of code lengths, as (numerator, 2^15)"""
    return sum(1 << (15 - l) for l in lens if l), 1 << 15


def _table(lens, what, single_ok):
    """the decoding table of a canonical Huffman code (RFC 1951 3.2.2): a list of 2^maxlen entries indexed by the next maxlen bits of the
    stream (LSB first), each sym << 4 | len, or -1 where an incomplete code has no symbol; (table, maxlen).  Over-subscribed codes are
    refused; incomplete ones too, except a code whose longest length is 1 where single_ok (zlib's rule: inftrees.c)"""
    maxlen = max(lens) if lens else 0
    if maxlen == 0:
        return [-1, -1], 1                                        # no code at all: every use of it is an error
    count = [0] * (maxlen + 1)
    for l in lens:
        count[l] += 1
    count[0] = 0
    left = 1
    for b in range(1, maxlen + 1):
        left = 2 * left - count[b]
        if left < 0:
            raise DeflateError("over-subscribed %s code" % what)
    if left > 0 and not (single_ok and maxlen == 1):
        raise DeflateError("incomplete %s code" % what)
    nxt = [0] * (maxlen + 2)
    code = 0
    for b in range(1, maxlen + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    size = 1 << maxlen
    table = [-1] * size
    for sym, l in enumerate(lens):
        if not l:
            continue
        c = nxt[l]
        nxt[l] += 1
        rev = int(format(c, "0%db" % l)[::-1], 2)
        entry = sym << 4 | l
        step = 1 << l
        n = (size - rev + step - 1) // step
        table[rev::step] = [entry] * n
    return table, maxlen


class _Bits:
    """LSB-first bit reader over bytes"""
    def __init__(self, data, pos=0):
        self.data = data
        self.pos = pos            # next byte to take
        self.buf = 0
        self.cnt = 0

    def need(self, n):
        while self.cnt < n:
            if self.pos >= len(self.data):
                raise DeflateError("the stream ends inside a block")
            self.buf |= self.data[self.pos] << self.cnt
            self.pos += 1
            self.cnt += 8

    def take(self, n):
        self.need(n)
        v = self.buf & ((1 << n) - 1)
        self.buf >>= n
        self.cnt -= n
        return v

    def sym(self, table, maxlen, what):
        # (a code may be shorter than maxlen and the stream may end right behind it: peek what there is)
        while self.cnt < maxlen and self.pos < len(self.data):
            self.buf |= self.data[self.pos] << self.cnt
            self.pos += 1
            self.cnt += 8
        e = table[self.buf & ((1 << maxlen) - 1)]
        if e < 0:
            raise DeflateError("invalid %s code" % what)
        l = e & 15
        if l > self.cnt:
            raise DeflateError("the stream ends inside a block")
        self.buf >>= l
        self.cnt -= l
        return e >> 4

    def bit_pos(self):
        return self.pos * 8 - self.cnt

    def byte_pos(self):
        """the byte behind the last bit taken (whole bytes still in the buffer are given back)"""
        return self.pos - self.cnt // 8


def inflate(data, pos=0, trace=True):
    """a raw deflate stream starting at data[pos] -> (output bytes, [block trace ...], the byte offset behind the stream).
    A block trace is a dict: bfinal, btype, and for btype 2 hlit / hdist / hclen, cl_lens (the 19 code-length-code lengths by symbol),
    ll_lens, d_lens, header_bits (from BFINAL to the last code length); for btype 1 and 2 tokens, a list of ("lit", byte) and
    ("match", length, distance, length symbol, distance symbol), the end-of-block symbol not included; for btype 0 `stored_len`; `bits`,
    the size of the whole block.
    trace=False keeps no token lists.  A DeflateError carries the bytes that were read before it as its `partial`."""
    out = bytearray()
    try:
        return _inflate(data, pos, trace, out)
    except DeflateError as e:
        e.partial = bytes(out)
        raise


def _inflate(data, pos, trace, out):
    br = _Bits(data, pos)
    blocks = []
    while True:
        bit0 = br.bit_pos()
        bfinal = br.take(1)
        btype = br.take(2)
        blk = {"bfinal": bfinal, "btype": btype}
        if btype == 3:
            raise DeflateError("invalid block type")
        if btype == 0:
            br.pos -= br.cnt // 8                                # the rest of the current byte is skipped; whole bytes go back
            br.buf = 0
            br.cnt = 0
            if br.pos + 4 > len(data):
                raise DeflateError("the stream ends inside a block")
            ln, nln = struct.unpack_from("<HH", data, br.pos)
            if ln != (~nln & 0xffff):
                raise DeflateError("invalid stored block lengths")
            br.pos += 4
            if br.pos + ln > len(data):
                raise DeflateError("the stream ends inside a block")
            out += data[br.pos:br.pos + ln]
            br.pos += ln
            blk["stored_len"] = ln
        else:
            if btype == 1:
                ll_lens, d_lens = FIXED_LL, FIXED_D
            else:
                hlit = br.take(5) + 257
                hdist = br.take(5) + 1
                hclen = br.take(4) + 4
                if hlit > 286 or hdist > 30:
                    raise DeflateError("too many length or distance symbols")
                cl_lens = [0] * 19
                for i in range(hclen):
                    cl_lens[CL_ORDER[i]] = br.take(3)
                ct, cm = _table(cl_lens, "code lengths", False)
                lens = []
                while len(lens) < hlit + hdist:
                    s = br.sym(ct, cm, "code length")
                    if s < 16:
                        lens.append(s)
                        continue
                    if s == 16:
                        if not lens:
                            raise DeflateError("invalid bit length repeat")
                        v, n = lens[-1], 3 + br.take(2)
                    elif s == 17:
                        v, n = 0, 3 + br.take(3)
                    else:
                        v, n = 0, 11 + br.take(7)
                    if len(lens) + n > hlit + hdist:
                        raise DeflateError("invalid bit length repeat")
                    lens += [v] * n
                ll_lens, d_lens = lens[:hlit], lens[hlit:]
                if ll_lens[256] == 0:
                    raise DeflateError("invalid code -- missing end-of-block")
                blk.update(hlit=hlit, hdist=hdist, hclen=hclen, cl_lens=cl_lens, ll_lens=ll_lens, d_lens=d_lens,
                           header_bits=br.bit_pos() - bit0)
            lt, lm = _table(ll_lens, "literal/length", True)
            dt, dm = _table(d_lens, "distances", True)
            tokens = [] if trace else None
            while True:
                s = br.sym(lt, lm, "literal/length")
                if s < 256:
                    out.append(s)
                    if trace:
                        tokens.append(("lit", s))
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise DeflateError("invalid literal/length code")
                length = LEN_BASE[s - 257] + (br.take(LEN_EXTRA[s - 257]) if LEN_EXTRA[s - 257] else 0)
                d = br.sym(dt, dm, "distance")
                if d > 29:
                    raise DeflateError("invalid distance code")
                dist = DIST_BASE[d] + (br.take(DIST_EXTRA[d]) if DIST_EXTRA[d] else 0)
                if dist > len(out):
                    raise DeflateError("invalid distance too far back")
                if dist == 1:
                    out += out[-1:] * length
                elif dist >= length:
                    out += out[len(out) - dist:len(out) - dist + length]
                else:
                    piece = bytes(out[-dist:])
                    out += (piece * (length // dist + 1))[:length]
                if trace:
                    tokens.append(("match", length, dist, s, d))
            blk["tokens"] = tokens
        blk["bits"] = br.bit_pos() - bit0                      # header and all
        blocks.append(blk)
        if bfinal:
            break
    return bytes(out), blocks, br.byte_pos()


# ---- CRC-32 (RFC 1952 section 8) ---------------------------------------------------------------------------------------------------------
_CRC_TABLE = []
for _n in range(256):
    _c = _n
    for _ in range(8):
        _c = (_c >> 1) ^ 0xedb88320 if _c & 1 else _c >> 1
    _CRC_TABLE.append(_c)


def crc32(data):
    c = 0xffffffff
    t = _CRC_TABLE
    for b in data:
        c = t[(c ^ b) & 0xff] ^ (c >> 8)
    return c ^ 0xffffffff


# ---- BGZF (SAM specification 4.1): gzip members with a `BC` extra subfield that holds the member's size - 1 ----------------------------------
def parse_member(data, at=0):
    """the BGZF member at data[at]: a dict of its header fields (mtime, xfl, os, xlen), bsize (BSIZE + 1: the member's length), payload
    (the deflate data), crc, isize, end (the offset behind the member).  Nothing is inflated here."""
    if len(data) - at < 28:
        raise DeflateError("no room for a BGZF member at %d" % at)
    id1, id2, cm, flg, mtime, xfl, osb, xlen = struct.unpack_from("<BBBBIBBH", data, at)
    if (id1, id2, cm, flg) != (31, 139, 8, 4):
        raise DeflateError("not a BGZF member at %d: ID1 ID2 CM FLG = %r" % (at, (id1, id2, cm, flg)))
    bsize = None
    p, end_x = at + 12, at + 12 + xlen
    while p + 4 <= end_x:
        si1, si2, slen = struct.unpack_from("<BBH", data, p)
        if (si1, si2) == (66, 67):
            if slen != 2:
                raise DeflateError("BC subfield of %d bytes at %d" % (slen, at))
            bsize = struct.unpack_from("<H", data, p + 4)[0] + 1
        p += 4 + slen
    if p != end_x or bsize is None:
        raise DeflateError("no BC subfield in the extra field at %d" % at)
    if at + bsize > len(data) or bsize < 12 + xlen + 8:
        raise DeflateError("BSIZE of the member at %d does not fit" % at)
    crc, isize = struct.unpack_from("<II", data, at + bsize - 8)
    return dict(mtime=mtime, xfl=xfl, os=osb, xlen=xlen, bsize=bsize, payload=bytes(data[end_x:at + bsize - 8]), crc=crc, isize=isize, end=at + bsize)


def members(data):
    """the members of a BGZF byte string, in order"""
    out = []
    at = 0
    while at < len(data):
        out.append(parse_member(data, at))
        at = out[-1]["end"]
    return out


def inflate_member(m, trace=True):
    """a parsed member -> (its bytes, its block traces); the payload has to be used up exactly, CRC32 and ISIZE have to agree"""
    raw, blocks, end = inflate(m["payload"], 0, trace)
    if end != len(m["payload"]):
        raise DeflateError("%d bytes of the payload are behind the final block" % (len(m["payload"]) - end))
    if m["isize"] != len(raw) or m["crc"] != crc32(raw):
        raise DeflateError("CRC32 / ISIZE do not agree with the data")
    return raw, blocks
