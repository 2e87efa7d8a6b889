"""The counterpart of tests/deflate_spec.py: a writer of deflate streams from RFC 1951, plain Python, no zlib and no project code.  It
writes what the caller says, legal or not: blocks of stored bytes or of tokens -- ("lit", byte), ("match", length, distance) or
("match", length, distance, length symbol) -- under the fixed code or under code lengths of the caller's choice, with the header of a
dynamic block run-length-coded plainly, greedily or symbol by symbol as given.  complete_lengths() makes complete codes of a wanted depth,
member() / gzip_member() wrap a raw stream as a BGZF or a plain gzip member, with a wrong CRC-32, ISIZE or BSIZE where asked."""
import struct

import deflate_spec as ds


class BitWriter:
    def __init__(self):
        self.v = 0
        self.n = 0

    def put(self, value, bits):
        self.v |= value << self.n
        self.n += bits

    def code(self, code, bits):                             # a Huffman code: most significant bit first
        for i in range(bits - 1, -1, -1):
            self.put((code >> i) & 1, 1)

    def align(self):
        self.n = (self.n + 7) & ~7

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def hand_built(ll, dist, body):
    """a dynamic block whose code-length code gives the lengths 0, 1, 2 and 3 two bits each: ll / dist = the code lengths to declare,
    body(w) writes what follows the header"""
    w = BitWriter()
    w.put(1, 1); w.put(2, 2); w.put(len(ll) - 257, 5); w.put(len(dist) - 1, 5); w.put(19 - 4, 4)
    cl = {0: 2, 1: 2, 2: 2, 3: 2}
    for s in ds.CL_ORDER:
        w.put(cl.get(s, 0), 3)
    for l in list(ll) + list(dist):
        w.code(l, 2)                                        # (four codes of two bits: the canonical code of symbol s is s)
    body(w)
    return w.bytes()


# ---- codes -------------------------------------------------------------------------------------------------------------------------------
def canonical(lens):
    """code lengths by symbol -> {symbol: (code, bits)} of the canonical code (RFC 1951 3.2.2)"""
    maxlen = max(lens) if len(lens) else 0
    count = [0] * (maxlen + 2)
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt = [0] * (maxlen + 2)
    code = 0
    for b in range(1, maxlen + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def complete_lengths(n, fixed=None, fillers=(), depth=None, limit=15, use_all=True):
    """a list of n code lengths that form a complete code: `fixed` {symbol: length} as given, what is left of the Kraft sum shared among
    the symbols of `fillers`, earlier ones getting the shorter codes.  depth: the longest code wanted (a leaf is split, the deepest one
    first, until one of that length exists); use_all: every filler gets a code (the shortest leaf is split until there is one each)"""
    fixed = dict(fixed or {})
    fillers = [s for s in fillers if s not in fixed]
    left = (1 << limit) - sum(1 << (limit - l) for l in fixed.values())
    assert left >= 0, "the fixed lengths are over-subscribed"
    ls = [limit - p for p in range(limit + 1) if left >> p & 1]
    assert len(ls) <= len(fillers), "not enough symbols for a complete code"
    if ls == [0]:
        assert len(fillers) >= 2
        ls = [1, 1]
    have = max(list(fixed.values()) + ls)
    if depth is not None:
        assert depth <= limit
        while have < depth:
            assert len(ls) < len(fillers), "not enough symbols for a code of depth %d" % depth
            l = max(ls)
            ls.remove(l)
            ls += [l + 1, l + 1]
            have = max(have, l + 1)
    cap = depth if depth is not None else limit
    while use_all and len(ls) < len(fillers):
        l = min(ls)
        assert l < cap, "too many symbols for a code of depth %d" % cap
        ls.remove(l)
        ls += [l + 1, l + 1]
    lens = [0] * n
    for s, l in fixed.items():
        lens[s] = l
    for s, l in zip(fillers, sorted(ls)):
        lens[s] = l
    assert ds.kraft(lens)[0] == 1 << 15, lens
    return lens


# ---- tokens -> bits --------------------------------------------------------------------------------------------------------------------------
def distance_symbol(dist):
    assert 1 <= dist <= 32768
    return max(i for i in range(30) if ds.DIST_BASE[i] <= dist)


def put_tokens(w, tokens, ll_lens, d_lens, eob=True):
    lc, dc = canonical(ll_lens), canonical(d_lens)
    for t in tokens:
        if t[0] == "lit":
            w.code(*lc[t[1]])
        elif t[0] == "match":
            length, dist = t[1], t[2]
            sym = t[3] if len(t) > 3 and t[3] is not None else ds.length_symbol(length)
            base, extra = ds.LEN_BASE[sym - 257], ds.LEN_EXTRA[sym - 257]
            assert 0 <= length - base < 1 << extra, t
            w.code(*lc[sym])
            w.put(length - base, extra)
            dsym = distance_symbol(dist)
            w.code(*dc[dsym])
            w.put(dist - ds.DIST_BASE[dsym], ds.DIST_EXTRA[dsym])
        else:
            raise ValueError(t)
    if eob:
        w.code(*lc[256])


def rle_lengths(lens, how):
    """the code lengths of a dynamic header as code-length symbols [(symbol, extra value) ...]: "plain" one symbol per length, "greedy" the
    longest repeat at every place: 18 for 11..138 zeros, 17 for 3..10, the length and then 16s of 3..6 for a run of another length"""
    if how == "plain":
        return [(l, 0) for l in lens]
    out = []
    i = 0
    while i < len(lens):
        v = lens[i]
        j = i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 3:
                k = min(run, 138)
                out.append((18, k - 11) if k >= 11 else (17, k - 3))
                run -= k
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3))
                run -= k
            out += [(v, 0)] * run
        i = j
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


def put_dynamic_header(w, final, ll_lens, d_lens, header="greedy", hclen=None, cl_lens=None):
    """BFINAL, BTYPE 2 and the header: HLIT = len(ll_lens), HDIST = len(d_lens); header: "plain", "greedy" or the code-length symbols
    themselves [(symbol, extra value) ...]; hclen: None = the fewest the code-length code allows; cl_lens: the code-length code's 19
    lengths (None: a complete code over the symbols used, frequent ones short, 7 bits at most)"""
    syms = rle_lengths(list(ll_lens) + list(d_lens), header) if isinstance(header, str) else list(header)
    if cl_lens is None:
        freq = {}
        for s, _ in syms:
            freq[s] = freq.get(s, 0) + 1
        used = sorted(freq, key=lambda s: (-freq[s], s))
        if len(used) == 1:
            used.append(0 if used[0] else 1)                 # zlib wants the code-length code complete: a second code of one bit
        cl_lens = complete_lengths(19, fillers=used, limit=7)
    need = max(i + 1 for i, s in enumerate(ds.CL_ORDER) if cl_lens[s])
    hclen = max(need, 4) if hclen is None else hclen
    assert hclen >= need
    w.put(final, 1); w.put(2, 2); w.put(len(ll_lens) - 257, 5); w.put(len(d_lens) - 1, 5); w.put(hclen - 4, 4)
    for s in ds.CL_ORDER[:hclen]:
        w.put(cl_lens[s], 3)
    cc = canonical(cl_lens)
    for s, x in syms:
        w.code(*cc[s])
        if s >= 16:
            w.put(x, CL_EXTRA[s])


def put_block(w, blk, final):
    """blk: ("stored", bytes) | ("fixed", tokens) | ("dynamic", tokens, ll_lens, d_lens[, {header=, hclen=, cl_lens=}])"""
    kind = blk[0]
    if kind == "stored":
        w.put(final, 1); w.put(0, 2)
        w.align()
        w.put(len(blk[1]), 16); w.put(len(blk[1]) ^ 0xffff, 16)
        for b in blk[1]:
            w.put(b, 8)
    elif kind == "fixed":
        w.put(final, 1); w.put(1, 2)
        put_tokens(w, blk[1], ds.FIXED_LL, ds.FIXED_D)
    else:
        put_dynamic_header(w, final, blk[2], blk[3], **(blk[4] if len(blk) > 4 else {}))
        put_tokens(w, blk[1], blk[2], blk[3])


def deflate(blocks):
    """the raw deflate stream of a list of blocks, the last one final"""
    w = BitWriter()
    for i, blk in enumerate(blocks):
        put_block(w, blk, int(i == len(blocks) - 1))
    return w.bytes()


def text_of(blocks):
    """the bytes a list of blocks stands for"""
    out = bytearray()
    for blk in blocks:
        if blk[0] == "stored":
            out += blk[1]
            continue
        for t in blk[1]:
            if t[0] == "lit":
                out.append(t[1])
            elif t[0] == "match":
                assert t[2] <= len(out), "distance too far back"
                for _ in range(t[1]):
                    out.append(out[-t[2]])
    return bytes(out)


def lengths_for(tokens, n_ll=None, n_d=None, depth_ll=None, depth_d=None, more_ll=(), more_d=(), rare_first=False):
    """complete literal/length and distance code lengths for a token list: the symbols used (and more_ll / more_d) get codes, frequent
    ones the shorter (rare_first: the other way round), of depth depth_ll / depth_d where given"""
    fl, fd = {256: 1}, {}
    for t in tokens:
        if t[0] == "lit":
            fl[t[1]] = fl.get(t[1], 0) + 1
        elif t[0] == "match":
            s = t[3] if len(t) > 3 and t[3] is not None else ds.length_symbol(t[1])
            fl[s] = fl.get(s, 0) + 1
            d = distance_symbol(t[2])
            fd[d] = fd.get(d, 0) + 1
    for s in more_ll:
        fl.setdefault(s, 0)
    for s in more_d:
        fd.setdefault(s, 0)
    sign = 1 if rare_first else -1
    ol = sorted(fl, key=lambda s: (sign * fl[s], s))
    od = sorted(fd, key=lambda s: (sign * fd[s], s))
    n_ll = n_ll or max(257, max(ol) + 1)
    n_d = n_d or max(1, max(od) + 1 if od else 1)
    if len(ol) == 1:
        ol.append(0)                                        # (the end-of-block code alone: a second symbol completes the code)
    ll = complete_lengths(n_ll, fillers=ol, depth=depth_ll)
    if not od:
        d = [0] * n_d
    elif len(od) == 1:
        d = [0] * n_d
        d[od[0]] = 1                                        # the single one-bit code zlib lets pass
    else:
        d = complete_lengths(n_d, fillers=od, depth=depth_d)
    return ll, d


# ---- gzip members ------------------------------------------------------------------------------------------------------------------------------
def member(raw, text, crc=None, isize=None, bsize=None):
    """a raw deflate stream as a BGZF member whose trailer speaks of `text`; crc / isize / bsize (the member's size) replace the true ones"""
    size = 18 + len(raw) + 8
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", (size if bsize is None else bsize) - 1) + bytes(raw) +
            struct.pack("<II", ds.crc32(text) if crc is None else crc, len(text) if isize is None else isize))


def gzip_member(raw, text, crc=None, isize=None):
    """the same as a plain gzip member, without an extra field"""
    return (b"\x1f\x8b\x08\0\0\0\0\0\0\xff" + bytes(raw) +
            struct.pack("<II", ds.crc32(text) if crc is None else crc, len(text) if isize is None else isize))
