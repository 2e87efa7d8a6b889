"""Conformance of the device's BGZF deflater (bmbs_bam.hip: k_bgzf_block, k_bgzf_gather) on bytes chosen to reach what BAM records of
reads never reach: stored blocks of full size, blocks without a single run, every run length at every bit offset of the parser's mask,
codes at the 15-bit limit, the largest header, every tail length and every alignment of trailer and gather.

The yardstick is tests/deflate_spec.py (an inflater written from RFC 1951 that keeps a trace of what it read) and zlib; the first part
of this file checks the yardstick against zlib and the premises of the generators, without a GPU.  The device tests go through
Mapper(None, 0).bam_sort: a stream is a few records whose first 36 bytes are a BAM core (refID 0, increasing pos, flag 0: already in
key order, so the sorted stream is the stream) and whose other bytes are the generator's."""
import heapq
import struct
import zlib

import numpy as np
import pytest

import deflate_spec as ds
from deflate_writer import BitWriter as _BitWriter, hand_built as _hand_built

BLK = 0xff00                                  # input bytes of a BGZF block
HDR = 36                                      # block_size word + the 32-byte core of a BAM record
SEG = 256                                     # input bytes one thread of k_bgzf_block parses


# ---- streams ---------------------------------------------------------------------------------------------------------------------------------
def record(pos, payload):
    core = struct.pack("<iiBBHHHIiii", 0, pos, 0, 0, 4680, 0, 0, 0, -1, -1, 0)
    return struct.pack("<I", len(core) + len(payload)) + core + bytes(payload)


def stream_of(payloads):
    """(stream, record lengths) of one record per payload"""
    recs = [record(i, p) for i, p in enumerate(payloads)]
    return b"".join(recs), np.array([len(r) for r in recs], dtype=np.uint32)


def framed(chosen, lead=None):
    """two records: the first fills block 0 together with the second's 36 bytes, so that `chosen` starts with block 1 and the blocks
    from there on hold nothing but chosen bytes"""
    if lead is None:
        lead = (np.arange(BLK - 2 * HDR) * 11 >> 3).astype(np.uint8).tobytes()
    assert len(lead) == BLK - 2 * HDR
    return stream_of([lead, chosen])


# ---- generators (numpy only) -------------------------------------------------------------------------------------------------------------------
def gen_uniform(seed, n, alphabet=256):
    """(a) / (b): uniform bytes below `alphabet`, patched until no three adjacent bytes are equal"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, alphabet, n).astype(np.uint8)
    while True:
        i = np.nonzero((b[2:] == b[1:-1]) & (b[1:-1] == b[:-2]))[0]
        if not i.size:
            return b.tobytes()
        b[i + 2] = (b[i + 2].astype(np.int64) + 1 + rng.integers(0, alphabet - 1, i.size)) % alphabet


def no_adjacent_equal(b, rng, values):
    """re-draws, front to back, every byte that equals its predecessor"""
    b = list(b)
    for i in range(1, len(b)):
        while b[i] == b[i - 1]:
            b[i] = int(values[int(rng.integers(0, len(values)))])
    return bytes(b)


def gen_skewed(seed, n, letters=12):
    """(c): a skewed alphabet of `letters` values, no two adjacent bytes equal"""
    rng = np.random.default_rng(seed)
    values = rng.choice(256, letters, replace=False)
    p = 1.0 / np.arange(1, letters + 1) ** 1.5
    return no_adjacent_equal(values[rng.choice(letters, size=n, p=p / p.sum())], rng, values)


def spread(counts, seed):
    """a byte string with counts[v] bytes of value v, shuffled, then mended by swaps until no two adjacent bytes are equal"""
    rng = np.random.default_rng(seed)
    b = np.repeat(np.arange(256, dtype=np.uint8), counts)
    rng.shuffle(b)
    b = b.tolist()
    n = len(b)

    def fits(v, i):                                         # may value v stand at i?
        return (i == 0 or b[i - 1] != v) and (i + 1 == n or b[i + 1] != v)
    for i in range(1, n):
        while b[i] == b[i - 1]:
            j = int(rng.integers(0, n))
            if abs(j - i) > 1 and fits(b[j], i) and fits(b[i], j):
                b[i], b[j] = b[j], b[i]
    return bytes(b)


# (g): the counts of 22 byte values, Fibonacci numbers all: 1, 2, 3, 5 .. 17711 and 2584 once more (48950 bytes).  With the end-of-block
# symbol's count of 1 the Huffman tree of 1, 2, 3, 5 .. is one chain whatever the order of ties: the node over everything up to F(k) weighs
# F(k+2) - 1, more than the next leaf and less than the one after.  (1, 1, 2, 3 .. would not do: the three ones pair off into two
# interleaved chains of half the depth.)
FIB22 = [1, 2]
while len(FIB22) < 21:
    FIB22.append(FIB22[-1] + FIB22[-2])
FIB22.append(2584)


def gen_deep(seed, bush, top=22):
    """(g): 22 byte values with the counts FIB22 (top: only the first `top` of them); with bush, 200 further values share what is left of
    a full block"""
    rng = np.random.default_rng(seed)
    values = rng.permutation(256)
    counts = np.zeros(256, dtype=np.int64)
    counts[values[:top]] = FIB22[:top]
    if bush:
        left = BLK - sum(FIB22)
        c = np.full(200, left // 200)
        c[:left % 200] += 1
        counts[values[22:222]] = c + np.where(np.arange(200) % 2 == 0, 20, -20)
    return spread(counts, seed + 1)


def gen_runs():
    """(e): runs of every length 1..300 over a background whose adjacent bytes always differ.  Four passes place each length at a start
    whose position within its 256-byte segment is: L * 37 mod 256 (every residue), 0, 256 - L mod 256 (the run ends at position 255), 250
    (the run straddles one segment edge, two from L = 263 on); then a run across a block edge, and one that ends the stream.
    -> (bytes, [(start, length) ...])"""
    n = 7 * BLK
    data = ((np.arange(n) * 7 + 3) & 0xff).astype(np.uint8)
    placed = []
    cursor = 0

    def place(start, L):
        v = L & 0xff
        while v == data[start - 1] or v == data[start + L]:
            v = (v + 1) & 0xff
        data[start:start + L] = v
        placed.append((start, L))
        return start + L
    for target in (lambda L: L * 37 % SEG, lambda L: 0, lambda L: (SEG - L) % SEG, lambda L: 250):
        for L in range(1, 301):
            start = cursor + 2
            start += (target(L) - start) % SEG
            cursor = place(start, L)
    edge = ((cursor + 64) // BLK + 1) * BLK
    cursor = place(edge - 20, 40)                            # 20 bytes at the end of a block, 20 at the start of the next
    cursor = place(edge + 3 * SEG - 9, 9)                    # ends at position 255 of a segment
    end = cursor + 500
    end += (77 - end) % SEG                                  # the stream ends inside a segment, with a run
    assert end + 1 < n
    place(end - 17, 17)
    return data[:end].tobytes(), placed


def gen_all_symbols(seed):
    """(h): a full block with all 256 byte values at very different frequencies, and 28 runs that give one match of each length symbol
    257..284 (a run of base + 1 bytes from position 0 of a segment: one literal and a match of the symbol's base length)"""
    rng = np.random.default_rng(seed)
    values = rng.permutation(256)
    p = 1.0 / np.arange(1, 257) ** 1.3
    body = values[rng.choice(256, size=BLK, p=p / p.sum())]
    body[:256] = values                                      # every value at least once
    b = bytearray(no_adjacent_equal(body, rng, values))
    for k in range(28):
        at = (2 + k) * SEG
        L = ds.LEN_BASE[k] + 1
        v = int(values[k])
        while v in (b[at - 1], b[at + L]):
            v = (v + 1) & 0xff
        b[at:at + L] = bytes([v]) * L
    return bytes(b)


def gen_fuzz(seed):
    """(k): 1..3 blocks of random pieces in 1..3 records -> the records' payloads"""
    rng = np.random.default_rng(seed)
    n_rec = int(rng.integers(1, 4))
    total = (int(rng.integers(1, 4)) - 1) * BLK + int(rng.integers(1, BLK + 1)) - n_rec * HDR
    total = max(total, 1)
    pieces = []
    have = 0
    while have < total:
        n = int(min(total - have, rng.integers(1, 1 << int(rng.integers(1, 16)))))
        kind = int(rng.integers(0, 5))
        if kind == 0:
            p = rng.integers(0, 256, n).astype(np.uint8)
        elif kind == 1:
            k = int(rng.integers(2, 40))
            w = 1.0 / np.arange(1, k + 1) ** float(rng.uniform(0.5, 3))
            p = rng.choice(256, k, replace=False)[rng.choice(k, size=n, p=w / w.sum())].astype(np.uint8)
        elif kind == 2:
            q = float(rng.uniform(0.01, 0.6))
            k = int(n * q) + 8                               # about 1 / q bytes per run
            p = np.resize(np.repeat(rng.integers(0, int(rng.integers(2, 257)), k), rng.geometric(q, k)), n).astype(np.uint8)
        elif kind == 3 and pieces:
            src = pieces[int(rng.integers(0, len(pieces)))]
            p = np.resize(src[int(rng.integers(0, len(src))):], n)
        else:
            nb = n // 3                                      # 4-bit bases two to a byte, then Phred 2..40
            base = np.array([1, 2, 4, 8], dtype=np.uint8)[rng.integers(0, 4, 2 * nb)]
            p = np.concatenate([base[0::2] << 4 | base[1::2], rng.integers(2, 41, n - nb).astype(np.uint8)])
        pieces.append(p)
        have += n
    data = np.concatenate(pieces).tobytes()
    cuts = sorted(int(x) for x in rng.integers(0, total + 1, n_rec - 1))
    return [data[a:b] for a, b in zip([0] + cuts, cuts + [total])]


# ---- a plain Huffman code (heapq): the cost of the best prefix code of a count table, and its depth ---------------------------------------------
def huffman_cost(counts):
    """(bits of the data under an optimal prefix code without a length limit, depth of its deepest leaf)"""
    heap = [(c, i, 0) for i, c in enumerate(c for c in counts if c)]
    heapq.heapify(heap)
    bits = 0
    tick = len(heap)
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        bits += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], tick, max(a[2], b[2]) + 1))
        tick += 1
    return bits, heap[0][2]


def literal_cost(data):
    counts = np.bincount(np.frombuffer(data, dtype=np.uint8), minlength=256).tolist() + [1]     # + the end-of-block symbol
    return huffman_cost(counts)


def longest_run(data):
    b = np.frombuffer(data, dtype=np.uint8)
    change = np.nonzero(np.concatenate([[True], b[1:] != b[:-1], [True]]))[0]
    return int(np.diff(change).max())


# ---- no GPU: the yardstick against zlib ------------------------------------------------------------------------------------------------------------
def _raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_every:
        return b"".join(co.compress(data[i:i + flush_every]) + co.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(data), flush_every)) + co.flush()
    return co.compress(data) + co.flush()


def _replay(blocks, data):
    """the bytes a trace's tokens stand for (the bytes of stored blocks are not in the trace: taken from `data`)"""
    out = bytearray()
    for b in blocks:
        if b["btype"] == 0:
            out += data[len(out):len(out) + b["stored_len"]]
            continue
        for t in b["tokens"]:
            if t[0] == "lit":
                out.append(t[1])
            else:
                for _ in range(t[1]):
                    out.append(out[-t[2]])
    return bytes(out)


def _samples():
    rng = np.random.default_rng(5)
    text = b"".join(b"@read%d\n%s\n+\n%s\n" % (i, bytes(rng.choice(list(b"ACGT"), 60).astype(np.uint8)), bytes(rng.integers(35, 75, 60).astype(np.uint8)))
                    for i in range(300))
    runs = b"".join(bytes([int(rng.integers(65, 70))]) * int(rng.integers(1, 600)) for _ in range(120))
    return {"text": text, "runs": runs, "random": bytes(rng.integers(0, 256, 20000).astype(np.uint8)), "deep": gen_deep(3, False, 19),
            "one": b"x", "empty": b""}


@pytest.mark.parametrize("form", ["l0", "l1", "l6", "l9", "fixed", "huffman_only", "rle", "full_flush"])
def test_spec_inflater_equals_zlib(form):
    kw = {"l0": dict(level=0), "l1": dict(level=1), "l6": dict(level=6), "l9": dict(level=9), "fixed": dict(strategy=zlib.Z_FIXED),
          "huffman_only": dict(strategy=zlib.Z_HUFFMAN_ONLY), "rle": dict(strategy=zlib.Z_RLE), "full_flush": dict(flush_every=1777)}[form]
    for name, data in _samples().items():
        z = _raw_deflate(data, **kw)
        assert zlib.decompress(z, -15) == data
        out, blocks, end = ds.inflate(z)
        assert out == data and end == len(z), (form, name)
        assert blocks[-1]["bfinal"] == 1 and all(b["bfinal"] == 0 for b in blocks[:-1])
        assert sum(b["bits"] for b in blocks[:-1]) + blocks[-1]["bits"] <= 8 * len(z)
        types = {b["btype"] for b in blocks}
        tokens = [t for b in blocks if b["btype"] for t in b["tokens"]]
        assert _replay(blocks, data) == data
        if form == "l0":
            assert types == {0} and sum(b["stored_len"] for b in blocks) == len(data)
        else:
            if form == "fixed":
                assert types == {1} if name == "text" else 2 not in types
            if form == "full_flush":
                assert 0 in types or not data                # (the empty stored block of a flush)
            if form == "huffman_only":
                assert all(t[0] == "lit" for t in tokens)
            if form == "rle":
                assert all(t[0] == "lit" or t[2] == 1 for t in tokens)
            for t in tokens:
                if t[0] == "match":
                    assert t[3] == ds.length_symbol(t[1]) and ds.DIST_BASE[t[4]] <= t[2] < ds.DIST_BASE[t[4]] + (1 << ds.DIST_EXTRA[t[4]])
        for b in blocks:
            if b["btype"] == 2:
                assert ds.kraft(b["ll_lens"])[0] == 1 << 15 and ds.kraft(b["cl_lens"])[0] == 1 << 15
                assert len(b["ll_lens"]) == b["hlit"] and len(b["d_lens"]) == b["hdist"]


def test_spec_inflater_reads_the_deep_trees_zlib_writes():
    """the generator of case (g) through zlib's Huffman-only coder: codes of 15 bits, read back exactly (zlib cuts a deflate block after
    32767 symbols: the chain has to be deeper than 15 inside one, so only its first 19 counts are used)"""
    for bush in (False, True):
        data = gen_deep(3, bush, 19)
        z = _raw_deflate(data, strategy=zlib.Z_HUFFMAN_ONLY)
        out, blocks, end = ds.inflate(z)
        assert out == data and end == len(z)
        assert max(max(b["ll_lens"]) for b in blocks if b["btype"] == 2) == 15


def _both(z):
    """(zlib's verdict, the yardstick's): the output, or None where the stream is refused"""
    d = zlib.decompressobj(-15)
    try:
        a = d.decompress(z)
        a = (a, len(z) - len(d.unused_data)) if d.eof else None      # (zlib.decompress refuses a stream that stops short)
    except zlib.error:
        a = None
    try:
        out, _, end = ds.inflate(z)
        b = (out, end)
    except ds.DeflateError:
        b = None
    return a, b


def test_spec_inflater_refuses_what_zlib_refuses():
    ll = [0] * 257
    ok = list(ll); ok[65] = 1; ok[256] = 1                   # 'A' = 0, end of block = 1
    # the yardstick accepts the well-formed one, and the single 1-bit distance code zlib lets pass
    a, b = _both(_hand_built(ok, [1], lambda w: (w.code(0, 1), w.code(0, 1), w.code(1, 1))))
    assert a == b == (b"AA", a[1])
    over = list(ok); over[66] = 1                            # three codes of one bit
    assert _both(_hand_built(over, [1], lambda w: w.code(1, 1))) == (None, None)
    thin = list(ll); thin[65] = 2; thin[256] = 2             # incomplete, and not the single one-bit code
    assert _both(_hand_built(thin, [1], lambda w: w.code(1, 2))) == (None, None)
    assert _both(_hand_built(ok, [2], lambda w: w.code(1, 1))) == (None, None)          # an incomplete distance code of two bits
    no_eob = list(ll); no_eob[65] = 1; no_eob[66] = 1
    assert _both(_hand_built(no_eob, [1], lambda w: w.code(1, 1))) == (None, None)
    # a match that uses the unassigned half of the one-bit distance code; a distance behind the start of the data
    withlen = list(ok) + [0]; withlen[65] = 2; withlen[256] = 2; withlen[257] = 1
    assert _both(_hand_built(withlen, [1], lambda w: (w.code(2, 2), w.code(0, 1), w.code(1, 1), w.code(3, 2)))) == (None, None)
    assert _both(_hand_built(withlen, [1], lambda w: (w.code(0, 1), w.code(0, 1), w.code(3, 2)))) == (None, None)
    a, b = _both(_hand_built(withlen, [1], lambda w: (w.code(2, 2), w.code(0, 1), w.code(0, 1), w.code(3, 2))))
    assert a == b == (b"AAAA", a[1])
    # fixed blocks: the length symbols 286 / 287 and the distance symbols 30 / 31 exist as codes and are refused
    for sym in (286, 287):
        w = _BitWriter(); w.put(1, 1); w.put(1, 2); w.code(0x30 + 65, 8); w.code(0xc0 + sym - 280, 8); w.code(0, 5); w.code(0, 7)
        assert _both(w.bytes()) == (None, None)
    for dsym in (30, 31):
        w = _BitWriter(); w.put(1, 1); w.put(1, 2); w.code(0x30 + 65, 8); w.code(1, 7); w.code(dsym, 5); w.code(0, 7)
        assert _both(w.bytes()) == (None, None)
    w = _BitWriter(); w.put(1, 1); w.put(1, 2); w.code(0x30 + 65, 8); w.code(1, 7); w.code(0, 5); w.code(0, 7)
    a, b = _both(w.bytes())
    assert a == b == (b"AAAA", a[1])
    # stored: LEN and NLEN
    assert _both(b"\x01\x03\x00\xfc\xffabc") == ((b"abc", 8),) * 2
    assert _both(b"\x01\x03\x00\xfc\xfeabc") == (None, None)
    assert _both(b"\x01\x03\x00\x03\x00abc") == (None, None)
    assert _both(b"\x07") == (None, None)                     # BTYPE 3


def test_spec_inflater_and_zlib_agree_on_every_flipped_header_bit():
    """a dynamic block, a fixed one and a stored one with each of their first bits flipped in turn: refused by both or read alike by both"""
    rng = np.random.default_rng(8)
    data = bytes(rng.choice(list(b"ACGTN#IIIIFF:,"), 600).astype(np.uint8)) + b"G" * 40
    refused = 0
    for z, nbits in ((_raw_deflate(data, 9), 700), (_raw_deflate(data, strategy=zlib.Z_FIXED), 120), (_raw_deflate(data, 0), 48)):
        assert ds.inflate(z)[0] == data
        for bit in range(nbits):
            bad = bytearray(z)
            bad[bit >> 3] ^= 1 << (bit & 7)
            a, b = _both(bytes(bad))
            assert a == b, bit
            refused += a is None
        for cut in (1, 2, len(z) // 2, len(z) - 1):
            assert _both(z[:cut]) == (None, None)
    assert refused > 300


def test_bgzf_member_parser():
    data = b"some bytes " * 50
    z = _raw_deflate(data)
    mem = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(z) + 25) + z + struct.pack("<II", zlib.crc32(data), len(data))
    two = mem + mem
    ms = ds.members(two)
    assert [m["bsize"] for m in ms] == [len(mem)] * 2 and ms[1]["end"] == len(two)
    assert ms[0]["payload"] == z and ms[0]["isize"] == len(data) and ms[0]["crc"] == zlib.crc32(data) and ms[0]["xlen"] == 6 and ms[0]["os"] == 255
    assert ds.inflate_member(ms[0])[0] == data
    assert ds.crc32(data) == zlib.crc32(data) and ds.crc32(b"") == 0
    # another subfield in front of BC is legal
    other = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x0b\0XY\x01\0\x07BC\x02\0" + struct.pack("<H", len(z) + 30) + z + struct.pack("<II", zlib.crc32(data), len(data))
    assert ds.inflate_member(ds.parse_member(other))[0] == data
    for bad in (b"\x1f\x8b\x08\x00" + mem[4:], mem[:12] + b"BD" + mem[14:], mem[:-1], mem[:16] + struct.pack("<H", len(mem) + 5) + mem[18:]):
        with pytest.raises(ds.DeflateError):
            ds.members(bad)
    for bad in (mem[:-8] + struct.pack("<II", zlib.crc32(data) ^ 1, len(data)), mem[:-4] + struct.pack("<I", len(data) + 1)):
        with pytest.raises(ds.DeflateError):
            ds.inflate_member(ds.parse_member(bad))


# ---- no GPU: the premises of the generators ----------------------------------------------------------------------------------------------------------
def test_premise_a_no_distance_1_coder_beats_stored_on_the_uniform_block():
    """no three adjacent bytes are equal, so a coder whose only matches are runs of >= 3 at distance 1 has nothing but literals, and the
    best prefix code for this block's literals and one end-of-block symbol -- a lower bound for any length-limited one, headers not
    counted -- is already larger than the stored form's blen + 5"""
    a = gen_uniform(1, BLK)
    assert len(a) == BLK and longest_run(a) <= 2
    bits, _ = literal_cost(a)
    print("case a: best literal-only body %d bytes, stored %d" % ((bits + 7) // 8, BLK + 5))
    assert (bits + 7) // 8 > BLK + 5
    for k in (250, 252, 254):
        b = gen_uniform(k, BLK, k)
        assert max(b) == k - 1 and longest_run(b) <= 2
        print("case b: %d values, best literal-only body %d bytes" % (k, (literal_cost(b)[0] + 7) // 8))


def test_premise_c_f_no_two_adjacent_bytes_are_equal():
    c = gen_skewed(2, BLK)
    assert longest_run(c) == 1 and len(set(c)) == 12
    assert (literal_cost(c)[0] + 7) // 8 < BLK // 2          # compressible: the dynamic form has to win
    for f in (b"AB" * (BLK // 2), b"ABC" * (BLK // 3)):
        assert len(f) == BLK and longest_run(f) == 1


def test_premise_e_the_runs_cover_the_parsers_cases():
    data, placed = gen_runs()
    b = np.frombuffer(data, dtype=np.uint8)
    # the runs of the data are exactly the placed ones: everything else is background
    change = np.nonzero(np.concatenate([[True], b[1:] != b[:-1], [True]]))[0]
    runs = {(int(s), int(e - s)) for s, e in zip(change[:-1], change[1:]) if e - s > 1}
    assert runs == {(s, L) for s, L in placed if L > 1}
    assert all(b[s - 1] != b[s] and (s + L == len(b) or b[s + L] != b[s]) for s, L in placed)
    for L in range(1, 301):
        assert sum(1 for _, l in placed if l == L) >= 4
    long = [(s, L) for s, L in placed if L >= 3]
    assert {s % 64 for s, _ in long} == set(range(64)) and {(s + 1) % 64 for s, _ in long} == set(range(64))
    assert {L for s, L in long if s % SEG == 0} >= set(range(3, 301))                    # starts at segment position 0
    assert {L for s, L in long if (s + L) % SEG == 0} >= set(range(3, 301))              # ends at position 255
    edges = lambda s, L: (s + L - 1) // SEG - s // SEG
    assert any(edges(s, L) == 1 for s, L in long) and any(edges(s, L) == 2 for s, L in long)
    assert any(s // BLK != (s + L - 1) // BLK for s, L in long)                          # across a block edge
    assert any(s + L == len(data) for s, L in long) and len(data) % SEG and len(data) % 4
    # every match length 3..256 is the run of "equals its predecessor" bytes of some run inside one segment of one block
    inside = set()
    for s, L in placed:
        p = s + 1                                            # bytes p .. s + L - 1 equal their predecessor
        while p < s + L:
            q = min(s + L, (p // SEG + 1) * SEG)
            inside.add(q - p if p % BLK else q - p - 1)      # (a block's first byte has no predecessor)
            p = q
    assert inside >= set(range(3, 257))


def test_premise_g_the_trees_are_deeper_than_15():
    for bush in (False, True):
        g = gen_deep(3, bush)
        counts = np.bincount(np.frombuffer(g, dtype=np.uint8), minlength=256)
        assert longest_run(g) == 1
        assert (len(g), int((counts > 0).sum())) == ((BLK, 222) if bush else (sum(FIB22), 22))
        rest = sorted(counts[counts > 0].tolist())
        for f in FIB22:
            rest.remove(f)                                   # the Fibonacci counts are all there
        assert len(rest) == (200 if bush else 0) and all(50 <= c <= 150 for c in rest)
        bits, depth = literal_cost(g)
        print("case g (bush %s): unlimited Huffman depth %d, body %d bytes" % (bush, depth, (bits + 7) // 8))
        assert depth > 15 and (bits + 7) // 8 < len(g) * 3 // 4


def test_premise_h_every_symbol_is_there():
    h = gen_all_symbols(4)
    assert len(h) == BLK and len(set(h)) == 256
    b = np.frombuffer(h, dtype=np.uint8)
    change = np.nonzero(np.concatenate([[True], b[1:] != b[:-1], [True]]))[0]
    runs = sorted(int(e - s) for s, e in zip(change[:-1], change[1:]) if e - s > 1)
    assert runs == sorted(x + 1 for x in ds.LEN_BASE[:28])
    assert [ds.length_symbol(r - 1) for r in runs] == list(range(257, 285))


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bitmapperbs_amd import mapper
    m = mapper.Mapper(None, 0)
    yield m
    m.close()


def device_members(m, stream, lens, trace=False):
    """the common checks of every case -> (the BGZF bytes, per member a dict: at, size, blen, btype, clen, and with trace its `blocks`)"""
    z = m.bam_sort(stream, lens)
    n = (len(stream) + BLK - 1) // BLK
    mem = ds.members(z)
    assert len(mem) == n
    at = 0
    out = []
    for i, x in enumerate(mem):
        blen = BLK if i < n - 1 else len(stream) - BLK * (n - 1)
        want = stream[i * BLK:i * BLK + blen]
        size = x["end"] - at
        d = zlib.decompressobj(31)                           # gzip framing: zlib checks CRC32 and ISIZE
        assert d.decompress(z[at:x["end"]]) == want and d.eof and d.unused_data == b"", i
        assert x["isize"] == blen and x["bsize"] == size and (x["xlen"], x["mtime"]) == (6, 0), i
        assert size <= 65536 and size <= blen + 31, (i, size, blen)
        raw, blocks = ds.inflate_member(x, trace)
        assert raw == want, i
        assert len(blocks) == 1 and blocks[0]["bfinal"] == 1, i
        info = dict(at=at, size=size, blen=blen, btype=blocks[0]["btype"], clen=len(x["payload"]))
        if blocks[0]["btype"] == 0:
            assert size == blen + 31, i
        else:
            assert blocks[0]["btype"] == 2, i
        if trace:
            info["blocks"] = blocks
        out.append(info)
        at = x["end"]
    assert at == len(z)
    assert m.inflate_bgzf(z) == stream
    assert m.bam_sort(stream, lens, raw=True) == stream
    return z, out


def _tokens(info):
    return info["blocks"][0]["tokens"]


def _matches(info):
    return [t for t in _tokens(info) if t[0] == "match"]


@pytest.mark.gpu
def test_a_uniform_block_is_stored_at_full_size(dev):
    a = gen_uniform(1, BLK)
    _, mem = device_members(dev, *framed(a))
    print("case a: member of %d bytes, BTYPE %d" % (mem[1]["size"], mem[1]["btype"]))
    assert mem[1]["btype"] == 0 and mem[1]["size"] == BLK + 31 == 65311


@pytest.mark.gpu
@pytest.mark.parametrize("values", [250, 252, 254])
def test_b_near_the_threshold_either_mode_is_well_formed(dev, values):
    b = gen_uniform(values, 2 * BLK, values)
    _, mem = device_members(dev, *framed(b))
    print("case b: %d values: members of %s bytes, BTYPE %s" % (values, [x["size"] for x in mem[1:]], [x["btype"] for x in mem[1:]]))


@pytest.mark.gpu
def test_c_a_block_without_a_run_is_dynamic_and_has_no_match(dev):
    _, mem = device_members(dev, *framed(gen_skewed(2, BLK)), trace=True)
    blk = mem[1]["blocks"][0]
    print("case c: member of %d bytes, BTYPE %d, %d tokens, HDIST %d, distance lengths %s" % (mem[1]["size"], blk["btype"], len(blk["tokens"]), blk["hdist"], blk["d_lens"]))
    assert blk["btype"] == 2 and not _matches(mem[1]) and len(blk["tokens"]) == BLK
    assert ds.kraft(blk["ll_lens"])[0] == 1 << 15


@pytest.mark.gpu
def test_d_one_byte_value_for_three_blocks(dev):
    _, mem = device_members(dev, *framed(b"\xa7" * (3 * BLK)), trace=True)
    for x in mem[1:]:
        t = _tokens(x)
        assert x["btype"] == 2 and t[0] == ("lit", 0xa7)
        assert all(k[0] == "match" and k[2] == 1 for k in t[1:])
        # at most 2 tokens per 256 input bytes of 15 + 5 + 15 bits, 5632 header bits, 26 bytes of framing: < 3000
        assert x["size"] < 3000
    print("case d: members of %s bytes, %s tokens" % ([x["size"] for x in mem[1:]], [len(_tokens(x)) for x in mem[1:]]))


@pytest.mark.gpu
def test_e_run_length_sweep(dev):
    data, placed = gen_runs()
    _, mem = device_members(dev, *framed(data), trace=True)
    lengths, symbols = set(), set()
    covered = np.zeros(len(data), dtype=bool)                # bytes that a match stands for
    for i, x in enumerate(mem[1:]):
        at = i * BLK                                         # (block 1 starts with the first chosen byte)
        for t in _tokens(x):
            if t[0] == "match":
                assert t[2] == 1 and t[4] == 0
                lengths.add(t[1]); symbols.add(t[3])
                covered[at:at + t[1]] = True
                at += t[1]
            else:
                at += 1
    print("case e: match lengths %d..%d (%d values), length symbols %d..%d" % (min(lengths), max(lengths), len(lengths), min(symbols), max(symbols)))
    assert lengths >= set(range(3, 257)) and max(lengths) <= 256
    assert symbols == set(range(257, 285))
    for s, L in placed:
        if L <= 2:
            assert not covered[s:s + L].any(), (s, L)
    b = np.frombuffer(data, dtype=np.uint8)
    assert not covered[np.concatenate([[True], b[1:] != b[:-1]])].any()      # a match never covers a byte that differs from its predecessor


@pytest.mark.gpu
def test_f_periods_of_two_and_three_have_no_match(dev):
    _, mem = device_members(dev, *framed(b"AB" * (BLK // 2) + b"ABC" * (BLK // 3 + 100)), trace=True)
    assert len(mem) == 4
    for x in mem[1:]:
        assert x["btype"] == 2 and not _matches(x) and len(_tokens(x)) == x["blen"]


@pytest.mark.gpu
@pytest.mark.parametrize("bush", [False, True])
def test_g_deep_trees_reach_15_bits_inside_a_block(dev, bush):
    _, mem = device_members(dev, *framed(gen_deep(3, bush)), trace=True)
    blk = mem[1]["blocks"][0]
    print("case g (bush %s): member of %d bytes, longest literal/length code %d, Kraft sum %d / %d" % ((bush, mem[1]["size"], max(blk["ll_lens"])) + ds.kraft(blk["ll_lens"])))
    assert blk["btype"] == 2 and max(blk["ll_lens"]) == 15
    assert ds.kraft(blk["ll_lens"])[0] == 1 << 15
    assert not _matches(mem[1])


@pytest.mark.gpu
def test_h_every_symbol_in_one_block(dev):
    _, mem = device_members(dev, *framed(gen_all_symbols(4)), trace=True)
    blk = mem[1]["blocks"][0]
    print("case h: member of %d bytes, HLIT %d, HDIST %d, HCLEN %d, header bits %d" % (mem[1]["size"], blk["hlit"], blk["hdist"], blk["hclen"], blk["header_bits"]))
    assert blk["btype"] == 2 and blk["hlit"] == 285
    assert all(blk["ll_lens"][s] for s in range(285))
    assert {t[3] for t in _matches(mem[1])} == set(range(257, 285)) and {t[1] for t in _tokens(mem[1]) if t[0] == "lit"} == set(range(256))
    assert ds.kraft(blk["ll_lens"])[0] == 1 << 15 and ds.kraft(blk["cl_lens"])[0] == 1 << 15


TAILS = [1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 511, 512, 513, BLK - 1]


@pytest.mark.gpu
def test_i_tail_lengths_and_trailer_alignments(dev):
    a = gen_uniform(6, 2 * BLK)
    seen = {0: set(), 2: set()}
    for t in TAILS:
        n = BLK + t - 3 * HDR
        for payload in (bytes([t & 0xff]) * n, a[:n]):
            _, mem = device_members(dev, *stream_of([payload[:1000], payload[1000:40000], payload[40000:]]))
            assert len(mem) == 2 and mem[1]["blen"] == t
            for x in mem:
                seen[x["btype"]].add((18 + x["clen"]) & 3)
    print("case i: trailer offsets mod 4: stored %s, dynamic %s" % (sorted(seen[0]), sorted(seen[2])))
    assert seen[0] == {0, 1, 2, 3} and seen[2] == {0, 1, 2, 3}


def _forty_blocks():
    a = gen_uniform(9, 9 * BLK + 5)
    c, d, g0, g1 = gen_skewed(2, BLK), b"\x11" * BLK, gen_deep(3, False), gen_deep(3, True)
    pieces = [a[:4 * BLK], c, d, g1, c[:30000], d[:777], g1, d, c, g0, a[4 * BLK:7 * BLK], d, g0, c, g1, d[:5000], g0, c]
    tail = a[7 * BLK:]
    fill = 38 * BLK + 5 - sum(len(p) for p in pieces) - len(tail)
    assert fill > 0
    pieces += [b"\x12" * (fill // 2), gen_skewed(7, fill - fill // 2), tail]
    return framed(b"".join(pieces))


@pytest.mark.gpu
def test_j_forty_blocks_in_one_call(dev):
    from bitmapperbs_amd import mapper
    stream, lens = _forty_blocks()
    z, mem = device_members(dev, stream, lens)
    sizes = [x["size"] for x in mem]
    print("case j: member sizes %s" % sizes)
    assert len(mem) == 40 and mem[-1]["blen"] == 5
    assert {x["at"] & 3 for x in mem} == {0, 1, 2, 3}
    assert any(max(p, q) == 65311 and min(p, q) < 100 for p, q in zip(sizes, sizes[1:]))
    assert {x["btype"] for x in mem} == {0, 2}
    for cap in (1000, len(z) - 1):
        with pytest.raises(mapper.BamSortNoRoom) as e:
            dev.bam_sort(stream, lens, cap=cap)
        assert e.value.needed == len(z)
    assert dev.bam_sort(stream, lens, cap=len(z)) == z


@pytest.mark.gpu
@pytest.mark.parametrize("group", range(8))
def test_k_seeded_fuzz(dev, group):
    for seed in range(100 + 5 * group, 105 + 5 * group):
        stream, lens = stream_of(gen_fuzz(seed))
        _, mem = device_members(dev, stream, lens)
        print("case k: seed %d: %d bytes in %d records -> members %s" % (seed, len(stream), len(lens), [(x["size"], x["btype"]) for x in mem]))
