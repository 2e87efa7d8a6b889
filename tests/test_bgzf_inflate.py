"""Conformance of the device's BGZF inflater (bmbs_inflate.hip: k_bgzf_inflate) and of the host's block-parallel one (csrc/pgz.h) on
deflate streams that zlib's compressor never writes: codes at the 15-bit limit for literals, lengths, distances and the end-of-block
symbol, every length and distance symbol at both ends of its extra bits, long matches that overlap themselves, windows filled to the
byte, block headers at every bit offset, the extremes of the dynamic header -- and the streams zlib's inflate refuses.

The streams come from tests/deflate_writer.py; the yardsticks are zlib's inflate and tests/deflate_spec.py, whose trace says what a stream
really holds.  The first part of this file runs without a GPU: every member meant to be accepted is read alike by both yardsticks and
shows the property it was built for (a case whose premise fails cannot quietly test nothing on the device), every member meant to be
refused is refused by both.  steps() is a model of how the kernel cuts a token stream into decode steps, for the premises that speak of
its 256-byte window.

One form the format cannot have is listed with the refusals instead of the headers: HCLEN 4 leaves the code-length code the symbols
16, 17, 18 and 0 only, so every code length is 0 and the end-of-block code is missing -- HCLEN 5 (which adds the length 8) is the
smallest header that can be accepted.  A decode step reads 128 bits, and no token is shorter than 2 bits (a one-bit length code and a
one-bit distance code): a chain of matches inside one window is at most 64 tokens deep, so the chains here are counted in the hops of a
byte's references (180 and more)."""
import functools
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import deflate_spec as ds
import deflate_writer as dw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FQ = b"ACGTN@+\n#,:FI0123456789./_-"


# ---- text ----------------------------------------------------------------------------------------------------------------------------------
def fastq(rng, records, length, tag=b"r"):
    """FASTQ-shaped text: whole records, qualities in runs, now and then a record a second time"""
    out = []
    for i in range(records):
        n = int(length if isinstance(length, int) else rng.integers(*length))
        seq = bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
        q = np.repeat(rng.choice(list(b"F:,#I"), n // 3 + 1, p=[.5, .2, .1, .1, .1]), rng.integers(1, 12, n // 3 + 1))[:n]
        q = np.resize(q, n)
        kind = rng.random()
        if kind < 0.3:
            q[:] = 70                                       # one long run
        elif kind < 0.5:
            q = np.resize(rng.choice(list(b"F:,#I"), int(rng.integers(2, 7))), n)       # a period of 2 .. 6
        out.append(b"@%s.%d/1\n%s\n+\n%s\n" % (tag, i, seq, bytes(q.astype(np.uint8))))
        if rng.random() < 0.25:
            out.append(out[int(rng.integers(0, len(out)))])
    return b"".join(out)


def lits(data):
    return [("lit", b) for b in data]


def filler(rng, n):
    return bytes(rng.choice(list(FQ[:12]), n).astype(np.uint8))


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
class Case:
    """a member: `text` the bytes it stands for (None: it is meant to be refused), `premise(blocks)` -> what the trace has to show"""
    def __init__(self, name, mem, text, premise=None):
        self.name, self.mem, self.text, self.premise = name, mem, text, premise
        self.payload = mem[18:-8]
        self.crc, self.isize = struct.unpack("<II", mem[-8:])

    def __repr__(self):
        return "<%s>" % self.name


def accepted(name, blocks, premise=None):
    raw = dw.deflate(blocks)
    text = dw.text_of(blocks)
    return Case(name, dw.member(raw, text), text, premise)


def dyn(tokens, opts=None, **kw):
    ll, d = dw.lengths_for(tokens, **kw)
    return ("dynamic", tokens, ll, d) + ((opts,) if opts else ())


def matches(blocks):
    return [t for b in blocks if b["btype"] for t in b["tokens"] if t[0] == "match"]


def verdicts(mem):
    """(zlib's reading of a member, the yardstick's): the text, or None where the member is refused"""
    d = zlib.decompressobj(31)
    try:
        a = d.decompress(mem)
        a = a if d.eof and d.unused_data == b"" else None
    except zlib.error:
        a = None
    try:
        b = ds.inflate_member(ds.parse_member(mem), False)[0]
    except ds.DeflateError:
        b = None
    return a, b


# ---- a model of the kernel's decode steps -----------------------------------------------------------------------------------------------------------
def steps(blocks, align=0):
    """how k_bgzf_inflate cuts the tokens of a member into steps when its text starts at an address = align mod 4: a step takes the plain
    tokens that START within 128 bits (two literals are one token where both codes fit into the 10-bit root table) until the text reaches
    256 bytes from the 4-byte boundary at or below the step's start; a token with a code longer than its root table (10 bits for
    literals / lengths, 9 for distances), a match longer than 250 and the end of a block are taken by the whole wave, between steps.
    -> [dict(start, lo, hi, toks [(text offset, length, distance or 0) ...], by_wave (text offset, length, distance) or None) ...]"""
    out = []
    n_out = 0
    for b in blocks:
        if b["btype"] == 0:
            n_out += b["stored_len"]
            continue
        ll, dl = (ds.FIXED_LL, ds.FIXED_D) if b["btype"] == 1 else (b["ll_lens"], b["d_lens"])
        toks = b["tokens"]
        i = 0
        done = False
        while not done:
            st = dict(start=n_out, lo=(align + n_out) & 3, toks=[], by_wave=None)
            t = 0
            run = 0
            while t < 128:
                if i == len(toks):                           # the end-of-block code
                    done = True
                    break
                k = toks[i]
                if k[0] == "lit":
                    l1 = ll[k[1]]
                    if l1 > 10:
                        st["by_wave"] = (n_out + run, 1, 0)
                        i += 1
                        break
                    two = i + 1 < len(toks) and toks[i + 1][0] == "lit" and l1 < 10 and l1 + ll[toks[i + 1][1]] <= 10
                    ol, bits, adv = (2, l1 + ll[toks[i + 1][1]], 2) if two else (1, l1, 1)
                    dist = 0
                else:
                    ol, dist = k[1], k[2]
                    if ll[k[3]] > 10 or dl[k[4]] > 9 or ol > 250:
                        st["by_wave"] = (n_out + run, ol, dist)
                        i += 1
                        break
                    bits, adv = ll[k[3]] + ds.LEN_EXTRA[k[3] - 257] + dl[k[4]] + ds.DIST_EXTRA[k[4]], 1
                if st["lo"] + run + ol > 256:
                    break
                st["toks"].append((n_out + run, ol, dist))
                run += ol
                t += bits
                i += adv
            st["hi"] = st["lo"] + run
            n_out += run + (st["by_wave"][1] if st["by_wave"] else 0)
            out.append(st)
    return out


def hops(st):
    """the longest chain of references among the bytes of one step's window"""
    depth = {}
    best = 0
    for at, ol, dist in st["toks"]:
        for p in range(at, at + ol):
            depth[p] = depth[p - dist] + 1 if dist and p - dist >= st["start"] else 0
            best = max(best, depth[p])
    return best


# ---- (a) codes ---------------------------------------------------------------------------------------------------------------------------------
def _deep_case(depth_ll, depth_d, seed):
    """literals on short codes, then a literal, a length symbol and the end-of-block symbol on codes of depth_ll bits, a distance symbol on
    one of depth_d bits, and matches of all four kinds: short / long length code with short / long distance code"""
    rng = np.random.default_rng(seed)
    body = filler(rng, 40)
    deep_lit, deep_len, short_len = ord("~"), 262, 258                       # lengths 8 and 4
    deep_d, short_d = 3, 5                                                   # distances 4 and 7..8
    tokens = lits(body) + [("lit", deep_lit), ("match", 4, 7), ("lit", 65), ("match", 4, 4), ("lit", 67), ("match", 8, 8), ("match", 8, 4),
                           ("lit", deep_lit), ("match", 8, 4), ("match", 4, 4)] + lits(body[:9])
    common = sorted(set(body) | {65, 67, short_len})
    extra_ll = [s for s in range(32, 127) if s not in common and s != deep_lit] + list(range(265, 280))
    ll = dw.complete_lengths(286, fixed={deep_lit: depth_ll, deep_len: depth_ll, 256: depth_ll}, fillers=common + extra_ll, depth=depth_ll)
    d = dw.complete_lengths(30, fixed={deep_d: depth_d}, fillers=[short_d] + [s for s in range(30) if s not in (deep_d, short_d)], depth=depth_d)

    def premise(blocks):
        b = blocks[0]
        m = matches(blocks)
        kinds = {(b["ll_lens"][t[3]] > 10, b["d_lens"][t[4]] > 9) for t in m}
        return (b["ll_lens"][deep_lit], b["ll_lens"][deep_len], b["ll_lens"][256], b["d_lens"][deep_d]) == (depth_ll, depth_ll, depth_ll, depth_d) and \
            len(kinds) == 4 and max(b["ll_lens"]) == depth_ll and max(b["d_lens"]) == depth_d and b["ll_lens"][short_len] <= 10 and b["d_lens"][short_d] <= 9
    return accepted("deep_ll%d_d%d" % (depth_ll, depth_d), [("dynamic", tokens, ll, d)], premise)


def _length_sweep(kind):
    """every length symbol at its smallest and largest extra bits, 258 both as symbol 285 and as 284 with 31 extra bits"""
    tokens = lits(b"ACGTTGCA")
    want = []
    for s in range(257, 286):
        base, ex = ds.LEN_BASE[s - 257], ds.LEN_EXTRA[s - 257]
        for length in sorted({base, base + (1 << ex) - 1}):
            tokens += [("match", length, 7 if s % 2 else 9, s), ("lit", 65 + s % 4)]
            want.append((length, s))
    blk = ("fixed", tokens) if kind == "fixed" else dyn(tokens)
    return accepted("length_sweep_" + kind, [blk],
                    lambda blocks: [(t[1], t[3]) for t in matches(blocks)] == want and (258, 284) in want and (258, 285) in want)


def _distance_sweep():
    """every distance symbol at its smallest and largest extra bits, 32768 among them, behind a stored block of 32 KiB"""
    rng = np.random.default_rng(21)
    tokens = []
    want = []
    for s in range(30):
        base, ex = ds.DIST_BASE[s], ds.DIST_EXTRA[s]
        for dist in sorted({base, base + (1 << ex) - 1}):
            tokens += [("match", 3 + s, dist), ("lit", 65 + s % 4)]
            want.append((dist, s))
    return accepted("distance_sweep", [("stored", filler(rng, 32768)), ("fixed", tokens)],
                    lambda blocks: [(t[2], t[4]) for t in matches(blocks)] == want and (32768, 29) in want and (1, 0) in want)


def _literal_pairs():
    """nine literals with codes of 2 .. 10 bits in every order of two: the table entries that hold two literals end where the two codes
    total 10 bits; 11 and more are two tokens"""
    letters = b"ACGTN#IF:"
    fixed = {c: 2 + i for i, c in enumerate(letters)}
    ll = dw.complete_lengths(257, fixed=fixed, fillers=[256, 10, 64, 43], limit=15)
    tokens = [("lit", a) for x in letters for y in letters for a in (x, y)]

    def premise(blocks):
        b = blocks[0]
        t = b["tokens"]
        sums = {b["ll_lens"][t[i][1]] + b["ll_lens"][t[i + 1][1]] for i in range(len(t) - 1)}
        return [b["ll_lens"][c] for c in letters] == list(range(2, 11)) and sums >= set(range(4, 21))
    return accepted("literal_pairs", [("dynamic", tokens, ll, [0])], premise)


@functools.lru_cache(None)
def family_a():
    cases = [_deep_case(a, b, 100 + a + b) for a, b in ((11, 10), (12, 11), (13, 12), (14, 13), (15, 14), (15, 15), (11, 15), (15, 10))]
    return cases + [_length_sweep("fixed"), _length_sweep("dynamic"), _distance_sweep(), _literal_pairs()]


# ---- (b) window assembly ---------------------------------------------------------------------------------------------------------------------------
OVERLAP_D = (1, 2, 3, 4, 5, 63, 64, 65, 249)
OVERLAP_L = (3, 250, 251, 258)


def _fill_case(extra):
    """a literal, a run of 250 and `extra` literals in the first 128 bits: with the text at the four alignments the window of the first
    step ends one byte short of 256, exactly at 256 and one byte past it"""
    tokens = [("lit", 71), ("match", 250, 1)] + lits(b"ACGTACGTAC"[:extra]) + [("match", 40, 5), ("lit", 84), ("match", 9, 251 + extra)] + lits(b"TTGA")
    return accepted("fill_%d" % (251 + extra), [("fixed", tokens)],
                    lambda blocks: all(steps(blocks, a)[0]["hi"] == min(256, a + 251 + extra) for a in range(4)))


def _overlap_case(dist, order):
    rng = np.random.default_rng(dist)
    tokens = lits(filler(rng, dist + 3))
    for length in order:
        tokens += [("match", length, dist), ("lit", 65 + length % 4)]
    return accepted("overlap_d%d_%s" % (dist, "up" if order[0] == 3 else "down"), [("fixed", tokens)],
                    lambda blocks: [(t[1], t[2]) for t in matches(blocks)] == [(length, dist) for length in order])


def _chain_case(length, dsym):
    """sixty matches of two bits each (a one-bit length code, the single one-bit distance code), every one a copy of the one before it"""
    dist = ds.DIST_BASE[dsym]
    tokens = lits(b"GATTACA"[:max(dist, 3)]) + [("match", length, dist)] * 60 + lits(b"CAT")
    ll = dw.complete_lengths(255 + length, fixed={254 + length: 1}, fillers=[65, 67, 71, 84, 256])
    d = [0] * dsym + [1]
    return accepted("chain_l%d_d%d" % (length, dist), [("dynamic", tokens, ll, d)],
                    lambda blocks: all(max(hops(st) for st in steps(blocks, a)) >= 80 for a in range(4)) and
                    all(max(len(st["toks"]) for st in steps(blocks, a)) >= 50 for a in range(4)))


def _sources(blocks, align):
    """the kinds of source the in-window matches of a member have, byte by byte as the kernel sees them: inside (every byte is a copy of a
    byte of the same step), before (every byte comes from in front of the step, the byte just in front of it not among them), edge (the
    same, and the last one is the byte just in front of the step), straddle (the first bytes come from in front of the step, the others
    from the step itself)"""
    kinds = set()
    for st in steps(blocks, align):
        for at, ol, dist in st["toks"]:
            if dist:
                ext = [p - dist for p in range(at, at + ol) if p - dist < st["start"]]
                kinds.add("inside" if not ext else "straddle" if len(ext) < ol else "edge" if ext[-1] == st["start"] - 1 else "before")
    return kinds


def _source_case():
    """matches right behind a token taken by the whole wave (a run of 258, a literal on a 12-bit code): the first token of the next step,
    whose source ends at the byte stored just before, lies wholly in front of it, or reaches from there into the step itself"""
    rng = np.random.default_rng(31)
    rare = ord("~")
    tokens = lits(filler(rng, 30))
    for k in range(6):
        stop = [("match", 258, 1 + k)] if k % 2 else [("lit", rare)]
        tokens += stop + [("match", 5 + k, 5 + k) if k < 3 else ("match", 9, 3), ("lit", 65), ("match", 7, 3), ("match", 6, 20 + k), ("lit", 67), ("lit", 71), ("match", 9, 5)] + lits(filler(rng, 7))
    common = sorted({t[1] for t in tokens if t[0] == "lit"} - {rare})
    used = sorted({ds.length_symbol(t[1]) for t in tokens if t[0] == "match"})
    ll = dw.complete_lengths(286, fixed={rare: 12}, fillers=common + used + [256] + list(range(97, 123)), depth=12)
    d = dw.lengths_for(tokens)[1]
    return accepted("sources", [("dynamic", tokens, ll, d)],
                    lambda blocks: all(_sources(blocks, a) == {"inside", "edge", "before", "straddle"} for a in range(4)))


def _first_token_case():
    rng = np.random.default_rng(32)
    return accepted("first_token_258_into_stored", [("stored", filler(rng, 300)), ("fixed", [("match", 258, 258), ("match", 258, 300), ("lit", 65)])],
                    lambda blocks: blocks[1]["tokens"][0][:3] == ("match", 258, 258))


@functools.lru_cache(None)
def family_b():
    cases = [_fill_case(x) for x in range(0, 9)]
    cases += [_overlap_case(d, o) for d in OVERLAP_D for o in (OVERLAP_L, OVERLAP_L[::-1])]
    cases += [_chain_case(3, 0), _chain_case(5, 2), _chain_case(4, 1), _source_case(), _first_token_case()]
    return cases


# ---- (c) block structure -----------------------------------------------------------------------------------------------------------------------------
def _header_offsets(blocks):
    """{(btype, bit offset of the block's header mod 8) ...} of a trace"""
    out = set()
    at = 0
    for b in blocks:
        out.add((b["btype"], at & 7))
        at += b["bits"]
    return out


def _alternating_case(seed):
    """stored (empty and not), fixed and dynamic blocks in turn, each Huffman block beginning with a match into the blocks before it: more
    are added until a header of every type has stood at every bit offset"""
    rng = np.random.default_rng(seed)
    blocks = [("fixed", lits(filler(rng, 12)))]
    have = 12
    while True:
        for kind in rng.integers(0, 3, 6):
            n = int(rng.integers(0, 6))
            if kind == 0:
                blocks.append(("stored", filler(rng, n if rng.random() < 0.7 else 0)))
                have += len(blocks[-1][1])
                continue
            toks = [("match", int(rng.integers(3, 12)), int(rng.integers(1, min(have, 1 << int(rng.integers(1, 12))) + 1)))] + lits(filler(rng, n)) + [("match", 4, int(rng.integers(1, 9)))]
            have += toks[0][1] + n + 4
            blocks.append(("fixed", toks) if kind == 1 else dyn(toks, {"header": "greedy" if rng.random() < 0.5 else "plain"}))
        trace = ds.inflate(dw.deflate(blocks))[1][:-1]       # (the last block would be written as the final one)
        if _header_offsets(trace) >= {(t, o) for t in (0, 1, 2) for o in range(8)} or len(blocks) > 400:
            break
    blocks.append(("fixed", []))                             # an empty final fixed block
    return accepted("alternating_%d" % seed, blocks,
                    lambda tr: _header_offsets(tr) >= {(t, o) for t in (0, 1, 2) for o in range(8)} and tr[-1]["btype"] == 1 and tr[-1]["tokens"] == [] and
                    any(b["btype"] == 0 and b["stored_len"] == 0 for b in tr) and
                    all(b["tokens"][0][0] == "match" for b in tr[1:-1] if b["btype"]))


def _big_cases():
    rng = np.random.default_rng(41)
    head = filler(rng, 30000)
    toks = []
    have = 30000
    while have + 258 <= 65536 - 100:
        toks.append(("match", 258, int(rng.integers(1, min(have, 32768) + 1))))
        have += 258
    toks += lits(filler(rng, 65536 - have))
    full = accepted("isize_65536", [("stored", head), ("fixed", toks)], lambda tr: True)
    stored = accepted("stored_65505", [("stored", filler(rng, 65505))], lambda tr: tr[0]["stored_len"] == 65505)
    assert len(full.text) == 65536 and len(stored.mem) == 65536
    return [full, stored]


@functools.lru_cache(None)
def family_c():
    only_eob = accepted("isize_0_only_end_of_block", [("dynamic", [], [0] * 256 + [1], [0])],
                        lambda tr: tr[0]["ll_lens"] == [0] * 256 + [1] and tr[0]["tokens"] == [])
    empties = [accepted("empty_fixed", [("fixed", [])], lambda tr: tr[0]["tokens"] == []),
               accepted("empty_stored", [("stored", b"")], lambda tr: tr[0]["stored_len"] == 0),
               accepted("stored_fixed_stored", [("stored", b"ACGT"), ("fixed", [("match", 4, 4)]), ("stored", b"\n")], lambda tr: len(tr) == 3)]
    return [_alternating_case(s) for s in (51, 52)] + [only_eob] + empties + _big_cases()


# ---- (d) dynamic headers -------------------------------------------------------------------------------------------------------------------------------
def _expand(syms):
    out = []
    for s, x in syms:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + x)
        else:
            out += [0] * ((3 if s == 17 else 11) + x)
    return out


def _header_case(name, syms, hlit, tokens, hclen=None, cl_lens=None):
    """a dynamic block whose header is the given code-length symbols; the premise: the lengths read back are their expansion and the
    header has exactly the bits those symbols take"""
    lens = _expand(syms)
    ll, d = lens[:hlit], lens[hlit:]
    assert 257 <= len(ll) <= 286 and 1 <= len(d) <= 30, (name, len(lens))
    opts = dict(header=syms, hclen=hclen, cl_lens=cl_lens)

    def premise(tr):
        b = tr[0]
        cc = dw.canonical(b["cl_lens"])
        bits = 17 + 3 * b["hclen"] + sum(cc[s][1] + dw.CL_EXTRA.get(s, 0) for s, _ in syms)
        return b["ll_lens"] == ll and b["d_lens"] == d and b["header_bits"] == bits and (hclen is None or b["hclen"] == hclen)
    return accepted("header_" + name, [("dynamic", tokens, ll, d, opts)], premise)


@functools.lru_cache(None)
def family_d():
    out = []
    text = lits(b"ACGTTGCAAC") + [("match", 6, 4), ("lit", 10)]
    # HLIT 257 / HDIST 1 / the smallest HCLEN that can be accepted (5: the symbols 16, 17, 18, 0 and 8) -- the byte values 1 .. 255 and the
    # end-of-block symbol, 8 bits each, no distance code
    all8 = [(0, 0), (8, 0)] + [(16, 3)] * 42 + [(16, 0)] + [(0, 0)]
    assert _expand(all8) == [0] + [8] * 256 + [0]
    out.append(_header_case("hlit257_hdist1_hclen5", all8, 257, lits(b"ACGT\nACGT\n"), hclen=5))
    # HLIT 286 / HDIST 30 / HCLEN 19, plain lengths: every symbol has a code
    ll = dw.complete_lengths(286, fillers=list(b"ACGT\n") + [256, 257, 258, 260] + [s for s in range(286) if s not in list(b"ACGT\n") + [256, 257, 258, 260]], depth=15)
    d = dw.complete_lengths(30, fillers=[3, 0, 1] + [s for s in range(30) if s not in (3, 0, 1)], depth=15)
    cl = dw.complete_lengths(19, fillers=sorted(set(ll + d), key=lambda s: -(ll + d).count(s)) + [s for s in range(19) if s not in ll + d], limit=7)
    out.append(_header_case("hlit286_hdist30_hclen19_plain", [(l, 0) for l in ll + d], 286, text, hclen=19, cl_lens=cl))
    out.append(_crossing_case())
    out.append(_repeat_case())
    # no distance code at all / the single one-bit distance code, for symbol 0 and for symbol 3
    out.append(accepted("no_distance_code", [dyn(lits(b"ACGTNACGT\n" * 3))], lambda tr: tr[0]["d_lens"] == [0] and tr[0]["hdist"] == 1))
    for dsym in (0, 3):
        dist = ds.DIST_BASE[dsym]
        toks = lits(b"ACGTN") + [("match", 9, dist), ("lit", 10), ("match", 251, dist), ("lit", 10)]
        out.append(accepted("one_distance_code_%d" % dsym, [dyn(toks)], lambda tr, dsym=dsym: tr[0]["d_lens"] == [0] * dsym + [1]))
    return out


def _crossing_case():
    """the last two literal/length lengths and the first two distance lengths are one length and three repeats of it: the 16 begins among
    the literal lengths and ends among the distance lengths"""
    ll = [0] * 259
    for s, l in ((65, 2), (67, 2), (71, 3), (84, 3), (10, 4), (256, 4), (257, 4), (258, 4)):
        ll[s] = l
    assert ds.kraft(ll)[0] == 1 << 15
    d = [4, 4] + [3] * 6 + [4, 4]
    assert ds.kraft(d)[0] == 1 << 15
    syms = dw.rle_lengths(ll[:257], "greedy") + [(4, 0), (16, 0)] + dw.rle_lengths(d[2:], "greedy")
    assert _expand(syms) == ll + d
    toks = lits(b"ACGT\nGATTACA") + [("match", 3, 1), ("match", 4, 2), ("lit", 10)]
    return _header_case("16_from_literals_into_distances", syms, 259, toks)


def _repeat_case():
    """16, 17 and 18 with their smallest and largest counts each, a 16 right behind an 18 and right behind a 17 (more zeros); the byte
    values that get codes are wherever the repeats leave them, and the text is written with those"""
    syms = [(17, 7), (3, 0),                                # 0 .. 9: the largest 17; 10: 3 bits
            (18, 0), (16, 0), (2, 0),                       # 11 .. 21: the smallest 18; 22 .. 24: the smallest 16, behind it; 25: 2 bits
            (17, 0), (16, 3), (3, 0),                       # 26 .. 28: the smallest 17; 29 .. 34: the largest 16, behind it; 35: 3 bits
            (18, 127), (3, 0),                              # 36 .. 173: the largest 18; 174: 3 bits
            (4, 0), (16, 0),                                # 175 .. 178: 4 bits, and three more
            (18, 66), (3, 0),                               # 179 .. 255; the end-of-block symbol: 3 bits
            (0, 0)]                                         # no distance code
    lens = _expand(syms)
    assert len(lens) == 258 and [i for i, l in enumerate(lens) if l] == [10, 25, 35, 174, 175, 176, 177, 178, 256]
    rng = np.random.default_rng(71)
    return _header_case("repeats_at_their_ends", syms, 257, lits(bytes(rng.choice([10, 25, 35, 174, 175, 176, 177, 178], 60).astype(np.uint8))))


# ---- (f) seeded fuzz -----------------------------------------------------------------------------------------------------------------------------------
def random_parse(text, rng, long_bias):
    """a random LZ parse of `text`: at every place a match with one of the earlier places that begin with the same three bytes -- the
    nearest ones first -- of a length drawn between 3 and what the texts share (258 at most; lengths around 250 where they share that
    much), or a literal"""
    tokens = []
    seen = {}
    i = 0
    n = len(text)
    while i < n:
        key = text[i:i + 3]
        cands = seen.get(key, ())
        tok = None
        if cands and rng.random() < 0.85:
            j = cands[-1 - min(len(cands) - 1, int(rng.geometric(0.5)) - 1)]
            m = 3
            while m < 258 and i + m < n and text[j + m] == text[i + m]:
                m += 1
            if m > 240 and rng.random() < long_bias:
                m = min(m, int(rng.integers(246, 259)))
            elif rng.random() < 0.5:
                m = int(rng.integers(3, m + 1))
            tok = ("match", m, i - j)
        step = tok[1] if tok else 1
        for p in range(i, min(i + step, n - 2)):
            seen.setdefault(text[p:p + 3], []).append(p)
        tokens.append(tok or ("lit", text[i]))
        i += step
    return tokens


def fuzz_member(seed):
    """-> (blocks, text): FASTQ-shaped text in a random parse, cut into blocks at random places, each stored, fixed or dynamic with codes
    of a random depth and a header coded plainly or greedily"""
    rng = np.random.default_rng(seed)
    text = fastq(rng, int(rng.integers(1, 4)), (30, 300), b"f%d" % seed)
    tokens = random_parse(text, rng, 0.8)
    cuts = sorted({int(x) for x in rng.integers(1, len(tokens), int(rng.integers(0, 4)))})
    blocks = []
    at = 0
    for a, b in zip([0] + cuts, cuts + [len(tokens)]):
        part = tokens[a:b]
        size = sum(t[1] if t[0] == "match" else 1 for t in part)
        kind = int(rng.integers(0, 8))
        if kind == 0:
            blocks.append(("stored", text[at:at + size]))
        elif kind == 1:
            blocks.append(("fixed", part))
        else:
            n_sym = len({t[1] if t[0] == "lit" else ds.length_symbol(t[1]) for t in part}) + 1
            n_d = len({dw.distance_symbol(t[2]) for t in part if t[0] == "match"})
            depth_ll = int(rng.integers(9, 16)) if rng.random() < 0.7 else None
            depth_d = int(rng.integers(6, 16)) if rng.random() < 0.7 else None
            more_ll = [int(x) for x in rng.choice(286, 30, replace=False)] if depth_ll and n_sym <= depth_ll + 1 else ()
            more_d = [int(x) for x in rng.choice(30, 20, replace=False)] if depth_d and n_d <= depth_d + 1 else ()
            blocks.append(dyn(part, {"header": "plain" if rng.random() < 0.3 else "greedy"}, depth_ll=depth_ll, depth_d=depth_d if n_d > 1 or more_d else None,
                              more_ll=more_ll, more_d=more_d, rare_first=bool(rng.random() < 0.3)))
        at += size
    assert at == len(text)
    return blocks, text


FUZZ_GROUPS, FUZZ_PER_GROUP = 8, 200


@functools.lru_cache(None)
def fuzz_group(group):
    out = []
    for seed in range(1000 * (group + 1), 1000 * (group + 1) + FUZZ_PER_GROUP):
        blocks, text = fuzz_member(seed)
        c = accepted("fuzz_%d" % seed, blocks)
        assert c.text == text, seed
        out.append(c)
    return out


# ---- (e) refusals ----------------------------------------------------------------------------------------------------------------------------------------
def refused_member(raw, note=None):
    """a raw stream meant to be refused, as a member whose ISIZE is honest: the length of what the yardstick read before it gave up"""
    try:
        part = ds.inflate(raw, 0, False)[0]
    except ds.DeflateError as e:
        part = e.partial
    return dw.member(raw, part)


def _raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return co.compress(data) + co.flush()


def malformed_streams():
    """every malformed form of test_spec_inflater_refuses_what_zlib_refuses (tests/test_bgzf_deflate.py), as (name, raw stream)"""
    ll = [0] * 257
    ok = list(ll); ok[65] = 1; ok[256] = 1
    over = list(ok); over[66] = 1
    thin = list(ll); thin[65] = 2; thin[256] = 2
    no_eob = list(ll); no_eob[65] = 1; no_eob[66] = 1
    withlen = list(ok) + [0]; withlen[65] = 2; withlen[256] = 2; withlen[257] = 1
    out = [("over_subscribed", dw.hand_built(over, [1], lambda w: w.code(1, 1))),
           ("incomplete", dw.hand_built(thin, [1], lambda w: w.code(1, 2))),
           ("incomplete_distances", dw.hand_built(ok, [2], lambda w: w.code(1, 1))),
           ("no_end_of_block", dw.hand_built(no_eob, [1], lambda w: w.code(1, 1))),
           ("unassigned_distance", dw.hand_built(withlen, [1], lambda w: (w.code(2, 2), w.code(0, 1), w.code(1, 1), w.code(3, 2)))),
           ("distance_before_the_start", dw.hand_built(withlen, [1], lambda w: (w.code(0, 1), w.code(0, 1), w.code(3, 2))))]
    for sym in (286, 287):
        w = dw.BitWriter(); w.put(1, 1); w.put(1, 2); w.code(0x30 + 65, 8); w.code(0xc0 + sym - 280, 8); w.code(0, 5); w.code(0, 7)
        out.append(("length_symbol_%d" % sym, w.bytes()))
    for dsym in (30, 31):
        w = dw.BitWriter(); w.put(1, 1); w.put(1, 2); w.code(0x30 + 65, 8); w.code(1, 7); w.code(dsym, 5); w.code(0, 7)
        out.append(("distance_symbol_%d" % dsym, w.bytes()))
    out += [("stored_nlen", b"\x01\x03\x00\xfc\xfeabc"), ("stored_len_twice", b"\x01\x03\x00\x03\x00abc"), ("btype_3", b"\x07")]
    # HCLEN 4: the code-length code has the symbols 16, 17, 18 and 0 only -- no length but 0 can be written, the end-of-block code is missing
    w = dw.BitWriter(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(0, 4)
    for l in (0, 0, 1, 1):
        w.put(l, 3)
    w.code(1, 1); w.put(127, 7); w.code(1, 1); w.put(109, 7)                       # 18: 138 zeros, 18: 120 zeros = 257 + 1 lengths
    out.append(("hclen_4", w.bytes()))
    # a repeat of the previous length with no length before it; a repeat that runs past the last length; HLIT 287; HDIST 31
    lens = [0] * 257; lens[65] = 1; lens[256] = 1
    out.append(("16_first", dw.deflate([("dynamic", [("lit", 65)], lens, [0], dict(header=[(16, 0)] + dw.rle_lengths(lens[3:] + [0], "greedy"), cl_lens=_cl_all()))])))
    out.append(("repeat_past_the_end", dw.deflate([("dynamic", [("lit", 65)], lens, [0], dict(header=dw.rle_lengths(lens, "greedy") + [(18, 0)], cl_lens=_cl_all()))])))
    for name, hlit, hdist in (("hlit_287", 287, 1), ("hdist_31", 257, 31), ("hdist_32", 257, 32)):
        ll2 = dw.complete_lengths(hlit, fillers=[65, 256])
        out.append((name, dw.deflate([("dynamic", [("lit", 65)], ll2, [0] * hdist)])))
    return out


def _cl_all():
    """a code-length code with a code for 0, 1, 16, 17 and 18"""
    return dw.complete_lengths(19, fillers=[0, 1, 18, 16, 17], limit=7)


def _overrun(strategy):
    """a member whose deflate data ends one byte inside its trailer: the text is varied until the last byte of its deflate stream is the
    first byte of its CRC-32; that byte is then left out of the payload (and of BSIZE).  Read with the trailer where BSIZE says, the
    stream goes on through the first CRC byte and all is well; zlib reads the CRC from where the deflate data really ends"""
    for k in range(100000):
        text = b"@r%d\nGATTACAGATTACCA\n+\nFFFFFFFF:FFFFFF\n" % k
        raw = _raw_deflate(text, 9, strategy)
        if raw[-1] == ds.crc32(text) & 0xff:
            return dw.member(raw[:-1], text), text
    raise AssertionError("no text found")


@functools.lru_cache(None)
def flipped_streams():
    """the per-bit flips of test_spec_inflater_and_zlib_agree_on_every_flipped_header_bit as members -> ([accepted Case ...], [refused
    Case ...]): where zlib still reads the flipped stream to its end, the trailer is written from what zlib read"""
    rng = np.random.default_rng(8)
    data = bytes(rng.choice(list(b"ACGTN#IIIIFF:,"), 600).astype(np.uint8)) + b"G" * 40
    good, bad = [], []
    for kind, z, nbits in (("dynamic", _raw_deflate(data, 9), 700), ("fixed", _raw_deflate(data, strategy=zlib.Z_FIXED), 120), ("stored", _raw_deflate(data, 0), 48)):
        for bit in range(nbits):
            raw = bytearray(z)
            raw[bit >> 3] ^= 1 << (bit & 7)
            raw = bytes(raw)
            d = zlib.decompressobj(-15)
            try:
                text = d.decompress(raw)
                ok = d.eof and d.unused_data == b""
            except zlib.error:
                ok = False
            name = "flip_%s_%d" % (kind, bit)
            if ok:
                good.append(Case(name, dw.member(raw, text), text))
            else:
                bad.append(Case(name, refused_member(raw), None))
        for cut in (1, 2, len(z) // 2, len(z) - 1):
            bad.append(Case("cut_%s_%d" % (kind, cut), refused_member(z[:cut]), None))
    return good, bad


@functools.lru_cache(None)
def family_e():
    """the members meant to be refused (the flipped ones apart)"""
    out = [Case(name, refused_member(raw), None) for name, raw in malformed_streams()]
    text = fastq(np.random.default_rng(61), 3, 80)
    raw = _raw_deflate(text, 9)
    out += [Case("wrong_crc", dw.member(raw, text, crc=ds.crc32(text) ^ 0x10000), None),
            Case("isize_one_too_small", dw.member(raw, text, isize=len(text) - 1), None),
            Case("isize_one_too_large", dw.member(raw, text, isize=len(text) + 1), None),
            Case("a_byte_behind_the_final_block", dw.member(raw + b"\0", text), None),
            Case("stored_final_block_cut_by_one", dw.member(_raw_deflate(text, 0)[:-1], text[:-1]), None)]
    for strategy, name in ((zlib.Z_DEFAULT_STRATEGY, "dynamic"), (zlib.Z_FIXED, "fixed")):
        out.append(Case("deflate_data_ends_inside_the_trailer_" + name, _overrun(strategy)[0], None))
    return out


# ---- no GPU: the premises ------------------------------------------------------------------------------------------------------------------------------
def check_accepted(cases):
    for c in cases:
        a, b = verdicts(c.mem)
        assert a == c.text, ("zlib", c.name)
        assert b == c.text, ("deflate_spec", c.name)
        if c.premise is not None:
            blocks = ds.inflate_member(ds.parse_member(c.mem))[1]
            assert c.premise(blocks), c.name


@pytest.mark.parametrize("family", ["a", "b", "c", "d"])
def test_premise_accepted_members_are_read_by_zlib_and_show_their_property(family):
    cases = {"a": family_a, "b": family_b, "c": family_c, "d": family_d}[family]()
    assert len({c.name for c in cases}) == len(cases)
    check_accepted(cases)


def test_premise_b_windows_end_one_short_at_and_one_past_256():
    """the first step of the fill cases over the four alignments: text that ends at window byte 255 and at 256 with tokens left over, and
    text that would end at 257, so that its last literal waits for the next step"""
    ends = {}
    for c in family_b():
        if c.name.startswith("fill"):
            tr = ds.inflate_member(ds.parse_member(c.mem))[1]
            for a in range(4):
                ends.setdefault(steps(tr, a)[0]["hi"], set()).add(a + int(c.name[5:]))
    print("first-step window ends: %s" % ends)
    assert 255 in ends[255] and 256 in ends[256] and 257 in ends[256] and set(ends) >= {251, 255, 256}


def test_premise_b_the_overlap_sweep_is_whole():
    seen = {(t[1], t[2]) for c in family_b() if c.name.startswith("overlap") for t in matches(ds.inflate_member(ds.parse_member(c.mem))[1])}
    assert seen == {(length, d) for length in OVERLAP_L for d in OVERLAP_D}


@pytest.mark.parametrize("group", range(FUZZ_GROUPS))
def test_premise_f_zlib_reads_every_fuzz_member(group):
    cases = fuzz_group(group)
    assert len(cases) == FUZZ_PER_GROUP                      # none is discarded
    check_accepted(cases)
    stats = dict(types=set(), ll=0, d=0, long_overlap=0, near_250=0, blocks=0)
    for c in cases:
        tr = ds.inflate_member(ds.parse_member(c.mem))[1]
        stats["blocks"] = max(stats["blocks"], len(tr))
        for b in tr:
            stats["types"].add(b["btype"])
            if b["btype"] == 2:
                stats["ll"] = max(stats["ll"], max(b["ll_lens"])); stats["d"] = max(stats["d"], max(b["d_lens"]))
        for t in matches(tr):
            stats["long_overlap"] += t[1] > 250 and 2 <= t[2] < t[1]
            stats["near_250"] += 246 <= t[1] <= 258
    print("fuzz group %d: %s" % (group, stats))
    assert stats["types"] == {0, 1, 2} and stats["ll"] == 15 and stats["d"] == 15 and stats["blocks"] >= 3
    assert stats["near_250"] >= 20


def test_premise_e_refused_members_are_refused_by_zlib_and_the_yardstick():
    good, bad = flipped_streams()
    cases = family_e() + bad
    for c in cases:
        assert verdicts(c.mem) == (None, None), c.name
        assert c.isize <= 65536 and struct.unpack("<H", c.mem[16:18])[0] + 1 == len(c.mem) >= 26, c.name
    check_accepted(good)
    print("refusals: %d members, %d of them flipped bits; %d flipped streams are still read" % (len(cases), len(bad), len(good)))
    assert len(bad) > 300 and len(good) > 100
    # the overrun members are what they say: the payload with the first CRC byte behind it is a whole deflate stream
    for c in cases:
        if c.name.startswith("deflate_data_ends_inside"):
            out, _, end = ds.inflate(c.payload + struct.pack("<I", c.crc))
            assert end == len(c.payload) + 1 and ds.crc32(out) == c.crc and len(out) == c.isize


# ---- no GPU: the host's inflater (csrc/pgz.h) ---------------------------------------------------------------------------------------------------------------
def _reader(path, threads, span):
    exe = os.path.join(ROOT, "bitmapperbs_amd", os.environ.get("BMBS_READER_TEST", "bmbs_reader_test"))
    assert os.path.exists(exe), "bmbs_reader_test is not built"
    env = dict(os.environ)
    env.pop("BMBS_GZ_SPAN", None)
    if span:
        env["BMBS_GZ_SPAN"] = str(span)
    return subprocess.run([exe, path, str(1 << 22), str(threads)], capture_output=True, timeout=120, env=env)


def as_gzip(c):
    """a corpus member without its BC subfield: a plain gzip member"""
    return dw.gzip_member(c.payload, b"", crc=c.crc, isize=c.isize)


def zlib_reads(z):
    """the text of a multi-member gzip file by zlib, None where zlib refuses a member or the file ends inside one"""
    out = b""
    while z:
        o = zlib.decompressobj(31)
        try:
            out += o.decompress(z)
        except zlib.error:
            return None
        if not o.eof:
            return None
        z = o.unused_data
    return out


@pytest.mark.parametrize("span", [4096, 0])
def test_host_inflater_reads_the_fastq_shaped_corpus(tmp_path, span):
    """the fuzz members (FASTQ text, whole records) as one plain gzip file of 1600 members through the driver's reader: the same text at
    1 and 5 threads, with cuts every 4 KiB and with the default span"""
    cases = [c for g in range(FUZZ_GROUPS) for c in fuzz_group(g)]
    src = str(tmp_path / "corpus.gz")
    with open(src, "wb") as f:
        f.write(b"".join(as_gzip(c) for c in cases))
    want = b"".join(c.text for c in cases)
    assert want.count(b"\n") % 4 == 0 and want.endswith(b"\n")
    for threads in (1, 5):
        p = _reader(src, threads, span)
        assert p.returncode == 0, (threads, p.stderr)
        assert p.stdout == want, (span, threads, len(p.stdout), len(want))


def test_host_inflater_refuses_what_zlib_refuses(tmp_path):
    """a good stretch of members, one refused member, a good member: the reader ends with an error.  (A member whose deflate data ends
    early or late is read by the host from where the data really ends, as zlib does; the bytes it then takes for the trailer do not match)"""
    from concurrent.futures import ThreadPoolExecutor
    good = fuzz_group(0)[:20]
    lead = b"".join(as_gzip(c) for c in good)
    want = b"".join(x.text for x in good)

    def one(c):
        src = str(tmp_path / (c.name + ".gz"))
        z = lead + as_gzip(c) + as_gzip(good[0])
        with open(src, "wb") as f:
            f.write(z)
        assert zlib_reads(z) is None, c.name
        for span in (4096, 0):
            p = _reader(src, 5, span)
            assert p.returncode != 0 and p.stderr, (c.name, span)
            assert want.startswith(p.stdout), c.name
    with ThreadPoolExecutor(4) as pool:
        list(pool.map(one, family_e() + flipped_streams()[1][::20]))


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bitmapperbs_amd import mapper
    m = mapper.Mapper(None, 0)
    yield m
    m.close()


def _pad(da, db):
    """stored members that move what follows by da bytes of BGZF and db bytes of text, mod 4: a member of n stored bytes is 31 + n long"""
    k = (db - da) % 4 or (4 if db % 4 else 0)               # k members: 3 k = da - db mod 4 (none at all only where nothing is to move)
    sizes = [db % 4] + [0] * (k - 1) if k else []
    return [accepted("pad", [("stored", b"\n" * n)]) for n in sizes]


def laid_out(cases):
    """the cases four times over, with padding members in front of each so that in pass r member i starts at an offset = r mod 4 and its
    text at an offset = r + i mod 4 -> ([Case ...] in order, {name: set of (member offset mod 4, text offset mod 4)})"""
    out, seen = [], {}
    at = tat = 0
    for r in range(4):
        for i, c in enumerate(cases):
            for p in _pad((r - at) % 4, (r + i - tat) % 4):
                out.append(p); at += len(p.mem); tat += len(p.text)
            assert (at % 4, tat % 4) == (r, (r + i) % 4)
            seen.setdefault(c.name, set()).add((at % 4, tat % 4))
            out.append(c); at += len(c.mem); tat += len(c.text)
    return out, seen


def device_reads(dev, cases, passes=True):
    order, seen = laid_out(cases) if passes else (list(cases), None)
    if seen:
        assert all({a for a, _ in s} == {0, 1, 2, 3} and {b for _, b in s} == {0, 1, 2, 3} for s in seen.values())
    got = dev.inflate_bgzf(b"".join(c.mem for c in order))
    want = b"".join(c.text for c in order)
    if got != want:
        at = 0
        for k, c in enumerate(order):
            assert got[at:at + len(c.text)] == c.text, "member %d of the call (%s, at %d, text at %d)" % (k, c.name, sum(len(x.mem) for x in order[:k]), at)
            at += len(c.text)
    assert len(got) == len(want)
    return len(order)


def raw_call(dev, members, isizes):
    """bmbs_inflate_bgzf on a list of members -> (return code, the text buffer, the error text)"""
    from bitmapperbs_amd import capi
    blk = np.cumsum([0] + [len(x) for x in members]).astype(np.uint64)
    out = np.cumsum([0] + list(isizes)).astype(np.uint64)
    a = np.frombuffer(b"".join(members), dtype=np.uint8)
    text = np.full(max(1, int(out[-1])), 0xee, dtype=np.uint8)
    rc = dev._lib.bmbs_inflate_bgzf(dev._ctx, capi.ptr(a), a.size, capi.ptr(blk), capi.ptr(out), len(members), capi.ptr(text), int(out[-1]), None, 0)
    return rc, text[:int(out[-1])].tobytes(), dev._lib.bmbs_last_error(dev._ctx).decode() if rc else ""


CANARY = (b"@canary/1\nGATTACAGATTACA\n+\nFFFFFFFFFF:F,#\n", b"@canary/2\nTTGACCA\n+\nIIIIIII\n")


def device_refuses(dev, cases):
    """per case one call of a canary member, the refused one and a second canary: the call has to fail and name block 1, and both canaries
    have to come back whole.  Every case is tried; the ones that went wrong are reported together"""
    front, back = (dw.member(_raw_deflate(t), t) for t in CANARY)
    wrong = []
    for c in cases:
        rc, text, msg = raw_call(dev, [front, c.mem, back], [len(CANARY[0]), c.isize, len(CANARY[1])])
        if rc == 0:
            wrong.append(c.name + ": accepted")
        elif "block 1 of this window" not in msg:
            wrong.append(c.name + ": " + msg)
        if text[:len(CANARY[0])] != CANARY[0] or text[len(CANARY[0]) + c.isize:] != CANARY[1]:
            wrong.append(c.name + ": a canary was overwritten")
    assert not wrong, "%d of %d: %s" % (len(wrong), len(cases), wrong[:40])


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["a", "b", "c", "d"])
def test_device_reads_the_family(dev, family):
    cases = {"a": family_a, "b": family_b, "c": family_c, "d": family_d}[family]()
    n = device_reads(dev, cases)
    print("family %s: %d cases, %d members in the call" % (family, len(cases), n))


@pytest.mark.gpu
def test_c_forty_members_in_one_call(dev):
    cases = (family_a() + family_d() + family_c()[:6] + family_b()[::2])[:40]
    assert len(cases) == 40
    assert device_reads(dev, cases, passes=False) == 40


@pytest.mark.gpu
@pytest.mark.parametrize("group", range(FUZZ_GROUPS))
def test_f_seeded_fuzz(dev, group):
    device_reads(dev, fuzz_group(group))


@pytest.mark.gpu
def test_e_flipped_streams_that_zlib_still_reads_are_read_alike(dev):
    device_reads(dev, flipped_streams()[0])


@pytest.mark.gpu
def test_e_malformed_members_are_refused(dev):
    """no stream is discarded: every member zlib refuses has to be refused here"""
    device_refuses(dev, family_e())


@pytest.mark.gpu
def test_e_flipped_and_cut_streams_are_refused(dev):
    bad = flipped_streams()[1]
    device_refuses(dev, bad)
    print("refused: %d flipped or cut streams, none discarded" % len(bad))


@pytest.mark.gpu
def test_e_one_bad_member_among_forty(dev):
    good = fuzz_group(1)[:40]
    for at, bad in ((0, "btype_3"), (17, "wrong_crc"), (39, "deflate_data_ends_inside_the_trailer_dynamic")):
        c = next(x for x in family_e() if x.name == bad)
        order = good[:at] + [c] + good[at + 1:]
        with pytest.raises(RuntimeError, match="block %d of this window" % at):
            dev.inflate_bgzf(b"".join(x.mem for x in order))
        rc, text, msg = raw_call(dev, [x.mem for x in order], [x.isize for x in order])
        assert rc != 0 and "block %d of this window" % at in msg
        pos = 0
        for k, x in enumerate(order):
            n = x.isize
            assert k == at or text[pos:pos + n] == x.text, (bad, k)
            pos += n
