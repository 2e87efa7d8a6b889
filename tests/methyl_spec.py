"""The methylation-calling rule of `bmbs_search --bam --sort --methyl` (bmbs_bam_methyl / bmbs_bam_sort_methyl / bmbs_methyl_sites /
bmbs_text_sorted_clip, include/bmbs.h), restated as plain Python.  It follows MethylDackel's defaults (records with any of the flags
0xF00 are out, MAPQ >= 10, base quality >= 5, the strand from the flags alone) and Bismark's --no_overlap for mates; the percent
rounding is defined here.  Everything is exact integer arithmetic.

The genome is the one the attached index holds: `seqs[ref]` = the letters of sequence `ref`, A0 C1 G2 T3 (genome_of_pac).  A record is
`bytes` with its block_size word, or None / b"" for "no record here"."""
import struct

A, C, G, T = 0, 1, 2, 3
CPG, CHG, CHH = 0, 1, 2
CONTEXT_NAMES = ("CpG", "CHG", "CHH")
SEQ_C, SEQ_T, SEQ_G, SEQ_A = 2, 8, 4, 1                 # BAM's 4-bit base codes ("=ACMGRSVTWYHKDBN")


def genome_of_pac(pac: bytes, chrom_len):
    """the index's packed genome (4 bases a byte, first base in the top bits) -> one bytes object of letters per sequence"""
    out, at = [], 0
    for n in chrom_len:
        out.append(bytes((pac[(at + i) >> 2] >> (6 - 2 * ((at + i) & 3))) & 3 for i in range(int(n))))
        at += int(n)
    return out


def context(seq, p):
    """(context, strand) of the cytosine at forward position p of one sequence, strand 0 = a forward C, 1 = a forward G; None: there is
    none, or it has no context (too close to the sequence's end)"""
    n = len(seq)
    if not 0 <= p < n:
        return None
    if seq[p] == C:
        if p + 1 < n and seq[p + 1] == G:
            return CPG, 0
        if p + 2 < n and seq[p + 2] == G:
            return CHG, 0
        return (CHH, 0) if p + 2 < n else None
    if seq[p] == G:
        if p - 1 >= 0 and seq[p - 1] == C:
            return CPG, 1
        if p - 2 >= 0 and seq[p - 2] == C:
            return CHG, 1
        return (CHH, 1) if p - 2 >= 0 else None
    return None


def fields(rec: bytes):
    """ref, pos, mapq, flag, cigar [(op, length)], the 4-bit base codes, the qualities"""
    ref, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHI", rec, 4)
    cigar = struct.unpack_from("<%dI" % n_cig, rec, 36 + l_name)
    s_at = 36 + l_name + 4 * n_cig
    q_at = s_at + (l_seq + 1) // 2
    packed = rec[s_at:q_at]
    bases = [(packed[i >> 1] >> (0 if i & 1 else 4)) & 15 for i in range(l_seq)]
    return ref, pos, mapq, flag, [(c & 15, c >> 4) for c in cigar], bases, rec[q_at:q_at + l_seq]


def ref_span(cigar):
    return sum(l for op, l in cigar if op in (0, 2, 3, 7, 8))            # M D N = X


def skip_reason(rec, min_mapq=10):
    """None when the record counts, else why it does not"""
    if not rec:
        return "none"
    ref, _pos, mapq, flag, cigar, _b, _q = fields(rec)
    if ref < 0 or flag & 4:
        return "unmapped"
    if flag & 0xF00:
        return "flag"
    if not cigar:
        return "cigar"
    if mapq < min_mapq:
        return "mapq"
    if flag & 1 and not flag & 2:
        return "improper"
    return None


def is_ob(flag):
    """the strand of a record from its flags alone: paired -- read 1 reverse or read 2 forward is OB; single -- reverse is OB"""
    if flag & 1:
        return bool((flag & 0x40 and flag & 0x10) or (flag & 0x80 and not flag & 0x10))
    return bool(flag & 0x10)


def check(rec, seqs, index):
    """what the calls refuse (BMBS_EINVAL, naming the record `index`)"""
    if not rec:
        return
    if len(rec) < 36 or struct.unpack_from("<I", rec, 0)[0] + 4 != len(rec):
        raise ValueError("the length given for record %d is not its block_size + 4" % index)
    ref, pos, l_name, _mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHI", rec, 4)
    if 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > len(rec):
        raise ValueError("the fields of record %d do not fit its length" % index)
    if ref >= len(seqs):
        raise ValueError("record %d: refID beyond the index's sequences" % index)
    if ref >= 0 and not flag & 4 and n_cig:
        span = ref_span(fields(rec)[4])
        if pos < 0 or pos + span > len(seqs[ref]):
            raise ValueError("record %d: its reference span runs off its sequence" % index)


def clip_of(rec2, rec1):
    """the clip word of one record given the other record of its pair: (beg - pos) << 16 | (end - beg) for [beg, end) = the intersection
    of the two reference spans, for the read-2 record (flag 0x80) only, when both are there, mapped, have a CIGAR and share refID; else 0"""
    if not rec2 or not rec1:
        return 0
    r2, p2, _m, f2, c2, _b, _q = fields(rec2)
    r1, p1, _m, f1, c1, _b, _q = fields(rec1)
    if not f2 & 0x80 or f2 & 4 or f1 & 4 or not c2 or not c1 or r1 != r2 or r2 < 0:
        return 0
    beg, end = max(p1, p2), min(p1 + ref_span(c1), p2 + ref_span(c2))
    if end <= beg:
        return 0
    if beg - p2 >= 1 << 16 or end - beg >= 1 << 16:
        raise ValueError("a reference span of 65536 bases and more")
    return (beg - p2) << 16 | (end - beg)


def clips(records):
    """records in input order, entries 2p and 2p + 1 a pair -> the clip word of each"""
    assert len(records) % 2 == 0
    return [clip_of(records[i], records[i ^ 1]) for i in range(len(records))]


def calls(rec, seqs, clip=0, min_phred=5):
    """(ref, pos, methylated, (context, strand)) of every call of a record that counts, every context"""
    ref, pos, _mapq, flag, cigar, bases, quals = fields(rec)
    ob = is_ob(flag)
    lo, hi = pos + (clip >> 16), pos + (clip >> 16) + (clip & 0xffff)
    seq = seqs[ref]
    r, i = pos, 0
    for op, l in cigar:
        if op in (0, 7, 8):                                              # M = X: a read base against a reference position
            for k in range(l):
                if i + k >= len(bases):                                      # (a CIGAR that asks for more bases than the record has)
                    break
                p, b = r + k, bases[i + k]
                q = quals[i + k]
                if lo <= p < hi or (0 if q == 0xff else q) < min_phred:
                    continue
                if seq[p] != (G if ob else C):
                    continue
                ctx = context(seq, p)
                if ctx is None:
                    continue
                if b == (SEQ_G if ob else SEQ_C):
                    yield ref, p, 1, ctx
                elif b == (SEQ_A if ob else SEQ_T):
                    yield ref, p, 0, ctx
            r += l; i += l
        elif op in (1, 4):                                               # I S: read only
            i += l
        elif op in (2, 3):                                               # D N: reference only
            r += l
        # H P: nothing


def sites(seqs, records, clip=None, contexts=1, min_mapq=10, min_phred=5):
    """[(ref, pos, meth, unmeth, kind)] ordered by (ref, pos), kind = context | strand << 2; contexts: 1 CpG | 2 CHG | 4 CHH"""
    acc = {}
    for j, rec in enumerate(records):
        check(rec, seqs, j)
    for j, rec in enumerate(records):
        if skip_reason(rec, min_mapq):
            continue
        for ref, p, m, (ctx, strand) in calls(rec, seqs, clip[j] if clip is not None else 0, min_phred):
            if contexts >> ctx & 1:
                a = acc.setdefault((ref, p), [0, 0, ctx | strand << 2])
                a[0 if m else 1] += 1
    return [(ref, p, a[0], a[1], a[2]) for (ref, p), a in sorted(acc.items())]


def select(all_sites, contexts):
    """the sites of sites(..., contexts=7) that a narrower selection keeps: a site's counts do not depend on the selection"""
    return [s for s in all_sites if contexts >> (s[4] & 3) & 1]


def pct(meth, unmeth):
    """the percentage, rounded half up"""
    return (200 * meth + meth + unmeth) // (2 * (meth + unmeth))


def bedgraph(prefix, ctx, chrom_names, all_sites):
    """the file of one context"""
    out = ['track type="bedGraph" description="%s %s methylation levels"\n' % (prefix, CONTEXT_NAMES[ctx])]
    for ref, p, m, u, kind in all_sites:
        if kind & 3 == ctx:
            out.append("%s\t%d\t%d\t%d\t%d\t%d\n" % (chrom_names[ref], p, p + 1, pct(m, u), m, u))
    return "".join(out).encode()


def non_acgt_runs(fasta_text: str):
    """per sequence of a FASTA the [beg, end) runs of bases that are not A, C, G or T (either case): the index holds a pseudo-random
    letter there"""
    runs = []
    for block in fasta_text.split(">")[1:]:
        seq = "".join(block.split("\n")[1:]).replace("\r", "").replace(" ", "").upper()
        r, i = [], 0
        while i < len(seq):
            if seq[i] in "ACGT":
                i += 1
                continue
            j = i
            while j < len(seq) and seq[j] not in "ACGT":
                j += 1
            r.append((i, j))
            i = j
        runs.append(r)
    return runs


def window(site):
    """the positions [lo, hi] a site's context was read from: the cytosine and the one (CpG) or two bases behind it on its strand"""
    _ref, p, _m, _u, kind = site
    w = 1 if kind & 3 == CPG else 2
    return (p - w, p) if kind & 4 else (p, p + w)


def drop_non_acgt(all_sites, runs):
    """the sites whose window touches no run"""
    def touches(s):
        lo, hi = window(s)
        return any(beg <= hi and end > lo for beg, end in runs[s[0]])
    return [s for s in all_sites if not touches(s)]


# ---- record builder of the tests ---------------------------------------------------------------------------------------------------
CIGAR_OPS = "MIDNSHP=X"
SEQ_CODES = "=ACMGRSVTWYHKDBN"


def make_record(ref, pos, flag, cigar, seq, quals, name=b"r", mapq=30):
    """a BAM record (block_size word included): cigar = [(op letter or number, length)], seq = its bases as letters or 4-bit codes,
    quals = its quality bytes (as many)"""
    codes = [SEQ_CODES.index(b) if isinstance(b, str) else int(b) for b in seq]
    assert len(codes) == len(quals)
    codes2 = codes + [0]
    packed = bytes(codes2[i] << 4 | codes2[i + 1] for i in range(0, len(codes), 2))
    ops = b"".join(struct.pack("<I", (l << 4) | (CIGAR_OPS.index(op) if isinstance(op, str) else op)) for op, l in cigar)
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name) + 1, mapq, 4681, len(cigar), flag, len(codes), -1, -1, 0) + name + b"\0" + ops + \
        packed + bytes(quals)
    return struct.pack("<I", len(body)) + body
