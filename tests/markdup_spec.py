"""The duplicate-marking rule of `bmbs_search --bam --sort --markdup` (bmbs_bam_dup_sigs / bmbs_text_sorted_dup / bmbs_dup_select,
include/bmbs.h), restated as plain Python: Picard MarkDuplicates' pair-level rule, per template, with one deliberate departure
(DESIGN.md §7): "lo is read 1" is part of EVERY pair signature, because read 1 forward and read 1 reverse come from different
original strands of a bisulfite library.

A template is one record (single end) or the two records of a pair; a record is `bytes` (block_size word included) or None / b""
for "no record here".  Everything is exact integer arithmetic."""
import struct

DUP_NONE = 0x80000000
NO_SIG = (-1, -1, -1, -1, DUP_NONE, 0)


def _i32(x):
    x &= 0xffffffff
    return x - (1 << 32) if x >> 31 else x


def fields(rec: bytes):
    ref, pos, l_name, _mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHI", rec, 4)
    cigar = struct.unpack_from("<%dI" % n_cig, rec, 36 + l_name)
    q_at = 36 + l_name + 4 * n_cig + (l_seq + 1) // 2
    return ref, pos, flag, [(c & 15, c >> 4) for c in cigar], rec[q_at:q_at + l_seq]


def usable(rec) -> bool:
    """there, mapped, primary, with a CIGAR"""
    if not rec:
        return False
    n_cig, flag = struct.unpack_from("<HH", rec, 16)
    return not (flag & 4) and not (flag & 0x900) and n_cig > 0


def five_prime(rec: bytes):
    """(refID, 5' coordinate, strand, is read 1): forward pos - leading S/H, reverse pos + reference length + trailing S/H - 1"""
    ref, pos, flag, cigar, _ = fields(rec)
    clip = lambda ops: next((i for i, (op, _) in enumerate(ops) if op not in (4, 5)), len(ops))
    if flag & 16:
        reflen = sum(l for op, l in cigar if op in (0, 2, 3, 7, 8))          # M D N = X
        trail = sum(l for _, l in cigar[len(cigar) - clip(cigar[::-1]):])
        c = pos + reflen + trail - 1
    else:
        c = pos - sum(l for _, l in cigar[:clip(cigar)])
    return ref, _i32(c), (flag >> 4) & 1, (flag >> 6) & 1


def score(rec: bytes) -> int:
    """Picard's SUM_OF_BASE_QUALITIES: the qualities >= 15; 0xff (no quality) counts as 0"""
    return sum(q for q in fields(rec)[4] if 15 <= q != 0xff)


def signature(records):
    """records: the 1 or 2 records of a template -> (ref_lo, pos_lo, ref_hi, pos_hi, orient, score)"""
    ok = [r for r in records if usable(r)]
    if not ok:
        return NO_SIG
    if len(ok) == 1:                                     # single end, or the one usable record of a pair
        ref, c, strand, _ = five_prime(ok[0])
        return (ref, c, -1, -1, strand, score(ok[0]) & 0xffffffff)
    a, b = five_prime(ok[0]), five_prime(ok[1])
    # lo: the smaller end by (refID, coordinate); a tie goes to the forward strand, a further tie to read 1 (then to the first record)
    lo, hi = sorted([a, b], key=lambda e: (e[0], e[1], e[2], 1 - e[3]))
    return (lo[0], lo[1], hi[0], hi[1], lo[2] | (hi[2] << 1) | (lo[3] << 2) | 8, (score(ok[0]) + score(ok[1])) & 0xffffffff)


def signatures(records, paired: bool):
    """records in input order (None / b"": no record); paired: entries 2p and 2p + 1 are one template"""
    if paired:
        assert len(records) % 2 == 0
        return [signature(records[i:i + 2]) for i in range(0, len(records), 2)]
    return [signature([r]) for r in records]


def select(sigs):
    """dup[i] = 1 when template i loses its group: among equal (ref_lo, pos_lo, ref_hi, pos_hi, orient) the highest score stays,
    among equal scores the earliest; templates without a signature are never marked"""
    best = {}
    for i, s in enumerate(sigs):
        if s[4] & DUP_NONE:
            continue
        k = tuple(s[:5])
        if k not in best or s[5] > sigs[best[k]][5]:
            best[k] = i
    return [0 if (s[4] & DUP_NONE) or best[tuple(s[:5])] == i else 1 for i, s in enumerate(sigs)]


def mark(records, paired: bool):
    """the records with flag |= 0x400 (byte 19 |= 0x04) in every record of every duplicate template; nothing else changes"""
    dup = select(signatures(records, paired))
    out = []
    for i, r in enumerate(records):
        if r and dup[i >> 1 if paired else i]:
            r = r[:19] + bytes([r[19] | 0x04]) + r[20:]
        out.append(r)
    return out


# ---- record builder of the tests ---------------------------------------------------------------------------------------------------
CIGAR_OPS = "MIDNSHP=X"


def make_record(ref, pos, flag, cigar, quals, name=b"r", fill=0x12):
    """a BAM record (block_size word included): cigar = [(op letter or number, length)], quals = its quality bytes (l_seq of them)"""
    l_seq = len(quals)
    ops = b"".join(struct.pack("<I", (l << 4) | (CIGAR_OPS.index(op) if isinstance(op, str) else op)) for op, l in cigar)
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name) + 1, 30, 4681, len(cigar), flag, l_seq, -1, -1, 0) + name + b"\0" + ops + \
        bytes([fill]) * ((l_seq + 1) // 2) + bytes(quals)
    return struct.pack("<I", len(body)) + body
