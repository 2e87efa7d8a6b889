"""Read-end trimming and the M-bias table of the methylation calls (bmbs_bam_methyl_opts / bmbs_bam_sort_methyl_opts / bmbs_methyl_mbias,
`bmbs_search --methyl ... --methyl-ignore* --mbias`; the rule is in include/bmbs.h), restated as plain Python on top of methyl_spec.py.
Bismark's four --ignore* options and its M-bias report are the model.  Everything is exact integer arithmetic.

The CYCLE of a call is the 0-based position of the called read base in sequencing order: `ri` is the base's index in SEQ as the record
stores it (soft-clipped and inserted bases count; H and P are not in SEQ), cycle = ri for a forward record, l_seq - 1 - ri with flag
0x10.  The MATE of a record is 1 when flags 0x1 and 0x80 are both set, else 0.  A call of a record of mate m counts towards the sites
iff ignore_5p[m] <= cycle < l_seq - ignore_3p[m].  The mate-overlap clip stays geometric: it does not look at the trim.

The table is table[mate][strand][context][methylated][min(cycle, CYCLES - 1)] over every call that passes every filter EXCEPT the trim."""
import methyl_spec as spec

CYCLES = 1024
SHAPE = (2, 2, 3, 2, CYCLES)


def cycle_of(ri, l_seq, flag):
    return l_seq - 1 - ri if flag & 0x10 else ri


def mate_of(flag):
    return 1 if flag & 1 and flag & 0x80 else 0


def keeps(cycle, l_seq, mate, ignore_5p, ignore_3p):
    return ignore_5p[mate] <= cycle < l_seq - ignore_3p[mate]


def calls(rec, seqs, clip=0, min_phred=5):
    """(ref, pos, methylated, (context, strand), cycle) of every call of a record that counts, every context, no trim -- methyl_spec.calls
    with the read index kept"""
    ref, pos, _mapq, flag, cigar, bases, quals = spec.fields(rec)
    ob = spec.is_ob(flag)
    lo, hi = pos + (clip >> 16), pos + (clip >> 16) + (clip & 0xffff)
    seq = seqs[ref]
    r, i = pos, 0
    for op, l in cigar:
        if op in (0, 7, 8):
            for k in range(l):
                ri = i + k
                if ri >= len(bases):
                    break
                p = r + k
                q = quals[ri]
                if lo <= p < hi or (0 if q == 0xff else q) < min_phred:
                    continue
                if seq[p] != (spec.G if ob else spec.C):
                    continue
                ctx = spec.context(seq, p)
                if ctx is None:
                    continue
                if bases[ri] == (spec.SEQ_G if ob else spec.SEQ_C):
                    yield ref, p, 1, ctx, cycle_of(ri, len(bases), flag)
                elif bases[ri] == (spec.SEQ_A if ob else spec.SEQ_T):
                    yield ref, p, 0, ctx, cycle_of(ri, len(bases), flag)
            r += l; i += l
        elif op in (1, 4):
            i += l
        elif op in (2, 3):
            r += l


def walk(seqs, records, clip=None, min_mapq=10, min_phred=5):
    """[(record index, mate, l_seq, ref, pos, methylated, context, strand, cycle)] of every call of every record that counts, every
    context, no trim: what the sites and the table are both made of"""
    for j, rec in enumerate(records):
        spec.check(rec, seqs, j)
    out = []
    for j, rec in enumerate(records):
        if spec.skip_reason(rec, min_mapq):
            continue
        _r, _p, _q, flag, _c, bases, _ql = spec.fields(rec)
        for ref, p, m, (ctx, strand), cyc in calls(rec, seqs, clip[j] if clip is not None else 0, min_phred):
            out.append((j, mate_of(flag), len(bases), ref, p, m, ctx, strand, cyc))
    return out


def sites_of(walked, contexts=1, ignore_5p=(0, 0), ignore_3p=(0, 0)):
    """[(ref, pos, meth, unmeth, kind)] ordered by (ref, pos): the calls of the selected contexts that the trim keeps, added up"""
    acc = {}
    for _j, mate, l_seq, ref, p, m, ctx, strand, cyc in walked:
        if contexts >> ctx & 1 and keeps(cyc, l_seq, mate, ignore_5p, ignore_3p):
            a = acc.setdefault((ref, p), [0, 0, ctx | strand << 2])
            a[0 if m else 1] += 1
    return [(ref, p, a[0], a[1], a[2]) for (ref, p), a in sorted(acc.items())]


def table_of(walked, contexts=1):
    """the M-bias table as nested lists of SHAPE: every call of the selected contexts, whatever the trim"""
    t = [[[[[0] * CYCLES for _ in range(2)] for _ in range(3)] for _ in range(2)] for _ in range(2)]
    for _j, mate, _l, _ref, _p, m, ctx, strand, cyc in walked:
        if contexts >> ctx & 1:
            t[mate][strand][ctx][m][min(cyc, CYCLES - 1)] += 1
    return t


def sites(seqs, records, clip=None, contexts=1, min_mapq=10, min_phred=5, ignore_5p=(0, 0), ignore_3p=(0, 0)):
    """methyl_spec.sites with the trim"""
    return sites_of(walk(seqs, records, clip, min_mapq, min_phred), contexts, ignore_5p, ignore_3p)


def table(seqs, records, clip=None, contexts=1, min_mapq=10, min_phred=5):
    return table_of(walk(seqs, records, clip, min_mapq, min_phred), contexts)


def total(t):
    return sum(x for a in t for b in a for c in b for d in c for x in d)


def tsv(t):
    """the bytes of <prefix>_mbias.tsv: the entries with methylated + unmethylated > 0, ordered by context, strand, read, cycle"""
    out = ["#context\tstrand\tread\tcycle\tmethylated\tunmethylated\tpercent\n"]
    for ctx in range(3):
        for strand in range(2):
            for mate in range(2):
                for cyc in range(CYCLES):
                    me, un = int(t[mate][strand][ctx][1][cyc]), int(t[mate][strand][ctx][0][cyc])
                    if me + un:
                        out.append("%s\t%s\t%d\t%d\t%d\t%d\t%d\n" % (spec.CONTEXT_NAMES[ctx], "OB" if strand else "OT", mate + 1, cyc + 1, me, un, spec.pct(me, un)))
    return "".join(out).encode()
