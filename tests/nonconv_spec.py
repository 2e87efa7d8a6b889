"""The non-conversion filter of `bmbs_search --bam --sort --filter-non-conversion` (bmbs_bam_nonconv / bmbs_text_sorted_nonconv,
include/bmbs.h), restated as plain Python on top of tests/methyl_spec.py.  It follows Bismark's filter_non_conversion: a read with
several methylated cytosines outside CpG context is a read the bisulfite treatment did not convert, and either read fails its pair.
Everything is exact integer arithmetic.

A record is `bytes` with its block_size word, or None / b"" for "no record here"; `seqs` as in methyl_spec."""
from collections import namedtuple

import methyl_spec as spec

Params = namedtuple("Params", "threshold percent min_count min_phred")
DEFAULTS = Params(3, 0, 5, 0)                 # Bismark's --threshold and --minimum_count; no percent rule, no quality bound
QC_FAIL = 0x200                               # the flag a caller sets in every record of a failed template (record byte 19 |= 0x02)


def check_params(p):
    """what the calls refuse (BMBS_EINVAL)"""
    if p.threshold < 0 or p.min_count < 0 or not 0 <= p.percent <= 100 or not 0 <= p.min_phred <= 255:
        raise ValueError("bad parameters")


def examined(rec):
    """there, on a reference, mapped, with a CIGAR, neither secondary nor supplementary; MAPQ, the proper-pair flag, 0x200 and 0x400
    are not looked at"""
    if not rec:
        return False
    ref, _pos, _mapq, flag, cigar, _b, _q = spec.fields(rec)
    return ref >= 0 and not flag & 4 and not flag & 0x900 and bool(cigar)


def tally(rec, seqs, min_phred=0):
    """[context][0 unmethylated, 1 methylated] = the calls of an examined record (methyl_spec.calls: the strand from the flags, M = X,
    the context from the genome, no clip, no trim); None when the record is not examined"""
    if not examined(rec):
        return None
    t = [[0, 0], [0, 0], [0, 0]]
    for _ref, _p, m, (ctx, _strand) in spec.calls(rec, seqs, clip=0, min_phred=min_phred):
        t[ctx][m] += 1
    return t


def counts_of(t):
    """(nm, nu) of a record's tally: the methylated / unmethylated calls in CHG and CHH together; 0, 0 when it is not examined"""
    return (0, 0) if t is None else (t[spec.CHG][1] + t[spec.CHH][1], t[spec.CHG][0] + t[spec.CHH][0])


def counts(rec, seqs, min_phred=0):
    return counts_of(tally(rec, seqs, min_phred))


def fails(nm, nu, params=DEFAULTS):
    if params.threshold > 0 and nm >= params.threshold:
        return True
    return params.percent > 0 and nm + nu >= params.min_count and 100 * nm >= params.percent * (nm + nu)


def verdicts(tallies, paired, params=DEFAULTS):
    """the tallies of records in input order -> 1 / 0 per template: one entry each, or entries 2p and 2p + 1; a template fails iff any
    of its records does"""
    rec = [t is not None and fails(*counts_of(t), params) for t in tallies]
    if not paired:
        return [int(f) for f in rec]
    assert len(rec) % 2 == 0
    return [int(rec[i] or rec[i + 1]) for i in range(0, len(rec), 2)]


def templates(seqs, records, paired, params=DEFAULTS):
    check_params(params)
    for j, rec in enumerate(records):
        spec.check(rec, seqs, j)
    return verdicts([tally(r, seqs, params.min_phred) for r in records], paired, params)


def totals_of(records, tallies):
    """[strand 0 OT, 1 OB][context][0 unmethylated, 1 methylated]: the calls of all examined records, failed or not"""
    out = [[[0, 0] for _ in range(3)] for _ in range(2)]
    for rec, t in zip(records, tallies):
        if t is not None:
            s = int(spec.is_ob(spec.fields(rec)[3]))
            for ctx in range(3):
                for m in range(2):
                    out[s][ctx][m] += t[ctx][m]
    return out


def totals(seqs, records, min_phred=0):
    return totals_of(records, [tally(r, seqs, min_phred) for r in records])


def mark(records, paired, failed):
    """the records with flag 0x200 set in EVERY record of a failed template, the mate that is unmapped or was not examined too"""
    out = []
    for i, rec in enumerate(records):
        if rec and failed[i >> 1 if paired else i]:
            b = bytearray(rec)
            b[19] |= QC_FAIL >> 8
            rec = bytes(b)
        out.append(rec)
    return out


def report_text(tot, n_templates, n_failed) -> bytes:
    """the --conversion-report file: the totals by strand and context with methyl_spec.pct (rounded half up; NA without calls), the
    non-CpG conversion rate = the unmethylated CHG and CHH calls of all CHG and CHH calls, in hundredths of a percent rounded half up
    (NA without calls), the templates of the run and those that failed"""
    out = ["#strand\tcontext\tmethylated\tunmethylated\tpercent\n"]
    nm = nu = 0
    for s in range(2):
        for ctx in range(3):
            u, m = tot[s][ctx]
            if ctx != spec.CPG:
                nm += m; nu += u
            out.append("%s\t%s\t%d\t%d\t%s\n" % (("OT", "OB")[s], spec.CONTEXT_NAMES[ctx], m, u, spec.pct(m, u) if m + u else "NA"))
    if nm + nu:
        bp = (20000 * nu + nm + nu) // (2 * (nm + nu))
        out.append("non-CpG conversion rate\t%d\t%d\t%d.%02d\n" % (nu, nm + nu, bp // 100, bp % 100))
    else:
        out.append("non-CpG conversion rate\t0\t0\tNA\n")
    out.append("templates\t%d\tfailed\t%d\n" % (n_templates, n_failed))
    return "".join(out).encode()
