"""The genome-wide cytosine report of `bmbs_search --methyl <prefix> --cytosine-report` (bmbs_methyl_report, include/bmbs.h), restated as
plain Python on top of methyl_spec: one line for every cytosine of a selected context in a window of one sequence, on both strands,
covered by a read or not.  Everything is exact: the decimal numbers have no sign and no padding, nothing is rounded, there is no
percent column.

`seqs`, `names`, `runs`, `sites` and `contexts` are methyl_spec's: seqs[ref] = the letters of sequence ref as the index holds them
(A0 C1 G2 T3), runs[ref] = its [beg, end) runs of bases the FASTA does not spell A, C, G or T (non_acgt_runs), sites =
[(ref, pos, meth, unmeth, kind)] ordered by (ref, pos), contexts = 1 CpG | 2 CHG | 4 CHH."""
import methyl_spec

REPORT_OMIT = 8                                         # BMBS_REPORT_OMIT, in a site's kind: the position gets no line at all
CONTEXT_COLUMN = ("CG", "CHG", "CHH")
LETTERS = "ACGT"


def in_run(runs_of_seq, p):
    return any(beg <= p < end for beg, end in runs_of_seq)


def touches(runs_of_seq, lo, hi):
    """the positions [lo, hi] touch a run (the rule of methyl_spec.drop_non_acgt)"""
    return any(beg <= hi and end > lo for beg, end in runs_of_seq)


def letter(seq, runs_of_seq, p, complement):
    """the letter printed for forward position p: N off the sequence's ends and inside a run"""
    if not 0 <= p < len(seq) or in_run(runs_of_seq, p):
        return "N"
    return LETTERS[3 - seq[p]] if complement else LETTERS[seq[p]]


def check(seqs, runs, sites, contexts, ref, beg, end):
    """what the call refuses (BMBS_EINVAL, naming the first offender)"""
    if not 0 <= ref < len(seqs):
        raise ValueError("ref %d is outside the index's sequences" % ref)
    seq = seqs[ref]
    if not 0 <= beg <= end <= len(seq):
        raise ValueError("the window [%d, %d) does not lie in the sequence" % (beg, end))
    if not 1 <= contexts <= 7:
        raise ValueError("contexts %d is outside 1..7" % contexts)
    rs = runs[ref] if runs else []
    last = 0
    for i, (b, e) in enumerate(rs):
        if b < last or e <= b:
            raise ValueError("run %d is out of order or overlaps its predecessor" % i)
        last = e
    prev = -1
    for i, (r, p, _m, _u, kind) in enumerate(sites):
        if r != ref:
            raise ValueError("site %d has another ref" % i)
        if not beg <= p < end:
            raise ValueError("site %d lies outside the window" % i)
        if p <= prev:
            raise ValueError("site %d does not sit behind its predecessor" % i)
        prev = p
        c = methyl_spec.context(seq, p)
        if kind & ~(7 | REPORT_OMIT) or c is None or (c[0] | c[1] << 2) != kind & 7:
            raise ValueError("the kind of site %d is not what the genome says at its position" % i)
        if not contexts >> c[0] & 1:
            raise ValueError("the context of site %d is not selected" % i)
        lo, hi = methyl_spec.window((r, p, 0, 0, kind & 7))
        if touches(rs, lo, hi):
            raise ValueError("the window of site %d touches a run" % i)


def report(seqs, names, runs, sites, contexts, ref, beg, end) -> bytes:
    """the lines of forward positions [beg, end) of sequence ref, ascending; `sites` = the sites of that window"""
    check(seqs, runs, sites, contexts, ref, beg, end)
    seq, rs = seqs[ref], (runs[ref] if runs else [])
    at = {p: (m, u, kind) for _r, p, m, u, kind in sites}
    out = []
    for p in range(beg, end):
        c = methyl_spec.context(seq, p)
        if c is None or not contexts >> c[0] & 1:
            continue
        ctx, strand = c
        lo, hi = methyl_spec.window((ref, p, 0, 0, ctx | strand << 2))
        if touches(rs, lo, hi):
            continue
        m, u, kind = at.get(p, (0, 0, 0))
        if kind & REPORT_OMIT:
            continue
        step = -1 if strand else 1
        tri = "".join(letter(seq, rs, p + step * k, bool(strand)) for k in range(3))
        out.append("%s\t%d\t%s\t%d\t%d\t%s\t%s\n" % (names[ref], p + 1, "-" if strand else "+", m, u, CONTEXT_COLUMN[ctx], tri))
    return "".join(out).encode()


def report_all(seqs, names, runs, sites, contexts) -> bytes:
    """the driver's file: every sequence whole, in index order"""
    return b"".join(report(seqs, names, runs, [s for s in sites if s[0] == ref], contexts, ref, 0, len(seqs[ref])) for ref in range(len(seqs)))
