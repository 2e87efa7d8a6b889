"""The opposite-strand variant filter, merged contexts and the minimum depth of the methylation calls (bmbs_bam_methyl_opposite /
bmbs_bam_sort_methyl_opposite / bmbs_methyl_opposite / bmbs_methyl_drop_variants, `bmbs_search --methyl ... --methyl-min-opposite-depth
--methyl-max-variant-frac --methyl-merge-context --methyl-min-depth`; the rule is in include/bmbs.h), restated as plain Python on top of
methyl_spec.py and mbias_spec.py.  MethylDackel's --minOppositeDepth / --maxVariantFrac, --mergeContext and --minDepth are the model.
Everything is exact integer arithmetic.

A C->T polymorphism of the sample looks like an unmethylated cytosine on the reads of the cytosine's own bisulfite strand; the reads of
the OTHER strand show the position unconverted.  So every record that counts is walked a second time: an OB record where the genome has
a forward C of a selected context, an OT record where it has a forward G -- the positions the other strand's records are called at.  A
read base that passes the filters a call passes (quality, mate-overlap clip, trim) is a MATCH when its BAM code is the genome's base
there (C = 2, G = 4), a VARIANT when it is one of the other three of {1, 2, 4, 8}, and nothing otherwise.  An entry is
(ref, pos, variant, match, kind): the layout of a site, `meth` holding the variants and `unmeth` the matches."""
import mbias_spec
import methyl_spec as spec

PLAIN_CODES = (1, 2, 4, 8)                              # A C G T
PPM = 1_000_000


def observations(rec, seqs, clip=0, min_phred=5):
    """(ref, pos, variant, (context, strand), cycle) of every opposite-strand observation of a record that counts, every context, no trim"""
    ref, pos, _mapq, flag, cigar, bases, quals = spec.fields(rec)
    ob = spec.is_ob(flag)
    lo, hi = pos + (clip >> 16), pos + (clip >> 16) + (clip & 0xffff)
    seq = seqs[ref]
    letter, code = (spec.C, spec.SEQ_C) if ob else (spec.G, spec.SEQ_G)
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
                if seq[p] != letter:
                    continue
                ctx = spec.context(seq, p)
                if ctx is None:
                    continue
                if bases[ri] == code:
                    yield ref, p, 0, ctx, mbias_spec.cycle_of(ri, len(bases), flag)
                elif bases[ri] in PLAIN_CODES:
                    yield ref, p, 1, ctx, mbias_spec.cycle_of(ri, len(bases), flag)
            r += l; i += l
        elif op in (1, 4):
            i += l
        elif op in (2, 3):
            r += l


def walk(seqs, records, clip=None, min_mapq=10, min_phred=5):
    """[(record index, mate, l_seq, ref, pos, variant, context, strand, cycle)] of every observation of every record that counts: the
    layout of mbias_spec.walk, so that mbias_spec.sites_of adds them up"""
    for j, rec in enumerate(records):
        spec.check(rec, seqs, j)
    out = []
    for j, rec in enumerate(records):
        if spec.skip_reason(rec, min_mapq):
            continue
        _r, _p, _q, flag, _c, bases, _ql = spec.fields(rec)
        for ref, p, v, (ctx, strand), cyc in observations(rec, seqs, clip[j] if clip is not None else 0, min_phred):
            out.append((j, mbias_spec.mate_of(flag), len(bases), ref, p, v, ctx, strand, cyc))
    return out


def entries_of(walked, contexts=1, ignore_5p=(0, 0), ignore_3p=(0, 0)):
    """[(ref, pos, variant, match, kind)] ordered by (ref, pos): the observations of the selected contexts that the trim keeps"""
    return mbias_spec.sites_of(walked, contexts, ignore_5p, ignore_3p)


def entries(seqs, records, clip=None, contexts=1, min_mapq=10, min_phred=5, ignore_5p=(0, 0), ignore_3p=(0, 0)):
    return entries_of(walk(seqs, records, clip, min_mapq, min_phred), contexts, ignore_5p, ignore_3p)


def is_variant(entry, min_opposite_depth, max_variant_ppm):
    _ref, _pos, variant, match, _kind = entry
    depth = variant + match
    return depth >= min_opposite_depth and variant * PPM > max_variant_ppm * depth


def drop_variants(sites, opp, min_opposite_depth, max_variant_ppm):
    """the sites without those the opposite strand shows to be variants; a site without an entry stays, an entry without a site does
    nothing"""
    if min_opposite_depth < 1 or not 0 <= max_variant_ppm <= PPM:
        raise ValueError("min_opposite_depth >= 1, max_variant_ppm 0..1000000")
    for lst in (sites, opp):
        if any((a[0], a[1]) >= (b[0], b[1]) for a, b in zip(lst, lst[1:])):
            raise ValueError("a list out of order")
    bad = {(e[0], e[1]) for e in opp if is_variant(e, min_opposite_depth, max_variant_ppm)}
    return [s for s in sites if (s[0], s[1]) not in bad]


def interval(site):
    """[beg, end) of the line of a site with merged contexts: the dinucleotide of a CpG, the trinucleotide of a CHG, the base of a CHH"""
    _ref, p, _m, _u, kind = site
    ctx, strand = kind & 3, kind >> 2
    if ctx == spec.CHH:
        return p, p + 1
    w = 2 if ctx == spec.CPG else 3
    return (p - w + 1, p + 1) if strand else (p, p + w)


def merge_context(sites, merge=True):
    """[(ref, beg, end, meth, unmeth, context)] ordered by (context, ref, beg): the sites of one context with the same interval added"""
    acc = {}
    for s in sites:
        beg, end = interval(s) if merge else (s[1], s[1] + 1)
        a = acc.setdefault((s[4] & 3, s[0], beg, end), [0, 0])
        a[0] += s[2]; a[1] += s[3]
    return [(ref, beg, end, a[0], a[1], ctx) for (ctx, ref, beg, end), a in sorted(acc.items())]


def lines(sites, merge=False, min_depth=1):
    return [l for l in merge_context(sites, merge) if l[3] + l[4] >= min_depth]


def bedgraph(prefix, ctx, chrom_names, sites, merge=False, min_depth=1):
    """the file of one context from the sites that are left (after the non-ACGT drop and the filter)"""
    out = ['track type="bedGraph" description="%s %s methylation levels"\n' % (prefix, spec.CONTEXT_NAMES[ctx])]
    for ref, beg, end, m, u, c in lines(sites, merge, min_depth):
        if c == ctx:
            out.append("%s\t%d\t%d\t%d\t%d\t%d\n" % (chrom_names[ref], beg, end, spec.pct(m, u), m, u))
    return "".join(out).encode()


def parse_frac(text):
    """a plain decimal in [0, 1] -> parts per million, without floating point: digits, or digits '.' digits with the first digits
    optional; at most 6 digits behind the point, no sign, no exponent"""
    whole, point, frac = text.partition(".")
    if not (whole + frac).isascii() or not (whole + frac).isdigit() or len(frac) > 6 or (point and not frac):
        raise ValueError("not a fraction: %r" % text)
    ppm = int(whole or "0") * PPM + int((frac + "000000")[:6])
    if ppm > PPM:
        raise ValueError("above 1: %r" % text)
    return ppm
