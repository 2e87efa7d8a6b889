"""Reads and pairs at and across chromosome ends (seeded, numpy only): the inputs of tests/test_chrom_ends.py and of the `ends_*`
goldens (tests/golden/make_golden.py --only ends).

Every record the mapper emits passes the off-end check of output_sam_end_to_end (Schema.cpp:11974-11986: `map_location + end_site -
start_site > chrome_length` rejects) or, in a pair, `site + matched > chrome_length + 1`.  bitmapperbs_amd.synth draws every read at
least 8 bases away from both ends of its chromosome, so nothing drawn there reaches either comparison.  Here every read is placed
relative to an end:

  genome   chr1 chr2 (30 kb) | ctg1 .. ctg20 (400 bases) | s1 .. s4 (80 bases, shorter than a read) | chr3 chr4 (30 kb); chr4 ends at
           the forward/reverse seam of the doubled text
  plants   (i)   the 100 bases across the chr1|chr2 join copied into chr3: two exact hits, one of them across an end
           (ii)  the ctg7|ctg8 join made a copy of the ctg3|ctg4 join (60 + 60 bases): two exact hits, BOTH across an end
           (iii) a 100-base element inside chr4 and flush against chr2's last base: two exact hits, one touching an end
           (i) and (ii) are written in A/T only, so a read of them has no C and takes the exact-ambiguous exit
           (output_ambiguous_exact_map, Schema.cpp:24072-24121) on both strands.

Plant (ii) is NOT part of the golden inputs (genome(plant_ii=False)).  With --ambiguous_out such a read walks the loop of
output_ambiguous_exact_map through all its hits, every placement is rejected, and the function then runs off its end: it is declared
`int`, has `return 1` inside the loop and no return after it (Schema.cpp:24115-24121).  That is undefined behaviour.  g++ -O3 drops
the loop's `i < number_of_hits` exit (leaving through it would reach the missing return), so the compiled reference goes on to
SA rows beyond the read's interval and prints the read at whichever neighbouring suffix places inside a chromosome; the same
sources at -O0 leave the loop and print nothing.  What the read's record should be is therefore not a function of index and read
that could be pinned: the oracle and the device leave the loop after the read's own hits and count the read as unmapped
(status 3, path 4), and the oracle-parity tests keep plant (ii) in (genome(plant_ii=True), se_reads(..., plant_ii=True)).
"""
import numpy as np

L = 100
INSERT = 250
OVERS = tuple(range(-2, 12)) + (30, 50, 70, 90, 98, 99, 100, 101)      # bases of the read beyond its chromosome's last base
STARTS = (0, 1, 2)
# fragment end relative to the chromosome's last base: wholly inside .. mate 2 crosses .. mates on two chromosomes .. mate 1 crosses
# .. wholly beyond
PE_SHIFTS = (-2, -1, 0, 1, 2, 3, 10, 25, 50, 75, 98, 99, 100, 101, 102, 110, 125, 140, 149, 150, 151, 152, 160, 175, 200, 225, 248, 249,
             250, 251)
PE_MIN, PE_MAX = 200, 300                                                # the --min/--max run; inserts at each bound and each bound +- 1
BOUND_INSERTS = (PE_MIN - 1, PE_MIN, PE_MIN + 1, PE_MAX - 1, PE_MAX, PE_MAX + 1)
SEAM_KEEP = 25          # of a read across the forward/reverse seam at least a quarter stays on the forward side (see seam_state)

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_AT = np.frombuffer(b"AT", dtype=np.uint8)
_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    _COMP[_a] = _b
# binned base qualities, as current sequencers write them (Phred + 33)
_QBINS = (np.array([2, 11, 20, 25, 30, 35, 38, 40]) + 33).astype(np.uint8)

SE_DTYPE = np.dtype([("kind", "U8"), ("chrom", "<i4"), ("minus", "?"), ("over", "<i4"), ("form", "U6"), ("near", "?")])
PE_DTYPE = np.dtype([("kind", "U8"), ("chrom", "<i4"), ("minus", "?"), ("shift", "<i4"), ("insert", "<i4"), ("form", "U6")])


def revcomp(a):
    return _COMP[a][::-1]


def genome(plant_ii=False, n_ctg=20, seed=4242):
    """-> (names, chroms).  n_ctg > 20 pads the 400-base contigs out (more than 1024 sequences: the device reads its chromosome
    table from global memory instead of the LDS copy); the plants stay where they are."""
    rng = np.random.default_rng(seed)
    big = [_ACGT[rng.integers(0, 4, n)] for n in (30011, 29987, 30029, 30005)]
    ctg = [_ACGT[rng.integers(0, 4, 400)] for _ in range(20)]
    short = [_ACGT[rng.integers(0, 4, 80)] for _ in range(4)]
    p1 = _AT[rng.integers(0, 2, 100)]; p2 = _AT[rng.integers(0, 2, 120)]; p3 = _ACGT[rng.integers(0, 4, 100)]
    if n_ctg > 20:
        xr = np.random.default_rng(seed + 1)           # a stream of its own: the sequences above stay what they are
        ctg += [_ACGT[xr.integers(0, 4, 400)] for _ in range(n_ctg - 20)]
    names = ["chr1", "chr2"] + ["ctg%d" % (i + 1) for i in range(len(ctg))] + ["s%d" % (i + 1) for i in range(4)] + ["chr3", "chr4"]
    chroms = big[:2] + ctg + short + big[2:]
    # (i): across chr1|chr2 and inside chr3
    chroms[0][-50:] = p1[:50]; chroms[1][:50] = p1[50:]; chroms[-2][10000:10100] = p1
    # (iii): inside chr4 and flush against chr2's last base
    chroms[-1][5000:5100] = p3; chroms[1][-100:] = p3
    # ... and the base behind the inside copy cannot be read as the one behind chr2's end (ctg1's first) on either strand, so the
    # read one base across chr2's end has ONE best hit, the one across the end
    chroms[-1][5100] = _COMP[chroms[2][0]]
    if plant_ii:
        for a in (2 + 2, 2 + 6):                       # ctg3|ctg4 and ctg7|ctg8
            chroms[a][-60:] = p2[:60]; chroms[a + 1][:60] = p2[60:]
    return names, chroms


def write_fasta(path, names, chroms, width=60):
    with open(path, "wb") as f:
        for nm, s in zip(names, chroms):
            f.write(b">" + nm.encode() + b"\n")
            for a in range(0, s.size, width):
                f.write(s[a:a + width].tobytes() + b"\n")


class _Text:
    """the doubled text the index is built over: the chromosomes back to back, then the reverse complement of all of it"""
    def __init__(self, chroms):
        self.cat = np.concatenate(chroms)
        self.G = self.cat.size
        self.dbl = np.concatenate([self.cat, revcomp(self.cat)])
        lens = np.array([c.size for c in chroms], dtype=np.int64)
        self.end = np.cumsum(lens); self.start = self.end - lens


def _convert(rng, r, conv=0.9):
    m = (r == ord("C")) & (rng.random(r.size) < conv)
    r = r.copy(); r[m] = ord("T")
    return r


def _mutated(rng, tmpl, n, form, near=None):
    """n read bases from the template (forward strand, n + 8 bases long).  form 'exact' | 'subs' (3 % substitutions, 1 % N) | 'indel'
    (one base of the template skipped or one base added, at read offset `near` +- 5 when given)"""
    r = tmpl[:n].copy()
    if form == "subs":
        m = rng.random(n) < 0.03
        r[m] = _ACGT[rng.integers(0, 4, int(m.sum()))]
        r[rng.random(n) < 0.01] = ord("N")
    elif form == "indel":
        p = int(rng.integers(5, n - 5)) if near is None else int(np.clip(near + rng.integers(-5, 6), 1, n - 2))
        if rng.random() < 0.5:
            r[p:] = tmpl[p + 1:n + 1]                                    # deletion: the read spans n + 1 template bases
        else:
            r[p + 1:] = tmpl[p:n - 1]; r[p] = _ACGT[rng.integers(0, 4)]  # insertion: n - 1 template bases
    return r


def _quals(rng, n):
    return _QBINS[rng.integers(0, _QBINS.size, n)]


def se_reads(chroms, seed=77, plant_ii=False, ends=None, forms=("exact", "subs", "indel")):
    """-> dict(seq[n, L], qual[n, L], names, meta[n] SE_DTYPE).  meta.kind: 'end' (over = bases beyond the last base of meta.chrom),
    'start' (over = offset of the read's first base in meta.chrom), 'plant1' / 'plant2' / 'plant3'.  ends: chromosome numbers to
    use (default all)."""
    rng = np.random.default_rng(seed)
    T = _Text(chroms)
    nc = len(chroms)
    seqs, quals, meta = [], [], []

    def add(kind, c, minus, over, form, s, near_at):
        near = near_at is not None and form == "indel" and rng.random() < 0.5
        t = T.dbl[s:s + L + 8]
        r = _mutated(rng, t, L, form, near_at if near else None)
        if minus:
            r = revcomp(r)
        seqs.append(_convert(rng, r)); quals.append(_quals(rng, L)); meta.append((kind, c, minus, over, form, near))

    for c in (range(nc) if ends is None else ends):
        E, S = int(T.end[c]), int(T.start[c])
        for minus in (False, True):
            for over in OVERS:
                s = E - L + over
                if s < 0 or (E == T.G and over > L - SEAM_KEEP):
                    continue
                for form in forms:
                    add("end", c, minus, over, form, s, L - over)
            for st in STARTS:
                if S + st + L + 8 > 2 * T.G:
                    continue
                for form in forms:
                    add("start", c, minus, st, form, S + st, 0)
    # the plants: exact reads, both strands, a few times each so that every exit sees them
    p1 = int(T.end[0]) - 50; p3 = int(T.start[nc - 1]) + 5000
    sites = [("plant1", 0, p1), ("plant1", nc - 2, int(T.start[nc - 2]) + 10000), ("plant3", nc - 1, p3), ("plant3", 1, int(T.end[1]) - L)]
    if plant_ii:
        sites += [("plant2", 4, int(T.end[4]) - 50), ("plant2", 8, int(T.end[8]) - 50), ("plant2", 4, int(T.end[4]) - 58), ("plant2", 8, int(T.end[8]) - 42)]
    for kind, c, s in sites:
        for minus in (False, True):
            add(kind, c, minus, 0, "exact", s, None)
    seq = np.array(seqs, dtype=np.uint8); qual = np.array(quals, dtype=np.uint8)
    names = [b"e%d" % i for i in range(seq.shape[0])]
    return dict(seq=seq, qual=qual, names=names, meta=np.array(meta, dtype=SE_DTYPE))


def pe_reads(chroms, seed=78, ends=None, forms=("exact", "subs")):
    """-> (mate1, mate2, meta[n] PE_DTYPE): mates as in the FASTQ files.  meta.kind 'sweep' (insert 250, the fragment's last base
    `shift` bases beyond the last base of meta.chrom) or 'bound' (inserts at --min/--max and one beside each, `shift` 0 = flush against
    the end, or inside the chromosome)"""
    rng = np.random.default_rng(seed)
    T = _Text(chroms)
    nc = len(chroms)
    if ends is None:
        ends = [c for c in range(nc) if chroms[c].size >= 400]
    s1, q1, s2, q2, meta = [], [], [], [], []

    def add(kind, c, minus, shift, ins, form, g):
        frag = T.dbl[g:g + ins]
        if minus:
            frag = revcomp(frag)
        frag = _convert(rng, frag)
        pad = np.full(8, ord("A"), dtype=np.uint8)
        a = _mutated(rng, np.concatenate([frag, pad]), L, form)
        b = _mutated(rng, np.concatenate([revcomp(frag), pad]), L, form)
        s1.append(a); s2.append(b); q1.append(_quals(rng, L)); q2.append(_quals(rng, L)); meta.append((kind, c, minus, shift, ins, form))

    for c in ends:
        E = int(T.end[c])
        for minus in (False, True):
            for d in PE_SHIFTS:
                g = E - INSERT + d
                if g < 0 or (E == T.G and d > L - SEAM_KEEP):
                    continue
                for form in forms:
                    add("sweep", c, minus, d, INSERT, form, g)
    for c in (0, 1, nc - 2):
        E = int(T.end[c])
        for ins in BOUND_INSERTS:
            for minus in (False, True):
                add("bound", c, minus, 0, ins, "exact", E - ins)
                add("bound", c, minus, -7000, ins, "exact", E - 7000 - ins)
    n = len(s1)
    base = [b"q%d" % i for i in range(n)]
    m1 = dict(seq=np.array(s1, dtype=np.uint8), qual=np.array(q1, dtype=np.uint8), names=[b + b"/1" for b in base])
    m2 = dict(seq=np.array(s2, dtype=np.uint8), qual=np.array(q2, dtype=np.uint8), names=[b + b"/2" for b in base])
    return m1, m2, np.array(meta, dtype=PE_DTYPE)


def write_fastq(path, reads):
    with open(path, "wb") as f:
        for nm, s, q in zip(reads["names"], reads["seq"], reads["qual"]):
            f.write(b"@" + nm + b"\n" + s.tobytes() + b"\n+\n" + q.tobytes() + b"\n")


def read_fastq_var(path, stride=L):
    """a FASTQ file whose records have their own lengths -> names, seq[n, stride], qual[n, stride] (zero-filled rows), lens[n]"""
    names, lens = [], []
    lines = open(path, "rb").read().split(b"\n")
    n = len(lines) // 4
    seq = np.zeros((n, stride), dtype=np.uint8); qual = np.zeros((n, stride), dtype=np.uint8)
    for i in range(n):
        s, q = lines[4 * i + 1], lines[4 * i + 3]
        names.append(lines[4 * i][1:]); lens.append(len(s))
        seq[i, :len(s)] = np.frombuffer(s, dtype=np.uint8); qual[i, :len(q)] = np.frombuffer(q, dtype=np.uint8)
    return names, seq, qual, np.array(lens, dtype=np.uint16)


def seam_state(recs, G):
    """reads whose record sits where the reference's chromosome lookup is undefined: the site lies on the forward side and the placed
    start (site + start_site) on the reverse side of the doubled text (`site < G <= site + start_site`): the reference's table walk
    finds no chromosome there and reads beyond the table, the oracle takes the last chromosome and the device none.  The sets hold
    no such read; tests/test_chrom_ends.py asserts it on the oracle's records."""
    site = recs["site"].astype(np.int64); st = recs["start_site"].astype(np.int64)
    return np.nonzero((recs["path"] != 0) & (recs["path"] != 4) & (site < G) & (site + st >= G))[0]
