"""tests/variant_spec.py on hand-worked records, and bmbs_methyl_drop_variants (host only: no GPU) against it."""
import ctypes

import numpy as np
import pytest

import methyl_spec as spec
import variant_spec as vs

#          0123456789012345
GENOME = "ATCGATCAGTTCCGAA"
# C 2 CpG, G 3 CpG, C 6 CHG (CAG), G 8 CHG, C 11 CHG (CCG), C 12 CpG, G 13 CpG (in CCG the G is a CpG cytosine)
SEQS = [bytes("ACGT".index(c) for c in GENOME)]
Q = [30] * 16


def _read(changes=None, text=GENOME):
    b = list(text)
    for p, c in (changes or {}).items():
        b[p] = c
    return "".join(b)


def _rec(flag, seq, quals=None, cigar=(("M", 16),), pos=0, mapq=30):
    return spec.make_record(0, pos, flag, list(cigar), seq, quals or [30] * len(seq), mapq=mapq)


def test_the_contexts_of_the_hand_genome():
    assert [(p, spec.context(SEQS[0], p)) for p in range(16) if spec.context(SEQS[0], p)] == \
        [(2, (0, 0)), (3, (0, 1)), (6, (1, 0)), (8, (1, 1)), (11, (1, 0)), (12, (0, 0)), (13, (0, 1))]


def test_an_ob_read_over_forward_c_showing_c_t_and_n():
    rec = _rec(16, _read({6: "T", 11: "N"}))
    # C at 2 and 12: matches; T at 6: a variant; N at 11: nothing; the G positions are not looked at on an OB read
    assert vs.entries(SEQS, [rec], contexts=7) == [(0, 2, 0, 1, 0), (0, 6, 1, 0, 1), (0, 12, 0, 1, 0)]
    assert vs.entries(SEQS, [rec], contexts=1) == [(0, 2, 0, 1, 0), (0, 12, 0, 1, 0)]
    assert vs.entries(SEQS, [rec], contexts=4) == []
    # '=' and an ambiguity code are nothing either; A and G are variants as T is
    rec = _rec(16, _read({2: "=", 6: "A", 11: "Y", 12: "G"}))
    assert vs.entries(SEQS, [rec], contexts=7) == [(0, 6, 1, 0, 1), (0, 12, 1, 0, 0)]


def test_an_ot_read_over_forward_g():
    rec = _rec(0, _read({8: "A", 2: "T", 6: "T"}))                       # (its own conversions at 2 and 6 are not looked at)
    assert vs.entries(SEQS, [rec], contexts=7) == [(0, 3, 0, 1, 4), (0, 8, 1, 0, 5), (0, 13, 0, 1, 4)]
    # paired: read 2 forward is OB, read 1 forward OT
    assert [e[1] for e in vs.entries(SEQS, [_rec(0x83, GENOME)], contexts=7)] == [2, 6, 11, 12]
    assert [e[1] for e in vs.entries(SEQS, [_rec(0x43, GENOME)], contexts=7)] == [3, 8, 13]
    # two reads add up per position
    both = [_rec(0, _read({8: "A"})), _rec(0, _read({3: "C"}))]
    assert vs.entries(SEQS, both, contexts=7) == [(0, 3, 1, 1, 4), (0, 8, 1, 1, 5), (0, 13, 0, 2, 4)]


def test_the_filters_of_a_call_apply():
    full = [2, 6, 11, 12]
    q = list(Q); q[6] = 4; q[11] = 0xff; q[12] = 5
    assert [e[1] for e in vs.entries(SEQS, [_rec(16, GENOME, q)], contexts=7)] == [2, 12]           # below the bound, 0xff counts as 0
    clip = [5 << 16 | 7]                                                                            # positions 5 .. 11
    assert [e[1] for e in vs.entries(SEQS, [_rec(16, GENOME)], clip, contexts=7)] == [2, 12]
    # a reverse record: cycle = 15 - ri.  ignore_5p 4 takes cycles 0..3 = positions 12..15; ignore_3p 3 takes positions 0..2
    assert [e[1] for e in vs.entries(SEQS, [_rec(16, GENOME)], contexts=7, ignore_5p=(4, 0), ignore_3p=(3, 0))] == [6, 11]
    assert [e[1] for e in vs.entries(SEQS, [_rec(16, GENOME)], contexts=7, ignore_5p=(0, 4), ignore_3p=(0, 3))] == full     # (mate 0: read 2's trim is not its)
    # read 2 forward (OB): cycle = ri
    assert [e[1] for e in vs.entries(SEQS, [_rec(0x83, GENOME)], contexts=7, ignore_5p=(0, 3), ignore_3p=(9, 4))] == [6, 11]


def test_a_record_that_does_not_count_gives_nothing():
    for rec in (_rec(16 | 0x400, GENOME), _rec(16 | 0x100, GENOME), _rec(16, GENOME, mapq=9), _rec(0x11, GENOME), _rec(4 | 16, GENOME), b""):
        assert vs.entries(SEQS, [rec], contexts=7) == []
    assert len(vs.entries(SEQS, [_rec(16, GENOME, mapq=10)], contexts=7)) == 4


def test_an_insertion_and_a_deletion_in_front_of_the_position():
    # 4M 2I 3M 1D 7M: reference 0-3 = read 0-3, read 4-5 inserted, reference 4-6 = read 6-8, reference 7 deleted, reference 8-14 = read 9-15
    seq = GENOME[0:4] + "CC" + GENOME[4:7] + GENOME[8:15]
    assert len(seq) == 16
    cigar = (("M", 4), ("I", 2), ("M", 3), ("D", 1), ("M", 7))
    assert vs.entries(SEQS, [_rec(16, seq, cigar=cigar)], contexts=7) == [(0, 2, 0, 1, 0), (0, 6, 0, 1, 1), (0, 11, 0, 1, 1), (0, 12, 0, 1, 0)]
    seq2 = list(seq); seq2[8] = "T"; seq2[12] = "T"; seq2[4] = "T"                                 # read 8 = reference 6, read 12 = reference 11
    assert vs.entries(SEQS, [_rec(16, "".join(seq2), cigar=cigar)], contexts=7) == [(0, 2, 0, 1, 0), (0, 6, 1, 0, 1), (0, 11, 1, 0, 1), (0, 12, 0, 1, 0)]
    # the cycles of a reverse record count the inserted bases: ignore_5p 3 takes read 13-15 = reference 12-14
    assert [e[1] for e in vs.entries(SEQS, [_rec(16, seq, cigar=cigar)], contexts=7, ignore_5p=(3, 0))] == [2, 6, 11]
    # a position inside a deletion has no read base
    cigar = (("M", 6), ("D", 1), ("M", 9))
    assert [e[1] for e in vs.entries(SEQS, [_rec(16, GENOME[:6] + GENOME[7:], [30] * 15, cigar=cigar)], contexts=7)] == [2, 11, 12]


# ---- bmbs_methyl_drop_variants --------------------------------------------------------------------------------------------------------------
def _array(lst):
    from bitmapperbs_amd import capi
    a = np.zeros(len(lst), dtype=capi.METHYL_SITE_DTYPE)
    for i, (ref, pos, m, u, kind) in enumerate(lst):
        a[i] = (ref, pos, m, u, kind, 0)
    return a


def _tuples(a):
    return [(int(r["ref"]), int(r["pos"]), int(r["meth"]), int(r["unmeth"]), int(r["kind"])) for r in a]


def _drop(sites, opp, depth, ppm):
    from bitmapperbs_amd import mapper
    return _tuples(mapper.drop_variants(_array(sites), _array(opp), depth, ppm))


def _random_lists(rng, n, n_opp):
    def ordered(k):
        keys = sorted({(int(r), int(p)) for r, p in zip(rng.integers(0, 3, k), rng.integers(0, 400, k))})
        return keys
    sites = [(r, p, int(rng.integers(0, 30)), int(rng.integers(1, 30)), int(rng.integers(0, 3)) | int(rng.integers(0, 2)) << 2) for r, p in ordered(n)]
    opp = [(r, p, int(rng.integers(0, 12)), int(rng.integers(0, 12)), 0) for r, p in ordered(n_opp)]
    return sites, [e for e in opp if e[2] + e[3]]


def test_drop_variants_equals_the_spec_on_random_ordered_lists():
    rng = np.random.default_rng(41)
    seen_drop = seen_keep = lonely_site = lonely_entry = 0
    for _ in range(60):
        sites, opp = _random_lists(rng, int(rng.integers(0, 500)), int(rng.integers(0, 500)))
        for depth, ppm in ((1, 0), (3, 500_000), (5, 200_000), (1, 1_000_000), (12, 333_333), (65535, 0)):
            want = vs.drop_variants(sites, opp, depth, ppm)
            assert _drop(sites, opp, depth, ppm) == want
            seen_drop += len(sites) - len(want); seen_keep += len(want)
        keys_s, keys_o = {s[:2] for s in sites}, {e[:2] for e in opp}
        lonely_site += len(keys_s - keys_o); lonely_entry += len(keys_o - keys_s)
    assert seen_drop > 1000 and seen_keep > 1000 and lonely_site > 100 and lonely_entry > 100


def test_drop_variants_at_the_bounds():
    site = [(0, 7, 1, 9, 0)]
    # depth = min - 1 is not looked at, depth = min is
    assert _drop(site, [(0, 7, 4, 0, 0)], 5, 0) == site and _drop(site, [(0, 7, 5, 0, 0)], 5, 0) == []
    assert _drop(site, [(0, 7, 2, 2, 0)], 5, 0) == site and _drop(site, [(0, 7, 2, 3, 0)], 5, 0) == []
    # variant * 10^6 == ppm * depth exactly: kept; one variant more: dropped
    assert _drop(site, [(0, 7, 1, 3, 0)], 1, 250_000) == site and _drop(site, [(0, 7, 2, 3, 0)], 1, 250_000) == []
    assert _drop(site, [(0, 7, 1, 2, 0)], 1, 333_333) == [] and _drop(site, [(0, 7, 1, 2, 0)], 1, 333_334) == site
    # ppm 0: any variant drops, none keeps; ppm 1 000 000: nothing is ever dropped
    assert _drop(site, [(0, 7, 0, 9, 0)], 1, 0) == site and _drop(site, [(0, 7, 1, 900, 0)], 1, 0) == []
    assert _drop(site, [(0, 7, 9, 0, 0)], 1, 1_000_000) == site
    # counts of 2^32 - 1: the product does not wrap in 64 bits
    top = 2 ** 32 - 1
    assert _drop(site, [(0, 7, top, top, 0)], 1, 500_000) == site and _drop(site, [(0, 7, top, top - 1, 0)], 1, 500_000) == []
    assert _drop(site, [(0, 7, top, top, 0)], 1, 499_999) == [] and _drop(site, [(0, 7, top, 0, 0)], 65535, 999_999) == []
    assert _drop(site, [(0, 7, 1, top, 0)], 1, 0) == [] and _drop(site, [(0, 7, 0, top, 0)], 1, 0) == site
    for case in ((site, [(0, 7, top, top, 0)], 1, 500_000), (site, [(0, 7, top, top - 1, 0)], 1, 500_000), (site, [(0, 7, top, 0, 0)], 65535, 999_999)):
        assert _drop(*case) == vs.drop_variants(*case)
    # the same position of another sequence is another position; entries without sites, sites without entries, empty lists
    sites = [(0, 7, 1, 1, 0), (1, 7, 2, 2, 0), (1, 9, 3, 3, 4)]
    assert _drop(sites, [(0, 9, 5, 0, 0), (1, 7, 5, 0, 0), (2, 7, 5, 0, 0)], 1, 0) == [sites[0], sites[2]]
    assert _drop(sites, [], 1, 0) == sites and _drop([], [(0, 7, 5, 0, 0)], 1, 0) == [] and _drop([], [], 1, 0) == []
    # kind and pad of what is kept stay
    assert _drop(sites, [(1, 9, 0, 5, 0)], 1, 0) == sites


def test_drop_variants_refusals():
    from bitmapperbs_amd import capi
    lib = capi.lib()
    site, opp = _array([(0, 7, 1, 9, 0), (0, 9, 1, 9, 0)]), _array([(0, 7, 4, 0, 0), (1, 2, 4, 0, 0)])
    kept = ctypes.c_int64(-5)

    def call(s, o, depth, ppm):
        return lib.bmbs_methyl_drop_variants(capi.ptr(s), s.size, capi.ptr(o), o.size, depth, ppm, ctypes.byref(kept))
    assert call(site.copy(), opp, 1, 0) == 0 and kept.value == 1
    for depth, ppm in ((0, 0), (-1, 0), (1, -1), (1, 1_000_001)):
        assert call(site.copy(), opp, depth, ppm) == -22 and kept.value == 0
        with pytest.raises(ValueError):
            vs.drop_variants(_tuples(site), _tuples(opp), depth, ppm)
    for bad_s, bad_o in ((site[::-1].copy(), opp), (site, opp[::-1].copy()), (_array([(0, 7, 1, 1, 0)] * 2), opp), (site, _array([(0, 7, 1, 1, 0)] * 2))):
        before = bad_s.copy()
        assert call(bad_s, bad_o, 1, 0) == -22 and (bad_s == before).all()
        with pytest.raises(ValueError):
            vs.drop_variants(_tuples(bad_s), _tuples(bad_o), 1, 0)
    from bitmapperbs_amd import mapper
    with pytest.raises(ValueError):
        mapper.drop_variants(site, opp, 0, 0)
    # the arguments of the Python call stay as they are
    s2 = site.copy()
    assert len(mapper.drop_variants(s2, opp, 1, 0)) == 1 and (s2 == site).all()


# ---- merged contexts ---------------------------------------------------------------------------------------------------------------------------
def test_merge_context():
    # CG at 2-3: both strands, one line [2, 4)
    assert vs.merge_context([(0, 2, 3, 1, 0), (0, 3, 2, 2, 4)]) == [(0, 2, 4, 5, 3, 0)]
    # either strand alone keeps the dinucleotide's interval
    assert vs.merge_context([(0, 2, 3, 1, 0)]) == [(0, 2, 4, 3, 1, 0)] and vs.merge_context([(0, 3, 2, 2, 4)]) == [(0, 2, 4, 2, 2, 0)]
    # CAG at 6-8: the trinucleotide [6, 9)
    assert vs.merge_context([(0, 6, 1, 0, 1), (0, 8, 0, 4, 5)]) == [(0, 6, 9, 1, 4, 1)]
    assert vs.merge_context([(0, 8, 0, 4, 5)]) == [(0, 6, 9, 0, 4, 1)]
    # CCG at 11-13: C 11 is CHG [11, 14) and stands alone; C 12 and G 13 are the CpG [12, 14)
    got = vs.merge_context([(0, 11, 1, 1, 1), (0, 12, 2, 2, 0), (0, 13, 3, 3, 4)])
    assert got == [(0, 12, 14, 5, 5, 0), (0, 11, 14, 1, 1, 1)]
    # CHH is never merged; without merging every site is its base
    assert vs.merge_context([(0, 20, 1, 2, 2), (0, 22, 3, 4, 6)]) == [(0, 20, 21, 1, 2, 2), (0, 22, 23, 3, 4, 2)]
    assert vs.merge_context([(0, 2, 3, 1, 0), (0, 3, 2, 2, 4)], merge=False) == [(0, 2, 3, 3, 1, 0), (0, 3, 4, 2, 2, 0)]
    # the same interval of another sequence is another line
    assert vs.merge_context([(0, 2, 3, 1, 0), (1, 3, 2, 2, 4)]) == [(0, 2, 4, 3, 1, 0), (1, 2, 4, 2, 2, 0)]
    # a sequence's first and last bases: "CG...CG" of length n -- C at 0 / G at 1, C at n - 2 / G at n - 1; CTG at the very end
    n = 50
    assert vs.merge_context([(0, 0, 1, 0, 0), (0, 1, 0, 1, 4), (0, n - 2, 1, 1, 0), (0, n - 1, 1, 1, 4)]) == [(0, 0, 2, 1, 1, 0), (0, n - 2, n, 2, 2, 0)]
    assert vs.merge_context([(0, n - 1, 1, 1, 5)]) == [(0, n - 3, n, 1, 1, 1)] and vs.merge_context([(0, 0, 1, 1, 1)]) == [(0, 0, 3, 1, 1, 1)]
    # a partner dropped by the filter: the other strand's site is written alone, with the interval
    sites = [(0, 2, 0, 6, 0), (0, 3, 5, 1, 4)]
    left = vs.drop_variants(sites, [(0, 2, 4, 1, 0)], 3, 500_000)
    assert left == [sites[1]] and vs.merge_context(left) == [(0, 2, 4, 5, 1, 0)]
    # the depth bound looks at the lines as written: 2 + 2 passes 4 merged, neither passes alone
    two = [(0, 2, 1, 1, 0), (0, 3, 2, 0, 4)]
    assert vs.lines(two, merge=True, min_depth=4) == [(0, 2, 4, 3, 1, 0)] and vs.lines(two, merge=False, min_depth=4) == [] and len(vs.lines(two, min_depth=2)) == 2
    text = vs.bedgraph("p", 0, ["chrA"], two, merge=True, min_depth=4).decode().split("\n")
    assert text[1:] == ["chrA\t2\t4\t75\t3\t1", ""] and text[0].startswith("track ")
    assert vs.bedgraph("p", 0, ["chrA"], two) == spec.bedgraph("p", 0, ["chrA"], two)               # no option: the file as ever


def test_on_the_hand_genome_the_intervals_hold_the_context():
    """every site's interval spells CG or C.G on the forward strand"""
    for p in range(16):
        c = spec.context(SEQS[0], p)
        if c and c[0] != spec.CHH:
            beg, end = vs.interval((0, p, 1, 1, c[0] | c[1] << 2))
            word = GENOME[beg:end]
            assert (word == "CG") if c[0] == spec.CPG else (len(word) == 3 and word[0] == "C" and word[2] == "G" and word[1] != "G"), (p, word)


# ---- the fraction ------------------------------------------------------------------------------------------------------------------------------
def test_parse_frac():
    assert [vs.parse_frac(t) for t in ("0", "1", "1.0", "0.000001", ".5", "0.5", "0.25", "1.000000", "0.333333", "00.1")] == \
        [0, 1_000_000, 1_000_000, 1, 500_000, 500_000, 250_000, 1_000_000, 333_333, 100_000]
    for bad in ("1.0000001", "1.1", "-0", "1e-3", "", ".", "1.", "+1", " 1", "0x1", "2", "0,5", "1.000001", "١"):
        with pytest.raises(ValueError):
            vs.parse_frac(bad)
