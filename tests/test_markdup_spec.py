"""The duplicate-marking rule (tests/markdup_spec.py, include/bmbs.h) on hand-written records with the answer written out, and the
driver's refusal of --markdup without --sort.  No GPU."""
import os
import subprocess

from common import ROOT
from markdup_spec import DUP_NONE, NO_SIG, five_prime, make_record, mark, score, select, signature, signatures

Q30 = bytes([30])


def _se(pos, flag, cigar, quals, ref=0, name=b"r"):
    return make_record(ref, pos, flag, cigar, quals, name)


def _flags(recs):
    return [int.from_bytes(r[18:20], "little") for r in recs]


def test_two_forward_copies_the_lower_score_is_marked():
    a = _se(500, 0, [("M", 10)], Q30 * 10)                                  # 300
    b = _se(500, 0, [("M", 10)], bytes([40]) * 7 + bytes(3))                # 280
    assert [s[5] for s in signatures([a, b], False)] == [300, 280]
    assert select(signatures([a, b], False)) == [0, 1]
    assert select(signatures([b, a], False)) == [1, 0]
    out = mark([a, b], False)
    assert out[0] == a and _flags(out) == [0, 0x400]
    assert out[1][:19] == b[:19] and out[1][20:] == b[20:]                  # nothing else changes


def test_equal_scores_keep_the_earliest():
    a = _se(500, 0, [("M", 10)], Q30 * 10, name=b"first")
    b = _se(500, 0, [("M", 10)], Q30 * 10, name=b"second")
    c = _se(500, 0, [("M", 10)], Q30 * 10, name=b"third")
    assert select(signatures([a, b, c], False)) == [0, 1, 1]


def test_reverse_reads_with_equal_ends_are_duplicates_whatever_their_pos():
    a = _se(1000, 16, [("M", 100)], Q30 * 100)
    b = _se(1007, 16, [("M", 93)], Q30 * 93)                                # trimmed at its 3' end: pos moves, the 5' end does not
    assert five_prime(a)[:3] == (0, 1099, 1) and five_prime(b)[:3] == (0, 1099, 1)
    assert signature([a]) == (0, 1099, -1, -1, 1, 3000)
    assert select(signatures([a, b], False)) == [0, 1]
    assert select(signatures([b, a], False)) == [1, 0]                      # the higher score stays, not the first


def test_same_start_on_both_strands_is_no_duplicate():
    a = _se(1000, 0, [("M", 1)], Q30)                                       # forward: 5' end 1000
    b = _se(1000, 16, [("M", 1)], Q30)                                      # reverse, one base: 5' end 1000 too
    assert five_prime(a)[:2] == five_prime(b)[:2] == (0, 1000)
    assert select(signatures([a, b], False)) == [0, 0]


def _pair(p1, p2, l2=100, q=Q30, swap=False, ref2=0):
    """an FR pair: read 1 forward at p1 (100M), read 2 reverse at p2 (l2 M)"""
    f1, f2 = (0x80, 0x40) if swap else (0x40, 0x80)
    return [make_record(0, p1, 1 | 2 | 0x20 | f1, [("M", 100)], q * 100), make_record(ref2, p2, 1 | 2 | 0x10 | f2, [("M", l2)], q * l2)]


def test_pair_against_its_copy_with_a_trimmed_reverse_mate():
    a = _pair(1000, 1200)
    b = _pair(1000, 1207, l2=93)
    sa, sb = signatures(a + b, True)
    assert sa == (0, 1000, 0, 1299, 0 | 2 | 4 | 8, 6000) and sb == (0, 1000, 0, 1299, 14, 5790)
    assert select([sa, sb]) == [0, 1]
    assert _flags(mark(a + b, True)) == [0x63, 0x93, 0x463, 0x493]          # BOTH records of the loser
    assert _flags(mark(b + a, True)) == [0x463, 0x493, 0x63, 0x93]


def test_read_1_and_read_2_swapped_is_no_duplicate():
    a = _pair(1000, 1200)
    b = _pair(1000, 1200, swap=True)
    sa, sb = signatures(a + b, True)
    assert sa[:4] == sb[:4] and sa[4] == 14 and sb[4] == 10                 # bit 2 (lo is read 1) differs
    assert select([sa, sb]) == [0, 0]


def test_mates_on_two_references():
    a = _pair(5000, 100, ref2=2)                                            # read 2 on reference 2
    b = [a[1], a[0]]                                                        # the same pair, records in the other order
    c = _pair(5000, 100, ref2=1)
    sa, sb, sc = signatures(a + b + c, True)
    assert sa == (0, 5000, 2, 199, 14, 6000) and sb == sa and sc[:4] == (0, 5000, 1, 199)
    assert select([sa, sb, sc]) == [0, 1, 0]
    low = [make_record(3, 10, 0x41, [("M", 5)], Q30 * 5), make_record(1, 900, 0x81, [("M", 5)], Q30 * 5)]
    assert signature(low) == (1, 900, 3, 10, 0 | 0 | 0 | 8, 300)            # lo = the smaller reference, here read 2


def test_lo_hi_tie():
    # both 5' ends at (0, 1000): the forward mate is lo whichever record it is and whichever read it is
    fwd1 = make_record(0, 1000, 0x41, [("M", 10)], Q30 * 10); rev2 = make_record(0, 991, 0x91, [("M", 10)], Q30 * 10)
    assert five_prime(fwd1)[:2] == five_prime(rev2)[:2] == (0, 1000)
    assert signature([fwd1, rev2]) == signature([rev2, fwd1]) == (0, 1000, 0, 1000, 0 | 2 | 4 | 8, 600)
    fwd2 = make_record(0, 1000, 0x81, [("M", 10)], Q30 * 10); rev1 = make_record(0, 991, 0x51, [("M", 10)], Q30 * 10)
    assert signature([rev1, fwd2]) == (0, 1000, 0, 1000, 0 | 2 | 0 | 8, 600)
    # same strand too: read 1 is lo
    f1 = make_record(0, 1000, 0x41, [("M", 10)], Q30 * 10); f2 = make_record(0, 1000, 0x81, [("M", 10)], Q30 * 10)
    assert signature([f2, f1]) == signature([f1, f2]) == (0, 1000, 0, 1000, 0 | 0 | 4 | 8, 600)


def test_cigar_with_every_kind_of_operation():
    cig = [("H", 3), ("S", 2), ("M", 10), ("I", 4), ("D", 5), ("N", 100), ("=", 6), ("X", 1), ("S", 7), ("H", 11)]
    l_seq = 2 + 10 + 4 + 6 + 1 + 7
    f = _se(1000, 0, cig, Q30 * l_seq)
    r = _se(1000, 16, cig, Q30 * l_seq)
    assert five_prime(f)[:3] == (0, 1000 - 5, 0)
    assert five_prime(r)[:3] == (0, 1000 + (10 + 5 + 100 + 6 + 1) + 18 - 1, 1)
    assert five_prime(_se(2, 0, [("S", 5), ("M", 3)], Q30 * 8))[1] == -3    # a clip may reach in front of the reference
    # an unclipped read whose 5' end is the clipped one's: duplicates
    assert select(signatures([f, _se(995, 0, [("M", 30)], Q30 * 30)], False)) == [0, 1]            # (equal scores: 30 bases each)


def test_quality_threshold_and_missing_qualities():
    assert score(_se(1, 0, [("M", 4)], bytes([14, 15, 14, 15]))) == 30
    assert score(_se(1, 0, [("M", 3)], bytes([0xff, 0xff, 0xff]))) == 0
    assert score(_se(1, 0, [("M", 3)], bytes([93, 0xff, 16]))) == 109
    a = _se(7, 0, [("M", 2)], bytes([14, 14])); b = _se(7, 0, [("M", 2)], bytes([15, 0]))
    assert select(signatures([a, b], False)) == [1, 0]                      # 0 against 15


def test_unusable_templates_are_never_marked_and_never_stand_for_a_group():
    q = Q30 * 10
    good = _se(100, 0, [("M", 10)], q)
    unmapped = _se(100, 4, [("M", 10)], bytes([40]) * 10)
    secondary = _se(100, 0x100, [("M", 10)], bytes([40]) * 10)
    supplementary = _se(100, 0x800, [("M", 10)], bytes([40]) * 10)
    no_cigar = _se(100, 0, [], bytes([40]) * 10)
    recs = [unmapped, secondary, supplementary, no_cigar, None, b"", good, good]
    sigs = signatures(recs, False)
    assert sigs[:6] == [NO_SIG] * 6 and all(s[4] == DUP_NONE for s in sigs[:6])
    assert select(sigs) == [0, 0, 0, 0, 0, 0, 0, 1]                         # the better-scored unusable ones stand for nothing
    assert mark(recs, False)[:7] == recs[:7]
    # pairs: none usable -> no signature; one usable -> the single-record form of that record; both records of a marked template change
    m1 = make_record(0, 100, 0x49, [("M", 10)], q); m2u = make_record(0, 100, 0x85, [], q)
    assert signature([m2u, m2u]) == NO_SIG and signature([None, None]) == NO_SIG
    assert signature([m1, m2u]) == signature([m1, None]) == signature([None, m1]) == (0, 100, -1, -1, 0, 300)
    assert select(signatures([m1, m2u, m1, m2u, None, None], True)) == [0, 1, 0]
    assert _flags(mark([m1, m2u, m1, m2u], True)) == [0x49, 0x85, 0x449, 0x485]


def test_markdup_without_sort_is_refused_by_name():
    drv = os.path.join(ROOT, "bitmapperbs_amd", "bmbs_search")
    assert os.path.exists(drv), "bmbs_search not built (make -C bitmapperbs_amd/csrc)"
    p = subprocess.run([drv, "--search", "nowhere", "--seq", "none.fq", "--bam", "--markdup"], capture_output=True, text=True)
    assert p.returncode == 2
    assert "bmbs_search: --markdup needs --sort" in p.stderr
