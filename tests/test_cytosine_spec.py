"""tests/cytosine_spec.py on hand-written cases: the expected lines are typed out here, worked out from the rule in include/bmbs.h by hand.
No GPU; this is what tests/test_cytosine_report.py measures the device against."""
import pytest

import cytosine_spec as cs


def S(text):
    return bytes("ACGT".index(c) for c in text)


def rep(text, contexts=7, runs=(), sites=(), beg=0, end=None, name="s"):
    seq = S(text)
    return cs.report([seq], [name], [list(runs)], list(sites), contexts, 0, beg, len(seq) if end is None else end).decode()


def test_a_cpg_in_the_middle_gives_a_line_on_either_strand():
    # A C G T: the C reads C G T on its strand; the G is the cytosine of the other strand, which reads C G T from there too
    assert rep("ACGT") == "s\t2\t+\t0\t0\tCG\tCGT\n" "s\t3\t-\t0\t0\tCG\tCGT\n"


def test_a_cpg_on_the_last_two_bases_has_no_third_letter():
    assert rep("AACG") == "s\t3\t+\t0\t0\tCG\tCGN\n" "s\t4\t-\t0\t0\tCG\tCGT\n"


def test_a_minus_strand_cpg_at_position_1_has_no_third_letter():
    assert rep("CGAA") == "s\t1\t+\t0\t0\tCG\tCGA\n" "s\t2\t-\t0\t0\tCG\tCGN\n"


@pytest.mark.parametrize("text, want", [
    ("C", ""), ("G", ""), ("A", ""),
    ("CG", "s\t1\t+\t0\t0\tCG\tCGN\n" "s\t2\t-\t0\t0\tCG\tCGN\n"),
    ("CC", ""), ("GG", ""), ("CA", ""),
    ("CAG", "s\t1\t+\t0\t0\tCHG\tCAG\n" "s\t3\t-\t0\t0\tCHG\tCTG\n"),
    ("CAA", "s\t1\t+\t0\t0\tCHH\tCAA\n"),
    ("CCC", "s\t1\t+\t0\t0\tCHH\tCCC\n"),
    ("TTG", "s\t3\t-\t0\t0\tCHH\tCAA\n"),
    ("GCG", "s\t2\t+\t0\t0\tCG\tCGN\n" "s\t3\t-\t0\t0\tCG\tCGC\n"),
])
def test_sequences_of_one_two_and_three_bases(text, want):
    assert rep(text) == want


def test_every_context_and_the_selection():
    #        0 1 2 3 4 5 6 7 8
    text = "CCGCAGCAA"
    chg = "s\t1\t+\t0\t0\tCHG\tCCG\n" "s\t4\t+\t0\t0\tCHG\tCAG\n" "s\t6\t-\t0\t0\tCHG\tCTG\n"
    cpg = "s\t2\t+\t0\t0\tCG\tCGC\n" "s\t3\t-\t0\t0\tCG\tCGG\n"
    chh = "s\t7\t+\t0\t0\tCHH\tCAA\n"
    assert rep(text, 1) == cpg and rep(text, 2) == chg and rep(text, 4) == chh
    assert rep(text, 7) == "s\t1\t+\t0\t0\tCHG\tCCG\n" + cpg + "s\t4\t+\t0\t0\tCHG\tCAG\n" "s\t6\t-\t0\t0\tCHG\tCTG\n" + chh
    assert rep(text, 5) == cpg + chh


def test_a_cpg_directly_in_front_of_a_run_is_written_with_n():
    # the T at 3 is not a letter of the FASTA: the window of the C (1, 2) and of the G (1, 2) stays clear of it
    assert rep("ACGTT", runs=[(3, 4)]) == "s\t2\t+\t0\t0\tCG\tCGN\n" "s\t3\t-\t0\t0\tCG\tCGT\n"
    # ... and mirrored: a run directly in front of the CpG takes the third letter of the G's line
    assert rep("TTCGA", runs=[(1, 2)]) == "s\t3\t+\t0\t0\tCG\tCGA\n" "s\t4\t-\t0\t0\tCG\tCGN\n"


def test_a_cytosine_beside_a_run_whose_window_reaches_into_it_has_no_line():
    assert rep("ACATT", runs=[(3, 4)]) == ""                 # CHH: its window is 1..3
    assert rep("ACATT", runs=[(4, 5)]) == "s\t2\t+\t0\t0\tCHH\tCAT\n"
    assert rep("TTAGA", runs=[(1, 2)]) == ""                 # the G at 3: CHH on the other strand, window 1..3
    assert rep("ACGT", runs=[(2, 3)]) == ""                  # a CpG whose G is in the run: neither strand has a line


def test_a_cytosine_inside_a_run_has_no_line():
    assert rep("ACGT", runs=[(1, 2)]) == ""
    assert rep("AACAAGAA", runs=[(2, 3)]) == "s\t6\t-\t0\t0\tCHH\tCTT\n"
    assert rep("AACAAGAA", runs=[(0, 8)]) == ""


def test_counts_of_a_site_and_an_omitted_site():
    assert rep("ACGT", sites=[(0, 1, 5, 7, 0), (0, 2, 0, 1000000000, 4)]) == "s\t2\t+\t5\t7\tCG\tCGT\n" "s\t3\t-\t0\t1000000000\tCG\tCGT\n"
    assert rep("ACGT", sites=[(0, 1, 3, 4, 0 | cs.REPORT_OMIT)]) == "s\t3\t-\t0\t0\tCG\tCGT\n"
    assert rep("ACGT", sites=[(0, 1, 4294967295, 0, 0), (0, 2, 1, 1, 4 | cs.REPORT_OMIT)]) == "s\t2\t+\t4294967295\t0\tCG\tCGT\n"


def test_windows_names_and_sequences():
    assert rep("ACGT", beg=2, end=3) == "s\t3\t-\t0\t0\tCG\tCGT\n"
    assert rep("ACGT", beg=1, end=2) == "s\t2\t+\t0\t0\tCG\tCGT\n"
    assert rep("ACGT", beg=2, end=2) == "" and rep("ACGT", beg=0, end=1) == "" and rep("ACGT", beg=4, end=4) == ""
    seqs, names = [S("AAAA"), S("ACGT"), S("CAA")], ["a", "chr2", "x" * 40]
    assert cs.report(seqs, names, None, [], 1, 1, 0, 4) == b"chr2\t2\t+\t0\t0\tCG\tCGT\n" b"chr2\t3\t-\t0\t0\tCG\tCGT\n"
    assert cs.report(seqs, names, None, [], 7, 0, 0, 4) == b""
    sites = [(1, 2, 9, 10, 4), (2, 0, 99, 100, 2)]
    assert cs.report_all(seqs, names, [[], [], []], sites, 7) == \
        b"chr2\t2\t+\t0\t0\tCG\tCGT\n" b"chr2\t3\t-\t9\t10\tCG\tCGT\n" + ("x" * 40).encode() + b"\t1\t+\t99\t100\tCHH\tCAA\n"


@pytest.mark.parametrize("kw, what", [
    (dict(ref=1), "outside the index"), (dict(ref=-1), "outside the index"),
    (dict(beg=-1), "window"), (dict(beg=3, end=2), "window"), (dict(end=5), "window"),
    (dict(contexts=0), "contexts"), (dict(contexts=8), "contexts"),
    (dict(runs=[(2, 3), (0, 1)]), "run 1"), (dict(runs=[(0, 2), (1, 3)]), "run 1"), (dict(runs=[(1, 1)]), "run 0"),
    (dict(sites=[(1, 1, 0, 0, 0)]), "site 0 has another ref"),
    (dict(sites=[(0, 1, 0, 0, 0)], beg=2), "site 0 lies outside"), (dict(sites=[(0, 2, 0, 0, 4)], end=2), "site 0 lies outside"),
    (dict(sites=[(0, 2, 0, 0, 4), (0, 1, 0, 0, 0)]), "site 1 does not sit behind"), (dict(sites=[(0, 1, 0, 0, 0), (0, 1, 0, 0, 0)]), "site 1 does not sit behind"),
    (dict(sites=[(0, 1, 0, 0, 4)]), "kind of site 0"), (dict(sites=[(0, 1, 0, 0, 1)]), "kind of site 0"), (dict(sites=[(0, 0, 0, 0, 0)]), "kind of site 0"),
    (dict(sites=[(0, 1, 0, 0, 16)]), "kind of site 0"),
    (dict(sites=[(0, 1, 0, 0, 0)], contexts=6), "context of site 0"),
    (dict(sites=[(0, 1, 0, 0, 0)], runs=[(2, 3)]), "window of site 0"), (dict(sites=[(0, 1, 0, 0, 0), (0, 2, 0, 0, 4 | cs.REPORT_OMIT)], runs=[(1, 2)]), "window of site 0"),
])
def test_what_check_refuses(kw, what):
    args = dict(ref=0, beg=0, end=4, contexts=7, runs=[], sites=[])
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        cs.report([S("ACGT")], ["s"], [args["runs"]], args["sites"], args["contexts"], args["ref"], args["beg"], args["end"])
