"""tests/methyl_spec.py (the methylation-calling rule of `--bam --sort --methyl`) on hand-worked records, and the driver's refusals that
need no device."""
import os
import subprocess

import pytest

import methyl_spec as spec
from common import ROOT

L = {"A": 0, "C": 1, "G": 2, "T": 3}


def g(text):
    return bytes(L[c] for c in text)


def rec(pos, flag, cigar, seq, quals=None, ref=0, mapq=30):
    return spec.make_record(ref, pos, flag, cigar, seq, quals if quals is not None else [30] * len(seq), mapq=mapq)


def test_contexts_on_both_strands():
    #          0123456789
    seq = g("ACGTCAGTCTTAGG")
    assert spec.context(seq, 1) == (spec.CPG, 0)                # C G
    assert spec.context(seq, 2) == (spec.CPG, 1)                # the G of that CpG
    assert spec.context(seq, 4) == (spec.CHG, 0)                # C A G
    assert spec.context(seq, 6) == (spec.CHG, 1)                # C A G read from the other strand
    assert spec.context(seq, 8) == (spec.CHH, 0)                # C T T
    assert spec.context(seq, 12) == (spec.CHH, 1)               # T A G: no C one or two before
    assert spec.context(seq, 13) == (spec.CHH, 1)
    assert spec.context(seq, 0) is None and spec.context(seq, 3) is None      # A, T
    assert spec.context(seq, -1) is None and spec.context(seq, 14) is None


def test_contexts_at_the_first_and_last_two_bases():
    # a C needs p + 2 inside unless p + 1 is G; a G needs p - 2 inside unless p - 1 is C
    assert spec.context(g("GGCAC"), 0) is None                  # G at 0: nothing before it
    assert spec.context(g("GGCAC"), 1) is None                  # G at 1: p - 1 is G, p - 2 is outside
    assert spec.context(g("CGCAC"), 1) == (spec.CPG, 1)         # G at 1 behind a C
    assert spec.context(g("CAGAC"), 2) == (spec.CHG, 1)         # G at 2, C at 0
    assert spec.context(g("AAGAC"), 2) == (spec.CHH, 1)
    assert spec.context(g("GGCAC"), 4) is None                  # C at the last base
    assert spec.context(g("GGCCA"), 3) is None                  # C at the last but one, no G behind
    assert spec.context(g("GGACG"), 3) == (spec.CPG, 0)         # ... but a CpG needs only p + 1
    assert spec.context(g("GGCAG"), 2) == (spec.CHG, 0)
    assert spec.context(g("GGCAA"), 2) == (spec.CHH, 0)
    assert spec.context(g("C"), 0) is None and spec.context(g("G"), 0) is None


def test_the_flag_to_strand_table():
    ob = {f: spec.is_ob(f) for f in (0, 16, 0x43, 0x53, 0x83, 0x93, 1, 17)}
    assert ob == {0: False, 16: True, 0x43: False, 0x53: True, 0x83: True, 0x93: False, 1: False, 17: False}
    # (17: paired without a read number -- neither clause of the paired rule holds, so OT)


GEN = [g("ACGTCAGTCTTACGCCGGATCACGTTAGCA")]
#         012345678901234567890123456789


def test_every_cigar_operation():
    # 2S 3M 1I 2M 2D 1N 2= 1X 1P 2H from position 1: S S | C G T | i | C A | (G T C) | T T | A | -
    #                                    read index       0 1   2 3 4   5   6 7             8 9   10
    #                                    reference                1 2 3       4 5   6 7 8   9 10  11
    r = rec(1, 0, [("S", 2), ("M", 3), ("I", 1), ("M", 2), ("D", 2), ("N", 1), ("=", 2), ("X", 1), ("P", 1), ("H", 2)], "CCCGTCTAGTC")
    assert spec.ref_span(spec.fields(r)[4]) == 11
    got = spec.sites(GEN, [r], contexts=7)
    # forward C at 1 (CpG, read C), at 4 (CHG, read T); 8 lies in the deletion; the X base at 11 is A in the genome
    assert got == [(0, 1, 1, 0, spec.CPG), (0, 4, 0, 1, spec.CHG)]
    # the same record on the other strand is called at G: 2 (CpG, read G)
    r = rec(1, 16, [("S", 2), ("M", 3), ("I", 1), ("M", 2), ("D", 2), ("N", 1), ("=", 2), ("X", 1), ("P", 1), ("H", 2)], "CCCGTCTAGTC")
    assert spec.sites(GEN, [r], contexts=7) == [(0, 2, 1, 0, spec.CPG | 4)]


def test_calls_by_strand_and_context_selection():
    ot = rec(0, 0, [("M", 12)], "ATGTTAGTCTTA")                 # C at 1 read T, C at 4 read T, C at 8 read C
    obr = rec(0, 16, [("M", 12)], "ACATCAATCTTA")               # G at 2 read A, G at 6 read A
    assert spec.sites(GEN, [ot, obr], contexts=7) == [(0, 1, 0, 1, 0), (0, 2, 0, 1, 4), (0, 4, 0, 1, 1), (0, 6, 0, 1, 5), (0, 8, 1, 0, 2)]
    assert spec.sites(GEN, [ot, obr]) == [(0, 1, 0, 1, 0), (0, 2, 0, 1, 4)]
    assert spec.sites(GEN, [ot, obr], contexts=6) == spec.select(spec.sites(GEN, [ot, obr], contexts=7), 6)
    # anything but C / T (G / A) counts as nothing; two records add up
    assert spec.sites(GEN, [rec(0, 0, [("M", 3)], "AGG"), rec(0, 0, [("M", 3)], "ACG"), rec(1, 0, [("M", 2)], "TG")]) == [(0, 1, 1, 1, 0)]


def test_thresholds_at_t_minus_one_and_t():
    s = "ACG"
    assert spec.sites(GEN, [rec(0, 0, [("M", 3)], s, mapq=9)]) == []
    assert spec.sites(GEN, [rec(0, 0, [("M", 3)], s, mapq=10)]) == [(0, 1, 1, 0, 0)]
    assert spec.sites(GEN, [rec(0, 0, [("M", 3)], s, mapq=10)], min_mapq=11) == []
    assert spec.sites(GEN, [rec(0, 0, [("M", 3)], s, [30, 4, 30])]) == []
    assert spec.sites(GEN, [rec(0, 0, [("M", 3)], s, [30, 5, 30])]) == [(0, 1, 1, 0, 0)]
    assert spec.sites(GEN, [rec(0, 0, [("M", 3)], s, [0, 0xff, 0])]) == []          # "no quality" counts as 0
    assert spec.sites(GEN, [rec(0, 0, [("M", 3)], s, [0, 0xff, 0])], min_phred=0) == [(0, 1, 1, 0, 0)]


def test_which_records_count():
    s = "ACG"
    why = lambda r: spec.skip_reason(r)
    assert why(rec(0, 0, [("M", 3)], s)) is None and why(b"") == "none"
    assert why(rec(0, 4, [("M", 3)], s)) == "unmapped" and why(rec(0, 0, [("M", 3)], s, ref=-1)) == "unmapped"
    for f in (0x100, 0x200, 0x400, 0x800):
        assert why(rec(0, f, [("M", 3)], s)) == "flag"
    assert why(rec(0, 0, [], s)) == "cigar"
    assert why(rec(0, 0x41, [("M", 3)], s)) == "improper" and why(rec(0, 0x43, [("M", 3)], s)) is None
    with pytest.raises(ValueError, match="record 1.*beyond"):
        spec.sites(GEN, [rec(0, 0, [("M", 3)], s), rec(0, 0, [("M", 3)], s, ref=1)])
    with pytest.raises(ValueError, match="record 0.*runs off"):
        spec.sites(GEN, [rec(28, 0, [("M", 3)], s)])
    assert spec.sites(GEN, [rec(27, 0, [("M", 3)], "AGC")]) == []                    # the C at the last base has no context


def test_a_clip():
    # read 1 covers 0..7, read 2 (forward: OB) covers 4..15: the overlap 4..7 is read 1's alone
    r1 = rec(0, 0x63, [("M", 8)], "ATGTTAGT")
    r2 = rec(4, 0x83, [("S", 1), ("M", 12)], "ACAATCTTACACC")
    assert spec.clips([r1, r2]) == [0, 0 << 16 | 4] and spec.clips([r2, r1]) == [4, 0]
    assert spec.clip_of(rec(6, 0x83, [("M", 4)], "ACGT"), rec(0, 0x63, [("M", 8)], "ATGTTAGT")) == 0 << 16 | 2
    assert spec.clip_of(rec(0, 0x83, [("M", 8)], "ATGTTAGT"), rec(6, 0x63, [("M", 4)], "ACGT")) == 6 << 16 | 2
    assert spec.clip_of(r2, rec(0, 0x67, [("M", 8)], "ATGTTAGT")) == 0              # the mate is unmapped
    assert spec.clip_of(r2, rec(0, 0x63, [("M", 8)], "ATGTTAGT", ref=-1)) == 0      # another reference
    assert spec.clip_of(r2, rec(20, 0x63, [("M", 8)], "ATGTTAGT")) == 0             # no overlap
    without = spec.sites(GEN, [r1, r2], contexts=7)
    with_clip = spec.sites(GEN, [r1, r2], clip=spec.clips([r1, r2]), contexts=7)
    assert (0, 6, 0, 1, 5) in without and (0, 6, 0, 1, 5) not in with_clip          # the G at 6 was read 2's call (A)
    assert [s for s in without if s[1] >= 8] == [s for s in with_clip if s[1] >= 8] and any(s[1] >= 8 for s in with_clip)
    assert [s for s in with_clip if s[1] < 8] == spec.sites(GEN, [r1], contexts=7)


def test_the_percent_rounds_half_up():
    assert spec.pct(1, 0) == 100 and spec.pct(0, 1) == 0
    assert spec.pct(1, 1) == 50
    assert spec.pct(1, 7) == 13                                 # 12.5
    assert spec.pct(1, 199) == 1                                # 0.5
    assert spec.pct(1, 200) == 0                                # 0.4975...
    assert spec.pct(3, 5) == 38                                 # 37.5
    assert spec.pct(2, 1) == 67 and spec.pct(1, 2) == 33
    text = spec.bedgraph("out/x", spec.CHG, ["chrA"], [(0, 4, 1, 7, spec.CHG), (0, 6, 3, 5, spec.CHG | 4), (0, 1, 1, 0, spec.CPG)]).decode()
    assert text == 'track type="bedGraph" description="out/x CHG methylation levels"\nchrA\t4\t5\t13\t1\t7\nchrA\t6\t7\t38\t3\t5\n'


def test_the_driver_refuses_methyl_without_sort_before_any_device_work():
    exe = os.path.join(ROOT, "bitmapperbs_amd", "bmbs_search")
    assert os.path.exists(exe), "bmbs_search not built (make -C bitmapperbs_amd/csrc)"
    for args in (["--methyl", "x"], ["--bam", "--methyl", "x"]):
        p = subprocess.run([exe, "--search", "/nonexistent/index", "--seq", "/nonexistent/r.fq"] + args, capture_output=True, text=True)
        assert p.returncode == 2 and "--methyl needs --sort" in p.stderr, p.stderr
    p = subprocess.run([exe, "--search", "/nonexistent/index", "--seq", "/nonexistent/r.fq", "--bam", "--sort", "--methy_out"], capture_output=True, text=True)
    assert p.returncode == 2 and "--methy_out" in p.stderr, p.stderr
