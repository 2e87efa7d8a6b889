"""tests/mbias_spec.py against tests/methyl_spec.py, on the letters of the golden genome (no GPU): without a trim the two give the same
sites, and the M-bias table holds exactly the calls the sites are made of -- all of them, and, cut down to the cycles a trim keeps, the
calls of the trimmed sites."""
import gzip
import os

import numpy as np
import pytest

import mbias_spec
import methyl_spec as spec
import test_methyl
from common import GOLD

L_SEQS = (1, 2, 31, 32, 33, 63, 64, 65, 151, 255, 256, 257, 998, 1023)             # (no bin is clamped: l_seq <= 1023)
# (ignore_5p, ignore_3p), each (read 1 or single end, read 2)
TRIMS = (((5, 0), (0, 0)), ((0, 3), (0, 0)), ((2, 1), (7, 4)), ((40, 40), (0, 0)), ((0, 0), (30, 2)))


def golden_seqs():
    text = gzip.open(os.path.join(GOLD, "genome.fa.gz"), "rt").read()
    return [bytes("ACGT".index(c) for c in "".join(block.split("\n")[1:]).upper()) for block in text.split(">")[1:]]


def random_records(rng, seqs, n, l_seqs, stack=False):
    """n records of test_methyl.py's generator with l_seq drawn from l_seqs (the generator reads its lengths from the module)"""
    keep = test_methyl.L_SEQS
    test_methyl.L_SEQS = tuple(l_seqs)
    try:
        return [test_methyl._random_record(rng, seqs, stack=stack) for _ in range(n)]
    finally:
        test_methyl.L_SEQS = keep


@pytest.fixture(scope="module")
def made():
    rng = np.random.default_rng(17)
    seqs = golden_seqs()
    recs = random_records(rng, seqs, 3000, L_SEQS)
    recs = [b"" if i % 13 == 5 else r for i, r in enumerate(recs)]
    clip = [test_methyl._random_clip(rng, r) if r else 0 for r in recs]
    return dict(seqs=seqs, recs=recs, clip=clip, walked=mbias_spec.walk(seqs, recs, clip))


def test_without_a_trim_the_sites_are_those_of_methyl_spec(made):
    for clip in (made["clip"], None):
        for contexts in (7, 2):
            want = spec.sites(made["seqs"], made["recs"], clip, contexts=contexts)
            assert mbias_spec.sites(made["seqs"], made["recs"], clip, contexts=contexts) == want and len(want) > 1000
    assert mbias_spec.sites_of(made["walked"], 7) == spec.sites(made["seqs"], made["recs"], made["clip"], contexts=7)


def test_the_table_holds_the_calls_of_the_untrimmed_sites(made):
    t = mbias_spec.table_of(made["walked"], 7)
    all_sites = mbias_spec.sites_of(made["walked"], 7)
    assert mbias_spec.total(t) == sum(s[2] + s[3] for s in all_sites) > 10_000
    # row by row: the sites know context, strand and the two counts, not the mate
    for ctx in range(3):
        for strand in range(2):
            for m in range(2):
                assert sum(t[0][strand][ctx][m]) + sum(t[1][strand][ctx][m]) == sum(s[2 if m else 3] for s in all_sites if s[4] == ctx | strand << 2) > 0
    # a narrower selection leaves the other rows zero and these as they are
    t2 = mbias_spec.table_of(made["walked"], 2)
    assert t2[0][0][1] == t[0][0][1] and t2[1][1][1] == t[1][1][1] and not any(x for mate in t2 for strand in mate for ctx in (0, 2) for m in strand[ctx] for x in m)
    assert mbias_spec.tsv(t).count(b"\n") == 1 + sum(1 for mate in t for strand in mate for ctx in strand for c in range(mbias_spec.CYCLES) if ctx[0][c] + ctx[1][c])


@pytest.mark.parametrize("trim", TRIMS)
def test_the_table_cut_to_the_kept_cycles_holds_the_calls_of_the_trimmed_sites(made, trim):
    """per l_seq (the 3' bound of a record is counted from its own length): the table of the records of one length, summed over the bins
    ignore_5p[mate] <= cycle < l_seq - ignore_3p[mate], against the counts of the same records' trimmed sites"""
    i5, i3 = trim
    by_len = {}
    for c in made["walked"]:
        by_len.setdefault(c[2], []).append(c)
    assert set(by_len) >= set(L_SEQS[2:])
    removed = 0
    for l_seq, walked in by_len.items():
        t = mbias_spec.table_of(walked, 7)
        trimmed = mbias_spec.sites_of(walked, 7, i5, i3)
        for ctx in range(3):
            for strand in range(2):
                for m in range(2):
                    kept = sum(sum(t[mate][strand][ctx][m][i5[mate]:max(i5[mate], l_seq - i3[mate])]) for mate in range(2))
                    assert kept == sum(s[2 if m else 3] for s in trimmed if s[4] == ctx | strand << 2), (l_seq, ctx, strand, m)
        removed += mbias_spec.total(t) - sum(s[2] + s[3] for s in trimmed)
    assert removed > 100
