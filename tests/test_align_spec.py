"""Host only: the two references of the alignment stage -- tests/align_spec.py (plain numpy, from ksw.cpp) and orc.align (the
oracle) -- agree on every crafted job of tests/align_cases.py, and the jobs are what they claim to be.  Both must hold before
either judges the device (tests/test_align_forms.py)."""
import re

import numpy as np
import pytest

import align_cases as ac
import align_spec
import orc

SPEC_KEYS = ("start", "end", "nm", "score", "cigar")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    wd = tmp_path_factory.mktemp("align_spec")
    _, env_oix = ac.build_index(wd, *ac.make_env_genome(), "g")
    _, hp_oix = ac.build_index(wd, *ac.make_homopolymer_genome(), "hp")
    return dict(env=env_oix, hp=hp_oix, cache={})


def case_data(world, name):
    """jobs, oracle results and spec results of a case, computed once"""
    if name not in world["cache"]:
        case = ac.CASE_BY_NAME[name]
        jobs = ac.build_jobs(case, world[case["genome"]])
        L, k = case["L"], case["k"]
        prm = orc.params(**ac.params_of(case["scoring"], L, k))
        n = len(jobs["pattern"])
        d = dict(case=case, jobs=jobs, prm=prm, orc=ac.reference_results(case, jobs),
                 spec=align_spec.align_batch(prm, jobs["windows"], jobs["seq"][:, :L], jobs["qual"][:, :L], k, jobs["end"], jobs["err"], jobs["forward"]))
        rq = np.arange(n) >= n // 2          # mirrored qualities for the second half of the reads, as the device test runs them
        d["orc_rev"] = ac.reference_results(case, jobs, rq)
        d["spec_rev"] = align_spec.align_batch(prm, jobs["windows"], jobs["seq"][:, :L], jobs["qual"][:, :L], k, jobs["end"], jobs["err"],
                                               jobs["forward"], rq)
        world["cache"][name] = d
    return world["cache"][name]


def everything(world):
    return [case_data(world, c["name"]) for c in ac.CASES]


@pytest.mark.parametrize("name", [c["name"] for c in ac.CASES])
def test_spec_and_oracle_agree_and_every_job_is_accepted(world, name):
    d = case_data(world, name)
    jobs, k = d["jobs"], d["case"]["k"]
    assert jobs["accepted"].all(), [(j, jobs["pattern"][j], int(jobs["err"][j])) for j in np.nonzero(~jobs["accepted"])[0]]
    # the case's count is the number of jobs that reach the DP kernels, and align_cases.needs_dp knows which they are
    assert [s["raw"] is not None for s in d["spec"]] == jobs["dp"].tolist()
    assert int(jobs["dp"].sum()) == d["case"]["n"] > 0
    if d["case"]["n"] >= 63:          # several patterns, both strands
        dp = jobs["dp"]
        assert len({p for p, x in zip(jobs["pattern"], dp) if x}) >= 2 and (jobs["forward"] & dp).sum() >= 20 and (~jobs["forward"] & dp).sum() >= 20
    assert ac.packed16_by_the_guard(d["case"]["scoring"], d["case"]["L"]) == d["case"]["packed16"]
    for which in ("", "_rev"):
        for j, (o, s) in enumerate(zip(d["orc" + which], d["spec" + which])):
            assert tuple(s[f] for f in SPEC_KEYS) == tuple(o[f] for f in SPEC_KEYS), (j, jobs["pattern"][j], which)
    if d["case"]["genome"] == "hp":
        for j, p in enumerate(jobs["pattern"]):
            if p in ac.HP_PATTERNS:
                assert (jobs["windows"][j, k + 40:k + 40 + ac.HP_RUN] == ac.A).all() and jobs["windows"][j, k + 39] != ac.A


def test_mirrored_qualities_change_results(world):
    """the mirrored runs are not the plain runs again"""
    diff = 0
    for d in everything(world):
        diff += sum(a["score"] != b["score"] for a, b in zip(d["orc"], d["orc_rev"]))
    assert diff >= 20, diff


def test_a_read_of_nothing_but_n_is_never_accepted(world):
    """why no case carries the `all_n` pattern"""
    oix = world["env"]
    for L, k in sorted({(c["L"], c["k"]) for c in ac.CASES}):
        w = oix.window(5000, L + 2 * k)
        err, _ = orc.bpm(w, np.full(L, ac.N, dtype=np.uint8), k)
        assert err > k, (L, k, err)


def _gap_read_offset(raw, op):
    """read offsets at which runs of `op` start in a raw CIGAR"""
    at, out = 0, []
    for n, o in re.findall(r"(\d+)([MDI])", raw):
        if o == op:
            out.append(at)
        if o != "D":
            at += int(n)
    return out


def _n_class(p_of):
    """an N class counts where the read really has its N at the class's position, the DP ran, and NM counts the N on top of the deletion"""
    return lambda o, s, k, L, read: read[p_of(L)] == ac.N and s["raw"] is not None and o["nm"] >= 2


# what a job of the class must show for the class to count as exercised: (oracle result, spec result, k, L, read) -> bool
INTENDED = {
    "exact": lambda o, s, k, L, read: s["raw"] is None and o["nm"] == 0 and o["cigar"] == "%dM" % L,
    "ins_first": lambda o, s, k, L, read: s["raw"] is not None and re.match(r"^\d+I", s["raw"]) is not None,           # rewritten to M afterwards
    "ins_last": lambda o, s, k, L, read: s["raw"] is not None and re.search(r"\d+I$", s["raw"]) is not None,
    "ins_second": lambda o, s, k, L, read: s["raw"] is not None and re.match(r"^1M1I", s["raw"]) is not None,
    # (a deletion next to an end base costs what dropping that base as an insertion costs, and the DP's tie-breaking takes the latter:
    # either way the CIGAR has a gap within one base of that end)
    "del_second": lambda o, s, k, L, read: s["raw"] is not None and re.match(r"^(1M)?\d+[ID]", s["raw"]) is not None,
    "del_before_last": lambda o, s, k, L, read: s["raw"] is not None and re.search(r"\d+[ID](1M)?$", s["raw"]) is not None,
    "gap_k_ins": lambda o, s, k, L, read: s["raw"] is not None and "M%dI" % k in s["raw"],
    "gap_k_del": lambda o, s, k, L, read: s["raw"] is not None and "M%dD" % k in s["raw"],
    # (see test_no_cigar_has_an_insertion_next_to_a_deletion: the pair is one mismatch to the filter and to the un-gapped exit)
    "ins_del": lambda o, s, k, L, read: s["raw"] is None and o["nm"] == 1 and o["cigar"] == "%dM" % L,
    "k_mismatches": lambda o, s, k, L, read: o["nm"] == k and o["cigar"] == "%dM" % L,
    "t_over_c": lambda o, s, k, L, read: s["raw"] is not None and o["nm"] == 1,                                        # the deletion alone: every T over C matched
    "c_over_t": lambda o, s, k, L, read: o["nm"] >= 2 or (k == 1 and o["nm"] == 1),
    "n_first": _n_class(lambda L: 0),
    "n_mid": _n_class(lambda L: L // 2),
    "n_last": _n_class(lambda L: L - 1),
    "hp_ins": lambda o, s, k, L, read: s["raw"] is not None and any(40 <= x <= 52 for x in _gap_read_offset(s["raw"], "I")),
    "hp_del": lambda o, s, k, L, read: s["raw"] is not None and any(40 <= x <= 52 for x in _gap_read_offset(s["raw"], "D")),
}


def test_every_edit_class_shows_its_operation_in_at_least_20_jobs(world):
    count = {p: 0 for p in INTENDED}
    for d in everything(world):
        k, L = d["case"]["k"], d["case"]["L"]
        for j, (p, o, s) in enumerate(zip(d["jobs"]["pattern"], d["orc"], d["spec"])):
            count[p] += bool(INTENDED[p](o, s, k, L, d["jobs"]["seq"][j, :L]))
    print(count)
    assert all(v >= 20 for v in count.values()), count


def test_no_cigar_has_an_insertion_next_to_a_deletion(world):
    """E and F open from the diagonal term alone (ksw.cpp:1961-1971), so the traceback never steps from one kind of gap into the
    other: what the `ins_del` jobs (an I immediately followed by a D in the read's history) come out as is a mismatch or two gaps
    with a match between them, never `1I1D`"""
    seen = 0
    for d in everything(world):
        for s in d["spec"]:
            if s["raw"] is not None:
                seen += 1
                assert re.search(r"I\d+D|D\d+I", s["raw"]) is None, s["raw"]
    assert seen > 1000


def test_the_tie_set_scores_at_least_20_jobs_differently(world):
    d = case_data(world, "tie")
    case = dict(d["case"], scoring="defaults")
    other = ac.reference_results(case, d["jobs"])
    assert sum(a["score"] != b["score"] or a["cigar"] != b["cigar"] for a, b in zip(d["orc"], other)) >= 20
    assert sum(a["score"] != b["score"] for a, b in zip(d["orc"], other)) >= 20


def test_positive_scores_exist_under_phred64(world):
    d = case_data(world, "phred64")
    assert sum(o["score"] > 0 for o in d["orc"]) >= 20


def _range(d):
    ran = [s for s in d["spec"] if s["raw"] is not None]
    return min(s["lo"] for s in ran), max(s["hi"] for s in ran), len(ran)


def test_range_tracker_16_bits(world):
    """Which crafted parameter sets leave what signed 16 bits hold (the packed form, k_align_sw2, computes in 16 bits).

    mp_max = 2, mp_min = 60, L = 998 with every quality at q_base was expected to (an all-mismatch diagonal would reach -45 000).  It
    does not, for any job the filter accepts: H is a maximum, every cell of the band is within one gap of the diagonal of the accepted
    alignment, and that one has at most k = 31 edits -- the tracker stays above -4 000.  What does leave 16 bits is a single penalty
    that does not fit them (mp_min = 40 000): the diagonal candidate M = H - 40 000 of the first mismatching cell."""
    lo, hi, n = _range(case_data(world, "inverted60_L998"))
    print("inverted60_L998: lo %d hi %d over %d DP jobs" % (lo, hi, n))
    assert n >= 60 and -4000 < lo and hi <= 0
    d = case_data(world, "inverted40000")
    ran = [s for s in d["spec"] if s["raw"] is not None]
    assert len(ran) >= 30 and all(s["lo"] < -32768 for s in ran)
    for name in ("defaults_k8_L100", "maxpen12_L935", "maxpen12_L936", "phred64", "L998_k31"):
        lo, hi, n = _range(case_data(world, name))
        assert -12000 < lo and hi < 12000 and n > 0, (name, lo, hi)
