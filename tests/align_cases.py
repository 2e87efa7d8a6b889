"""Crafted jobs for the alignment stage (tests/test_align_spec.py on the host, tests/test_align_forms.py on the device).

A job is a read laid over the window `oix.window(site, L + 2k)`: the window's bases k .. k + L, bisulfite-converted (C -> T with
probability 0.7, the same rule on both strands of the doubled genome), with ONE named edit pattern applied.  What the filter would
hand to the stage, (err, end), comes from orc.bpm on the host, so a failure on the device isolates the alignment stage.

Everything here is deterministic in (case, genome): the host test and the device test build the same jobs."""
import zlib

import numpy as np

import orc

A, C_, G_, T, N = (ord(c) for c in "ACGTN")

# ---- the genomes -------------------------------------------------------------------------------------------------------------
GENOME = dict(total=1_500_000, n_chrom=3, seed=77, repeats_seed=78)          # what the `env` fixture of test_gpu_parity.py builds
HP_RUN = 12


def make_env_genome():
    from bitmapperbs_amd import synth
    from common import plant_repeats
    names, chroms = synth.make_genome(GENOME["total"], GENOME["n_chrom"], seed=GENOME["seed"])
    plant_repeats(chroms, seed=GENOME["repeats_seed"])
    return names, chroms


def make_homopolymer_genome():
    """a random genome of 4^12 bases has no run of twelve A: a small one with such runs planted every 1000 bases, A at the odd
    thousands and T (twelve A on the reverse strand) at the even ones"""
    from bitmapperbs_amd import synth
    names, chroms = synth.make_genome(200_000, 1, seed=4242)
    ch = chroms[0]
    for j, p in enumerate(range(1000, ch.size - 1000, 1000)):
        ch[p:p + HP_RUN] = A if j % 2 == 0 else T
        for q in (p - 1, p + HP_RUN):          # the run is exactly twelve long
            if ch[q] == ch[p]:
                ch[q] = G_
    return names, chroms


def build_index(wd, names, chroms, tag):
    """-> (fasta / index prefix, orc.OrcIndex); the index is built on the host cores"""
    import os
    from bitmapperbs_amd import synth, mapper
    fa = os.path.join(str(wd), tag + ".fa")
    synth.write_fasta(fa, names, chroms)
    mapper.Index.build(fa, fa, threads=8)
    return fa, orc.OrcIndex(fa)


# ---- scoring sets ------------------------------------------------------------------------------------------------------------
# (the quality bytes are Phred+33, '!' .. 'J', unless build_jobs says otherwise for the set)
SCORING = {
    "defaults": dict(),
    "gap_open0": dict(gap_open=0),
    "gap_ext255": dict(gap_ext=255),                       # the two sides of the `gap_ext < 256` condition of the packed form
    "gap_ext256": dict(gap_ext=256),
    "tie": dict(mp_max=8, mp_min=8, gap_open=5, gap_ext=3),          # a gap of one costs what a mismatch costs
    "np0": dict(np=0),
    "np_big": dict(np=9),                                  # above mp_max
    "flat": dict(mp_max=6, mp_min=6),
    "inverted": dict(mp_max=2, mp_min=6),
    "maxpen12": dict(gap_open=9, gap_ext=3),               # (L + 64) * 12 < 12000 at L = 935, not at L = 936
    "phred64": dict(q_base=64),                            # on Phred+33 bytes: penalties below zero, scores above
    "inverted60": dict(mp_max=2, mp_min=60),               # with qualities at q_base: every mismatch costs 60
    "inverted40000": dict(mp_max=2, mp_min=40000),         # a single mismatch is more than 16 bits hold
}
QUAL_AT_BASE = ("inverted60", "inverted40000")


def params_of(scoring, L, k):
    kw = dict(SCORING[scoring])
    kw["e_f"] = e_for(L, k)
    return kw


def e_for(L, k):
    """an -e that gives threshold k at length L (threshold = min(int(e * L), 31))"""
    e = (k + 0.5) / L
    assert min(int(np.uint64(e * L)), 31) == k, (L, k)
    return e


# ---- edit patterns -----------------------------------------------------------------------------------------------------------
# a script is a list of steps over the window, starting at column k:
#   ("M", n) n window bases, converted      ("X", 1) a base that mismatches the window's      ("I", g) g bases the window does not have
#   ("D", g) g window bases skipped         ("N", 1) an N over a window base                   ("T", 1) T over a window base (a C: a match)
#   ("C", 1) C over a window base (a T: a mismatch)                                     ("A", 1) an extra A (into a run of A)
def _split(total, cuts):
    """steps ("M", ..) around single-base steps at the sorted positions `cuts` = [(pos, step)], over `total` read bases"""
    out, at = [], 0
    for pos, step in cuts:
        if pos > at:
            out.append(("M", pos - at))
        out.append(step)
        at = pos + 1
    if total > at:
        out.append(("M", total - at))
    return out


def script_for(name, L, k, w, rng, turn):
    """-> script, or None when this window cannot carry the pattern (the caller draws another site).  turn: how often the case has
    used the pattern before"""
    core = w[k:k + L]
    if name == "exact":
        return [("M", L)]
    if name in END_GAPS:
        # a gap at an end of the read is one mismatch to the filter and to the un-gapped exit; every other pair of turns the read
        # carries a deletion in its middle as well, so that the DP runs and has to decide what the end is
        h = L // 2
        mid = k >= 2 and (turn // 2) % 2 == 1
        head, tail = ([("M", h), ("D", 1)], L - h) if mid else ([], L)          # steps before the tail, read bases the tail has
        if name == "ins_first":
            return [("I", 1), ("M", h - 1), ("D", 1), ("M", L - h)] if mid else [("I", 1), ("M", L - 1)]
        if name == "ins_second":
            return [("M", 1), ("I", 1), ("M", h - 2), ("D", 1), ("M", L - h)] if mid else [("M", 1), ("I", 1), ("M", L - 2)]
        if name == "del_second":
            return [("M", 1), ("D", 1), ("M", h - 1), ("D", 1), ("M", L - h)] if mid else [("M", 1), ("D", 1), ("M", L - 1)]
        if name == "ins_last":
            return head + [("M", tail - 1), ("I", 1)]
        return head + [("M", tail - 1), ("D", 1), ("M", 1)]          # del_before_last
    if name == "gap_k_ins":
        a = L // 3
        return [("M", a), ("I", k), ("M", L - a - k)]
    if name == "gap_k_del":
        a = L // 3
        return [("M", a), ("D", k), ("M", L - a)]
    if name == "ins_del":
        a = L // 2
        return [("M", a), ("I", 1), ("D", 1), ("M", L - a - 1)]
    if name == "k_mismatches":
        pos = sorted(rng.choice(L, size=k, replace=False).tolist())
        return _split(L, [(p, ("X", 1)) for p in pos])
    if name in ("t_over_c", "c_over_t"):
        want = C_ if name == "t_over_c" else T
        step = ("T", 1) if name == "t_over_c" else ("C", 1)
        at = np.nonzero(core == want)[0]
        at = at[at < L // 2 - 1] if k >= 2 else at          # left of the deletion below, where read and window columns still agree
        if at.size == 0:
            return None
        take = at if name == "t_over_c" else at[:max(1, min(3, k - 1))]
        s = _split(L // 2 if k >= 2 else L, [(int(p), step) for p in take])
        if k >= 2:                                          # one deletion, so that the DP runs and not only the un-gapped exit
            s += [("D", 1), ("M", L - L // 2)]
        return s
    if name in ("n_first", "n_mid", "n_last"):
        p = {"n_first": 0, "n_mid": L // 2, "n_last": L - 1}[name]
        if k >= 2 and (turn // 2) % 2 == 1:                 # alternately (per strand): the un-gapped exit, and a deletion as well (the DP)
            d = L // 4
            return _split(d, [(p, ("N", 1))] if p < d else []) + [("D", 1)] + \
                _split(L - d, [(p - d, ("N", 1))] if p >= d else [])
        return _split(L, [(p, ("N", 1))])
    raise KeyError(name)


PATTERNS = ("exact", "ins_first", "ins_second", "ins_last", "del_second", "del_before_last", "gap_k_ins", "gap_k_del", "ins_del",
            "k_mismatches", "t_over_c", "c_over_t", "n_first", "n_mid", "n_last")
# a read of nothing but N has L edits against any window and L > k always: the filter accepts it at no threshold, so no case carries
# it (tests/test_align_spec.py asserts the rejection at every threshold used here)
NEVER_ACCEPTED = ("all_n",)
END_GAPS = ("ins_first", "ins_second", "ins_last", "del_second", "del_before_last")
HP_PATTERNS = ("hp_ins", "hp_del")


def pattern_names(L, k):
    """the patterns a case of (L, k) carries; what is left out is left out here, by name"""
    names = list(PATTERNS)
    if 3 * k + 3 > L:          # a gap of k plus flanks that pin it do not fit the read
        names.remove("gap_k_ins"); names.remove("gap_k_del")
    return names


def render(script, w, k, L, rng, conv=0.7):
    out = []
    pos = k
    for op, n in script:
        if op == "M":
            seg = w[pos:pos + n].copy()
            m = (seg == C_) & (rng.random(n) < conv)
            seg[m] = T
            out.extend(seg.tolist()); pos += n
        elif op == "X":
            wb = int(w[pos])
            choices = [b for b in (A, C_, G_, T) if b != wb and not (b == T and wb == C_)]
            out.append(choices[int(rng.integers(len(choices)))]); pos += 1
        elif op == "I":
            for _ in range(n):          # bases that match neither neighbour of the gap, so that the gap is a gap
                bad = {int(w[pos]), int(w[pos - 1])}
                if C_ in bad:
                    bad.add(T)
                choices = [b for b in (A, C_, G_, T) if b not in bad] or [A]
                out.append(choices[int(rng.integers(len(choices)))])
        elif op == "D":
            pos += n
        elif op == "N":
            out.append(N); pos += 1
        elif op == "A":          # an A the window does not have (the homopolymer jobs)
            out.extend([A] * n)
        elif op == "T":
            assert w[pos] == C_
            out.append(T); pos += 1
        elif op == "C":
            assert w[pos] == T
            out.append(C_); pos += 1
    assert len(out) == L and pos <= L + 2 * k, (len(out), pos, script)
    return np.array(out, dtype=np.uint8)


# ---- cases -------------------------------------------------------------------------------------------------------------------
# (k, L, n) with n = the jobs that reach the DP kernels (build_jobs counts them with needs_dp).  k: 3 4 7 8 15 16 23 24 31 put the band
# 2k + 1 on either side of 8, 16, 32 and 48 cells; every band bound the register kernels are instantiated for (2 4 6 8 10 12 16 20 24
# 31) appears as k == KB and as k == KB - 1, each with dozens of DP jobs of several patterns on both strands.  The counts: 63 64 65 and
# 127 128 129 130 fill whole waves of one-job lanes, or leave one job over or one lane idle; as pairs (two jobs per lane) 63 65 127 129
# leave lane B of the last pair empty and 128 130 fill one wave of pairs exactly and spill one pair; 1 2 3 are the smallest launches.
BAND_CASES = [(1, 20, 63), (2, 61, 64), (3, 100, 65), (4, 151, 127), (5, 250, 128), (6, 61, 129), (7, 100, 130), (8, 151, 63), (9, 250, 64),
              (10, 61, 65), (11, 100, 127), (12, 151, 128), (15, 250, 129), (16, 61, 130), (19, 100, 63), (20, 151, 64), (23, 250, 65),
              (24, 100, 127), (30, 151, 128), (31, 250, 129), (4, 20, 130), (3, 20, 65), (8, 100, 1), (8, 100, 2), (8, 100, 3), (12, 151, 1)]


def _case(name, scoring, k, L, n, genome="env", packed16=True):
    """packed16: whether run_align is to take the 16-bit form for this case when it may choose (packed16_by_the_guard must agree)"""
    return dict(name=name, scoring=scoring, k=k, L=L, n=n, genome=genome, packed16=packed16)


CASES = [_case("k%d_L%d_n%d" % (k, L, n), "defaults", k, L, n) for k, L, n in BAND_CASES]
CASES += [_case("batch1500", "defaults", 8, 100, 1500), _case("L998_k31", "defaults", 31, 998, 65)]
CASES += [_case(s, s, 8, 100, 130, packed16=s not in ("gap_ext255", "gap_ext256"))
          for s in ("gap_open0", "gap_ext255", "gap_ext256", "tie", "np0", "np_big", "flat", "inverted", "phred64")]
CASES += [_case("tie_k12_L151", "tie", 12, 151, 130), _case("defaults_k8_L100", "defaults", 8, 100, 130)]
# gaps cheaper than most mismatches: where a gap at the very end of a read really comes out as a gap (leading / trailing I)
CASES += [_case("gap_open0_n840", "gap_open0", 8, 100, 840)]
CASES += [_case("maxpen12_L935", "maxpen12", 18, 935, 64), _case("maxpen12_L936", "maxpen12", 18, 936, 64, packed16=False)]
CASES += [_case("inverted60_L998", "inverted60", 31, 998, 128, packed16=False), _case("inverted40000", "inverted40000", 8, 100, 64, packed16=False)]
CASES += [_case("hp_defaults", "defaults", 8, 100, 64, genome="hp"), _case("hp_tie", "tie", 8, 100, 64, genome="hp"),
          _case("hp_gap_open0", "gap_open0", 8, 100, 64, genome="hp")]
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
N_EXACT = 4          # jobs with err == 0 appended to every case
MAX_UNGAPPED = 16    # jobs with err > 0 that the un-gapped exit settles, at most, per case


def packed16_by_the_guard(scoring, L):
    """the condition of run_align for the 16-bit form, once BMBS_SW=reg2 asks for it and the batch has one read length"""
    import align_spec
    p = dict(mp_max=6, mp_min=2, np=1, gap_open=5, gap_ext=3, q_base=33)
    p.update(SCORING[scoring])
    pen = align_spec.mismatch_penalty(p["mp_max"], p["mp_min"], p["q_base"], np.arange(256))
    maxpen = max(int(pen.max()), -int(pen.min()), p["np"], p["gap_open"] + p["gap_ext"])
    return p["gap_ext"] < 256 and (L + 64) * maxpen < 12000 and min(p["mp_min"], p["gap_ext"], p["gap_open"], p["np"]) >= 0


def needs_dp(w, read, err, end):
    """whether the job reaches the DP: err > 0 and try_cigar_without_path (ksw.cpp:2515) does not settle it"""
    L = read.size
    start = end - L + 1
    if err == 0:
        return False
    if start < 0:
        return True
    pat = w[start:start + L]
    return int(((read != pat) & ~((read == T) & (pat == C_))).sum()) != err


def build_jobs(case, oix):
    """-> dict(seq[n, stride], qual[n, stride], site[n] u64, err[n] u32, end[n] i32, windows[n, L + 2k], pattern[n] (names),
    forward[n] bool, accepted[n] bool, dp[n] bool).  The patterns take turns until case["n"] jobs reach the DP; jobs that the
    un-gapped exit settles are kept too, up to MAX_UNGAPPED; a pattern that has not reached the DP in four turns running (at k = 1
    only a gap in the middle of the read does) takes no further turn."""
    L, k, G = case["L"], case["k"], oix.G
    rng = np.random.default_rng(zlib.crc32(case["name"].encode()))
    hp = case["genome"] == "hp"
    names = list(HP_PATTERNS) if hp else [p for p in pattern_names(L, k) if p != "exact"]
    q_base = SCORING[case["scoring"]].get("q_base", 33)
    stride = (L + 15) // 16 * 16
    rows = []          # (pattern, site, window, read, qual, err, end, dp)

    def make(pat, fwd, turn):
        for _ in range(50):
            if hp or pat == "exact":
                s, script = _hp_job(pat, L, k, G, fwd, rng) if hp else (int(rng.integers(2000, G - 5000)) + (0 if fwd else G), [("M", L)])
                w = oix.window(s, L + 2 * k)
            else:
                s = int(rng.integers(2000, G - 5000)) + (0 if fwd else G)
                w = oix.window(s, L + 2 * k)
                script = script_for(pat, L, k, w, rng, turn)
            if script is not None:
                break
        assert script is not None, (case["name"], pat)
        read = render(script, w, k, L, rng)
        if case["scoring"] in QUAL_AT_BASE:
            q = np.full(L, q_base, dtype=np.uint8)
        elif case["scoring"] == "phred64":          # '!' .. '%': 27 .. 31 below q_base, where the penalty formula gives -1 and 0
            q = rng.integers(33, 38, L).astype(np.uint8)
        else:
            q = rng.integers(33, 75, L).astype(np.uint8)
            if pat in END_GAPS:                     # a mismatch at either end is dear, so that a cheap gap is worth taking there
                q[:2] = 74; q[L - 2:] = 74
        e, en = orc.bpm(w, read, k)
        return (pat, s, w, read, q, e, en, needs_dp(w, read, e, en))

    turn = {p: 0 for p in names}
    barren = {p: 0 for p in names}
    n_dp = n_ungapped = at = 0
    while n_dp < case["n"]:
        assert any(barren[p] < 4 for p in names), (case["name"], "no pattern reaches the DP")
        idx = at % len(names); at += 1
        pat = names[idx]
        if barren[pat] >= 4:
            continue
        t = turn[pat]; turn[pat] += 1
        row = make(pat, (idx + t) % 2 == 0, t)          # strands alternate per pattern
        if row[-1]:
            rows.append(row); n_dp += 1; barren[pat] = 0
        else:
            barren[pat] += 1
            if n_ungapped < MAX_UNGAPPED:
                rows.append(row); n_ungapped += 1
    rows += [make("exact", j % 2 == 0, 0) for j in range(N_EXACT)]
    n = len(rows)
    seq = np.zeros((n, stride), dtype=np.uint8); qual = np.zeros((n, stride), dtype=np.uint8)
    for j, r in enumerate(rows):
        seq[j, :L] = r[3]; qual[j, :L] = r[4]
    site = np.array([r[1] for r in rows], dtype=np.uint64)
    err = np.array([r[5] for r in rows], dtype=np.uint32)
    return dict(seq=seq, qual=qual, site=site, err=err, end=np.array([r[6] for r in rows], dtype=np.int32),
                windows=np.array([r[2] for r in rows], dtype=np.uint8), pattern=[r[0] for r in rows],
                forward=site < np.uint64(G), accepted=err <= np.uint32(k), dp=np.array([r[7] for r in rows], dtype=bool))


def _hp_job(pat, L, k, G, fwd, rng):
    """a site whose window carries a planted run of twelve A at read bases 40 .. 51, and the script that puts one more A (hp_ins) or
    one fewer (hp_del) into the run"""
    # planted at p = 1000, 2000, ...: A at the odd thousands, T at the even ones -- twelve A on the reverse strand, the last of them
    # at doubled-genome coordinate 2G - 1 - p
    t = 2 * int(rng.integers(1, (G - 4000) // 2000))
    if fwd:
        run_at = 1000 * (t - 1)
    else:
        run_at = 2 * G - 1 - (1000 * t + HP_RUN - 1)
    s = run_at - k - 40
    if pat == "exact":
        return s, [("M", L)]
    if pat == "hp_ins":          # the read has thirteen A where the window has twelve
        return s, [("M", 46), ("A", 1), ("M", L - 47)]
    return s, [("M", 46), ("D", 1), ("M", L - 46)]


def reference_results(case, jobs, reverse_quality=None):
    """orc.align on every job -> list of dicts"""
    L, k = case["L"], case["k"]
    prm = orc.params(**params_of(case["scoring"], L, k))
    out = []
    for j in range(len(jobs["pattern"])):
        rq = 0 if reverse_quality is None else int(reverse_quality[j])
        out.append(orc.align(prm, jobs["windows"][j], jobs["seq"][j, :L], jobs["qual"][j, :L], k, int(jobs["end"][j]), int(jobs["err"][j]),
                             int(jobs["forward"][j]), rq))
    return out
