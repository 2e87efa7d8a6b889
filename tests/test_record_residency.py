"""What the record stages leave on the device, and which later call takes it away (bmbs_records.hip; Lane::ends in bmbs_host.h).

A sorted text call, bmbs_bam_sort and the methyl calls each leave results behind that a later "fetch" call hands out:
bmbs_text_sorted_index / _dup / _clip, bmbs_bam_sort_index, bmbs_bam_sort_methyl, bmbs_methyl_sites, bmbs_methyl_mbias.  Any call that
rewrites a buffer such a result lives in has to end it: the fetch then answers BMBS_ESTATE instead of another call's bytes.  RULES below
is that contract as data; the one test runs every ordered pair of makers on one context and asks every fetch afterwards.  A fetch either
answers BMBS_ESTATE or exactly the bytes it gave directly after the call it describes (every call here is deterministic, so those
bytes are taken once, SNAPSHOTS, each maker on its own).

The three fetches that compute when asked (index pieces, signatures, clips) go through the size query first (cap 0, BMBS_ENOMEM with the
counts) and then the real call, as the mapper's wrappers do; every pair runs once without and once with a round of fetches between the
two makers, so that what a fetch keeps for the call behind its size query (bai_done, dup_done) is covered as well."""
import numpy as np
import pytest

from test_sorted_bam import split_records

pytestmark = pytest.mark.gpu

N_PAIRS = 64
# (bmbs_bam_sort_methyl is a methyl call of its own: asked last, behind the fetches of the methyl results it replaces)
FETCHES = ("index", "dup", "clip", "bai", "sites", "mbias", "sort_methyl")

NEW, KEEP, DEAD = "new", "keep", "dead"
# maker -> what each fetch answers after it: NEW this call's result, KEEP what it answered before, DEAD BMBS_ESTATE; and why
RULES = {
    "text_sorted": {
        "index": (NEW, "a sorted text call rewrites bs_key2 / bs_slen"),
        "dup": (NEW, "a sorted text call rewrites bam_raw / sam_off / sam_len / bs_idx2"),
        "clip": (NEW, "a sorted text call rewrites bam_raw / sam_off / sam_len / bs_idx2"),
        "bai": (DEAD, "the sort of a text call rewrites bs_sorted / bs_soff"),
        "sort_methyl": (DEAD, "the sort of a text call ends what the last bmbs_bam_sort left, as for its index (sc.in itself stays)"),
        "sites": (KEEP, "a text call rewrites no methyl buffer"),
        "mbias": (KEEP, "a text call rewrites no methyl buffer"),
    },
    "text_bam": {
        "index": (KEEP, "a plain BAM call rewrites no sort buffer"),
        "dup": (DEAD, "a text call rewrites bam_raw / sam_off / sam_len"),
        "clip": (DEAD, "a text call rewrites bam_raw / sam_off / sam_len"),
        "bai": (DEAD, "the deflater rewrites bam_off"),
        "sort_methyl": (KEEP, "a plain BAM call rewrites no sc.in"),
        "sites": (KEEP, "a text call rewrites no methyl buffer"),
        "mbias": (KEEP, "a text call rewrites no methyl buffer"),
    },
    "text_sam": {
        "index": (KEEP, "a SAM call rewrites no sort buffer"),
        "dup": (DEAD, "a text call rewrites sam_off / sam_len"),
        "clip": (DEAD, "a text call rewrites sam_off / sam_len"),
        "bai": (KEEP, "a SAM call rewrites no bs_sorted / bs_soff / bam_off: neither the sort nor the deflater runs"),
        "sort_methyl": (KEEP, "a SAM call rewrites no sc.in"),
        "sites": (KEEP, "a text call rewrites no methyl buffer"),
        "mbias": (KEEP, "a text call rewrites no methyl buffer"),
    },
    "sort_bgzf": {
        "index": (DEAD, "bmbs_bam_sort rewrites bs_key2 / bs_slen"),
        "dup": (DEAD, "bmbs_bam_sort rewrites bs_idx2"),
        "clip": (DEAD, "bmbs_bam_sort rewrites bs_idx2"),
        "bai": (NEW, "bmbs_bam_sort rewrites bs_sorted / bs_soff / bam_off"),
        "sort_methyl": (NEW, "bmbs_bam_sort rewrites sc.in"),
        "sites": (KEEP, "bmbs_bam_sort rewrites no methyl buffer"),
        "mbias": (KEEP, "bmbs_bam_sort rewrites no methyl buffer"),
    },
    "sort_raw": {
        "index": (DEAD, "bmbs_bam_sort rewrites bs_key2 / bs_slen"),
        "dup": (DEAD, "bmbs_bam_sort rewrites bs_idx2"),
        "clip": (DEAD, "bmbs_bam_sort rewrites bs_idx2"),
        "bai": (DEAD, "bmbs_bam_sort rewrites bs_sorted / bs_soff, and a RAW call makes no blocks to index"),
        "sort_methyl": (NEW, "bmbs_bam_sort rewrites sc.in"),
        "sites": (KEEP, "bmbs_bam_sort rewrites no methyl buffer"),
        "mbias": (KEEP, "bmbs_bam_sort rewrites no methyl buffer"),
    },
    "sort_refused_on_host": {      # a length below 36: refused by the argument checks
        "index": (KEEP, "a bmbs_bam_sort refused by its argument checks rewrites no buffer"),
        "dup": (KEEP, "a bmbs_bam_sort refused by its argument checks rewrites no buffer"),
        "clip": (KEEP, "a bmbs_bam_sort refused by its argument checks rewrites no buffer"),
        "bai": (DEAD, "bmbs_bam_sort_index describes the LAST bmbs_bam_sort call, and that failed"),
        "sort_methyl": (DEAD, "bmbs_bam_sort_methyl reads the LAST bmbs_bam_sort call's records, and that failed"),
        "sites": (KEEP, "bmbs_bam_sort rewrites no methyl buffer"),
        "mbias": (KEEP, "bmbs_bam_sort rewrites no methyl buffer"),
    },
    "sort_refused_on_device": {    # a length that is not the record's block_size + 4: found by the key kernel
        "index": (DEAD, "bmbs_bam_sort rewrites bs_key / bs_idx before the device refuses the length"),
        "dup": (DEAD, "bmbs_bam_sort rewrites bs_key / bs_idx before the device refuses the length"),
        "clip": (DEAD, "bmbs_bam_sort rewrites bs_key / bs_idx before the device refuses the length"),
        "bai": (DEAD, "bmbs_bam_sort_index describes the LAST bmbs_bam_sort call, and that failed"),
        "sort_methyl": (DEAD, "bmbs_bam_sort rewrites sc.in, and the call failed"),
        "sites": (KEEP, "bmbs_bam_sort rewrites no methyl buffer"),
        "mbias": (KEEP, "bmbs_bam_sort rewrites no methyl buffer"),
    },
    "dup_sigs": {
        "index": (KEEP, "bmbs_bam_dup_sigs rewrites dp_in / dp_sig only"),
        "dup": (KEEP, "bmbs_bam_dup_sigs rewrites dp_sig: the sorted call's signatures are computed again from bam_raw, which stays"),
        "clip": (KEEP, "bmbs_bam_dup_sigs rewrites dp_in / dp_sig only"),
        "bai": (KEEP, "bmbs_bam_dup_sigs rewrites dp_in / dp_sig only"),
        "sort_methyl": (KEEP, "bmbs_bam_dup_sigs rewrites dp_in / dp_sig only"),
        "sites": (KEEP, "bmbs_bam_dup_sigs rewrites dp_in / dp_sig only"),
        "mbias": (KEEP, "bmbs_bam_dup_sigs rewrites dp_in / dp_sig only"),
    },
    "dup_select": {
        "index": (KEEP, "bmbs_dup_select rewrites dp_sig, its keys and bs_tmp only"),
        "dup": (KEEP, "bmbs_dup_select rewrites dp_sig: the sorted call's signatures are computed again from bam_raw, which stays"),
        "clip": (KEEP, "bmbs_dup_select rewrites dp_sig, its keys and bs_tmp only"),
        "bai": (KEEP, "bmbs_dup_select rewrites dp_sig, its keys and bs_tmp only (bs_tmp holds nothing between calls)"),
        "sort_methyl": (KEEP, "bmbs_dup_select rewrites dp_sig, its keys and bs_tmp only"),
        "sites": (KEEP, "bmbs_dup_select rewrites dp_sig, its keys and bs_tmp only"),
        "mbias": (KEEP, "bmbs_dup_select rewrites dp_sig, its keys and bs_tmp only"),
    },
    "methyl_mbias": {
        "index": (KEEP, "bmbs_bam_methyl_opts rewrites methyl buffers and bs_tmp only"),
        "dup": (KEEP, "bmbs_bam_methyl_opts rewrites methyl buffers and bs_tmp only"),
        "clip": (KEEP, "bmbs_bam_methyl_opts rewrites methyl buffers (mt_cl2 is written by the clip fetch itself) and bs_tmp only"),
        "bai": (KEEP, "bmbs_bam_methyl_opts rewrites methyl buffers and bs_tmp only"),
        "sort_methyl": (KEEP, "bmbs_bam_methyl_opts rewrites mt_in, not sc.in"),
        "sites": (NEW, "bmbs_bam_methyl_opts rewrites mt_site"),
        "mbias": (NEW, "bmbs_bam_methyl_opts with BMBS_METHYL_MBIAS rewrites mt_mbias"),
    },
    "methyl_plain": {
        "index": (KEEP, "bmbs_bam_methyl_opts rewrites methyl buffers and bs_tmp only"),
        "dup": (KEEP, "bmbs_bam_methyl_opts rewrites methyl buffers and bs_tmp only"),
        "clip": (KEEP, "bmbs_bam_methyl_opts rewrites methyl buffers (mt_cl2 is written by the clip fetch itself) and bs_tmp only"),
        "bai": (KEEP, "bmbs_bam_methyl_opts rewrites methyl buffers and bs_tmp only"),
        "sort_methyl": (KEEP, "bmbs_bam_methyl_opts rewrites mt_in, not sc.in"),
        "sites": (NEW, "bmbs_bam_methyl_opts rewrites mt_site"),
        "mbias": (DEAD, "the table describes the LAST methyl call, and that one did not ask for it (mt_mbias itself stays)"),
    },
    # (refused with BMBS_ESTATE itself when bmbs_bam_sort's records are not resident: "sites" is then DEAD, not NEW)
    "sort_methyl": {
        "index": (KEEP, "bmbs_bam_sort_methyl rewrites methyl buffers and bs_tmp only"),
        "dup": (KEEP, "bmbs_bam_sort_methyl rewrites methyl buffers and bs_tmp only"),
        "clip": (KEEP, "bmbs_bam_sort_methyl rewrites methyl buffers and bs_tmp only"),
        "bai": (KEEP, "bmbs_bam_sort_methyl rewrites methyl buffers and bs_tmp only"),
        "sort_methyl": (KEEP, "bmbs_bam_sort_methyl reads sc.in and rewrites none of them"),
        "sites": (NEW, "bmbs_bam_sort_methyl rewrites mt_site; refused, it still ends the last methyl call's result"),
        "mbias": (DEAD, "the table describes the LAST methyl call, and that one did not ask for it"),
    },
}
MAKERS = tuple(RULES)
# the calls whose refusal is the case, with the code they answer
REFUSED = {"sort_refused_on_host": -22, "sort_refused_on_device": -22}
ESTATE = -1


def _rc_of(call):
    """0, or the code of the `bmbs error <code>: ...` the mapper raised"""
    try:
        call()
    except RuntimeError as e:
        assert str(e).startswith("bmbs error "), e
        return int(str(e).split()[2].rstrip(":"))
    return 0


def _fetch(m, f):
    """the bytes fetch `f` answers, None for BMBS_ESTATE; index / dup / clip / bai / sites / mbias ask for the sizes first (cap 0)"""
    def cat(x):
        return b"|".join(np.ascontiguousarray(a).tobytes() for a in (x if isinstance(x, tuple) else (x,)))
    call = {"index": m.sorted_index, "dup": m.sorted_dup, "clip": m.sorted_clip, "sites": m.methyl_sites, "mbias": m.methyl_mbias,
            "bai": lambda: (lambda r: r[:3] + (np.uint64(r[3]),))(m.bam_sort_index()),
            "sort_methyl": lambda: m.bam_sort_methyl(None, contexts=7)}[f]
    try:
        return cat(call())
    except RuntimeError as e:
        assert str(e).startswith("bmbs error %d:" % ESTATE), (f, e)
        return None


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    """a genome of two sequences, 30 kb in all, its index, 64 pairs and the records they map to"""
    from bitmapperbs_amd import mapper, synth
    wd = tmp_path_factory.mktemp("residency")
    names, chroms = synth.make_genome(30_000, 2, seed=1201)
    fa = str(wd / "g.fa")
    synth.write_fasta(fa, names, chroms)
    mapper.Index.build(fa, fa, threads=4)
    m1, m2 = synth.make_reads_pe(chroms, n=N_PAIRS, L=100, seed=1202, sub=0.01, indel=0.0, qual="random")
    fq = [b"".join(b"@" + mm["names"][i] + b"\n" + mm["seq"][i].tobytes() + b"\n+\n" + mm["qual"][i].tobytes() + b"\n" for i in range(N_PAIRS)) for mm in (m1, m2)]
    ix = mapper.Index(fa)
    m = mapper.Mapper(ix, 0)
    M = mapper.Mapper
    # the 128 records in input order (every line prints: TEXT_UNMAPPED), as the plain BAM call's blocks hold them
    from common import bgzf_blocks
    recs = split_records(b"".join(raw for _, raw in bgzf_blocks(m.map_text(fq[0], N_PAIRS, fq[1], flags=M.TEXT_BAM | M.TEXT_UNMAPPED))))
    assert len(recs) == 2 * N_PAIRS
    yield dict(m=m, fq=fq, recs=recs)
    m.close()
    ix.close()


def _makers(env):
    """maker -> a call without arguments.  Each works on records of its own, so that no two leave the same bytes behind"""
    m, fq, recs = env["m"], env["fq"], env["recs"]
    M = type(m)

    def lens(rs):
        return np.array([len(r) for r in rs], dtype=np.uint32)

    def text(flags):
        return lambda: m.map_text(fq[0], N_PAIRS, fq[1], flags=flags | M.TEXT_UNMAPPED)

    def sort(rs, ln=None, raw=False):
        return lambda: m.bam_sort(b"".join(rs), lens(rs) if ln is None else ln, raw=raw)
    raw_recs, short, swapped = recs[::-1][:96], lens(recs), lens(recs)
    short[41] = 35; short[42] += len(recs[41]) - 35                 # (the lengths still add up)
    swapped[41] += 4; swapped[42] -= 4
    sigs = m.dup_sigs(b"".join(recs), lens(recs), paired=True)
    return {
        "text_sorted": text(M.TEXT_BAM | M.TEXT_BAM_SORTED),
        "text_bam": text(M.TEXT_BAM),
        "text_sam": text(0),
        "sort_bgzf": sort(recs),
        "sort_raw": sort(raw_recs, raw=True),
        "sort_refused_on_host": sort(recs, short),
        "sort_refused_on_device": sort(recs, swapped),
        "dup_sigs": lambda: m.dup_sigs(b"".join(recs[:64]), lens(recs[:64]), paired=True),
        "dup_select": lambda: m.dup_select(sigs[::-1]),
        "methyl_mbias": lambda: m.bam_methyl(b"".join(recs[:120]), lens(recs[:120]), None, contexts=7, mbias=True),
        "methyl_plain": lambda: m.bam_methyl(b"".join(recs[:80]), lens(recs[:80]), None, contexts=3, ignore_5p=(1, 0)),     # (a trim: the _opts call, flags 0)
        "sort_methyl": lambda: m.bam_sort_methyl(None, contexts=1),
    }


def test_every_fetch_after_every_pair_of_makers(env):
    m = env["m"]
    makers = _makers(env)
    assert set(makers) == set(MAKERS) and all(set(RULES[k]) == set(FETCHES) for k in MAKERS)

    # ---- each maker on its own, every fetch directly behind it: the bytes its NEW results are.  bmbs_bam_sort_methyl as a maker gives
    # other sites for either resident call's records
    SNAPSHOTS = {}
    for k in MAKERS:
        if k == "sort_methyl":
            continue
        assert _rc_of(makers[k]) == REFUSED.get(k, 0), k
        SNAPSHOTS[k] = {f: _fetch(m, f) for f in FETCHES}
        for f in FETCHES:
            if RULES[k][f][0] == NEW:
                assert SNAPSHOTS[k][f] is not None and len(SNAPSHOTS[k][f]) > 64, (k, f)
            if RULES[k][f][0] == DEAD:
                assert SNAPSHOTS[k][f] is None, (k, f, RULES[k][f][1])
    for k in ("sort_bgzf", "sort_raw"):
        assert _rc_of(makers[k]) == 0 and _rc_of(makers["sort_methyl"]) == 0
        SNAPSHOTS["sort_methyl", k] = _fetch(m, "sites")
    # no two makers of a result leave the same bytes: a stale result cannot pass for the right one
    for f in FETCHES:
        made = [SNAPSHOTS[k][f] for k in MAKERS if k != "sort_methyl" and RULES[k][f][0] == NEW]
        if f == "sites":
            made += [SNAPSHOTS["sort_bgzf"]["sort_methyl"], SNAPSHOTS["sort_raw"]["sort_methyl"], SNAPSHOTS["sort_methyl", "sort_bgzf"], SNAPSHOTS["sort_methyl", "sort_raw"]]
        assert len(set(made)) == len(made), f

    # ---- the model: what each fetch has to answer now (None: BMBS_ESTATE), and whose records bmbs_bam_sort left.  It starts with
    # nothing resident: a sort the device refuses and a bmbs_bam_sort_methyl that finds no records end every result there is
    assert _rc_of(makers["sort_refused_on_device"]) == -22 and _rc_of(makers["sort_methyl"]) == ESTATE
    want = {f: None for f in FETCHES}
    resident = [None]

    def make(k):
        rc = _rc_of(makers[k])
        if k == "sort_methyl":
            assert rc == (0 if resident[0] else ESTATE), (k, rc)
        else:
            assert rc == REFUSED.get(k, 0), (k, rc)
        for f in FETCHES:
            how = RULES[k][f][0]
            if how == DEAD or (k == "sort_methyl" and f == "sites" and not resident[0]):
                want[f] = None
            elif how == NEW:
                want[f] = SNAPSHOTS["sort_methyl", resident[0]] if k == "sort_methyl" else SNAPSHOTS[k][f]
        if RULES[k]["sort_methyl"][0] != KEEP:
            resident[0] = k if RULES[k]["sort_methyl"][0] == NEW else None

    def fetch_all(trail):
        for f in FETCHES:
            got = _fetch(m, f)
            assert (got is None) == (want[f] is None), (trail, f, "BMBS_ESTATE" if got is None else "an answer", [RULES[k][f] for k in trail[-2:]])
            assert got == want[f], (trail, f, [RULES[k][f] for k in trail[-2:]])
            if f == "sort_methyl":
                # as a fetch it is a methyl call of its own: its sites are the last call's now, and it asked for no table
                want["sites"] = got
                want["mbias"] = None

    n_estate = n_same = 0
    for between in (False, True):
        for a in MAKERS:
            for b in MAKERS:
                make(a)
                if between:
                    fetch_all((a,))
                make(b)
                fetch_all((a, b))
                n_estate += sum(1 for f in FETCHES if want[f] is None)
                n_same += sum(1 for f in FETCHES if want[f] is not None)
    assert n_estate > 100 and n_same > 100
