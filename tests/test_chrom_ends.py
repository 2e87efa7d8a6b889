"""Reads and pairs at and across chromosome ends (tests/ends.py): the off-end rejection (status 3) on every exit path of the
single-end kernels (k_finalize: verdicts 1, 2, 3 and the exact-ambiguous loop of verdict 4), of the paired-end kernels (k_finalize_pe,
the exit-A/C settling of the fast path), in the SAM / BAM text kernels and in the record stages behind them.

First, without a GPU: the inputs do what they are for -- conditions on the ORACLE's records, which tests/test_oracle.py pins to the
reference's own output for the same reads (ends_* goldens).  Then, -m gpu: the device against the oracle, record by record and status by
status, and against the reference's SAM / BAM byte for byte."""
import gzip
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import ends
import orc
from common import GOLD, ROOT, bam_payload, gunzip_to, trim_fastq

gpu = pytest.mark.gpu
L = ends.L


# ---- the oracle's records of every set, computed once ---------------------------------------------------------------------------------------
class _Ref:
    """genome WITH plant (ii), oracle-built index, and the oracle's records of each read set under each parameter set (made on first use)"""
    def __init__(self, wd, n_ctg=20, ends_used=None, pe_ends=None):
        self.wd = str(wd)
        self.names, self.chroms = ends.genome(plant_ii=True, n_ctg=n_ctg)
        self.clen = np.array([c.size for c in self.chroms], dtype=np.int64)
        self.fa = os.path.join(self.wd, "genome.fa")
        ends.write_fasta(self.fa, self.names, self.chroms)
        assert orc.load().orc_index_build(self.fa.encode(), self.fa.encode()) == 0
        self.oix = orc.OrcIndex(self.fa)
        self.se = ends.se_reads(self.chroms, plant_ii=True, ends=ends_used)
        self.m1, self.m2, self.pe_meta = ends.pe_reads(self.chroms, ends=pe_ends)
        self._made = {}

    def trimmed(self, which):
        """the set as an adapter trimmer leaves it (common.trim_fastq, the seeds of the ends_*_trim goldens) -> seq, qual, lens"""
        key = ("trim", which)
        if key not in self._made:
            reads, seed = {"se": (self.se, 21), "pe1": (self.m1, 22), "pe2": (self.m2, 23)}[which]
            src = os.path.join(self.wd, which + ".fq")
            ends.write_fastq(src, reads); trim_fastq(src, src + ".trim", seed)
            self._made[key] = ends.read_fastq_var(src + ".trim")[1:]
        return self._made[key]

    def se_recs(self, amb=0, trim=False):
        key = ("se", amb, trim)
        if key not in self._made:
            if trim:
                s, q, ln = self.trimmed("se")
                self._made[key] = self.oix.map_se_var(orc.params(ambiguous_out=amb), s, q, ln)[:2]
            else:
                self._made[key] = self.oix.map_se(orc.params(ambiguous_out=amb), self.se["seq"], self.se["qual"], L)[:2]
        return self._made[key]

    def pe_recs(self, trim=False, **prm):
        key = ("pe", trim, tuple(sorted(prm.items())))
        if key not in self._made:
            if trim:
                (s1, q1, l1), (s2, q2, l2) = self.trimmed("pe1"), self.trimmed("pe2")
                self._made[key] = self.oix.map_pe_var(orc.params(**prm), s1, q1, s2, q2, l1, l2)[:2]
            else:
                self._made[key] = self.oix.map_pe(orc.params(**prm), self.m1["seq"], self.m1["qual"], self.m2["seq"], self.m2["qual"], L)[:2]
        return self._made[key]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return _Ref(tmp_path_factory.mktemp("ends_ref"))


PE_MODES = {"fast": {}, "sensitive": dict(sensitive=1), "ambiguous_out": dict(ambiguous_out=1),
            "minmax": dict(min_ins=ends.PE_MIN, max_ins=ends.PE_MAX)}


def _ops(cigar):
    return [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNS])", cigar.decode())]


def _span(cigar):
    return sum(n for n, op in _ops(cigar) if op in "MD")


def _indel_near_end(rec, clen, within=5):
    """an I or D of the alignment lies within `within` bases of its chromosome's first or last base"""
    at = int(rec["pos"])
    for n, op in _ops(rec["cigar"]):
        if op in "ID" and (at - 1 <= within or clen - (at + (n - 1 if op == "D" else 0)) <= within):
            return True
        if op in "MD":
            at += n
    return False


# ---- without a GPU: the inputs do what they are for ----------------------------------------------------------------------------------------------
def test_single_end_inputs_reach_every_exit_with_and_without_rejection(ref):
    recs, _ = ref.se_recs(0)
    st, path = recs["status"], recs["path"]
    for p in (1, 2, 3):
        assert int(((st == 3) & (path == p)).sum()) >= 50, p
    mapped = np.nonzero(st == 1)[0]
    touching = [i for i in mapped if int(recs[i]["pos"]) == 1 or int(recs[i]["pos"]) + _span(recs[i]["cigar"]) - 1 == ref.clen[recs[i]["chrom"]]]
    assert len(touching) >= 50
    indel = np.array([b"I" in c or b"D" in c for c in recs["cigar"]])
    assert int(((st == 3) & indel).sum()) >= 20
    assert sum(1 for i in mapped if indel[i] and _indel_near_end(recs[i], ref.clen[recs[i]["chrom"]])) >= 20


def test_the_exact_read_on_the_last_base_maps_and_one_base_further_is_rejected(ref):
    """for every end and both strands.  Three kinds of end cannot do both and are held to what they do instead: a sequence shorter
    than the read (the read ending on its last base starts in the sequence before: rejected); chr2, whose last 100 bases are plant
    (iii)'s second copy (that read has two hits); and the last sequence, whose end is the seam of the doubled text and no join of
    two sequences -- the reference fetches no genome window across it, so a read across the seam is unmapped unless its first seed
    alone settles it (then it is rejected like any other)."""
    recs, _ = ref.se_recs(0)
    m = ref.se["meta"]
    nc = len(ref.chroms)
    seen = 0
    for i in np.nonzero((m["kind"] == "end") & (m["form"] == "exact") & ((m["over"] == 0) | (m["over"] == 1)))[0]:
        c, over, st = int(m[i]["chrom"]), int(m[i]["over"]), int(recs[i]["status"])
        seen += 1
        if over == 0:
            want = (3,) if ref.clen[c] < L else (2,) if c == 1 else (1,)
        else:
            want = (0, 3) if c == nc - 1 else (3,)
        assert st in want, (ref.names[c], bool(m[i]["minus"]), over, st)
        if st == 1:
            assert int(recs[i]["chrom"]) == c and int(recs[i]["pos"]) == ref.clen[c] - L + 1
    assert seen == 4 * nc


def test_the_plants_are_ambiguous_where_a_copy_lies_inside_and_unmapped_where_none_does(ref):
    m = ref.se["meta"]
    plain, _ = ref.se_recs(0)
    amb, _ = ref.se_recs(1)
    nc = len(ref.chroms)
    for kind, inside in (("plant1", (nc - 2, 10001)), ("plant3", None)):
        w = np.nonzero(m["kind"] == kind)[0]
        assert w.size == 4
        assert (plain["status"][w] == 2).all() and (amb["status"][w] == 2).all()
        if inside:          # the exact-ambiguous loop skips the row across the chr1|chr2 join, in whichever order the rows come
            assert (plain["path"][w] == 4).all()
            assert [(int(r["chrom"]), int(r["pos"])) for r in amb[w]] == [inside] * 4
        else:               # both copies lie inside; the one against chr2's last base touches it
            assert {(int(r["chrom"]), int(r["pos"])) for r in amb[w]} == {(1, int(ref.clen[1]) - L + 1), (nc - 1, 5001)}
    # plant (ii): both hits lie across an end.  Without --ambiguous_out the read is ambiguous; with it, the loop finds no row to
    # print and the read counts as unmapped (tests/ends.py says why the reference's own output cannot be pinned here)
    w = np.nonzero(m["kind"] == "plant2")[0]
    assert w.size == 8
    assert (plain["status"][w] == 2).all() and (plain["path"][w] == 4).all()
    assert (amb["status"][w] == 3).all() and (amb["path"][w] == 4).all()


def test_the_golden_inputs_hold_no_read_of_plant_two(tmp_path):
    """the reads the reference's output is pinned for never leave output_ambiguous_exact_map's loop without a placement"""
    names, chroms = ends.genome()
    fa = str(tmp_path / "genome.fa")
    ends.write_fasta(fa, names, chroms)
    assert gzip.open(os.path.join(GOLD, "ends_genome.fa.gz"), "rb").read() == open(fa, "rb").read()
    assert orc.load().orc_index_build(fa.encode(), fa.encode()) == 0
    oix = orc.OrcIndex(fa)
    r = ends.se_reads(chroms)
    fq = str(tmp_path / "se.fq")
    ends.write_fastq(fq, r)
    assert gzip.open(os.path.join(GOLD, "ends_se.fq.gz"), "rb").read() == open(fq, "rb").read()
    trim_fastq(fq, fq + ".trim", 21)
    _, s, q, ln = ends.read_fastq_var(fq + ".trim")
    for recs in (oix.map_se(orc.params(ambiguous_out=1), r["seq"], r["qual"], L)[0], oix.map_se_var(orc.params(ambiguous_out=1), s, q, ln)[0]):
        assert (recs["path"] == 4).sum() >= 4 and not ((recs["path"] == 4) & (recs["status"] != 2)).any()
    oix.close()


def test_no_read_sits_where_the_chromosome_lookup_is_undefined(ref):
    for amb in (0, 1):
        for trim in (False, True):
            assert ends.seam_state(ref.se_recs(amb, trim)[0], ref.oix.G).size == 0


def test_paired_inputs_cross_ends_both_ways_and_meet_both_insert_bounds(ref):
    meta = ref.pe_meta
    for mode in ("fast", "sensitive", "ambiguous_out"):
        recs, _ = ref.pe_recs(**PE_MODES[mode])
        assert int((recs["status"] == 3).sum()) >= 200, mode
        assert int(((recs["status"] == 1) & (recs["chrom1"] != recs["chrom2"])).sum()) >= 200, mode
    recs, _ = ref.pe_recs()
    bounded, _ = ref.pe_recs(**PE_MODES["minmax"])
    b = meta["kind"] == "bound"
    # exact pairs: TLEN is the insert.  Under the default bounds all of them map; under --min 200 --max 300 exactly those within
    assert (recs["status"][b] == 1).all() and (recs["tlen"][b] == meta["insert"][b]).all()
    for tlen in (ends.PE_MIN - 1, ends.PE_MIN, ends.PE_MAX, ends.PE_MAX + 1):
        w = np.nonzero(b & (meta["insert"] == tlen))[0]
        assert w.size >= 1
        inside = ends.PE_MIN <= tlen <= ends.PE_MAX
        assert (bounded["status"][w] == (1 if inside else 3)).all(), tlen
        assert not inside or (bounded["tlen"][w] == tlen).all()
    assert not ((bounded["status"] == 1) & (bounded["chrom1"] != bounded["chrom2"]) & (bounded["tlen"] > ends.PE_MAX)).any()


# ---- -m gpu: the device against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev(ref, tmp_path_factory):
    """the product's own index of the same genome"""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bitmapperbs_amd import mapper
    fa = str(tmp_path_factory.mktemp("ends_dev") / "genome.fa")
    ends.write_fasta(fa, ref.names, ref.chroms)
    mapper.Index.build(fa, fa, threads=4)
    return dict(fa=fa, ix=mapper.Index(fa))


def _se_equal(m, res, pool, want, lens, amb):
    from test_gpu_parity import compare_records
    recs, ost = want
    assert (res["status"].astype(np.int64) == recs["status"].astype(np.int64)).all(), \
        [(int(i), int(res[i]["status"]), int(recs[i]["status"])) for i in np.nonzero(res["status"] != recs["status"])[0][:10]]
    bad = compare_records(res, pool, recs, lens, amb=bool(amb))
    assert not bad, bad[:10]
    assert (m.stats() == ost).all(), (m.stats(), ost)


@gpu
@pytest.mark.parametrize("form", ["default", "legacy", "packed"])
@pytest.mark.parametrize("amb", [0, 1])
def test_map_se_at_chromosome_ends_matches_oracle(ref, dev, monkeypatch, amb, form):
    from bitmapperbs_amd import mapper
    if form == "legacy":
        monkeypatch.setenv("BMBS_LEGACY", "1")
    m = mapper.Mapper(dev["ix"], 0, ambiguous_out=amb)
    seq, qual = ref.se["seq"], ref.se["qual"]
    if form == "packed":
        res, pool = m.map_se_packed(mapper.Mapper.pack_rows(seq, L), qual, L)
    else:
        res, pool = m.map_se(seq, qual, L)
    _se_equal(m, res, pool, ref.se_recs(amb), L, amb)
    m.close()


@gpu
@pytest.mark.parametrize("form", ["default", "legacy", "packed"])
def test_map_se_var_trimmed_reads_at_chromosome_ends_match_oracle(ref, dev, monkeypatch, form):
    from bitmapperbs_amd import mapper
    if form == "legacy":
        monkeypatch.setenv("BMBS_LEGACY", "1")
    s, q, ln = ref.trimmed("se")
    m = mapper.Mapper(dev["ix"], 0, ambiguous_out=1)
    if form == "packed":
        res, pool = m.map_se_packed(mapper.Mapper.pack_rows(s, L, ln), q, L, ln)
    else:
        res, pool = m.map_se_var(s, q, ln)
    _se_equal(m, res, pool, ref.se_recs(1, trim=True), ln, 1)
    m.close()


def _pe_equal(m, res, pool, want, l1, l2=None):
    from test_gpu_parity import compare_pe
    recs, ost = want
    bad = compare_pe(res, pool, recs, l1, l2)
    assert not bad, bad[:5]
    assert (m.stats() == ost).all(), (m.stats(), ost)


@gpu
@pytest.mark.parametrize("mode", sorted(PE_MODES))
def test_map_pe_at_chromosome_ends_matches_oracle(ref, dev, mode):
    from bitmapperbs_amd import mapper
    m = mapper.Mapper(dev["ix"], 0, **PE_MODES[mode])
    res, pool = m.map_pe(ref.m1["seq"], ref.m1["qual"], ref.m2["seq"], ref.m2["qual"], L)
    _pe_equal(m, res, pool, ref.pe_recs(**PE_MODES[mode]), L)
    m.close()


@gpu
@pytest.mark.parametrize("sensitive", [0, 1])
def test_map_pe_var_trimmed_pairs_at_chromosome_ends_match_oracle(ref, dev, sensitive):
    from bitmapperbs_amd import mapper
    (s1, q1, l1), (s2, q2, l2) = ref.trimmed("pe1"), ref.trimmed("pe2")
    m = mapper.Mapper(dev["ix"], 0, sensitive=sensitive)
    res, pool = m.map_pe_var(s1, q1, s2, q2, l1, l2)
    _pe_equal(m, res, pool, ref.pe_recs(trim=True, sensitive=sensitive), l1, l2)
    m.close()


@gpu
def test_ends_with_the_chromosome_table_in_global_memory_match_oracle(tmp_path):
    """the 400-base contigs padded out to 1030 sequences (more than the 1024 the finalize kernels keep in LDS): the same reads and
    pairs at the ends of the first and last sequences and of contigs on both sides of entry 1024"""
    from bitmapperbs_amd import mapper
    n_ctg = 1030
    nc = 2 + n_ctg + 4 + 2
    used = [0, 1, 2, 3, 1020, 1021, 1022, 1023, 1024, 1025, 1026, 1031, 1032, 1035, nc - 2, nc - 1]
    R = _Ref(tmp_path, n_ctg=n_ctg, ends_used=used, pe_ends=[c for c in used if c not in (1032, 1035)])
    assert len(R.chroms) == nc > 1024 and R.clen[1035] == 80
    mapper.Index.build(R.fa, R.fa, threads=4)
    ix = mapper.Index(R.fa)
    m = mapper.Mapper(ix, 0, ambiguous_out=1)
    res, pool = m.map_se(R.se["seq"], R.se["qual"], L)
    want = R.se_recs(1)
    assert int(((want[0]["status"] == 3) & (want[0]["chrom"] >= 1024)).sum()) >= 50
    _se_equal(m, res, pool, want, L, 1)
    m.close()
    for prm in (dict(), dict(sensitive=1)):
        m = mapper.Mapper(ix, 0, **prm)
        res, pool = m.map_pe(R.m1["seq"], R.m1["qual"], R.m2["seq"], R.m2["qual"], L)
        want = R.pe_recs(**prm)
        assert int(((want[0]["status"] == 1) & (want[0]["chrom1"] != want[0]["chrom2"])).sum()) >= 100
        _pe_equal(m, res, pool, want, L)
        m.close()


# ---- -m gpu: SAM / BAM from the device and the driver against the reference's own output -------------------------------------------------------------------
def _runs():
    return json.load(open(os.path.join(GOLD, "ends.json")))


@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    """the golden ends genome (without plant (ii)), the product's index of it"""
    from bitmapperbs_amd import mapper
    fa = str(tmp_path_factory.mktemp("ends_gold") / "genome.fa")
    gunzip_to(os.path.join(GOLD, "ends_genome.fa.gz"), fa)
    mapper.Index.build(fa, fa, threads=4)
    return dict(fa=fa, ix=mapper.Index(fa))


def _params(args):
    from test_oracle import pe_params
    kw = pe_params(args)
    kw["ambiguous_out"] = int("--ambiguous_out" in args)
    return kw


@gpu
@pytest.mark.parametrize("name", sorted(_runs()))
def test_device_text_at_chromosome_ends_equals_the_reference(name, gold, tmp_path):
    """bmbs_map_se_text / bmbs_map_pe_text: the SAM lines (or, --bam, the records inside the BGZF blocks) and the mapstats are the
    reference's"""
    from bitmapperbs_amd import mapper, distributed
    from common import bgzf_blocks
    from test_oracle import ends_inputs
    M = mapper.Mapper
    v = _runs()[name]
    files = ends_inputs(v, tmp_path)[1::2]
    texts = [open(f, "rb").read() for f in files]
    n = texts[0].count(b"\n") // 4
    flags = (M.TEXT_UNMAPPED if "--unmapped_out" in v["args"] else 0) | (M.TEXT_BAM if v.get("bam") else 0)
    m = M(gold["ix"], 0, **_params(v["args"]))
    out = m.map_text(texts[0], n, texts[1] if len(texts) > 1 else None, flags=flags)
    if v.get("bam"):
        assert b"".join(raw for _, raw in bgzf_blocks(out)) == bam_payload(os.path.join(GOLD, "ends_%s.ref.bam" % name))[1]
    else:
        want = "".join(l for l in gzip.open(os.path.join(GOLD, "ends_%s.ref.sam.gz" % name), "rt") if not l.startswith("@"))
        assert out.decode() == want
    assert distributed.mapstats_text(m.stats()) == open(os.path.join(GOLD, "ends_%s.ref.stats" % name)).read()
    m.close()


def _driver():
    p = os.path.join(ROOT, "bitmapperbs_amd", "bmbs_search")
    assert os.path.exists(p), "bmbs_search not built (make -C bitmapperbs_amd/csrc)"
    return p


@gpu
@pytest.mark.parametrize("name", sorted(_runs()))
def test_driver_at_chromosome_ends_equals_the_reference(name, gold, tmp_path):
    from test_oracle import ends_inputs
    v = _runs()[name]
    out = str(tmp_path / "o.out")
    parts = 3 if name == "pe_ua" else 0
    more = ["--out-parts", "3"] if parts else []
    p = subprocess.run([_driver(), "--search", gold["fa"]] + ends_inputs(v, tmp_path) + ["-o", out, "--batch", "700"] + more + v["args"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    if parts:
        open(out, "wb").write(b"".join(open(out + ".part%03d" % i, "rb").read() for i in range(parts)))
    if v.get("bam"):
        want = os.path.join(GOLD, "ends_%s.ref.bam" % name)
        assert bam_payload(out) == bam_payload(want)
        assert open(out, "rb").read()[-28:] == open(want, "rb").read()[-28:]
    else:
        mine = "".join(l for l in open(out) if not l.startswith("@PG"))
        assert mine == gzip.open(os.path.join(GOLD, "ends_%s.ref.sam.gz" % name), "rt").read()
    stats = "".join(l + "\n" for l in p.stderr.splitlines() if l.startswith("No. of") or l.startswith("Mismatch"))
    assert stats == open(os.path.join(GOLD, "ends_%s.ref.stats" % name)).read()


# ---- -m gpu: the record stages behind the mapping ---------------------------------------------------------------------------------------------------------
@gpu
def test_record_stages_on_pairs_whose_mates_lie_on_two_references(gold, tmp_path):
    """--bam --sort --bai --markdup --methyl --mbias on the ends pairs.  Hundreds of them have their mates on two sequences and still
    name each other `=` (the reference accepts them: both coordinates are relative to their own sequence, so TLEN stays within
    --max), each mate's record carrying its own refID with next_refID equal to it.  The sorted file, its index, the duplicate marks,
    the bedGraph files and the M-bias table are what the spec modules make of the plain --bam output of the same command."""
    import ctypes
    import bai_spec
    import markdup_spec
    import mbias_spec
    import methyl_spec
    import test_methyl as tm
    from test_sorted_bam import EOF_BLOCK, split_records, stable_sorted
    from test_oracle import ends_inputs
    inputs = ends_inputs(dict(kind="pe"), tmp_path)
    n = sum(1 for _ in open(inputs[1])) // 4
    plain = str(tmp_path / "plain.bam"); pre = str(tmp_path / "all"); out = pre + ".bam"
    tm._run(gold["fa"], inputs, [], plain)
    entries = tm._by_template(split_records(bam_payload(plain)[1]), n, True, "q")
    two_refs = sum(1 for a, b in zip(entries[::2], entries[1::2]) if a and b and a[4:8] != b[4:8])
    assert two_refs >= 200
    assert all(r[4:8] == r[24:28] for r in entries if r)                       # ... and every record says `=`
    err = tm._run(gold["fa"], inputs, ["--sort", "--bai", "--markdup", "--methyl", pre, "--mbias"] + tm.ALL_CONTEXTS, out)
    marked = markdup_spec.mark(entries, True)
    assert sum(1 for r in marked if r and struct.unpack_from("<H", r, 18)[0] & 0x400) >= 100
    assert bam_payload(out) == (bam_payload(plain)[0], stable_sorted(b"".join(marked)))
    assert open(out, "rb").read()[-28:] == EOF_BLOCK
    assert open(out + ".bai", "rb").read() == bai_spec.spec_bai(out)
    ix = gold["ix"]
    seqs = methyl_spec.genome_of_pac(ctypes.string_at(ix.view.pac, int(ix.view.pac_bytes)), ix.chrom_len)
    clip = methyl_spec.clips(entries)
    walked = mbias_spec.walk(seqs, marked, clip)
    want_sites = mbias_spec.sites_of(walked, 7)
    assert len(want_sites) > 1000
    assert tm._files(pre) == tm._spec_files(pre, ix.chrom_names, want_sites)
    want_t = mbias_spec.table_of(walked, 7)
    assert open(pre + "_mbias.tsv", "rb").read() == mbias_spec.tsv(want_t)
    assert int(re.search(r"methyl: sites .*, mbias calls (\d+)", err).group(1)) == mbias_spec.total(want_t)
