"""The oracle (CPU restatement) is pinned: (1) against the committed golden SAM the REAL reference wrote
(tests/golden/make_golden.py), (2) against the reference binary itself on fresh seeded data when
oracle/_ref/bitmapperBS is present."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import orc
from common import GOLD, ROOT, e_of, golden_args, gunzip_to, plant_repeats
from conftest import ref_binary


@pytest.fixture(scope="module")
def golden_index(tmp_path_factory, oracle):
    wd = tmp_path_factory.mktemp("gold")
    fa = str(wd / "genome.fa")
    gunzip_to(os.path.join(GOLD, "genome.fa.gz"), fa)
    assert oracle.orc_index_build(fa.encode(), fa.encode()) == 0
    return fa


@pytest.mark.parametrize("name", sorted(golden_args()))
def test_oracle_reproduces_reference_golden_sam(name, golden_index, tmp_path, oracle):
    args = golden_args()[name]
    fq = str(tmp_path / "r.fq"); out = str(tmp_path / "o.sam")
    gunzip_to(os.path.join(GOLD, "se_%s.fq.gz" % name), fq)
    ix = orc.OrcIndex(golden_index)
    st = np.zeros(5, dtype=np.int64)
    import ctypes as C
    prm = orc.params(e_f=e_of(args))
    assert oracle.orc_search_se(ix.h, C.byref(prm), fq.encode(), out.encode(), b"", st.ctypes.data) == 0
    mine = "".join(l for l in open(out) if not l.startswith("@PG"))
    gold = gzip.open(os.path.join(GOLD, "se_%s.ref.sam.gz" % name), "rt").read()
    assert mine == gold
    # mapstats (Bitmapper_main.cpp:275-284)
    ref_stats = open(os.path.join(GOLD, "se_%s.ref.stats" % name)).read().split("\n")
    assert int(ref_stats[0].split()[-1]) == st[0]
    assert int(ref_stats[1].split()[5]) == st[1] and int(ref_stats[2].split()[5]) == st[2]


@pytest.mark.skipif(ref_binary() is None, reason="oracle/_ref/bitmapperBS not built")
@pytest.mark.parametrize("cfg", [
    dict(n=20000, L=100, seed=11, sub=0.01, indel=0.001, qual="random", e=0.08),
    dict(n=15000, L=150, seed=12, sub=0.02, indel=0.002, qual="random", n_rate=0.003, e=0.04),
    dict(n=6000, L=250, seed=13, sub=0.03, indel=0.001, qual="random", e=0.08),
    dict(n=8000, L=60, seed=14, sub=0.03, indel=0.002, qual="const", e=0.1),
])
def test_oracle_vs_reference_binary_fresh_data(cfg, tmp_path, oracle):
    from bitmapperbs_amd import synth
    cfg = dict(cfg); e = cfg.pop("e")
    names, chroms = synth.make_genome(600_000, 3, seed=31 + cfg["seed"])
    plant_repeats(chroms, seed=cfg["seed"])
    fa = str(tmp_path / "g.fa")
    synth.write_fasta(fa, names, chroms)
    assert oracle.orc_index_build(fa.encode(), fa.encode()) == 0
    r = synth.make_reads_se(chroms, **cfg)
    fq = str(tmp_path / "r.fq")
    synth.write_fastq(fq, r)
    ref_sam = str(tmp_path / "ref.sam"); my_sam = str(tmp_path / "orc.sam")
    p = subprocess.run([ref_binary(), "--search", fa, "--seq", fq, "-t", "1", "-e", str(e), "-o", ref_sam],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    q = subprocess.run([os.path.join(ROOT, "oracle", "bmbs_oracle"), "search", fa, "--seq", fq, "-e", str(e), "-o", my_sam],
                       capture_output=True, text=True)
    assert q.returncode == 0, q.stderr
    a = [l for l in open(ref_sam) if not l.startswith("@PG")]
    b = [l for l in open(my_sam) if not l.startswith("@PG")]
    assert a == b
    sa = [l.split() for l in p.stderr.splitlines() if l.startswith("No. of")]
    sb = [l.split() for l in q.stderr.splitlines() if l.startswith("No. of")]
    assert sa == sb


def test_bpm_known_answers():
    """hand-checked cases of the BS banded Myers rules (Levenshtein_Cal.h:351-567)"""
    k = 2
    read = np.frombuffer(b"ACGTTGCA", dtype=np.uint8)
    # exact match on the un-gapped diagonal: window = 2 pad + read + 2 pad
    w = np.frombuffer(b"GG" + b"ACGTTGCA" + b"GG", dtype=np.uint8)
    assert orc.bpm(w, read, k) == (0, len(read) - 1 + k)
    # read T on window C is a match (bisulfite), read C on window T is not
    w2 = np.frombuffer(b"GG" + b"ACGCCGCA" + b"GG", dtype=np.uint8)
    assert orc.bpm(w2, read, k)[0] == 0
    read_c = np.frombuffer(b"ACGCCGCA", dtype=np.uint8)
    assert orc.bpm(w, read_c, k)[0] == 2
    # more than k errors -> (0xFFFFFFFF, -1)
    w3 = np.frombuffer(b"GG" + b"TTTTTTTT" + b"GG", dtype=np.uint8)
    assert orc.bpm(w3, np.frombuffer(b"AAAAAAAA", dtype=np.uint8), k) == (0xFFFFFFFF, -1)
    # all-zero (out-of-range) window never matches
    assert orc.bpm(np.zeros(12, np.uint8), read, k) == (0xFFFFFFFF, -1)


def test_mapq_table_spot_values():
    """MAP_Calculation (Schema.cpp:168-405) spot values"""
    L = orc.load()
    import ctypes as C
    p = orc.params()
    assert L.orc_mapq(C.byref(p), 0xFFFFFFFF, 6, 0) == 42
    assert L.orc_mapq(C.byref(p), 0xFFFFFFFF, 6, -6) == 42      # 42/48 = 0.875
    assert L.orc_mapq(C.byref(p), 0xFFFFFFFF, 6, -12) == 40     # 36/48 = 0.75
    assert L.orc_mapq(C.byref(p), 0, 6, 0) == 1
    assert L.orc_mapq(C.byref(p), 6, 6, 0) == 39
    assert L.orc_mapq(C.byref(p), 3, 6, -6) == 25               # rank_error 0.5, rank 0.875


def pe_golden_args():
    import json
    return json.load(open(os.path.join(GOLD, "pe_args.json")))


def pe_params(args):
    kw = dict(e_f=e_of(args))
    if "--min" in args:
        kw["min_ins"] = int(args[args.index("--min") + 1])
    if "--max" in args:
        kw["max_ins"] = int(args[args.index("--max") + 1])
    if "--sensitive" in args:
        kw["sensitive"] = 1
    return kw


@pytest.mark.parametrize("name", sorted(pe_golden_args()))
def test_oracle_reproduces_reference_golden_sam_paired_end(name, golden_index, tmp_path, oracle):
    import ctypes as C
    args = pe_golden_args()[name]
    f1 = str(tmp_path / "1.fq"); f2 = str(tmp_path / "2.fq"); out = str(tmp_path / "o.sam")
    gunzip_to(os.path.join(GOLD, "pe_%s_1.fq.gz" % name), f1)
    gunzip_to(os.path.join(GOLD, "pe_%s_2.fq.gz" % name), f2)
    ix = orc.OrcIndex(golden_index)
    st = np.zeros(5, dtype=np.int64)
    prm = orc.params(**pe_params(args))
    assert oracle.orc_search_pe(ix.h, C.byref(prm), f1.encode(), f2.encode(), out.encode(), b"", st.ctypes.data) == 0
    mine = "".join(l for l in open(out) if not l.startswith("@PG"))
    assert mine == gzip.open(os.path.join(GOLD, "pe_%s.ref.sam.gz" % name), "rt").read()
    from bitmapperbs_amd import distributed
    assert distributed.mapstats_text(st) == open(os.path.join(GOLD, "pe_%s.ref.stats" % name)).read()


@pytest.mark.skipif(ref_binary() is None, reason="oracle/_ref/bitmapperBS not built")
@pytest.mark.parametrize("cfg", [
    dict(n=15000, L=150, seed=21, sub=0.01, indel=0.001, qual="random", args=[]),
    dict(n=15000, L=100, seed=22, sub=0.02, indel=0.002, qual="random", ins_hi=560, args=["-e", "0.04", "--max", "520"]),
    dict(n=5000, L=250, seed=23, sub=0.03, indel=0.001, qual="random", ins_hi=700, args=["--max", "800"]),
    dict(n=12000, L=100, seed=24, sub=0.06, indel=0.003, qual="random", args=["--sensitive"]),
    dict(n=8000, L=150, seed=25, sub=0.07, indel=0.004, qual="random", ins_hi=450, args=["--sensitive", "-e", "0.1", "--max", "450"]),
    dict(n=8000, L=100, seed=26, sub=0.02, indel=0.002, qual="random", ins_hi=560, args=["--sensitive", "-e", "0.04", "--max", "520"]),
])
def test_oracle_vs_reference_binary_fresh_data_paired_end(cfg, tmp_path, oracle):
    from bitmapperbs_amd import synth
    cfg = dict(cfg); args = cfg.pop("args")
    names, chroms = synth.make_genome(600_000, 3, seed=41 + cfg["seed"])
    plant_repeats(chroms, seed=cfg["seed"])
    fa = str(tmp_path / "g.fa")
    synth.write_fasta(fa, names, chroms)
    assert oracle.orc_index_build(fa.encode(), fa.encode()) == 0
    m1, m2 = synth.make_reads_pe(chroms, **cfg)
    f1 = str(tmp_path / "1.fq"); f2 = str(tmp_path / "2.fq")
    synth.write_fastq(f1, m1); synth.write_fastq(f2, m2)
    ref_sam = str(tmp_path / "ref.sam"); my_sam = str(tmp_path / "orc.sam")
    p = subprocess.run([ref_binary(), "--search", fa, "--seq1", f1, "--seq2", f2, "-t", "1", "-o", ref_sam] + args,
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    q = subprocess.run([os.path.join(ROOT, "oracle", "bmbs_oracle"), "search", fa, "--seq1", f1, "--seq2", f2, "-o", my_sam] + args,
                       capture_output=True, text=True)
    assert q.returncode == 0, q.stderr
    assert [l for l in open(ref_sam) if not l.startswith("@PG")] == [l for l in open(my_sam) if not l.startswith("@PG")]
    assert [l.split() for l in p.stderr.splitlines() if l.startswith("No. of")] == \
           [l.split() for l in q.stderr.splitlines() if l.startswith("No. of")]


# ---- output variants: --unmapped_out / --ambiguous_out / --pbat (Process_CommandLines.cpp:93-105) ---------------
def variants():
    import json
    return json.load(open(os.path.join(GOLD, "variants.json")))


def variant_inputs(v, tmp_path):
    """FASTQ arguments of a variant, built from the committed read sets"""
    from common import pbat_fastq, trim_fastq
    if v["kind"] == "se":
        fq = str(tmp_path / "r.fq")
        gunzip_to(os.path.join(GOLD, "se_%s.fq.gz" % v["base"]), fq)
        if v.get("pbat"):
            pbat_fastq(fq, str(tmp_path / "r_pbat.fq")); fq = str(tmp_path / "r_pbat.fq")
        if v.get("trim"):
            trim_fastq(fq, str(tmp_path / "r_trim.fq"), v["trim"][0]); fq = str(tmp_path / "r_trim.fq")
        return ["--seq", fq]
    f1 = str(tmp_path / "1.fq"); f2 = str(tmp_path / "2.fq")
    gunzip_to(os.path.join(GOLD, "pe_%s_1.fq.gz" % v["base"]), f1)
    gunzip_to(os.path.join(GOLD, "pe_%s_2.fq.gz" % v["base"]), f2)
    if v.get("swap"):
        f1, f2 = f2, f1
    if v.get("trim"):
        t1 = str(tmp_path / "1t.fq"); t2 = str(tmp_path / "2t.fq")
        trim_fastq(f1, t1, v["trim"][0]); trim_fastq(f2, t2, v["trim"][1])
        f1, f2 = t1, t2
    return ["--seq1", f1, "--seq2", f2]


@pytest.mark.parametrize("name", sorted(k for k, v in variants().items() if not v.get("bam")))
def test_oracle_cli_reproduces_reference_output_variants(name, golden_index, tmp_path, oracle):
    v = variants()[name]
    out = str(tmp_path / "o.sam")
    q = subprocess.run([os.path.join(ROOT, "oracle", "bmbs_oracle"), "search", golden_index] + variant_inputs(v, tmp_path) + ["-o", out] + v["args"],
                       capture_output=True, text=True)
    assert q.returncode == 0, q.stderr
    mine = "".join(l for l in open(out) if not l.startswith("@PG"))
    assert mine == gzip.open(os.path.join(GOLD, "var_%s.ref.sam.gz" % name), "rt").read()
    stats = "".join(l + "\n" for l in q.stderr.splitlines() if l.startswith("No. of") or l.startswith("Mismatch"))
    assert stats == open(os.path.join(GOLD, "var_%s.ref.stats" % name)).read()


# ---- the `return 0;` splices of oracle/build_ref.sh are behaviour-neutral -----------------------------------------------------------
@pytest.mark.skipif(ref_binary() is None or not os.path.isdir(os.environ.get("BMBS_REFERENCE_DIR", "/root/reference")),
                    reason="needs /root/reference (this container) to compile the control binary")
@pytest.mark.parametrize("kind,name", [("se", "b150"), ("se", "e75"), ("pe", "s100"), ("pe", "p150")])
def test_unpatched_O0_reference_writes_the_committed_goldens(kind, name, golden_index, tmp_path):
    """oracle/build_ref.sh splices `return 0;` into 33 non-void functions that fall off their end (with g++ >= 8 the -O3 binary
    otherwise crashes).  Control: the same four sources compiled WITHOUT any splice at -O0 (oracle/build_ref_unpatched.sh), where
    the compiler does not exploit the undefined behaviour, must write the SAM the spliced -O3 binary wrote into tests/golden/."""
    subprocess.run([os.path.join(ROOT, "oracle", "build_ref_unpatched.sh")], check=True, capture_output=True)
    exe = os.path.join(ROOT, "oracle", "_ref", "bitmapperBS_unpatched_O0")
    assert os.path.exists(exe)
    out = str(tmp_path / "o.sam")
    if kind == "se":
        fq = str(tmp_path / "r.fq")
        gunzip_to(os.path.join(GOLD, "se_%s.fq.gz" % name), fq)
        cmd = [exe, "--search", golden_index, "--seq", fq, "-t", "1", "-o", out] + golden_args()[name]
        gold = os.path.join(GOLD, "se_%s.ref.sam.gz" % name)
    else:
        f1 = str(tmp_path / "1.fq"); f2 = str(tmp_path / "2.fq")
        gunzip_to(os.path.join(GOLD, "pe_%s_1.fq.gz" % name), f1)
        gunzip_to(os.path.join(GOLD, "pe_%s_2.fq.gz" % name), f2)
        cmd = [exe, "--search", golden_index, "--seq1", f1, "--seq2", f2, "-t", "1", "-o", out] + pe_golden_args()[name]
        gold = os.path.join(GOLD, "pe_%s.ref.sam.gz" % name)
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    mine = "".join(l for l in open(out) if not l.startswith("@PG"))
    assert mine == gzip.open(gold, "rt").read()


def test_oracle_cli_equals_reference_on_random_files_and_options(tmp_path):
    """six fixed draws of tools/fuzz_e2e.py --oracle: random FASTQ files (lengths 30-250, trimmed records, letters outside ACGT,
    lower case) and random --search options (-e, mismatch / N / gap penalties, insert bounds, --sensitive, --pbat, --unmapped_out,
    --ambiguous_out) through the real reference binary (-t 1) and through the oracle's command line: same SAM body, same
    mapstats.  Pins the restatement to the reference beyond the committed goldens' parameter sets (400 such trials ran in round 2:
    profiles/r02_fuzz_oracle_vs_reference.txt)."""
    import importlib.util
    import numpy as np
    from common import ROOT
    spec = importlib.util.spec_from_file_location("fuzz_e2e", os.path.join(ROOT, "tools", "fuzz_e2e.py"))
    fz = importlib.util.module_from_spec(spec); spec.loader.exec_module(fz)
    if not os.path.exists(fz.REF):
        pytest.skip("oracle/_ref/bitmapperBS is not built here")
    fz.USE_ORACLE = True
    env = fz.make_env(str(tmp_path))
    rng = np.random.default_rng(31337)
    for _ in range(6):
        t = fz.draw(rng)
        bad, lines = fz.run_trial(t, env, str(tmp_path))
        assert not bad, (t, bad[:2])


# ---- reads and pairs at and across chromosome ends (tests/ends.py; the reference's own output: make_golden.py --only ends) ------------
def ends_runs():
    import json
    return json.load(open(os.path.join(GOLD, "ends.json")))


def ends_inputs(v, tmp_path):
    """FASTQ arguments of an `ends_*` run, built from the committed read sets"""
    from common import trim_fastq
    files = [str(tmp_path / "se.fq")] if v["kind"] == "se" else [str(tmp_path / "pe_1.fq"), str(tmp_path / "pe_2.fq")]
    for i, f in enumerate(files):
        gunzip_to(os.path.join(GOLD, "ends_" + os.path.basename(f) + ".gz"), f)
        if v.get("trim"):
            trim_fastq(f, f[:-3] + "_trim.fq", v["trim"][i]); files[i] = f[:-3] + "_trim.fq"
    return ["--seq", files[0]] if v["kind"] == "se" else ["--seq1", files[0], "--seq2", files[1]]


@pytest.fixture(scope="module")
def ends_index(tmp_path_factory, oracle):
    wd = tmp_path_factory.mktemp("ends")
    fa = str(wd / "genome.fa")
    gunzip_to(os.path.join(GOLD, "ends_genome.fa.gz"), fa)
    assert oracle.orc_index_build(fa.encode(), fa.encode()) == 0
    return fa


@pytest.mark.parametrize("name", sorted(ends_runs()))
def test_oracle_cli_reproduces_reference_at_chromosome_ends(name, ends_index, tmp_path):
    """off-end rejection on every exit path, pairs whose mates lie on two chromosomes, TLEN at --min/--max: the oracle's SAM and
    mapstats equal the reference's; its --bam runs are compared record by record (the oracle writes SAM only)"""
    v = ends_runs()[name]
    out = str(tmp_path / "o.sam")
    q = subprocess.run([os.path.join(ROOT, "oracle", "bmbs_oracle"), "search", ends_index] + ends_inputs(v, tmp_path) + ["-o", out] +
                       [a for a in v["args"] if a != "--bam"], capture_output=True, text=True)
    assert q.returncode == 0, q.stderr
    if v.get("bam"):
        from common import bam_payload, sam_to_bam_records
        refs = [l.split("\t")[1][3:] for l in open(out) if l.startswith("@SQ")]
        assert sam_to_bam_records(open(out, "rb").read(), refs) == bam_payload(os.path.join(GOLD, "ends_%s.ref.bam" % name))[1]
    else:
        mine = "".join(l for l in open(out) if not l.startswith("@PG"))
        assert mine == gzip.open(os.path.join(GOLD, "ends_%s.ref.sam.gz" % name), "rt").read()
    stats = "".join(l + "\n" for l in q.stderr.splitlines() if l.startswith("No. of") or l.startswith("Mismatch"))
    assert stats == open(os.path.join(GOLD, "ends_%s.ref.stats" % name)).read()
