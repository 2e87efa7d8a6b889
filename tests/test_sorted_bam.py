"""Coordinate-sorted BAM (`bmbs_search --bam --sort`, BMBS_TEXT_BAM_SORTED, bmbs_bam_sort): the record sequence of a sorted file is the
STABLE sort, by the key below, of the record sequence the same command writes without --sort.  The sort is a permutation: every
comparison here is exact."""
import os
import struct
import subprocess

import numpy as np
import pytest

from common import GOLD, ROOT, bam_payload, bgzf_blocks, gunzip_to

EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


# ---- the specification, in Python ------------------------------------------------------------------------------------------------
def bam_key(rec: bytes) -> int:
    """refID (int32 at byte 4 of the record, counting its block_size word), pos (int32 at byte 8), flag (uint16 at byte 18) ->
    (uint32)refID << 32 | (uint32)(pos + 1) << 1 | reverse-strand bit: reference index, position, strand; refID -1 last, pos -1 -> 0"""
    ref, pos = struct.unpack_from("<ii", rec, 4)
    flag = struct.unpack_from("<H", rec, 18)[0]
    return ((ref & 0xffffffff) << 32) | (((pos + 1) & 0xffffffff) << 1) | ((flag >> 4) & 1)


def split_records(stream: bytes):
    out = []
    at = 0
    while at < len(stream):
        n = struct.unpack_from("<I", stream, at)[0] + 4
        out.append(stream[at:at + n])
        at += n
    assert at == len(stream)
    return out


def stable_sorted(stream: bytes) -> bytes:
    return b"".join(sorted(split_records(stream), key=bam_key))          # (Python's sort is stable)


def make_record(ref, pos, flag, name=b"r", n_cigar=1, l_seq=10, fill=0x5a):
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name) + 1, 30, 4681, n_cigar, flag, l_seq, -1, -1, 0) + name + b"\0" + \
        b"".join(struct.pack("<I", (l_seq << 4)) for _ in range(n_cigar)) + bytes([fill & 0xff]) * ((l_seq + 1) // 2) + bytes([(fill >> 1) & 0x3f]) * l_seq
    return struct.pack("<I", len(body)) + body


def _driver():
    p = os.path.join(ROOT, "bitmapperbs_amd", "bmbs_search")
    assert os.path.exists(p), "bmbs_search not built (make -C bitmapperbs_amd/csrc)"
    return p


# ---- no GPU ------------------------------------------------------------------------------------------------------------------------
def test_key_of_hand_written_records():
    unmapped = make_record(-1, -1, 4)                  # refID -1, pos -1: behind everything
    no_pos = make_record(2, -1, 0)                     # pos -1 on a reference: in front of that reference's records
    fwd = make_record(2, 99, 0)
    rev = make_record(2, 99, 16)                       # both strands at one position: forward first
    placed = make_record(2, 99, 4 | 8 | 1 | 64)        # a placed flag-4 mate sorts by its refID / pos
    later = make_record(2, 100, 0)
    other_ref = make_record(1, 5000, 16)
    assert bam_key(unmapped) == 0xffffffff << 32
    assert bam_key(no_pos) == 2 << 32
    assert bam_key(fwd) == (2 << 32) | (100 << 1)
    assert bam_key(rev) == (2 << 32) | (100 << 1) | 1
    assert bam_key(placed) == bam_key(fwd)
    assert bam_key(other_ref) == (1 << 32) | (5001 << 1) | 1
    stream = unmapped + later + rev + placed + no_pos + fwd + other_ref
    # equal keys (placed, fwd) keep their order
    assert split_records(stable_sorted(stream)) == [other_ref, no_pos, placed, fwd, rev, later, unmapped]


def test_sort_without_bam_is_refused_by_name():
    p = subprocess.run([_driver(), "--search", "nowhere", "--seq", "none.fq", "--sort"], capture_output=True, text=True)
    assert p.returncode == 2
    assert "bmbs_search: --sort needs --bam" in p.stderr


def test_sort_with_several_output_parts_is_refused_by_name():
    p = subprocess.run([_driver(), "--search", "nowhere", "--seq", "none.fq", "--bam", "--sort", "--out-parts", "3"], capture_output=True, text=True)
    assert p.returncode == 2
    assert "bmbs_search: --sort writes one file (--out-parts 1)" in p.stderr


# ---- GPU: the library ----------------------------------------------------------------------------------------------------------------
def _synthetic_records(n=200_000, seed=11):
    """random name / CIGAR / sequence lengths, refID -1 .. 24, positions from a range small enough that most keys are tied, both
    strands, refID -1 records scattered throughout, and a few records larger than the gather kernel's LDS image"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(-1, 25, n); pos = rng.integers(0, 40, n); strand = rng.integers(0, 2, n)
    nlen = rng.integers(1, 40, n); ncig = rng.integers(0, 7, n); lseq = rng.integers(1, 400, n)
    big = rng.choice(n, 6, replace=False)
    lseq[big] = [40_000, 70_000, 33_000, 25_000, 90_000, 50_000]
    recs = []
    for i in range(n):
        r = int(ref[i])
        if r < 0 and i % 3:
            recs.append(make_record(-1, -1, 4, b"u%d" % i + b"x" * int(nlen[i]), 0, int(lseq[i]), i))
        else:
            recs.append(make_record(r, int(pos[i]), 16 if strand[i] else 0, b"q%d" % i + b"y" * int(nlen[i]), int(ncig[i]), int(lseq[i]), i))
    return recs


@pytest.mark.gpu
def test_bam_sort_of_synthetic_records_is_the_stable_sort():
    """bmbs_bam_sort on a context without an index: RAW output = the Python stable sort byte for byte; the default output is well-formed
    BGZF (BC field, CRC-32, ISIZE; every block 0xff00 input bytes except the last) and inflates to the same bytes; n = 0, n = 1, a
    wrong length (BMBS_EINVAL naming the record), a short buffer (BMBS_ENOMEM with the size needed, then success)"""
    from bitmapperbs_amd import mapper
    recs = _synthetic_records()
    stream = b"".join(recs)
    lens = np.array([len(r) for r in recs], dtype=np.uint32)
    keys = [bam_key(r) for r in recs]
    assert len(set(keys)) < len(keys) // 20                                  # most keys are tied
    want = b"".join(r for _, r in sorted(zip(keys, recs), key=lambda t: t[0]))
    m = mapper.Mapper(None, 0)
    raw = m.bam_sort(stream, lens, raw=True)
    assert raw == want
    z = m.bam_sort(stream, lens)
    blocks = bgzf_blocks(z)
    assert len(blocks) == (len(stream) + 0xff00 - 1) // 0xff00
    assert all(len(b) == 0xff00 for _, b in blocks[:-1])
    assert b"".join(b for _, b in blocks) == want
    # n = 0, n = 1
    assert m.bam_sort(b"", np.zeros(0, dtype=np.uint32), raw=True) == b""
    assert m.bam_sort(b"", np.zeros(0, dtype=np.uint32)) == b""
    assert m.bam_sort(recs[7], lens[7:8], raw=True) == recs[7]
    assert b"".join(b for _, b in bgzf_blocks(m.bam_sort(recs[7], lens[7:8]))) == recs[7]
    # a length that disagrees with the record's block_size (the sum still matches)
    bad = lens[:1000].copy(); bad[412] += 4; bad[413] -= 4
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 412\b"):
        m.bam_sort(b"".join(recs[:1000]), bad, raw=True)
    with pytest.raises(RuntimeError, match=r"bmbs error -22"):
        m.bam_sort(stream[:-1], lens, raw=True)                              # sum(len) != bytes
    # too small a buffer: the size needed, then success
    for rawmode in (True, False):
        with pytest.raises(mapper.BamSortNoRoom) as e:
            m.bam_sort(stream, lens, raw=rawmode, cap=1000)
        assert e.value.needed == (len(stream) if rawmode else len(z))
        assert m.bam_sort(stream, lens, raw=rawmode, cap=e.value.needed) == (want if rawmode else z)
    m.close()


@pytest.fixture(scope="module")
def senv(tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bitmapperbs_amd import synth, mapper
    from common import plant_repeats
    wd = tmp_path_factory.mktemp("sorted")
    names, chroms = synth.make_genome(1_500_000, 3, seed=77)
    plant_repeats(chroms, seed=78)
    fa = str(wd / "g.fa")
    synth.write_fasta(fa, names, chroms)
    mapper.Index.build(fa, fa, threads=8)
    return dict(fa=fa, chroms=chroms, ix=mapper.Index(fa), wd=str(wd))


def _fq(mm, n):
    return b"".join(b"@" + mm["names"][i] + b"\n" + mm["seq"][i].tobytes() + b"\n+\n" + mm["qual"][i].tobytes() + b"\n" for i in range(n))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["se_odd_unmapped", "pe_p100", "pe_s150_unmapped", "se_repeated_reads"])
def test_sorted_text_call_returns_the_stable_sort_of_the_unsorted_records(senv, case):
    """TEXT_BAM | TEXT_BAM_SORTED: the uncompressed records = the stable sort of the records the TEXT_BAM call's blocks inflate to;
    sorted_index() = their keys (non-decreasing) and lengths; the statistics are those of the unsorted call"""
    from bitmapperbs_amd import mapper, synth
    from test_gpu_parity import _odd_fastq
    M = mapper.Mapper
    t2 = None; kw = {}
    if case == "se_odd_unmapped":
        t1 = _odd_fastq(senv); n = 6000; flags = M.TEXT_UNMAPPED
    elif case == "se_repeated_reads":
        # a few reads many times over, among others: ties between real records
        r = synth.make_reads_se(senv["chroms"], n=3000, L=100, seed=9, sub=0.01, indel=0.001, qual="random")
        order = [i if i % 4 else (i // 4) % 5 for i in range(3000)]
        t1 = b"".join(b"@s%d\n" % j + r["seq"][i].tobytes() + b"\n+\n" + r["qual"][i].tobytes() + b"\n" for j, i in enumerate(order))
        n = 3000; flags = M.TEXT_UNMAPPED
    else:
        sens = case.startswith("pe_s")
        m1, m2 = synth.make_reads_pe(senv["chroms"], n=4000, L=150 if sens else 100, seed=5, sub=0.03, indel=0.003, qual="random")
        t1, t2 = _fq(m1, 4000), _fq(m2, 4000); n = 4000
        kw = dict(sensitive=1 if sens else 0)
        flags = M.TEXT_UNMAPPED if case.endswith("unmapped") else 0
    m = M(senv["ix"], 0, **kw)
    z = m.map_text(t1, n, t2, flags=flags | M.TEXT_BAM)
    st_unsorted = m.stats().copy()
    m.reset_stats()
    unsorted = b"".join(raw for _, raw in bgzf_blocks(z))
    got = m.map_text(t1, n, t2, flags=flags | M.TEXT_BAM | M.TEXT_BAM_SORTED)
    key, ln = m.sorted_index()
    assert (m.stats() == st_unsorted).all()
    want = stable_sorted(unsorted)
    assert got == want
    recs = split_records(got)
    assert len(recs) > 1000
    assert int(ln.astype(np.int64).sum()) == len(got)
    assert ln.tolist() == [len(r) for r in recs]
    assert key.tolist() == [bam_key(r) for r in recs]
    assert (key[1:] >= key[:-1]).all()
    if case == "se_repeated_reads":
        assert len(set(key.tolist())) < len(recs) * 0.85                      # there are ties
    # a buffer that is too small: the size needed, statistics restored, then the same bytes
    m.reset_stats()
    with pytest.raises(RuntimeError, match="bmbs error -12"):
        m.map_text(t1, n, t2, flags=flags | M.TEXT_BAM | M.TEXT_BAM_SORTED, cap=4096)
    assert m.map_text(t1, n, t2, flags=flags | M.TEXT_BAM | M.TEXT_BAM_SORTED, cap=len(got)) == got
    assert (m.stats() == st_unsorted).all()
    # the flag on its own is refused
    with pytest.raises(RuntimeError, match="bmbs error -22"):
        m.map_text(t1, n, t2, flags=flags | M.TEXT_BAM_SORTED)
    m.close()


# ---- GPU: the driver -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    """the golden genome's index, built once"""
    from bitmapperbs_amd import mapper
    wd = tmp_path_factory.mktemp("sorted_gold")
    fa = str(wd / "genome.fa")
    gunzip_to(os.path.join(GOLD, "genome.fa.gz"), fa)
    mapper.Index.build(fa, fa, threads=4)
    return fa


def _bam_header_text(path):
    import gzip
    d = gzip.open(path, "rb").read()
    assert d[:4] == b"BAM\x01"
    return d[8:8 + struct.unpack("<i", d[4:8])[0]].decode()


def _run(gold, inputs, args, out, sort, env=None):
    cmd = [_driver(), "--search", gold] + inputs + ["-o", out, "--mapstats", out + ".stats", "--verbose"] + args + (["--sort"] if sort else [])
    return subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))


def _sort_counts(stderr):
    import re
    m = re.search(r"sort: bins (\d+) .*pass-2 calls (\d+), store bytes (\d+)", stderr)
    assert m, stderr
    return int(m.group(1)), int(m.group(2)), int(m.group(3))


def _check_sorted_file(path, unsorted_path, stderr=""):
    """dictionary unchanged, records = the stable sort of the unsorted file's, header text differs in SO: only, BGZF EOF block, same mapstats"""
    ref_dict, ref_recs = bam_payload(unsorted_path)
    got_dict, got_recs = bam_payload(path)
    assert got_dict == ref_dict
    assert got_recs == stable_sorted(ref_recs), stderr
    assert open(path, "rb").read()[-28:] == EOF_BLOCK
    mine = [l for l in _bam_header_text(path).split("\n") if not l.startswith("@PG")]
    theirs = [l for l in _bam_header_text(unsorted_path).split("\n") if not l.startswith("@PG")]
    assert mine[0] == "@HD\tVN:1.4\tSO:coordinate" and theirs[0] == "@HD\tVN:1.4\tSO:unsorted"
    assert mine[1:] == theirs[1:]
    return got_recs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["se_e75_bam", "pe_p75_bam"])
def test_sorted_driver_output_is_the_stable_sort_of_the_reference_bam(name, gold, tmp_path):
    """--bam --sort against the reference's own (htslib-written, unsorted) BAM of the same command"""
    from test_oracle import variants, variant_inputs
    v = variants()[name]
    out = str(tmp_path / "o.bam")
    p = _run(gold, variant_inputs(v, tmp_path), v["args"], out, True)
    assert p.returncode == 0, p.stderr
    _check_sorted_file(out, os.path.join(GOLD, "var_%s.ref.bam" % name), p.stderr)
    assert open(out + ".stats").read() == open(os.path.join(GOLD, "var_%s.ref.stats" % name)).read()


def _inputs(kind, name, tmp_path, gz=False):
    import shutil
    if kind == "se":
        fq = str(tmp_path / "r.fq")
        if gz:
            shutil.copy(os.path.join(GOLD, "se_%s.fq.gz" % name), fq + ".gz")
            return ["--seq", fq + ".gz"]
        gunzip_to(os.path.join(GOLD, "se_%s.fq.gz" % name), fq)
        return ["--seq", fq]
    f1 = str(tmp_path / "1.fq"); f2 = str(tmp_path / "2.fq")
    gunzip_to(os.path.join(GOLD, "pe_%s_1.fq.gz" % name), f1)
    gunzip_to(os.path.join(GOLD, "pe_%s_2.fq.gz" % name), f2)
    return ["--seq1", f1, "--seq2", f2]


def _sorted_against_own_unsorted(gold, inputs, args, tmp_path, env=None, tag="", sorted_args=()):
    """sorted_args: further options of the sorted run only (the unsorted file of one input is made once, under the name u.bam)"""
    un = str(tmp_path / "u.bam"); so = str(tmp_path / ("s%s.bam" % tag))
    if not os.path.exists(un):
        p = _run(gold, inputs, ["--bam"] + args, un, False)
        assert p.returncode == 0, p.stderr
        open(un + ".err", "w").write(p.stderr)
    p = type("P", (), {"stderr": open(un + ".err").read()})
    q = _run(gold, inputs, ["--bam"] + args + list(sorted_args), so, True, env)
    assert q.returncode == 0, q.stderr
    recs = _check_sorted_file(so, un, q.stderr)
    assert open(so + ".stats").read() == open(un + ".stats").read()          # mapstats: identical with and without --sort
    stats = lambda e: [l for l in e.splitlines() if l.startswith("No. of") or l.startswith("Mismatch")]
    assert stats(q.stderr) == stats(p.stderr) and len(stats(p.stderr)) == 5
    return recs, q.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["se", "pe", "sensitive", "pbat", "unmapped_ambiguous", "gz"])
def test_sorted_driver_output_is_the_stable_sort_of_the_unsorted_run(case, gold, tmp_path):
    from test_oracle import variants, variant_inputs
    from common import golden_args
    pe_args = __import__("json").load(open(os.path.join(GOLD, "pe_args.json")))
    if case == "se":
        inputs, args = _inputs("se", "b150", tmp_path), golden_args()["b150"]
    elif case == "pe":
        inputs, args = _inputs("pe", "p100", tmp_path), pe_args["p100"]
    elif case == "sensitive":
        inputs, args = _inputs("pe", "s100", tmp_path), pe_args["s100"]
    elif case == "pbat":
        v = variants()["se_b150_pbat"]; inputs, args = variant_inputs(v, tmp_path), v["args"]
    elif case == "unmapped_ambiguous":
        v = variants()["se_e75_ua"]; inputs, args = variant_inputs(v, tmp_path), v["args"]
    else:
        inputs, args = _inputs("se", "e75", tmp_path, gz=True), golden_args()["e75"] + ["--unmapped_out", "--batch", "700"]
    recs, _ = _sorted_against_own_unsorted(gold, inputs, args, tmp_path)
    assert len(split_records(recs)) > 500


@pytest.mark.gpu
@pytest.mark.parametrize("kind,name", [("se", "b150"), ("pe", "p100")])
def test_sorted_driver_paths_give_one_payload(kind, name, gold, tmp_path):
    """small batches on one and on four contexts, 1 / 7 / the default number of bins, a call budget that forces many pass-2 calls (and,
    with one bin, the re-cut of a bin that is over the budget): the payload is the same every time"""
    from common import golden_args
    pe_args = __import__("json").load(open(os.path.join(GOLD, "pe_args.json")))
    inputs = _inputs(kind, name, tmp_path)
    args = (golden_args()[name] if kind == "se" else pe_args[name]) + ["--unmapped_out", "--batch", "300"]
    first = None
    for contexts in ("1", "4"):
        for bins in ("1", "7", None):
            env = {"BMBS_SORT_CALL_BYTES": "40000"}
            if bins:
                env["BMBS_SORT_BINS"] = bins
            recs, err = _sorted_against_own_unsorted(gold, inputs, args, tmp_path, env, "_%s_%s" % (contexts, bins), ["--contexts", contexts])
            n_bins, n_calls, store = _sort_counts(err)
            assert n_calls > 1 and store >= len(recs)
            assert n_bins == (2 if bins == "1" else 8 if bins == "7" else n_bins) and (bins == "1" or n_bins > 1)
            if bins is None:
                assert n_bins > 100
            first = first or recs
            assert recs == first


def _skew_fastq(tmp_path, gold):
    """the reads of se_b150, and one of them (one that maps) 5 000 times over in between"""
    import gzip
    lines = gzip.open(os.path.join(GOLD, "se_b150.fq.gz"), "rt").read().split("\n")
    sam = [l.split("\t") for l in gzip.open(os.path.join(GOLD, "se_b150.ref.sam.gz"), "rt").read().split("\n") if l and not l.startswith("@")]
    mapped = {f[0] for f in sam}
    recs = [lines[i:i + 4] for i in range(0, len(lines) - 3, 4)]
    pick = next(r for r in recs[50:] if r[0][1:].split(" ")[0].split("/")[0] in mapped)
    out = []
    copies = 0
    for i, r in enumerate(recs):
        out.append("\n".join(r))
        for _ in range(5000 // 200 if i < 200 else 0):
            out.append("@pile%d\n%s\n+\n%s" % (copies, pick[1], pick[3])); copies += 1
    assert copies == 5000
    fq = str(tmp_path / "skew.fq")
    open(fq, "w").write("\n".join(out) + "\n")
    return fq


@pytest.mark.gpu
def test_sorted_driver_skew_and_store_cap(gold, tmp_path):
    """one locus holds most of the records and is several times the call budget: a single key is cut in input order; a --sort-mem that
    is too small stops the run with exit 1, says so and leaves no file"""
    from common import golden_args
    fq = _skew_fastq(tmp_path, gold)
    args = golden_args()["b150"] + ["--batch", "1000"]
    recs, err = _sorted_against_own_unsorted(gold, ["--seq", fq], args, tmp_path, {"BMBS_SORT_CALL_BYTES": "200000"})
    keys = [bam_key(r) for r in split_records(recs)]
    top = max(set(keys), key=keys.count)
    pile = sum(len(r) for r in split_records(recs) if bam_key(r) == top)
    assert keys.count(top) >= 5000 and pile > 3 * 200000
    assert _sort_counts(err)[1] > pile // 200000
    out = str(tmp_path / "capped.bam")
    p = _run(gold, ["--seq", fq], ["--bam", "--sort-mem", "0.0005"] + args, out, True)
    assert p.returncode == 1
    assert "--sort-mem" in p.stderr and "records fit" in p.stderr
    assert not os.path.exists(out)
