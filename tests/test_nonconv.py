"""The non-conversion filter on the device (bmbs_bam_nonconv, bmbs_text_sorted_nonconv, `bmbs_search --bam --sort
--filter-non-conversion`) against tests/nonconv_spec.py.  Counts, verdicts, totals and flags are integers, files are bytes: every
comparison here is exact."""
import ctypes
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bai_spec
import mbias_spec
import methyl_spec as spec
import nonconv_spec as nc
import test_mbias
import test_methyl as tm
from common import GOLD, bam_payload, bgzf_blocks, golden_args
from nonconv_spec import Params
from test_mbias_spec import random_records
from test_methyl import gold, mapper_on_gold  # noqa: F401  (fixtures)
from test_sorted_bam import split_records

pytestmark = pytest.mark.gpu

# templates of a call: below, at and above the 4 records a wave holds and the 16 a block holds at a time, more than one block, all
COUNTS = (1, 2, 3, 4, 63, 64, 65, 257, 20_000)
N_RECORDS = 20_000
PARAMS = {"default": nc.DEFAULTS, "percent": Params(0, 50, 5, 0), "both": Params(3, 50, 5, 0), "off": Params(0, 0, 5, 0), "phred20": Params(3, 50, 5, 20)}


def _table(recs, tallies):
    """[record][strand][context][unmethylated, methylated]: what each record adds to the totals"""
    t = np.zeros((len(recs), 2, 3, 2), dtype=np.uint64)
    for i, (r, ta) in enumerate(zip(recs, tallies)):
        if ta is not None:
            t[i, int(spec.is_ob(struct.unpack_from("<H", r, 18)[0]))] = ta
    return t


@pytest.fixture(scope="module")
def crafted(gold):
    """20 000 random records (every 11th entry a hole) and 20 000 stacked on 200 bases, and the spec's tally of each at both quality
    bounds -- walked once; counts, verdicts and totals of any number of records and any parameters are sums over these.  No GPU."""
    rng = np.random.default_rng(23)
    seqs = gold["seqs"]
    recs = [b"" if i % 11 == 6 else r for i, r in enumerate(random_records(rng, seqs, N_RECORDS, test_mbias.L_SEQS))]
    stack = random_records(rng, seqs, N_RECORDS, test_mbias.L_SEQS, stack=True)
    out = dict(recs=recs, stack=stack, lens=np.array([len(r) for r in recs], dtype=np.uint32))
    for q in (0, 20):
        out["tally", q] = [nc.tally(r, seqs, q) for r in recs]
        out["table", q] = _table(recs, out["tally", q])
    out["stack_tally"] = [nc.tally(r, seqs, 0) for r in stack]
    return out


def _check(got, recs, tallies, table, paired, p):
    count, fail, n_fail, totals = got
    want_counts = np.array([nc.counts_of(t) for t in tallies], dtype=np.uint32).reshape(-1, 2)
    assert count.dtype.names == ("meth", "unmeth") and len(count) == len(recs)
    assert (count["meth"] == want_counts[:, 0]).all() and (count["unmeth"] == want_counts[:, 1]).all()
    want = nc.verdicts(tallies, paired, p)
    assert fail.dtype == np.uint8 and fail.tolist() == want
    assert n_fail == sum(want)
    assert totals.dtype == np.uint64 and totals.shape == (2, 3, 2) and (totals == table.sum(axis=0)).all()
    return want


@pytest.mark.parametrize("par", sorted(PARAMS))
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("count", COUNTS)
def test_bam_nonconv_equals_the_spec(crafted, mapper_on_gold, count, paired, par):
    p = PARAMS[par]
    n = min(N_RECORDS, 2 * count if paired else count)
    recs, tallies, table = crafted["recs"][:n], crafted["tally", p.min_phred][:n], crafted["table", p.min_phred][:n]
    got = mapper_on_gold.bam_nonconv(b"".join(recs), crafted["lens"][:n], paired, *p)
    want = _check(got, recs, tallies, table, paired, p)
    if n <= 257:
        assert got[3].tolist() == nc.totals_of(recs, tallies)                    # (the table's sums are the spec's totals)
    if par == "off":
        assert not any(want)
    elif n == N_RECORDS:
        assert 100 < sum(want) < len(want) - 100 and got[3].all()


def test_the_calls_leave_other_results_alone(crafted, mapper_on_gold):
    """the methylation result and the records of a bmbs_bam_sort call stay as they are"""
    m = mapper_on_gold
    recs = [r for r in crafted["recs"][:3000] if r]
    lens = [len(r) for r in recs]
    sites = m.bam_methyl(b"".join(recs), lens, None, contexts=7, mbias=True).tobytes()
    table = m.methyl_mbias().tobytes()
    m.bam_sort(b"".join(recs), lens, raw=True)
    m.bam_nonconv(b"".join(crafted["recs"][:500]), crafted["lens"][:500], True)
    assert m.methyl_sites().tobytes() == sites and m.methyl_mbias().tobytes() == table
    assert m.bam_sort_methyl(None, contexts=7).tobytes() == sites


@pytest.mark.parametrize("paired", [False, True])
def test_a_stack_of_records_on_200_bases(crafted, mapper_on_gold, gold, paired):
    """20 000 records of 32 bases on the same 200 bases: every group of every block adds to the same few counters of its tally, and
    every total is the sum over all blocks"""
    recs, tallies = crafted["stack"], crafted["stack_tally"]
    got = mapper_on_gold.bam_nonconv(b"".join(recs), [len(r) for r in recs], paired, 3, 60, 4, 0)
    want = _check(got, recs, tallies, _table(recs, tallies), paired, Params(3, 60, 4, 0))
    assert 100 < sum(want) < len(want) - 100 and got[3].sum() > 20_000


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals(crafted, mapper_on_gold, gold):
    from bitmapperbs_amd import capi, mapper
    m = mapper_on_gold
    recs = [r for r in crafted["recs"][:400] if r][:100]
    lens = np.array([len(r) for r in recs], dtype=np.uint32)
    stream = b"".join(recs)
    count, fail, n_fail, totals = m.bam_nonconv(stream, lens, True)
    assert len(count) == 100 and len(fail) == 50 and 0 < n_fail < 50
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 41\b.*36"):
        bad = lens.copy(); bad[42] += bad[41] - 20; bad[41] = 20
        m.bam_nonconv(stream, bad)
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 12\b.*block_size"):
        bad = lens.copy(); bad[12] += 4; bad[13] -= 4
        m.bam_nonconv(stream, bad)
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*add up"):
        m.bam_nonconv(stream[:-1], lens)
    r = bytearray(recs[5]); struct.pack_into("<I", r, 20, len(r))                      # l_seq = the whole record's size
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 5\b.*do not fit"):
        m.bam_nonconv(b"".join(recs[:5]) + bytes(r) + b"".join(recs[6:]), lens)
    r = bytearray(recs[7]); struct.pack_into("<i", r, 4, 2)                            # refID 2 of two sequences
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 7\b.*beyond"):
        m.bam_nonconv(b"".join(recs[:7]) + bytes(r) + b"".join(recs[8:]), lens)
    # (a secondary record is not examined, but its span is checked as every mapped record's is)
    off_end = spec.make_record(1, len(gold["seqs"][1]) - 9, 0x100, [("M", 10)], "ACGTACGTAC", [30] * 10)
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 3\b.*runs off"):
        m.bam_nonconv(b"".join(recs[:3]) + off_end, list(lens[:3]) + [len(off_end)])
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 0\b.*runs off"):
        neg = spec.make_record(0, -1, 0, [("M", 10)], "ACGTACGTAC", [30] * 10)
        m.bam_nonconv(neg, [len(neg)])
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*odd number"):
        m.bam_nonconv(b"".join(recs[:99]), lens[:99], True)
    for bad in (Params(-1, 0, 5, 0), Params(3, -1, 5, 0), Params(3, 101, 5, 0), Params(3, 0, -1, 0), Params(3, 0, 5, -1), Params(3, 0, 5, 256)):
        with pytest.raises(RuntimeError, match=r"bmbs error -22: .*parameters"):
            m.bam_nonconv(stream, lens, False, *bad)
    assert len(m.bam_nonconv(stream, lens, False, 2 ** 31 - 1, 100, 2 ** 31 - 1, 255)[1]) == 100
    # n = 0 is valid, holes only too; NULL parameters are the defaults; a cap that is too small: BMBS_ENOMEM with n_tmpl set
    count, fail, n_fail, totals = m.bam_nonconv(b"", np.zeros(0, dtype=np.uint32))
    assert len(count) == 0 and len(fail) == 0 and n_fail == 0 and not totals.any()
    count, fail, n_fail, totals = m.bam_nonconv(b"", np.zeros(6, dtype=np.uint32), True)
    assert not count["meth"].any() and fail.tolist() == [0, 0, 0] and n_fail == 0 and not totals.any()
    a = np.frombuffer(stream, dtype=np.uint8)
    nt, nf = ctypes.c_int64(0), ctypes.c_int64(0)
    f = np.full(100, 7, dtype=np.uint8)
    assert m._lib.bmbs_bam_nonconv(m._ctx, capi.ptr(a), a.size, capi.ptr(lens), 100, 0, None, None, capi.ptr(f), 99, ctypes.byref(nt), ctypes.byref(nf), None) == -12
    assert nt.value == 100 and (f == 7).all()
    assert m._lib.bmbs_bam_nonconv(m._ctx, capi.ptr(a), a.size, capi.ptr(lens), 100, 0, None, None, None, 0, ctypes.byref(nt), ctypes.byref(nf), None) == -12 and nt.value == 100
    assert m._lib.bmbs_bam_nonconv(m._ctx, capi.ptr(a), a.size, capi.ptr(lens), 100, 0, None, None, capi.ptr(f), 100, ctypes.byref(nt), ctypes.byref(nf), None) == 0
    assert f.tolist() == m.bam_nonconv(stream, lens)[1].tolist() and nf.value == int(f.sum()) > 0
    # no index: BMBS_ESTATE
    bare = mapper.Mapper(None, 0)
    with pytest.raises(RuntimeError, match="bmbs error -1: .*no index"):
        bare.bam_nonconv(stream, lens)
    with pytest.raises(RuntimeError, match="bmbs error -1: .*no index"):
        bare.sorted_nonconv()
    bare.close()


# ---- bmbs_text_sorted_nonconv ---------------------------------------------------------------------------------------------------------------
_COMP = str.maketrans("ACGT", "TGCA")


def _unconverted(gold, fq1, fq2, entries, n):
    """the golden pairs with a share of the reads replaced by what the genome spells where they map (one M operation, on the strand
    the record is on): template t % 4 == 0 both reads, t % 4 == 1 read 2 only; -> the two FASTQ texts, the templates touched"""
    text = ["".join("ACGT"[b] for b in s) for s in gold["seqs"]]
    out, touched = ([], []), set()
    for t in range(n):
        for mate, fq in enumerate((fq1, fq2)):
            seq = fq[t][1]
            rec = entries[2 * t + mate]
            if rec and (t % 4 == 0 or (t % 4 == 1 and mate == 1)):
                ref, pos, _mq, flag, cigar, _b, _q = spec.fields(rec)
                if not flag & 4 and len(cigar) == 1 and cigar[0] == (0, len(seq)):
                    seq = text[ref][pos:pos + len(seq)]
                    if flag & 0x10:
                        seq = seq.translate(_COMP)[::-1]
                    touched.add(t)
            out[mate].append("@t%d/%d\n%s\n+\n%s\n" % (t, mate + 1, seq, fq[t][3]))
    return "".join(out[0]).encode(), "".join(out[1]).encode(), touched


def test_sorted_nonconv_of_a_text_call_equals_the_spec(gold):
    from bitmapperbs_amd import mapper
    M = mapper.Mapper
    fq1, fq2 = tm._fastq_records(os.path.join(GOLD, "pe_p100_1.fq.gz")), tm._fastq_records(os.path.join(GOLD, "pe_p100_2.fq.gz"))
    n = len(fq1)
    t1, t2 = tm._renamed(fq1, "t", "/1")[0].encode(), tm._renamed(fq2, "t", "/2")[0].encode()
    m = M(gold["index"], 0, e_f=0.04, max_ins=520)
    with pytest.raises(RuntimeError, match="bmbs error -1:"):
        m.sorted_nonconv()                                                    # no sorted call yet

    def unsorted_entries(a, b):
        return tm._by_template(split_records(b"".join(raw for _, raw in bgzf_blocks(m.map_text(a, n, b, flags=M.TEXT_BAM)))), n, True, "t")

    def check(a, b, p):
        entries = unsorted_entries(a, b)
        want = nc.templates(gold["seqs"], entries, True, p)
        got = split_records(m.map_text(a, n, b, flags=M.TEXT_BAM | M.TEXT_BAM_SORTED))
        fail, n_failed, totals = m.sorted_nonconv(*p)
        assert fail.size == len(got) == sum(1 for r in entries if r)
        assert fail.tolist() == [want[int(tm._name(r)[1:])] for r in got]
        assert n_failed == sum(want) and totals.tolist() == nc.totals(gold["seqs"], entries, p.min_phred)
        return want, totals

    plain, tot_plain = check(t1, t2, nc.DEFAULTS)
    u1, u2, touched = _unconverted(gold, fq1, fq2, unsorted_entries(t1, t2), n)
    assert len(touched) > n // 4
    want, tot = check(u1, u2, nc.DEFAULTS)
    assert sum(want) > sum(plain) + n // 8 and sum(want) < n - n // 8
    assert sum(1 for t in touched if want[t]) > n // 4                               # the unconverted copies are what fails ...
    assert any(want[t] for t in touched if t % 4 == 1)                                # ... read 2 alone too
    assert tot[:, 1:, 1].sum() > tot_plain[:, 1:, 1].sum() + 1000
    # both switches off: all-zero verdicts, the same totals; other parameters
    off, tot_off = check(u1, u2, Params(0, 0, 5, 0))
    assert not any(off) and (tot_off == tot).all()
    check(u1, u2, Params(0, 50, 5, 20))
    # the call leaves the sorted call's other results as they are, and needs its buffers
    clip = m.sorted_clip()
    m.sorted_nonconv()
    assert (m.sorted_clip() == clip).all() and m.sorted_index()[0].size == clip.size
    # a single-end call: every record is its own template
    got = split_records(m.map_text(u1, n, None, flags=M.TEXT_BAM | M.TEXT_BAM_SORTED))
    fail, n_failed, totals = m.sorted_nonconv()
    by_rec = nc.templates(gold["seqs"], got, False)
    assert fail.tolist() == by_rec and n_failed == sum(by_rec) > n // 8 and totals.tolist() == nc.totals(gold["seqs"], got)
    m.map_text(t1, n, t2, flags=M.TEXT_BAM)
    with pytest.raises(RuntimeError, match="bmbs error -1:"):
        m.sorted_nonconv()                                                    # a call that rewrites the buffers
    m.close()


# ---- the driver -------------------------------------------------------------------------------------------------------------------------------
def _shown(text, lo, hi, ob, keep_all):
    """the bases lo .. hi - 1 of one sequence as a bisulfite read shows them on the forward strand: a cytosine of the read's strand (C
    for OT, G for OB) in CpG context stays when its position is even, every other one reads T (A) -- or, keep_all, every one stays:
    a read the treatment did not convert"""
    if keep_all:
        return text[lo:hi]
    out = bytearray(text[lo:hi])
    for p in range(lo, hi):
        if ob and text[p:p + 1] == b"G" and not (p % 2 == 0 and text[p - 1:p] == b"C"):
            out[p - lo] = ord("A")
        if not ob and text[p:p + 1] == b"C" and not (p % 2 == 0 and text[p + 1:p + 2] == b"G"):
            out[p - lo] = ord("T")
    return bytes(out)


def _reads(gold, n_se, n_pe, L=100):
    """error-free reads in the manner of test_methyl._planted_reads (directional library, fragments of 120..320 bases); read or pair
    i % 5 == 0 is unconverted, of pair i % 5 == 1 read 2 alone"""
    rng = np.random.default_rng(29)
    texts = [t.encode() for t in ("".join(b.split("\n")[1:]).upper() for b in open(gold["fa"]).read().split(">")[1:])]
    q = "I" * L
    se, pe1, pe2 = [], [], []
    for i in range(n_se):
        ref = int(rng.integers(0, len(texts))); p = int(rng.integers(2, len(texts[ref]) - L - 2)); ob = bool(rng.integers(0, 2))
        s = _shown(texts[ref], p, p + L, ob, i % 5 == 0)
        if ob:
            s = s.translate(tm._COMP)[::-1]
        se.append("@s%d_%d_%d_%d\n%s\n+\n%s\n" % (i, ref, p, ob, s.decode(), q))
    for i in range(n_pe):
        ref = int(rng.integers(0, len(texts))); F = int(rng.integers(120, 321)); p = int(rng.integers(2, len(texts[ref]) - F - 2)); ob = bool(rng.integers(0, 2))
        # (the left read of the fragment is read 1 of an OT pair and read 2 of an OB pair)
        keep_left, keep_right = (i % 5 == 0 or (i % 5 == 1 and ob)), (i % 5 == 0 or (i % 5 == 1 and not ob))
        left = _shown(texts[ref], p, p + L, ob, keep_left)
        right = _shown(texts[ref], p + F - L, p + F, ob, keep_right).translate(tm._COMP)[::-1]
        r1, r2 = (right, left) if ob else (left, right)
        nm = "p%d_%d_%d_%d" % (i, ref, p, ob)
        pe1.append("@%s/1\n%s\n+\n%s\n" % (nm, r1.decode(), q)); pe2.append("@%s/2\n%s\n+\n%s\n" % (nm, r2.decode(), q))
    return "".join(se), "".join(pe1), "".join(pe2)


def _serial(rec):
    return int(tm._name(rec).decode().split("_")[0][1:])


def _entries(recs, n, paired):
    """the records of a sorted file by template: entry i, or entries 2 i (read 1) and 2 i + 1 (read 2); b"" where there is none"""
    out = [b""] * (2 * n if paired else n)
    for r in recs:
        at = 2 * _serial(r) + (1 if spec.fields(r)[3] & 0x80 else 0) if paired else _serial(r)
        assert not out[at]
        out[at] = r
    return out


def _clips(recs, paired):
    if not paired:
        return None
    by_name = {(tm._name(r), spec.fields(r)[3] & 0xc0): r for r in recs}
    return [spec.clip_of(r, by_name.get((tm._name(r), spec.fields(r)[3] & 0xc0 ^ 0xc0))) for r in recs]


@pytest.mark.parametrize("kind,more", [("se", []), ("pe", ["--markdup", "--mbias"])])
def test_driver_flags_the_failed_templates_and_every_later_stage_leaves_them_out(gold, tmp_path, kind, more):
    n_se, n_pe = 300, 250
    se, pe1, pe2 = _reads(gold, n_se, n_pe)
    paired = kind == "pe"
    if paired:
        open(tmp_path / "1.fq", "w").write(pe1); open(tmp_path / "2.fq", "w").write(pe2)
        inputs, args, n = ["--seq1", str(tmp_path / "1.fq"), "--seq2", str(tmp_path / "2.fq")], json.load(open(os.path.join(GOLD, "pe_args.json")))["p100"], n_pe
    else:
        open(tmp_path / "r.fq", "w").write(se)
        inputs, args, n = ["--seq", str(tmp_path / "r.fq")], golden_args()["b150"], n_se
    base = args + ["--sort", "--bai"] + more
    pre0, pre1, rep = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "conv.txt")
    tm._run(gold["fa"], inputs, base + ["--methyl", pre0] + tm.ALL_CONTEXTS, pre0 + ".bam")
    err = tm._run(gold["fa"], inputs, base + ["--methyl", pre1] + tm.ALL_CONTEXTS + ["--filter-non-conversion", "--conversion-report", rep], pre1 + ".bam")
    recs0, recs1 = split_records(bam_payload(pre0 + ".bam")[1]), split_records(bam_payload(pre1 + ".bam")[1])
    # the spec on the run without the option: which templates fail
    entries = _entries(recs0, n, paired)
    failed = nc.templates(gold["seqs"], entries, paired)
    planted = [i for i in range(n) if i % 5 == 0 or (paired and i % 5 == 1)]
    assert sum(failed[i] for i in planted) > len(planted) // 2 and sum(failed) < n // 2
    assert not paired or any(failed[i] for i in planted if i % 5 == 1)
    # the records of exactly those templates carry 0x200, mates included; nothing else differs, the order is the same
    assert len(recs0) == len(recs1)
    want = [nc.mark([r], False, [failed[_serial(r)]])[0] for r in recs0]
    assert recs1 == want and recs1 != recs0
    assert not any(spec.fields(r)[3] & 0x200 for r in recs0)
    if paired:
        by_tmpl = {}
        for r in recs1:
            by_tmpl.setdefault(_serial(r), set()).add(bool(spec.fields(r)[3] & 0x200))
        assert all(len(v) == 1 for v in by_tmpl.values())
    # the index: right for its file, with the bins, chunk counts, windows and per-reference counts of the run without the option
    bai0, bai1 = open(pre0 + ".bam.bai", "rb").read(), open(pre1 + ".bam.bai", "rb").read()
    assert bai1 == bai_spec.spec_bai(pre1 + ".bam")
    shape = lambda b: [({k: len(v) for k, v in r["bins"].items()}, len(r["lin"]), r["meta"] and r["meta"][2:]) for r in bai_spec.parse_bai(b)["refs"]]
    assert shape(bai0) == shape(bai1)
    # bedGraphs and M-bias table: the spec on the flagged file's records; they differ from the unfiltered run's
    clip = _clips(recs1, paired)
    sites = spec.sites(gold["seqs"], recs1, clip, contexts=7)
    assert tm._files(pre1) == tm._spec_files(pre1, gold["names"], sites)
    assert tm._files(pre0) == tm._spec_files(pre0, gold["names"], spec.sites(gold["seqs"], recs0, _clips(recs0, paired), contexts=7))
    assert [f.split(b"\n", 1)[1] for f in tm._files(pre1)] != [f.split(b"\n", 1)[1] for f in tm._files(pre0)]
    if "--mbias" in more:
        t1 = open(pre1 + "_mbias.tsv", "rb").read()
        assert t1 == mbias_spec.tsv(mbias_spec.table_of(mbias_spec.walk(gold["seqs"], recs1, clip), 7)) != open(pre0 + "_mbias.tsv", "rb").read()
    # the report and the --verbose line
    assert open(rep, "rb").read() == nc.report_text(nc.totals(gold["seqs"], entries), n, sum(failed))
    got = re.search(r"nonconv: templates (\d+), failed (\d+)", err)
    assert got and [int(x) for x in got.groups()] == [n, sum(failed)]


def test_driver_conversion_report_alone_flags_nothing_and_other_parameters(gold, tmp_path):
    se, _pe1, _pe2 = _reads(gold, 200, 0)
    open(tmp_path / "r.fq", "w").write(se)
    inputs, args = ["--seq", str(tmp_path / "r.fq")], golden_args()["b150"] + ["--sort"]
    out, rep = str(tmp_path / "o.bam"), str(tmp_path / "conv.txt")
    tm._run(gold["fa"], inputs, args + ["--conversion-report", rep], out)
    recs = split_records(bam_payload(out)[1])
    assert recs and not any(spec.fields(r)[3] & 0x200 for r in recs)
    entries = _entries(recs, 200, False)
    assert open(rep, "rb").read() == nc.report_text(nc.totals(gold["seqs"], entries), 200, 0)
    # each parameter implies the switch; a threshold no read reaches with the percent rule on
    p = Params(0, 40, 7, 0)
    tm._run(gold["fa"], inputs, args + ["--non-conversion-threshold", "0", "--non-conversion-percent", "40", "--non-conversion-min-count", "7", "--conversion-report", rep], out)
    failed = nc.templates(gold["seqs"], entries, False, p)
    assert split_records(bam_payload(out)[1]) == nc.mark(recs, False, [failed[_serial(r)] for r in recs]) and 20 < sum(failed) < 100
    assert open(rep, "rb").read() == nc.report_text(nc.totals(gold["seqs"], entries), 200, sum(failed))
    tm._run(gold["fa"], inputs, args + ["--non-conversion-threshold", "1000"], out)
    assert split_records(bam_payload(out)[1]) == recs


def test_driver_refusals(gold, tmp_path):
    open(tmp_path / "r.fq", "w").write(_reads(gold, 4, 0)[0])
    rep = str(tmp_path / "conv.txt")
    for bad, named in ((["--bam", "--filter-non-conversion"], "--filter-non-conversion"), (["--bam", "--non-conversion-percent", "50"], "need --sort"),
                       (["--bam", "--conversion-report", rep], "--conversion-report needs --sort"), (["--sort", "--filter-non-conversion"], "--sort needs --bam"),
                       (["--bam", "--sort", "--non-conversion-percent", "101"], "--non-conversion-percent takes 0..100"),
                       (["--bam", "--sort", "--non-conversion-threshold", "-1"], "--non-conversion-threshold takes"),
                       (["--bam", "--sort", "--non-conversion-min-count", "x"], "--non-conversion-min-count takes"),
                       (["--bam", "--sort", "--filter-non-conversions"], "unsupported option")):
        p = subprocess.run([tm._driver(), "--search", gold["fa"], "--seq", str(tmp_path / "r.fq"), "-o", str(tmp_path / "x.bam")] + bad, capture_output=True, text=True)
        assert p.returncode == 2 and named in p.stderr, (bad, p.stderr)
    assert not os.path.exists(rep) and not os.path.exists(str(tmp_path / "x.bam"))
