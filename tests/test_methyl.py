"""Methylation counts on the device (`bmbs_search --bam --sort --methyl`, bmbs_bam_methyl, bmbs_bam_sort_methyl, bmbs_methyl_sites,
bmbs_text_sorted_clip) against tests/methyl_spec.py.  Sites and counts are integers, files are bytes: every comparison here is exact."""
import ctypes
import gzip
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bai_spec
import markdup_spec
import methyl_spec as spec
from common import GOLD, ROOT, bam_payload, bgzf_blocks, golden_args, gunzip_to
from test_sorted_bam import split_records

pytestmark = pytest.mark.gpu

MIN_MAPQ, MIN_PHRED = 10, 5
L_SEQS = (1, 2, 31, 32, 33, 63, 64, 65, 151, 998)
COUNTS = (1, 63, 64, 65, 257, 20_000)
# paired-proper on all four strand / read combinations, single end on both strands, and what keeps a record out: unmapped, secondary,
# QC-fail, duplicate, supplementary, paired but not proper, paired without a read number
FLAGS = (0, 16, 0x43, 0x53, 0x83, 0x93, 0x63, 0xa3, 4, 0x100, 0x210, 0x400, 0x443, 0x800, 0x41, 0x91, 0x13)


@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    """the golden genome's index, built once; its sequences as the index holds them"""
    from bitmapperbs_amd import mapper
    wd = tmp_path_factory.mktemp("methyl_gold")
    fa = str(wd / "genome.fa")
    gunzip_to(os.path.join(GOLD, "genome.fa.gz"), fa)
    mapper.Index.build(fa, fa, threads=4)
    ix = mapper.Index(fa)
    seqs = spec.genome_of_pac(ctypes.string_at(ix.view.pac, int(ix.view.pac_bytes)), ix.chrom_len)
    text = "".join(l.strip() for l in open(fa) if not l.startswith(">"))
    assert b"".join(seqs) == bytes("ACGT".index(c) for c in text.upper())           # (the golden genome has no other letter)
    return dict(fa=fa, index=ix, seqs=seqs, names=ix.chrom_names)


@pytest.fixture(scope="module")
def mapper_on_gold(gold):
    from bitmapperbs_amd import mapper
    m = mapper.Mapper(gold["index"], 0)
    yield m
    m.close()


def _site_tuples(a):
    return [(int(r["ref"]), int(r["pos"]), int(r["meth"]), int(r["unmeth"]), int(r["kind"])) for r in a]


# ---- 1. crafted records -------------------------------------------------------------------------------------------------------------------
READ_OPS, REF_OPS = (0, 1, 4, 7, 8), (0, 2, 3, 7, 8)


def _random_record(rng, seqs, stack=False):
    """one record whose bases follow the genome with the cytosines of its strand converted or not at random: l_seq of L_SEQS, 0..6 CIGAR
    operations of every kind (the read-consuming ones add up to l_seq, now and then to more), a name of 1..40 characters, a position
    anywhere its span fits -- one time in three at the sequence's first or last base; stack: on the first 200 bases of sequence 0"""
    l_seq = 32 if stack else L_SEQS[int(rng.integers(0, len(L_SEQS)))]
    n_ops = int(rng.integers(1, 4)) if stack else int(rng.integers(0, 7))
    ops = [int(rng.integers(0, 9)) for _ in range(n_ops)]
    if n_ops and not any(o in READ_OPS for o in ops):
        ops[int(rng.integers(0, n_ops))] = 0
    on_read = [k for k, o in enumerate(ops) if o in READ_OPS]
    lens = [int(rng.integers(1, 12)) for _ in ops]
    if on_read:
        # l_seq dealt out over the read-consuming operations (at least 1 each: the surplus of a short read stays, a CIGAR that asks for more)
        cuts = sorted(int(x) for x in rng.integers(0, l_seq + 1, len(on_read) - 1))
        for k, a, b in zip(on_read, [0] + cuts, cuts + [l_seq]):
            lens[k] = max(1, b - a)
    cigar = list(zip(ops, lens))
    span = spec.ref_span(cigar)
    ref = 0 if stack else int(rng.integers(0, len(seqs)))
    room = (200 if stack else len(seqs[ref])) - span
    assert room >= 0
    r = rng.random()
    pos = 0 if r < 0.17 and not stack else room if r < 0.34 and not stack else int(rng.integers(0, room + 1))
    flag = FLAGS[int(rng.integers(0, 8))] if rng.random() < 0.8 else FLAGS[int(rng.integers(8, len(FLAGS)))]
    ob = spec.is_ob(flag)
    # the bases: the genome's under M = X, random elsewhere; the strand's cytosines stay or convert, 3 % of all bases are errors
    codes = rng.integers(0, 4, l_seq).astype(np.uint8)
    rp, ip = pos, 0
    for op, ln in cigar:
        if op in (0, 7, 8):
            take = max(0, min(ln, l_seq - ip))
            codes[ip:ip + take] = np.frombuffer(seqs[ref][rp:rp + take], dtype=np.uint8)
        rp += ln if op in REF_OPS else 0
        ip += ln if op in READ_OPS else 0
    conv = rng.random(l_seq) < 0.5
    codes = np.where(conv & (codes == (2 if ob else 1)), 0 if ob else 3, codes)       # G -> A on OB, C -> T on OT
    err = rng.random(l_seq) < 0.03
    codes = np.where(err, rng.integers(0, 4, l_seq), codes)
    bam = np.array([1, 2, 4, 8], dtype=np.uint8)[codes]
    bam[rng.random(l_seq) < 0.01] = 15                                                # N
    q = rng.integers(0, 42, l_seq).astype(np.uint8)
    q[rng.random(l_seq) < 0.05] = MIN_PHRED - 1
    q[rng.random(l_seq) < 0.05] = MIN_PHRED
    q[rng.random(l_seq) < 0.05] = 0xff
    name = bytes(rng.integers(97, 123, int(rng.integers(1, 41))).astype(np.uint8))
    mapq = int(rng.choice([MIN_MAPQ - 1, MIN_MAPQ, 3, 30, 42, 60], p=[0.05, 0.05, 0.05, 0.35, 0.3, 0.2]))
    return spec.make_record(ref, pos, flag, cigar, bam.tolist(), q.tobytes(), name, mapq)


def _random_clip(rng, rec):
    """a clip inside the record's span, for one record in three"""
    span = spec.ref_span(spec.fields(rec)[4])
    if rng.random() < 0.67 or span == 0:
        return 0
    off = int(rng.integers(0, span))
    return off << 16 | int(rng.integers(1, span - off + 1))


@pytest.fixture(scope="module")
def crafted(gold):
    """20 000 random records (every 11th entry a hole) and 20 000 stacked on 200 bases, their clips, and what the spec says of them with
    every context selected, with and without the clips -- computed once"""
    rng = np.random.default_rng(5)
    seqs = gold["seqs"]
    recs = [b"" if i % 11 == 6 else _random_record(rng, seqs) for i in range(COUNTS[-1])]
    clip = [_random_clip(rng, r) if r else 0 for r in recs]
    stack = [_random_record(rng, seqs, stack=True) for _ in range(COUNTS[-1])]
    starts = np.cumsum([0] + [len(r) for r in recs[:-1]])
    assert len({int(s) % 16 for s, r in zip(starts, recs) if r}) == 16
    kw = dict(contexts=7, min_mapq=MIN_MAPQ, min_phred=MIN_PHRED)
    want = {}
    for n in COUNTS:
        want[n, True] = spec.sites(seqs, recs[:n], clip[:n], **kw)
        want[n, False] = spec.sites(seqs, recs[:n], None, **kw)
    return dict(recs=recs, clip=clip, stack=stack, want=want, stack_want=spec.sites(seqs, stack, None, **kw))


def test_the_crafted_records_are_not_trivial(crafted, gold):
    all_sites = crafted["want"][COUNTS[-1], True]
    for ctx in range(3):
        for strand in range(2):
            assert sum(1 for s in all_sites if s[4] == ctx | strand << 2) > 100
    assert any(s[2] and s[3] for s in all_sites)
    why = [spec.skip_reason(r, MIN_MAPQ) for r in crafted["recs"]]
    for reason in ("none", "unmapped", "flag", "cigar", "mapq", "improper", None):
        assert why.count(reason) > 20, reason
    assert len(crafted["want"][COUNTS[-1], False]) > len(all_sites)                   # the clips took calls away
    # positions at both ends of both sequences, and CIGARs of every operation
    ends = {(spec.fields(r)[0], spec.fields(r)[1] == 0) for r in crafted["recs"] if r}
    assert ends == {(0, False), (0, True), (1, False), (1, True)}
    lens = [len(s) for s in gold["seqs"]]
    assert {spec.fields(r)[0] for r in crafted["recs"] if r and spec.fields(r)[4] and spec.fields(r)[1] + spec.ref_span(spec.fields(r)[4]) == lens[spec.fields(r)[0]]} == {0, 1}
    assert {op for r in crafted["recs"] if r for op, _ in spec.fields(r)[4]} == set(range(9))
    # the stack: a site's events fill more than one workgroup of the reduction
    assert max(s[2] + s[3] for s in crafted["stack_want"]) > 2 * 256 and all(s[1] < 200 and s[0] == 0 for s in crafted["stack_want"])


@pytest.mark.parametrize("clipped", [True, False])
@pytest.mark.parametrize("count", COUNTS)
def test_bam_methyl_equals_the_spec(crafted, mapper_on_gold, count, clipped):
    recs = crafted["recs"][:count]
    got = mapper_on_gold.bam_methyl(b"".join(recs), [len(r) for r in recs], crafted["clip"][:count] if clipped else None, contexts=7,
                                    min_mapq=MIN_MAPQ, min_phred=MIN_PHRED)
    assert _site_tuples(got) == crafted["want"][count, clipped]
    assert not got["pad"].any()


@pytest.fixture(scope="module")
def first_3000(crafted, gold):
    recs, clip = crafted["recs"][:3000], crafted["clip"][:3000]
    return recs, clip, spec.sites(gold["seqs"], recs, clip, contexts=7, min_mapq=MIN_MAPQ, min_phred=MIN_PHRED)


@pytest.mark.parametrize("contexts", [1, 2, 3, 4, 5, 6, 7])
def test_each_context_selection(first_3000, mapper_on_gold, contexts):
    recs, clip, all_sites = first_3000
    got = mapper_on_gold.bam_methyl(b"".join(recs), [len(r) for r in recs], clip, contexts=contexts, min_mapq=MIN_MAPQ, min_phred=MIN_PHRED)
    want = spec.select(all_sites, contexts)
    assert _site_tuples(got) == want and 0 < len(want) and (contexts == 7 or len(want) < len(all_sites))


def test_other_thresholds(crafted, mapper_on_gold, gold):
    recs = crafted["recs"][:2000]
    for mq, ph in ((0, 0), (MIN_MAPQ + 1, MIN_PHRED + 1), (43, 41)):
        got = mapper_on_gold.bam_methyl(b"".join(recs), [len(r) for r in recs], None, contexts=7, min_mapq=mq, min_phred=ph)
        assert _site_tuples(got) == spec.sites(gold["seqs"], recs, None, contexts=7, min_mapq=mq, min_phred=ph)


def test_a_stack_of_records_on_200_bases_in_one_call_and_in_slices(crafted, gold):
    """20 000 records on the same 200 bases: every site's run of events crosses waves and workgroups; with BMBS_METHYL_EVENTS the same
    records go through in slices whose sites are merged (a child process: the variable is read once)"""
    from bitmapperbs_amd import mapper
    m = mapper.Mapper(gold["index"], 0)
    recs = crafted["stack"]
    got = m.bam_methyl(b"".join(recs), [len(r) for r in recs], None, contexts=7, min_mapq=MIN_MAPQ, min_phred=MIN_PHRED)
    assert _site_tuples(got) == crafted["stack_want"]
    # bmbs_bam_sort_methyl reads the records bmbs_bam_sort left on the device, clips in that call's input order
    some, clip = crafted["recs"][:5000], crafted["clip"][:5000]
    keep = [i for i, r in enumerate(some) if r]
    m.bam_sort(b"".join(some[i] for i in keep), [len(some[i]) for i in keep], raw=True)
    got = m.bam_sort_methyl([clip[i] for i in keep], contexts=7, min_mapq=MIN_MAPQ, min_phred=MIN_PHRED)
    assert _site_tuples(got) == spec.sites(gold["seqs"], some, clip, contexts=7, min_mapq=MIN_MAPQ, min_phred=MIN_PHRED)
    m.bam_sort(b"".join(some[i] for i in keep), [len(some[i]) for i in keep])
    assert m.bam_sort_methyl(None, contexts=1).tobytes() == m.bam_methyl(b"".join(some), [len(r) for r in some], None, contexts=1).tobytes()
    m.close()


SLICE_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from bitmapperbs_amd import mapper
d = np.load(sys.argv[3], allow_pickle=False)
m = mapper.Mapper(mapper.Index(sys.argv[2]), 0)
got = m.bam_methyl(d["stream"].tobytes(), d["lens"], d["clip"], contexts=7, min_mapq=int(sys.argv[5]), min_phred=int(sys.argv[6]))
np.save(sys.argv[4], got)
m.close()
"""


def test_slices_of_records_give_the_same_sites(crafted, gold, tmp_path):
    recs = crafted["recs"][:5000] + crafted["stack"][:5000]
    clip = crafted["clip"][:5000] + [0] * 5000
    np.savez(tmp_path / "in.npz", stream=np.frombuffer(b"".join(recs), dtype=np.uint8), lens=np.array([len(r) for r in recs], dtype=np.uint32),
             clip=np.array(clip, dtype=np.uint32))
    open(tmp_path / "child.py", "w").write(SLICE_CHILD)
    p = subprocess.run([os.sys.executable, str(tmp_path / "child.py"), ROOT, gold["fa"], str(tmp_path / "in.npz"), str(tmp_path / "out.npy"), str(MIN_MAPQ), str(MIN_PHRED)],
                       capture_output=True, text=True, env=dict(os.environ, BMBS_METHYL_EVENTS="5000"))
    assert p.returncode == 0, p.stderr
    want = spec.sites(gold["seqs"], recs, clip, contexts=7, min_mapq=MIN_MAPQ, min_phred=MIN_PHRED)
    n_events = sum(s[2] + s[3] for s in want)
    assert n_events > 10 * 5000                                                        # more than ten slices
    assert _site_tuples(np.load(tmp_path / "out.npy")) == want


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(crafted, mapper_on_gold, gold):
    from bitmapperbs_amd import mapper
    m = mapper_on_gold
    recs = [r for r in crafted["recs"][:400] if r][:100]
    lens = np.array([len(r) for r in recs], dtype=np.uint32)
    stream = b"".join(recs)
    assert len(m.bam_methyl(stream, lens)) > 0
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 41\b.*36"):
        bad = lens.copy(); bad[42] += bad[41] - 20; bad[41] = 20
        m.bam_methyl(stream, bad)
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 12\b.*block_size"):
        bad = lens.copy(); bad[12] += 4; bad[13] -= 4
        m.bam_methyl(stream, bad)
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*add up"):
        m.bam_methyl(stream[:-1], lens)
    r = bytearray(recs[5]); struct.pack_into("<I", r, 20, len(r))                      # l_seq = the whole record's size
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 5\b.*do not fit"):
        m.bam_methyl(b"".join(recs[:5]) + bytes(r) + b"".join(recs[6:]), lens)
    r = bytearray(recs[7]); struct.pack_into("<i", r, 4, 2)                            # refID 2 of two sequences
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 7\b.*beyond"):
        m.bam_methyl(b"".join(recs[:7]) + bytes(r) + b"".join(recs[8:]), lens)
    off_end = spec.make_record(1, len(gold["seqs"][1]) - 9, 0, [("M", 10)], "ACGTACGTAC", [30] * 10)
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 3\b.*runs off"):
        m.bam_methyl(b"".join(recs[:3]) + off_end, list(lens[:3]) + [len(off_end)])
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*record 0\b.*runs off"):
        neg = spec.make_record(0, -1, 0, [("M", 10)], "ACGTACGTAC", [30] * 10)
        m.bam_methyl(neg, [len(neg)])
    with pytest.raises(RuntimeError, match=r"bmbs error -22: .*parameters"):
        m.bam_methyl(stream, lens, contexts=8)
    with pytest.raises(RuntimeError, match="bmbs error -1:"):
        m.methyl_sites()                                                               # the failed call left no result
    # n = 0 is valid, holes only too
    assert len(m.bam_methyl(b"", np.zeros(0, dtype=np.uint32))) == 0 and len(m.bam_methyl(b"", np.zeros(5, dtype=np.uint32))) == 0
    assert len(m.methyl_sites()) == 0
    # no index: BMBS_ESTATE
    bare = mapper.Mapper(None, 0)
    with pytest.raises(RuntimeError, match="bmbs error -1: .*no index"):
        bare.bam_methyl(stream, lens)
    bare.bam_sort(stream, lens, raw=True)
    with pytest.raises(RuntimeError, match="bmbs error -1: .*no index"):
        bare.bam_sort_methyl()
    bare.close()
    # bmbs_bam_sort_methyl: no sort call yet on a fresh context; after one it works; after a failed one, or another call that used the
    # sort's buffers (a sorted text call), BMBS_ESTATE again
    m2 = mapper.Mapper(gold["index"], 0)
    with pytest.raises(RuntimeError, match="bmbs error -1: .*resident"):
        m2.bam_sort_methyl()
    m2.bam_sort(stream, lens)
    assert m2.bam_sort_methyl().tobytes() == m.bam_methyl(stream, lens).tobytes()
    text = ("".join("@%s\n%s\n+\n%s\n" % (r[0][1:], r[1], r[3]) for r in _fastq_records(os.path.join(GOLD, "se_b150.fq.gz"))[:20])).encode()
    assert len(split_records(m2.map_text(text, 20, None, flags=m2.TEXT_BAM | m2.TEXT_BAM_SORTED))) > 10
    with pytest.raises(RuntimeError, match="bmbs error -1: .*resident"):
        m2.bam_sort_methyl()
    m2.bam_sort(stream, lens, raw=True)
    assert len(m2.bam_sort_methyl()) > 0
    with pytest.raises(RuntimeError):
        bad = lens.copy(); bad[41] = 20
        m2.bam_sort(stream, bad)
    with pytest.raises(RuntimeError, match="bmbs error -1: .*resident"):
        m2.bam_sort_methyl()
    m2.close()


# ---- 3. bmbs_text_sorted_clip -----------------------------------------------------------------------------------------------------------------
def _fastq_records(path):
    lines = gzip.open(path, "rt").read().split("\n")
    return [lines[i:i + 4] for i in range(0, len(lines) - 3, 4)]


def _name(rec):
    return rec[36:36 + rec[12] - 1]


def _renamed(recs, tag, mate=""):
    return "".join("@%s%d%s\n%s\n+\n%s\n" % (tag, i, mate, r[1], r[3]) for i, r in enumerate(recs)), len(recs)


def _by_template(records, n_tmpl, paired, tag):
    """the records of a run's unsorted output, in order -> 1 or 2 entries per template, b"" where a template's line printed nothing"""
    out = []
    at = 0
    for t in range(n_tmpl):
        nm = b"%s%d" % (tag.encode(), t)
        for _ in range(2 if paired else 1):
            if at < len(records) and _name(records[at]) == nm:
                out.append(records[at]); at += 1
            else:
                out.append(b"")
    assert at == len(records)
    return out


def _clip_by_record(entries):
    """the spec's clip of every record of a paired run, keyed by the record's bytes' identity (name, flag)"""
    cl = spec.clips(entries)
    return {(_name(r), struct.unpack_from("<H", r, 18)[0]): c for r, c in zip(entries, cl) if r}


def test_sorted_clip_of_a_text_call_equals_the_spec(gold):
    from bitmapperbs_amd import mapper
    M = mapper.Mapper
    t1, n = _renamed(_fastq_records(os.path.join(GOLD, "pe_p100_1.fq.gz")), "t", "/1")
    t2, _ = _renamed(_fastq_records(os.path.join(GOLD, "pe_p100_2.fq.gz")), "t", "/2")
    t1, t2 = t1.encode(), t2.encode()
    m = M(gold["index"], 0, e_f=0.04, max_ins=520)
    with pytest.raises(RuntimeError, match="bmbs error -1:"):
        m.sorted_clip()                                                       # no sorted call yet
    unsorted = split_records(b"".join(raw for _, raw in bgzf_blocks(m.map_text(t1, n, t2, flags=M.TEXT_BAM))))
    entries = _by_template(unsorted, n, True, "t")
    want = _clip_by_record(entries)
    got = split_records(m.map_text(t1, n, t2, flags=M.TEXT_BAM | M.TEXT_BAM_SORTED))
    clip = m.sorted_clip()
    assert clip.size == len(got)
    flags = [struct.unpack_from("<H", r, 18)[0] for r in got]
    assert clip.tolist() == [want[_name(r), f] for r, f in zip(got, flags)]
    assert not any(c for c, f in zip(clip.tolist(), flags) if not f & 0x80)            # all zero for read 1
    assert sum(1 for c in clip.tolist() if c) > 50                                    # mates of the golden pairs do overlap
    assert any(c >> 16 for c in clip.tolist()) and any(c and not c >> 16 for c in clip.tolist())
    # a single-end call has no clips; a call that rewrites the buffers: BMBS_ESTATE
    m.map_text(t1, n, None, flags=M.TEXT_BAM | M.TEXT_BAM_SORTED)
    assert not m.sorted_clip().any()
    m.map_text(t1, n, t2, flags=M.TEXT_BAM)
    with pytest.raises(RuntimeError, match="bmbs error -1:"):
        m.sorted_clip()
    m.close()


# ---- the driver -------------------------------------------------------------------------------------------------------------------------------
def _driver():
    p = os.path.join(ROOT, "bitmapperbs_amd", "bmbs_search")
    assert os.path.exists(p), "bmbs_search not built (make -C bitmapperbs_amd/csrc)"
    return p


def _run(index, inputs, args, out, env=None):
    cmd = [_driver(), "--search", index] + inputs + ["-o", out, "--verbose", "--bam"] + args
    p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stderr
    return p.stderr


ALL_CONTEXTS = ["--CpG", "--CHG", "--CHH"]


def _files(prefix):
    return [open("%s_%s.bedGraph" % (prefix, c), "rb").read() for c in spec.CONTEXT_NAMES]


def _spec_files(prefix, names, sites):
    return [spec.bedgraph(prefix, c, names, sites) for c in range(3)]


# ---- 4. planted truth ---------------------------------------------------------------------------------------------------------------------------
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _planted(text, lo, hi, ob):
    """the bases lo .. hi - 1 of one sequence as a bisulfite read shows them on the forward strand: a cytosine of the read's strand (C
    for OT, G for OB) stays exactly when its position is a multiple of 3, else it reads T (A)"""
    a, b = (b"G", b"A") if ob else (b"C", b"T")
    return b"".join(b if text[p:p + 1] == a and p % 3 else text[p:p + 1] for p in range(lo, hi))


def _planted_reads(gold, n_se, n_pe, L=100):
    """error-free reads of both strands, single and paired (directional library: an OT pair is read 1 forward + read 2 reverse, an OB
    pair read 1 reverse + read 2 forward; fragments of 120..320 bases, so some mates overlap); the name says where a read comes from"""
    rng = np.random.default_rng(11)
    fa = [l.strip().encode() for l in open(gold["fa"])]
    texts, cur = [], []
    for l in fa:
        if l.startswith(b">"):
            if cur:
                texts.append(b"".join(cur))
            cur = []
        else:
            cur.append(l.upper())
    texts.append(b"".join(cur))
    q = "I" * L
    se, pe1, pe2 = [], [], []
    for i in range(n_se):
        ref = int(rng.integers(0, len(texts))); p = int(rng.integers(0, len(texts[ref]) - L)); ob = bool(rng.integers(0, 2))
        s = _planted(texts[ref], p, p + L, ob)
        if ob:
            s = s.translate(_COMP)[::-1]
        se.append("@s%d_%d_%d_%d\n%s\n+\n%s\n" % (i, ref, p, ob, s.decode(), q))
    for i in range(n_pe):
        ref = int(rng.integers(0, len(texts))); F = int(rng.integers(120, 321)); p = int(rng.integers(0, len(texts[ref]) - F)); ob = bool(rng.integers(0, 2))
        left, right = _planted(texts[ref], p, p + L, ob), _planted(texts[ref], p + F - L, p + F, ob).translate(_COMP)[::-1]
        r1, r2 = (right, left) if ob else (left, right)
        p1, p2 = (p + F - L, p) if ob else (p, p + F - L)
        nm = "p%d_%d_%d_%d_%d" % (i, ref, p1, p2, ob)
        pe1.append("@%s/1\n%s\n+\n%s\n" % (nm, r1.decode(), q)); pe2.append("@%s/2\n%s\n+\n%s\n" % (nm, r2.decode(), q))
    return "".join(se), "".join(pe1), "".join(pe2)


@pytest.mark.parametrize("kind", ["se", "pe"])
def test_planted_methylation_comes_back(gold, mapper_on_gold, tmp_path, kind):
    n_se, n_pe = 600, 400
    se, pe1, pe2 = _planted_reads(gold, n_se, n_pe)
    if kind == "se":
        open(tmp_path / "r.fq", "w").write(se)
        inputs, args, n_reads = ["--seq", str(tmp_path / "r.fq")], golden_args()["b150"], n_se
    else:
        open(tmp_path / "1.fq", "w").write(pe1); open(tmp_path / "2.fq", "w").write(pe2)
        inputs, args, n_reads = ["--seq1", str(tmp_path / "1.fq"), "--seq2", str(tmp_path / "2.fq")], json.load(open(os.path.join(GOLD, "pe_args.json")))["p100"], 2 * n_pe
    out = str(tmp_path / "o.bam")
    _run(gold["fa"], inputs, args + ["--sort", "--methyl", str(tmp_path / "m")] + ALL_CONTEXTS, out)
    recs = split_records(bam_payload(out)[1])
    home = []
    for r in recs:
        ref, pos, _mq, flag, cigar, _b, _q = spec.fields(r)
        f = _name(r).decode().split("_")
        origin = (int(f[1]), int(f[2])) if kind == "se" else (int(f[1]), int(f[3] if flag & 0x80 else f[2]))
        if (ref, pos) == origin and len(cigar) == 1 and cigar[0][0] == 0 and not flag & 4:
            # the strand the flags give is the strand the read was made from
            assert spec.is_ob(flag) == bool(int(f[-1])), (_name(r), flag)
            home.append(r)
    assert 2 * len(home) >= n_reads, (len(home), n_reads)
    got = mapper_on_gold.bam_methyl(b"".join(home), [len(r) for r in home], None, contexts=7, min_mapq=0, min_phred=0)
    assert len(got) > 1000
    third = got["pos"] % 3 == 0
    assert not got["unmeth"][third].any() and not got["meth"][~third].any()
    assert got["meth"][third].all() and got["unmeth"][~third].all() and third.any() and (~third).any()
    for ctx in range(3):
        for strand in range(2):
            assert (got["kind"] == (ctx | strand << 2)).sum() > 20
    # the driver's files hold the planted pattern too, wherever every caller of a site sits at its origin
    at_home = {(int(r["ref"]), int(r["pos"])) for r in got}
    names = {n: i for i, n in enumerate(gold["names"])}
    checked = 0
    for f in _files(str(tmp_path / "m")):
        for line in f.decode().split("\n")[1:-1]:
            c, p, _e, pct, me, un = line.split("\t")
            if len(home) == len(recs) and (names[c], int(p)) in at_home:
                assert (int(un) == 0 and pct == "100") if int(p) % 3 == 0 else (int(me) == 0 and pct == "0")
                checked += 1
    assert len(home) < len(recs) or checked > 1000


# ---- 5. the driver against the spec -----------------------------------------------------------------------------------------------------------------
def _with_copies(recs, tag, mate=""):
    """every fifth read three times under new names: as it is, with lowered qualities, with 7 bases trimmed from its 3' end (what
    test_markdup.py feeds --markdup); names are `<tag><serial>` (+ /1, /2), the serial counts output records"""
    out = []
    def put(seq, qual):
        out.append("@%s%d%s\n%s\n+\n%s" % (tag, len(out), mate, seq, qual))
    for i, r in enumerate(recs):
        put(r[1], r[3])
        if i % 5 == 0:
            put(r[1], "".join(chr(max(35, ord(c) - 4)) for c in r[3]))
            put(r[1][:-7], r[3][:-7])
    return "\n".join(out) + "\n", len(out)


@pytest.fixture(scope="module")
def runs(gold, tmp_path_factory):
    """per kind: the FASTQ with copies, the plain --bam run, the --sort --bai run (single end; into the file the --methyl run writes again), the spec's sites of the plain run's records (with their
    clips; as they are and marked by markdup_spec) -- made once"""
    pe_args = json.load(open(os.path.join(GOLD, "pe_args.json")))
    made = {}

    def get(kind):
        if kind in made:
            return made[kind]
        wd = tmp_path_factory.mktemp("methyl_" + kind)
        paired = kind == "pe"
        if paired:
            t1, n = _with_copies(_fastq_records(os.path.join(GOLD, "pe_p100_1.fq.gz"))[:300], "d", "/1")
            t2, _ = _with_copies(_fastq_records(os.path.join(GOLD, "pe_p100_2.fq.gz"))[:300], "d", "/2")
            open(wd / "1.fq", "w").write(t1); open(wd / "2.fq", "w").write(t2)
            inputs, args = ["--seq1", str(wd / "1.fq"), "--seq2", str(wd / "2.fq")], pe_args["p100"]
        else:
            t1, n = _with_copies(_fastq_records(os.path.join(GOLD, "se_b150.fq.gz"))[:500], "d")
            open(wd / "r.fq", "w").write(t1)
            inputs, args = ["--seq", str(wd / "r.fq")], golden_args()["b150"]
        _run(gold["fa"], inputs, args, str(wd / "plain.bam"))
        without = None
        if not paired:                                                        # (one kind is enough for "the same bytes without --methyl")
            _run(gold["fa"], inputs, args + ["--sort", "--bai"], str(wd / "m.bam"))
            without = (open(wd / "m.bam", "rb").read(), open(str(wd / "m.bam") + ".bai", "rb").read())
        entries = _by_template(split_records(bam_payload(str(wd / "plain.bam"))[1]), n, paired, "d")
        marked = markdup_spec.mark(entries, paired)
        clip = spec.clips(entries) if paired else None
        made[kind] = dict(wd=wd, inputs=inputs, args=args, paired=paired, clip=clip, without=without,
                          sites=spec.sites(gold["seqs"], entries, clip, contexts=7), marked_sites=spec.sites(gold["seqs"], marked, clip, contexts=7))
        return made[kind]
    return get


@pytest.mark.parametrize("kind", ["se", "pe"])
def test_driver_files_equal_the_spec(gold, runs, kind):
    R = runs(kind)
    wd = R["wd"]
    pre = str(wd / "m")
    err = _run(gold["fa"], R["inputs"], R["args"] + ["--sort", "--bai", "--methyl", pre] + ALL_CONTEXTS, str(wd / "m.bam"))
    assert _files(pre) == _spec_files(pre, gold["names"], R["sites"])
    assert all(len(f.split(b"\n")) > 100 for f in _files(pre))
    assert not R["paired"] or sum(1 for c in R["clip"] if c) > 50                      # mates of the golden pairs do overlap
    # the BAM and its index are those of the run without --methyl into the same file, byte for byte (the header does not name the option)
    if R["without"]:
        assert (open(wd / "m.bam", "rb").read(), open(str(wd / "m.bam") + ".bai", "rb").read()) == R["without"]
    else:
        assert open(str(wd / "m.bam") + ".bai", "rb").read() == bai_spec.spec_bai(str(wd / "m.bam"))
    # the --verbose line counts what the files hold
    m = re.search(r"methyl: sites CpG (\d+) CHG (\d+) CHH (\d+), calls CpG (\d+) CHG (\d+) CHH (\d+)", err)
    assert m, err
    assert [int(x) for x in m.groups()] == [sum(1 for s in R["sites"] if s[4] & 3 == c) for c in range(3)] + \
        [sum(s[2] + s[3] for s in R["sites"] if s[4] & 3 == c) for c in range(3)]


GEOMETRIES = [(dict(BMBS_SORT_CALL_BYTES="8000", BMBS_SORT_BINS="7"), []),
              (dict(BMBS_SORT_CALL_BYTES="8000"), ["--batch", "50"]),
              (dict(BMBS_SORT_BINS="1"), ["--batch", "31", "--contexts", "2"])]


@pytest.mark.parametrize("geometry", range(len(GEOMETRIES)))
@pytest.mark.parametrize("kind", ["se", "pe"])
def test_driver_files_with_markdup_under_other_geometries(gold, runs, kind, geometry):
    """duplicates (flag 0x400, set while pass 2 stages its records) are skipped: some site's counts differ from the run without
    --markdup; small pass-2 calls, few bins, small batches and two contexts change nothing"""
    R = runs(kind)
    want = R["marked_sites"]
    assert len(want) > 100 and want != R["sites"]
    env, more = GEOMETRIES[geometry]
    pre = str(R["wd"] / ("g%d" % geometry))
    err = _run(gold["fa"], R["inputs"], R["args"] + ["--sort", "--bai", "--markdup", "--methyl", pre] + ALL_CONTEXTS + more, pre + ".bam", env)
    assert _files(pre) == _spec_files(pre, gold["names"], want), (env, more)
    if "BMBS_SORT_CALL_BYTES" in env:
        assert int(re.search(r"pass-2 calls (\d+)", err).group(1)) > 1
    assert open(pre + ".bam.bai", "rb").read() == bai_spec.spec_bai(pre + ".bam")


def test_driver_thresholds_one_context_and_refusals(gold, runs, tmp_path):
    R = runs("se")
    pre = str(tmp_path / "t")
    # (the index under another name, without its FASTA: said on stderr, and nothing to filter in the golden genome)
    moved = str(tmp_path / "moved")
    for f in os.listdir(os.path.dirname(gold["fa"])):
        if f.startswith("genome.fa."):
            os.symlink(os.path.join(os.path.dirname(gold["fa"]), f), moved + f[len("genome.fa"):])
    err = _run(moved, R["inputs"], R["args"] + ["--sort", "--methyl", pre, "--CHG", "--methyl-min-mapq", "40", "--methyl-min-phred", "30"], pre + ".bam",
               dict(BMBS_SORT_CALL_BYTES="8000"))
    assert "not filtered" in err
    entries = split_records(bam_payload(pre + ".bam")[1])
    want = spec.sites(gold["seqs"], entries, None, contexts=2, min_mapq=40, min_phred=30)
    assert open(pre + "_CHG.bedGraph", "rb").read() == spec.bedgraph(pre, spec.CHG, gold["names"], want)
    assert len(want) > 100 and want != spec.select(R["sites"], 2)
    assert not os.path.exists(pre + "_CpG.bedGraph") and not os.path.exists(pre + "_CHH.bedGraph")       # only the selected context is written
    for bad in (["--methyl", pre], ["--sort", "--CHG"], ["--sort", "--methyl", pre, "--methy_out"]):
        p = subprocess.run([_driver(), "--search", gold["fa"]] + R["inputs"] + ["-o", str(tmp_path / "x.bam"), "--bam"] + bad, capture_output=True, text=True)
        assert p.returncode == 2, p.stderr


# ---- 6. bases other than A, C, G, T -------------------------------------------------------------------------------------------------------------
def test_sites_at_bases_the_fasta_does_not_spell_are_left_out(tmp_path):
    """a genome with runs of N (1..3 bases inside reads, 60 bases that reads only reach into) and a few other letters; error-free OT
    reads laid across every run's borders, the run's bases read as T: where the index holds a C there, the device calls a site"""
    from bitmapperbs_amd import mapper
    rng = np.random.default_rng(3)
    seqs = ["".join("ACGT"[x] for x in rng.integers(0, 4, 6000)) for _ in range(2)]
    runs_in = [(300, 301), (700, 702), (1100, 1103), (1500, 1560), (2500, 2501), (3000, 3060), (4000, 4002)]
    mut = []
    for s in seqs:
        b = list(s)
        for lo, hi in runs_in:
            b[lo:hi] = "N" * (hi - lo)
        b[5000] = "R"; b[5003] = "n"
        mut.append("".join(b))
    fa = str(tmp_path / "n.fa")
    open(fa, "w").write("".join(">c%d some text\n%s\n" % (i, "\n".join(s[k:k + 70] for k in range(0, len(s), 70))) for i, s in enumerate(mut)))
    mapper.Index.build(fa, fa, threads=4)
    ix = mapper.Index(fa)
    held = spec.genome_of_pac(ctypes.string_at(ix.view.pac, int(ix.view.pac_bytes)), ix.chrom_len)
    runs = spec.non_acgt_runs(open(fa).read())
    assert runs[0] == runs_in + [(5000, 5001), (5003, 5004)] and runs[1] == runs[0]
    reads = []
    for ref, s in enumerate(mut):
        starts = sorted({max(0, min(len(s) - 100, b + d)) for lo, hi in runs[ref] for b in (lo, hi) for d in (-97, -50, -3, 1)} | set(range(0, 5900, 37)))
        for p in starts:
            seq = "".join("T" if c not in "ACGT" else ("C" if c == "C" and p % 2 else "T" if c == "C" else c) for c in s[p:p + 100].upper())
            reads.append("@r%d_%d_%d\n%s\n+\n%s\n" % (len(reads), ref, p, seq, "I" * 100))
    open(tmp_path / "r.fq", "w").write("".join(reads))
    pre = str(tmp_path / "m")
    err = _run(fa, ["--seq", str(tmp_path / "r.fq")], ["--sort", "--methyl", pre] + ALL_CONTEXTS, pre + ".bam")
    recs = split_records(bam_payload(pre + ".bam")[1])
    unfiltered = spec.sites(held, recs, None, contexts=7)
    want = spec.drop_non_acgt(unfiltered, runs)
    dropped = [s for s in unfiltered if s not in set(want)]
    inside = lambda s: any(lo <= s[1] < hi for lo, hi in runs[s[0]])
    # in both sequences: sites inside a run, and sites beside one whose context window reaches into it
    for ref in range(2):
        assert any(s[0] == ref and inside(s) for s in dropped) and any(s[0] == ref and not inside(s) for s in dropped)
    assert len(want) > 1000
    assert int(re.search(r"sites left out at bases other than ACGT (\d+)", err).group(1)) == len(unfiltered) - len(want)
    assert _files(pre) == _spec_files(pre, ix.chrom_names, want)
    # no site of the files touches a run, and records reach across the borders of every run
    for f in _files(pre):
        for line in f.decode().split("\n")[1:-1]:
            c, p = line.split("\t")[:2]
            assert not any(lo <= int(p) < hi for lo, hi in runs[int(c[1:])])
    spans = [(spec.fields(r)[0], spec.fields(r)[1], spec.fields(r)[1] + spec.ref_span(spec.fields(r)[4])) for r in recs if not spec.fields(r)[3] & 4]
    for ref in range(2):
        for lo, hi in runs[ref]:
            assert any(r == ref and a < lo < b for r, a, b in spans) and any(r == ref and a < hi < b for r, a, b in spans), (ref, lo, hi)
    ix.close()
