"""The trimming rule of the text calls (include/bmbs.h: bmbs_set_trim; bmbs_search --trim) in plain Python: what the device has to
compute, restated from the rule's text alone.  Exact integer arithmetic throughout.

A record is (name line, sequence, '+' line, quality line) as bytes without newlines.  Steps, in this order: quality (BWA rule, 3' end),
3' adapter (leftmost accepted start, no indels), fixed clips, length filter."""
from collections import namedtuple

Opts = namedtuple("Opts", "quality adapter min_overlap error_permille min_length clip_5p clip_3p base")
# trim_galore's defaults (adapter: per mate); base: the context's Phred base (bmbs_params.q_base)
DEFAULTS = Opts(20, ("AGATCGGAAGAGC", "AGATCGGAAGAGC"), 1, 100, 20, (0, 0), (0, 0), 33)
COUNTERS = ("records_in", "bases_in", "bases_out", "quality_records", "quality_bases", "adapter_records", "adapter_bases", "clip_records", "clip_bases")


def qual_at(q: bytes, i: int) -> int:
    """a quality character missing from a short quality line counts as ' '"""
    return q[i] if i < len(q) else 32


def quality_stop(s: bytes, q: bytes, cutoff: int, base: int) -> int:
    """cutadapt's -q (the BWA rule), 3' end only: the loop"""
    L = len(s)
    if cutoff <= 0:
        return L
    acc, best, stop = 0, 0, L
    for i in range(L - 1, -1, -1):
        acc += cutoff - (qual_at(q, i) - base)
        if acc < 0:
            break
        if acc > best:
            best, stop = acc, i
    return stop


def quality_stop_closed(s: bytes, q: bytes, cutoff: int, base: int) -> int:
    """the same in the form a parallel kernel computes: suffix sums S_i, b = the largest i with S_i < 0, stop = the largest i > b at
    which S_i is largest, if that is > 0"""
    L = len(s)
    if cutoff <= 0:
        return L
    S = [0] * (L + 1)
    for i in range(L - 1, -1, -1):
        S[i] = S[i + 1] + cutoff - (qual_at(q, i) - base)
    b = max([i for i in range(L) if S[i] < 0], default=-1)
    cand = range(b + 1, L)
    if not cand:
        return L
    mx = max(S[i] for i in cand)
    if mx <= 0:
        return L
    return max(i for i in cand if S[i] == mx)


def adapter_start(s: bytes, L: int, adapter: str, min_overlap: int, error_permille: int) -> int:
    """the smallest accepted start of the adapter in s[0..L), or L"""
    if not adapter:
        return L
    A = adapter.upper().encode()
    up = s.upper()
    for i in range(L):
        o = min(len(A), L - i)
        mm = sum(1 for j in range(o) if up[i + j] != A[j])
        if o >= min_overlap and mm <= o * error_permille // 1000:
            return i
    return L


Trimmed = namedtuple("Trimmed", "k L qual_len after_quality after_adapter")


def trim_record(s: bytes, q: bytes, mate: int, o: Opts) -> Trimmed:
    """steps 1-3 of one record: the sequence and the quality line begin k characters later, L sequence characters and qual_len
    quality characters stay"""
    q = q[:len(s)]
    L0 = len(s)
    L1 = quality_stop(s, q, o.quality, o.base)
    L2 = adapter_start(s, L1, o.adapter[mate], o.min_overlap, o.error_permille)
    L = L2 - min(L2, o.clip_3p[mate])
    k = min(L, o.clip_5p[mate])
    L -= k
    return Trimmed(k, L, max(0, min(len(q) - k, L)), L1, L2)


def records_of(text: bytes):
    lines = text.split(b"\n")
    return [lines[i:i + 4] for i in range(0, len(lines) - 3, 4)]


def trim_fastq(text1: bytes, text2, o: Opts):
    """-> (trimmed text 1, trimmed text 2 or None, kept templates, counters): the FASTQ text(s) a host trimmer following the rule leaves,
    the templates that pass the length filter, and counters[name] = [mate 1, mate 2] (+ "templates_dropped")"""
    files = [records_of(text1)] + ([records_of(text2)] if text2 is not None else [])
    assert len({len(f) for f in files}) == 1
    cnt = {k: [0, 0] for k in COUNTERS}
    cut = [[trim_record(r[1], r[3], m, o) for r in f] for m, f in enumerate(files)]
    keep = [all(c[i].L >= o.min_length for c in cut) for i in range(len(files[0]))]
    out = []
    for m, f in enumerate(files):
        lines = []
        for r, t, kp in zip(f, cut[m], keep):
            L0 = len(r[1])
            cnt["records_in"][m] += 1; cnt["bases_in"][m] += L0
            for step, a, b in (("quality", L0, t.after_quality), ("adapter", t.after_quality, t.after_adapter), ("clip", t.after_adapter, t.L)):
                if b < a:
                    cnt[step + "_records"][m] += 1; cnt[step + "_bases"][m] += a - b
            if kp:
                cnt["bases_out"][m] += t.L
                lines += [r[0], r[1][t.k:t.k + t.L], r[2], r[3][:L0][t.k:t.k + t.qual_len]]
        out.append(b"".join(l + b"\n" for l in lines))
    cnt["templates_dropped"] = len(keep) - sum(keep)
    return out[0], (out[1] if text2 is not None else None), sum(keep), cnt
