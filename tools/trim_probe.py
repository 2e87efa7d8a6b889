#!/usr/bin/env python3
"""tools/trim_probe.py -- what `bmbs_search --trim` costs, file to file, on one input and one build.

150-base pairs drawn from the probe genome; in a known share of the reads the insert ends early and the adapter (and random bases behind
it) follows, and a further share gets a low-quality tail.  Alternating runs of `bmbs_search` with and without `--trim` (at least three
each): medians and spread of the mapping wall.  --other-driver <bmbs_search of another build>: that build's run without --trim
alternates with them -- this build's median without the option against the other's median and spread -- and --compare-runs runs of
either build without --trim go under `rocprofv3 --kernel-trace --stats`, alternating: do both launch the same kernels the same number of
times (the project's kernels and the runtime's fill kernel counted apart)?  --compare-only: that comparison alone.  Also one --trim
run of its own under the kernel trace (no counters in it): k_fq_trim and k_fq_compact beside k_fq_records and k_fastq_rows, which reads
the same sequence and quality bytes once.  Every GPU step runs under its own `timeout`; the script stops at the first failure.  No host
trimmer is timed: none is installed where this runs.

  python tools/trim_probe.py [--reads 1000000] [--loop 4] [--runs 3] [--adapter-share 0.3] [--other-driver path] [--out profiles/trim_probe.txt]
"""
import argparse
import csv
import glob
import os
import re
import shutil
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

ADAPTER = np.frombuffer(b"AGATCGGAAGAGC", dtype=np.uint8)


def step(cmd, limit, **kw):
    """one GPU step under its own time limit; anything but success ends the probe"""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, **kw)
    if p.returncode:
        sys.stderr.write("trim_probe: step failed (exit %d): %s\n%s\n" % (p.returncode, " ".join(cmd), p.stderr[-3000:]))
        sys.exit(1)
    return p


def make_raw(s, q, L, rng, adapter_share, tail_share):
    """reads [n, stride] made raw in place: adapter read-through behind an insert of 30 .. L - 1 bases, low-quality tails"""
    n = s.shape[0]
    u = rng.random(n)
    cut = rng.integers(30, L, n)
    for p in range(30, L):
        rows = np.nonzero((u < adapter_share) & (cut == p))[0]
        if rows.size:
            k = min(ADAPTER.size, L - p)
            s[rows, p:p + k] = ADAPTER[:k]
            if p + k < L:
                s[rows, p + k:L] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (rows.size, L - p - k))]
        rows = np.nonzero((u >= adapter_share) & (u < adapter_share + tail_share) & (cut == p))[0]
        if rows.size:
            q[rows, p:L] = ord("#")
    return int((u < adapter_share).sum()), int(((u >= adapter_share) & (u < adapter_share + tail_share)).sum())


def wall_of(err):
    return float(re.search(r"mapping wall ([\d.]+)s", err).group(1))


def kernel_rows(tr):
    f = glob.glob(os.path.join(tr, "**", "*kernel_stats.csv"), recursive=True)
    return list(csv.DictReader(open(f[0]))) if f else []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000, help="pairs in the file")
    ap.add_argument("--loop", type=int, default=4, help="--loop-input: the FASTQ is read this many times over")
    ap.add_argument("--genome", type=int, default=46_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("-e", type=float, default=0.04)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=500_000)
    ap.add_argument("--adapter-share", type=float, default=0.3)
    ap.add_argument("--tail-share", type=float, default=0.2)
    ap.add_argument("--compare-runs", type=int, default=2, help="with --other-driver: traced runs without --trim of either build, alternating")
    ap.add_argument("--compare-only", action="store_true", help="with --other-driver: only the traced runs without --trim (appended to --out)")
    ap.add_argument("--other-driver", default="", help="bmbs_search of another build, whose run without --trim alternates with this build's")
    ap.add_argument("--workdir", default=os.environ.get("BMBS_BENCH_DIR", "/tmp/bmbs_bench"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trim_probe.txt"))
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "trim_kernel_stats.csv"))
    args = ap.parse_args()
    import torch
    from bitmapperbs_amd import gpusynth
    cfg = dict(genome=args.genome, n_chrom=4 if args.genome < 1_000_000_000 else 24)
    args.host_index = False
    fa, names, chroms, _ = bench.ensure_index(args, cfg, 0, 0, 1, None)
    L = args.read_len
    stride = (L + 15) // 16 * 16
    genome_d, lens_d = gpusynth.upload_genome(chroms)
    wd = args.workdir
    s1, q1, s2, q2 = gpusynth.make_reads_pe(genome_d, lens_d, args.reads, L, stride, seed=7, sub=0.005)
    rng = np.random.default_rng(17)
    mates = []
    planted = []
    for s, q in ((s1, q1), (s2, q2)):
        s, q = s.cpu().numpy(), q.cpu().numpy()
        planted.append(make_raw(s, q, L, rng, args.adapter_share, args.tail_share))
        mates.append((s, q))
    f1 = os.path.join(wd, "trimp_1.fq"); f2 = os.path.join(wd, "trimp_2.fq")
    bench.write_fastq_sample(f1, mates[0][0], mates[0][1], L)
    bench.write_fastq_sample(f2, mates[1][0], mates[1][1], L)
    del genome_d
    torch.cuda.empty_cache()
    n_reads = 2 * args.reads * args.loop
    drv = os.path.join(ROOT, "bitmapperbs_amd", "bmbs_search")
    base = [drv, "--search", fa, "--seq1", f1, "--seq2", f2, "-e", str(args.e), "--unmapped_out", "--batch", str(args.batch), "--loop-input", str(args.loop), "--verbose"]
    out = os.path.join(wd, "trimp.sam")
    rep = os.path.join(wd, "trimp_report.tsv")
    legs = [("plain", drv, []), ("trim", drv, ["--trim", "--trim-report", rep])]
    if args.other_driver:
        legs.append(("other", args.other_driver, []))
    runs = {k: [] for k, _, _ in legs}
    step(base + ["-o", out], 600)                       # warm-up: page cache, index files
    for _ in range(0 if args.compare_only else max(3, args.runs)):
        for kind, d, extra in legs:
            p = step([d] + base[1:] + extra + ["-o", out], 600)
            runs[kind].append(wall_of(p.stderr))
    lines = []
    say = lines.append
    say("trim_probe: %d pairs of %d bp x %d passes over the files = %d reads per run, genome %d bp, batch %d; adapter read-through planted in %d + %d reads (insert 30 .. %d), low-quality tails in %d + %d"
        % (args.reads, L, args.loop, n_reads, args.genome, args.batch, planted[0][0], planted[1][0], L - 1, planted[0][1], planted[1][1]))
    say("  " + " ".join(base[3:]))
    med = {}
    if args.compare_only:
        runs = {}
    label = {"plain": "without --trim", "trim": "--trim", "other": "other build, without"}
    for kind in runs:
        w = runs[kind]
        med[kind] = statistics.median(w)
        say("%-22s mapping wall s: %s   median %.3f  spread (max - min) %.3f   %.1f M reads/s at the median"
            % (label[kind], " ".join("%.3f" % x for x in w), med[kind], max(w) - min(w), n_reads / med[kind] / 1e6))
    if not args.compare_only:
      say("--trim against no --trim on this build (medians): %+.3f s = %+.1f %% (the --trim run maps fewer and shorter reads and writes less)"
        % (med["trim"] - med["plain"], 100 * (med["trim"] - med["plain"]) / med["plain"]))
    if os.path.exists(rep) and not args.compare_only:
        say("the last --trim run's report (all passes over the files): " + "; ".join(l.strip().replace("\t", " ") for l in open(rep)))
    if args.other_driver and not args.compare_only:
        ow = runs["other"]
        say("without --trim, this build against the other build (%s): median wall %.3f s against %.3f s = %+.3f s; the other build's own spread (max - min) %.3f s: %s"
            % (args.other_driver, med["plain"], med["other"], med["plain"] - med["other"], max(ow) - min(ow),
               "within it" if abs(med["plain"] - med["other"]) <= max(ow) - min(ow) else "OUTSIDE it"))
    say("no host trimmer (cutadapt, trim_galore) is installed where this ran: there is no timing against one")
    # ---- one --trim run of its own under the kernel trace
    tr = os.path.join(wd, "trimp_trace")
    shutil.rmtree(tr, ignore_errors=True)
    if not args.compare_only:
        step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tr, "--"] + base + ["--trim", "-o", out], 900)
    rows = [] if args.compare_only else kernel_rows(tr)
    if rows:
        os.makedirs(os.path.dirname(args.stats_out), exist_ok=True)
        with open(args.stats_out, "w") as o:
            w = csv.writer(o); w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs"])
            for r in rows:
                w.writerow([r["Name"], r["Calls"], r["TotalDurationNs"], r["AverageNs"], r["MinNs"], r["MaxNs"]])
        tot = sum(int(r["TotalDurationNs"]) for r in rows)
        say("kernel trace (one --trim run under rocprofv3, %s): all kernels %.1f ms" % (os.path.relpath(args.stats_out, ROOT), tot / 1e6))
        ns = {}
        for name in ("k_fq_count", "k_fq_lines", "k_fq_records", "k_fq_trim", "k_trim_keep", "k_fq_compact", "k_fastq_rows"):
            t = [(int(r["Calls"]), int(r["TotalDurationNs"])) for r in rows if name in r["Name"]]
            ns[name] = sum(x[1] for x in t)
            say("  %-14s %9.3f ms in %d calls" % (name, ns[name] / 1e6, sum(x[0] for x in t)))
        if ns["k_fastq_rows"] and ns["k_fq_trim"]:
            say("  k_fq_trim = %.2f x k_fastq_rows (which reads the same sequence and quality bytes once, of the records that stay), k_fq_compact = %.2f x k_fq_records"
                % (ns["k_fq_trim"] / ns["k_fastq_rows"], ns["k_fq_compact"] / max(1, ns["k_fq_records"])))
    # ---- without --trim: do both builds launch the same kernels the same number of times?
    # The runtime's own fill kernel (hipMemsetAsync; a lane's zeroed buffers are cleared when a context first gets a batch, and the
    # batches go to whichever context is free) is counted apart from the project's kernels, and every build is traced more than once,
    # so that what differs between two runs of ONE build is not taken for a difference between the builds.
    if args.other_driver:
        seen = {"this build": [], "the other build": []}
        for _ in range(max(1, args.compare_runs)):
            for who, d in (("this build", drv), ("the other build", args.other_driver)):
                shutil.rmtree(tr, ignore_errors=True)
                step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tr, "--", d] + base[1:] + ["-o", out], 900)
                seen[who].append({r["Name"]: int(r["Calls"]) for r in kernel_rows(tr)})

        def own(c):
            return {n: k for n, k in c.items() if not n.startswith("__amd_rocclr")}

        def fills(c):
            return sum(k for n, k in c.items() if n.startswith("__amd_rocclr"))
        if not all(seen["this build"]) or not all(seen["the other build"]):
            say("without --trim under the kernel trace: a run without kernel rows -- nothing to compare")
        else:
            a, b = own(seen["this build"][0]), own(seen["the other build"][0])
            steady = all(own(c) == a for c in seen["this build"]) and all(own(c) == b for c in seen["the other build"])
            differ = sorted(n for n in set(a) | set(b) if a.get(n, 0) != b.get(n, 0))
            say("without --trim under the kernel trace, %d runs of either build, alternating: the project's kernels -- %d and %d names, %d and %d launches, %s from run to run; names and call counts %s"
                % (len(seen["this build"]), len(a), len(b), sum(a.values()), sum(b.values()), "the same" if steady else "NOT the same", "identical" if not differ else "differ in %d rows:" % len(differ)))
            for n in differ:
                say("  %s: %d calls here, %d there" % (n.split("(")[0], a.get(n, 0), b.get(n, 0)))
            say("  the runtime's fill kernel (hipMemsetAsync), each run: this build %s, the other build %s"
                % (" ".join(str(fills(c)) for c in seen["this build"]), " ".join(str(fills(c)) for c in seen["the other build"])))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.compare_only else "w") as o:
        o.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
