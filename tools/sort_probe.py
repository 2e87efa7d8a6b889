#!/usr/bin/env python3
"""tools/sort_probe.py -- what `--bam --sort` costs next to `--bam`, file to file, on one input and one build.

Alternating runs of `bmbs_search --bam` and `bmbs_search --bam --sort` (at least three each), medians and spread of the mapping
wall (for --sort: both passes); beside the measured ratio the one the link bytes alone predict, (2R + c) / c -- R = raw record
bytes per read (down in pass 1, up in pass 2), c = compressed bytes per read, both from the runs' own counts.  Then ONE run of its
own under `rocprofv3 --kernel-trace --stats`: k_bam_gather's bytes/s (2 x record bytes over its kernel time) beside
k_line_write<true>'s (same records, same count) in the same trace, and the pass-2 kernels' share.  Every GPU step runs under its
own `timeout`; the script stops at the first failure.
--bai: a third leg, `--bam --sort --bai`, alternating with the other two -- its walls beside the sorted runs', the size of the index,
and the k_bai_* rows of the kernel trace (which then is a --bai run) beside k_bam_gather.
--markdup: a leg `--bam --sort --markdup`, alternating with the others -- its walls beside the sorted runs', the counts of the
driver's markdup line, and the k_dup_* rows of the kernel trace (which then is a --markdup run) beside k_bam_gather.
--methyl: a leg `--bam --sort --methyl <prefix> --CpG --CHG --CHH`, alternating with the others -- its walls beside the sorted runs' on the
same build, the counts of the driver's methyl line, and the k_meth_* rows of the kernel trace (which then is a --methyl run).
--mbias (with --methyl): a leg `--methyl ... --mbias` beside the --methyl leg -- its walls beside that leg's, the `mbias calls` figure,
and k_meth_mbias's kernel time beside the counting pass's (k_meth_events<false, ..>, the same walk) in the trace (then a --mbias run).
--other-driver <bmbs_search of another build> (with --methyl): that build's `--methyl` leg alternates with this build's, to show that
a run which asks for neither the table nor a trim costs what it did: this build's median against the other's median and spread.
(The other build's runs write the same sortp_y.bam and bedGraphs as this build's --methyl leg, one after the other.)
--variant (with --methyl): a leg `--methyl ... --methyl-min-opposite-depth 3 --methyl-max-variant-frac 0.5` beside the --methyl leg --
its walls beside that leg's, the numbers of sites dropped as variants, and the opposite passes' kernel time (k_meth_events<.., .., true>)
beside the calling passes' (k_meth_events<.., .., false>: k_meth_count / k_meth_emit) in the trace (then a run with the filter on).  The
report goes to profiles/variant_probe.txt and the kernel rows to profiles/variant_kernel_stats.csv unless --out / --stats-out say otherwise.
--report (with --methyl): a leg `--methyl ... --cytosine-report` beside the --methyl leg -- its walls beside that leg's, the report's
lines and bytes and the seconds the driver spent on it (inside the device calls, and waiting for the file), what the file system takes
for as many bytes, the k_cyt_* rows of the trace (then a run with the report), and k_cyt_emit's bytes written per second beside
k_line_write<true>'s.  With --other-driver the plain --methyl run of either build goes under the kernel trace too, as with --variant.
The report goes to profiles/cytosine_report_probe.txt and the kernel rows to profiles/cytosine_report_kernel_stats.csv.
--nonconv (with --methyl): a leg `--methyl ... --filter-non-conversion` beside the --methyl leg -- its walls beside that leg's and its
own spread, the templates examined and failed, the k_nonconv_* rows of the trace (then a run with the filter), and k_nonconv_walk's
kernel time beside the counting pass k_meth_events<false, false>'s of the same run (the same walk over the same records with one context
fewer and a clip).  With --other-driver the plain --methyl run of either build goes under the kernel trace too, as with --variant.  The
report goes to profiles/nonconv_probe.txt and the kernel rows to profiles/nonconv_kernel_stats.csv.
With --mbias the report goes to profiles/mbias_probe.txt and the kernel rows to profiles/mbias_kernel_stats.csv unless --out /
--stats-out name other files.

  python tools/sort_probe.py [--reads 4000000] [--loop 8] [--pe] [--runs 3] [--bai] [--markdup] [--methyl [--mbias] [--variant] [--report] [--nonconv] [--other-driver path]] [--out profiles/sorted_bam_probe.txt | profiles/mbias_probe.txt]
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


VARIANT_ARGS = ["--methyl-min-opposite-depth", "3", "--methyl-max-variant-frac", "0.5"]


def step(cmd, limit, **kw):
    """one GPU step under its own time limit; anything but success ends the probe"""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, **kw)
    if p.returncode:
        sys.stderr.write("sort_probe: step failed (exit %d): %s\n%s\n" % (p.returncode, " ".join(cmd), p.stderr[-3000:]))
        sys.exit(1)
    return p


def verbose_numbers(err):
    out = {}
    out["wall"] = float(re.search(r"mapping wall ([\d.]+)s", err).group(1))
    m = re.search(r"sort: bins (\d+) .*pass-2 calls (\d+), store bytes (\d+) \((\d+) records\), pass 1 ([\d.]+)s .*pass 2 ([\d.]+)s", err)
    if m:
        out.update(bins=int(m.group(1)), calls=int(m.group(2)), store=int(m.group(3)), records=int(m.group(4)), pass1=float(m.group(5)), pass2=float(m.group(6)))
    m = re.search(r"index: (chunks \d+, windows \d+, \d+ bytes)", err)
    if m:
        out["index"] = m.group(1)
    m = re.search(r"(markdup: templates \d+, with signature \d+, duplicates \d+ \(select calls \d+, [\d.]+s of pass 2\))", err)
    if m:
        out["markdup"] = m.group(1)
    m = re.search(r"(methyl: sites CpG \d+ CHG \d+ CHH \d+, calls CpG \d+ CHG \d+ CHH \d+)", err)
    if m:
        out["methyl"] = m.group(1)
    m = re.search(r"sites dropped as variants (\d+), lines left out below the minimum depth (\d+)", err)
    if m:
        out["variants"] = int(m.group(1))
    m = re.search(r"report lines (\d+) bytes (\d+) in ([\d.]+)s \(device calls ([\d.]+)s, waiting for the file ([\d.]+)s\)", err)
    if m:
        out["report"] = (int(m.group(1)), int(m.group(2)), float(m.group(3)), float(m.group(4)), float(m.group(5)))
    m = re.search(r"nonconv: templates (\d+), failed (\d+)", err)
    if m:
        out["nonconv"] = (int(m.group(1)), int(m.group(2)))
    m = re.search(r"mbias calls (\d+)", err)
    if m:
        out["mbias"] = int(m.group(1))
    m = re.search(r"busy fractions of the mapping wall: link up ([\d.]+), link down ([\d.]+)", err)
    if m:
        out["link_up"], out["link_down"] = float(m.group(1)), float(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--loop", type=int, default=8, help="--loop-input: the FASTQ is read this many times over, so that a run maps for seconds")
    ap.add_argument("--genome", type=int, default=46_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("-e", type=float, default=0.04)
    ap.add_argument("--pe", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--bai", action="store_true", help="also measure --bam --sort --bai (the index written in the same run)")
    ap.add_argument("--markdup", action="store_true", help="also measure --bam --sort --markdup (PCR duplicates flagged in the same run)")
    ap.add_argument("--methyl", action="store_true", help="also measure --bam --sort --methyl (methylation counts per cytosine from the same run)")
    ap.add_argument("--mbias", action="store_true", help="with --methyl: also measure --methyl ... --mbias (the M-bias table from the same run)")
    ap.add_argument("--variant", action="store_true", help="with --methyl: also measure --methyl with the opposite-strand variant filter on")
    ap.add_argument("--report", action="store_true", help="with --methyl: also measure --methyl ... --cytosine-report (the genome-wide cytosine report)")
    ap.add_argument("--nonconv", action="store_true", help="with --methyl: also measure --methyl ... --filter-non-conversion (unconverted templates flagged in pass 1)")
    ap.add_argument("--other-driver", default="", help="with --methyl: bmbs_search of another build, whose --methyl leg alternates with this build's")
    ap.add_argument("--driver-args", default="")
    ap.add_argument("--workdir", default=os.environ.get("BMBS_BENCH_DIR", "/tmp/bmbs_bench"))
    ap.add_argument("--out", default="")
    ap.add_argument("--stats-out", default="")
    args = ap.parse_args()
    stem = "nonconv" if args.methyl and args.nonconv else "cytosine_report" if args.methyl and args.report else "variant" if args.methyl and args.variant else "mbias" if args.methyl and args.mbias else "sorted_bam"
    args.out = args.out or os.path.join(ROOT, "profiles", stem + "_probe.txt")
    args.stats_out = args.stats_out or os.path.join(ROOT, "profiles", stem + "_kernel_stats.csv")
    import torch
    from bitmapperbs_amd import gpusynth
    cfg = dict(genome=args.genome, n_chrom=4 if args.genome < 1_000_000_000 else 24)
    args.host_index = False
    fa, names, chroms, _ = bench.ensure_index(args, cfg, 0, 0, 1, None)
    L = args.read_len
    stride = (L + 15) // 16 * 16
    genome_d, lens_d = gpusynth.upload_genome(chroms)
    wd = args.workdir
    if not args.pe:
        s, q = gpusynth.make_reads_se(genome_d, lens_d, args.reads, L, stride, seed=7, sub=0.005)
        fq = os.path.join(wd, "sortp.fq")
        bench.write_fastq_sample(fq, s.cpu().numpy(), q.cpu().numpy(), L)
        in_args = ["--seq", fq]
    else:
        s1, q1, s2, q2 = gpusynth.make_reads_pe(genome_d, lens_d, args.reads, L, stride, seed=7, sub=0.005)
        f1 = os.path.join(wd, "sortp_1.fq"); f2 = os.path.join(wd, "sortp_2.fq")
        bench.write_fastq_sample(f1, s1.cpu().numpy(), q1.cpu().numpy(), L)
        bench.write_fastq_sample(f2, s2.cpu().numpy(), q2.cpu().numpy(), L)
        in_args = ["--seq1", f1, "--seq2", f2]
    del genome_d
    torch.cuda.empty_cache()
    n_reads = args.reads * args.loop * (2 if args.pe else 1)
    drv = os.path.join(ROOT, "bitmapperbs_amd", "bmbs_search")
    base = [drv, "--search", fa] + in_args + ["-e", str(args.e), "--bam", "--unmapped_out", "--batch", str(args.batch), "--loop-input", str(args.loop), "--verbose"] + args.driver_args.split()
    out_u = os.path.join(wd, "sortp_u.bam"); out_s = os.path.join(wd, "sortp_s.bam")
    out_b = os.path.join(wd, "sortp_b.bam"); out_m = os.path.join(wd, "sortp_m.bam")
    runs = {"bam": [], "sort": []}
    legs = [("bam", out_u, []), ("sort", out_s, ["--sort"])]
    if args.bai:
        runs["bai"] = []
        legs.append(("bai", out_b, ["--sort", "--bai"]))
    if args.markdup:
        runs["markdup"] = []
        legs.append(("markdup", out_m, ["--sort", "--markdup"]))
    meth_args = ["--methyl", os.path.join(wd, "sortp_meth"), "--CpG", "--CHG", "--CHH"]
    if args.methyl:
        runs["methyl"] = []
        legs.append(("methyl", os.path.join(wd, "sortp_y.bam"), ["--sort"] + meth_args))
        if args.mbias:
            runs["mbias"] = []
            legs.append(("mbias", os.path.join(wd, "sortp_y.bam"), ["--sort"] + meth_args + ["--mbias"]))
        if args.variant:
            runs["variant"] = []
            legs.append(("variant", os.path.join(wd, "sortp_y.bam"), ["--sort"] + meth_args + VARIANT_ARGS))
        if args.report:
            runs["report"] = []
            legs.append(("report", os.path.join(wd, "sortp_y.bam"), ["--sort"] + meth_args + ["--cytosine-report"]))
        if args.nonconv:
            runs["nonconv"] = []
            legs.append(("nonconv", os.path.join(wd, "sortp_y.bam"), ["--sort"] + meth_args + ["--filter-non-conversion"]))
        if args.other_driver:
            runs["methyl_other"] = []
            legs.append(("methyl_other", os.path.join(wd, "sortp_y.bam"), ["--sort"] + meth_args))
    size = {}
    step(base + ["-o", out_u], 600)                     # warm-up: page cache, index files
    for _ in range(max(3, args.runs)):
        for kind, out, extra in legs:
            if os.path.exists(out):
                os.unlink(out)
            p = step(([args.other_driver] + base[1:] if kind == "methyl_other" else base) + extra + ["-o", out], 600)
            runs[kind].append(verbose_numbers(p.stderr))
            size[kind] = os.path.getsize(out)
    # the same sorted run with ONE staging slot and context in pass 2 (the default is two): what overlapping the calls is worth
    one = [verbose_numbers(step(base + ["--sort", "-o", out_s], 600, env=dict(os.environ, BMBS_SORT_SLOTS="1")).stderr) for _ in range(3)]
    lines = []
    say = lines.append
    say("sort_probe: %d %s of %d bp x %d passes over the file = %d records per run, genome %d bp, batch %d, %s"
        % (args.reads, "pairs" if args.pe else "SE reads", L, args.loop, n_reads, args.genome, args.batch, " ".join(base[3:])))
    med = {}
    label = {"bam": "--bam", "sort": "--bam --sort", "bai": "--bam --sort --bai", "markdup": "--bam --sort --markdup", "methyl": "--bam --sort --methyl",
             "mbias": "... --methyl --mbias", "variant": "... --methyl, filter", "report": "... --cytosine-report", "nonconv": "... --filter-non-conv.", "methyl_other": "--methyl, other build"}
    for kind in runs:
        w = [r["wall"] for r in runs[kind]]
        med[kind] = statistics.median(w)
        say("%-18s mapping wall s: %s   median %.3f  spread (max - min) %.3f   %.1f M records/s at the median   file %d bytes"
            % (label[kind], " ".join("%.3f" % x for x in w), med[kind], max(w) - min(w), n_reads / med[kind] / 1e6, size[kind]))
    last = runs["sort"][-1]
    say("--sort: bins %d, pass-2 calls %d, store %d bytes, pass 1 %s s, pass 2 %s s (each run)" % (
        last["bins"], last["calls"], last["store"], " ".join("%.3f" % r["pass1"] for r in runs["sort"]), " ".join("%.3f" % r["pass2"] for r in runs["sort"])))
    say("pass 2 with BMBS_SORT_SLOTS=1: %s s (walls %s)" % (" ".join("%.3f" % r["pass2"] for r in one), " ".join("%.3f" % r["wall"] for r in one)))
    R = (last["store"] - 4 * last["records"]) / n_reads
    c = size["sort"] / n_reads
    ratio = med["sort"] / med["bam"]
    spread = max(max(r["wall"] for r in runs[k]) - min(r["wall"] for r in runs[k]) for k in runs) / med["bam"]
    bound = (2 * R + c) / c
    say("raw record bytes per read R = %.1f, compressed bytes per read c = %.1f" % (R, c))
    say("measured ratio sorted / unsorted (medians) = %.3f; the link bytes alone predict (2R + c) / c = %.3f; spread of the walls in this job = %.3f of the unsorted median"
        % (ratio, bound, spread))
    say("link busy fractions (per device), last runs: --bam up %.3f down %.3f; --bam --sort up %.3f down %.3f (pass 1 only: the text calls' copies)"
        % (runs["bam"][-1].get("link_up", 0), runs["bam"][-1].get("link_down", 0), last.get("link_up", 0), last.get("link_down", 0)))
    if args.bai:
        sw = [r["wall"] for r in runs["sort"]]
        say("--bai: index %d bytes (%s) beside a file of %d; median wall %.3f s against %.3f s without it = %+.3f s; spread (max - min) of the sorted runs %.3f s; pass 2 %s s"
            % (os.path.getsize(out_b + ".bai"), runs["bai"][-1].get("index", "?"), size["bai"], med["bai"], med["sort"], med["bai"] - med["sort"], max(sw) - min(sw),
               " ".join("%.3f" % r["pass2"] for r in runs["bai"])))
    if args.markdup:
        sw = [r["wall"] for r in runs["sort"]]
        say("--markdup: %s; median wall %.3f s against %.3f s without it = %+.3f s; spread (max - min) of the sorted runs %.3f s; pass 1 %s s, pass 2 %s s"
            % (runs["markdup"][-1].get("markdup", "?"), med["markdup"], med["sort"], med["markdup"] - med["sort"], max(sw) - min(sw),
               " ".join("%.3f" % r["pass1"] for r in runs["markdup"]), " ".join("%.3f" % r["pass2"] for r in runs["markdup"])))
    if args.methyl:
        sw = [r["wall"] for r in runs["sort"]]
        say("--methyl: %s; median wall %.3f s against %.3f s without it = %+.3f s; spread (max - min) of the sorted runs %.3f s; pass 1 %s s, pass 2 %s s"
            % (runs["methyl"][-1].get("methyl", "?"), med["methyl"], med["sort"], med["methyl"] - med["sort"], max(sw) - min(sw),
               " ".join("%.3f" % r["pass1"] for r in runs["methyl"]), " ".join("%.3f" % r["pass2"] for r in runs["methyl"])))
    if args.methyl and args.mbias:
        mw = [r["wall"] for r in runs["methyl"]]
        say("--mbias: mbias calls %s; median wall %.3f s against %.3f s of --methyl without it = %+.3f s; spread (max - min) of the --methyl runs %.3f s; pass 2 %s s"
            % (runs["mbias"][-1].get("mbias", "?"), med["mbias"], med["methyl"], med["mbias"] - med["methyl"], max(mw) - min(mw), " ".join("%.3f" % r["pass2"] for r in runs["mbias"])))
    if args.methyl and args.variant:
        mw = [r["wall"] for r in runs["methyl"]]
        say("variant filter (%s): sites dropped as variants %s; median wall %.3f s against %.3f s of --methyl without it = %+.3f s; spread (max - min) of the --methyl runs %.3f s; pass 2 %s s"
            % (" ".join(VARIANT_ARGS), runs["variant"][-1].get("variants", "?"), med["variant"], med["methyl"], med["variant"] - med["methyl"], max(mw) - min(mw),
               " ".join("%.3f" % r["pass2"] for r in runs["variant"])))
    if args.methyl and args.report:
        mw = [r["wall"] for r in runs["methyl"]]
        n_l, n_b = runs["report"][-1]["report"][:2]
        say("cytosine report: %d lines, %d bytes (%.1f bytes a line); median wall %.3f s against %.3f s of --methyl without it = %+.3f s; spread (max - min) of the --methyl runs %.3f s"
            % (n_l, n_b, n_b / max(1, n_l), med["report"], med["methyl"], med["report"] - med["methyl"], max(mw) - min(mw)))
        say("  the driver's own clock, each run: report %s s, of which inside bmbs_methyl_report %s s and waiting for the writer thread to hand a buffer back %s s"
            % tuple(" ".join("%.3f" % r["report"][k] for r in runs["report"]) for k in (2, 3, 4)))
        # what the file system takes for as many bytes, written the way the driver writes them (pwrite of 64 MiB pieces into a new file)
        import time
        scratch = os.path.join(wd, "sortp_meth.write_probe")
        piece = bytes(64 << 20)
        t0 = time.time()
        fd = os.open(scratch, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        at = 0
        while at < n_b:
            at += os.pwrite(fd, piece[:min(len(piece), n_b - at)], at)
        os.close(fd)
        t_fs = time.time() - t0
        os.unlink(scratch)
        say("  the file system alone: %d bytes into a new file in %.3f s = %.2f GB/s" % (n_b, t_fs, n_b / t_fs / 1e9))
    if args.methyl and args.nonconv:
        mw, nw = [r["wall"] for r in runs["methyl"]], [r["wall"] for r in runs["nonconv"]]
        n_t, n_f = runs["nonconv"][-1].get("nonconv", (0, 0))
        say("--filter-non-conversion: templates %d, failed %d; median wall %.3f s against %.3f s of --methyl without it = %+.3f s; spread (max - min) of this leg %.3f s, of the --methyl runs %.3f s; pass 1 %s s"
            % (n_t, n_f, med["nonconv"], med["methyl"], med["nonconv"] - med["methyl"], max(nw) - min(nw), max(mw) - min(mw), " ".join("%.3f" % r["pass1"] for r in runs["nonconv"])))
    if args.methyl and args.other_driver:
        ow = [r["wall"] for r in runs["methyl_other"]]
        say("--methyl on this build against the other build (%s): median wall %.3f s against %.3f s = %+.3f s; the other build's own spread (max - min) %.3f s: %s"
            % (args.other_driver, med["methyl"], med["methyl_other"], med["methyl"] - med["methyl_other"], max(ow) - min(ow),
               "within it" if abs(med["methyl"] - med["methyl_other"]) <= max(ow) - min(ow) else "OUTSIDE it"))
    # ---- one run of its own under the kernel trace
    tr = os.path.join(wd, "sortp_trace")
    shutil.rmtree(tr, ignore_errors=True)
    if os.path.exists(out_s):
        os.unlink(out_s)
    step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tr, "--"] + base + ["--sort"] + (["--bai"] if args.bai else []) + (["--markdup"] if args.markdup else []) + (meth_args if args.methyl else []) + (["--mbias"] if args.methyl and args.mbias else []) + (VARIANT_ARGS if args.methyl and args.variant else []) + (["--cytosine-report"] if args.methyl and args.report else []) + (["--filter-non-conversion"] if args.methyl and args.nonconv else []) + ["-o", out_s], 900)
    f = glob.glob(os.path.join(tr, "**", "*kernel_stats.csv"), recursive=True)
    if f:
        rows = list(csv.DictReader(open(f[0])))
        tot = sum(int(r["TotalDurationNs"]) for r in rows)
        os.makedirs(os.path.dirname(args.stats_out), exist_ok=True)
        with open(args.stats_out, "w") as o:
            w = csv.writer(o); w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs"])
            for r in rows:
                w.writerow([r["Name"], r["Calls"], r["TotalDurationNs"], r["AverageNs"], r["MinNs"], r["MaxNs"]])
        rec_bytes = last["store"] - 4 * last["records"]

        def total_ns(pred):
            return sum(int(r["TotalDurationNs"]) for r in rows if pred(r["Name"]))
        g = total_ns(lambda n: "k_bam_gather" in n)
        lw = total_ns(lambda n: "k_line_write<true>" in n)
        say("kernel trace (one --bam --sort run under rocprofv3, %s): all kernels %.1f ms" % (os.path.relpath(args.stats_out, ROOT), tot / 1e6))
        # the gather runs twice over the records (pass 1 per batch, pass 2 per call); k_line_write<true> once
        if g:
            say("k_bam_gather: %.2f ms for 2 x %d record bytes read + written (pass 1 and pass 2) = %.0f GB/s" % (g / 1e6, rec_bytes, 2 * 2 * rec_bytes / g))
        if lw:
            say("k_line_write<true>: %.2f ms for %d record bytes written = %.0f GB/s counted the same way (2 x record bytes; its source is the FASTQ text)" % (lw / 1e6, rec_bytes, 2 * rec_bytes / lw))
        for name in ("k_bam_keys", "k_bam_slen", "radix", "onesweep", "k_bgzf_block", "k_bgzf_gather"):
            t = total_ns(lambda n: name in n.lower() if name in ("radix", "onesweep") else name in n)
            if t:
                say("  %-14s %.2f ms" % (name, t / 1e6))
        if args.bai:
            for r in rows:
                if "k_bai_" in r["Name"]:
                    say("  %-14s %.3f ms in %s calls" % (r["Name"].split("(")[0], int(r["TotalDurationNs"]) / 1e6, r["Calls"]))
            say("  k_bai_* together %.3f ms beside k_bam_gather's %.2f ms (the index passes read the fixed fields and the CIGAR of each record, not the record)"
                % (total_ns(lambda n: "k_bai_" in n) / 1e6, g / 1e6))
        if args.markdup:
            for r in rows:
                if "k_dup_" in r["Name"]:
                    say("  %-14s %.3f ms in %s calls" % (r["Name"].split("(")[0], int(r["TotalDurationNs"]) / 1e6, r["Calls"]))
            say("  k_dup_* together %.3f ms beside k_bam_gather's %.2f ms (k_dup_sig reads the qualities of every record once more, the others 24-byte signatures)"
                % (total_ns(lambda n: "k_dup_" in n) / 1e6, g / 1e6))
        if args.methyl:
            for r in rows:
                if "k_meth_" in r["Name"]:
                    say("  %-14s %.3f ms in %s calls" % (r["Name"].split("(")[0], int(r["TotalDurationNs"]) / 1e6, r["Calls"]))
            say("  k_meth_* together %.3f ms beside k_bam_gather's %.2f ms (the event passes read the fixed fields, the CIGAR and, at cytosines only, bases and qualities)"
                % (total_ns(lambda n: "k_meth_" in n) / 1e6, g / 1e6))
            if args.mbias:
                mb, cnt = total_ns(lambda n: "k_meth_mbias" in n), total_ns(lambda n: "k_meth_events<false" in n)
                say("  k_meth_mbias %.3f ms beside the counting pass k_meth_events<false, ..> %.3f ms (the same walk; the tally adds one LDS or global add per call)" % (mb / 1e6, cnt / 1e6))
            if args.variant:
                opp, own = total_ns(lambda n: re.search(r"k_meth_events<\w+, \w+, true>", n)), total_ns(lambda n: re.search(r"k_meth_events<\w+, \w+, false>", n))
                if not opp or not own:
                    say("  the trace has no rows named k_meth_events<.., .., true> or none named k_meth_events<.., .., false> (%d and %d ns): the opposite passes cannot be set beside the calling passes"
                        % (opp, own))
                else:
                    say("  the opposite passes k_meth_events<.., .., true> %.3f ms beside the calling passes k_meth_events<.., .., false> (k_meth_count + k_meth_emit) %.3f ms = %.2f x (the same walk over the other half of the masks)"
                        % (opp / 1e6, own / 1e6, opp / own))
            if args.nonconv:
                for r in rows:
                    if "k_nonconv_" in r["Name"]:
                        say("  %-14s %.3f ms in %s calls" % (r["Name"].split("(")[0], int(r["TotalDurationNs"]) / 1e6, r["Calls"]))
                nw, cnt = total_ns(lambda n: "k_nonconv_walk" in n), total_ns(lambda n: "k_meth_events<false, false" in n)
                if nw and cnt:
                    say("  k_nonconv_walk %.3f ms beside the counting pass k_meth_events<false, false> %.3f ms of the same run = %.2f x (the same walk: pass 1 over every record of the batches, all three contexts, no clip; the counting pass over the records that are left, without those the filter flagged)"
                        % (nw / 1e6, cnt / 1e6, nw / cnt))
            if args.report:
                for r in rows:
                    if "k_cyt_" in r["Name"]:
                        say("  %-14s %.3f ms in %s calls" % (r["Name"].split("(")[0], int(r["TotalDurationNs"]) / 1e6, r["Calls"]))
                em = total_ns(lambda n: "k_cyt_emit" in n)
                n_b = runs["report"][-1]["report"][1]
                if em and lw:
                    say("  k_cyt_emit writes %d bytes of text in %.3f ms = %.0f GB/s; k_line_write<true> writes %d record bytes in %.2f ms = %.0f GB/s (bytes written only, same trace)"
                        % (n_b, em / 1e6, n_b / em, rec_bytes, lw / 1e6, rec_bytes / lw))
                say("  k_cyt_* together %.3f ms for the whole genome of %d bp" % (total_ns(lambda n: "k_cyt_" in n) / 1e6, args.genome))
    # ---- --variant, --report or --nonconv with --other-driver: a plain --methyl run of either build under the kernel trace -- do they launch the same kernels?
    if args.methyl and (args.variant or args.report or args.nonconv) and args.other_driver:
        seen = {}
        for who, drv_w in (("this build", drv), ("the other build", args.other_driver)):
            shutil.rmtree(tr, ignore_errors=True)
            if os.path.exists(out_s):
                os.unlink(out_s)
            step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tr, "--", drv_w] + base[1:] + ["--sort"] + meth_args + ["-o", out_s], 900)
            f = glob.glob(os.path.join(tr, "**", "*kernel_stats.csv"), recursive=True)
            seen[who] = {r["Name"]: (int(r["Calls"]), int(r["TotalDurationNs"])) for r in csv.DictReader(open(f[0]))} if f else {}
        a, b = seen["this build"], seen["the other build"]
        if not a or not b:
            say("--methyl without the filter under the kernel trace: no kernel rows for %s -- nothing to compare" % " and ".join(w for w in seen if not seen[w]))
        else:
            def calls(rows, plain):
                """name -> calls; plain: k_meth_events<x, y, false> counted as k_meth_events<x, y> (a defaulted third template argument)"""
                out = {}
                for n, (c, _ns) in rows.items():
                    n = re.sub(r"(k_meth_events<\w+, \w+), false>", r"\1>", n) if plain else n
                    out[n] = out.get(n, 0) + c
                return out
            for plain in (False, True):
                ca, cb = calls(a, plain), calls(b, plain)
                differ = sorted(n for n in set(ca) | set(cb) if ca.get(n, 0) != cb.get(n, 0))
                say("--methyl without the filter under the kernel trace, this build against the other%s: %d and %d kernel names; names and call counts %s"
                    % (", k_meth_events<x, y, false> read as k_meth_events<x, y>" if plain else "", len(ca), len(cb), "identical" if not differ else "differ in %d rows:" % len(differ)))
                for n in differ:
                    say("  %s: %d calls here, %d there" % (n.split("(")[0], ca.get(n, 0), cb.get(n, 0)))
                if not differ:
                    break
            for n in sorted(set(a) | set(b)):
                if "k_meth_" in n:
                    say("  %-40s here %d calls %.3f ms, there %d calls %.3f ms" % (n.split("(")[0], a.get(n, (0, 0))[0], a.get(n, (0, 0))[1] / 1e6, b.get(n, (0, 0))[0], b.get(n, (0, 0))[1] / 1e6))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as o:
        o.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
