// bitmapperbs_amd/csrc/bmbs_search.cpp -- C++ host driver over the C-ABI: the `bitmapperBS --search`
// command line (Process_CommandLines.cpp:88-132), FASTQ in (Process_Reads.cpp:155-317, 810-890), SAM out
// (Process_sam_out.cpp:1137-1153, Schema.cpp:11989-12039, 10537-10640, 11494-11590), mapstats
// (Bitmapper_main.cpp:266-308) -- with the per-read mapping loops of Schema.cpp replaced by batch calls into
// libbmbs_hip.so.  Record order is the input order (== the reference at -t 1).
//
//   bmbs_search --search <index prefix | dir> --seq r.fq[.gz] [-o out.sam] [-e 0.08] [--mapstats f]
//   bmbs_search --search <index> --seq1 a.fq --seq2 b.fq [--min 0] [--max 500] [--sensitive] ...
//   output variants (Process_CommandLines.cpp:93-105): --pbat, --unmapped_out, --ambiguous_out, --bam (BGZF-compressed BAM)
//   extra: --device N | --devices a,b,... (one index copy per listed device, batches dealt to whichever context is free, output
//          order kept), --contexts S (contexts per device sharing its index: S batches in flight per GPU so that the copies of
//          one overlap the kernels of another; default 4), --batch N (records per GPU batch, default 500 k), -t N (host I/O
//          threads), --out-parts N (the input is cut into N contiguous record ranges, each written to its own file
//          <out>.part000 ... concurrently; `cat` of the parts in order == the one-file output), --verbose,
//          --bam --sort [--sort-mem GiB] (ONE coordinate-sorted BAM: its records are the stable sort, by reference / position /
//          strand, of the records --bam writes; sorted on the device, see "--bam --sort" below; needs --out-parts 1)
//          --bam --sort --markdup (PCR duplicates get flag 0x400 in that file: Picard's pair-level rule, decided on the device, see
//          "--markdup" below; nothing else in any record changes)
//          --bam --sort --methyl <prefix> [--CpG] [--CHG] [--CHH] (per-cytosine methylation counts of that file's records, computed on the
//          device while its blocks are written: <prefix>_CpG.bedGraph ..., see "--methyl" below)
//          --methyl ... [--methyl-ignore n] [--methyl-ignore-3prime n] [--methyl-ignore-r2 n] [--methyl-ignore-3prime-r2 n] (cycles left
//          out of the calls at the 5' / 3' end of read 1 (or a single-end read) / read 2: Bismark's --ignore options) [--mbias]
//          (<prefix>_mbias.tsv: the calls by context, strand, read and cycle, before the trim)
//          --methyl ... [--methyl-min-opposite-depth n [--methyl-max-variant-frac f]] (a site is left out when at least n bases of the
//          OTHER bisulfite strand's reads cover it and more than the fraction f of them is not the genome's letter: a C->T polymorphism
//          of the sample, not an unmethylated cytosine; MethylDackel's --minOppositeDepth / --maxVariantFrac, a second walk on the device)
//          [--methyl-merge-context] (one line per CpG / CHG, both strands added) [--methyl-min-depth n] (lines with fewer calls are left out)
//          --methyl ... --cytosine-report [--methyl-report-window bases] (<prefix>.cytosine_report.txt: one line for EVERY cytosine of the
//          selected contexts in the genome, both strands, covered or not -- Bismark's CX_report; the lines are made on the device window
//          by window, see "--cytosine-report" below.  --methyl-merge-context and --methyl-min-depth shape the bedGraphs only: the report
//          stays per strand and includes depth 0)
//          --bam --sort --filter-non-conversion [--non-conversion-threshold n] [--non-conversion-percent p] [--non-conversion-min-count m]
//          (templates with a read the bisulfite treatment did not convert -- n methylated calls outside CpG, or p percent of at least m
//          such calls -- get flag 0x200 in every record: Bismark's filter_non_conversion, decided on the device in pass 1; every later
//          stage, --methyl included, leaves flagged records out) [--conversion-report file] (the calls of all examined records by strand
//          and context and the non-CpG conversion rate; alone it flags nothing)
//          --trim (adapter and quality trimming of every read on the device, in front of the mapping: what a pipeline otherwise runs
//          trim_galore for; its defaults -- quality 20, adapter AGATCGGAAGAGC on both mates, overlap 1, error rate 0.1, length 20; the rule
//          and its departures from cutadapt: include/bmbs.h, bmbs_set_trim) [--trim-quality n] (0: off) [--trim-adapter SEQ] (both mates
//          unless --trim-adapter2 SEQ names mate 2's; `none`: off) [--trim-stringency n] [--trim-error-rate f] [--trim-min-length n]
//          [--trim-clip-r1 n] [--trim-clip-r2 n] [--trim-three-prime-clip-r1 n] [--trim-three-prime-clip-r2 n] [--trim-report file] (the
//          totals of all batches, one line per counter and mate).  Templates that end up shorter than the minimum length (pairs: either
//          mate) are dropped: they reach no output and no statistic but the "removed by trimming" line.  M-bias cycles and
//          --methyl-ignore* count from the trimmed read's first base, as Bismark's do behind trim_galore
//
// The reference has ONE reader thread and ONE fprintf sink (Process_Reads.cpp:2057-2260, Process_sam_out.cpp:954-1006), which is
// what limits it.  Round 2 of this driver indexed the lines and formatted the SAM text with the host's
// I/O threads; those two stages were as long as the GPU stage.  Now the host touches file bytes only to move them:
//   stage R  pread of a window of the FASTQ file(s) into a page-locked buffer (parallel; .gz: one inflate thread per file); the
//            reader COUNTS the newlines (SWAR over the bytes it has just read) to know how many whole records the window holds
//   stage G  one bmbs_map_se_text / bmbs_map_pe_text call per batch: text up, newline index + rows + mapping + SAM formatting on
//            the device (bmbs_text.hip), finished SAM text down into a page-locked buffer; one worker thread per context
//   stage W  pwrite of the SAM text at the part's running offset (--bam: the text is converted to BAM records and BGZF blocks by
//            the I/O threads first, bam_prase.cpp:201-221)
// Buffered writes to ONE file serialise on its inode lock at the speed of one memcpy (~10 GB/s = 28 M SAM records/s on the MI355X
// boxes): --out-parts N gives N inodes.  Every part is a pipeline of its own (reader -> shared GPU workers -> writer) over its own
// record range of the input; for pairs the ranges are cut at the same record in both files (found by the read names, by counting
// lines when the names do not tell).
//
// This file: the state of a run (Options, Run, Pass2) and its stages as functions, main() at the end being the list of them.  What the
// stages are built from lies in search_util.h (pool, queues, page-locked buffers), search_source.h (the FASTQ reader and the cutting
// into parts; bmbs_reader_test.cpp runs it without a GPU) and search_sort.h (the store, plan and staging of --sort, .bai, --methyl).
#include "search_util.h"
#include "search_source.h"
#include "search_sort.h"
#include <sys/vfs.h>

namespace {

void print_stats(FILE* o, const int64_t st[5])
{
    long long reads = st[0], uniq = st[1], amb = st[2], unm = st[0] - st[1] - st[2];
    fprintf(o, "%-48s%lld\n", "No. of Reads:", reads);
    fprintf(o, "%-48s%lld (%0.2f%%)\n", "No. of Unique Mapped Reads:", uniq, ((double)uniq / (double)reads) * 100);
    fprintf(o, "%-48s%lld (%0.2f%%)\n", "No. of Ambiguous Mapped Reads:", amb, ((double)amb / (double)reads) * 100);
    fprintf(o, "%-48s%lld (%0.2f%%)\n", "No. of Unmapped Reads:", unm, ((double)unm / (double)reads) * 100);
    fprintf(o, "%-47s %0.2f%%\n", "Mismatch and Indel Rate:", ((double)st[4] / (double)st[3]) * 100);
}

bool is_dir(const std::string& p) { struct stat sb; return stat(p.c_str(), &sb) == 0 && S_ISDIR(sb.st_mode); }

// ================ state =========================================================================================================

// ---- what the command line says, and what follows from it alone.  Filled by parse_options, read-only afterwards. ------------------
struct Options {
    bmbs_params P;
    std::string index, seq, seq1, seq2, out = "output", mapstats, build_fasta, index_folder;
    std::string methyl;                          // --methyl <prefix>: <prefix>_CpG.bedGraph ... from the sorted file's records
    std::vector<std::string> args;               // argv as given (the @PG line)
    std::vector<int> devices;
    int io_threads = 0, contexts = 4, parts = 1, reader_threads = 0, loop_input = 1;
    long batch = 500000;
    bool verbose = false, unmapped_out = false, pbat = false, bam = false, print_parts = false, print_plan = false;
    bool sort = false, bai = false, markdup = false;
    bmbs_methyl_params mpar = {0, 10, 5, 0};     // --CpG (the default) --CHG --CHH, --methyl-min-mapq, --methyl-min-phred
    long ignore[4] = {0, 0, 0, 0};               // --methyl-ignore, --methyl-ignore-r2 (5' of mate 0, 1), --methyl-ignore-3prime, --methyl-ignore-3prime-r2 (3')
    bool ignore_given = false, mbias = false;    // --mbias: <prefix>_mbias.tsv
    long min_opp_depth = 0;                      // --methyl-min-opposite-depth (0: no variant filter), --methyl-max-variant-frac in parts per million,
    int32_t max_variant_ppm = 0;                 // --methyl-min-depth, --methyl-merge-context
    long min_depth = 1;
    bool variant_frac_given = false, site_opts_given = false, merge_context = false;
    bool cytosine_report = false;                // --cytosine-report: <prefix>.cytosine_report.txt, every cytosine of the selected contexts
    long report_window = 0;                      // --methyl-report-window: bases per bmbs_methyl_report call (0: what fits the buffers, write_report)
    // --filter-non-conversion: templates with unconverted reads get flag 0x200 (--non-conversion-threshold, -percent, -min-count set the
    // rule and imply the switch); --conversion-report <file>: the calls of all examined records and the non-CpG conversion rate
    bool nonconv_filter = false;
    bmbs_nonconv_params ncpar = {3, 0, 5, 0};
    std::string conversion_report;
    bool nonconv = false;                        // derived: pass 1 calls bmbs_text_sorted_nonconv (the filter, the report or both)
    // --trim: the reads are trimmed on the device before they are mapped (bmbs_set_trim); the --trim-* refinements need it
    bool trim = false, trim_opt_given = false, trim_a2_given = false;
    bmbs_trim_opts tpar = {20, 1, 100, 20, {0, 0}, {0, 0}, {"AGATCGGAAGAGC", "AGATCGGAAGAGC"}};
    std::string trim_report;
    double sort_mem_gib = 0;                     // --sort-mem: cap of the in-memory record store of --sort (0: half of the machine's memory)
    // derived once
    bool pe = false, gz_in = false, methyl_out = false;
    bool methyl_clip = false;                    // --methyl of pairs: the records carry their mate-overlap clips
    bool methyl_use_opts = false;                // a trim or --mbias: pass 2 calls bmbs_bam_sort_methyl_opts with mopt (else bmbs_bam_sort_methyl, as ever)
    bmbs_methyl_opts mopt = {1, 10, 5, 0, {0, 0}, {0, 0}};
    bmbs_methyl_opts oopt = {1, 10, 5, 0, {0, 0}, {0, 0}};      // the variant filter: what pass 2 calls bmbs_bam_sort_methyl_opposite with (mopt without flags)
    std::string in1;                             // the first (or only) read file
    int live_parts = 1;                          // a .gz stream cannot be entered in the middle: everything goes through part 0, the other part files stay empty
    int32_t flags = 0;                           // BMBS_TEXT_* of every mapping call
    int nf() const { return pe ? 2 : 1; }
    int n_ctx() const { return (int)devices.size() * contexts; }
};

struct Part;
struct Batch {
    Part* part = nullptr;
    long seq = 0;                                // position within the part (output order)
    long n = 0;                                  // records (pairs)
    bool end = false;                            // the part's input ends with this batch
    Pinned text1, text2, sam;                    // FASTQ windows in, SAM text out
    size_t used1 = 0, used2 = 0;
    uint64_t sam_bytes = 0;
    std::vector<uint64_t> skey; std::vector<uint32_t> slen; int64_t n_sorted = 0;      // --sort: key and length of each record in `sam`
    std::vector<bmbs_dup_sig> sig; std::vector<uint32_t> tmpl; int64_t n_sig = 0;      // --markdup: the batch's signatures, the template of each record in `sam`
    std::vector<uint32_t> clip;                                                         // --methyl of pairs: the mate-overlap clip of each record in `sam`
    std::vector<uint8_t> ncfail;                                                        // --filter-non-conversion: 1 for each record in `sam` whose template failed
    std::vector<uint32_t> counts1, counts2;
    bmbs_ctx* open_ctx = nullptr;                // compressed input kept on the device: the context that holds this batch's open window
};
// (a batch belongs to one thread at a time: whoever took it from free_q, gpu_q or the part's out_q, until it puts it into the next)

struct Part {                                    // one contiguous record range of the input -> one output file
    int id = 0;
    Source s1, s2;                               // the part's reader; while its `ahead` thread stages a BGZF window, that thread has znext, zblk, zout and loops_left, the reader `carry`
    int ofd = -1;
    size_t out_off = 0;                          // the part's writer while it runs; main before (header) and after it has joined (pass 2, EOF block)
    size_t alloc_end = 0;                        // the file's blocks are reserved up to here (fallocate ahead of the writers); the writer, then main (ftruncate)
    bool can_alloc = true, regular = false;      // set by main before the threads start; can_alloc: the writer alone from then on
    OrderedChan<Batch*> out_q;                   // gpu workers put, the part's writer gets
    long next_seq = 0;                           // the part's reader alone
    std::thread reader, writer;
    double t_read = 0, t_wait_r = 0; long records = 0;      // the reader alone; main after the join
    double t_write = 0, t_wait_w = 0;                        // the writer alone; main after the join
};

// BGZF input that is inflated on the device: the compressed bytes of a window, staged (block tables and a page-locked copy per
// file).  Two of them: while a context opens one window, a helper thread stages the next
struct Staged {
    Pinned buf[2]; std::vector<uint64_t> blk[2], out[2];
    size_t a[2] = {0, 0}, q[2] = {0, 0};
    bool foreign_any = false, ok = true; std::string err;
    bool last[2] = {false, false};               // the window ends its file (--loop-input: for the last time)
};

// ---- the shared state of a mapping run ------------------------------------------------------------------------------------------
struct Run {
    const Options& o;
    // the index and the contexts: written by load_index_and_contexts, read-only while the threads run
    std::string index;                           // the index prefix (--search, or <dir>/genome)
    bmbs_index_file* ixf = nullptr;
    bmbs_index_view view;
    std::vector<std::string> chrom_names;
    size_t max_chrom = 0;
    std::vector<bmbs_ctx*> ctxs;                 // owners first
    size_t n_owner = 0;
    size_t est0 = 400;                           // bytes per record of the input, from its first records; read-only
    std::vector<Batch> batches;                  // n_batches = live_parts + n_ctx + 2; the pre-allocation threads pin them, one batch each
    Staged zst[2];                               // the one reader of device-inflated input and its `ahead` thread: one window each, handed over by thread start and join
    std::thread prealloc;                        // main starts and joins it
    Joiner prealloc_guard{prealloc};             // error returns must not leave it running (declared behind what it writes to)
    Chan<Batch*> free_q, gpu_q;                  // writers -> readers -> gpu workers
    Chan<bmbs_ctx*> ctx_pool;                    // device-inflated input: contexts without an open window (the reader takes, whoever ends the batch's call gives back)
    std::vector<std::unique_ptr<Part>> parts;
    int r_threads = 1;
    SortStore sort_store;                        // --sort: filled by the ONE writer (--sort: one part), read by main and pass 2 after it has joined
    uint64_t tmpl_base = 0;                      // --markdup: template ids run over the batches in Batch.seq order; the ONE writer alone
    std::atomic<bool> failed{false};             // any thread
    std::mutex err_mu;                           // the first failure's message
    std::mutex g_mu;                             // t_gpu and t_wait_g: the gpu workers add under it, main reads after their join
    double t_gpu = 0, t_wait_g = 0;
    // --filter-non-conversion / --conversion-report: the batches' totals, templates and failed templates added up (under g_mu, as t_gpu)
    uint64_t nc_totals[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    long nc_templates = 0, nc_failed = 0;
    // --trim: the batches' counters and kept templates added up (under g_mu, as t_gpu)
    bmbs_trim_counts trim_cnt = {};
    long trim_in = 0, trim_kept = 0;
    double t_start = 0, t_loaded = 0, t_pass1 = 0, t_pass2 = 0, t_joined = 0;      // main alone

    explicit Run(const Options& opt) : o(opt), batches((size_t)(opt.live_parts + opt.n_ctx() + 2))
    {
        for (auto& b : batches) { b.text1.kind = 1; b.text2.kind = 1; b.sam.kind = 2; }
        for (auto& x : zst) { x.buf[0].kind = 1; x.buf[1].kind = 1; }
    }
    void fail(const std::string& why) { std::lock_guard<std::mutex> l(err_mu); if (!failed.exchange(true)) fprintf(stderr, "bmbs_search: %s\n", why.c_str()); }
    // the device inflates this part's input: the reader opens windows on contexts of ctx_pool
    bool z_mode(const Part& pt) const { return pt.s1.zdirect && (!o.pe || pt.s2.zdirect); }

    // ---- the sizes of the page-locked windows (one home: the pre-allocation and both readers) ----
    static constexpr size_t host_window_cap = (size_t)4000 << 20, bgzf_window_cap = (size_t)3500 << 20;
    // text bytes of a window of --batch records of `est` bytes each
    size_t window_bytes(size_t est, size_t cap) const { return std::min<size_t>((size_t)o.batch * est + (1u << 16), cap); }
    // SAM bytes a batch can need: QNAME + SEQ + QUAL come out of the text, the other columns are bounded per line
    size_t sam_bound(size_t text_bytes, size_t lines, int L) const
    {
        return text_bytes + lines * (max_chrom + 5 * (size_t)std::max(8, (int)bmbs_max_cigar_ops(&o.P, std::max(1, std::min(1000, L)))) + 96) + 4096;
    }
};

// ---- --sort, pass 2: main, its stager and its sorters ----------------------------------------------------------------------------------
struct Slot {
    Pinned in, out; std::vector<uint32_t> len, clip; size_t unit = 0; uint64_t out_bytes = 0; BaiPieces bai; std::vector<bmbs_methyl_site> site; int64_t n_site = 0;
    std::vector<uint64_t> mbias;                 // --mbias: the call's table
    std::vector<bmbs_methyl_site> opp; int64_t n_opp = 0;      // the variant filter: the call's opposite-strand entries
};
// (a slot belongs to one thread at a time: free_s -> stager -> staged_s -> a sorter -> done_s -> main)
struct Pass2 {
    std::vector<SortUnit> units;                 // written by main before the threads start, read-only then
    int n_slots = 1;
    std::vector<Slot> slots;
    Chan<Slot*> free_s, staged_s;
    OrderedChan<Slot*> done_s;                   // hands the calls to main in unit order
    std::vector<uint64_t> dup_bits;              // --markdup: a bit per template id, set for duplicates; dup_select_pass writes, the stager reads
    BaiIndex bai;                                // main alone (the calls' pieces, in call order)
    std::vector<bmbs_methyl_site> meth_sites;    // --methyl: the sites of the calls so far, merged; main alone
    std::vector<bmbs_methyl_site> meth_opp;      // the variant filter: the opposite-strand entries of the calls so far, merged the same way; main alone
    size_t meth_variants = 0, meth_shallow = 0;  // sites dropped as variants, lines left out below --methyl-min-depth
    uint64_t report_lines = 0, report_bytes = 0; // --cytosine-report: what the file holds; the seconds it took, of which inside the device
    double t_report = 0, t_report_calls = 0, t_report_wait = 0;      // calls, and waiting for the writer to hand a buffer back
    std::vector<uint64_t> mbias;                 // --mbias: the tables of the calls so far, added up; main alone
    uint64_t mbias_calls = 0;                    // ... and its total
    size_t sort_calls = 0, select_calls = 0, n_dup = 0, bai_bytes = 0;
    size_t meth_n[3] = {0, 0, 0}, meth_calls[3] = {0, 0, 0}, meth_dropped = 0;
    double t_select = 0;
};
const char* const ctx_names[3] = {"CpG", "CHG", "CHH"};

// ================ the command line ===============================================================================================
[[noreturn]] void refuse(const char* msg) { fputs(msg, stderr); exit(2); }

const char* const USAGE =
    "usage: bmbs_search --index <genome.fa> [--index_folder dir] [-t threads]\n       bmbs_search --search <index> (--seq r.fq | --seq1 a.fq --seq2 b.fq) [-o out.sam] [-e f] [--min n] [--max n] [--sensitive] [--pbat] [--unmapped_out] [--ambiguous_out] [--bam [--sort [--sort-mem GiB] [--markdup] [--bai] [--methyl prefix [--CpG] [--CHG] [--CHH] [--methyl-min-mapq n] [--methyl-min-phred n] [--methyl-ignore n] [--methyl-ignore-3prime n] [--methyl-ignore-r2 n] [--methyl-ignore-3prime-r2 n] [--mbias] [--methyl-min-opposite-depth n [--methyl-max-variant-frac f]] [--methyl-merge-context] [--methyl-min-depth n] [--cytosine-report [--methyl-report-window bases]]] [--filter-non-conversion] [--non-conversion-threshold n] [--non-conversion-percent p] [--non-conversion-min-count m] [--conversion-report file]]] [--trim [--trim-quality n] [--trim-adapter SEQ] [--trim-adapter2 SEQ] [--trim-stringency n] [--trim-error-rate f] [--trim-min-length n] [--trim-clip-r1 n] [--trim-clip-r2 n] [--trim-three-prime-clip-r1 n] [--trim-three-prime-clip-r2 n] [--trim-report file]] [--mapstats f] [-t io_threads] [--out-parts n]\n       --trim: quality (20) and adapter (AGATCGGAAGAGC, overlap 1, error rate 0.1) trimming of every read on the device before it is mapped, reads below 20 bases (pairs: either mate) dropped -- trim_galore's defaults; the leftmost accepted adapter start without indels, not cutadapt's best alignment; --trim-adapter sets both mates unless --trim-adapter2 is given, `none` turns the adapter step off, --trim-quality 0 the quality step; --trim-report: the counters of the run, one line per counter and mate\n       --cytosine-report: <prefix>.cytosine_report.txt, one line per cytosine of the selected contexts on both strands, covered or not; --methyl-merge-context and --methyl-min-depth shape the bedGraphs only, the report stays per strand and includes depth 0\n       --filter-non-conversion: flag 0x200 on every record of a template with a read that has 3 (--non-conversion-threshold) methylated calls outside CpG, or --non-conversion-percent of at least 5 (--non-conversion-min-count) such calls; --conversion-report: the calls of all examined records and the non-CpG conversion rate\n";

Options parse_options(int argc, char** argv)
{
    Options o;
    bmbs_params& P = o.P; bmbs_default_params(&P);
    bmbs_methyl_params& mpar = o.mpar;
    int device = 0;
    o.args.assign(argv, argv + argc);
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto val = [&]() -> const char* { if (i + 1 >= argc) { fprintf(stderr, "missing value for %s\n", a.c_str()); exit(2); } return argv[++i]; };
        if (a == "--search") o.index = val();
        else if (a == "--index") o.build_fasta = val();               // Process_CommandLines.cpp:107, 364-381
        else if (a == "--index_folder") o.index_folder = val();
        else if (a == "--seq") o.seq = val();
        else if (a == "--seq1") o.seq1 = val();
        else if (a == "--seq2") o.seq2 = val();
        else if (a == "-o") o.out = val();
        else if (a == "-e") P.e_f = atof(val());
        else if (a == "--min") P.min_ins = atoi(val());
        else if (a == "--max") P.max_ins = atoi(val());
        else if (a == "--mp_max") P.mp_max = atoi(val());
        else if (a == "--mp_min") P.mp_min = atoi(val());
        else if (a == "--np") P.np = atoi(val());
        else if (a == "--gap_open") P.gap_open = atoi(val());
        else if (a == "--gap_extension") P.gap_ext = atoi(val());
        else if (a == "--seed") P.seed_len = atoi(val());
        else if (a == "--phred33") P.q_base = 33;
        else if (a == "--phred64") P.q_base = 64;
        else if (a == "--sensitive") P.sensitive = 1;
        else if (a == "--fast") P.sensitive = 0;
        else if (a == "--pe") {}
        else if (a == "-t") o.io_threads = atoi(val());  // the reference's mapping threads; here: host I/O threads (the GPU maps)
        else if (a == "--mapstats") o.mapstats = val();
        else if (a == "--device") device = atoi(val());
        else if (a == "--devices") {                                  // comma-separated device ids, one index copy each
            const char* v = val();
            o.devices.clear();
            for (const char* q = v; *q;) { o.devices.push_back(atoi(q)); while (*q && *q != ',') q++; if (*q == ',') q++; }
        }
        else if (a == "--contexts") o.contexts = atoi(val());
        else if (a == "--batch") o.batch = atol(val());
        else if (a == "--loop-input") o.loop_input = std::max(1, atoi(val()));
        else if (a == "--out-parts") o.parts = atoi(val());
        else if (a == "--print-plan") o.print_parts = o.print_plan = true;       // ... and how the parts are worked off: devices, contexts, workers (no GPU needed: tests)
        else if (a == "--print-parts") o.print_parts = true;                 // the record ranges --out-parts would use, then exit (no GPU needed: tests)
        else if (a == "--reader-threads") o.reader_threads = atoi(val());   // pread threads per part (default: -t / (2 x parts))
        else if (a == "--verbose") o.verbose = true;
        else if (a == "--unmapped_out") o.unmapped_out = true;        // Process_CommandLines.cpp:104-105
        else if (a == "--ambiguous_out") P.ambiguous_out = 1;
        else if (a == "--pbat") o.pbat = true;                        // Process_CommandLines.cpp:93
        else if (a == "--bam") o.bam = true;                          // Process_CommandLines.cpp:94-95
        else if (a == "--sam") o.bam = false;
        else if (a == "--sort") o.sort = true;                        // --bam --sort: one coordinate-sorted BAM file (sorted on the device)
        else if (a == "--sort-mem") o.sort_mem_gib = atof(val());
        else if (a == "--markdup") o.markdup = true;                 // --bam --sort --markdup: flag 0x400 on PCR duplicates, decided on the device
        else if (a == "--bai") o.bai = true;                          // --bam --sort --bai: <out>.bai beside the sorted file, from the same run
        else if (a == "--methyl") o.methyl = val();                   // --bam --sort --methyl <prefix>: methylation counts per cytosine, from the device
        else if (a == "--CpG") mpar.contexts |= 1;                    // (the reference's names for the contexts of its own extractor)
        else if (a == "--CHG") mpar.contexts |= 2;
        else if (a == "--CHH") mpar.contexts |= 4;
        else if (a == "--methyl-min-mapq") mpar.min_mapq = atoi(val());
        else if (a == "--methyl-min-phred") mpar.min_phred = atoi(val());
        else if (a == "--methyl-ignore" || a == "--methyl-ignore-r2" || a == "--methyl-ignore-3prime" || a == "--methyl-ignore-3prime-r2") {
            char* end = nullptr;
            const char* v = val();
            const long x = strtol(v, &end, 10);
            if (end == v || *end || x < 0 || x > 65535) { fprintf(stderr, "bmbs_search: %s takes 0..65535\n", a.c_str()); exit(2); }
            o.ignore[(a.find("3prime") != std::string::npos ? 2 : 0) + (a.size() > 3 && a.compare(a.size() - 3, 3, "-r2") == 0 ? 1 : 0)] = x;
            o.ignore_given = true;
        }
        else if (a == "--mbias") o.mbias = true;                      // --methyl ... --mbias: <prefix>_mbias.tsv
        else if (a == "--methyl-min-opposite-depth" || a == "--methyl-min-depth") {      // MethylDackel's --minOppositeDepth, --minDepth
            const bool opp = a == "--methyl-min-opposite-depth";
            char* end = nullptr;
            const char* v = val();
            const long x = strtol(v, &end, 10);
            if (end == v || *end || x < (opp ? 0 : 1) || x > (opp ? 65535 : 2147483647l)) { fprintf(stderr, "bmbs_search: %s takes %s\n", a.c_str(), opp ? "0..65535" : "1..2147483647"); exit(2); }
            (opp ? o.min_opp_depth : o.min_depth) = x;
            o.site_opts_given = true;
        }
        else if (a == "--methyl-max-variant-frac") {                  // MethylDackel's --maxVariantFrac
            if (!methyl_parse_frac(val(), &o.max_variant_ppm)) refuse("bmbs_search: --methyl-max-variant-frac takes a plain decimal in 0..1 with at most 6 digits behind the point\n");
            o.variant_frac_given = o.site_opts_given = true;
        }
        else if (a == "--methyl-merge-context") o.merge_context = o.site_opts_given = true;      // MethylDackel's --mergeContext
        else if (a == "--filter-non-conversion") o.nonconv_filter = true;      // --bam --sort --filter-non-conversion: flag 0x200 on unconverted templates, decided on the device
        else if (a == "--non-conversion-threshold" || a == "--non-conversion-percent" || a == "--non-conversion-min-count") {      // Bismark's --threshold, --percentage_cutoff, --minimum_count
            const bool pct = a == "--non-conversion-percent";
            char* end = nullptr;
            const char* v = val();
            const long x = strtol(v, &end, 10);
            if (end == v || *end || x < 0 || x > (pct ? 100 : 2147483647l)) { fprintf(stderr, "bmbs_search: %s takes %s\n", a.c_str(), pct ? "0..100" : "0..2147483647"); exit(2); }
            (pct ? o.ncpar.percent : a == "--non-conversion-threshold" ? o.ncpar.threshold : o.ncpar.min_count) = (int32_t)x;
            o.nonconv_filter = true;
        }
        else if (a == "--trim") o.trim = true;                         // trim_galore's defaults, on the device (bmbs_set_trim)
        else if (a == "--trim-adapter" || a == "--trim-adapter2") {
            std::string v = val();
            if (v == "none") v.clear();
            if (v.size() > 32) { fprintf(stderr, "bmbs_search: %s takes at most 32 letters\n", a.c_str()); exit(2); }
            const bool second = a == "--trim-adapter2";
            if (second) o.trim_a2_given = true;
            for (int m = second ? 1 : 0; m < 2; m++) if (m == (second ? 1 : 0) || !o.trim_a2_given) { memset(o.tpar.adapter[m], 0, sizeof o.tpar.adapter[m]); memcpy(o.tpar.adapter[m], v.data(), v.size()); }
            o.trim_opt_given = true;
        }
        else if (a == "--trim-error-rate") {
            int32_t ppm = 0;
            if (!methyl_parse_frac(val(), &ppm) || ppm % 1000) refuse("bmbs_search: --trim-error-rate takes a plain decimal in 0..1 with at most 3 digits behind the point\n");
            o.tpar.error_permille = ppm / 1000;
            o.trim_opt_given = true;
        }
        else if (a == "--trim-report") { o.trim_report = val(); o.trim_opt_given = true; }
        else if (a == "--trim-quality" || a == "--trim-stringency" || a == "--trim-min-length" || a == "--trim-clip-r1" || a == "--trim-clip-r2" || a == "--trim-three-prime-clip-r1" ||
                 a == "--trim-three-prime-clip-r2") {
            const bool q = a == "--trim-quality", len = a == "--trim-min-length", ov = a == "--trim-stringency";
            const long lo = len || ov ? 1 : 0, hi = q ? 255 : 65535;
            char* end = nullptr;
            const char* v = val();
            const long x = strtol(v, &end, 10);
            if (end == v || *end || x < lo || x > hi) { fprintf(stderr, "bmbs_search: %s takes %ld..%ld\n", a.c_str(), lo, hi); exit(2); }
            const int mate = a.back() == '2' ? 1 : 0;                 // (of the four clips)
            (q ? o.tpar.quality : len ? o.tpar.min_length : ov ? o.tpar.min_overlap : a.find("three-prime") != std::string::npos ? o.tpar.clip_3p[mate] : o.tpar.clip_5p[mate]) = (int32_t)x;
            o.trim_opt_given = true;
        }
        else if (a == "--conversion-report") o.conversion_report = val();      // the calls of all examined records, the non-CpG conversion rate
        else if (a == "--help" || a == "-h") { fputs(USAGE, stdout); exit(0); }
        else if (a == "--cytosine-report") o.cytosine_report = true;  // --methyl ... --cytosine-report: Bismark's CX_report, from the device
        else if (a == "--methyl-report-window") {
            char* end = nullptr;
            const char* v = val();
            const long x = strtol(v, &end, 10);
            if (end == v || *end || x < 1 || x > 2147483647l) refuse("bmbs_search: --methyl-report-window takes 1..2147483647 (bases)\n");
            o.report_window = x;
        }
        else { fprintf(stderr, "bmbs_search: unsupported option %s\n", a.c_str()); exit(2); }
    }
    if (o.sort && !o.bam) refuse("bmbs_search: --sort needs --bam\n");
    if (o.sort && o.parts > 1) refuse("bmbs_search: --sort writes one file (--out-parts 1)\n");
    if (o.bai && !o.sort) refuse("bmbs_search: --bai needs --sort\n");
    if (o.markdup && !o.sort) refuse("bmbs_search: --markdup needs --sort\n");
    if (o.nonconv_filter && !o.sort) refuse("bmbs_search: --filter-non-conversion, --non-conversion-threshold, --non-conversion-percent and --non-conversion-min-count need --sort\n");
    if (!o.conversion_report.empty() && !o.sort) refuse("bmbs_search: --conversion-report needs --sort\n");
    o.nonconv = o.nonconv_filter || !o.conversion_report.empty();
    if (!o.nonconv_filter) o.ncpar.threshold = o.ncpar.percent = 0;      // (--conversion-report alone: nothing fails, the totals are still produced)
    if (o.trim_opt_given && !o.trim) refuse("bmbs_search: --trim-quality, --trim-adapter, --trim-adapter2, --trim-stringency, --trim-error-rate, --trim-min-length, --trim-clip-r1, --trim-clip-r2, --trim-three-prime-clip-r1, --trim-three-prime-clip-r2 and --trim-report need --trim\n");
    for (int m = 0; m < 2; m++)
        for (const char* q = o.tpar.adapter[m]; *q; q++)
            if (!strchr("ACGTacgt", *q)) { fprintf(stderr, "bmbs_search: --trim-adapter%s takes letters of ACGT (or `none`)\n", m ? "2" : ""); exit(2); }
    o.methyl_out = !o.methyl.empty();
    if (o.methyl_out && !o.sort) refuse("bmbs_search: --methyl needs --sort\n");
    if (!o.methyl_out && (mpar.contexts || mpar.min_mapq != 10 || mpar.min_phred != 5)) refuse("bmbs_search: --CpG, --CHG, --CHH, --methyl-min-mapq and --methyl-min-phred need --methyl\n");
    if (mpar.min_mapq < 0 || mpar.min_mapq > 255 || mpar.min_phred < 0 || mpar.min_phred > 255) refuse("bmbs_search: --methyl-min-mapq and --methyl-min-phred take 0..255\n");
    if (!o.methyl_out && o.ignore_given) refuse("bmbs_search: --methyl-ignore, --methyl-ignore-3prime, --methyl-ignore-r2 and --methyl-ignore-3prime-r2 need --methyl\n");
    if (!o.methyl_out && o.mbias) refuse("bmbs_search: --mbias needs --methyl\n");
    if (!o.methyl_out && o.site_opts_given) refuse("bmbs_search: --methyl-min-opposite-depth, --methyl-max-variant-frac, --methyl-min-depth and --methyl-merge-context need --methyl\n");
    if (!o.methyl_out && (o.cytosine_report || o.report_window)) refuse("bmbs_search: --cytosine-report and --methyl-report-window need --methyl\n");
    if (o.report_window && !o.cytosine_report) refuse("bmbs_search: --methyl-report-window needs --cytosine-report\n");
    if (o.variant_frac_given && o.min_opp_depth < 1) refuse("bmbs_search: --methyl-max-variant-frac needs --methyl-min-opposite-depth above 0\n");
    if (!mpar.contexts) mpar.contexts = 1;
    if (o.merge_context && !(mpar.contexts & 3)) refuse("bmbs_search: --methyl-merge-context needs --CpG or --CHG (CHH is never merged)\n");
    o.methyl_use_opts = o.mbias || o.ignore[0] || o.ignore[1] || o.ignore[2] || o.ignore[3];
    o.mopt = bmbs_methyl_opts{mpar.contexts, mpar.min_mapq, mpar.min_phred, o.mbias ? BMBS_METHYL_MBIAS : 0, {(int32_t)o.ignore[0], (int32_t)o.ignore[1]}, {(int32_t)o.ignore[2], (int32_t)o.ignore[3]}};
    o.oopt = o.mopt; o.oopt.flags = 0;
    if (o.bai) {
        // the index lies beside a file: a device or a pipe has no such place
        struct stat osb;
        if (stat(o.out.c_str(), &osb) == 0 && !S_ISREG(osb.st_mode)) { fprintf(stderr, "bmbs_search: --bai needs a regular output file (-o %s is none)\n", o.out.c_str()); exit(2); }
    }
    if (!o.build_fasta.empty()) return o;            // --index: nothing below applies
    if (o.index.empty() || (o.seq.empty() && (o.seq1.empty() || o.seq2.empty())))
        refuse(USAGE);
    if (o.batch < 1) o.batch = 1;
    if (o.io_threads <= 0) {
        // plain text needs few threads to read at memory speed; compressed input is inflated by them (csrc/pgz.h): more pay off
        const bool zin = Source::is_gz(o.seq.empty() ? o.seq1.c_str() : o.seq.c_str());
        const int hw = (int)std::thread::hardware_concurrency();
        // what the process may actually use: a container's CPU quota (cgroup v2 cpu.max "quota period") is often far below the hardware
        // threads it can see -- 16 cores' worth of 256 on the MI355X boxes -- and inflating on four times as many threads as that is slower
        int eff = hw;
        if (FILE* cf = fopen("/sys/fs/cgroup/cpu.max", "r")) {
            long long quota = 0, period = 0;
            if (fscanf(cf, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0) eff = (int)std::max<long long>(1, std::min<long long>(hw, (quota + period - 1) / period));
            fclose(cf);
        }
        o.io_threads = zin ? std::min(std::max(1, eff), 64) : std::min(hw, 32);
    }
    if (o.io_threads < 1) o.io_threads = 1;
    if (o.parts < 1) o.parts = 1;
    if (o.parts > 64) o.parts = 64;
    if (o.devices.empty()) o.devices.push_back(device);
    if (o.contexts < 1) o.contexts = 1;
    o.pe = o.seq.empty();
    // --pbat: single-end reads are mapped as their reverse complement with mirrored qualities (inputReads_single_directly_pbat,
    // Process_Reads.cpp:986-1075; Schema.cpp:15102 need_reverse_quality = 1); paired-end input files swap roles
    // (exchange_two_reads, Process_Reads.cpp:1628, called from Bitmapper_main.cpp:169)
    if (o.pbat && o.pe) std::swap(o.seq1, o.seq2);
    // (... and with them what --trim is told about read 1 and read 2)
    if (o.pbat && o.pe) { std::swap(o.tpar.clip_5p[0], o.tpar.clip_5p[1]); std::swap(o.tpar.clip_3p[0], o.tpar.clip_3p[1]); std::swap(o.tpar.adapter[0], o.tpar.adapter[1]); }
    o.in1 = o.pe ? o.seq1 : o.seq;
    o.gz_in = Source::is_gz(o.in1.c_str()) || (o.pe && Source::is_gz(o.seq2.c_str()));
    o.live_parts = o.gz_in ? 1 : o.parts;
    o.methyl_clip = o.methyl_out && o.pe;
    o.flags = (o.pbat && !o.pe ? BMBS_TEXT_PBAT : 0) | (o.unmapped_out ? BMBS_TEXT_UNMAPPED : 0) | (o.bam ? BMBS_TEXT_BAM : 0) | (o.sort ? BMBS_TEXT_BAM_SORTED : 0);
    return o;
}

// bitmapperBS --index <fasta> [--index_folder <dir>]: <fasta>.index* or <dir>/genome.index* (Index.cpp:832-938)
int build_index(const Options& o)
{
    std::string prefix = o.build_fasta, folder = o.index_folder;
    if (!folder.empty()) {
        while (folder.size() > 1 && folder.back() == '/') folder.pop_back();
        ::mkdir(folder.c_str(), 0755);
        prefix = folder + "/genome";
    }
    const int threads = o.io_threads <= 0 ? (int)std::thread::hardware_concurrency() : o.io_threads;
    const double t0 = now();
    const int rc = bmbs_index_build(o.build_fasta.c_str(), prefix.c_str(), threads < 1 ? 1 : threads);
    if (rc) { fprintf(stderr, "bmbs_search: index build failed (%d)\n", rc); return 1; }
    fprintf(stderr, "index written to %s.index* in %.1f s\n", prefix.c_str(), now() - t0);
    return 0;
}

// ================ the parts ======================================================================================================
// where the parts begin: byte offsets of record starts, the same record in both files of a pair (plain files; a .gz stream cannot
// be entered in the middle)
bool compute_cuts(const Options& o, std::vector<size_t>& cut1, std::vector<size_t>& cut2)
{
    const int live_parts = o.live_parts;
    cut1.assign((size_t)live_parts + 1, 0); cut2.assign((size_t)live_parts + 1, 0);
    if (o.gz_in) { cut1[1] = cut2[1] = ~(size_t)0; return true; }
    Pool pool(std::max(1, o.io_threads / 2) - 1);
    const int fd1 = ::open(o.in1.c_str(), O_RDONLY), fd2 = o.pe ? ::open(o.seq2.c_str(), O_RDONLY) : -1;
    struct stat sb1, sb2;
    if (fd1 < 0 || fstat(fd1, &sb1) || (o.pe && (fd2 < 0 || fstat(fd2, &sb2)))) return false;
    const size_t size1 = (size_t)sb1.st_size, size2 = o.pe ? (size_t)sb2.st_size : 0;
    cut1[(size_t)live_parts] = size1; cut2[(size_t)live_parts] = size2;
    for (int p = 1; p < live_parts; p++) {
        cut1[(size_t)p] = std::max(cut1[(size_t)p - 1], record_start_at(fd1, size1, (size_t)((double)size1 * p / live_parts)));
        if (o.pe) cut2[(size_t)p] = std::max(cut2[(size_t)p - 1], mate_boundary(pool, fd1, size1, cut1[(size_t)p], fd2, size2));
    }
    ::close(fd1); if (fd2 >= 0) ::close(fd2);
    return true;
}

// --print-parts, --print-plan
int print_parts_and_plan(const Options& o)
{
    std::vector<size_t> cut1, cut2;
    if (!compute_cuts(o, cut1, cut2)) { fprintf(stderr, "Cannot open the read file(s)\n"); return 1; }
    for (int p = 0; p <= o.live_parts; p++) printf("%d\t%zu\t%zu\n", p, cut1[(size_t)p], cut2[(size_t)p]);
    if (o.print_plan) {
        // record ranges of the input -> GPUs, index replicated, no exchange step, output concatenated in range order.
        // Here a range is a part; its batches go to whichever context is free (one worker thread per context, `contexts` contexts
        // on every listed device sharing that device's index copy) and come back in order through the part's own queue.
        printf("plan\tdevices\t%zu\tcontexts_per_device\t%d\tworkers\t%zu\tparts\t%d\tbatches_in_flight\t%zu\tbatch\t%ld\n",
               o.devices.size(), o.contexts, o.devices.size() * (size_t)o.contexts, o.live_parts, (size_t)o.live_parts + o.devices.size() * (size_t)o.contexts + 2, o.batch);
        for (size_t d = 0; d < o.devices.size(); d++) printf("device\t%d\tindex_copy\t1\tcontexts\t%d\n", o.devices[d], o.contexts);
        printf("stats\tsum over %zu contexts (bmbs_stats_allreduce)\n", o.devices.size() * (size_t)o.contexts);
    }
    return 0;
}

// bytes per record of the input, from its first records (plain text): sizes the page-locked windows, which cost ~0.2 ms per MB
// to pin and are therefore allocated once, by several threads, while the index loads
size_t record_bytes_estimate(const std::string& path)
{
    size_t est0 = 400;
    char head[1 << 16];
    FILE* fp = fopen(path.c_str(), "rb");
    const size_t got = fp ? fread(head, 1, sizeof head, fp) : 0;
    if (fp) fclose(fp);
    if (got > 2 && !((unsigned char)head[0] == 0x1f && (unsigned char)head[1] == 0x8b)) {
        size_t lines = 0, last = 0;
        for (size_t i = 0; i < got; i++) if (head[i] == '\n') { lines++; if (lines % 4 == 0) last = i + 1; }
        if (lines >= 4) est0 = std::max<size_t>(est0, last / (lines / 4) + 32);
    }
    return est0;
}

// ================ set-up ==========================================================================================================
// the page-locked windows of every batch (and of the two staged windows of compressed input), pinned side by side
void prealloc_buffers(Run& R)
{
    const Options& o = R.o;
    const size_t want = R.window_bytes(R.est0, Run::host_window_cap) + 64;
    const int L_est = (int)std::min<size_t>(1000, (R.est0 / 2) + (R.est0 / 4));
    std::vector<std::thread> th;
    if (o.gz_in)
        for (auto& x : R.zst)
            for (int f = 0; f < o.nf(); f++) {
                struct stat sb;
                const size_t fsize = stat((f ? o.seq2 : o.in1).c_str(), &sb) == 0 ? (size_t)sb.st_size : 0;
                Pinned* pb = &x.buf[f];
                th.emplace_back([pb, fsize, want] { pb->need(std::min(fsize + 64, want / 2)); });
            }
    for (auto& b : R.batches) {
        Batch* bb = &b;
        th.emplace_back([bb, &R, want, L_est] {
            const Options& o = R.o;
            bb->text1.need(want); if (o.pe) bb->text2.need(want);
            bb->sam.need(R.sam_bound(want * (size_t)o.nf(), (size_t)o.batch * (size_t)o.nf(), L_est));
        });
    }
    for (auto& t : th) t.join();
}

// the index file, then -- while R.prealloc pins the buffers -- one owner context per listed device (attached in parallel: each uploads
// and re-packs its own index copy), plus contexts-1 further contexts per device on the owner's index (bmbs_index_share)
int load_index_and_contexts(Run& R)
{
    const Options& o = R.o;
    std::string& index = R.index = o.index;
    if (is_dir(index)) index += "/genome";           // Index.cpp:1048-1069
    R.ixf = bmbs_index_file_load(index.c_str());
    if (!R.ixf) { fprintf(stderr, "Cannot open index %s.index*\n", index.c_str()); return 1; }
    bmbs_index_file_view(R.ixf, &R.view);
    for (int i = 0; i < R.view.n_chrom; i++) { R.chrom_names.push_back(bmbs_index_file_chrom_name(R.ixf, i)); R.max_chrom = std::max(R.max_chrom, R.chrom_names.back().size()); }
    if (o.bai)
        for (int i = 0; i < R.view.n_chrom; i++)
            if (R.view.chrom_len[i] > (1ull << 29)) {
                fprintf(stderr, "bmbs_search: --bai: sequence %s is longer than 2^29 bases: a BAI index cannot hold it (CSI is not written)\n", R.chrom_names[(size_t)i].c_str());
                return 2;
            }
    R.prealloc = std::thread(prealloc_buffers, std::ref(R));
    for (int d : o.devices) {
        bmbs_ctx* c = bmbs_create(d, &o.P);
        if (!c) { fprintf(stderr, "bmbs_search: no usable HIP device %d (this driver has no CPU mapping path)\n", d); return 1; }
        R.ctxs.push_back(c);
    }
    {
        std::vector<int> rcs(R.ctxs.size(), 0);
        std::vector<std::thread> th;
        for (size_t i = 0; i < R.ctxs.size(); i++) th.emplace_back([&rcs, &R, i] { rcs[i] = bmbs_index_attach(R.ctxs[i], &R.view); });
        for (auto& t : th) t.join();
        for (size_t i = 0; i < R.ctxs.size(); i++) if (rcs[i]) { fprintf(stderr, "%s\n", bmbs_last_error(R.ctxs[i])); return 1; }
    }
    R.n_owner = R.ctxs.size();
    for (size_t i = 0; i < R.n_owner; i++)
        for (int s = 1; s < o.contexts; s++) {
            bmbs_ctx* c = bmbs_create(o.devices[i], &o.P);
            if (!c || bmbs_index_share(c, R.ctxs[i])) { fprintf(stderr, "bmbs_search: cannot create a shared context on device %d\n", o.devices[i]); return 1; }
            R.ctxs.push_back(c);
        }
    {
        std::vector<const char*> nm;
        for (const auto& s : R.chrom_names) nm.push_back(s.c_str());
        for (bmbs_ctx* c : R.ctxs) if (bmbs_sam_refs(c, nm.data(), (int32_t)nm.size())) { fprintf(stderr, "%s\n", bmbs_last_error(c)); return 1; }
    }
    if (o.trim)
        for (bmbs_ctx* c : R.ctxs) if (bmbs_set_trim(c, &o.tpar)) { fprintf(stderr, "bmbs_search: %s\n", bmbs_last_error(c)); return 2; }
    // device memory for the work buffers of a batch, taken while the index loads instead of inside the first calls
    for (bmbs_ctx* c : R.ctxs) (void)bmbs_reserve(c, (uint64_t)o.batch * (uint64_t)o.nf() * (1200 + 3 * (uint64_t)std::max<size_t>(R.est0 / 2, 100)));
    return 0;
}

// the parts: record ranges of the input, one output file each
int open_inputs(Run& R)
{
    const Options& o = R.o;
    R.parts.resize((size_t)o.parts);
    for (int p = 0; p < o.parts; p++) { R.parts[(size_t)p].reset(new Part()); R.parts[(size_t)p]->id = p; }
    std::vector<size_t> cut1, cut2;
    if (!compute_cuts(o, cut1, cut2)) { fprintf(stderr, "Cannot open the read file(s)\n"); return 1; }
    for (int p = 0; p < o.live_parts; p++) {
        Part& pt = *R.parts[(size_t)p];
        const int zt = std::max(1, o.io_threads / o.nf());           // compressed input: inflate threads per file
        if (!pt.s1.open(o.in1.c_str(), cut1[(size_t)p], cut1[(size_t)p + 1], zt, o.devices[(size_t)p % o.devices.size()]) ||
            (o.pe && !pt.s2.open(o.seq2.c_str(), cut2[(size_t)p], cut2[(size_t)p + 1], zt, o.devices[(size_t)p % o.devices.size()]))) {
            fprintf(stderr, "Cannot open the read file(s)\n"); return 1;
        }
    }
    return 0;
}

// OutPutSAM_Nounheader (Process_sam_out.cpp:1137-1153)
std::string sam_header_text(bool sorted, const std::vector<std::string>& chrom_names, const uint64_t* chrom_len, const std::vector<std::string>& args)
{
    std::string h = sorted ? "@HD\tVN:1.4\tSO:coordinate\n" : "@HD\tVN:1.4\tSO:unsorted\n";
    for (size_t i = 0; i < chrom_names.size(); i++) { h += "@SQ\tSN:" + chrom_names[i] + "\tLN:"; put_uint(h, chrom_len[i]); h += '\n'; }
    h += "@PG\tID:BitMapperBS\tVN:1.0.2.3\tCL:";
    // (--methyl and its options shape no byte of this file, so they stay out of its header: the BAM and its .bai are the same
    // bytes with and without them)
    for (size_t i = 0; i < args.size(); i++) {
        const std::string& a = args[i];
        if (a == "--methyl" || a == "--methyl-min-mapq" || a == "--methyl-min-phred") { i++; continue; }
        if (a == "--methyl-ignore" || a == "--methyl-ignore-r2" || a == "--methyl-ignore-3prime" || a == "--methyl-ignore-3prime-r2") { i++; continue; }
        if (a == "--methyl-min-opposite-depth" || a == "--methyl-max-variant-frac" || a == "--methyl-min-depth") { i++; continue; }
        if (a == "--methyl-report-window" || a == "--conversion-report") { i++; continue; }      // (the filter's own options set flags in this file: they stay)
        // (--trim and its options: a run on trimmed files names none of them, and its output is this run's)
        if (a == "--trim") continue;
        if (a.compare(0, 7, "--trim-") == 0) { i++; continue; }
        if (a == "--CpG" || a == "--CHG" || a == "--CHH" || a == "--mbias" || a == "--methyl-merge-context" || a == "--cytosine-report") continue;
        h += a; h += ' ';
    }
    h += '\n';
    return h;
}
// BAM header: magic, the same text, the reference dictionary; one BGZF block series
std::string bam_header_block(const std::string& text, const std::vector<std::string>& chrom_names, const uint64_t* chrom_len)
{
    std::vector<char> hb = {'B', 'A', 'M', 1}, z;
    put_le32(hb, (uint32_t)text.size()); hb.insert(hb.end(), text.begin(), text.end());
    put_le32(hb, (uint32_t)chrom_names.size());
    for (size_t i = 0; i < chrom_names.size(); i++) {
        const std::string& nm = chrom_names[i];
        put_le32(hb, (uint32_t)nm.size() + 1); hb.insert(hb.end(), nm.begin(), nm.end()); hb.push_back(0);
        put_le32(hb, (uint32_t)chrom_len[i]);
    }
    bgzf_append(hb.data(), hb.size(), z);
    return std::string(z.begin(), z.end());
}

// every part's file; the header goes into the first
int open_outputs(Run& R)
{
    const Options& o = R.o;
    for (int p = 0; p < o.parts; p++) {
        Part& pt = *R.parts[(size_t)p];
        std::string path = o.out;
        if (o.parts > 1) { char suf[32]; snprintf(suf, sizeof suf, ".part%03d", p); path += suf; }
        pt.ofd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (pt.ofd < 0) { fprintf(stderr, "Cannot open %s\n", path.c_str()); return 1; }
        {
            struct stat osb; pt.regular = fstat(pt.ofd, &osb) == 0 && S_ISREG(osb.st_mode);
            // blocks are reserved ahead only where that is a table entry (extent file systems): tmpfs answers fallocate by taking and
            // clearing the pages (4 GiB ahead of eight parts: slower than the writes, then ENOSPC), overlayfs refuses it
            struct statfs fsb;
            pt.can_alloc = pt.regular && fstatfs(pt.ofd, &fsb) == 0 &&
                           ((unsigned long)fsb.f_type == 0xEF53ul || (unsigned long)fsb.f_type == 0x58465342ul || (unsigned long)fsb.f_type == 0x9123683Eul);
        }
        if (p == 0) {
            std::string h = sam_header_text(o.sort, R.chrom_names, R.view.chrom_len, o.args);
            if (o.bam) h = bam_header_block(h, R.chrom_names, R.view.chrom_len);
            if (pwrite(pt.ofd, h.data(), h.size(), 0) != (ssize_t)h.size()) { fprintf(stderr, "write error on %s\n", path.c_str()); return 1; }
            pt.out_off = h.size();
        }
    }
    return 0;
}

// the device touches every staging buffer once now (BMBS_NO_PREFAULT=1 skips it)
void prefault_buffers(Run& R)
{
    if (getenv("BMBS_NO_PREFAULT")) return;
    std::vector<std::thread> th;
    for (size_t i = 0; i < R.batches.size(); i++) {
        Batch* b = &R.batches[i];
        bmbs_ctx* c = R.ctxs[i % R.ctxs.size()];
        th.emplace_back([b, c] {
            if (b->text1.p) (void)bmbs_host_prefault(c, b->text1.p, b->text1.cap, 1);
            if (b->text2.p) (void)bmbs_host_prefault(c, b->text2.p, b->text2.cap, 1);
            if (b->sam.p) (void)bmbs_host_prefault(c, b->sam.p, b->sam.cap, 2);
        });
    }
    for (auto& t : th) t.join();
}

// --sort: the store of pass 1.  Bins: BMBS_SORT_BINS, by default 4096 of equal genomic length (0.76 Mbp of a human genome each) + one
// for records without a reference; its cap: --sort-mem, by default half of the machine's memory
void init_sort_store(Run& R)
{
    const char* e = getenv("BMBS_SORT_BINS");
    R.sort_store.init(R.view, e ? atol(e) : 4096);
    const double phys = (double)sysconf(_SC_PHYS_PAGES) * (double)sysconf(_SC_PAGE_SIZE);
    R.sort_store.cap = (size_t)(R.o.sort_mem_gib > 0 ? R.o.sort_mem_gib * 1073741824.0 : phys / 2);
}

// ================ stage R (one per part): text window + newline count -> how many whole records ===================================
// a free batch for the part's next window, and -- device-inflated input -- a context without an open window; t0: when the reader had them
Batch* begin_batch(Run& R, Part* pt, bmbs_ctx** ctx, double& t0)
{
    const double tw0 = now();
    Batch* b = R.free_q.get();
    if (ctx) *ctx = R.ctx_pool.get();
    t0 = now();
    pt->t_wait_r += t0 - tw0;
    b->part = pt; b->seq = pt->next_seq++; b->n = 0; b->end = false; b->used1 = b->used2 = 0; b->sam_bytes = 0; b->open_ctx = nullptr;
    return b;
}
// the batch goes down the pipeline empty, as the part's last
void hand_on_empty(Run& R, Batch* b, bmbs_ctx* ctx)
{
    b->end = true; b->n = 0;
    if (ctx) R.ctx_pool.put(ctx);
    R.gpu_q.put(b);
}
// the reader gives up
void bail(Run& R, Batch* b, bmbs_ctx* ctx, const std::string& why) { R.fail(why); hand_on_empty(R, b, ctx); }

// BGZF input that stays on the device (bmbs_text_open_bgzf / bmbs_text_map_open): the reader hands the compressed blocks of a window
// to a context, learns how many whole records they held and what is left over (the next window's prefix), and passes the context on
// to a worker for the mapping.  The inflated text never crosses the link -- the host moves compressed bytes and tails only.
struct BgzfReader {
    Run& R; Part* pt;
    Pool* pool[2];                               // the memcpy threads of file 1 and file 2
    Source* S[2];
    int nf;
    Pinned tails[2];
    std::thread ahead;                           // stages R.zst[cur ^ 1] while the device opens R.zst[cur]

    // the compressed blocks of the next window of every file, copied into g's page-locked buffers
    void stage(Staged& g, size_t room0, size_t room1)
    {
        g.foreign_any = false; g.ok = true;
        const size_t room[2] = {room0, room1};
        for (int f = 0; f < nf && g.ok; f++) {
            Source& s = *S[f];
            bool foreign = false;
            if (!s.next_blocks(room[f], g.a[f], g.q[f], foreign)) { g.ok = false; g.err = s.err; break; }
            if (foreign && g.q[f] == g.a[f]) { g.foreign_any = true; continue; }
            g.blk[f] = s.zblk; g.out[f] = s.zout;
            const size_t zbytes = g.q[f] - g.a[f];
            if (zbytes) {
                if (!g.buf[f].need(zbytes + 64)) { g.ok = false; g.err = "cannot allocate page-locked staging memory"; break; }
                Pool& pl = *pool[f];
                const int T = pl.size() * 2;
                const size_t per = ((zbytes + (size_t)T - 1) / (size_t)T + 4095) & ~(size_t)4095;
                char* dst = g.buf[f].p; const unsigned char* src = s.zmap + g.a[f];
                pl.run(T, [dst, src, zbytes, per](int t) { const size_t x = std::min(zbytes, per * (size_t)t), y = std::min(zbytes, x + per); if (x < y) memcpy(dst + x, src + x, y - x); });
            }
            s.znext = g.q[f];
            g.last[f] = g.q[f] >= s.zsize && s.loops_left == 0;
            if (g.q[f] >= s.zsize && s.loops_left > 0) { s.znext = 0; s.loops_left--; }      // --loop-input: the file once more
        }
    }
    // text bytes the next window of file f may hold behind what the last one left over
    size_t room_for(size_t est_now, int f) const
    {
        const size_t target = R.window_bytes(est_now, Run::bgzf_window_cap);
        return target > S[f]->carry.size() ? target - S[f]->carry.size() : (size_t)0;
    }
    void join_ahead() { if (ahead.joinable()) ahead.join(); }
    void bail(Batch* b, bmbs_ctx* ctx, const std::string& why) { join_ahead(); ::bail(R, b, ctx, why); }

    // true: the input is finished (or failed); false: go on with the host-window reader (a member that is not a BGZF block turned up)
    bool run()
    {
        const Options& o = R.o;
        const bool pe = o.pe;
        size_t est = R.est0;
        tails[0].kind = 2; tails[1].kind = 2;
        // (what a window leaves over is a partial record, plus -- when the mates' records differ in size -- the surplus of one file, which the
        // next window's smaller block count evens out: never more than a window)
        // in practice a fraction of a record; the buffers grow when a call says so (page-locked memory is slow to get: ~0.1 ms per MB)
        size_t tail_cap = (size_t)4 << 20;
        if (const char* tv = getenv("BMBS_Z_TAIL")) { const long v = atol(tv); if (v >= 1) tail_cap = (size_t)v; }      // tests: the growth path
        if (!tails[0].need(tail_cap) || (pe && !tails[1].need(tail_cap))) { R.fail("cannot allocate page-locked staging memory"); return true; }
        Staged* st = R.zst;
        int cur = 0;
        stage(st[0], room_for(est, 0), pe ? room_for(est, 1) : 0);
        Joiner joiner{ahead};
        for (;;) {
            bmbs_ctx* ctx = nullptr; double t0;
            Batch* b = begin_batch(R, pt, &ctx, t0);
            if (R.failed) { join_ahead(); hand_on_empty(R, b, ctx); return true; }
            join_ahead();
            Staged& g = st[cur];
            if (!g.ok) { bail(b, ctx, g.err); return true; }
            const size_t target = R.window_bytes(est, Run::bgzf_window_cap);
            bmbs_ztext z[2]; memset(z, 0, sizeof z);
            if (g.foreign_any) {
                // the rest of such a file goes through the host's stream inflater; blocks already taken for this window are given back
                for (int f = 0; f < nf; f++) {
                    Source& s = *S[f];
                    s.znext = g.a[f];
                    if (s.znext < s.zsize && !s.bgzf_block(s.zmap + s.znext, s.zsize - s.znext)) { std::lock_guard<std::mutex> l(s.m); s.zdirect = false; const size_t at = s.znext; s.znext = s.zsize; s.start_pgz(at, 0); }
                }
                pt->next_seq--;                                     // (the batch was not used)
                R.free_q.put(b);
                // every window opened so far has to be mapped before the workers go back to contexts of their own
                for (size_t i = 1; i < R.ctxs.size(); i++) (void)R.ctx_pool.get();
                return false;
            }
            size_t text_bytes = 0;
            for (int f = 0; f < nf; f++) {
                Source& s = *S[f];
                z[f].prefix = s.carry.empty() ? nullptr : s.carry.data(); z[f].prefix_bytes = s.carry.size();
                z[f].comp = g.buf[f].p; z[f].comp_bytes = g.q[f] - g.a[f]; z[f].blk_off = g.blk[f].data(); z[f].out_off = g.out[f].data(); z[f].n_blocks = (int64_t)g.blk[f].size() - 1;
                text_bytes += s.carry.size() + (size_t)g.out[f].back();
            }
            const bool last1 = g.last[0], last2 = pe && g.last[1];
            // the window behind this one is staged while the device works on this one (what this window will leave over is not known
            // yet: the last window's leftover stands in for it when the room is measured)
            {
                const size_t r0 = room_for(est, 0), r1 = pe ? room_for(est, 1) : 0;
                Staged* nx = &st[cur ^ 1];
                ahead = std::thread([this, nx, r0, r1] { stage(*nx, r0, r1); });
                cur ^= 1;
            }
            int64_t nrec = 0; uint64_t tb[2] = {0, 0};
            // every whole record of the window is taken (the window is what bounds a batch here: --batch records by the running estimate of a record's size)
            int rc = 0;
            for (int attempt = 0; attempt < 2; attempt++) {
                rc = bmbs_text_open_bgzf(ctx, &z[0], pe ? &z[1] : nullptr, 4 * (int64_t)o.batch, last1 ? 1 : 0, last2 ? 1 : 0, &nrec, tails[0].p, tail_cap, &tb[0],
                                         pe ? tails[1].p : nullptr, &tb[1]);
                if (rc != BMBS_ENOMEM || attempt || std::max(tb[0], tb[1]) <= tail_cap) break;
                // more text behind the window's records than the tail buffers hold (the mates' records differ in size): once more with room
                tail_cap = (size_t)std::max(tb[0], tb[1]) + ((size_t)4 << 20);
                if (!tails[0].need(tail_cap) || (pe && !tails[1].need(tail_cap))) { bail(b, ctx, "cannot allocate page-locked staging memory"); return true; }
            }
            if (rc) { bail(b, ctx, bmbs_last_error(ctx)); return true; }
            for (int f = 0; f < nf; f++) S[f]->carry.assign(tails[f].p, tails[f].p + tb[f]);
            // the part's input ends with this batch when a file has nothing left behind it (PE: the shorter file decides)
            b->end = (last1 && tb[0] == 0) || (pe && last2 && tb[1] == 0);
            if (nrec == 0) {
                if (!b->end && (last1 || (pe && last2))) b->end = true;            // a trailing fragment that is not a whole record
                if (!b->end) { bail(b, ctx, "FASTQ record larger than the " + std::to_string(target) + "-byte window"); return true; }
                R.ctx_pool.put(ctx); R.gpu_q.put(b);
                return true;
            }
            est = std::max<size_t>(64, text_bytes / (size_t)nf / (size_t)nrec + 16);
            b->n = nrec; b->open_ctx = ctx;
            const int Lg = (int)std::min<size_t>(1000, est / 2);
            if (!b->sam.need(R.sam_bound(text_bytes, (size_t)nrec * (size_t)nf, Lg))) { bail(b, ctx, "cannot allocate page-locked staging memory"); return true; }
            pt->t_read += now() - t0;
            pt->records += nrec;
            const bool end = b->end;
            R.gpu_q.put(b);
            if (end) return true;
        }
    }
};
bool reader_device_bgzf(Run& R, Part* pt, Pool& pool, Pool& pool2)
{
    BgzfReader z{R, pt, {&pool, &pool2}, {&pt->s1, &pt->s2}, R.o.nf(), {}, {}};
    return z.run();
}

// windows of text in host memory: plain files, and compressed input that the host inflates
void reader_host(Run& R, Part* pt)
{
    const Options& o = R.o;
    const bool pe = o.pe;
    Pool pool(R.r_threads - 1);
    Pool pool2(pe && pt->s2.gz ? std::max(1, R.r_threads / 2) - 1 : 0);          // second mate's window of compressed input
    if (o.live_parts == 1 && R.z_mode(*pt) && reader_device_bgzf(R, pt, pool, pool2)) return;
    size_t est = R.est0;
    for (;;) {
        double t0;
        Batch* b = begin_batch(R, pt, nullptr, t0);
        if (R.failed) { hand_on_empty(R, b, nullptr); return; }
        // (.gz: what the previous window left over is copied in first and must fit whatever the new estimate says)
        const size_t want = std::max(R.window_bytes(est, Run::host_window_cap), std::max(pt->s1.carry.size(), pt->s2.carry.size()) + (1u << 16));
        if (!b->text1.need(want + 64) || (pe && !b->text2.need(want + 64))) { bail(R, b, nullptr, "cannot allocate page-locked staging memory"); return; }
        bool last1 = true, last2 = true;
        size_t n1 = 0, n2 = 0;
        if (pe && pt->s2.gz) {
            // compressed input: the two windows are assembled side by side (each waits for its own inflaters)
            bool ok2 = true;
            std::thread w2([pt, b, want, &pool2, &ok2, &n2, &last2] { ok2 = pt->s2.window(pool2, b->text2.p, want, n2, last2, b->counts2); });
            const bool ok1 = pt->s1.window(pool, b->text1.p, want, n1, last1, b->counts1);
            w2.join();
            if (!ok1) { bail(R, b, nullptr, pt->s1.err); return; }
            if (!ok2) { bail(R, b, nullptr, pt->s2.err); return; }
        } else {
            if (!pt->s1.window(pool, b->text1.p, want, n1, last1, b->counts1)) { bail(R, b, nullptr, pt->s1.err); return; }
            if (pe && !pt->s2.window(pool, b->text2.p, want, n2, last2, b->counts2)) { bail(R, b, nullptr, pt->s2.err); return; }
        }
        size_t l1 = 0, l2 = 0;
        for (uint32_t c : b->counts1) l1 += c;
        for (uint32_t c : b->counts2) l2 += c;
        const long avail1 = (long)(l1 / 4), avail2 = pe ? (long)(l2 / 4) : 0;
        long nrec = pe ? std::min(avail1, avail2) : avail1;
        if (nrec > o.batch) nrec = o.batch;
        // the part's input ends with this batch when a file has no complete record left after it (PE: the shorter file decides)
        b->end = (last1 && avail1 == nrec) || (pe && last2 && avail2 == nrec);
        if (nrec == 0) {
            if (!b->end) { bail(R, b, nullptr, "FASTQ record larger than the " + std::to_string(want) + "-byte window"); return; }
            R.gpu_q.put(b);
            return;
        }
        b->used1 = after_kth_nl_blocks(b->text1.p, n1, b->counts1, (size_t)nrec * 4);
        pt->s1.consumed(b->text1.p, n1, b->used1);
        if (pe) { b->used2 = after_kth_nl_blocks(b->text2.p, n2, b->counts2, (size_t)nrec * 4); pt->s2.consumed(b->text2.p, n2, b->used2); }
        est = std::max<size_t>(64, std::max(b->used1, b->used2) / (size_t)nrec + 16);
        b->n = nrec;
        const int Lg = (int)std::min<size_t>(1000, est / 2);
        if (!b->sam.need(R.sam_bound(b->used1 + b->used2, (size_t)nrec * (size_t)o.nf(), Lg))) { bail(R, b, nullptr, "cannot allocate page-locked staging memory"); return; }
        pt->t_read += now() - t0;
        pt->records += nrec;
        const bool end = b->end;
        R.gpu_q.put(b);
        if (end) return;
    }
}

// ================ stage W (one per part): the SAM text (or its BAM form) goes into the part's file, in order =======================
void writer(Run& R, Part* pt)
{
    const Options& o = R.o;
    SortStore& store = R.sort_store;
    Pool wpool(std::max(1, std::min(8, o.io_threads / (2 * o.live_parts))) - 1);       // slices of a batch written side by side
    for (;;) {
        const double tw0 = now();
        Batch* b = pt->out_q.get();
        const double t0 = now();
        pt->t_wait_w += t0 - tw0;
        const bool end = b->end;
        if (o.sort) {
            bool room = true;
            if (b->n && !R.failed && o.markdup) room = store.add_sigs(wpool, b->sig.data(), (size_t)b->n_sig, R.tmpl_base);
            if (b->n && !R.failed && b->sam_bytes && room)
                room = store.add(wpool, b->sam.p, (size_t)b->sam_bytes, b->skey.data(), b->slen.data(), (size_t)b->n_sorted, o.markdup ? b->tmpl.data() : nullptr, R.tmpl_base,
                                 o.methyl_clip ? b->clip.data() : nullptr);
            if (b->n && o.markdup) R.tmpl_base += (uint64_t)b->n_sig;
            if (!room) {
                char msg[256];
                snprintf(msg, sizeof msg, "--sort-mem: the record store of --sort is used up (%.3f GiB allowed): %ld records fit, the run has more (spilling to disk is not implemented)",
                         (double)store.cap / 1073741824.0, store.records);
                R.fail(msg);
            }
        } else if (b->n && !R.failed && b->sam_bytes) {
            const char* text = b->sam.p;
            const size_t len = (size_t)b->sam_bytes;
            // One buffered pwrite per batch extends the file under its inode lock at the speed of one memcpy (10 GB/s = 28 M SAM
            // records/s on the MI355X boxes).  With the blocks reserved ahead (fallocate in 4 GiB steps, cut back to the true size
            // at the end) several slices of a batch go into the page cache side by side: 17 GB/s (profiles/r02_write_probe.txt)
            if (pt->can_alloc && pt->out_off + len > pt->alloc_end) {
                const size_t step = std::max<size_t>((size_t)4 << 30, 2 * len);
                if (fallocate(pt->ofd, 0, (off_t)pt->alloc_end, (off_t)(pt->out_off + len + step - pt->alloc_end)) == 0) pt->alloc_end = pt->out_off + len + step;
                else { pt->can_alloc = false; if (o.verbose && pt->alloc_end == 0) fprintf(stderr, "[bmbs_search] part %d: fallocate not available on the output (%s): one writer per batch\n", pt->id, strerror(errno)); }      // not a regular file (/dev/null, a pipe), or a file system without it
            }
            // (no fallocate -- overlayfs says ENODEV: four slices still extend a regular file a little faster than one, 12.8 against 10 GB/s)
            const int T = pt->can_alloc ? wpool.size() : (pt->regular ? std::min(4, wpool.size()) : 1);
            const size_t per = ((len + (size_t)T - 1) / (size_t)T + 4095) & ~(size_t)4095;
            const int ofd = pt->ofd; const size_t off = pt->out_off;
            wpool.run(T, [&R, ofd, off, text, len, per](int t) {
                const size_t a = std::min(len, per * (size_t)t), e = std::min(len, a + per);
                if (!pwrite_all(ofd, text + a, e - a, off + a)) R.fail(std::string("write error: ") + strerror(errno));
            });
            pt->out_off += len;
        }
        pt->t_write += now() - t0;
        R.free_q.put(b);
        if (end) return;
    }
}

// ================ stage G: one worker per context, one library call per batch =====================================================
void gpu_worker(Run& R, bmbs_ctx* own_ctx)
{
    const Options& o = R.o;
    for (;;) {
        bmbs_ctx* ctx = own_ctx;
        const double tw0 = now();
        Batch* b = R.gpu_q.get();
        if (!b) return;
        const double t0 = now();
        bmbs_ctx* octx = b->open_ctx;                                        // compressed input on the device: the batch's window is open on this context
        b->open_ctx = nullptr;
        if (octx) ctx = octx;
        if (!R.failed && b->n) {
            for (int attempt = 0; attempt < 2; attempt++) {
                uint64_t bytes = 0; int64_t lines = 0;
                const int rc = octx ? bmbs_text_map_open(ctx, o.flags, b->sam.p, b->sam.cap, &bytes, &lines)
                             : o.pe ? bmbs_map_pe_text(ctx, b->text1.p, b->used1, b->text2.p, b->used2, b->n, o.flags, b->sam.p, b->sam.cap, &bytes, &lines)
                                    : bmbs_map_se_text(ctx, b->text1.p, b->used1, b->n, o.flags, b->sam.p, b->sam.cap, &bytes, &lines);
                if (rc == BMBS_ENOMEM && bytes > b->sam.cap && attempt == 0 && b->sam.need((size_t)bytes + 64)) continue;   // reads longer than guessed
                if (rc) R.fail(bmbs_last_error(ctx));
                b->sam_bytes = rc ? 0 : bytes;
                if (o.trim && !rc) {
                    // the batch is what trimming left of it, before anything else looks at it
                    bmbs_trim_counts tc; int64_t kept = 0;
                    if (bmbs_text_trim_counts(ctx, &tc, &kept)) { R.fail(bmbs_last_error(ctx)); b->sam_bytes = 0; break; }
                    {
                        std::lock_guard<std::mutex> l(R.g_mu);
                        static_assert(sizeof(bmbs_trim_counts) == 19 * sizeof(int64_t), "bmbs_trim_counts is int64_t words and nothing else: they are added up as such");
                        int64_t* const sum = reinterpret_cast<int64_t*>(&R.trim_cnt); const int64_t* const add = reinterpret_cast<const int64_t*>(&tc);
                        for (size_t x = 0; x < sizeof tc / sizeof(int64_t); x++) sum[x] += add[x];
                        R.trim_in += b->n; R.trim_kept += (long)kept;
                    }
                    b->n = (long)kept;
                    if (!kept) { b->sam_bytes = 0; b->n_sorted = 0; b->n_sig = 0; break; }
                }
                if (o.sort && !rc) {
                    b->skey.resize((size_t)lines + 1); b->slen.resize((size_t)lines + 1);
                    if (bmbs_text_sorted_index(ctx, b->skey.data(), b->slen.data(), lines, &b->n_sorted)) { R.fail(bmbs_last_error(ctx)); b->sam_bytes = 0; }
                    b->n_sig = 0;
                    if (o.markdup && !R.failed) {
                        int64_t nt = 0;
                        b->sig.resize((size_t)b->n + 1); b->tmpl.resize((size_t)lines + 1);
                        if (bmbs_text_sorted_dup(ctx, b->sig.data(), b->n, &b->n_sig, b->tmpl.data(), lines, &nt)) { R.fail(bmbs_last_error(ctx)); b->sam_bytes = 0; }
                        else if (nt != b->n_sorted || b->n_sig != b->n) { R.fail("--markdup: the batch's templates do not match its records"); b->sam_bytes = 0; }
                    }
                    if (o.methyl_clip && !R.failed) {
                        int64_t nc = 0;
                        b->clip.resize((size_t)lines + 1);
                        if (bmbs_text_sorted_clip(ctx, b->clip.data(), lines, &nc)) { R.fail(bmbs_last_error(ctx)); b->sam_bytes = 0; }
                        else if (nc != b->n_sorted) { R.fail("--methyl: the batch's clips do not match its records"); b->sam_bytes = 0; }
                    }
                    if (o.nonconv && !R.failed) {
                        // the verdicts of the batch's templates, per record; the records of a failed one get flag 0x200 (byte 19 |= 0x02) here,
                        // in the batch's own buffer: the store, pass 2 and every later stage see flagged records
                        int64_t nv = 0, nf = 0;
                        uint64_t tot[12];
                        b->ncfail.resize((size_t)lines + 1);
                        if (bmbs_text_sorted_nonconv(ctx, &o.ncpar, b->ncfail.data(), lines, &nv, &nf, tot)) { R.fail(bmbs_last_error(ctx)); b->sam_bytes = 0; }
                        else if (nv != b->n_sorted) { R.fail("--filter-non-conversion: the batch's verdicts do not match its records"); b->sam_bytes = 0; }
                        else {
                            if (nf) { size_t at = 0; for (int64_t j = 0; j < nv; at += b->slen[(size_t)j], j++) if (b->ncfail[(size_t)j]) b->sam.p[at + 19] |= 0x02; }
                            std::lock_guard<std::mutex> l(R.g_mu);
                            for (int x = 0; x < 12; x++) R.nc_totals[x] += tot[x];
                            R.nc_templates += b->n; R.nc_failed += (long)nf;
                        }
                    }
                }
                break;
            }
        }
        { std::lock_guard<std::mutex> l(R.g_mu); R.t_wait_g += t0 - tw0; R.t_gpu += now() - t0; }
        if (octx) R.ctx_pool.put(octx);
        b->part->out_q.put(b->seq, b);
    }
}

// the mapping: every part a pipeline of its own (reader -> shared gpu workers -> writer)
void map_all(Run& R)
{
    const Options& o = R.o;
    for (auto& b : R.batches) R.free_q.put(&b);
    // the writers only pwrite (SAM text or finished BGZF blocks), every I/O thread reads
    R.r_threads = o.reader_threads > 0 ? o.reader_threads : std::max(1, o.io_threads / o.live_parts);
    if (o.live_parts == 1 && R.z_mode(*R.parts[0])) for (bmbs_ctx* c : R.ctxs) R.ctx_pool.put(c);
    std::vector<std::thread> workers;
    for (bmbs_ctx* c : R.ctxs) workers.emplace_back(gpu_worker, std::ref(R), c);
    for (int p = 0; p < o.live_parts; p++) { Part* pt = R.parts[(size_t)p].get(); pt->writer = std::thread(writer, std::ref(R), pt); pt->reader = std::thread(reader_host, std::ref(R), pt); }
    for (int p = 0; p < o.live_parts; p++) R.parts[(size_t)p]->reader.join();
    for (int p = 0; p < o.live_parts; p++) R.parts[(size_t)p]->writer.join();           // every batch has passed its writer: the workers are idle
    for (size_t i = 0; i < workers.size(); i++) R.gpu_q.put(nullptr);
    for (auto& t : workers) t.join();
}

// ================ --sort: between the passes, and pass 2 ================================================================================
// --markdup, between the passes: bmbs_dup_select over groups of consecutive signature bins of at most the call budget (a template's
// group lies in one bin, in input order: bins are filled in Batch.seq order), a bit per losing template
void dup_select_pass(Run& R, Pass2& S, size_t budget)
{
    S.dup_bits.assign(((size_t)R.sort_store.templates + 63) / 64 + 1, 0);
    const size_t lim = std::max<size_t>(1, budget / sizeof(bmbs_dup_sig));
    std::vector<bmbs_dup_sig> gs; std::vector<uint64_t> gg; std::vector<uint8_t> gd;
    auto run = [&] {
        if (gs.empty() || R.failed) { gs.clear(); gg.clear(); return; }
        gd.assign(gs.size(), 0);
        int64_t nd = 0;
        if (bmbs_dup_select(R.ctxs[0], gs.data(), (int64_t)gs.size(), gd.data(), &nd)) R.fail(bmbs_last_error(R.ctxs[0]));
        else for (size_t i = 0; i < gs.size(); i++) if (gd[i]) S.dup_bits[gg[i] >> 6] |= (uint64_t)1 << (gg[i] & 63);
        if (!R.failed) S.n_dup += (size_t)nd;
        S.select_calls++; gs.clear(); gg.clear();
    };
    for (SigBin& sb : R.sort_store.sbin) {
        if (sb.sig.empty()) continue;
        if (!gs.empty() && gs.size() + sb.sig.size() > lim) run();
        gs.insert(gs.end(), sb.sig.begin(), sb.sig.end()); gg.insert(gg.end(), sb.gid.begin(), sb.gid.end());
        std::vector<bmbs_dup_sig>().swap(sb.sig); std::vector<uint64_t>().swap(sb.gid);
    }
    run();
}

// the units' records into the slots' page-locked buffers, in unit order
void pass2_stager(Run& R, Pass2& S)
{
    const Options& o = R.o;
    Pool spool(std::max(1, std::min(16, o.io_threads)) - 1);
    for (size_t i = 0; i < S.units.size(); i++) {
        Slot* sl = S.free_s.get();
        sl->unit = i;
        if (!R.failed) sort_stage(R.sort_store, S.units[i], spool, sl->in.p, sl->len.data(), o.markdup ? S.dup_bits.data() : nullptr, o.methyl_clip ? sl->clip.data() : nullptr);
        S.staged_s.put(sl);
    }
    for (int i = 0; i < S.n_slots; i++) S.staged_s.put(nullptr);
}
// one bmbs_bam_sort call per staged slot, and what --bai and --methyl take from the device behind it
void pass2_sorter(Run& R, Pass2& S, bmbs_ctx* ctx)
{
    const Options& o = R.o;
    for (;;) {
        Slot* sl = S.staged_s.get();
        if (!sl) return;
        const SortUnit& u = S.units[sl->unit];
        sl->out_bytes = 0;
        for (int attempt = 0; attempt < 2 && !R.failed; attempt++) {
            const int rc = bmbs_bam_sort(ctx, sl->in.p, u.bytes, sl->len.data(), (int64_t)u.n, 0, sl->out.p, sl->out.cap, &sl->out_bytes);
            if (rc == BMBS_ENOMEM && attempt == 0 && sl->out_bytes > sl->out.cap && sl->out.need((size_t)sl->out_bytes + 64)) continue;
            if (rc) { R.fail(bmbs_last_error(ctx)); sl->out_bytes = 0; }
            break;
        }
        if (o.bai && !R.failed && !sl->bai.fetch(ctx)) { R.fail(bmbs_last_error(ctx)); sl->out_bytes = 0; }
        // --methyl: the call's records are still on the device (the staged copies: duplicates carry 0x400)
        sl->n_site = sl->n_opp = 0;
        if (o.mbias) std::fill(sl->mbias.begin(), sl->mbias.end(), 0);      // (a call that fails leaves no table of the call before)
        if (o.methyl_out && !R.failed) {
            int64_t ns = 0;
            const uint32_t* const clip = o.pe ? sl->clip.data() : nullptr;
            if (o.methyl_use_opts ? bmbs_bam_sort_methyl_opts(ctx, clip, &o.mopt, &ns) : bmbs_bam_sort_methyl(ctx, clip, &o.mpar, &ns)) { R.fail(bmbs_last_error(ctx)); sl->out_bytes = 0; }
            else {
                if ((size_t)ns > sl->site.size()) sl->site.resize((size_t)ns + (size_t)ns / 8);
                if (bmbs_methyl_sites(ctx, sl->site.data(), (int64_t)sl->site.size(), &sl->n_site)) { R.fail(bmbs_last_error(ctx)); sl->out_bytes = 0; sl->n_site = 0; }
                int64_t nt = 0;
                if (o.mbias && !R.failed && bmbs_methyl_mbias(ctx, sl->mbias.data(), (int64_t)sl->mbias.size(), &nt)) { R.fail(bmbs_last_error(ctx)); sl->out_bytes = 0; }
            }
            // the variant filter: the same records once more, for what they show of the other strand's cytosines
            if (o.min_opp_depth > 0 && !R.failed) {
                int64_t no = 0;
                if (bmbs_bam_sort_methyl_opposite(ctx, clip, &o.oopt, &no)) { R.fail(bmbs_last_error(ctx)); sl->out_bytes = 0; }
                else {
                    if ((size_t)no > sl->opp.size()) sl->opp.resize((size_t)no + (size_t)no / 8);
                    if (bmbs_methyl_opposite(ctx, sl->opp.data(), (int64_t)sl->opp.size(), &sl->n_opp)) { R.fail(bmbs_last_error(ctx)); sl->out_bytes = 0; sl->n_opp = 0; }
                }
            }
        }
        S.done_s.put((long)sl->unit, sl);
    }
}

// pass 2: bins in key order -> bmbs_bam_sort -> BGZF blocks behind the header.
// Calls of at most BMBS_SORT_CALL_BYTES (default 1 GiB) of records; staged by the I/O threads into page-locked buffers, sorted and
// deflated on the device, appended by this thread in call order.  BMBS_SORT_SLOTS staging slots (default 2) on as many contexts:
// the staging and upload of one call run beside the kernels and the download of the other.
void sort_pass2(Run& R, Pass2& S)
{
    const Options& o = R.o;
    Part& pt = *R.parts[0];
    const char* e = getenv("BMBS_SORT_CALL_BYTES");
    const size_t budget = (size_t)std::max(1l, e ? atol(e) : 1l << 30);
    if (o.markdup) dup_select_pass(R, S, budget);
    if (o.mbias) S.mbias.assign((size_t)24 * BMBS_MBIAS_CYCLES, 0);
    S.t_select = now();
    sort_plan(R.sort_store, budget, S.units);
    S.sort_calls = S.units.size();
    size_t max_bytes = 0, max_n = 0;
    for (const SortUnit& u : S.units) { max_bytes = std::max(max_bytes, u.bytes); max_n = std::max(max_n, u.n); }
    e = getenv("BMBS_SORT_SLOTS");
    S.n_slots = (int)std::max<size_t>(1, std::min<size_t>({(size_t)(e ? atoi(e) : 2), R.ctxs.size(), S.units.size(), (size_t)4}));
    S.slots = std::vector<Slot>((size_t)S.n_slots);
    if (!S.units.empty()) {
        // (the mapping's page-locked windows are of no use here: a call is larger than a batch)
        for (auto& b : R.batches) { b.text1.release(); b.text2.release(); b.sam.release(); }
        std::vector<std::thread> th;
        std::atomic<bool> ok(true);
        for (Slot& sl : S.slots) {
            sl.in.kind = 1; sl.out.kind = 2; sl.len.resize(max_n + 1);
            if (o.methyl_clip) sl.clip.resize(max_n + 1);
            if (o.mbias) sl.mbias.assign((size_t)24 * BMBS_MBIAS_CYCLES, 0);
            Slot* s = &sl;
            th.emplace_back([s, &ok, max_bytes] { if (!s->in.need(max_bytes + 64)) ok = false; });
            th.emplace_back([s, &ok, max_bytes] { if (!s->out.need((max_bytes / 0xff00 + 1) * 65536 + 64)) ok = false; });
        }
        for (auto& t : th) t.join();
        if (!ok) R.fail("cannot allocate page-locked staging memory");
    }
    if (!R.failed && !S.units.empty()) {
        for (Slot& sl : S.slots) S.free_s.put(&sl);
        std::thread stager(pass2_stager, std::ref(R), std::ref(S));
        std::vector<std::thread> sorters;
        for (int w = 0; w < S.n_slots; w++) sorters.emplace_back(pass2_sorter, std::ref(R), std::ref(S), R.ctxs[(size_t)w]);
        for (size_t i = 0; i < S.units.size(); i++) {
            Slot* sl = S.done_s.get();
            if (!R.failed && !pwrite_all(pt.ofd, sl->out.p, (size_t)sl->out_bytes, pt.out_off)) R.fail(std::string("write error: ") + strerror(errno));
            if (o.bai && !R.failed && !S.bai.add(sl->bai, (uint64_t)pt.out_off)) R.fail("--bai: a record names a sequence the header does not have");
            if (o.methyl_out && !R.failed) methyl_merge(S.meth_sites, sl->site.data(), (size_t)sl->n_site);
            if (o.min_opp_depth > 0 && !R.failed) methyl_merge(S.meth_opp, sl->opp.data(), (size_t)sl->n_opp);
            if (o.mbias && !R.failed) for (size_t k = 0; k < S.mbias.size(); k++) S.mbias[k] += sl->mbias[k];
            pt.out_off += (size_t)sl->out_bytes;
            S.free_s.put(sl);
        }
        stager.join();
        for (auto& t : sorters) t.join();
    }
    for (Slot& sl : S.slots) { sl.in.release(); sl.out.release(); }
}

// ================ the end of the files ============================================================================================
// --bam: the BGZF end-of-file block behind the last part; every part cut back to its true size and closed
void finish_files(Run& R)
{
    const Options& o = R.o;
    if (o.bam && !R.failed) {
        static const unsigned char eof_block[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        Part& lastp = *R.parts[(size_t)o.parts - 1];
        if (pwrite(lastp.ofd, eof_block, 28, (off_t)lastp.out_off) != 28) R.failed = true;
        lastp.out_off += 28;
    }
    R.t_joined = now();
    for (int p = 0; p < o.parts; p++) {
        Part& pt = *R.parts[(size_t)p];
        if (pt.alloc_end > pt.out_off && ftruncate(pt.ofd, (off_t)pt.out_off) != 0) R.failed = true;
        ::close(pt.ofd);
        if (p < o.live_parts) { pt.s1.close(); if (o.pe) pt.s2.close(); }
    }
}

// --bai: the index, written once the file is complete
void write_bai(Run& R, Pass2& S)
{
    const Options& o = R.o;
    if (!R.parts[0]->regular) { fprintf(stderr, "bmbs_search: --bai needs a regular output file (-o %s is none)\n", o.out.c_str()); R.failed = true; return; }
    std::string ix;
    S.bai.serialize(ix);
    S.bai_bytes = ix.size();
    const int fd = ::open((o.out + ".bai").c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0 || !pwrite_all(fd, ix.data(), ix.size(), 0) || ::close(fd) != 0) { fprintf(stderr, "bmbs_search: cannot write %s.bai: %s\n", o.out.c_str(), strerror(errno)); R.failed = true; }
}

// --cytosine-report: <prefix>.cytosine_report.txt, every cytosine of the selected contexts of every sequence, in index order, no header
// line.  The genome is walked in windows of `window` bases, one bmbs_methyl_report call each, with the window's sites and the runs that
// reach into it; a window never spans two sequences.  The default window is what a 256 MiB page-locked buffer holds whatever the genome
// says: a line has at most name + 44 bytes (six tabs, strand, three letters, newline: 11; three numbers of at most ten digits; CHG).
// Two buffers: a writer thread puts one window into the file while the device makes the next.  `sites` are those the bedGraphs start
// from (behind the non-ACGT filter), the ones the variant filter dropped marked BMBS_REPORT_OMIT; --methyl-merge-context and
// --methyl-min-depth do not touch the report
void write_report(Run& R, Pass2& S, const std::vector<bmbs_methyl_site>& sites, const std::vector<std::vector<std::pair<int64_t, int64_t>>>& runs)
{
    const Options& o = R.o;
    const double t_begin = now();
    const std::string path = o.methyl + ".cytosine_report.txt";
    const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) { fprintf(stderr, "bmbs_search: cannot write %s: %s\n", path.c_str(), strerror(errno)); R.failed = true; return; }
    size_t name_max = 0;
    for (const std::string& n : R.chrom_names) name_max = std::max(name_max, n.size());
    const uint64_t buf_bytes = 256ull << 20;
    const int64_t window = o.report_window ? (int64_t)o.report_window : std::max<int64_t>(32, (int64_t)(buf_bytes / (name_max + 44)) & ~31ll);
    bmbs_ctx* const ctx = R.ctxs[0];
    Pinned buf[2];
    struct Job { int b; uint64_t bytes, off; };      // (b < 0: the last)
    Chan<Job> full; Chan<int> empty;
    empty.put(0); empty.put(1);
    std::atomic<bool> write_failed{false};
    std::thread writer([&] {
        for (Job j = full.get(); j.b >= 0; j = full.get()) {
            if (!write_failed && !pwrite_all(fd, buf[j.b].p, (size_t)j.bytes, (size_t)j.off)) write_failed = true;
            empty.put(j.b);
        }
    });
    uint64_t off = 0;
    size_t s0 = 0;
    for (int32_t ref = 0; ref < R.view.n_chrom && !R.failed && !write_failed; ref++) {
        const int64_t len = (int64_t)R.view.chrom_len[ref];
        static const std::vector<std::pair<int64_t, int64_t>> none;
        const auto& rr = (size_t)ref < runs.size() ? runs[(size_t)ref] : none;
        size_t r0 = 0;
        for (int64_t beg = 0; beg < len && !R.failed && !write_failed; beg += window) {
            const int64_t end = std::min(len, beg + window);
            size_t s1 = s0;
            while (s1 < sites.size() && sites[s1].ref == ref && sites[s1].pos < end) s1++;
            // the runs that reach into [beg - 2, end + 2): what a context window of this window's cytosines can touch
            while (r0 < rr.size() && rr[r0].second <= beg - 2) r0++;
            size_t r1 = r0;
            while (r1 < rr.size() && rr[r1].first < end + 2) r1++;
            const double t_w = now();
            const int b = empty.get();
            const double t_c = now();
            S.t_report_wait += t_c - t_w;
            uint64_t bytes = 0; int64_t lines = 0;
            int rc = BMBS_ENOMEM;
            for (int attempt = 0; attempt < 2 && rc == BMBS_ENOMEM; attempt++) {
                if (!buf[b].need(attempt ? (size_t)bytes : (size_t)std::min<uint64_t>(buf_bytes, (uint64_t)(end - beg) * (name_max + 44)))) { rc = BMBS_ENOMEM; break; }
                rc = bmbs_methyl_report(ctx, ref, beg, end, sites.data() + s0, (int64_t)(s1 - s0), r1 > r0 ? &rr[r0].first : nullptr, (int64_t)(r1 - r0), o.mpar.contexts,
                                        buf[b].p, buf[b].cap, &bytes, &lines);
            }
            S.t_report_calls += now() - t_c;
            if (rc) { fprintf(stderr, "bmbs_search: --cytosine-report: %s\n", rc == BMBS_ENOMEM ? "no page-locked memory for a window's text" : bmbs_last_error(ctx)); R.failed = true; empty.put(b); break; }
            full.put(Job{b, bytes, off});
            off += bytes; S.report_lines += (uint64_t)lines;
            s0 = s1;
        }
        while (s0 < sites.size() && sites[s0].ref == ref) s0++;              // (none: every site lies in its sequence)
    }
    full.put(Job{-1, 0, 0});
    writer.join();
    if (write_failed || ::close(fd) != 0) { fprintf(stderr, "bmbs_search: cannot write %s: %s\n", path.c_str(), strerror(errno)); R.failed = true; }
    buf[0].release(); buf[1].release();
    S.report_bytes = off;
    S.t_report = now() - t_begin;
}

// --methyl: the files, written once the BAM is complete.  In this order: sites that touch a base the FASTA does not spell A, C, G or T
// are left out; the variant filter drops the sites the opposite strand shows to be polymorphisms (bmbs_methyl_drop_variants);
// --methyl-merge-context adds the two strands of a CpG / CHG; --methyl-min-depth leaves out the lines below it
void write_methyl(Run& R, Pass2& S)
{
    const Options& o = R.o;
    const std::string& index = R.index;
    std::vector<bmbs_methyl_site>& sites = S.meth_sites;
    std::vector<std::vector<std::pair<int64_t, int64_t>>> runs;
    if (!non_acgt_runs(index, R.view, runs)) {
        fprintf(stderr, "bmbs_search: --methyl: cannot read the sequences of the index from %s: sites at bases other than A, C, G and T are not filtered out\n", index.c_str());
        runs.clear();                                                        // (--cytosine-report: no runs either, so that it agrees with the sites)
    } else {
        size_t kept = 0;
        for (const bmbs_methyl_site& s : sites) if (runs[(size_t)s.ref].empty() || !methyl_touches(runs[(size_t)s.ref], s)) sites[kept++] = s;
        S.meth_dropped = sites.size() - kept;
        sites.resize(kept);
    }
    // --cytosine-report: the sites as they are now; those the variant filter drops stay in this list, marked
    std::vector<bmbs_methyl_site> rsites;
    if (o.cytosine_report && o.min_opp_depth > 0) rsites = sites;
    if (o.min_opp_depth > 0) {
        int64_t kept = 0;
        if (bmbs_methyl_drop_variants(sites.data(), (int64_t)sites.size(), S.meth_opp.data(), (int64_t)S.meth_opp.size(), (int32_t)o.min_opp_depth, o.max_variant_ppm, &kept)) {
            fprintf(stderr, "bmbs_search: --methyl: the sites or the opposite-strand entries are out of order\n"); R.failed = true; return;
        }
        S.meth_variants = sites.size() - (size_t)kept;
        sites.resize((size_t)kept);
    }
    for (const bmbs_methyl_site& s : sites) { S.meth_n[s.kind & 3u]++; S.meth_calls[s.kind & 3u] += (size_t)s.meth + s.unmeth; }
    for (unsigned x = 0; x < 3 && !R.failed; x++) {
        if (!((o.mpar.contexts >> x) & 1)) continue;
        const std::string path = o.methyl + "_" + ctx_names[x] + ".bedGraph";
        if (!methyl_write(path, o.methyl, ctx_names[x], x, sites, R.ixf, o.merge_context, (uint64_t)o.min_depth, &S.meth_shallow)) { fprintf(stderr, "bmbs_search: cannot write %s: %s\n", path.c_str(), strerror(errno)); R.failed = true; }
    }
    if (o.cytosine_report && !R.failed) {
        // (a merge walk of the lists before and behind the filter: what is missing behind it was dropped)
        size_t k = 0;
        for (bmbs_methyl_site& s : rsites) { if (k < sites.size() && sites[k].ref == s.ref && sites[k].pos == s.pos) k++; else s.kind |= BMBS_REPORT_OMIT; }
        write_report(R, S, o.min_opp_depth > 0 ? rsites : sites, runs);
    }
    // --mbias: the table as the device made it (calls at bases the FASTA does not spell A, C, G or T are in it: only sites are filtered)
    if (o.mbias && !R.failed) {
        S.mbias.resize((size_t)24 * BMBS_MBIAS_CYCLES, 0);               // (a run without a pass-2 call: all zero)
        for (const uint64_t v : S.mbias) S.mbias_calls += v;
        const std::string path = o.methyl + "_mbias.tsv";
        if (!mbias_write(path, S.mbias)) { fprintf(stderr, "bmbs_search: cannot write %s: %s\n", path.c_str(), strerror(errno)); R.failed = true; }
    }
}

// --conversion-report <file>: the calls of all examined records by strand and context, the non-CpG conversion rate (unmethylated CHG and
// CHH calls of all such calls, in hundredths of a percent, rounded half up), the templates and how many failed the filter.  Exact
// integers; tests/nonconv_spec.py::report_text defines the text
void write_conversion_report(Run& R)
{
    const Options& o = R.o;
    FILE* f = fopen(o.conversion_report.c_str(), "w");
    if (!f) { fprintf(stderr, "bmbs_search: cannot write %s: %s\n", o.conversion_report.c_str(), strerror(errno)); R.failed = true; return; }
    fputs("#strand\tcontext\tmethylated\tunmethylated\tpercent\n", f);
    unsigned long long nm = 0, nu = 0;
    for (int s = 0; s < 2; s++)
        for (int x = 0; x < 3; x++) {
            const unsigned long long u = R.nc_totals[(s * 3 + x) * 2], m = R.nc_totals[(s * 3 + x) * 2 + 1];
            if (x) { nm += m; nu += u; }
            if (m + u) fprintf(f, "%s\t%s\t%llu\t%llu\t%llu\n", s ? "OB" : "OT", ctx_names[x], m, u, (200 * m + m + u) / (2 * (m + u)));
            else fprintf(f, "%s\t%s\t0\t0\tNA\n", s ? "OB" : "OT", ctx_names[x]);
        }
    if (nm + nu) { const unsigned long long bp = (20000 * nu + nm + nu) / (2 * (nm + nu)); fprintf(f, "non-CpG conversion rate\t%llu\t%llu\t%llu.%02llu\n", nu, nm + nu, bp / 100, bp % 100); }
    else fputs("non-CpG conversion rate\t0\t0\tNA\n", f);
    fprintf(f, "templates\t%ld\tfailed\t%ld\n", R.nc_templates, R.nc_failed);
    if (fclose(f)) { fprintf(stderr, "bmbs_search: cannot write %s: %s\n", o.conversion_report.c_str(), strerror(errno)); R.failed = true; }
}

// --trim-report: the counters of all batches, one line per counter and mate (mate 0: the line counts templates)
void write_trim_report(Run& R)
{
    const Options& o = R.o;
    FILE* f = fopen(o.trim_report.c_str(), "w");
    if (!f) { fprintf(stderr, "bmbs_search: cannot write %s: %s\n", o.trim_report.c_str(), strerror(errno)); R.failed = true; return; }
    const bmbs_trim_counts& t = R.trim_cnt;
    const struct { const char* name; const int64_t* v; } rows[] = {{"records_in", t.records_in}, {"bases_in", t.bases_in}, {"bases_out", t.bases_out},
        {"quality_records", t.quality_records}, {"quality_bases", t.quality_bases}, {"adapter_records", t.adapter_records}, {"adapter_bases", t.adapter_bases},
        {"clip_records", t.clip_records}, {"clip_bases", t.clip_bases}};
    // (--pbat pairs: the files went in swapped; the report speaks of read 1 and read 2 as the command line does)
    const bool swapped = o.pbat && o.pe;
    for (const auto& r : rows) for (int m = 0; m < o.nf(); m++) fprintf(f, "%s\t%d\t%lld\n", r.name, m + 1, (long long)r.v[swapped ? 1 - m : m]);
    fprintf(f, "templates_in\t0\t%ld\ntemplates_kept\t0\t%ld\ntemplates_dropped\t0\t%lld\n", R.trim_in, R.trim_kept, (long long)t.templates_dropped);
    if (fclose(f)) { fprintf(stderr, "bmbs_search: cannot write %s: %s\n", o.trim_report.c_str(), strerror(errno)); R.failed = true; }
}

// a failed run leaves no half-made sorted file, index or bedGraph behind
int give_up(Run& R)
{
    const Options& o = R.o;
    if (!o.conversion_report.empty()) ::unlink(o.conversion_report.c_str());
    if (!o.trim_report.empty()) ::unlink(o.trim_report.c_str());
    if (o.methyl_out) for (unsigned x = 0; x < 3; x++) if ((o.mpar.contexts >> x) & 1) ::unlink((o.methyl + "_" + ctx_names[x] + ".bedGraph").c_str());
    if (o.mbias) ::unlink((o.methyl + "_mbias.tsv").c_str());
    if (o.cytosine_report) ::unlink((o.methyl + ".cytosine_report.txt").c_str());
    if (o.sort && R.parts[0]->regular) ::unlink(o.out.c_str());      // a sorted file is whole or absent (a device or a pipe is left alone)
    if (o.bai && R.parts[0]->regular) ::unlink((o.out + ".bai").c_str());      // ... and so is its index
    fprintf(stderr, "bmbs_search: failed\n");
    return 1;
}

// the mapping statistics (stderr, --mapstats) and the --verbose lines
void report(const Run& R, const Pass2& S)
{
    const Options& o = R.o;
    int64_t st[5];
    bmbs_stats_allreduce(const_cast<bmbs_ctx**>(R.ctxs.data()), (int)R.ctxs.size(), st);      // get_mapping_informations: the counters of every worker summed
    // (--trim: the statistics count what was mapped; the reads of the dropped templates get a line of their own)
    const long long trimmed_away = (long long)R.trim_cnt.templates_dropped * o.nf();
    print_stats(stderr, st);
    if (o.trim) fprintf(stderr, "%-48s%lld\n", "No. of Reads Removed by Trimming:", trimmed_away);
    if (!o.mapstats.empty()) { FILE* m = fopen(o.mapstats.c_str(), "w"); if (m) { print_stats(m, st); if (o.trim) fprintf(m, "%-48s%lld\n", "No. of Reads Removed by Trimming:", trimmed_away); fclose(m); } }
    const double t_end = now();
    if (!o.verbose) return;
    long total_records = 0;
    double t_read = 0, t_write = 0, t_wait_r = 0, t_wait_w = 0;
    for (int p = 0; p < o.live_parts; p++) {
        const Part& pt = *R.parts[(size_t)p];
        total_records += pt.records; t_read += pt.t_read; t_write += pt.t_write; t_wait_r += pt.t_wait_r; t_wait_w += pt.t_wait_w;
    }
    const int n_ctx = o.n_ctx();
    const double t_format = 0;                   // (the device formats)
    fprintf(stderr, "[bmbs_search] records %ld  load+attach %.3fs  mapping wall %.3fs  (pipeline %.3fs; stage busy, summed over %d part(s): read + newline count %.3fs, gpu calls %.3fs over %d context(s), host format %.3fs, write %.3fs)  %d I/O threads, batch %ld, %zu device(s) x %d context(s), %d output part(s)\n",
            total_records, R.t_loaded - R.t_start, t_end - R.t_loaded, R.t_joined - R.t_loaded, o.live_parts, t_read, R.t_gpu, n_ctx, t_format, t_write, o.io_threads, o.batch,
            R.n_owner, o.contexts, o.parts);
    if (o.sort) {
        const SortStore& store = R.sort_store;
        char ixs[1000] = "";
        if (o.bai) snprintf(ixs, sizeof ixs, ", index: chunks %zu, windows %zu, %zu bytes", S.bai.n_chunks(), S.bai.n_windows(), S.bai_bytes);
        if (o.markdup)
            snprintf(ixs + strlen(ixs), sizeof ixs - strlen(ixs), ", markdup: templates %ld, with signature %ld, duplicates %zu (select calls %zu, %.3fs of pass 2)", store.templates,
                     store.with_sig, S.n_dup, S.select_calls, S.t_select - R.t_pass1);
        if (o.nonconv) snprintf(ixs + strlen(ixs), sizeof ixs - strlen(ixs), ", nonconv: templates %ld, failed %ld", R.nc_templates, R.nc_failed);
        if (o.methyl_out)
            snprintf(ixs + strlen(ixs), sizeof ixs - strlen(ixs), ", methyl: sites CpG %zu CHG %zu CHH %zu, calls CpG %zu CHG %zu CHH %zu, sites left out at bases other than ACGT %zu", S.meth_n[0],
                     S.meth_n[1], S.meth_n[2], S.meth_calls[0], S.meth_calls[1], S.meth_calls[2], S.meth_dropped);
        if (o.methyl_out)
            snprintf(ixs + strlen(ixs), sizeof ixs - strlen(ixs), ", sites dropped as variants %zu, lines left out below the minimum depth %zu", S.meth_variants, S.meth_shallow);
        if (o.mbias) snprintf(ixs + strlen(ixs), sizeof ixs - strlen(ixs), ", mbias calls %llu", (unsigned long long)S.mbias_calls);
        if (o.cytosine_report) snprintf(ixs + strlen(ixs), sizeof ixs - strlen(ixs), ", report lines %llu bytes %llu in %.3fs (device calls %.3fs, waiting for the file %.3fs)", (unsigned long long)S.report_lines, (unsigned long long)S.report_bytes, S.t_report, S.t_report_calls, S.t_report_wait);
        fprintf(stderr, "[bmbs_search] sort: bins %zu (one of them for records without a reference), pass-2 calls %zu, store bytes %zu (%ld records), pass 1 %.3fs (mapping, binning), pass 2 %.3fs (sort, deflate, write)%s\n",
                store.bin.size(), S.sort_calls, store.bytes, store.records, R.t_pass1 - R.t_loaded, R.t_pass2 - R.t_pass1, ixs);
    }
    fprintf(stderr, "[bmbs_search] stage idle (waiting for a batch, summed): readers %.3fs, gpu workers %.3fs, writers %.3fs\n", t_wait_r, R.t_wait_g, t_wait_w);
    // what bounds the run: the link's busy time per direction (copies of the text calls, summed over the contexts: one copy per direction
    // and device at a time) and the workers' busy time against the mapping wall
    double up = 0, down = 0, in_calls = 0, calls = 0;
    for (bmbs_ctx* c : R.ctxs) { double t4[4]; if (bmbs_text_times(c, t4) == 0) { up += t4[0]; down += t4[1]; in_calls += t4[2]; calls += t4[3]; } }
    const double wall_s = t_end - R.t_loaded, nd = (double)std::max<size_t>(1, R.n_owner);
    fprintf(stderr, "[bmbs_search] busy fractions of the mapping wall: link up %.3f, link down %.3f (per device), gpu workers %.3f, readers %.3f, writers %.3f  (text calls %.0f, %.3fs inside them)\n",
            up / nd / wall_s, down / nd / wall_s, R.t_gpu / std::max(1, n_ctx) / wall_s, t_read / std::max(1, o.live_parts) / wall_s, t_write / std::max(1, o.live_parts) / wall_s, calls, in_calls);
}

void teardown(Run& R)
{
    // (the device side of compressed input first: contexts of the sources' own, staging)
    for (int p = 0; p < R.o.live_parts; p++) { R.parts[(size_t)p]->s1.release_device(); R.parts[(size_t)p]->s2.release_device(); }
    const double t0 = now();
    for (auto& b : R.batches) { b.text1.release(); b.text2.release(); b.sam.release(); }
    const double t1 = now();
    for (size_t i = R.ctxs.size(); i-- > 0;) bmbs_destroy(R.ctxs[i]);     // the sharing contexts go before their owners
    const double t2 = now();
    bmbs_index_file_free(R.ixf);
    if (R.o.verbose) fprintf(stderr, "[bmbs_search] teardown: unpin %.3fs, destroy ctx %.3fs, free index %.3fs\n", t1 - t0, t2 - t1, now() - t2);
}

}  // namespace

int main(int argc, char** argv)
{
    const Options o = parse_options(argc, argv);
    if (!o.build_fasta.empty()) return build_index(o);
    g_loop_input = o.loop_input;
    const double t_start = now();
    if (o.print_parts) return print_parts_and_plan(o);
    // the drivers' contexts run one batch at a time each: one lane per context is enough (BMBS_LANES is only read by bmbs_create)
    setenv("BMBS_LANES", "1", 0);
    Run R(o);
    R.t_start = t_start;
    R.est0 = record_bytes_estimate(o.in1);
    if (int rc = load_index_and_contexts(R)) return rc;      // (starts R.prealloc)
    if (int rc = open_inputs(R)) return rc;
    if (int rc = open_outputs(R)) return rc;
    R.prealloc.join();
    prefault_buffers(R);
    if (o.sort) init_sort_store(R);
    R.t_loaded = now();

    map_all(R);

    Pass2 S;
    S.bai.init((size_t)R.view.n_chrom);
    R.t_pass1 = S.t_select = now();
    if (o.sort && !R.failed) sort_pass2(R, S);
    R.t_pass2 = now();
    finish_files(R);
    if (o.bai && !R.failed) write_bai(R, S);
    if (o.methyl_out && !R.failed) write_methyl(R, S);
    if (!o.conversion_report.empty() && !R.failed) write_conversion_report(R);
    if (!o.trim_report.empty() && !R.failed) write_trim_report(R);
    if (R.failed) return give_up(R);
    report(R, S);
    teardown(R);
    return 0;
}
