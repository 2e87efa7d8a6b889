// bitmapperbs_amd/csrc/bmbs_words.h -- the small words a lane's stages pass between device and host, named in one table that kernels and
// host code both include (through bmbs_dev.h).  Three word arrays per lane:
//   Lane::totals    TOT_WORDS u64 on the device     scan totals and stage counts            enum Tot
//   Lane::tx_info   TXI_WORDS u32 on the device     error / flag words of the text and record kernels
//   Lane::h_tot, Lane::h_info                       their page-locked mirrors               struct CallWords, struct HostInfo
// A stage that needs a word claims it HERE: a name, who writes it, who reads it, and what lies between the two.  Nothing outside this
// file addresses the arrays by number (tests/test_scratch_words.py).  The numbers are part of no kernel: a kernel gets a pointer to
// its word from the host (tot_at(), bmbs_host.h) -- except k_call_chain_counts, which is handed the array.
#ifndef BMBS_WORDS_H
#define BMBS_WORDS_H
#include <stddef.h>
#include <stdint.h>

// ---- Lane::totals ------------------------------------------------------------------------------------------------------------------------
// Every word is written on the lane's stream (scan_u32's last kernel unless noted) and read by later kernels of the same stream through
// the pointer they are given, or by the host behind a copy and a wait on that stream: stream order is what lies between writer and
// reader everywhere; the table says so only where a word has more than one use.
// Three groups: [0, TOT_CALL_WORDS) belongs to a mapping call -- call_begin zeroes it, call_end copies it to the call's CallWords;
// [TOT_LINES_1, TOT_SORT_IN) to the text calls (bmbs_textpath.hip); [TOT_SORT_IN, TOT_WORDS) to the record stages (bmbs_records.hip).
// The text calls and the record stages run on lane 0 with nothing in flight (ON_LANE0, lane_settle), one at a time.
enum Tot : int {
    // -- a mapping call (bmbs_api.hip).                           written by                     read by
    TOT_CAND = 0,            // candidate slots of the call         scan_cand                      k_guard_cand / _done, cand_total (exact), k_vote_compact; lane_settle (lr_cand)
    TOT_JOBS = 1,            // alignment jobs                      scan_jobs                      k_guard_jobs / _done, align_jobs (exact), the K11-K13 kernels; lane_settle
    TOT_SW = 2,              // jobs that need the DP               scan_sw                        k_guard_count, the DP kernels; lane_settle (lr_sw)
    TOT_SEED_SECOND = 3,     // reads on k_seed_second's list       list_second                    k_seed_second
    TOT_SEED_EXTRA = 4,      // reads on k_seed_extra's list        list_extra                     k_seed_extra
    TOT_VOTES = 5,           // single end: votes to verify         vote_compact                   k_filter
    TOT_PE_WORK = 6,         // paired end: the work list of one    verify_round[_pairs]           k_filter_pe of that round (each round writes it anew)
                             // verification round
    TOT_RESEED = 7,          // --sensitive: pairs to re-seed       k_pes_reseed's scan            k_pes_reseed, k_pes_vote; verify_sensitive (exact: with TOT_RCAND, one copy)
    TOT_RCAND = 8,           // --sensitive: their candidates       the scan behind k_pes_reseed   k_guard_rcand / _done; verify_sensitive (exact); lane_settle (lr_rcand)
    TOT_LONG = 9,            // reads on the long list              k_vote[_pe]_long's scan        k_vote[_pe]_long (wave form); lane_settle (lr_long)
    TOT_VOTE_READS = 10,     // single end: reads with candidates   k_vote_fused's scan            k_vote_fused, k_reduce
    TOT_MID = 11,            // reads on the mid list               k_vote[_pe]_mid's scan         k_vote[_pe]_mid; lane_settle (lr_long)
    TOT_PEF_LONG = 12,       // pairs left to                       verify_fast's scan             k_pe_filter_pairs_long
                             // k_pe_filter_pairs_long
    TOT_BIG = 13,            // lists the wave form handed on       memset, then atomics of        the block forms of k_vote[_pe]_long
                             // (a counter, not a scan)             k_vote[_pe]_long (wave form)
    // One word, two uses.  --sensitive: mates on k_pes_vote_long's list -- written by the scan behind k_pes_vote, read by the three
    // k_pes_vote_long launches that follow it.  Every call: the 16-mer lookups of the call, with TOT_CHAIN_EXT the extensions -- written
    // by k_call_chain_counts in call_end, read by lane_settle (lr_chain).  call_end is the last thing a call puts on the stream, so the
    // list kernels have read their count before the lookups overwrite it; no reader of the second use sees the first.
    TOT_PESV_LONG = 14,
    TOT_CHAIN_LOOKUPS = 14,
    TOT_CHAIN_EXT = 15,      // (k_call_chain_counts writes totals[TOT_CHAIN_LOOKUPS + j], j = 0, 1)
    TOT_CALL_WORDS = 16,
    // -- the text calls (bmbs_textpath.hip).
    TOT_LINES_1 = 16,        // lines found in the text window of   text_index                     lane_text_finish, lane_text_open_finish (both words, one copy)
    TOT_LINES_2 = 17,        // file 1 / file 2 (tot_file)
    TOT_SAM_BYTES = 18,      // SAM text of the batch               k_sam_len's scan               lane_text_finish
    TOT_BAM_BYTES = 19,      // BAM records of the batch            k_bam_len's scan               lane_text_finish; k_bgzf_block (bgzf_deflate's total_ptr)
    // One word, two uses, one behind the other in a text call.  --trim: the templates the length filter keeps -- written by the scan of
    // k_trim_keep's flags (trim_stage), read by TextCall::records behind the wait it has anyway, with the lane's trim words.  Then the
    // compressed bytes of the call's blocks: bgzf_deflate runs behind the mapping, long after records() has read the first use.  (The
    // array keeps its size and every other word its place: a call with trimming off must not differ from what it was.)
    TOT_TRIM_KEPT = 20,
    TOT_BGZF_BYTES = 20,     // compressed bytes of the blocks      bgzf_deflate's scan            bgzf_deflate
    TOT_NL_ADDED_1 = 21,     // 1: the window of file 1 / file 2    k_close_last_line or a         lane_text_open_bgzf (both words, one copy, behind a wait for
    TOT_NL_ADDED_2 = 22,     // got a last newline (tot_file)       memset, on the FILE's stream   file 2's stream)
    TOT_SORTED_BYTES = 23,   // the sorted record stream            bam_sort_device's scan         k_bgzf_block (lane_bam_sort: bgzf_deflate's total_ptr)
    // -- the record stages (bmbs_records.hip).
    TOT_SORT_IN = 24,        // bytes bmbs_bam_sort uploaded        records_stage                  nobody (the host knows it: the scan needs a place for its total)
    TOT_BAI_HEADS = 25,      // bai_compute: chunk heads,           its three scans                bai_compute (the three words, one copy)
    TOT_BAI_WINS = 26,       // window candidates,
    TOT_BAI_REFS = 27,       // references that have records
    TOT_BAI_NWIN = 28,       // bai_compute: windows written        the scan of k_bai_win_flag     k_bai_win_out; bai_compute
    TOT_RECS_IN = 29,        // bytes bmbs_bam_dup_sigs /           records_stage                  nobody (as TOT_SORT_IN; dp_in and mt_in are different buffers, the
                             // bmbs_bam_methyl uploaded                                           word says nothing about either)
    // One word, two uses, both methyl_device's.  The events of all records: written by the scan behind the counting pass, read by the
    // host behind a wait, BEFORE the first slice is reduced.  The run heads of one reduction (meth_reduce): written by its first scan,
    // read by the host behind meth_reduce's own wait.  The host has the event count before meth_reduce is first called.
    TOT_METH_EVENTS = 30,
    TOT_METH_HEADS = 30,
    // One word, two throw-aways: meth_reduce scans the methylated and the unmethylated counts one behind the other; it needs the
    // offsets, nobody reads either total.
    TOT_METH_M = 31,
    TOT_METH_U = 31,
    TOT_CYT_BYTES = 32,      // bmbs_methyl_report: the text of the   the scan behind k_cyt_count    lane_methyl_report (the two words, one copy)
    TOT_CYT_LINES = 33,      // window, and its lines                 memset, then k_cyt_count's adds (a counter, not a scan)
    TOT_WORDS = 34
};
// the word of file f (0, 1) of a pair of words: TOT_LINES_1, TOT_NL_ADDED_1
constexpr Tot tot_file(Tot first, int f) { return (Tot)(first + f); }
static_assert(TOT_LINES_2 == TOT_LINES_1 + 1 && TOT_NL_ADDED_2 == TOT_NL_ADDED_1 + 1, "tot_file, and the copies that take both words");
static_assert(TOT_RCAND == TOT_RESEED + 1, "verify_sensitive copies the two as one");
static_assert(TOT_CHAIN_EXT == TOT_CHAIN_LOOKUPS + 1, "k_call_chain_counts writes the two from one base");
static_assert(TOT_BAI_WINS == TOT_BAI_HEADS + 1 && TOT_BAI_REFS == TOT_BAI_HEADS + 2, "bai_compute copies the three as one");
static_assert(TOT_CYT_LINES == TOT_CYT_BYTES + 1, "lane_methyl_report copies the two as one");
static_assert(TOT_CHAIN_EXT < TOT_CALL_WORDS && TOT_CALL_WORDS <= TOT_LINES_1 && TOT_CYT_LINES < TOT_WORDS, "the groups fit the array");

// ---- the guard flags of a mapping call (Lane::flags, u32; k_reduce.hip: the guards raise them, k_stats_commit and lane_settle read them) --
#define BMBS_FLAG_CAND   0   // candidate slots > capacity
#define BMBS_FLAG_SW     1   // DP jobs > capacity of the launches issued
#define BMBS_FLAG_RCAND  2   // --sensitive: re-seeded candidates > capacity
#define BMBS_FLAG_CIGAR  3   // the caller's CIGAR pool is too small for the jobs of this batch (an error, not a retry)
#define BMBS_FLAG_WORDS  8

// ---- Lane::h_tot: BMBS_SLOTS page-locked records, one per call a lane may have in flight.  call_end copies the call's group of totals
// and the flag words into its record, lane_settle reads them behind its wait for the stream.
#define BMBS_SLOTS 8
struct CallWords { uint64_t tot[TOT_CALL_WORDS]; uint32_t flags[BMBS_FLAG_WORDS]; };
#define BMBS_SLOT_WORDS (TOT_CALL_WORDS + BMBS_FLAG_WORDS / 2)          // u64 words of a record: the totals and, behind them, the flags
static_assert(BMBS_FLAG_CIGAR < BMBS_FLAG_WORDS && BMBS_FLAG_WORDS % 2 == 0, "the flags fill whole u64 words");
static_assert(sizeof(CallWords) == BMBS_SLOT_WORDS * 8 && offsetof(CallWords, flags) == TOT_CALL_WORDS * 8, "the flag words fit behind the totals");

// ---- Lane::tx_info: two halves of TXI_HALF_WORDS u32.  What a kernel does with info[0], info[1], ... of the pointer it is given is
// that kernel's contract, written at the kernel; here is only whose half it is.
//   the line half   k_fq_records (TXI_FQ_WORDS words per file: file 2's start behind file 1's) and k_bam_len (word 3) of a text call;
//                   zeroed with the whole array when a text call begins
//   the stage half  one kernel family at a time, zeroed by the stage that is about to use it: k_bam_keys (bam_sort_device),
//                   k_bai_records, k_dup_sig, k_dup_bits + k_dup_heads (words 0..5 as three u64, word TXI_DUP_COUNT),
//                   k_meth_events (the emitting pass is handed words TXI_METH_EMIT.. and writes none), k_meth_cut (words 0..1 as
//                   one u64), k_meth_clip, k_cyt_check (TXI_CYT_WORDS words).  Every stage waits for its words before it returns or launches the next family.
#define TXI_HALF_WORDS 8
#define TXI_LINE       0
#define TXI_STAGE      TXI_HALF_WORDS
#define TXI_WORDS      (2 * TXI_HALF_WORDS)
#define TXI_FQ_WORDS   4
#define TXI_DUP_COUNT  6     // k_dup_heads: the duplicates it marked
#define TXI_METH_EMIT  4
#define TXI_CYT_WORDS  6     // k_cyt_check: one word per kind of refusal
static_assert(2 * TXI_FQ_WORDS <= TXI_HALF_WORDS && TXI_DUP_COUNT >= 3 * 2 && TXI_DUP_COUNT < TXI_HALF_WORDS && TXI_METH_EMIT + 4 <= TXI_HALF_WORDS && TXI_CYT_WORDS <= TXI_HALF_WORDS, "the halves hold their kernels' words");

// ---- Lane::tr_words: what the trim stage of a text call (k_trim.hip; bmbs_set_trim) counts.  trim_stage zeroes the array on the lane's
// stream before its first kernel; k_fq_trim (one launch per file: mate m adds to the words TRW_PER_MATE * m + ...) and k_fq_compact add
// to it with 64-bit atomics; TextCall::records copies it to h_info->trim behind the wait it has anyway.  The counters belong to the call:
// a call repeated after BMBS_ENOMEM starts from zero again.
enum TrimWord : int {
    TRW_RECORDS_IN = 0,      // records k_fq_trim saw
    TRW_BASES_IN = 1,        // ... and their bases
    TRW_Q_RECORDS = 2,       // records the quality step shortened, and by how many bases
    TRW_Q_BASES = 3,
    TRW_A_RECORDS = 4,       // ... the adapter step
    TRW_A_BASES = 5,
    TRW_C_RECORDS = 6,       // ... the fixed clips
    TRW_C_BASES = 7,
    TRW_TRIM_COUNTERS = 8,   // (what k_fq_trim tallies in LDS)
    TRW_BASES_OUT = 8,       // k_fq_compact: bases of the records that stay
    TRW_PER_MATE = 9,
    TRW_MAX_LEN = 2 * TRW_PER_MATE,          // k_fq_compact, both files: the longest read that stays (atomic max),
    TRW_MIN_LEN_C = 2 * TRW_PER_MATE + 1,    // and the complement of the shortest (atomic max; 0: nothing stays)
    TRW_WORDS = 2 * TRW_PER_MATE + 2
};

// ---- Lane::h_info: the page-locked block the text calls and the record stages read their words from.  No kernel sees it; one field
// per use.  The uses that share bytes: `line` (one text call's k_fq_records, then its k_bam_len), `stage` (every stage's u32 words),
// `out_bytes` (SAM or BAM), `z_bytes` (two callers of bgzf_deflate), `meth_eoff` (two reads of one slice).  That is safe because each
// user copies, waits and reads before it goes on, and the text calls and record stages run one at a time (ON_LANE0).
struct HostInfo {
    uint32_t line[TXI_HALF_WORDS];      // the line half of tx_info as a text call left it (lane_text_finish: behind k_fq_records, and again behind k_bam_len)
    uint32_t stage[TXI_HALF_WORDS];     // the stage half, word for word; every stage's
    uint64_t dup_bits[3];               // ... and the same words where a kernel wrote them as u64: k_dup_bits' three ORs,
    uint64_t meth_cut;                  // k_meth_cut's end of a slice
    uint64_t meth_eoff;                 // mt_eoff[start], then mt_eoff[end] of that slice (meth_slice)
    uint64_t lines[2];                  // TOT_LINES_1, _2
    uint32_t last_nl[2];                // where the last newline of the window's whole records is (tx_nl, per file)
    uint64_t nl_added[2];               // TOT_NL_ADDED_1, _2
    uint64_t out_bytes;                 // TOT_SAM_BYTES or TOT_BAM_BYTES: a text call writes one of the two
    uint64_t z_bytes;                   // TOT_BGZF_BYTES (bgzf_deflate: the text calls' and bmbs_bam_sort's)
    uint64_t bai[3];                    // TOT_BAI_HEADS, _WINS, _REFS
    uint64_t bai_nwin;                  // TOT_BAI_NWIN
    uint64_t meth_events;               // TOT_METH_EVENTS
    uint64_t meth_heads;                // TOT_METH_HEADS
    uint64_t cyt[2];                    // TOT_CYT_BYTES, _LINES
    uint64_t trim_kept;                 // TOT_TRIM_KEPT
    uint64_t trim[TRW_WORDS];           // Lane::tr_words as a text call's trim stage left them
};
#endif
