/* include/bmbs.h -- C-ABI of the MI355X-native BitMapperBS mapping hot path (libbmbs_hip.so).
 *
 * BitMapperBS has no plugin/FFI layer: this is the boundary *cut* at L4 -> {L5,L6,L7}.
 * A host driver that keeps BitMapperBS's CLI, FASTQ reader and SAM writer calls these entry points
 * where the reference calls (per read, inline) the routines cited at each declaration; paths are
 * relative to the reference tree.  Conventions kept from the reference side of the cut:
 *   - index arrays are read-only after attach (Load_Index, Index.cpp:940);
 *   - errors are status codes / sentinels, never exceptions: err = 0xFFFFFFFF, end_site = -1
 *     (Levenshtein_Cal.h:354,512), calls return 0 or a negative BMBS_E*;
 *   - the caller owns host buffers, the library owns device buffers; one bmbs_ctx per GPU;
 *     calls on one ctx are serialised by the caller, different ctxs are fully concurrent.
 * Plain C types only (no torch / HIP types in any signature).
 */
#ifndef BMBS_H
#define BMBS_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BMBS_OK            0
/* the longest read the path takes.  The reference sizes its per-read buffers for 1000 characters (Auxiliary.h:14) and has no room for
 * their terminators at 999 and 1000: it prints 222 of 300 records at those lengths, one with bytes outside ASCII
 * (tests/golden/make_golden.py) -- there is nothing to be identical to, so reads of 999 and 1000 bases are refused (BMBS_EINVAL)
 * rather than mapped unpinned.  998 is pinned by goldens (se_g998, pe_p998).                                                    */
#define BMBS_MAX_READ    998
#define BMBS_EINVAL      (-22)
#define BMBS_ENOMEM      (-12)
#define BMBS_ENODEV      (-19)   /* no HIP device / runtime error: the product never falls back to CPU */
#define BMBS_ESTATE       (-1)   /* index not attached, batch too large, ... */

typedef struct bmbs_ctx bmbs_ctx;

/* mapping parameters == the reference's option globals (Process_CommandLines.cpp:40-75,88-132) */
typedef struct bmbs_params {
    double  e_f;        /* -e, thread_e_f: k = (uint64)(e_f * L) capped at 31 (Schema.cpp:24546)   */
    int32_t mp_max;     /* --mp_max 6  */
    int32_t mp_min;     /* --mp_min 2  */
    int32_t np;         /* --np 1      */
    int32_t gap_open;   /* --gap_open 5 */
    int32_t gap_ext;    /* --gap_extension 3 */
    int32_t q_base;     /* 33 | 64     */
    int32_t seed_len;   /* --seed (over_all_seed_length) 30 */
    int32_t min_ins;    /* --min 0     */
    int32_t max_ins;    /* --max 500   */
    int32_t sensitive;  /* --sensitive */
    int32_t ambiguous_out; /* --ambiguous_out: one hit of every ambiguous read / pair is aligned and returned with status
                            * BMBS_ST_AMBIG (Schema.cpp:24639, 25095, 19345); 0 = ambiguous reads carry no alignment.
                            * --unmapped_out and --pbat need nothing from the device: the former prints the records whose
                            * status is BMBS_ST_UNMAPPED / BMBS_ST_OFFEND, the latter maps the reverse complement of each
                            * read with mirrored qualities (Process_Reads.cpp:986-1075; see bmbs_search.cpp) */
} bmbs_params;

void bmbs_default_params(bmbs_params* p);

/* host view of the reference's loaded index: global `bitmapper_index_params` (bwt.h:34-163, filled by
 * load_index, bwt.cpp:2563-2643), the 2-bit genome `_ih_refGen` and the chromosome table
 * (Load_Index, Index.cpp:940-1045).  All pointers are host memory in the on-disk layouts. */
typedef struct bmbs_index_view {
    uint64_t        ref_len;            /* refGenLength (one strand) */
    const uint8_t*  pac;                /* .bs.pac payload, 4 bases/byte MSB first */
    uint64_t        pac_bytes;
    uint64_t        sa_length;          /* rows = 2*ref_len + 1 */
    uint64_t        shapline;
    uint64_t        nacgt[5];
    const uint64_t* bwt;                /* 5 x u64 per 128 rows */
    uint64_t        bwt_words;
    const uint64_t* high_occ;           /* 2 x u64 per 65536 rows */
    uint64_t        high_occ_words;
    const uint32_t* hash_hi;            /* 16-mer table, 3^16+1 entries */
    const uint8_t*  hash_lo;
    uint64_t        hash_entries;
    const uint32_t* sa;                 /* sampled SA (every 8th text position) */
    uint64_t        sa_entries;
    const uint64_t* sa_flag;            /* 5 x u64 per 256 rows */
    uint64_t        sa_flag_words;
    int32_t         n_chrom;
    const uint64_t* chrom_len;          /* _rg_chrome_length[n_chrom] */
} bmbs_index_view;

/* one mapped read; 32 bytes.  What output_sam_end_to_end (Schema.cpp:11928) is handed, after the
 * chromosome lookup and the off-end check it performs (11962-11986). */
typedef struct bmbs_result {
    uint64_t pos;          /* 1-based position on `chrom`                                    */
    uint32_t cigar_off;    /* first op in the cigar pool (only when n_cigar > 0; else "<L>M") */
    int32_t  chrom;        /* chromosome id (32 bits: scaffold-level assemblies have > 32 767 sequences) */
    uint16_t flag;         /* 0 | 16 (SE); 99/147/83/163 (PE)                                */
    uint16_t nm;           /* NM:i                                                           */
    int16_t  score;        /* alignment score (<= 0)                                         */
    uint8_t  status;       /* BMBS_ST_*                                                      */
    uint8_t  mapq;
    uint8_t  n_cigar;      /* ops in the pool; 0 means the single op <L>M                    */
    uint8_t  path;         /* 1 exact-unique exit, 2 one-mismatch exit, 3 general, 4 exact-ambiguous */
    uint16_t n_cand;       /* candidate sites located for this read (diagnostic, saturates at 65 535) */
    uint32_t tlen;         /* paired end: |TLEN| of the pair; 0 for single-end records       */
} bmbs_result;

#define BMBS_ST_UNMAPPED  0
#define BMBS_ST_UNIQUE    1   /* a SAM record is emitted                                       */
#define BMBS_ST_AMBIG     2   /* counted as ambiguous, nothing emitted (no --ambiguous_out)     */
#define BMBS_ST_OFFEND    3   /* alignment crosses a chromosome end: rejected at emit           */

/* cigar op = len << 4 | op, op 0 M, 1 D, 2 I, already in SAM (left-to-right on the forward strand)
 * order (ksw.cpp:2785-2857 prints them forward or reversed by strand) */

/* ---- launch sequence ----------------------------------------------------------------------------
 * A context owns BMBS_LANES (environment, default 3) lanes: a stream, work buffers and counters each, on one attached index.  A
 * mapping call of 500 000 units and more is cut into one chunk per lane, so that the issue-bound kernels of one chunk (DP, Myers,
 * row preparation) and the list kernels, which wait on their own chains, run beside the memory-bound seeding kernels of another; the host-pointer calls also overlap the copies of one
 * chunk with the kernels of another.  After the first call of a context no call waits for its stage counts: buffers and grids
 * are sized from what earlier calls needed per read (+25 %), guard kernels compare the real counts on the device, and a call that
 * did not fit is issued again with exact sizes when the context is next synchronised -- results and statistics are the same either
 * way.  BMBS_EXACT=1 makes every call wait for its counts (the round-2 sequence), BMBS_LANES=1 turns the split off.            */

/* ---- lifecycle -------------------------------------------------------------------------------- */
/* replaces Prepare_alignment (Schema.cpp:639: LUTs, score matrices) for one GPU                 */
bmbs_ctx* bmbs_create(int device_id, const bmbs_params* params);
void      bmbs_destroy(bmbs_ctx*);
const char* bmbs_last_error(const bmbs_ctx*);
/* replaces the in-memory result of Load_Index + load_index: uploads once, re-packs for HBM        */
int bmbs_index_attach(bmbs_ctx*, const bmbs_index_view*);
/* takes device memory for the work buffers of later calls now (bytes per lane; about 2.5 KB per read of the largest batch for the
 * text calls): optional, saves the first calls the device-wide allocation                                           */
int bmbs_reserve(bmbs_ctx*, uint64_t bytes_per_lane);
/* a further context on the index `owner` has attached (same device): shares the index in HBM, owns its stream and work buffers.
 * For keeping two batches in flight from two host threads; `owner` has to outlive it.                                  */
int bmbs_index_share(bmbs_ctx*, const bmbs_ctx* owner);

/* ---- stage entry points (host buffers in, host buffers out; used by the parity tests) ---------- */
/* reads: n rows of `stride` bytes ASCII upper-case (as produced by inputReads_single_directly,
 * Process_Reads.cpp:810), all of length L. */

/* K7 alone: get_actuall_genome / get_actuall_rc_genome (Schema.cpp:4998-5115): the `len` bases (len <= 1024) of the doubled
 * genome that start at doubled coordinate site[i], as ASCII into out + i*len; an out-of-strand request gives the reference's
 * all-zero window (bytes 0).  Used by the parity tests to check the HBM genome against the index files.                 */
int bmbs_window_batch(bmbs_ctx*, const uint64_t* site, int64_t n_sites, int32_t len, char* out);

/* K5 alone: locate_one_position_direct (bwt.h:2585) without the seed adjustment: the text position SA[row] of each
 * suffix-array row (0 <= row <= 2*ref_len).                                                                            */
int bmbs_locate_batch(bmbs_ctx*, const uint64_t* row, int64_t n_rows, uint64_t* pos);

/* a9 alone: the order in which `std::sort(votes, votes + n, compare_seed_votes)` (Schema.cpp:560-563, 24986 -- an unstable sort:
 * libstdc++'s introsort) visits vote lists.  List s is vote[seg_off[s] .. seg_off[s+1]) (counts 1..255); perm[seg_off[s] + j] =
 * index within list s of the entry visited j-th.  form 0: the one-wave kernel (lists of up to 256 entries), form 1: the
 * one-block kernel (up to 4096) -- the two forms k_vote_long runs on the candidate lists of repeat reads.               */
int bmbs_vote_order_batch(bmbs_ctx*, const uint8_t* vote, const int64_t* seg_off, int64_t n_seg, int32_t form, uint32_t* perm);

/* K7+K8: get_actuall_[rc_]genome + BS_Reserve_Banded_BPM{,_4_SSE,_8_SSE}
 * (Schema.cpp:4998-5115; Levenshtein_Cal.h:351,1678,2093): candidate i = (read_of[i], site[i]).   */
int bmbs_filter_batch(bmbs_ctx*, const char* seq, int32_t L, int32_t stride, int64_t n_reads,
                      const uint32_t* read_of, const uint64_t* site, int64_t n_cand,
                      uint32_t* err, int32_t* end_site);

/* the same call on the form the mapping calls run: the rows are packed on the device first (2 bits per base + a not-ACGT bit plane, what
 * k_filter / k_filter_pe read since round 4) and the Myers rows take their characters from the packed words.  Same results as
 * bmbs_filter_batch for every input, characters outside ACGT included (tests/test_gpu_parity.py).                                  */
int bmbs_filter_batch_packed(bmbs_ctx*, const char* seq, int32_t L, int32_t stride, int64_t n_reads,
                             const uint32_t* read_of, const uint64_t* site, int64_t n_cand,
                             uint32_t* err, int32_t* end_site);

/* K11-K13: fast_recalculate_bs_Cigar (ksw.cpp:2578) for job i = (read_of[i], site[i], end_site[i],
 * err[i]); cigar ops: max_ops per job, SAM order.                                                  */
int bmbs_align_batch(bmbs_ctx*, const char* seq, const char* qual, int32_t L, int32_t stride,
                     int64_t n_reads, const uint32_t* read_of, const uint64_t* site,
                     const int32_t* end_site_in, const uint32_t* err_in, int64_t n_jobs,
                     int32_t* start_site, int32_t* end_site, uint32_t* nm, int32_t* score,
                     uint32_t* cigar_ops, int32_t* n_ops, int32_t max_ops);

/* the same call on the form the mapping calls run: the rows are packed on the device first (as bmbs_filter_batch_packed does), the
 * un-gapped recheck and the DP kernels take the read letters from the packed words, and the form of the DP is chosen as in a
 * mapping call.  Jobs whose read index is >= rev_from read their quality row mirrored (what a mapping call does for mate 2);
 * 0xffffffff: none.  Same results as bmbs_align_batch for every input (tests/test_align_forms.py).                              */
int bmbs_align_batch_packed(bmbs_ctx*, const char* seq, const char* qual, int32_t L, int32_t stride,
                            int64_t n_reads, const uint32_t* read_of, const uint64_t* site,
                            const int32_t* end_site_in, const uint32_t* err_in, int64_t n_jobs,
                            int32_t* start_site, int32_t* end_site, uint32_t* nm, int32_t* score,
                            uint32_t* cigar_ops, int32_t* n_ops, int32_t max_ops, uint32_t rev_from);

/* K1-K6 (+a8-a10): the seeding state machine of Map_Single_Seq_end_to_end (Schema.cpp:24588-24986).
 * verdict[i]: 0 no candidate, 1 exact-unique exit (exit_site), 2 one-mismatch exit (exit_site),
 * 3 general path, 4 exact but ambiguous.  For verdict 3 the read's votes, in the reference's visiting
 * order (std::sort by vote, Schema.cpp:24986), are vote_site/vote_cnt[seg_off[i] .. seg_off[i]+n_votes[i]). */
int bmbs_seed_batch(bmbs_ctx*, const char* seq, int32_t L, int32_t stride, int64_t n_reads,
                    uint8_t* verdict, uint64_t* exit_site, uint64_t* seg_off, uint32_t* n_votes,
                    uint64_t* vote_site, uint32_t* vote_cnt, int64_t vote_cap, int64_t* total_slots);

/* Slots per read (per mate) the cigar pool of the mapping calls needs for reads of length L under these parameters (NULL: the
 * defaults): 2k + 8 with the default penalties, more when --gap_open / --gap_extension (Process_CommandLines.cpp:129-130) make
 * gaps cheaper than mismatches; -1 for L outside 1..BMBS_MAX_READ.  A pool of n_reads * bmbs_max_cigar_ops(params, L_max) entries (twice
 * that for pairs) is always enough; parameter sets that allow more than 254 operations per alignment are refused by the mapping
 * calls (BMBS_EINVAL): n_cigar of a record is 8 bits. */
int32_t bmbs_max_cigar_ops(const bmbs_params* params, int32_t L);

/* ---- fused single-end mapping (Map_Single_Seq_end_to_end loop body, Schema.cpp:24488-25119) ---- */
/* host buffers: copies in, maps, copies results out.  cigar_pool[cigar_cap] receives the ops.      */
int bmbs_map_se(bmbs_ctx*, const char* seq, const char* qual, int32_t L, int32_t stride,
                int64_t n_reads, bmbs_result* results, uint32_t* cigar_pool, int64_t cigar_cap,
                int64_t* n_cigar_used);
/* device-resident variant: d_seq/d_qual/d_results/d_cigar_pool are device addresses (e.g. from
 * torch tensors); nothing crosses PCIe; asynchronous on the ctx stream until bmbs_sync(): the input
 * buffers are read throughout the call (also by the paired-end variants) and have to stay untouched until then. */
int bmbs_map_se_device(bmbs_ctx*, uint64_t d_seq, uint64_t d_qual, int32_t L, int32_t stride,
                       int64_t n_reads, uint64_t d_results, uint64_t d_cigar_pool, int64_t cigar_cap);
int bmbs_sync(bmbs_ctx*);

/* ---- reads of different lengths in ONE batch (reads_soa.len of SURVEY.md section 8b; a trimmed library).  The reference maps
 * read by read and derives everything from current_read.length (error_threshold1 = thread_e_f * length, Schema.cpp:24546;
 * seed count L/10-1; p_length = L + 2k; MAP_Calculation over that read's threshold).  len[i] in [1, L_max], rows are still
 * `stride` bytes apart (stride >= L_max), bytes past len[i] are ignored.  The CIGAR pool reserves 2*k(L_max)+8 ops per read.
 * Paired-end: mates of one pair may have different lengths (the insert window uses the larger threshold and the longer
 * mate, Schema.cpp:18900-18935).  d_len of the device form = u16[2n]: the n first mates, then the n second mates.     */
int bmbs_map_se_var(bmbs_ctx*, const char* seq, const char* qual, const uint16_t* len, int32_t L_max, int32_t stride,
                    int64_t n_reads, bmbs_result* results, uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used);
int bmbs_map_se_var_device(bmbs_ctx*, uint64_t d_seq, uint64_t d_qual, uint64_t d_len, int32_t L_max, int32_t stride,
                           int64_t n_reads, uint64_t d_results, uint64_t d_cigar_pool, int64_t cigar_cap);
int bmbs_map_pe_var(bmbs_ctx*, const char* seq1, const char* qual1, const char* seq2, const char* qual2,
                    const uint16_t* len1, const uint16_t* len2, int32_t L_max, int32_t stride, int64_t n_pairs,
                    bmbs_result* results, uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used);
int bmbs_map_pe_var_device(bmbs_ctx*, uint64_t d_seq1, uint64_t d_qual1, uint64_t d_seq2, uint64_t d_qual2, uint64_t d_len,
                           int32_t L_max, int32_t stride, int64_t n_pairs, uint64_t d_results, uint64_t d_cigar_pool,
                           int64_t cigar_cap);

/* ---- packed reads (round 5): the same calls with 2 bits per base going over the link instead of a byte ---------------------------------
 * What the reference's reader hands a mapping thread is the upper-cased sequence line (Process_Reads.cpp:810-890; mate 2 reverse-
 * complemented, :262-267); the host-buffer entry points above move that as it is, 160 bytes of ASCII per 150-base read and mate, and are
 * bound by the link (SURVEY 8d counts H2D / D2H).  Here the caller packs the sequence once per batch (bmbs_pack_rows, a few GB/s on the
 * host's threads, or its own reader writes the format directly):
 *   row = W = ceil(L_max / 32) u64 words of bases -- base j in bits 2 (j % 32), 2 (j % 32) + 1 of word j / 32: A 0, C 1, G 2, T 3 --
 *         followed by M = ceil(L_max / 64) words of marks -- bit j % 64 of word j / 64 set: the character at j is 'N' (its base bits 0);
 *         bits at and beyond a read's length are ignored; rows `pwords` (>= W + M) words apart.  150 bases: 8 words = 64 bytes.
 * Characters other than A C G T N cannot be expressed (bmbs_pack_rows says BMBS_EINVAL and which row; the same for a length of 0 or
 * beyond L_max): such batches take the ASCII calls.  BOTH mates are given in FASTQ orientation (what bmbs_map_pe takes as seq2): the device reverse-complements mate 2 on the
 * packed words.  Qualities stay bytes (`stride` apart, as above); len NULL: every read has length L_max.  Results, CIGAR pool, errors:
 * exactly those of bmbs_map_se[_var] / bmbs_map_pe[_var] on the ASCII rows the packed ones stand for (tests/test_gpu_parity.py).     */
int bmbs_pack_rows(const char* seq, int32_t L_max, int32_t stride, int64_t n, const uint16_t* len /* NULL: uniform */, uint64_t* rows, int32_t pwords,
                   int32_t threads, int64_t* bad_row /* may be NULL */);
int bmbs_map_se_packed(bmbs_ctx*, const uint64_t* rows, int32_t pwords, const char* qual, const uint16_t* len, int32_t L_max, int32_t stride,
                       int64_t n_reads, bmbs_result* results, uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used);
int bmbs_map_pe_packed(bmbs_ctx*, const uint64_t* rows1, const uint64_t* rows2, int32_t pwords, const char* qual1, const char* qual2,
                       const uint16_t* len1, const uint16_t* len2, int32_t L_max, int32_t stride, int64_t n_pairs, bmbs_result* results,
                       uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used);

/* ---- packed quality classes: the packed calls with 4 bits per quality going over the link instead of a byte -----------------------------
 * The mapping path uses a quality byte for one thing, the mismatch penalty MismatchPenaltyByQuality gives it (ksw.h:148-161:
 * mp_min + (int)(min(Q - q_base, 40) / 40 * (mp_max - mp_min)), evaluated in double), and that function takes few distinct values: 8 over
 * the 256 bytes with the default penalties, 11 with --phred64.  So a 4-bit penalty CLASS per base carries everything a record needs, and
 * with bmbs_map_*_packed's 2-bit bases a 150-base read goes up as 64 + 80 bytes instead of 64 + 160:
 *   classes  the distinct penalties of the 256 bytes, sorted DESCENDING: class 0 is the largest penalty.  *n_classes = min(16, their number),
 *            penalty_of[c] for c < *n_classes, class_of[b] = the class of byte b, or 0xFF when b's penalty is not among the 16 largest
 *            ("cannot be packed").  With the defaults every byte has a class; every byte >= q_base has one whenever |mp_max - mp_min| <= 15;
 *            beyond that some ordinary qualities have none, and such batches take the byte calls (bmbs_map_*_packed), the rule
 *            bmbs_pack_rows has for letters outside ACGTN.  The bytes that fall off first are those far below q_base.
 *   row      Wq = ceil(L_max / 16) u64 words: the class of base j in bits 4 (j % 16) .. 4 (j % 16) + 3 of word j / 16; nibbles at and beyond a
 *            read's length are 0; rows `qwords` (>= Wq) words apart.  150 bases: 10 words = 80 bytes.  Qualities in FASTQ order for BOTH
 *            mates, exactly what the byte calls take.
 * bmbs_pack_quals packs a batch on the host's threads and needs no device (BMBS_EINVAL and *bad_row = the first row with a byte that has no
 * class, or a length of 0 or beyond L_max).  The caller packs with the SAME mp_max / mp_min / q_base the context was created with: a class
 * number means a penalty only under those.  The device writes, once per chunk, the byte rows its kernels have always read (k_qual_expand:
 * for class c the smallest byte with that penalty), so results, CIGAR pool, n_cigar_used, statistics, counters and errors are exactly those
 * of bmbs_map_{se,pe}_packed on the quality bytes the classes stand for (tests/test_packed_quals.py).  A context whose parameters leave
 * some bytes without a class still serves these calls.  The records do not carry QUAL: SAM's QUAL text is written by the caller from its
 * own FASTQ line, as for every record-level call; the text calls (bmbs_map_*_text), which print it, keep their bytes.                  */
int bmbs_qual_classes(const bmbs_params* params /* NULL: defaults */, uint8_t class_of[256], int32_t penalty_of[16], int32_t* n_classes);
int bmbs_pack_quals(const bmbs_params* params /* NULL: defaults */, const char* qual, int32_t L_max, int32_t stride, int64_t n,
                    const uint16_t* len /* NULL: uniform */, uint64_t* qrows, int32_t qwords, int32_t threads, int64_t* bad_row /* may be NULL */);
int bmbs_map_se_packedq(bmbs_ctx*, const uint64_t* rows, int32_t pwords, const uint64_t* qrows, int32_t qwords, const uint16_t* len, int32_t L_max,
                        int64_t n_reads, bmbs_result* results, uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used);
int bmbs_map_pe_packedq(bmbs_ctx*, const uint64_t* rows1, const uint64_t* rows2, int32_t pwords, const uint64_t* qrows1, const uint64_t* qrows2,
                        int32_t qwords, const uint16_t* len1, const uint16_t* len2, int32_t L_max, int64_t n_pairs, bmbs_result* results,
                        uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used);

/* ---- fused paired-end mapping, default (fast) mode: Map_Pair_Seq_end_to_end_fast (Schema.cpp:18570-19546)
 * = get_candidates x2 (18172), filter_pairs (16052), verify_candidate_locations (18130) on the smaller side,
 * filter_pairs_single_side (16186), new_faster_verify_pairs (15773), calculate_best_map_cigar_end_to_end_return
 * (14602), TLEN / insert / chromosome-end checks and MAPQ over k1+k2 (19400-19440).
 * seq2/qual2 = mate 2 exactly as in the FASTQ file (the library builds the reverse complement the reference's
 * reader builds, Process_Reads.cpp:262-267).  Both mates have length L.  results[2*i], results[2*i+1] = mate 1,
 * mate 2 of pair i: flag 99/83 and 147/163, `tlen` = |TLEN|, status BMBS_ST_* for the PAIR
 * (BMBS_ST_OFFEND also covers the insert-size rejection).  Stats count pairs (Schema.cpp:19531-19537).
 * With bmbs_params.sensitive = 1 the same entry points run --sensitive: Map_Pair_Seq_end_to_end (Schema.cpp:19953-21459)
 * = first seeds of both mates, process_rest_seed_debug (17574) on the mate with fewer first-seed candidates,
 * process_rest_seed_filter_debug (16298) on the other, reseed_filter / select_best_seeds (16678 / 16630) for a mate
 * left without a hit, then the same pairing and post-processing.                                          */
int bmbs_map_pe(bmbs_ctx*, const char* seq1, const char* qual1, const char* seq2, const char* qual2, int32_t L,
                int32_t stride, int64_t n_pairs, bmbs_result* results, uint32_t* cigar_pool, int64_t cigar_cap,
                int64_t* n_cigar_used);
int bmbs_map_pe_device(bmbs_ctx*, uint64_t d_seq1, uint64_t d_qual1, uint64_t d_seq2, uint64_t d_qual2, int32_t L,
                       int32_t stride, int64_t n_pairs, uint64_t d_results, uint64_t d_cigar_pool, int64_t cigar_cap);

/* ---- FASTQ text in: the reads are cut out of the text ON THE DEVICE -------------------------------------------------------------
 * What the reference's reader does per record on one host thread (inputReads_single_directly / inputReads_paired_directly,
 * Process_Reads.cpp:810-890, 155-317: kseq line splitting, toupper, `qual.resize(seq.size(), ' ')`, the reverse complement of
 * mate 2 at :262-267 and of every --pbat read with mirrored qualities at :986-1075) is done by one kernel over the batch; the host
 * hands over the text window as it came from the file plus the line starts it found.  A window is smaller than 4 GiB.
 * Records keep their own lengths (1..L_max, L_max <= BMBS_MAX_READ); `uniform` != 0 promises that every read has length L_max (the
 * fixed-length kernels are used).  results / cigar_pool as for bmbs_map_se / bmbs_map_pe.  Page-locked text buffers
 * (bmbs_host_alloc) are copied at link speed.                                                                                  */
typedef struct bmbs_fastq_view {
    const char*     text;        /* FASTQ text window (host memory)                                                   */
    uint64_t        text_bytes;
    const uint32_t* seq_off;     /* [n] offset of the first base of record i                                          */
    const uint32_t* qual_off;    /* [n] offset of its first quality character                                         */
    const uint16_t* seq_len;     /* [n] bases of record i                                                             */
    const uint16_t* qual_len;    /* [n] quality characters present (a shorter line is padded with ' ')                */
} bmbs_fastq_view;
int bmbs_map_se_fastq(bmbs_ctx*, const bmbs_fastq_view* reads, int64_t n_reads, int32_t L_max, int32_t uniform, int32_t pbat,
                      bmbs_result* results, uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used);
int bmbs_map_pe_fastq(bmbs_ctx*, const bmbs_fastq_view* mate1, const bmbs_fastq_view* mate2, int64_t n_pairs, int32_t L_max,
                      int32_t uniform, bmbs_result* results, uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used);

/* ---- FASTQ text in, SAM text out: both ends of the file-to-file path on the device -------------------------------------------------
 * The reference's reader and its SAM sink are one host thread each (Process_Reads.cpp:2057-2260, Process_sam_out.cpp:954-1006) and
 * bound the whole program.  Here the host hands over the text window exactly as it came from the file(s) together with the number
 * of complete records it holds (it only has to count newlines), and gets the finished SAM lines of those records back: the
 * newline index, the read rows, the mapping and the formatting of output_sam_end_to_end / directly_output_read1 / _read2 /
 * output_sam_unmapped / directly_output_unmapped_PE (Schema.cpp:11989-12039, 10537-10640, 11494-11590, 23955-23975, 10392-10430)
 * all happen on the device; QNAME, SEQ and QUAL are taken from the FASTQ text that is resident there anyway.
 * text = n_records * 4 lines (a window may hold more: the rest is ignored); paired end: record i of text1 and of text2 are a pair.
 * sam receives the lines in input order, *sam_bytes their total size; BMBS_ENOMEM with *sam_bytes = the size needed when sam_cap is
 * too small.  Page-locked buffers (bmbs_host_alloc) move at link speed.  bmbs_sam_refs sets the RNAME strings (the names of the
 * index's sequences, in index order: bmbs_index_file_chrom_name) once per context.                                           */
#define BMBS_TEXT_PBAT      1   /* single end --pbat: reads are mapped as their reverse complement (Process_Reads.cpp:986-1075)   */
#define BMBS_TEXT_UNMAPPED  2   /* --unmapped_out: unmapped reads / pairs are printed with flag 4 / 77 + 141                      */
#define BMBS_TEXT_BAM      16   /* --bam: `sam` receives the batch's records as BAM inside complete BGZF blocks (a piece of a .bam file
                                 * behind its header) instead of SAM text: what the reference gets from htslib's sam_parse1 + bam_write1
                                 * per line (bam_prase.cpp:201-221), built and deflated on the device; the INFLATED bytes are the
                                 * reference's, block boundaries and compressed bytes are not.  *sam_bytes = compressed bytes        */
#define BMBS_TEXT_BAM_SORTED 32 /* --bam --sort, only together with BMBS_TEXT_BAM (BMBS_EINVAL otherwise): `sam` receives the batch's
                                 * UNCOMPRESSED BAM records, stably sorted by the coordinate key below (equal keys keep the order the
                                 * unsorted call gives them); *sam_bytes = their size; BMBS_ENOMEM as above.  The records are sorted on
                                 * the device (csrc/k_bamsort.hip); a driver merges batches with bmbs_bam_sort                       */
int bmbs_sam_refs(bmbs_ctx*, const char* const* names, int32_t n_names);
int bmbs_map_se_text(bmbs_ctx*, const char* text, uint64_t text_bytes, int64_t n_records, int32_t flags,
                     char* sam, uint64_t sam_cap, uint64_t* sam_bytes, int64_t* n_lines);
int bmbs_map_pe_text(bmbs_ctx*, const char* text1, uint64_t bytes1, const char* text2, uint64_t bytes2, int64_t n_pairs, int32_t flags,
                     char* sam, uint64_t sam_cap, uint64_t* sam_bytes, int64_t* n_lines);

/* ---- bgzip'ed FASTQ inflated on the device -------------------------------------------------------------------------------------------
 * The reference reads .gz input through zlib's gzread on its reader thread (Process_Reads.cpp:1455-1514).  A BGZF file (bgzip) is a
 * series of independent gzip members of at most 64 KiB of text whose compressed size stands in the header: a window of them is
 * inflated here by one wave per block, CRC-32 and ISIZE of every block checked.  comp = the bytes of n_blocks consecutive blocks
 * (block i at comp + blk_off[i], blk_off[n_blocks] = their end), text receives block i's bytes at text + out_off[i]
 * (out_off[i + 1] - out_off[i] = the ISIZE in block i's trailer).  Needs no index.  BMBS_EINVAL (bmbs_last_error says which
 * block) for anything zlib's inflate would refuse or a CRC that does not match.  Page-locked `text` moves at link speed.
 * nl_per_64k (optional): what the driver's reader would otherwise count on the host -- the newlines of the inflated text per 64 KiB
 * of the caller's WINDOW, in which text byte i sits at offset window_shift + i: nl_per_64k[j] = newlines among the bytes at window
 * offsets [j * 65536, (j + 1) * 65536); (window_shift + text length + 65535) / 65536 entries.                                  */
int bmbs_inflate_bgzf(bmbs_ctx*, const void* comp, uint64_t comp_bytes, const uint64_t* blk_off, const uint64_t* out_off, int64_t n_blocks,
                      char* text, uint64_t text_bytes, uint32_t* nl_per_64k, uint64_t window_shift);

/* ... and the same blocks as the INPUT of a text call, so that the inflated text never leaves the device.  Two phases, because a
 * reader has to know what a window left over before it can cut the next one:
 *   bmbs_text_open_bgzf   the window(s) are assembled on the device -- `prefix` (uncompressed bytes: what the previous window left
 *                         over) followed by the text of the blocks --, their lines are indexed, *n_records = the complete records
 *                         (pairs: of both mates) they hold, at most max_records; tail1 / tail2 receive the text BEHIND those records
 *                         (the next window's prefix; BMBS_ENOMEM with *tail_bytes = the size needed when tail_cap is too small);
 *                         last1 / last2: the window ends its file (an unterminated last line is closed, as the reader does)
 *   bmbs_text_map_open    maps the open batch: records / SAM text / BAM blocks exactly as bmbs_map_*_text returns them
 * The context holds one open batch at a time.                                                                                    */
typedef struct bmbs_ztext {
    const char*     prefix;        /* host; NULL when prefix_bytes == 0 */
    uint64_t        prefix_bytes;
    const void*     comp;          /* the bytes of n_blocks consecutive BGZF blocks (page-locked memory moves at link speed) */
    uint64_t        comp_bytes;
    const uint64_t* blk_off;       /* [n_blocks + 1] */
    const uint64_t* out_off;       /* [n_blocks + 1]: ISIZE prefix sums */
    int64_t         n_blocks;      /* may be 0 (a window made of the prefix alone) */
} bmbs_ztext;
int bmbs_text_open_bgzf(bmbs_ctx*, const bmbs_ztext* mate1, const bmbs_ztext* mate2 /* NULL: single end */, int64_t max_records,
                        int32_t last1, int32_t last2, int64_t* n_records, char* tail1, uint64_t tail_cap, uint64_t* tail1_bytes,
                        char* tail2, uint64_t* tail2_bytes);
/* (An ordinary .gz file -- ONE deflate stream per member -- is inflated by the driver's block-parallel host inflater, csrc/pgz.h.  Round 4
 * also carried a device form of that scheme, bmbs_inflate_gzip / bmbs_text_open_gzip: exact, and slower than the host's; removed in round 5.) */
int bmbs_text_map_open(bmbs_ctx*, int32_t flags, char* sam, uint64_t sam_cap, uint64_t* sam_bytes, int64_t* n_lines);

/* ---- adapter and quality trimming of the reads of a text call, on the device (csrc/k_trim.hip; bmbs_search --trim) ------------------
 * What a pipeline otherwise runs trim_galore / cutadapt for before it maps.  bmbs_set_trim turns it on for the text calls of the context
 * (bmbs_map_se_text, bmbs_map_pe_text, bmbs_text_map_open; NULL turns it off): every record of a batch is trimmed behind the line index,
 * templates that end up too short are dropped, and the rows, the mapping, the statistics, the SAM / BAM records, the sort and everything
 * that describes the last sorted call (bmbs_text_sorted_index / _dup / _clip / _nonconv) see the remaining batch: the output is byte for
 * byte what the same call without trimming gives on a FASTQ text from which a host trimmer following the rule below removed and
 * shortened those records.  *n_lines counts the remaining templates' lines.  A batch that bmbs_text_open_bgzf opened while trimming was
 * off cannot be mapped with it on (BMBS_ESTATE: the window's buffer is sized when it is opened): bmbs_set_trim comes first.  The calls whose caller owns the read lengths (the row,
 * packed and bmbs_map_*_fastq calls) are not touched.  M-bias cycles and methylation read-end trimming count from the trimmed read's
 * first base, as Bismark's do behind trim_galore.
 * The rule, for a record of mate m (0 / 1) with L sequence characters (exact integer arithmetic; bases are upper-cased for comparison
 * only, a quality character missing from a short quality line counts as ' '); the steps in this order:
 *   1. quality (quality = c > 0; cutadapt -q, the BWA rule, 3' end only): s = 0, best = 0, stop = L; for i = L-1 down to 0:
 *      s += c - (q[i] - q_base); if s < 0 stop looking; if s > best { best = s; stop = i }.  L = stop.  q_base: bmbs_params.q_base
 *   2. 3' adapter (adapter[m] = 1..32 letters of ACGT; empty: no adapter step for that mate): a start i in [0, L) has the overlap
 *      o = min(|A|, L - i) and mm = the number of j < o with upper(s[i + j]) != A[j] (a read's N matches nothing); it is accepted iff
 *      o >= min_overlap and mm <= o * error_permille / 1000 (integer division).  L = the SMALLEST accepted i.
 *      Not cutadapt's choice: cutadapt takes the best-scoring alignment and allows indels by default; here it is the leftmost
 *      accepted start, without indels
 *   3. fixed clips: L -= min(L, clip_3p[m]); k = min(L, clip_5p[m]): both lines begin k characters later, L -= k, and the quality
 *      line keeps clamp(qual_len - k, 0, L) characters
 *   4. length filter (trim_galore --length without --retain_unpaired; min_length >= 1): a single-end record with L < min_length is
 *      dropped, a pair when either mate is
 * Not done: adapter auto-detection, 5' and anchored adapters, indels, --nextseq poly-G trimming, RRBS's two extra bases,
 * --retain_unpaired, writing trimmed FASTQ files.
 * BMBS_EINVAL (bmbs_last_error says why): an adapter letter outside ACGT (lower case is accepted), an adapter of more than 32 letters,
 * min_length < 1, error_permille outside 0..1000, a negative value, quality above 255 or a clip above 65535.                       */
typedef struct bmbs_trim_opts {
    int32_t quality, min_overlap, error_permille, min_length;
    int32_t clip_5p[2], clip_3p[2];
    char    adapter[2][33];        /* NUL-terminated */
} bmbs_trim_opts;
/* what the trim stage of the context's last text call did, per mate: the records it saw and their bases, the records each step
 * shortened and by how many bases, the bases of the records that stayed; and the templates the length filter dropped.  The counters
 * belong to the call, not to the running statistics: a call repeated after BMBS_ENOMEM counts anew.                                 */
typedef struct bmbs_trim_counts {
    int64_t records_in[2], bases_in[2], bases_out[2];
    int64_t quality_records[2], quality_bases[2], adapter_records[2], adapter_bases[2], clip_records[2], clip_bases[2];
    int64_t templates_dropped;
} bmbs_trim_counts;
int bmbs_set_trim(bmbs_ctx*, const bmbs_trim_opts* opts /* NULL: off */);
/* *n_kept = the templates of that call that stayed.  BMBS_ESTATE when the context has made no text call or trimming was off in it. */
int bmbs_text_trim_counts(bmbs_ctx*, bmbs_trim_counts* counts, int64_t* n_kept);
/* The stage alone: the four fields of every record of `text` (n_records * 4 lines, read as mate `mate`) after steps 1-3 and BEFORE the
 * filter -- a length of 0 is allowed here.  Needs no attached index; BMBS_ESTATE when trimming is off.                              */
int bmbs_trim_text(bmbs_ctx*, const char* text, uint64_t text_bytes, int64_t n_records, int32_t mate, uint32_t* seq_off,
                   uint32_t* qual_off, uint16_t* seq_len, uint16_t* qual_len);

/* ---- coordinate-sorted BAM: the records are sorted on the device (csrc/k_bamsort.hip) ---------------------------------------------------
 * The sort key of a BAM record -- refID = the int32 at byte 4 of the record (counting its block_size word), pos = the int32 at byte 8,
 * flag = the uint16 at byte 18 -- is
 *     key = (uint64)(uint32)refID << 32  |  (uint64)(uint32)(pos + 1) << 1  |  ((flag >> 4) & 1)
 * reference index, position, strand: coordinate order; refID -1 sorts last, pos -1 gives 0.  Every sort here is STABLE: records with
 * equal keys keep their input order.
 * bmbs_text_sorted_index: key and byte length of each record the context's last BMBS_TEXT_BAM_SORTED call returned, in the order
 * returned; *n = their number (BMBS_ENOMEM with *n set when cap is smaller; BMBS_ESTATE when there was no such call).  A driver cuts a
 * batch at coordinate boundaries with a binary search over `key`.
 * bmbs_bam_sort: `records` = n concatenated BAM records in host memory (input order), len[i] = their sizes (block_size + 4 each);
 * `out` receives the same records stably sorted by key -- as complete BGZF blocks of 0xff00 input bytes (the call's last block
 * shorter), or uncompressed with BMBS_BAMSORT_RAW; *out_bytes = the bytes written.  Needs no attached index.  BMBS_ENOMEM with
 * *out_bytes = the size needed when out_cap is too small; BMBS_EINVAL (bmbs_last_error names the record) when a len[i] disagrees with
 * its record's block_size or is below 36, or when sum(len) != bytes; n = 0 is valid (0 bytes).  Page-locked buffers move at link speed;
 * the upload takes its turn on the device's upload mutex like every host call.                                                    */
#define BMBS_BAMSORT_RAW 1
int bmbs_text_sorted_index(bmbs_ctx*, uint64_t* key, uint32_t* len, int64_t cap, int64_t* n);
int bmbs_bam_sort(bmbs_ctx*, const char* records, uint64_t bytes, const uint32_t* len, int64_t n, int32_t flags, char* out,
                  uint64_t out_cap, uint64_t* out_bytes);

/* ---- the .bai index of a sorted BAM (SAM specification section 5.2; csrc/k_bai.hip) -----------------------------------------------------
 * bmbs_bam_sort_index describes the output of the context's last successful bmbs_bam_sort call that returned BGZF blocks, computed on
 * the device from the buffers that call left there (bmbs_bam_sort itself does nothing for it).  BMBS_ESTATE: there was no such call,
 * it used BMBS_BAMSORT_RAW, or another call on the context has used the buffers since.  BMBS_ENOMEM when a cap is too small; *n_chunk,
 * *n_win and *n_ref are set then too (caps of 0: the size query).
 * Virtual offsets are relative to the first byte of that call's `out`: the byte at offset u of the uncompressed stream is
 * (compressed offset of block u / 0xff00) << 16 | u % 0xff00; u = the stream's size gives (compressed bytes of the call) << 16, the
 * first byte behind the call.  A driver that has put the call's blocks at file offset B adds B << 16 to every offset (exact).
 * Per record, in sorted order: beg = pos (a pos below 0 counts as 0, as in hts_idx_push), end = pos + the reference length of its
 * CIGAR (M D N = X), pos + 1 when flag 4 is set, n_cigar_op is 0 or that length is 0; bin = reg2bin(beg, end) (section 5.3).
 * Records with refID -1 are counted in *n_no_coor and appear nowhere else.  A record with refID >= 0 and end > 2^29 gives BMBS_EINVAL
 * (bmbs_last_error names it: BAI cannot hold it; CSI is not written).
 *   chunk  one entry per maximal run of consecutive records with equal (ref, bin), mapped or not: beg = the offset of the run's first
 *          record, end = that of the record behind the run (or the first byte behind the call); ordered by (ref, bin, beg)
 *   win    one entry per (ref, 16 kb window) that a MAPPED record overlaps (windows beg >> 14 .. (end - 1) >> 14): off = the smallest
 *          offset among those records; ordered by (ref, win); no fill
 *   ref    one entry per refID >= 0 that has records, ordered by ref: beg / end = the offset of its first record / just behind its
 *          last, n_mapped / n_unmapped = its records by flag 4                                                                    */
typedef struct bmbs_bai_chunk { int32_t ref; uint32_t bin; uint64_t beg, end; } bmbs_bai_chunk;
typedef struct bmbs_bai_win   { int32_t ref; uint32_t win; uint64_t off; } bmbs_bai_win;
typedef struct bmbs_bai_ref   { int32_t ref; uint32_t pad; uint64_t beg, end, n_mapped, n_unmapped; } bmbs_bai_ref;
int bmbs_bam_sort_index(bmbs_ctx*, bmbs_bai_chunk* chunk, int64_t chunk_cap, int64_t* n_chunk, bmbs_bai_win* win, int64_t win_cap,
                        int64_t* n_win, bmbs_bai_ref* ref, int64_t ref_cap, int64_t* n_ref, uint64_t* n_no_coor);

/* ---- PCR duplicates of a sorted BAM, marked on the device (csrc/k_markdup.hip; `bmbs_search --bam --sort --markdup`) ---------------------
 * Picard's pair-level rule, per TEMPLATE: one record of a single-end run, the two records of a pair.  A record is USABLE when it is
 * there, mapped (flag 4 clear), primary (0x100 and 0x800 clear) and has n_cigar_op > 0.  Its 5' coordinate: forward strand pos - (the
 * leading S and H lengths), reverse strand (flag 0x10) pos + (the sum of its M D N = X lengths) + (the trailing S and H lengths) - 1.
 *   both records of a pair usable: the two ends (refID, 5' coordinate, strand, is read 1 = flag 0x40); lo = the smaller by (refID,
 *     coordinate), a tie goes to the forward strand, a further tie to read 1; (ref_lo, pos_lo), (ref_hi, pos_hi) = the two ends,
 *     orient = strand of lo | strand of hi << 1 | (lo is read 1) << 2 | 8
 *   a single-end record, or the one usable record of a pair: (ref_lo, pos_lo) = its end, (ref_hi, pos_hi) = (-1, -1), orient = strand
 *   no usable record: every coordinate -1, orient = BMBS_DUP_NONE, score 0; such a template is never marked
 * Bit 2 of orient is ALWAYS part of the signature (Picard uses it for FF and RR pairs only): read 1 forward and read 1 reverse come
 * from different original strands of a bisulfite library and are never copies of one molecule.
 * score = the sum, over the usable records, of the base qualities that are >= 15 (a quality byte 0xff counts as 0).
 * Among templates with equal (ref_lo, pos_lo, ref_hi, pos_hi, orient) the one with the highest score stays, among equal scores the
 * earliest in input order; every other one is a duplicate.  A caller marks a duplicate by `flag |= 0x400` in EVERY record of the
 * template, which is one byte: record byte 19 (counting the block_size word) |= 0x04 -- its step when it stages records for
 * bmbs_bam_sort; nothing else in a record changes.
 * bmbs_bam_dup_sigs: `records` = n entries in host memory (input order), len[i] = their sizes; len[i] == 0: no record here (the text
 * calls' empty lines).  paired != 0: entries 2p and 2p + 1 are one template (n must be even).  sig[t] = template t; *n_sig = their
 * number (BMBS_ENOMEM with *n_sig set when sig_cap is smaller; a cap of 0: the size query).  Needs no attached index.  BMBS_EINVAL
 * (bmbs_last_error names the record) as for bmbs_bam_sort: a len[i] other than 0 below 36 or unlike its record's block_size + 4,
 * sum(len) != bytes, an odd n with `paired`; also a record whose read name, CIGAR, sequence and qualities do not fit its length.
 * bmbs_text_sorted_dup: the same for the context's last BMBS_TEXT_BAM_SORTED call, computed when asked for from the buffers that call
 * left on the device, where the two records of a pair still lie side by side.  sig[t] = template t of the batch in batch order
 * (*n_sig = the records / pairs handed to the call); tmpl[j] = the template of the j-th record the call returned, in sorted order
 * (*n = their number, that of bmbs_text_sorted_index).  BMBS_ESTATE: there was no such call, or another call on the context has
 * rewritten the buffers since; BMBS_ENOMEM when a cap is too small, *n_sig and *n are set then too (caps of 0: the size query).
 * bmbs_dup_select: dup[i] = 1 when template i loses its group, 0 otherwise; *n_dup = their number; the index is the input order;
 * n = 0 is valid.  The result for a template depends only on the templates of its group, so a caller may run it on any partition of
 * the templates by a function of (ref_lo, pos_lo), each part in input order.  Needs no attached index.                            */
typedef struct bmbs_dup_sig { int32_t ref_lo, pos_lo, ref_hi, pos_hi; uint32_t orient, score; } bmbs_dup_sig;   /* 24 bytes */
#define BMBS_DUP_NONE 0x80000000u      /* in orient: the template has no signature */
int bmbs_bam_dup_sigs(bmbs_ctx*, const char* records, uint64_t bytes, const uint32_t* len, int64_t n, int32_t paired,
                      bmbs_dup_sig* sig, int64_t sig_cap, int64_t* n_sig);
int bmbs_text_sorted_dup(bmbs_ctx*, bmbs_dup_sig* sig, int64_t sig_cap, int64_t* n_sig, uint32_t* tmpl, int64_t cap, int64_t* n);
int bmbs_dup_select(bmbs_ctx*, const bmbs_dup_sig* sig, int64_t n, uint8_t* dup, int64_t* n_dup);

/* ---- methylation counts per cytosine from BAM records, on the device (csrc/k_methyl.hip; `bmbs_search --bam --sort --methyl`) ---------------
 * The genome is the attached index's (two bits a base; a non-ACGT base of the FASTA is whatever letter the index holds for it), refID its
 * sequence number.  Contexts are defined on the genome alone.  A forward-strand C at p: CpG if p + 1 is inside the sequence and is G,
 * otherwise CHG if p + 2 is inside and is G, otherwise CHH if p + 2 is inside, otherwise none.  A G at p (a cytosine of the reverse
 * strand), mirrored: CpG if p - 1 is inside and is C, otherwise CHG if p - 2 is inside and is C, otherwise CHH if p - 2 is inside.
 * A record COUNTS when refID >= 0, flag 4 is clear, flag & 0xF00 == 0 (MethylDackel's default: no secondary, QC-fail, duplicate or
 * supplementary record), n_cigar_op > 0, MAPQ >= min_mapq, and flag 0x2 is set if flag 0x1 is.  Its strand comes from the flags alone:
 * paired -- read 1 reverse or read 2 forward is OB, otherwise OT; single -- reverse is OB, otherwise OT.
 * The CIGAR pairs read bases with reference positions (M = X; I S consume the read, D N the reference, H P nothing).  An OT record is
 * called at forward-strand C of a selected context: read base C is methylated, T unmethylated, anything else nothing; an OB record at
 * forward-strand G: G methylated, A unmethylated.  A call counts when the base quality is >= min_phred (a quality byte 0xff is 0).
 * clip[i] (mate overlap, Bismark's --no_overlap): record i is not called at the reference positions pos + (clip >> 16) ..
 * pos + (clip >> 16) + (clip & 0xffff) - 1.  bmbs_text_sorted_clip computes it for the records of the context's last
 * BMBS_TEXT_BAM_SORTED call while the two records of a pair (output lines 2p, 2p + 1) still lie side by side: for a read-2 record
 * (flag 0x80) whose mate and itself are there, mapped, have a CIGAR and share refID, (beg - pos) << 16 | (end - beg) with [beg, end) the
 * intersection of the two reference spans; 0 for every other record.  clip[j] belongs to the j-th record the call returned (*n = that
 * of bmbs_text_sorted_index); BMBS_ESTATE / BMBS_ENOMEM as for bmbs_text_sorted_dup; BMBS_EINVAL: an offset or length of 65536 and more.
 * bmbs_bam_methyl: `records` = n entries in host memory, len[i] their sizes (0: no record here), clip in the same order or NULL.
 * bmbs_bam_sort_methyl: the same for the records of the context's last bmbs_bam_sort call, which are still on the device, clip in THAT
 * call's input order (BMBS_BAMSORT_RAW or not).  Both leave one site per (ref, pos) of a selected context with meth + unmeth > 0 on the
 * device, ordered by (ref, pos), *n_site of them; bmbs_methyl_sites fetches the last result (BMBS_ENOMEM with *n set when cap is
 * smaller; a cap of 0: the size query).  params NULL: CpG, MAPQ 10, quality 5.
 * BMBS_ESTATE: no index attached; bmbs_bam_sort_methyl: no bmbs_bam_sort call's records are resident (none yet, it failed or had no
 * records), or another call has used its buffers since.  BMBS_EINVAL (bmbs_last_error names the record): the length checks of
 * bmbs_bam_dup_sigs, a refID beyond the index's sequences, a mapped record with a CIGAR whose reference span runs off its sequence.
 * n = 0 is valid.
 *
 * Read-end trimming and the M-bias table (bmbs_bam_methyl_opts, bmbs_bam_sort_methyl_opts, bmbs_methyl_mbias; tests/mbias_spec.py).
 * The CYCLE of a call is the 0-based position of the called read base in sequencing order: with ri the base's index in SEQ as the
 * record stores it (soft-clipped and inserted bases count; H and P are not part of SEQ and shift nothing), cycle = ri for a forward
 * record and l_seq - 1 - ri for a record with flag 0x10.  The MATE of a record is 1 when flags 0x1 and 0x80 are both set (read 2 of a
 * pair), else 0 (single end, read 1, no read number).  A call of a record of mate m counts towards the sites iff
 * ignore_5p[m] <= cycle < l_seq - ignore_3p[m] (Bismark's --ignore, --ignore_3prime, --ignore_r2, --ignore_3prime_r2; each 0..65535;
 * all zero: no trim).  A record all of whose cycles are ignored contributes nothing and is no error.  The mate-overlap clip stays
 * geometric and does not look at the trim: read 2 is still clipped where read 1 covers a position, even if read 1's call there was
 * trimmed away (Bismark does the same).
 * flags & BMBS_METHYL_MBIAS: the call also leaves uint64 table[2 mate][2 strand (0 OT, 1 OB)][3 context][2 (0 unmethylated,
 * 1 methylated)][BMBS_MBIAS_CYCLES] on the device, which counts every call that passes every filter EXCEPT the trim (record flags,
 * MAPQ, proper pair, base quality, selected contexts, overlap clip): one run gives the untrimmed curve and the trimmed sites.  Calls at
 * cycle >= BMBS_MBIAS_CYCLES are tallied in the last bin (the trim still uses the true cycle); rows of contexts that are not selected
 * stay zero; n = 0 leaves an all-zero table.  The table is made from the index's genome: calls at bases the FASTA does not spell A, C,
 * G or T, where the index holds a pseudo-random letter, are in it (bmbs_search filters their SITES out of the bedGraph, not the table).
 * bmbs_methyl_mbias fetches the table of the context's last methylation call: *n = 24 * BMBS_MBIAS_CYCLES; BMBS_ESTATE if that call
 * did not set BMBS_METHYL_MBIAS, failed, or there was none; BMBS_ENOMEM with *n set when cap (entries) is smaller, a cap of 0 being
 * the size query.  BMBS_EINVAL ("bad parameters") for unknown flags bits or an ignore value outside 0..65535.
 * bmbs_bam_methyl / bmbs_bam_sort_methyl are the _opts calls with flags 0 and no trim.                                           */
#define BMBS_MBIAS_CYCLES 1024
#define BMBS_METHYL_MBIAS 1            /* in bmbs_methyl_opts.flags */
typedef struct bmbs_methyl_params { int32_t contexts /* 1 CpG | 2 CHG | 4 CHH */, min_mapq, min_phred, reserved; } bmbs_methyl_params;
typedef struct bmbs_methyl_opts   { int32_t contexts, min_mapq, min_phred, flags; int32_t ignore_5p[2], ignore_3p[2]; } bmbs_methyl_opts;   /* 32 bytes */
typedef struct bmbs_methyl_site   { int32_t ref, pos; uint32_t meth, unmeth, kind /* context 0..2 | strand << 2 */, pad; } bmbs_methyl_site;   /* 24 bytes */
int bmbs_text_sorted_clip(bmbs_ctx*, uint32_t* clip, int64_t cap, int64_t* n);
int bmbs_bam_methyl(bmbs_ctx*, const char* records, uint64_t bytes, const uint32_t* len, int64_t n, const uint32_t* clip,
                    const bmbs_methyl_params* params, int64_t* n_site);
int bmbs_bam_sort_methyl(bmbs_ctx*, const uint32_t* clip, const bmbs_methyl_params* params, int64_t* n_site);
int bmbs_bam_methyl_opts(bmbs_ctx*, const char* records, uint64_t bytes, const uint32_t* len, int64_t n, const uint32_t* clip,
                         const bmbs_methyl_opts* opts, int64_t* n_site);
int bmbs_bam_sort_methyl_opts(bmbs_ctx*, const uint32_t* clip, const bmbs_methyl_opts* opts, int64_t* n_site);
int bmbs_methyl_sites(bmbs_ctx*, bmbs_methyl_site* site, int64_t cap, int64_t* n);
int bmbs_methyl_mbias(bmbs_ctx*, uint64_t* table, int64_t cap, int64_t* n);

/* ---- the opposite strand: what tells a C->T polymorphism of the sample from an unmethylated cytosine (tests/variant_spec.py) --------------
 * On the reads of its own bisulfite strand a C->T variant looks like an unmethylated C; the reads of the OTHER strand show the position
 * unconverted, so only they can tell the two apart (MethylDackel's --minOppositeDepth / --maxVariantFrac).
 * The opposite-strand OBSERVATION.  Every record that COUNTS under the rule above (flags, n_cigar_op > 0, MAPQ >= min_mapq, proper pair
 * when paired) is walked with the same CIGAR pairing (M = X).  An OB record is looked at where the genome has a forward C of a selected
 * context, an OT record where it has a forward G of a selected context: the positions the other strand's records are called at.  A read
 * base passes exactly the filters a call passes: quality >= min_phred (0xff counts as 0), not inside the record's mate-overlap clip,
 * ignore_5p[m] <= cycle < l_seq - ignore_3p[m].  Its BAM code against the genome's base there (C = 2, G = 4): equal -- a MATCH; one of
 * the other three of {1, 2, 4, 8} -- a VARIANT; any other code (=, N, the ambiguity codes) -- nothing.
 * bmbs_bam_methyl_opposite / bmbs_bam_sort_methyl_opposite (the records as for bmbs_bam_methyl_opts / bmbs_bam_sort_methyl_opts; the
 * latter works on the records of the context's last bmbs_bam_sort call, directly before or behind a bmbs_bam_sort_methyl[_opts] call on
 * the same records as well) leave one entry per (ref, pos) with match + variant > 0 on the device, ordered by (ref, pos), *n_entry of
 * them, as bmbs_methyl_site: meth = the VARIANT count, unmeth = the MATCH count (each saturates at 2^32 - 1), kind = context |
 * strand << 2 of the cytosine at that position (strand 0 where an OB record was looked at), pad = 0.  opts NULL: the defaults (CpG,
 * MAPQ 10, quality 5, no trim); opts->flags must be 0 (BMBS_METHYL_MBIAS there: BMBS_EINVAL); every other check and error is that of
 * bmbs_bam_methyl_opts; n = 0 is valid.  A context holds ONE methylation result at a time: an opposite call ends the sites and table of
 * the call before it, a bmbs_bam_methyl* / bmbs_bam_sort_methyl* call ends the entries.  bmbs_methyl_opposite fetches the entries
 * (BMBS_ENOMEM with *n set when cap is smaller; a cap of 0: the size query); it and bmbs_methyl_sites return BMBS_ESTATE, and say so,
 * when the context's last methylation call was of the other kind.
 * The FILTER (bmbs_methyl_drop_variants: host only -- no context, no device).  site[0 .. n_site) and opp[0 .. n_opp) are ordered by
 * (ref, pos), each position once.  A site is dropped iff an entry of opp has its (ref, pos) with match + variant >= min_opposite_depth and
 * variant * 1000000 > max_variant_ppm * (match + variant) (strict, in 64 bits).  A site without an entry is kept; an entry without a
 * site does nothing.  `site` is compacted in place, *n_kept = what is left.  BMBS_EINVAL: a list out of order, min_opposite_depth < 1,
 * max_variant_ppm outside 0..1000000, a NULL argument.                                                                            */
int bmbs_bam_methyl_opposite(bmbs_ctx*, const char* records, uint64_t bytes, const uint32_t* len, int64_t n, const uint32_t* clip,
                             const bmbs_methyl_opts* opts, int64_t* n_entry);
int bmbs_bam_sort_methyl_opposite(bmbs_ctx*, const uint32_t* clip, const bmbs_methyl_opts* opts, int64_t* n_entry);
int bmbs_methyl_opposite(bmbs_ctx*, bmbs_methyl_site* entry, int64_t cap, int64_t* n);
int bmbs_methyl_drop_variants(bmbs_methyl_site* site, int64_t n_site, const bmbs_methyl_site* opp, int64_t n_opp,
                              int32_t min_opposite_depth, int32_t max_variant_ppm, int64_t* n_kept);

/* ---- the genome-wide cytosine report (csrc/k_cytosine.hip; `--methyl <prefix> --cytosine-report`; tests/cytosine_spec.py) -----------------
 * One line of text for every cytosine of a selected context, on both strands, whether a read covered it or not (Bismark's CX_report,
 * MethylDackel's --cytosine_report): what tells "not covered" from "no cytosine there".  bmbs_methyl_report writes the lines of the
 * forward positions p in [beg, end) of sequence `ref`, ascending.  A position gets a line iff the rule above gives it a context and a
 * strand (a forward C: strand +, a forward G: strand -), the context is in `contexts`, and its WINDOW -- the cytosine and the one
 * (CpG) or two (CHG, CHH) positions behind it on its strand: [p, p + w] for +, [p - w, p] for - -- touches none of the runs.  run[2 r],
 * run[2 r + 1] = [beg, end) of the r-th run of bases of this sequence that the FASTA does not spell A, C, G or T (the index holds a
 * pseudo-random letter there): the rule bmbs_search filters the sites of its bedGraphs with, so both agree on which cytosines exist.
 * The line is
 *     name \t p + 1 \t strand \t meth \t unmeth \t context \t tri \n
 * name = the sequence's (bmbs_sam_refs), meth / unmeth = the counts of the site with pos = p, 0 and 0 when there is none, context = CG,
 * CHG or CHH, tri = three letters read on the cytosine's own strand from the cytosine on: the letters of p, p + 1, p + 2 for +, the
 * complements of those of p, p - 1, p - 2 for -; a position off the sequence's ends or inside a run is written N (this can only be the
 * third letter, and only of a CpG: one on the last two bases of a sequence, or directly in front of a run).  The decimal numbers have no
 * sign and no padding; nothing is rounded; there is no percent column and no header line.
 * A site whose kind has BMBS_REPORT_OMIT set takes the line of its position away: bmbs_search marks the sites its variant filter
 * dropped this way -- such a position is a polymorphism of the sample, not an uncovered cytosine.
 * site[0 .. n_site) (host memory): all of sequence `ref`, beg <= pos < end, pos strictly ascending, kind & 7 = context | strand << 2 as
 * the genome has it, the context selected, the window clear of the runs (the caller filters such sites first, as bmbs_search does).
 * run (host memory): n_run pairs, ascending and disjoint; NULL with n_run 0.
 * BMBS_ESTATE: no index attached, or bmbs_sam_refs has not been given the index's names.  BMBS_EINVAL (bmbs_last_error names the first
 * offender): ref outside the index's sequences; not 0 <= beg <= end <= the sequence's length; contexts outside 1..7; a run out of order
 * or overlapping; a site with another ref, outside [beg, end), not behind its predecessor, with a kind the genome does not have there,
 * of a context that is not selected, or whose window touches a run.  BMBS_ENOMEM with *out_bytes and *n_line set when cap is smaller
 * than the text, a cap of 0 being the size query; nothing is written behind out + cap or out + *out_bytes.  beg == end is valid: 0
 * bytes.  The call leaves the context's methylation result (sites, M-bias table, opposite-strand entries) as it is.
 * Unlike Bismark: a CpG whose third letter is unknown is written, with N (Bismark skips it); the caller gets one text, not one per
 * chromosome; positions are 1-based always (no --zero_based); no gzip; no CpG-merged report.                                       */
#define BMBS_REPORT_OMIT 8             /* in bmbs_methyl_site.kind, for bmbs_methyl_report only */
int bmbs_methyl_report(bmbs_ctx*, int32_t ref, int64_t beg, int64_t end, const bmbs_methyl_site* site, int64_t n_site,
                       const int64_t* run, int64_t n_run, int32_t contexts, char* out, uint64_t cap, uint64_t* out_bytes, int64_t* n_line);

/* ---- reads the bisulfite treatment did not convert (csrc/k_nonconv.hip; `--bam --sort --filter-non-conversion`; tests/nonconv_spec.py) ------
 * A read that carries several methylated cytosines outside CpG context is, in a mammalian sample, almost always a conversion failure
 * (Bismark's filter_non_conversion, MethylDackel's --minConversionEfficiency).  Exact integers throughout.
 * A record is EXAMINED when it is there (len != 0), refID >= 0, flag 4 is clear, flags 0x100 and 0x800 are clear and n_cigar_op > 0.
 * MAPQ, the proper-pair flag, 0x200 and 0x400 are not looked at: the filter sees every aligned read.  Its CALLS are those of the rule
 * above with the strand from the flags, M = X, the context from the genome alone, no mate-overlap clip, no trim, a base quality
 * >= min_phred (a quality byte 0xff is 0).  nm / nu = the methylated / unmethylated calls in CHG and CHH together; CpG calls are
 * counted for the totals only.  params NULL: threshold 3, percent 0, min_count 5, min_phred 0 (Bismark's --threshold and
 * --minimum_count, no quality bound as there).  A record FAILS iff
 *     threshold > 0 && nm >= threshold,  or  percent > 0 && nm + nu >= min_count && 100 * nm >= percent * (nm + nu)   (64-bit).
 * Both switches 0 is valid: nothing fails, counts and totals are still produced.  BMBS_EINVAL ("bad parameters") for a negative value,
 * percent > 100 or min_phred > 255.  A TEMPLATE is one entry, or with `paired` the entries 2p and 2p + 1; it fails iff any of its
 * records fails (either read fails the pair, as in Bismark).  A caller marks a failed template by `flag |= 0x200` (QC fail) in EVERY
 * record of it, the mate that is unmapped or was not examined too: record byte 19 |= 0x02, the byte --markdup uses; nothing else in a
 * record changes.  Every methylation call above, samtools and MethylDackel then leave such records out.
 * totals[2 strand (0 OT, 1 OB)][3 context][2 (0 unmethylated, 1 methylated)] = the calls of all examined records, failed or not: the
 * run's conversion estimate comes from them.
 * bmbs_bam_nonconv: `records` = n entries in host memory, len[i] their sizes (0: no record here).  count (n entries, or NULL): the
 * non-CpG calls of each record, 0 and 0 when it is not examined.  fail[t] = 1 when template t fails, else 0; *n_tmpl = the templates
 * (n, or n / 2), *n_fail = those that fail.  BMBS_ENOMEM with *n_tmpl set when fail_cap is smaller (a cap of 0: the size query; nothing
 * is computed then).  totals: 12 entries, or NULL.
 * bmbs_text_sorted_nonconv: the same for the context's last BMBS_TEXT_BAM_SORTED call, computed from the buffers that call left on the
 * device, a pair's two output lines being its template: fail[j] = 1 when the template of the j-th record the call returned failed
 * (*n = their number, that of bmbs_text_sorted_index), *n_tmpl_failed = the templates of the batch that failed.  BMBS_ENOMEM with *n
 * set when cap is smaller.
 * BMBS_ESTATE: no index attached; bmbs_text_sorted_nonconv: there was no such call, or another call on the context has rewritten the
 * buffers since.  BMBS_EINVAL (bmbs_last_error names the record): the length, refID and span checks of bmbs_bam_methyl; an odd n with
 * `paired`.  n = 0 is valid.  Both calls leave the context's methylation result and what a sort left on the device as they are.
 * Not done: Bismark's --consecutive; removing records (they are flagged); per-strand thresholds; any interaction with --markdup
 * (signatures and scores are computed as before, and a template may carry both flags).                                           */
typedef struct bmbs_nonconv_params { int32_t threshold, percent, min_count, min_phred; } bmbs_nonconv_params;
typedef struct bmbs_nonconv_count { uint32_t meth, unmeth; } bmbs_nonconv_count;   /* non-CpG calls of one record; 0, 0 when not examined */
int bmbs_bam_nonconv(bmbs_ctx*, const char* records, uint64_t bytes, const uint32_t* len, int64_t n, int32_t paired,
                     const bmbs_nonconv_params* params, bmbs_nonconv_count* count, uint8_t* fail, int64_t fail_cap,
                     int64_t* n_tmpl, int64_t* n_fail, uint64_t totals[12]);
int bmbs_text_sorted_nonconv(bmbs_ctx*, const bmbs_nonconv_params* params, uint8_t* fail, int64_t cap, int64_t* n,
                             int64_t* n_tmpl_failed, uint64_t totals[12]);

/* a21: per-ctx counters of the batches mapped so far = {reads, unique, ambiguous, mapped bases,
 * error bases} (Schema.cpp:25141-25146); bmbs_stats_allreduce sums them over the ctxs one process
 * drives (get_mapping_informations, Schema.cpp:451-476).  Multi-process jobs sum the five int64 with
 * one RCCL all-reduce in the host layer (bitmapperbs_amd.distributed).                             */
int bmbs_stats_get(bmbs_ctx*, int64_t stats[5]);
int bmbs_stats_reset(bmbs_ctx*);
int bmbs_stats_allreduce(bmbs_ctx** ctxs, int n, int64_t stats[5]);

/* ---- measurement ------------------------------------------------------------------------------- */
/* per-kernel HIP-event timings of the last bmbs_map_se[_device] call, on the ctx stream.
 * names/ms arrays of length >= *n (in: capacity, out: count).                                     */
int bmbs_profile_last(bmbs_ctx*, const char** names, float* ms, int* n);
/* the same HIP-event timings summed over every mapping call since bmbs_profile_reset (all lanes), and the number of calls (a
 * call split over two lanes counts twice): per-kernel averages of a timed region without a wait after every call           */
int bmbs_profile_total(bmbs_ctx*, const char** names, double* ms, int* n, int64_t* calls);
int bmbs_profile_reset(bmbs_ctx*);
/* event counters of the last call for the algorithmic-byte model:
 * c[0]=n_hash c[1]=n_ext(LF pairs) c[2]=n_sa c[3]=n_cand(windows filtered) c[4]=n_sw(jobs that ran the DP) c[5]=n_ungapped
 * c[6]=window bytes                                                                               */
int bmbs_counters_last(bmbs_ctx*, uint64_t c[8]);
/* all 32 words: c[0..7] as above, c[8] three-letter index steps taken (each counts three in c[1]); what the list kernels handled:
 * c[9] / c[10] / c[11] candidates located by the kernels for lists of 17..32 / 33..256 / more entries, c[12] lists of more than 32,
 * c[13] list entries filter_pairs read, c[14] candidates of re-seeded mates (--sensitive), c[15] located sites the paired-end vote
 * kernels dropped before sorting (no partner on the mate's list); c[16+4*kid+{0,1,2,3}] =
 * n_hash, n_ext, n_sa, n_ungapped of seeding kernel kid (0 k_seed_first, 1 k_seed_second, 2 k_seed_extra)          */
int bmbs_counters_all(bmbs_ctx*, uint64_t c[32]);
/* calls that were issued a second time with exact buffer sizes because a stage count (candidate slots, DP jobs, re-seeded
 * candidates) exceeded the capacity learned from earlier calls (see "launch sequence" below); diagnostic                      */
int64_t bmbs_retries(bmbs_ctx*);
/* diagnostic (bmbs_search --verbose, bench.py's e2e keys): out = { seconds the context's bmbs_map_*_text / bmbs_text_map_open calls kept
 * the link busy with uploads, with downloads (a copy and the wait for its end; waiting for another context's copy excluded), seconds
 * spent inside those calls, number of calls }                                                                                     */
int bmbs_text_times(bmbs_ctx*, double out[4]);
/* diagnostic: the Huffman code lengths the device's BGZF deflater (--bam) gives a table of symbol frequencies -- n <= 320 symbols,
 * maxbits <= 15; every used symbol gets a length, the lengths form a complete prefix code (tests/test_gpu_parity.py)              */
int bmbs_debug_huff_lengths(bmbs_ctx*, const uint32_t* freq, int32_t n, int32_t maxbits, uint8_t* len_out);

/* ---- index files (next-row (f)2: reader/writer of the reference's on-disk formats) ------------- */
typedef struct bmbs_index_file bmbs_index_file;
/* Load_Index/load_index equivalents: reads <prefix>.index, .index.bs.pac, .index.bs.index{,.bwt,.sa,.occ} */
bmbs_index_file* bmbs_index_file_load(const char* prefix);
void bmbs_index_file_view(const bmbs_index_file*, bmbs_index_view* out);
const char* bmbs_index_file_chrom_name(const bmbs_index_file*, int i);
void bmbs_index_file_free(bmbs_index_file*);
/* createIndex equivalent (Index.cpp:832-938) without the psascan dependency: FASTA -> the six files */
int bmbs_index_build(const char* fasta, const char* prefix, int n_threads);
/* the same builder with the suffix sort and every array-sized derivation (BWT planes, Occ counters, SA_flag, samples, 16-mer
 * rows) on HIP device `device_id`: the same six files byte for byte; a GRCh38-size genome (6.2 G suffixes) in well under a
 * minute instead of six on 64 host cores.  Needs about 60 bytes of device memory per base.  n_threads: host threads of the
 * FASTA / .pac preparation.  BMBS_ENODEV without a device (no silent fall-back to the host builder).                       */
int bmbs_index_build_device(int device_id, const char* fasta, const char* prefix, int n_threads);

/* Index and depth of a seed start in the balanced outcome table (bmbs_index_attach builds it for texts of 2^32 symbols and more,
 * BMBS_TDEPTH=h32|h33 forces it), as the seeding kernels compute them.  bases = the 32 bases read[tm .. tm+31], 2 bits each from
 * bit 0 on (A 0, C 1, G 2, T 3; C counts as T), not_acgt = one bit each, set where the character is none of these, len = the
 * characters read[tm ..] has, bits = 32 or 33.  The index is the first `bits` bits of the code T -> 0, G -> 10, A -> 11 of the
 * letters (first code bit highest); *depth gets the letters whose code lies completely inside them, 16 .. 32.  Returns the index, or
 * -1 when the lookup takes the 16-mer path instead: a character outside ACGT among the *depth letters, or len < *depth (-2: bad
 * `bits`).  Host arithmetic only: needs no context and no device.                                                                */
int64_t bmbs_outcome_index(uint64_t bases, uint32_t not_acgt, int32_t len, int32_t bits, int32_t* depth);

/* first 16 hex digits of the sha256 over the library's sources (in the Makefile's LIB_SRCS order) at build time: lets a run show
 * that the .so it loaded was built from the sources it sits next to (bitmapperbs_amd.capi.sources_id() recomputes it)          */
const char* bmbs_build_id(void);

/* Page-locked host buffers for the host-pointer entry points (bmbs_map_se / bmbs_map_pe copy from and to them at
 * full link speed).  The reference's per-thread scratch is plain malloc (Schema.cpp:24344-24362); a caller that
 * keeps malloc'ed buffers still works, only slower.  NULL on failure.                                     */
void* bmbs_host_alloc(uint64_t bytes);
/* the same with the buffer's role stated: 1 = the host writes it and the device reads it (FASTQ windows), 2 = the device writes it
 * and the host reads it (SAM text), 0 = either                                                             */
void* bmbs_host_alloc_kind(uint64_t bytes, int32_t kind);
void  bmbs_host_free(void* p);
/* lets the device touch a page-locked buffer once (kind 1: reads it, 2: writes it, 0: both): the first copy to or from a fresh
 * buffer is several times slower than the later ones; a driver does this while it loads                                  */
int   bmbs_host_prefault(bmbs_ctx*, void* p, uint64_t bytes, int32_t kind);

#ifdef __cplusplus
}
#endif
#endif
