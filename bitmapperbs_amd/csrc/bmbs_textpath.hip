// bitmapperbs_amd/csrc/bmbs_textpath.hip -- the two ends of the file path, their kernels and their entry points (a translation unit of its
// own since round 5): FASTQ text -> line index -> read rows (bmbs_map_*_fastq, bmbs_map_*_text), BGZF blocks inflated on the device
// (bmbs_inflate_bgzf, bmbs_text_open_bgzf / bmbs_text_map_open), records -> SAM text or BAM records in BGZF blocks, or (BMBS_TEXT_BAM_SORTED)
// the BAM records in coordinate order.  The mapping in between is bmbs_api.hip's (lane_enqueue / lane_settle).  Kernels: bmbs_text.hip,
// bmbs_bam.hip, bmbs_inflate.hip, k_bamsort.hip.  The sort, the deflater and the download (bam_sort_device, bgzf_deflate, bgzf_collect,
// download_locked) also serve the stages behind the sorted BAM, which are bmbs_records.hip's.
#include "bmbs_host.h"
#define DEVI __device__ __forceinline__
#include "bmbs_text.hip"
#include "k_trim.hip"
#include "bmbs_bam.hip"
#include "bmbs_inflate.hip"
#include "k_bamsort.hip"

// the constants the kernels of this file read: x^(2^n) mod P of CRC-32 for the BGZF blocks' CRCs (bmbs_bytes.h: crc_x8n); per device
void textpath_device_init(Lane* c)
{
    (void)c;
    u32 x2n[32];
    auto mult = [](u32 a, u32 b) { u32 m = 1u << 31, p = 0; for (;;) { if (a & m) { p ^= b; if ((a & (m - 1)) == 0) break; } m >>= 1; b = (b & 1) ? (b >> 1) ^ 0xedb88320u : b >> 1; } return p; };
    u32 p = 1u << 30;
    x2n[0] = p;
    for (int n = 1; n < 32; n++) { p = mult(p, p); x2n[n] = p; }
    (void)hipMemcpyToSymbol(HIP_SYMBOL(c_x2n), x2n, sizeof x2n);
}

// ---- one clock for the host-side phase times of this file (bmbs_text_times; BMBS_TEXT_TRACE=1, a diagnostic: a line per call on stderr)
static double wall() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
static bool text_trace() { static const bool on = getenv("BMBS_TEXT_TRACE") != nullptr; return on; }
// a call's phase marks, each taken when its phase has ended (an open call: uploaded = inflated, delivered = tails); down_wait: what of the download was not the copy
struct TextClock { double start = 0, uploaded = 0, lines = 0, records = 0, mapped = 0, sized = 0, written = 0, delivered = 0, down_wait = 0; };

// ------------------------------------------------------------------------------------------------
// FASTQ text in (the host only finds the line starts; the rows are cut out of the text on the device)
// what the row stage reads of one FASTQ text on the device: the text, and where each record's sequence and quality lines are
struct FqSrc { const char* text; const u32* seq_off; const u32* qual_off; const u16* seq_len; const u16* qual_len; };

int fastq_check(Lane* c, const bmbs_fastq_view* v, int64_t n, int L_max)
{
    if (!v || !v->text || !v->seq_off || !v->qual_off || !v->seq_len || !v->qual_len) { c->err = "fastq view: NULL field"; return BMBS_EINVAL; }
    if (v->text_bytes >= (1ull << 32)) { c->err = "fastq view: a text window has to be smaller than 4 GiB (32-bit offsets)"; return BMBS_EINVAL; }
    // every line the device is going to read lies inside the window (a bad index must not become an out-of-bounds device read)
    for (int64_t i = 0; i < n; i++) {
        const uint64_t sl = v->seq_len[i], ql = v->qual_len[i];
        if (sl < 1 || sl > (uint64_t)L_max || ql > sl || (uint64_t)v->seq_off[i] + sl > v->text_bytes || (uint64_t)v->qual_off[i] + ql > v->text_bytes) {
            c->err = "fastq view: record " + std::to_string(i) + " has a line outside the text window or a length outside 1..L_max";
            return BMBS_EINVAL;
        }
    }
    return BMBS_OK;
}
// text + index arrays of one file to the device; idx_at = byte offset of this file's arrays inside c->fq_idx
int fastq_upload(Lane* c, DevBuf& dtext, const bmbs_fastq_view* v, u64 n, u64 idx_at, FqSrc& out)
{
    ENS(c, dtext, v->text_bytes + 64);
    HIPCHK(c, hipMemcpyAsync(dtext.p, v->text, v->text_bytes, hipMemcpyHostToDevice, c->stream));
    char* base = c->fq_idx.as<char>() + idx_at;
    HIPCHK(c, hipMemcpyAsync(base, v->seq_off, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(base + n * 4, v->qual_off, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(base + n * 8, v->seq_len, n * 2, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(base + n * 10, v->qual_len, n * 2, hipMemcpyHostToDevice, c->stream));
    out.text = dtext.as<char>(); out.seq_off = reinterpret_cast<const u32*>(base); out.qual_off = reinterpret_cast<const u32*>(base + n * 4);
    out.seq_len = reinterpret_cast<const u16*>(base + n * 8); out.qual_len = reinterpret_cast<const u16*>(base + n * 10);
    return BMBS_OK;
}

// The row stage: n records (pairs: src[1] is mate 2's text) of at most L bases -> the lane's read rows (k_fastq_rows), and in P the
// call that maps them into out_res / cig_pool.  Sizes the lane's row, quality, length, result and CIGAR buffers.  pbat (single end):
// every read reverse-complemented, its qualities mirrored; uniform: the caller knows that every read has L bases
static int fastq_rows(Lane* c, bool pe, const FqSrc* src, u64 n, int L, int pbat, bool uniform, Pending& P)
{
    const u64 n2 = pe ? 2 * n : n;
    const int ds = (L + 15) / 16 * 16;
    const u64 pool = n2 * (u64)cigar_ops_bound(c->prm, L, threshold_k(c->prm, L));
    DevBuf& rows = pe ? c->pe_seq : c->in_seq;
    ENS(c, c->out_res, n2 * 32); ENS(c, c->cig_pool, pool * 4); ENS(c, c->in_len, n2 * 2 + 16);
    ENS(c, rows, n2 * (u64)ds + 64); ENS(c, c->in_qual, n * (u64)ds + 64);
    if (pe) ENS(c, c->in_qual2, n * (u64)ds + 64);
    // pairs: rows 0..n-1 = mate 1 as read, rows n..2n-1 = mate 2 reverse-complemented; the qualities stay in FASTQ order (qual_row)
    char* const seq = rows.as<char>();
    char* const seq2 = seq + n * (u64)ds;
    const unsigned g = nblk(n * (u64)(ds / 16), 256);
    hipLaunchKernelGGL(k_fastq_rows, dim3(g), dim3(256), 0, c->stream, src[0].text, src[0].seq_off, src[0].qual_off, src[0].seq_len, src[0].qual_len, (long)n, ds,
                       pbat, pbat, seq, c->in_qual.as<char>(), c->in_len.as<u16>());
    if (pe)
        hipLaunchKernelGGL(k_fastq_rows, dim3(g), dim3(256), 0, c->stream, src[1].text, src[1].seq_off, src[1].qual_off, src[1].seq_len, src[1].qual_len, (long)n, ds,
                           1, 0, seq2, c->in_qual2.as<char>(), c->in_len.as<u16>() + n);
    P = Pending();
    P.pe = pe; P.L = L; P.stride = ds; P.n = (int64_t)n; P.prepared = pe;
    P.a[0] = (uint64_t)seq; P.a[1] = (uint64_t)c->in_qual.p;
    if (pe) { P.a[2] = (uint64_t)seq2; P.a[3] = (uint64_t)c->in_qual2.p; }
    P.d_len = uniform ? nullptr : c->in_len.as<u16>();
    P.d_results = (uint64_t)c->out_res.p; P.d_cigar_pool = (uint64_t)c->cig_pool.p; P.cigar_cap = (int64_t)pool;
    return BMBS_OK;
}

// bmbs_map_se_fastq / bmbs_map_pe_fastq: check, upload, row stage, mapping, records and CIGAR words back to the host
static int lane_map_fastq(Lane* c, bool pe, const bmbs_fastq_view* const* views, int64_t n_in, int32_t L_max, int32_t uniform, int32_t pbat,
                          bmbs_result* results, uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used)
{
    if (!c) return BMBS_EINVAL;
    HIPCHK(c, hipSetDevice(c->dev));
    if (n_cigar_used) *n_cigar_used = 0;
    if (n_in <= 0) return BMBS_OK;
    if (L_max <= 0 || L_max > BMBS_MAX_READ) { c->err = "bad read geometry"; return BMBS_EINVAL; }
    const int nf = pe ? 2 : 1;
    for (int f = 0; f < nf; f++) { const int r0 = fastq_check(c, views[f], n_in, L_max); if (r0) return r0; }
    const u64 n = (u64)n_in, n2 = (u64)nf * n;
    ENS(c, c->fq_idx, n2 * 12 + 64 * (u64)nf);
    FqSrc src[2] = {};
    DevBuf* const text[2] = {&c->fq_text1, &c->fq_text2};
    for (int f = 0; f < nf; f++) { const int r1 = fastq_upload(c, *text[f], views[f], n, f ? (n * 12 + 63) & ~63ull : 0, src[f]); if (r1) return r1; }
    Pending P;
    int rc = fastq_rows(c, pe, src, n, L_max, !pe && pbat ? 1 : 0, uniform != 0, P);
    if (rc) return rc;
    rc = lane_enqueue(c, P, true);
    if (rc) return rc;
    rc = lane_settle(c);                         // counts (and, rarely, the repeat with exact sizes) before anything is copied back
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(results, c->out_res.p, n2 * 32, hipMemcpyDeviceToHost, c->stream));
    const u64 used = c->last_n_jobs * (u64)c->last_max_ops;
    if (used > (u64)cigar_cap) { c->err = "host cigar pool too small"; (void)hipStreamSynchronize(c->stream); return BMBS_ENOMEM; }
    if (used) HIPCHK(c, hipMemcpyAsync(cigar_pool, c->cig_pool.p, used * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_cigar_used) *n_cigar_used = (int64_t)used;
    return BMBS_OK;
}

// ------------------------------------------------------------------------------------------------
// FASTQ text in, SAM text out (bmbs_text.hip): the host reads and writes files, everything between is on the device
// newline index of one text window (already on the device): positions of its first 4 * n_cap newlines; the word TOT_LINES_1 (file 2: _2) gets
// the number of lines found
int text_index(Lane* c, DevBuf& dtext, u64 bytes, u64 n_cap, int f)
{
    const u64 tiles = (bytes + FQ_TILE_BYTES - 1) / FQ_TILE_BYTES;
    ENS(c, c->tx_tilecnt, tiles * 4 + 64); ENS(c, c->tx_tileoff, (tiles + 1) * 8 + 64);
    ENS(c, c->tx_nl[f], (4 * n_cap + 8) * 4);
    hipLaunchKernelGGL(k_fq_count, dim3((unsigned)tiles), dim3(FQ_TILE_THREADS), 0, c->stream, dtext.as<char>(), bytes, c->tx_tilecnt.as<u32>());
    int rc = scan_u32(c, c->tx_tilecnt.as<u32>(), tiles, c->tx_tileoff.as<u64>(), tot_file(TOT_LINES_1, f));
    if (rc) return rc;
    hipLaunchKernelGGL(k_fq_lines, dim3((unsigned)tiles), dim3(FQ_TILE_THREADS), 0, c->stream, dtext.as<char>(), bytes, c->tx_tileoff.as<u64>(), 4 * n_cap, c->tx_nl[f].as<u32>());
    return BMBS_OK;
}
// the per-record field arrays of n records, in `buf`; fq_rec_setup: those of file f that k_fq_records writes
static int fq_rec_carve(Lane* c, DevBuf& buf, u64 n, FqRec& rec)
{
    const u64 n4 = (n * 4 + 63) & ~63ull, n2 = (n * 2 + 63) & ~63ull;
    ENS(c, buf, 3 * n4 + 3 * n2 + 64);
    char* b = buf.as<char>();
    rec.seq_off = reinterpret_cast<u32*>(b); rec.qual_off = reinterpret_cast<u32*>(b + n4); rec.name_off = reinterpret_cast<u32*>(b + 2 * n4);
    rec.seq_len = reinterpret_cast<u16*>(b + 3 * n4); rec.qual_len = reinterpret_cast<u16*>(b + 3 * n4 + n2); rec.name_len = reinterpret_cast<u16*>(b + 3 * n4 + 2 * n2);
    return BMBS_OK;
}
int fq_rec_setup(Lane* c, u64 n, int f, FqRec& rec) { return fq_rec_carve(c, c->tx_rec[f], n, rec); }

// ---- the trim stage of a text call (k_trim.hip; bmbs_set_trim): behind k_fq_records, in front of everything that reads a record
// A 5' clip moves a line's start by up to a read's length, behind the end of a quality line that is shorter than that: while trimming
// is on, the text buffers carry 1 KiB more beyond the window, so that a range computed from such a start (k_line_write's staging) stays
// inside them.  With trimming off they are sized as ever.
#define TEXT_PAD 64
#define TEXT_PAD_TRIM 1024
static u64 text_pad(const Lane* c) { return TEXT_PAD + (c->trim.on ? TEXT_PAD_TRIM : 0); }
// what k_fq_trim is told about the records of mate m
static TrimArgs trim_args(const Lane* c, int m, int min_length)
{
    const bmbs_trim_opts& o = c->trim.opts;
    TrimArgs a = {};
    char ad[32] = {};
    a.alen = (int)strlen(o.adapter[m]);
    for (int j = 0; j < a.alen; j++) ad[j] = (char)(o.adapter[m][j] & ~32);
    memcpy(a.ad, ad, sizeof ad);
    a.quality = o.quality; a.base = c->prm.q_base; a.min_overlap = o.min_overlap; a.error_permille = o.error_permille;
    a.clip5 = o.clip_5p[m]; a.clip3 = o.clip_3p[m]; a.min_length = min_length;
    return a;
}
// the counters zeroed, then the records of one file (mate m) trimmed in place: their keep bytes in tr_keep (file f: behind file 0's)
static int trim_begin(Lane* c, u64 n)
{
    ENS(c, c->tr_words, TRW_WORDS * sizeof(u64)); ENS(c, c->tr_keep, 2 * ((n + 63) & ~63ull) + 64);
    HIPCHK(c, hipMemsetAsync(c->tr_words.p, 0, TRW_WORDS * sizeof(u64), c->stream));
    return BMBS_OK;
}
static u8* trim_keep_of(Lane* c, u64 n, int f) { return c->tr_keep.as<u8>() + (f ? (n + 63) & ~63ull : 0); }
static void trim_file(Lane* c, const char* text, const FqRec& rec, u64 n, int f, int m, int min_length)
{
    prof_begin(c, "k_fq_trim");
    hipLaunchKernelGGL(k_fq_trim, dim3(nblk(n, TRIM_RECS)), dim3(TRIM_BLOCK), 0, c->stream, text, rec, (long)n, trim_args(c, m, min_length), trim_keep_of(c, n, f),
                       c->tr_words.as<unsigned long long>() + TRW_PER_MATE * m);
    prof_end(c);
}
// every record trimmed, the templates that stay compacted into the second set of arrays, which `rec` names from here on; the kept
// count is left in TOT_TRIM_KEPT, the counters and the two lengths in tr_words.  No wait
static int trim_stage(Lane* c, bool pe, u64 n, FqRec* rec)
{
    const int nf = pe ? 2 : 1;
    int rc = trim_begin(c, n);
    if (rc) return rc;
    ENS(c, c->tr_flag, n * 4 + 64); ENS(c, c->tr_off, (n + 1) * 8 + 64);
    const char* const text[2] = {c->fq_text1.as<char>(), c->fq_text2.as<char>()};
    for (int f = 0; f < nf; f++) trim_file(c, text[f], rec[f], n, f, f, c->trim.opts.min_length);
    hipLaunchKernelGGL(k_trim_keep, dim3(nblk(n, 256)), dim3(256), 0, c->stream, trim_keep_of(c, n, 0), pe ? trim_keep_of(c, n, 1) : (const u8*)nullptr, (long)n, c->tr_flag.as<u32>());
    rc = scan_u32(c, c->tr_flag.as<u32>(), n, c->tr_off.as<u64>(), TOT_TRIM_KEPT);
    if (rc) return rc;
    unsigned long long* const w = c->tr_words.as<unsigned long long>();
    for (int f = 0; f < nf; f++) {
        FqRec dst;
        rc = fq_rec_carve(c, c->tr_rec[f], n, dst);
        if (rc) return rc;
        prof_begin(c, "k_fq_compact");
        hipLaunchKernelGGL(k_fq_compact, dim3(nblk(n, 256)), dim3(256), 0, c->stream, rec[f], dst, c->tr_flag.as<u32>(), c->tr_off.as<u64>(), (long)n,
                           w + TRW_PER_MATE * f + TRW_BASES_OUT, w + TRW_MAX_LEN);
        prof_end(c);
        rec[f] = dst;
    }
    return BMBS_OK;
}
// the counters of a call as the device left them (h_info->trim) -> the caller's form
static void trim_counts_from(const u64* w, bool pe, u64 n_in, u64 kept, bmbs_trim_counts* o)
{
    memset(o, 0, sizeof *o);
    for (int m = 0; m < (pe ? 2 : 1); m++) {
        const u64* x = w + TRW_PER_MATE * m;
        o->records_in[m] = (int64_t)x[TRW_RECORDS_IN]; o->bases_in[m] = (int64_t)x[TRW_BASES_IN]; o->bases_out[m] = (int64_t)x[TRW_BASES_OUT];
        o->quality_records[m] = (int64_t)x[TRW_Q_RECORDS]; o->quality_bases[m] = (int64_t)x[TRW_Q_BASES];
        o->adapter_records[m] = (int64_t)x[TRW_A_RECORDS]; o->adapter_bases[m] = (int64_t)x[TRW_A_BASES];
        o->clip_records[m] = (int64_t)x[TRW_C_RECORDS]; o->clip_bases[m] = (int64_t)x[TRW_C_BASES];
    }
    o->templates_dropped = (int64_t)(n_in - kept);
}
// D2H in pieces: one 2 GiB device-to-host copy ran at a quarter of the link rate on the MI355X boxes (tools/pcie_probe)
int d2h_chunked(Lane* c, char* dst, const char* src, u64 bytes, hipStream_t st)
{
    const u64 piece = 128ull << 20;
    for (u64 o = 0; o < bytes; o += piece) HIPCHK(c, hipMemcpyAsync(dst + o, src + o, std::min(piece, bytes - o), hipMemcpyDeviceToHost, st));
    return BMBS_OK;
}

// One upload and one download at a time per device, whatever the number of contexts: concurrent copies in one direction share the
// link badly (tools/pcie_probe: 48 GB/s each way with one stream per direction, 33 with three), and a context's copies are long
// enough (hundreds of MB) to fill the link on their own.  Held from the first copy of a phase until the wait that ends it.
std::mutex g_h2d_mu[16];
std::mutex g_d2h_mu[16];
// The results of a text call go down the lane's own copy stream under the device's download mutex: one copy per direction and device at
// a time (two at once share the link and both finish late).  Round 5 tried ONE download stream per device shared by all contexts, the
// copies queued back to back without the host in between: 320 M reads to /dev/null took 3.3-3.8 s instead of 2.9-3.05 s, whether the
// copy waited on the stream for its kernel or was queued once the kernel had ended (tools/e2e_quick.sh, same box, alternating runs).
// *copy_s = seconds the copy held the link.
int download_locked(Lane* c, char* dst, const char* src, u64 bytes, hipStream_t after, double* copy_s)
{
    hipStream_t ds = down_stream_of(c);
    HIPCHK(c, hipStreamSynchronize(after));                  // the bytes are complete before the link is claimed
    std::lock_guard<std::mutex> down(g_d2h_mu[c->dev & 15]);
    const double t0 = wall();
    const int rc = d2h_chunked(c, dst, src, bytes, ds);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(ds));
    if (copy_s) *copy_s = wall() - t0;
    return BMBS_OK;
}

// k_line_write's launch shape: lines per workgroup and the LDS it gets for the image of its piece of the output and for the staged
// FASTQ text, from the window's bytes per record.  `hb` bounds the computed columns of one line (the plain path keeps them in a
// quarter of the image buffer).  BMBS_TXW_TINY=1 (test aid): staging buffers too small for anything -- every workgroup takes the plain path.
struct TxwPlan { int lpb; u32 out_cap, src_cap; size_t lds; };
static TxwPlan txw_plan(bool pe, u64 text_bytes, u64 n_lines, int hb)
{
    static const bool tiny = getenv("BMBS_TXW_TINY") != nullptr;
    TxwPlan t = {0, 0, 0, 0};
    if (4 * (u64)hb > 30 * 1024) return t;
    const u64 rec = text_bytes / std::max<u64>(n_lines, 1) + 8, line = rec + 96;
    const u64 out_max = 30 * 1024, src_max = pe ? 15 * 1024 : 30 * 1024;
    int lpb = 32;
    auto need_out = [&](int l) { return ((u64)l * line * 5 / 4 + 64 + 15) & ~15ull; };
    auto need_src = [&](int l) { return ((u64)(pe ? l / 2 : l) * rec * 5 / 4 + 64 + 15) & ~15ull; };
    while (lpb > 2 && (need_out(lpb) > out_max || need_src(lpb) > src_max)) lpb /= 2;
    t.lpb = lpb;
    t.out_cap = (u32)std::min<u64>(std::max<u64>(need_out(lpb), (4 * (u64)hb + 15) & ~15ull), out_max);
    t.src_cap = tiny ? 16u : (u32)std::min<u64>(need_src(lpb), src_max);
    t.lds = (size_t)t.out_cap + 16 + (pe ? 2 : 1) * ((size_t)t.src_cap + 16);
    return t;
}

// ---- a record stream on the device -> BGZF blocks of BGZF_IN input bytes (the last one shorter), deflated by one workgroup each into
// the slots; total_ptr = the stream's size in device memory (what k_bgzf_block reads); *ztotal = the compressed bytes.  bgzf_collect
// then puts the blocks one behind the other into c->sam_out.
int bgzf_deflate(Lane* c, const char* raw, const u64* total_ptr, u64 raw_total, u64* ztotal)
{
    const u64 nb = (raw_total + BGZF_IN - 1) / BGZF_IN;
    c->ends(Lane::BGZF_BLOCKS);
    ENS(c, c->bam_slots, nb * (u64)BGZF_SLOT);
    ENS(c, c->bam_slot_len, nb * 4 + 64); ENS(c, c->bam_off, (nb + 1) * 8 + 64);
    const size_t lds = (size_t)BGZF_THREADS * BGZF_PSTRIDE * 4;                      // the block's bytes (padded segments)
    HIPCHK(c, hipMemsetAsync(c->bam_slots.p, 0, nb * (u64)BGZF_SLOT, c->stream));      // (k_bgzf_block ORs the shared words of its stream into the slots)
    static std::once_flag lds_once[16];
    std::call_once(lds_once[c->dev & 15], [&] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_bgzf_block), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); });
    prof_begin(c, "k_bgzf_block");
    hipLaunchKernelGGL(k_bgzf_block, dim3((unsigned)nb), dim3(BGZF_THREADS), lds, c->stream, raw, total_ptr, c->bam_slots.as<char>(), c->bam_slot_len.as<u32>());
    prof_end(c);
    const int rc = scan_u32(c, c->bam_slot_len.as<u32>(), nb, c->bam_off.as<u64>(), TOT_BGZF_BYTES);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(&c->h_info->z_bytes, tot_at(c, TOT_BGZF_BYTES), sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *ztotal = c->h_info->z_bytes;
    return BMBS_OK;
}
int bgzf_collect(Lane* c, u64 raw_total, u64 ztotal)
{
    const u64 nb = (raw_total + BGZF_IN - 1) / BGZF_IN;
    ENS(c, c->sam_out, ztotal + 64);
    prof_begin(c, "k_bgzf_gather");
    hipLaunchKernelGGL(k_bgzf_gather, dim3((unsigned)nb), dim3(256), 0, c->stream, c->bam_slots.as<char>(), c->bam_slot_len.as<u32>(), c->bam_off.as<u64>(), c->sam_out.as<char>());
    prof_end(c);
    return BMBS_OK;
}

// ---- coordinate sort of a record stream on the device (k_bamsort.hip): n entries, entry i = len[i] bytes at raw + off[i] (off: the
// exclusive scan of len, `total` bytes in all; raw is padded by 16 bytes and more) -> c->bs_sorted: the records stably sorted by key,
// c->bs_key2 / c->bs_slen their keys and lengths in that order, the word TOT_SORTED_BYTES their size.  skip_empty: entries of length 0 are output
// lines that print nothing, not records (they end up behind the records); *n_records = the others.
// BMBS_BSG_TINY=1 (test aid): no piece fits the gather kernel's image -- every workgroup takes the plain path.
int bam_sort_device(Lane* c, const char* raw, const u64* off, const u32* len, u64 n, u64 total, bool skip_empty, u64* n_records)
{
    static const bool tiny = getenv("BMBS_BSG_TINY") != nullptr;
    c->ends(Lane::SORT_BUFFERS);
    ENS(c, c->bs_key, n * 8 + 64); ENS(c, c->bs_key2, n * 8 + 64); ENS(c, c->bs_idx, n * 4 + 64); ENS(c, c->bs_idx2, n * 4 + 64);
    ENS(c, c->bs_slen, n * 4 + 64); ENS(c, c->bs_soff, (n + 1) * 8 + 64); ENS(c, c->bs_sorted, total + 256);
    u32* const info = stage_info(c);
    const u32* const got = c->h_info->stage;             // k_bam_keys' words: a bad record, the largest refID, entries of length 0
    HIPCHK(c, hipMemsetAsync(info, 0, 4 * sizeof(u32), c->stream));
    prof_begin(c, "k_bam_keys");
    hipLaunchKernelGGL(k_bam_keys, dim3(nblk(n, 256)), dim3(256), 0, c->stream, raw, off, len, (long)n, skip_empty ? 1 : 0, c->bs_key.as<u64>(), c->bs_idx.as<u32>(), info);
    prof_end(c);
    HIPCHK(c, hipMemcpyAsync(c->h_info->stage, info, 4 * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (got[0]) {
        c->err = "bam sort: the length given for record " + std::to_string(~got[0]) + " is not its block_size + 4 (or is below the 36 bytes every BAM record has)";
        return BMBS_EINVAL;
    }
    if (n_records) *n_records = n - got[2];
    c->sc.bai_ref_max = got[1];
    // the key bits that can be set: 33 of position and strand, and those of the largest reference index (-1 is all ones: it stays last
    // under any number of low bits, because no other index has them all set)
    int ref_bits = 1;
    while (ref_bits < 32 && ((u64)got[1] + 1) >> ref_bits) ref_bits++;
    const unsigned end_bit = (unsigned)(33 + ref_bits);
    { const int rc = bam_pair_sort(c, c->bs_key.as<u64>(), c->bs_key2.as<u64>(), c->bs_idx.as<u32>(), c->bs_idx2.as<u32>(), n, end_bit); if (rc) return rc; }
    hipLaunchKernelGGL(k_bam_slen, dim3(nblk(n, 256)), dim3(256), 0, c->stream, len, c->bs_idx2.as<u32>(), (long)n, c->bs_slen.as<u32>());
    const int rc = scan_u32(c, c->bs_slen.as<u32>(), n, c->bs_soff.as<u64>(), TOT_SORTED_BYTES);
    if (rc) return rc;
    // records per workgroup: three quarters of the image at the stream's mean record size
    const u64 mean = total / std::max<u64>(n, 1) + 1;
    const int rpb = (int)std::min<u64>(std::max<u64>((u64)BSG_CAP * 3 / 4 / mean, 1), 1024);
    prof_begin(c, "k_bam_gather");
    hipLaunchKernelGGL(k_bam_gather, dim3(nblk(n, (unsigned)rpb)), dim3(BSG_THREADS), 0, c->stream, raw, off, c->bs_idx2.as<u32>(), c->bs_soff.as<u64>(), (long)n, rpb,
                       tiny ? 0u : (u32)BSG_CAP, c->bs_sorted.as<char>());
    prof_end(c);
    return BMBS_OK;
}

// ---- a text call behind its upload, stage by stage (lane_text_finish runs them): the text window(s) are on the device (fq_text1 /
// fq_text2) and their newline positions are being indexed (text_index).  The caller's arguments and the clock; rec: the records' fields
// (records); max_ops, in: the CIGAR bound of the batch and what the length and write kernels read (map)
static const size_t STATS_BYTES = BMBS_SHARDS * BMBS_SHARD_WORDS * 8;
struct TextCall {
    Lane* c; bool pe; u64 in_bytes, n, n2; int32_t flags; char* sam; u64 sam_cap; u64* sam_bytes; int64_t* n_lines_out; TextClock t;
    FqRec rec[2]; int max_ops; SamIn in;
    // the fields of every record (k_fq_records) -> the longest and the shortest sequence line
    int records(int* maxL, int* minL)
    {
        for (int f = 0; f < (pe ? 2 : 1); f++) { const int rc = fq_rec_setup(c, n, f, rec[f]); if (rc) return rc; }
        // records can only be cut out once the host knows that every one of them is complete: the line counts first
        const u64* const lines = c->h_info->lines;
        HIPCHK(c, hipMemcpyAsync(c->h_info->lines, tot_at(c, TOT_LINES_1), sizeof c->h_info->lines, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        t.lines = wall();
        if (lines[0] < 4 * n || (pe && lines[1] < 4 * n)) { c->err = "text call: a window holds fewer than 4 lines per record"; return BMBS_EINVAL; }
        for (int f = 0; f < (pe ? 2 : 1); f++)
            hipLaunchKernelGGL(k_fq_records, dim3(nblk(n, 256)), dim3(256), 0, c->stream, c->tx_nl[f].as<u32>(), (long)n, rec[f], line_info(c) + TXI_FQ_WORDS * f);
        // trimming (bmbs_set_trim): the records rewritten and compacted before anybody reads them; its words come back with k_fq_records'
        const bool trim = c->trim.on;
        c->trim.counted = false;
        if (trim) {
            const int rc = trim_stage(c, pe, n, rec);
            if (rc) return rc;
            HIPCHK(c, hipMemcpyAsync(&c->h_info->trim_kept, tot_at(c, TOT_TRIM_KEPT), sizeof(u64), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->h_info->trim, c->tr_words.p, sizeof c->h_info->trim, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipMemcpyAsync(c->h_info->line, line_info(c), sizeof c->h_info->line, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        t.records = wall();
        const u32* const inf = c->h_info->line; const u32* const inf2 = inf + TXI_FQ_WORDS;      // k_fq_records' words of file 1, of file 2
        for (int f = 0; f < (pe ? 2 : 1); f++)
            if (inf[TXI_FQ_WORDS * f + 2]) {
                c->err = "record " + std::to_string(inf[TXI_FQ_WORDS * f + 2] - 1) + " of this batch has an empty or longer-than-" + std::to_string(BMBS_MAX_READ) + "-character sequence line: not supported (the reference's own buffers end there)";
                return BMBS_EINVAL;
            }
        *maxL = (int)inf[0]; *minL = (int)~inf[1];
        if (pe) { *maxL = std::max(*maxL, (int)inf2[0]); *minL = std::min(*minL, (int)~inf2[1]); }
        if (trim) {
            // the batch is the templates that stay, from here on
            const u64 kept = c->h_info->trim_kept;
            trim_counts_from(c->h_info->trim, pe, n, kept, &c->trim.cnt);
            c->trim.kept = (int64_t)kept; c->trim.counted = true;
            n = kept; n2 = pe ? 2 * kept : kept;
            *maxL = (int)c->h_info->trim[TRW_MAX_LEN]; *minL = (int)~(u32)c->h_info->trim[TRW_MIN_LEN_C];
        }
        return BMBS_OK;
    }
    // rows and mapping: the records are in out_res / cig_pool when this returns, and `in` names them for the kernels of every ending
    int map(int maxL, bool uniform)
    {
        max_ops = cigar_ops_bound(c->prm, maxL, threshold_k(c->prm, maxL));
        const FqSrc src[2] = {{c->fq_text1.as<char>(), rec[0].seq_off, rec[0].qual_off, rec[0].seq_len, rec[0].qual_len},
                              {c->fq_text2.as<char>(), rec[1].seq_off, rec[1].qual_off, rec[1].seq_len, rec[1].qual_len}};
        Pending P;
        int rc = fastq_rows(c, pe, src, n, maxL, (flags & BMBS_TEXT_PBAT) && !pe ? 1 : 0, uniform, P);
        if (rc) return rc;
        // a caller whose output buffer turns out too small repeats the call (too_small): the batch must not be counted twice
        ENS(c, c->stats_snap, STATS_BYTES);
        HIPCHK(c, hipMemcpyAsync(c->stats_snap.p, c->stats.p, STATS_BYTES, hipMemcpyDeviceToDevice, c->stream));
        rc = lane_enqueue(c, P, true);
        if (rc) return rc;
        rc = lane_settle(c);
        if (rc) return rc;
        t.mapped = wall();
        in.text[0] = src[0].text; in.text[1] = pe ? src[1].text : nullptr;
        in.rec[0] = rec[0]; in.rec[1] = rec[1];
        in.res = c->out_res.as<bmbs_result_dev>(); in.cigar = c->cig_pool.as<u32>();
        in.chrom_chars = c->chrom_chars.as<char>(); in.chrom_off = c->chrom_off.as<u32>();
        in.n = (long)n;
        in.flags = (flags & (BMBS_TEXT_PBAT | BMBS_TEXT_UNMAPPED)) | (c->prm.ambiguous_out ? BMBS_TEXT_AMBIG : 0) | (pe ? BMBS_TEXT_PE : 0);
        return BMBS_OK;
    }
    // BMBS_ENOMEM for an output buffer that is too small: the statistics go back to map's snapshot
    int too_small(const char* what)
    {
        (void)hipMemcpyAsync(c->stats.p, c->stats_snap.p, STATS_BYTES, hipMemcpyDeviceToDevice, c->stream);
        (void)hipStreamSynchronize(c->stream);
        c->err = what;
        return BMBS_ENOMEM;
    }
    // lengths -> offsets -> total on the host, for the SAM lines or the BAM records (k_bam_len also leaves a word in h_info->line)
    template <bool BAM> int sized(u64* total)
    {
        const Tot slot = BAM ? TOT_BAM_BYTES : TOT_SAM_BYTES;
        ENS(c, c->sam_len, n2 * 4 + 64); ENS(c, c->sam_off, (n2 + 1) * 8 + 64);
        prof_begin(c, BAM ? "k_bam_len" : "k_sam_len");
        if (BAM) hipLaunchKernelGGL(k_bam_len, dim3(nblk(n2, 256)), dim3(256), 0, c->stream, in, (long)n2, c->sam_len.as<u32>(), line_info(c));
        else hipLaunchKernelGGL(k_sam_len, dim3(nblk(n2, 256)), dim3(256), 0, c->stream, in, (long)n2, c->sam_len.as<u32>());
        const int rc = scan_u32(c, c->sam_len.as<u32>(), n2, c->sam_off.as<u64>(), slot);
        if (rc) return rc;
        prof_end(c);
        HIPCHK(c, hipMemcpyAsync(&c->h_info->out_bytes, tot_at(c, slot), sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        if (BAM) HIPCHK(c, hipMemcpyAsync(c->h_info->line, line_info(c), sizeof c->h_info->line, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        t.sized = wall();
        *total = c->h_info->out_bytes;
        return BMBS_OK;
    }
    // the lines into `out`, `total` bytes (k_line_write): hb bounds the computed columns of one line (txw_plan)
    template <bool BAM> int write(DevBuf& out, u64 total)
    {
        const int ops = std::max(max_ops, 1);
        ENS(c, out, total + (BAM ? 256 : 64));
        const TxwPlan tw = txw_plan(pe, in_bytes, n2, ((BAM ? 36 + 4 * ops + 8 : c->max_ref_len + 5 * ops + 96) + 15) & ~15);
        if (!tw.lpb) { c->err = BAM ? "text call: CIGARs too long" : "text call: reference names too long"; return BMBS_EINVAL; }
        prof_begin(c, BAM ? "k_bam_write" : "k_sam_write");
        hipLaunchKernelGGL(k_line_write<BAM>, dim3(nblk(n2, (unsigned)tw.lpb)), dim3(TXW_THREADS), tw.lds, c->stream, in, (long)n2, c->sam_off.as<u64>(), tw.lpb, tw.out_cap, tw.src_cap,
                           out.as<char>());
        prof_end(c);
        return BMBS_OK;
    }
    // `bytes` at src, which the lane's stream is still writing, go down into the caller's buffer; the call is counted (bmbs_text_times)
    int deliver(const char* src, u64 bytes)
    {
        if (text_trace()) { HIPCHK(c, hipStreamSynchronize(c->stream)); t.written = wall(); }
        double cs = 0;
        const double t_dn0 = wall();
        const int rc = download_locked(c, sam, src, bytes, c->stream, &cs);
        if (rc) return rc;
        c->link_down_s += cs;
        t.delivered = wall();
        t.down_wait = t.delivered - cs - t_dn0;
        c->text_call_s += t.delivered - t.start; c->text_calls++;
        return BMBS_OK;
    }
    // ---- records -> BAM records, all on the device (bmbs_bam.hip): the stream in bam_raw, *raw_total its bytes (0: nothing prints)
    int bam_records(u64* raw_total)
    {
        const int rc = sized<true>(raw_total);
        if (rc) return rc;
        if (n_lines_out) *n_lines_out = (int64_t)n2;
        const u32 long_name = c->h_info->line[3];
        if (long_name) { c->err = "output line " + std::to_string(long_name - 1) + " of this batch has a read name of more than 254 characters: BAM cannot hold it"; return BMBS_EINVAL; }
        if (!*raw_total) { if (flags & BMBS_TEXT_BAM_SORTED) c->st.holds(0, (int64_t)n2, pe); return BMBS_OK; }
        return write<true>(c->bam_raw, *raw_total);
    }
    // ---- ... -> BGZF blocks
    int emit_bam(u64 raw_total)
    {
        u64 ztotal = 0;
        int rc = bgzf_deflate(c, c->bam_raw.as<char>(), tot_at(c, TOT_BAM_BYTES), raw_total, &ztotal);
        if (rc) return rc;
        if (sam_bytes) *sam_bytes = ztotal;
        if (ztotal > sam_cap) return too_small("text call: the BAM buffer is too small (sam_bytes tells what this batch needs)");
        rc = bgzf_collect(c, raw_total, ztotal);
        if (rc) return rc;
        rc = deliver(c->sam_out.as<char>(), ztotal);
        if (!rc && text_trace())
            fprintf(stderr, "[text/bam] n=%ld in=%.1fMB records=%.1fMB out=%.1fMB  upload %.2f lines+records %.2f rows+map %.2f  len+scan %.2f  write+deflate %.2f  download %.2f  total %.2f ms\n",
                    (long)n2, (double)in_bytes / 1e6, (double)raw_total / 1e6, (double)ztotal / 1e6, (t.uploaded - t.start) * 1e3, (t.records - t.uploaded) * 1e3, (t.mapped - t.records) * 1e3, (t.sized - t.mapped) * 1e3,
                    (t.written - t.sized) * 1e3, (t.delivered - t.written) * 1e3, (t.delivered - t.start) * 1e3);
        return rc;
    }
    // ---- ... -> the uncompressed records in coordinate order (k_bamsort.hip); a driver merges the batches (bmbs_bam_sort)
    int emit_sorted(u64 raw_total)
    {
        if (sam_bytes) *sam_bytes = raw_total;
        if (raw_total > sam_cap) return too_small("text call: the BAM buffer is too small (sam_bytes tells what this batch needs)");
        u64 n_rec = 0;
        int rc = bam_sort_device(c, c->bam_raw.as<char>(), c->sam_off.as<u64>(), c->sam_len.as<u32>(), n2, raw_total, true, &n_rec);
        if (rc) return rc;
        c->st.holds((int64_t)n_rec, (int64_t)n2, pe);                         // (bmbs_text_sorted_dup: computed when asked for)
        rc = deliver(c->bs_sorted.as<char>(), raw_total);
        if (!rc && text_trace())
            fprintf(stderr, "[text/bam sorted] n=%ld in=%.1fMB records=%.1fMB  upload %.2f lines+records %.2f rows+map %.2f  len+scan %.2f  write+sort %.2f  download %.2f  total %.2f ms\n",
                    (long)n2, (double)in_bytes / 1e6, (double)raw_total / 1e6, (t.uploaded - t.start) * 1e3, (t.records - t.uploaded) * 1e3, (t.mapped - t.records) * 1e3, (t.sized - t.mapped) * 1e3,
                    (t.written - t.sized) * 1e3, (t.delivered - t.written) * 1e3, (t.delivered - t.start) * 1e3);
        return rc;
    }
    // ---- records -> SAM text
    int emit_sam()
    {
        u64 total = 0;
        int rc = sized<false>(&total);
        if (rc) return rc;
        if (sam_bytes) *sam_bytes = total;
        if (n_lines_out) *n_lines_out = (int64_t)n2;
        if (total > sam_cap) return too_small("text call: the SAM buffer is too small (sam_bytes tells what this batch needs)");
        if (!total) return BMBS_OK;
        rc = write<false>(c->sam_out, total);
        if (rc) return rc;
        rc = deliver(c->sam_out.as<char>(), total);
        // ("up", the wait for the upload lock, has never been measured: it prints the 0.00 it always has, and the line keeps its fields)
        if (!rc && text_trace())
            fprintf(stderr, "[text] n=%ld in=%.1fMB out=%.1fMB  (waits for the link: up %.2f, down %.2f)  upload %.2f lines %.2f  records %.2f  rows+map %.2f  len+scan %.2f  write %.2f  download %.2f  total %.2f ms\n",
                    (long)n2, (double)in_bytes / 1e6, (double)total / 1e6, 0.0, t.down_wait * 1e3, (t.uploaded - t.start) * 1e3, (t.lines - t.uploaded) * 1e3, (t.records - t.lines) * 1e3, (t.mapped - t.records) * 1e3,
                    (t.sized - t.mapped) * 1e3, (t.written - t.sized) * 1e3, (t.delivered - t.written) * 1e3, (t.delivered - t.start) * 1e3);
        return rc;
    }
};

// record fields, rows, mapping, then SAM text, BAM blocks or sorted BAM records, and their download; t0: the caller's start and uploaded marks
int lane_text_finish(Lane* c, bool pe, u64 bytes1, u64 bytes2, int64_t n_records, int32_t flags_in, char* sam, u64 sam_cap, u64* sam_bytes,
                     int64_t* n_lines_out, const TextClock& t0)
{
    c->ends(Lane::TEXT_LINES);
    const u64 n = (u64)n_records;
    TextCall T = {c, pe, bytes1 + bytes2, n, pe ? 2 * n : n, flags_in, sam, sam_cap, sam_bytes, n_lines_out, t0, {}, 0, {}};
    int maxL = 0, minL = 0;
    int rc = T.records(&maxL, &minL);
    // trimming left nothing: as a call without records (no mapping launch sees an empty batch)
    if (!rc && !T.n) { if (flags_in & BMBS_TEXT_BAM_SORTED) c->st.holds(0, 0, pe); return BMBS_OK; }
    if (!rc) rc = T.map(maxL, minL == maxL);
    if (rc) return rc;
    if (!(flags_in & BMBS_TEXT_BAM)) return T.emit_sam();
    u64 raw_total = 0;
    rc = T.bam_records(&raw_total);
    if (rc || !raw_total) return rc;
    return flags_in & BMBS_TEXT_BAM_SORTED ? T.emit_sorted(raw_total) : T.emit_bam(raw_total);
}

// what lane_map_text and lane_text_map_open begin with: nothing has been written yet; a sorted call needs BMBS_TEXT_BAM, and, whatever
// becomes of it, ends what the last one left
static int text_call_begin(Lane* c, int32_t flags_in, u64* sam_bytes, int64_t* n_lines_out)
{
    if (sam_bytes) *sam_bytes = 0;
    if (n_lines_out) *n_lines_out = 0;
    c->trim.counted = false;                            // (bmbs_text_trim_counts describes THIS call from here on, whatever becomes of it)
    if ((flags_in & BMBS_TEXT_BAM_SORTED) && !(flags_in & BMBS_TEXT_BAM)) { c->err = "text call: BMBS_TEXT_BAM_SORTED is only valid together with BMBS_TEXT_BAM"; return BMBS_EINVAL; }
    if (flags_in & BMBS_TEXT_BAM_SORTED) c->ends(Lane::SORTED_TEXT_CALL);
    return BMBS_OK;
}

int lane_map_text(Lane* c, bool pe, const char* text1, u64 bytes1, const char* text2, u64 bytes2, int64_t n_records, int32_t flags_in, char* sam,
                  u64 sam_cap, u64* sam_bytes, int64_t* n_lines_out)
{
    if (!c) return BMBS_EINVAL;
    { const int r0 = text_call_begin(c, flags_in, sam_bytes, n_lines_out); if (r0) return r0; }
    if (!c->attached) { c->err = "no index attached"; return BMBS_ESTATE; }
    if (c->n_refs != c->ix.n_chrom) { c->err = "bmbs_sam_refs has not been given the index's reference names"; return BMBS_ESTATE; }
    if (n_records <= 0) { if (flags_in & BMBS_TEXT_BAM_SORTED) c->st.holds(0, 0, pe); return BMBS_OK; }
    if (!text1 || (pe && !text2) || !sam) { c->err = "text call: NULL buffer"; return BMBS_EINVAL; }
    if (bytes1 >= (1ull << 32) || bytes2 >= (1ull << 32)) { c->err = "a text window has to be smaller than 4 GiB (32-bit offsets)"; return BMBS_EINVAL; }
    HIPCHK(c, hipSetDevice(c->dev));
    { const int rs = lane_settle(c); if (rs) return rs; }
    c->open_text.valid = false;
    TextClock t; t.start = wall();
    HIPCHK(c, hipMemsetAsync(c->tx_info.p, 0, TXI_WORDS * sizeof(u32), c->stream));
    ENS(c, c->fq_text1, bytes1 + text_pad(c));
    if (pe) ENS(c, c->fq_text2, bytes2 + text_pad(c));
    {
        // the link is claimed for the copies alone: the kernels behind them may have to queue behind other contexts' kernels
        std::lock_guard<std::mutex> up(g_h2d_mu[c->dev & 15]);
        const double t_up0 = wall();
        // on a stream of their own that never carries a kernel (the lane has nothing in flight here: the previous call ended with a wait)
        hipStream_t us = up_stream_of(c);
        HIPCHK(c, hipMemcpyAsync(c->fq_text1.p, text1, bytes1, hipMemcpyHostToDevice, us));
        if (pe) HIPCHK(c, hipMemcpyAsync(c->fq_text2.p, text2, bytes2, hipMemcpyHostToDevice, us));
        HIPCHK(c, hipStreamSynchronize(us));
        c->link_up_s += wall() - t_up0;
    }
    t.uploaded = text_trace() ? wall() : 0;
    // diagnostic (tools/e2e_trace.sh): BMBS_TEXT_COPY_ONLY=1 moves the bytes of a batch over the link and runs nothing in between
    static const bool copy_only = getenv("BMBS_TEXT_COPY_ONLY") != nullptr;
    if (copy_only) {
        const u64 total = std::min<u64>(sam_cap, (bytes1 + bytes2) * 115 / 100);
        ENS(c, c->sam_out, total + 64);
        std::lock_guard<std::mutex> down(g_d2h_mu[c->dev & 15]);
        const int rd = d2h_chunked(c, sam, c->sam_out.as<char>(), total, c->stream);
        if (rd) return rd;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (sam_bytes) *sam_bytes = 0;
        if (text_trace()) fprintf(stderr, "[text] copy only: upload %.2f download %.2f ms\n", (t.uploaded - t.start) * 1e3, (wall() - t.uploaded) * 1e3);
        return BMBS_OK;
    }
    int rc = text_index(c, c->fq_text1, bytes1, (u64)n_records, 0);
    if (rc) return rc;
    if (pe) { rc = text_index(c, c->fq_text2, bytes2, (u64)n_records, 1); if (rc) return rc; }
    return lane_text_finish(c, pe, bytes1, bytes2, n_records, flags_in, sam, sam_cap, sam_bytes, n_lines_out, t);
}

// the part of an "open" call behind the inflated text (bytes[f] of it in fq_text1 / fq_text2): newline index, whole records, what is left behind them
static int lane_text_open_finish(Lane* c, bool pe, const u64* bytes, int64_t max_records, int64_t* n_records, char* tail1, uint64_t tail_cap,
                                 uint64_t* tail1_bytes, char* tail2, uint64_t* tail2_bytes, TextClock& t, double comp_mb)
{
    DevBuf* const texts[2] = {&c->fq_text1, &c->fq_text2};
    const u64 n_cap = (u64)max_records;
    int rc = text_index(c, c->fq_text1, bytes[0], n_cap, 0);
    if (rc) return rc;
    if (pe) { rc = text_index(c, c->fq_text2, bytes[1], n_cap, 1); if (rc) return rc; }
    const u64* const lines = c->h_info->lines;
    HIPCHK(c, hipMemcpyAsync(c->h_info->lines, tot_at(c, TOT_LINES_1), sizeof c->h_info->lines, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    t.lines = wall();
    u64 n = lines[0] / 4;
    if (pe) n = std::min(n, lines[1] / 4);
    n = std::min(n, n_cap);
    // the text behind the n records: handed back for the next window
    u64 cut[2] = {0, 0};
    if (n) {
        for (int f = 0; f < (pe ? 2 : 1); f++) HIPCHK(c, hipMemcpyAsync(&c->h_info->last_nl[f], c->tx_nl[f].as<u32>() + (4 * n - 1), sizeof(u32), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int f = 0; f < (pe ? 2 : 1); f++) cut[f] = (u64)c->h_info->last_nl[f] + 1;
    }
    hipStream_t ds = down_stream_of(c);
    char* tails[2] = {tail1, tail2}; uint64_t* tb[2] = {tail1_bytes, tail2_bytes};
    for (int f = 0; f < (pe ? 2 : 1); f++) *tb[f] = bytes[f] - cut[f];                   // (both sizes are known to a caller that has to come back with room)
    for (int f = 0; f < (pe ? 2 : 1); f++)
        if (*tb[f] > tail_cap) { c->err = "text open: the tail buffer is too small (" + std::to_string(*tb[f]) + " bytes behind the window's records)"; return BMBS_ENOMEM; }
    for (int f = 0; f < (pe ? 2 : 1); f++)
        if (*tb[f]) HIPCHK(c, hipMemcpyAsync(tails[f], texts[f]->as<char>() + cut[f], *tb[f], hipMemcpyDeviceToHost, ds));
    HIPCHK(c, hipStreamSynchronize(ds));
    t.delivered = wall();
    if (text_trace())
        fprintf(stderr, "[text open bgzf] n=%ld comp=%.1fMB text=%.1fMB  upload+inflate %.2f  lines %.2f  tails %.2f (%.2f MB)  total %.2f ms\n", (long)n,
                comp_mb, (double)(bytes[0] + bytes[1]) / 1e6, (t.uploaded - t.start) * 1e3, (t.lines - t.uploaded) * 1e3, (t.delivered - t.lines) * 1e3,
                (double)(*tb[0] + (pe ? *tb[1] : 0)) / 1e6, (t.delivered - t.start) * 1e3);
    *n_records = (int64_t)n;
    c->open_text.valid = n > 0; c->open_text.pe = pe; c->open_text.bytes1 = cut[0]; c->open_text.bytes2 = cut[1]; c->open_text.n = (int64_t)n;
    return BMBS_OK;
}

// ---- BGZF blocks on the device (bmbs_inflate.hip): what bmbs_text_open_bgzf and bmbs_inflate_bgzf check alike
// every block has room for its header and trailer and inflates to at most 64 KiB, the offsets ascend; `who` begins the message
static int blk_table_check(Lane* c, const char* who, const uint64_t* blk_off, const uint64_t* out_off, u64 nb)
{
    for (u64 i = 0; i < nb; i++)
        if (blk_off[i + 1] < blk_off[i] + 26 || out_off[i + 1] < out_off[i] || out_off[i + 1] - out_off[i] > 65536) { c->err = std::string(who) + ": malformed block table"; return BMBS_EINVAL; }
    return BMBS_OK;
}
// k_bgzf_inflate's word per block, on the host: the first block that did not inflate is reported; file 1 / 2: the text-open call's
// input files, 0: the plain inflate call's
static int blk_errors(Lane* c, const u32* err, u64 nb, int file)
{
    for (u64 i = 0; i < nb; i++)
        if (err[i]) { c->err = "corrupt BGZF block in the .gz input (" + (file ? "file " + std::to_string(file) + ", " : std::string()) + "block " + std::to_string(i) + " of this window, code " + std::to_string(err[i]) + ")"; return BMBS_EINVAL; }
    return BMBS_OK;
}

// ---- compressed input that stays on the device: open (assemble + index a window from BGZF blocks) and map (everything after) -------
// one input file of an open call: its arguments, the lane's buffers for it, its blocks; bytes = prefix + inflated text
struct ZTextArgs { const bmbs_ztext* z; DevBuf* text; DevBuf* comp; DevBuf* off; DevBuf* err; u64 nb, bytes; };

// upload, inflate, last line of file f, all on stream s
static int ztext_inflate(Lane* c, const ZTextArgs& a, int f, int32_t last, hipStream_t s)
{
    const bmbs_ztext* z = a.z;
    const u64 nb = a.nb;
    if (z->prefix_bytes) HIPCHK(c, hipMemcpyAsync(a.text->p, z->prefix, z->prefix_bytes, hipMemcpyHostToDevice, s));
    if (nb) {
        HIPCHK(c, hipMemcpyAsync(a.comp->p, z->comp, z->comp_bytes, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(a.off->p, z->blk_off, (nb + 1) * 8, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(a.off->as<u64>() + (nb + 1), z->out_off, (nb + 1) * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)nb), dim3(64), 0, s, a.comp->as<u8>(), a.off->as<u64>(), a.off->as<u64>() + (nb + 1), (long)nb,
                           a.text->as<char>() + z->prefix_bytes, a.err->as<u32>());
    }
    if (last && a.bytes) {
        // an unterminated last line counts as a line (the reader's rule): the newline is added here, on the device
        hipLaunchKernelGGL(k_close_last_line, dim3(1), dim3(1), 0, s, a.text->as<char>(), a.bytes, tot_at(c, tot_file(TOT_NL_ADDED_1, f)));
    } else HIPCHK(c, hipMemsetAsync(tot_at(c, tot_file(TOT_NL_ADDED_1, f)), 0, sizeof(u64), s));
    return BMBS_OK;
}

int lane_text_open_bgzf(Lane* c, const bmbs_ztext* z1, const bmbs_ztext* z2, int64_t max_records, int32_t last1, int32_t last2, int64_t* n_records,
                        char* tail1, uint64_t tail_cap, uint64_t* tail1_bytes, char* tail2, uint64_t* tail2_bytes)
{
    if (!c) return BMBS_EINVAL;
    if (n_records) *n_records = 0;
    if (tail1_bytes) *tail1_bytes = 0;
    if (tail2_bytes) *tail2_bytes = 0;
    c->open_text.valid = false;
    if (!c->attached) { c->err = "no index attached"; return BMBS_ESTATE; }
    if (!z1 || max_records <= 0 || !n_records || !tail1 || !tail1_bytes || (z2 && (!tail2 || !tail2_bytes))) { c->err = "text open: NULL argument"; return BMBS_EINVAL; }
    HIPCHK(c, hipSetDevice(c->dev));
    { const int rs = lane_settle(c); if (rs) return rs; }
    const bool pe = z2 != nullptr;
    ZTextArgs A[2] = {{z1, &c->fq_text1, &c->z_comp, &c->z_off, &c->z_err, 0, 0}, {z2, &c->fq_text2, &c->z_comp2, &c->z_off2, &c->z_err2, 0, 0}};
    const int32_t last[2] = {last1, last2};
    TextClock t; t.start = wall();
    HIPCHK(c, hipMemsetAsync(c->tx_info.p, 0, TXI_WORDS * sizeof(u32), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // each file on a stream of its own: upload, inflate (one wave per block: a launch of one file's blocks leaves most of the chip's
    // wave slots empty, so the two files' launches run side by side), last line
    hipStream_t fs[2] = {c->stream, up_stream_of(c)};
    for (int f = 0; f < (pe ? 2 : 1); f++) {
        // the file's buffers and block table checked, the lane's buffers sized
        ZTextArgs& a = A[f];
        const bmbs_ztext* z = a.z;
        const u64 nb = a.nb = (u64)std::max<int64_t>(0, z->n_blocks);
        if ((z->prefix_bytes && !z->prefix) || (nb && (!z->comp || !z->blk_off || !z->out_off))) { c->err = "text open: NULL buffer"; return BMBS_EINVAL; }
        if (nb && z->blk_off[nb] > z->comp_bytes) { c->err = "text open: block table outside the compressed bytes"; return BMBS_EINVAL; }
        { const int rc = blk_table_check(c, "text open", z->blk_off, z->out_off, nb); if (rc) return rc; }
        // (the text has to be contiguous behind the prefix: the inflate kernel takes any byte offset, and the line kernels read the
        // window from its 16-byte aligned start)
        a.bytes = z->prefix_bytes + (nb ? z->out_off[nb] : 0);
        if (a.bytes + 1 >= (1ull << 32)) { c->err = "a text window has to be smaller than 4 GiB (32-bit offsets)"; return BMBS_EINVAL; }
        ENS(c, *a.text, a.bytes + text_pad(c) + 16);
        if (nb) { ENS(c, *a.comp, z->comp_bytes + 1024); ENS(c, *a.off, 2 * (nb + 1) * 8 + 64); ENS(c, *a.err, nb * 4 + 64); }
    }
    for (int f = 0; f < (pe ? 2 : 1); f++) { const int rc = ztext_inflate(c, A[f], f, last[f], fs[f]); if (rc) return rc; }
    if (pe && fs[1] != c->stream) HIPCHK(c, hipStreamSynchronize(fs[1]));
    // whether a newline was added has to be known before the lines are indexed
    HIPCHK(c, hipMemcpyAsync(c->h_info->nl_added, tot_at(c, TOT_NL_ADDED_1), sizeof c->h_info->nl_added, hipMemcpyDeviceToHost, c->stream));
    std::vector<u32> err[2];
    for (int f = 0; f < (pe ? 2 : 1); f++) {
        err[f].resize(A[f].nb);
        if (A[f].nb) HIPCHK(c, hipMemcpyAsync(err[f].data(), A[f].err->p, A[f].nb * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int f = 0; f < (pe ? 2 : 1); f++) { const int rc = blk_errors(c, err[f].data(), err[f].size(), f + 1); if (rc) return rc; }
    t.uploaded = wall();
    const u64* const added = c->h_info->nl_added;
    const u64 bytes[2] = {A[0].bytes + added[0], pe ? A[1].bytes + added[1] : 0};
    return lane_text_open_finish(c, pe, bytes, max_records, n_records, tail1, tail_cap, tail1_bytes, tail2, tail2_bytes, t, (double)(z1->comp_bytes + (z2 ? z2->comp_bytes : 0)) / 1e6);
}

int lane_text_map_open(Lane* c, int32_t flags_in, char* sam, u64 sam_cap, u64* sam_bytes, int64_t* n_lines_out)
{
    if (!c) return BMBS_EINVAL;
    { const int r0 = text_call_begin(c, flags_in, sam_bytes, n_lines_out); if (r0) return r0; }
    if (!c->open_text.valid) { c->err = "text map: no open batch (bmbs_text_open_bgzf first)"; return BMBS_ESTATE; }
    if (c->n_refs != c->ix.n_chrom) { c->err = "bmbs_sam_refs has not been given the index's reference names"; return BMBS_ESTATE; }
    if (!sam) { c->err = "text call: NULL buffer"; return BMBS_EINVAL; }
    if (c->trim.on && (c->fq_text1.cap < c->open_text.bytes1 + text_pad(c) || (c->open_text.pe && c->fq_text2.cap < c->open_text.bytes2 + text_pad(c)))) {
        c->err = "text map: the batch was opened before trimming was turned on (bmbs_set_trim comes before bmbs_text_open_bgzf)"; return BMBS_ESTATE;
    }
    HIPCHK(c, hipSetDevice(c->dev));
    TextClock t; t.start = t.uploaded = wall();
    // (an output buffer that turns out too small leaves the batch open: the call can be repeated)
    const int rc = lane_text_finish(c, c->open_text.pe, c->open_text.bytes1, c->open_text.bytes2, c->open_text.n, flags_in, sam, sam_cap, sam_bytes, n_lines_out, t);
    if (rc != BMBS_ENOMEM) c->open_text.valid = false;
    return rc;
}

// ---- trimming: the options, the last call's counters, the stage alone
static int trim_opts_check(std::string& err, const bmbs_trim_opts* o)
{
    if (o->quality < 0 || o->min_overlap < 0 || o->error_permille < 0 || o->min_length < 0 || o->clip_5p[0] < 0 || o->clip_5p[1] < 0 || o->clip_3p[0] < 0 || o->clip_3p[1] < 0) {
        err = "trim options: a negative value"; return BMBS_EINVAL;
    }
    if (o->min_length < 1) { err = "trim options: min_length has to be at least 1"; return BMBS_EINVAL; }
    if (o->error_permille > 1000) { err = "trim options: error_permille outside 0..1000"; return BMBS_EINVAL; }
    if (o->quality > 255) { err = "trim options: quality above 255"; return BMBS_EINVAL; }
    for (int m = 0; m < 2; m++) {
        if (o->clip_5p[m] > 65535 || o->clip_3p[m] > 65535) { err = "trim options: a clip above 65535"; return BMBS_EINVAL; }
        if (!memchr(o->adapter[m], 0, sizeof o->adapter[m])) { err = "trim options: an adapter of more than 32 letters"; return BMBS_EINVAL; }
        for (const char* p = o->adapter[m]; *p; p++)
            if (!strchr("ACGTacgt", *p)) { err = std::string("trim options: adapter letter '") + *p + "' of mate " + std::to_string(m + 1) + " is not one of ACGT"; return BMBS_EINVAL; }
    }
    return BMBS_OK;
}
extern "C" int bmbs_set_trim(bmbs_ctx* X, const bmbs_trim_opts* opts)
{
    if (!X) return BMBS_EINVAL;
    if (opts) { const int rc = trim_opts_check(X->err, opts); if (rc) return rc; }
    for (Lane* c : X->lanes) { c->trim.on = opts != nullptr; if (opts) c->trim.opts = *opts; }
    return BMBS_OK;
}
extern "C" int bmbs_text_trim_counts(bmbs_ctx* X, bmbs_trim_counts* counts, int64_t* n_kept)
{
    Lane* c = lane0(X);
    if (!c) return BMBS_EINVAL;
    if (!c->trim.counted) { c->err = "trim counts: the context has made no text call with trimming on"; return fin(X, c, BMBS_ESTATE); }
    if (counts) *counts = c->trim.cnt;
    if (n_kept) *n_kept = c->trim.kept;
    return BMBS_OK;
}
static int lane_trim_text(Lane* c, const char* text, u64 bytes, int64_t n_records, int32_t mate, uint32_t* seq_off, uint32_t* qual_off, uint16_t* seq_len, uint16_t* qual_len)
{
    if (!c->trim.on) { c->err = "trim text: trimming is off (bmbs_set_trim)"; return BMBS_ESTATE; }
    if (n_records <= 0) return BMBS_OK;
    if (!text || !seq_off || !qual_off || !seq_len || !qual_len || mate < 0 || mate > 1) { c->err = "trim text: bad argument"; return BMBS_EINVAL; }
    if (bytes >= (1ull << 32)) { c->err = "a text window has to be smaller than 4 GiB (32-bit offsets)"; return BMBS_EINVAL; }
    HIPCHK(c, hipSetDevice(c->dev));
    { const int rs = lane_settle(c); if (rs) return rs; }
    c->open_text.valid = false;                     // (the window of an open batch is overwritten)
    const u64 n = (u64)n_records;
    HIPCHK(c, hipMemsetAsync(c->tx_info.p, 0, TXI_WORDS * sizeof(u32), c->stream));
    ENS(c, c->fq_text1, bytes + text_pad(c));
    HIPCHK(c, hipMemcpyAsync(c->fq_text1.p, text, bytes, hipMemcpyHostToDevice, c->stream));
    int rc = text_index(c, c->fq_text1, bytes, n, 0);
    if (rc) return rc;
    FqRec rec;
    rc = fq_rec_setup(c, n, 0, rec);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->h_info->lines, tot_at(c, TOT_LINES_1), sizeof c->h_info->lines, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->h_info->lines[0] < 4 * n) { c->err = "trim text: the text holds fewer than 4 lines per record"; return BMBS_EINVAL; }
    hipLaunchKernelGGL(k_fq_records, dim3(nblk(n, 256)), dim3(256), 0, c->stream, c->tx_nl[0].as<u32>(), (long)n, rec, line_info(c));
    rc = trim_begin(c, n);
    if (rc) return rc;
    trim_file(c, c->fq_text1.as<char>(), rec, n, 0, mate, 1);
    HIPCHK(c, hipMemcpyAsync(c->h_info->line, line_info(c), sizeof c->h_info->line, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(seq_off, rec.seq_off, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(qual_off, rec.qual_off, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(seq_len, rec.seq_len, n * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(qual_len, rec.qual_len, n * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->h_info->line[2]) { c->err = "record " + std::to_string(c->h_info->line[2] - 1) + " of this text has an empty or longer-than-" + std::to_string(BMBS_MAX_READ) + "-character sequence line"; return BMBS_EINVAL; }
    return BMBS_OK;
}
extern "C" int bmbs_trim_text(bmbs_ctx* X, const char* text, uint64_t text_bytes, int64_t n_records, int32_t mate, uint32_t* seq_off, uint32_t* qual_off,
                              uint16_t* seq_len, uint16_t* qual_len)
{ ON_LANE0(lane_trim_text(c, text, text_bytes, n_records, mate, seq_off, qual_off, seq_len, qual_len)); }

// RNAME table of the SAM text: the names behind the index's sequences, in index order
int lane_sam_refs(Lane* c, const char* const* names, int n_names)
{
    if (!names || n_names < 1) { c->err = "sam refs: no names"; return BMBS_EINVAL; }
    HIPCHK(c, hipSetDevice(c->dev));
    std::vector<u32> off((size_t)n_names + 1, 0);
    std::string chars;
    int mx = 0;
    for (int i = 0; i < n_names; i++) {
        const size_t l = names[i] ? strlen(names[i]) : 0;
        if (l > 4096) { c->err = "sam refs: a reference name is longer than 4096 characters"; return BMBS_EINVAL; }
        chars.append(names[i] ? names[i] : "", l);
        off[(size_t)i + 1] = (u32)chars.size();
        mx = std::max(mx, (int)l);
    }
    ENS(c, c->chrom_chars, chars.size() + 64); ENS(c, c->chrom_off, off.size() * 4);
    HIPCHK(c, hipMemcpy(c->chrom_chars.p, chars.data(), chars.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->chrom_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    c->n_refs = n_names; c->max_ref_len = mx;
    return BMBS_OK;
}

// bgzip'ed input inflated on the device (bmbs_inflate.hip): needs no index
static int lane_inflate_bgzf(Lane* c, const void* comp, uint64_t comp_bytes, const uint64_t* blk_off, const uint64_t* out_off, int64_t n_blocks,
                             char* text, uint64_t text_bytes, uint32_t* nl_per_64k, uint64_t window_shift)
{
    if (n_blocks <= 0) return BMBS_OK;
    if (!comp || !blk_off || !out_off || !text) { c->err = "inflate: NULL buffer"; return BMBS_EINVAL; }
    const u64 n = (u64)n_blocks;
    if (blk_off[n] > comp_bytes || out_off[n] > text_bytes) { c->err = "inflate: block table outside the buffers"; return BMBS_EINVAL; }
    { const int r0 = blk_table_check(c, "inflate", blk_off, out_off, n); if (r0) return r0; }
    HIPCHK(c, hipSetDevice(c->dev));
    const double t0 = wall();
    ENS(c, c->z_comp, comp_bytes + 1024); ENS(c, c->z_off, 2 * (n + 1) * 8 + 64); ENS(c, c->z_text, out_off[n] + 64); ENS(c, c->z_err, n * 4 + 64);
    hipStream_t us = up_stream_of(c), ds = down_stream_of(c);
    HIPCHK(c, hipMemcpyAsync(c->z_comp.p, comp, comp_bytes, hipMemcpyHostToDevice, us));
    HIPCHK(c, hipMemcpyAsync(c->z_off.p, blk_off, (n + 1) * 8, hipMemcpyHostToDevice, us));
    HIPCHK(c, hipMemcpyAsync(c->z_off.as<u64>() + (n + 1), out_off, (n + 1) * 8, hipMemcpyHostToDevice, us));
    HIPCHK(c, hipStreamSynchronize(us));
    const double t1 = wall();
    hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)n), dim3(64), 0, c->stream, c->z_comp.as<u8>(), c->z_off.as<u64>(), c->z_off.as<u64>() + (n + 1), (long)n,
                       c->z_text.as<char>(), c->z_err.as<u32>());
    const u64 n_cnt = nl_per_64k ? (window_shift + out_off[n] + 65535) >> 16 : 0;
    if (n_cnt) {
        ENS(c, c->z_nl, n_cnt * 4 + 64);
        hipLaunchKernelGGL(k_nl_count64k, dim3((unsigned)n_cnt), dim3(256), 0, c->stream, c->z_text.as<char>(), out_off[n], window_shift, c->z_nl.as<u32>());
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double t2 = wall();
    std::vector<u32> err(n);
    HIPCHK(c, hipMemcpyAsync(err.data(), c->z_err.p, n * 4, hipMemcpyDeviceToHost, ds));
    if (n_cnt) HIPCHK(c, hipMemcpyAsync(nl_per_64k, c->z_nl.p, n_cnt * 4, hipMemcpyDeviceToHost, ds));
    const int rc = d2h_chunked(c, text, c->z_text.as<char>(), out_off[n], ds);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(ds));
    if (text_trace()) fprintf(stderr, "[inflate] %lu blocks, %.1f MB -> %.1f MB: alloc+upload %.2f  kernel %.2f  download %.2f ms\n", (unsigned long)n, (double)comp_bytes / 1e6, (double)out_off[n] / 1e6,
                              (t1 - t0) * 1e3, (t2 - t1) * 1e3, (wall() - t2) * 1e3);
    return blk_errors(c, err.data(), n, 0);
}

extern "C" int bmbs_inflate_bgzf(bmbs_ctx* X, const void* comp, uint64_t comp_bytes, const uint64_t* blk_off, const uint64_t* out_off, int64_t n_blocks,
                                 char* text, uint64_t text_bytes, uint32_t* nl_per_64k, uint64_t window_shift)
{
    Lane* c = lane0(X);
    if (!c) return BMBS_EINVAL;
    return fin(X, c, lane_inflate_bgzf(c, comp, comp_bytes, blk_off, out_off, n_blocks, text, text_bytes, nl_per_64k, window_shift));
}

#ifdef INF_PROFILE
// profiling build only (tools/inflate_prof.sh): the phase cycle sums of k_bgzf_inflate since the last call
extern "C" int bmbs_debug_inflate_prof(uint64_t* out16)
{
    unsigned long long z[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_inf_prof), sizeof z) != hipSuccess) return BMBS_ENODEV;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_inf_prof), z, sizeof z) == hipSuccess ? BMBS_OK : BMBS_ENODEV;
}
#endif

#ifdef BGZF_PROFILE
// profiling build only (tools/bgzf_prof.sh): the phase cycle sums of k_bgzf_block since the last call
extern "C" int bmbs_debug_bgzf_prof(uint64_t* out8)
{
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_bgzf_prof), sizeof z) != hipSuccess) return BMBS_ENODEV;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_bgzf_prof), z, sizeof z) == hipSuccess ? BMBS_OK : BMBS_ENODEV;
}
#endif

// diagnostic: the Huffman code lengths the device's BGZF deflater gives a table of symbol frequencies (n <= 320, maxbits <= 15)
extern "C" int bmbs_debug_huff_lengths(bmbs_ctx* X, const uint32_t* freq, int32_t n, int32_t maxbits, uint8_t* len_out)
{
    Lane* c = lane0(X);
    if (!c) return BMBS_EINVAL;
    if (!freq || !len_out || n < 2 || n > 320 || maxbits < 2 || maxbits > 15) { c->err = "huff lengths: bad argument"; return fin(X, c, BMBS_EINVAL); }
    if (hipSetDevice(c->dev) != hipSuccess) return BMBS_ENODEV;
    u32* df = nullptr; u8* dl = nullptr;
    if (hipMalloc((void**)&df, 321 * 4) != hipSuccess || hipMalloc((void**)&dl, 320) != hipSuccess) { if (df) (void)hipFree(df); return BMBS_ENOMEM; }
    int rc = BMBS_OK;
    u32 differ = 0;
    if (hipMemcpy(df, freq, (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemset(df + 320, 0, 4) != hipSuccess) rc = BMBS_ENODEV;
    if (!rc) { hipLaunchKernelGGL(k_debug_huff, dim3(1), dim3(256), 0, c->stream, df, n, maxbits, dl, df + 320); if (hipStreamSynchronize(c->stream) != hipSuccess) rc = BMBS_ENODEV; }
    if (!rc && (hipMemcpy(len_out, dl, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&differ, df + 320, 4, hipMemcpyDeviceToHost) != hipSuccess)) rc = BMBS_ENODEV;
    (void)hipFree(df); (void)hipFree(dl);
    if (!rc && differ) { c->err = "huff lengths: the workgroup forms (huff_lengths_block / huff_codes_block) differ from the serial ones"; return fin(X, c, BMBS_ESTATE); }
    return rc;
}

// diagnostic: seconds the context's text calls held the link (uploads, downloads: copy + wait for its end, the wait for the link's lock
// excluded), seconds inside those calls, and their number
extern "C" int bmbs_text_times(bmbs_ctx* X, double out[4])
{
    if (!X || !out) return BMBS_EINVAL;
    out[0] = out[1] = out[2] = out[3] = 0;
    for (Lane* c : X->lanes) { out[0] += c->link_up_s; out[1] += c->link_down_s; out[2] += c->text_call_s; out[3] += (double)c->text_calls; }
    return BMBS_OK;
}

extern "C" int bmbs_sam_refs(bmbs_ctx* X, const char* const* names, int32_t n_names) { ON_LANE0(lane_sam_refs(c, names, n_names)); }
extern "C" int bmbs_map_se_text(bmbs_ctx* X, const char* text, uint64_t text_bytes, int64_t n_records, int32_t flags, char* sam, uint64_t sam_cap,
                                uint64_t* sam_bytes, int64_t* n_lines)
{ ON_LANE0(lane_map_text(c, false, text, text_bytes, nullptr, 0, n_records, flags, sam, sam_cap, sam_bytes, n_lines)); }
extern "C" int bmbs_text_open_bgzf(bmbs_ctx* X, const bmbs_ztext* mate1, const bmbs_ztext* mate2, int64_t max_records, int32_t last1, int32_t last2,
                                   int64_t* n_records, char* tail1, uint64_t tail_cap, uint64_t* tail1_bytes, char* tail2, uint64_t* tail2_bytes)
{ ON_LANE0(lane_text_open_bgzf(c, mate1, mate2, max_records, last1, last2, n_records, tail1, tail_cap, tail1_bytes, tail2, tail2_bytes)); }
extern "C" int bmbs_text_map_open(bmbs_ctx* X, int32_t flags, char* sam, uint64_t sam_cap, uint64_t* sam_bytes, int64_t* n_lines)
{ ON_LANE0(lane_text_map_open(c, flags, sam, sam_cap, sam_bytes, n_lines)); }
extern "C" int bmbs_map_pe_text(bmbs_ctx* X, const char* text1, uint64_t bytes1, const char* text2, uint64_t bytes2, int64_t n_pairs, int32_t flags,
                                char* sam, uint64_t sam_cap, uint64_t* sam_bytes, int64_t* n_lines)
{ ON_LANE0(lane_map_text(c, true, text1, bytes1, text2, bytes2, n_pairs, flags, sam, sam_cap, sam_bytes, n_lines)); }
extern "C" int bmbs_map_se_fastq(bmbs_ctx* X, const bmbs_fastq_view* reads, int64_t n_reads, int32_t L_max, int32_t uniform, int32_t pbat,
                                 bmbs_result* results, uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used)
{ const bmbs_fastq_view* const v[2] = {reads, nullptr}; ON_LANE0(lane_map_fastq(c, false, v, n_reads, L_max, uniform, pbat, results, cigar_pool, cigar_cap, n_cigar_used)); }
extern "C" int bmbs_map_pe_fastq(bmbs_ctx* X, const bmbs_fastq_view* mate1, const bmbs_fastq_view* mate2, int64_t n_pairs, int32_t L_max,
                                 int32_t uniform, bmbs_result* results, uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used)
{ const bmbs_fastq_view* const v[2] = {mate1, mate2}; ON_LANE0(lane_map_fastq(c, true, v, n_pairs, L_max, uniform, 0, results, cigar_pool, cigar_cap, n_cigar_used)); }

