// bitmapperbs_amd/csrc/bmbs_records.hip -- the stages behind the sorted BAM, a translation unit of its own: they take BAM records that are
// on the device already (a sorted text call's, the last bmbs_bam_sort call's) or come from the host, and sort them (bmbs_bam_sort), index
// them (k_bai.hip: bmbs_bam_sort_index), sign them for duplicate marking (k_markdup.hip: bmbs_bam_dup_sigs, bmbs_text_sorted_dup,
// bmbs_dup_select) or call cytosines in them (k_methyl.hip: bmbs_bam_methyl[_opts], bmbs_bam_sort_methyl[_opts], bmbs_methyl_sites,
// bmbs_methyl_mbias, bmbs_text_sorted_clip), find the reads the bisulfite treatment did not convert (k_nonconv.hip: bmbs_bam_nonconv,
// bmbs_text_sorted_nonconv) or write the genome-wide cytosine report from the sites of such calls (k_cytosine.hip:
// bmbs_methyl_report); bmbs_text_sorted_index hands out a sorted text call's keys.  The sort itself, the deflater
// and the download are bmbs_textpath.hip's, which the text calls run too (bmbs_host.h).  What a call leaves on the device for a later one,
// and which call ends that, is Lane::ends (bmbs_host.h).
#include "bmbs_host.h"
#define DEVI __device__ __forceinline__
#include <cassert>
#include <rocprim/device/device_radix_sort.hpp>
// (k_bai.hip reads a record's words with k_bamsort.hip's loader; that file's kernels are bmbs_textpath.hip's, so the loader is restated
// here: the two have to stay the same)
DEVI u32 bs_ld32(const char* p)
{
    return (u32)(unsigned char)p[0] | ((u32)(unsigned char)p[1] << 8) | ((u32)(unsigned char)p[2] << 16) | ((u32)(unsigned char)p[3] << 24);
}
#include "k_bai.hip"
#include "k_markdup.hip"
#include "k_methyl.hip"
#include "k_nonconv.hip"
#include "k_cytosine.hip"

// ---- what the stages share -------------------------------------------------------------------------------------------------------------------
// Entries the host describes: n_in of them, entry i = len[i] bytes of `records`, `bytes` in all.  An entry is a BAM record (36 bytes and
// more) or, with empty_ok, nothing (length 0) -- then all of them may be, and `records` may be NULL: the caller looks at it once the
// lengths are known.  pairs: entries 2p and 2p + 1 belong together
static int records_check(Lane* c, const char* what, const char* records, uint64_t bytes, const uint32_t* len, int64_t n_in, bool empty_ok, bool pairs)
{
    const std::string w = what;
    if (n_in < 0 || n_in >= (1ll << 31)) { c->err = w + ": bad argument"; return BMBS_EINVAL; }
    if (pairs && (n_in & 1)) { c->err = w + ": an odd number of entries (" + std::to_string(n_in) + ") cannot be pairs"; return BMBS_EINVAL; }
    if (n_in && (!len || (!empty_ok && !records))) { c->err = w + ": NULL buffer"; return BMBS_EINVAL; }
    u64 sum = 0;
    for (u64 i = 0; i < (u64)n_in; i++) {
        if (len[i] < 36 && !(empty_ok && !len[i])) { c->err = w + ": the length given for record " + std::to_string(i) + " is below the 36 bytes every BAM record has"; return BMBS_EINVAL; }
        sum += len[i];
    }
    if (sum != bytes) { c->err = w + ": the record lengths add up to " + std::to_string(sum) + " bytes, not to the " + std::to_string(bytes) + " given"; return BMBS_EINVAL; }
    return BMBS_OK;
}

// checked entries -> r: the bytes (padded: the kernels read whole words) and the lengths go up under the device's upload lock, the bytes
// in pieces (bmbs_textpath.hip: d2h_chunked), r.off = the exclusive scan of the lengths (its total: the word `slot`); clip, if given, -> *clip_dst
static int records_stage(Lane* c, RecIn& r, const char* records, u64 bytes, const uint32_t* len, u64 n, Tot slot, const uint32_t* clip = nullptr, DevBuf* clip_dst = nullptr)
{
    ENS(c, r.in, bytes + 256); ENS(c, r.len, n * 4 + 64); ENS(c, r.off, (n + 1) * 8 + 64);
    if (clip) ENS(c, *clip_dst, n * 4 + 64);
    {
        std::lock_guard<std::mutex> up(g_h2d_mu[c->dev & 15]);
        hipStream_t us = up_stream_of(c);
        const u64 piece = 128ull << 20;
        for (u64 o = 0; o < bytes; o += piece) HIPCHK(c, hipMemcpyAsync(r.in.as<char>() + o, records + o, std::min(piece, bytes - o), hipMemcpyHostToDevice, us));
        HIPCHK(c, hipMemcpyAsync(r.len.p, len, n * 4, hipMemcpyHostToDevice, us));
        if (clip) HIPCHK(c, hipMemcpyAsync(clip_dst->p, clip, n * 4, hipMemcpyHostToDevice, us));
        HIPCHK(c, hipStreamSynchronize(us));
    }
    return scan_u32(c, r.len.as<u32>(), n, r.off.as<u64>(), slot);
}

// One array a fetch hands back: where its count goes, the count (read once the result is known to be there), the caller's room and array.
// How every fetch begins: a NULL count is refused and every count zeroed; BMBS_ESTATE (`none`) unless the result is resident; `make`, if
// given, computes what is not there yet; then the counts are set, BMBS_ENOMEM (`small`) tells that an array is too small, and an array
// with something to receive must not be NULL.  BMBS_OK: the caller copies whatever has a count
struct FetchArr { int64_t* n_out; const int64_t* n; int64_t cap; const void* dst; };
static int fetch_begin(Lane* c, const char* what, std::initializer_list<FetchArr> a, bool resident, const char* none, const char* small, int (*make)(Lane*) = nullptr)
{
    const std::string w = what;
    for (const FetchArr& f : a) if (!f.n_out) { c->err = w + ": NULL argument"; return BMBS_EINVAL; }
    for (const FetchArr& f : a) *f.n_out = 0;
    if (!resident) { c->err = w + ": " + none; return BMBS_ESTATE; }
    if (make) { const int rc = make(c); if (rc) return rc; }
    bool room = true, all = true;
    for (const FetchArr& f : a) { *f.n_out = *f.n; room = room && *f.n <= f.cap; all = all && (!*f.n || f.dst); }
    if (!room) { c->err = w + ": " + small; return BMBS_ENOMEM; }
    if (!all) { c->err = w + ": NULL argument"; return BMBS_EINVAL; }
    return BMBS_OK;
}

// n (key, value) pairs ka / va -> kb / vb, stably sorted by the key bits below end_bit: the radix sort of rocPRIM, its scratch (as many
// bytes as pair_sort_bytes tells) in c->bs_tmp, every stage's.  The scratch may be REPLACED when it grows, so a sort still in flight has to
// be through with it first: `wait`, for a caller that has queued one on the stream.  have: bs_tmp holds that much already, nothing is asked
// or grown (bmbs_dup_select queues three sorts: room for the largest before the first).  prof: the sort's name in the profile
template <class V>
static int pair_sort_bytes(Lane* c, const char* what, u64* ka, u64* kb, V* va, V* vb, u64 n, unsigned end_bit, size_t* tmp)
{
    *tmp = 0;
    if (rocprim::radix_sort_pairs(nullptr, *tmp, ka, kb, va, vb, (size_t)n, 0u, end_bit, c->stream) != hipSuccess) { c->err = std::string(what) + ": radix_sort_pairs (size query) failed"; return BMBS_ENODEV; }
    return BMBS_OK;
}
template <class V>
static int pair_sort(Lane* c, const char* what, u64* ka, u64* kb, V* va, V* vb, u64 n, unsigned end_bit, const char* prof, bool wait, size_t have = 0)
{
    size_t tmp = have;
    if (!have) {
        if (int rc = pair_sort_bytes(c, what, ka, kb, va, vb, n, end_bit, &tmp)) return rc;
        if (wait) HIPCHK(c, hipStreamSynchronize(c->stream));
        ENS(c, c->bs_tmp, tmp + 64);
    }
    if (prof) prof_begin(c, prof);
    if (rocprim::radix_sort_pairs(c->bs_tmp.p, tmp, ka, kb, va, vb, (size_t)n, 0u, end_bit, c->stream) != hipSuccess) { c->err = std::string(what) + ": radix_sort_pairs failed"; return BMBS_ENODEV; }
    if (prof) prof_end(c);
    return BMBS_OK;
}
// bam_sort_device's pair sort (bmbs_textpath.hip calls back into this unit, so that rocPRIM's kernels are compiled into one object only)
int bam_pair_sort(Lane* c, u64* ka, u64* kb, u32* va, u32* vb, u64 n, unsigned end_bit) { return pair_sort(c, "bam sort", ka, kb, va, vb, n, end_bit, "bam_pair_sort", false); }

// Work arrays carved out of one buffer, each on a 256-byte border: make() sizes the parts and makes room for all of them, get<T>() hands
// them out in that order
struct Carve {
    u64 off[12]; char* base = nullptr; int count = 0, next = 0;
    int make(Lane* c, DevBuf& b, std::initializer_list<u64> parts)
    {
        if (parts.size() > sizeof off / sizeof off[0]) { c->err = "carve: more parts than offsets"; return BMBS_ESTATE; }
        u64 at = 0;
        for (const u64 bytes : parts) { off[count++] = at; at += (bytes + 255) & ~255ull; }
        ENS(c, b, at + 64);
        base = b.as<char>();
        return BMBS_OK;
    }
    template <class T> T* get() { assert(next < count); return reinterpret_cast<T*>(base + off[next++]); }
};

// ---- coordinate sort (k_bamsort.hip): the index of the last sorted text call, and the sort of records the host holds ----------------------
static int lane_text_sorted_index(Lane* c, uint64_t* key, uint32_t* len, int64_t cap, int64_t* n)
{
    if (int rc = fetch_begin(c, "sorted index", {{n, &c->st.n, cap, key}, {n, &c->st.n, cap, len}}, c->st.n >= 0,
                             "the context's last text call was not a BMBS_TEXT_BAM_SORTED call that returned records",
                             "the arrays are too small (n tells what is needed)")) return rc;
    if (!c->st.n) return BMBS_OK;
    HIPCHK(c, hipSetDevice(c->dev));
    hipStream_t ds = down_stream_of(c);
    HIPCHK(c, hipMemcpyAsync(key, c->bs_key2.p, (size_t)c->st.n * 8, hipMemcpyDeviceToHost, ds));
    HIPCHK(c, hipMemcpyAsync(len, c->bs_slen.p, (size_t)c->st.n * 4, hipMemcpyDeviceToHost, ds));
    HIPCHK(c, hipStreamSynchronize(ds));
    return BMBS_OK;
}

static int lane_bam_sort(Lane* c, const char* records, uint64_t bytes, const uint32_t* len, int64_t n_in, int32_t flags, char* out, uint64_t out_cap, uint64_t* out_bytes)
{
    if (out_bytes) *out_bytes = 0;
    c->ends(Lane::BAM_SORT_CALL);
    if (flags & ~BMBS_BAMSORT_RAW) { c->err = "bam sort: bad argument"; return BMBS_EINVAL; }
    if (int rc = records_check(c, "bam sort", records, bytes, len, n_in, false, false)) return rc;
    const u64 n = (u64)n_in;
    if (!n) return BMBS_OK;
    const bool rawout = (flags & BMBS_BAMSORT_RAW) != 0;
    if (rawout) {
        if (out_bytes) *out_bytes = bytes;
        if (bytes > out_cap) { c->err = "bam sort: the output buffer is too small (out_bytes tells what is needed)"; return BMBS_ENOMEM; }
    }
    if (!out) { c->err = "bam sort: NULL buffer"; return BMBS_EINVAL; }
    HIPCHK(c, hipSetDevice(c->dev));
    c->ends(Lane::SORT_KEYS);
    RecIn& r = c->sc.in;
    int rc = records_stage(c, r, records, bytes, len, n, TOT_SORT_IN);
    if (rc) return rc;
    if ((rc = bam_sort_device(c, r.in.as<char>(), r.off.as<u64>(), r.len.as<u32>(), n, bytes, false, nullptr))) return rc;
    if (rawout) {
        rc = download_locked(c, out, c->bs_sorted.as<char>(), bytes, c->stream, nullptr);
        if (!rc) { c->sc.n = (int64_t)n; c->sc.bytes = bytes; }
        return rc;
    }
    u64 ztotal = 0;
    if ((rc = bgzf_deflate(c, c->bs_sorted.as<char>(), tot_at(c, TOT_SORTED_BYTES), bytes, &ztotal))) return rc;
    if (out_bytes) *out_bytes = ztotal;
    if (ztotal > out_cap) { c->err = "bam sort: the output buffer is too small (out_bytes tells what is needed)"; return BMBS_ENOMEM; }
    if ((rc = bgzf_collect(c, bytes, ztotal))) return rc;
    if ((rc = download_locked(c, out, c->sam_out.as<char>(), ztotal, c->stream, nullptr))) return rc;
    c->sc.bai_n = (int64_t)n; c->sc.bai_bytes = bytes; c->sc.bai_z = ztotal; c->sc.bai_done = false;      // (bmbs_bam_sort_index: computed when asked for)
    c->sc.n = (int64_t)n; c->sc.bytes = bytes;                                                            // (bmbs_bam_sort_methyl: sc.in stays as it is)
    return BMBS_OK;
}

// ---- the .bai pieces of that call (k_bai.hip) from bs_sorted / bs_soff / bam_off -> c->bai_out, counts in c->sc.bai_cnt ----------------------
static int bai_compute(Lane* c)
{
    Lane::SortCall& s = c->sc;
    const u64 n = (u64)s.bai_n, total = s.bai_bytes, nb = (total + BGZF_IN - 1) / BGZF_IN, nw = (n + 63) / 64;
    const u64 R = (u64)s.bai_ref_max + 1;
    if (R > (1ull << 24)) { c->err = "bam sort index: reference index " + std::to_string(s.bai_ref_max) + " is beyond the 2^24 sequences this call keeps counts for"; return BMBS_EINVAL; }
    Carve A;
    if (int rc = A.make(c, c->bai_a, {n * 8, n * 4, n * 4, (n + 1) * 8, nw * 4, (nw + 1) * 8, R * 8, R * 4, R * 4, R * 4, R * 4})) return rc;
    u64* const rb = A.get<u64>(); u32* const rw = A.get<u32>(); u32* const wc = A.get<u32>(); u64* const woff = A.get<u64>(); u32* const wave = A.get<u32>();
    u64* const hoff = A.get<u64>(); u32* const cnt = A.get<u32>(); u32* const has = A.get<u32>(); u32* const first = A.get<u32>(); u32* const last = A.get<u32>();
    u32* const rlist = A.get<u32>();
    u32* const info = stage_info(c);
    HostInfo* const hi = c->h_info;
    HIPCHK(c, hipMemsetAsync(info, 0, TXI_HALF_WORDS * sizeof(u32), c->stream));
    HIPCHK(c, hipMemsetAsync(cnt, 0, (size_t)(reinterpret_cast<char*>(first) - reinterpret_cast<char*>(cnt)), c->stream));      // cnt and has: one behind the other
    const BaiVoff v = {c->bs_soff.as<u64>(), c->bam_off.as<u64>(), total, nb};
    hipLaunchKernelGGL(k_bai_records, dim3(nblk(n, 256)), dim3(256), 0, c->stream, c->bs_sorted.as<char>(), c->bs_soff.as<u64>(), (long)n, (u32)R, rb, rw, cnt, info);
    hipLaunchKernelGGL(k_bai_heads, dim3(nblk(n, 256)), dim3(256), 0, c->stream, rb, rw, (long)n, (u32)R, wave, wc, has, first, last);
    int rc = scan_u32(c, wave, nw, hoff, TOT_BAI_HEADS);
    if (rc) return rc;
    if ((rc = scan_u32(c, wc, n, woff, TOT_BAI_WINS))) return rc;
    if ((rc = scan_u32(c, has, R, nullptr, TOT_BAI_REFS, rlist))) return rc;
    HIPCHK(c, hipMemcpyAsync(hi->stage, info, sizeof hi->stage, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hi->bai, tot_at(c, TOT_BAI_HEADS), sizeof hi->bai, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (hi->stage[1]) { c->err = "bam sort index: the read name and CIGAR of record " + std::to_string(~hi->stage[1]) + " (in sorted order) do not fit its length"; return BMBS_EINVAL; }
    if (hi->stage[0]) {
        c->err = "bam sort index: record " + std::to_string(~hi->stage[0]) + " (in sorted order) ends behind position 2^29: a BAI index cannot hold it (CSI is not written)";
        return BMBS_EINVAL;
    }
    const u64 nnc = hi->stage[2];
    const u64 m = hi->bai[0], T = hi->bai[1], n_ref = hi->bai[2];
    const u64 mr = m - (nnc ? 1 : 0);                    // (the first record without a reference only ends the last run)
    Carve B;
    if ((rc = B.make(c, c->bai_b, {(m + 1) * 4, m * 8, m * 8, m * 4, m * 4, m * 16, T * 8, T * 8, T * 4, T * 4, T * 4, T * 4}))) return rc;
    u32* const hj = B.get<u32>(); u64* const ckey = B.get<u64>(); u64* const ckey2 = B.get<u64>(); u32* const cidx = B.get<u32>(); u32* const cidx2 = B.get<u32>();
    u64* const be = B.get<u64>(); u64* const wkey = B.get<u64>(); u64* const wkey2 = B.get<u64>(); u32* const wval = B.get<u32>(); u32* const wval2 = B.get<u32>();
    u32* const wflag = B.get<u32>(); u32* const wlist = B.get<u32>();
    Carve O;
    if ((rc = O.make(c, c->bai_out, {mr * sizeof(bmbs_bai_chunk), T * sizeof(bmbs_bai_win), n_ref * sizeof(bmbs_bai_ref)}))) return rc;
    for (int i = 0; i < 3; i++) s.bai_at[i] = O.off[i];
    bmbs_bai_chunk* const o_chunk = O.get<bmbs_bai_chunk>(); bmbs_bai_win* const o_win = O.get<bmbs_bai_win>(); bmbs_bai_ref* const o_ref = O.get<bmbs_bai_ref>();
    // the key bits that can be set: those of the largest reference index above the bin's 16 / the window's 15 (as in bam_sort_device)
    int ref_bits = 1;
    while (ref_bits < 32 && R >> ref_bits) ref_bits++;
    hipLaunchKernelGGL(k_bai_emit, dim3(nblk(n, 256)), dim3(256), 0, c->stream, rb, rw, (long)n, hoff, woff, hj, wkey, wval);
    if (mr) {
        hipLaunchKernelGGL(k_bai_chunks, dim3(nblk(m, 256)), dim3(256), 0, c->stream, hj, (long)m, (long)n, rb, v, ckey, cidx, be);
        if ((rc = pair_sort(c, "bam sort index", ckey, ckey2, cidx, cidx2, mr, (unsigned)(16 + ref_bits), nullptr, false))) return rc;
        hipLaunchKernelGGL(k_bai_chunk_out, dim3(nblk(mr, 256)), dim3(256), 0, c->stream, ckey2, cidx2, be, (long)mr, o_chunk);
    }
    u64 n_win = 0;
    if (T) {
        if ((rc = pair_sort(c, "bam sort index", wkey, wkey2, wval, wval2, T, (unsigned)(15 + ref_bits), nullptr, true))) return rc;      // (the chunk sort)
        hipLaunchKernelGGL(k_bai_win_flag, dim3(nblk(T, 256)), dim3(256), 0, c->stream, wkey2, (long)T, wflag);
        if ((rc = scan_u32(c, wflag, T, nullptr, TOT_BAI_NWIN, wlist))) return rc;
        hipLaunchKernelGGL(k_bai_win_out, dim3(nblk(T, 256)), dim3(256), 0, c->stream, wlist, tot_at(c, TOT_BAI_NWIN), wkey2, wval2, v, o_win);
        HIPCHK(c, hipMemcpyAsync(&hi->bai_nwin, tot_at(c, TOT_BAI_NWIN), sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    }
    if (n_ref) hipLaunchKernelGGL(k_bai_ref_out, dim3(nblk(n_ref, 256)), dim3(256), 0, c->stream, rlist, (long)n_ref, first, last, cnt, v, o_ref);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    if (T) n_win = hi->bai_nwin;
    s.bai_cnt[0] = (int64_t)mr; s.bai_cnt[1] = (int64_t)n_win; s.bai_cnt[2] = (int64_t)n_ref; s.bai_cnt[3] = (int64_t)nnc;
    s.bai_done = true;
    return BMBS_OK;
}

static int lane_bam_sort_index(Lane* c, bmbs_bai_chunk* chunk, int64_t chunk_cap, int64_t* n_chunk, bmbs_bai_win* win, int64_t win_cap, int64_t* n_win,
                               bmbs_bai_ref* ref, int64_t ref_cap, int64_t* n_ref, uint64_t* n_no_coor)
{
    const Lane::SortCall& s = c->sc;
    if (!n_no_coor) { c->err = "bam sort index: NULL argument"; return BMBS_EINVAL; }
    *n_no_coor = 0;
    const int rc = fetch_begin(c, "bam sort index", {{n_chunk, &s.bai_cnt[0], chunk_cap, chunk}, {n_win, &s.bai_cnt[1], win_cap, win}, {n_ref, &s.bai_cnt[2], ref_cap, ref}}, s.bai_n >= 0,
                               "the context's last bmbs_bam_sort call returned no BGZF blocks (none yet, BMBS_BAMSORT_RAW, no records, or it failed), or another call has used its buffers since",
                               "an array is too small (n_chunk, n_win and n_ref tell what is needed)",
                               [](Lane* c) -> int { HIPCHK(c, hipSetDevice(c->dev)); return c->sc.bai_done ? BMBS_OK : bai_compute(c); });
    if (!rc || rc == BMBS_ENOMEM) *n_no_coor = (uint64_t)s.bai_cnt[3];      // (with the counts: a size query gets it too)
    if (rc) return rc;
    const char* const O = c->bai_out.as<char>();
    if (*n_chunk) HIPCHK(c, hipMemcpyAsync(chunk, O + s.bai_at[0], (size_t)*n_chunk * sizeof(bmbs_bai_chunk), hipMemcpyDeviceToHost, c->stream));
    if (*n_win) HIPCHK(c, hipMemcpyAsync(win, O + s.bai_at[1], (size_t)*n_win * sizeof(bmbs_bai_win), hipMemcpyDeviceToHost, c->stream));
    if (*n_ref) HIPCHK(c, hipMemcpyAsync(ref, O + s.bai_at[2], (size_t)*n_ref * sizeof(bmbs_bai_ref), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BMBS_OK;
}

// ---- duplicate marking (k_markdup.hip) -----------------------------------------------------------------------------------------------------
// the signatures of n_tmpl templates -> c->dp_sig; entry i = len[i] bytes at raw + off[i] (raw is padded by 16 bytes and more)
static int dup_sig_device(Lane* c, const char* raw, const u64* off, const u32* len, bool paired, u64 n_tmpl)
{
    ENS(c, c->dp_sig, n_tmpl * sizeof(bmbs_dup_sig) + 64);
    u32* const info = stage_info(c);
    HIPCHK(c, hipMemsetAsync(info, 0, TXI_HALF_WORDS * sizeof(u32), c->stream));
    prof_begin(c, "k_dup_sig");
    hipLaunchKernelGGL(k_dup_sig, dim3(nblk(n_tmpl * DUP_GROUP, 256)), dim3(256), 0, c->stream, raw, off, len, paired ? 1 : 0, (long)n_tmpl, c->dp_sig.as<bmbs_dup_sig>(), info);
    prof_end(c);
    const u32* const got = c->h_info->stage;
    HIPCHK(c, hipMemcpyAsync(c->h_info->stage, info, 2 * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    if (got[0]) {
        c->err = "dup sigs: the length given for record " + std::to_string(~got[0]) + " is not its block_size + 4 (or is below the 36 bytes every BAM record has)";
        return BMBS_EINVAL;
    }
    if (got[1]) { c->err = "dup sigs: the read name, CIGAR, sequence and qualities of record " + std::to_string(~got[1]) + " do not fit its length"; return BMBS_EINVAL; }
    return BMBS_OK;
}

static int lane_bam_dup_sigs(Lane* c, const char* records, uint64_t bytes, const uint32_t* len, int64_t n_in, int32_t paired, bmbs_dup_sig* sig, int64_t sig_cap,
                             int64_t* n_sig)
{
    if (!n_sig) { c->err = "dup sigs: NULL argument"; return BMBS_EINVAL; }
    *n_sig = 0;
    if (int rc = records_check(c, "dup sigs", records, bytes, len, n_in, true, paired != 0)) return rc;
    const u64 n = (u64)n_in, nt = paired ? n / 2 : n;
    *n_sig = (int64_t)nt;
    if ((int64_t)nt > sig_cap) { c->err = "dup sigs: the array is too small (n_sig tells what is needed)"; return BMBS_ENOMEM; }
    if (!nt) return BMBS_OK;
    if (!sig || (bytes && !records)) { c->err = "dup sigs: NULL buffer"; return BMBS_EINVAL; }
    HIPCHK(c, hipSetDevice(c->dev));
    c->ends(Lane::DUP_SIGS);
    RecIn& r = c->dp_in;
    int rc = records_stage(c, r, records, bytes, len, n, TOT_RECS_IN);
    if (rc) return rc;
    if ((rc = dup_sig_device(c, r.in.as<char>(), r.off.as<u64>(), r.len.as<u32>(), paired != 0, nt))) return rc;
    HIPCHK(c, hipMemcpyAsync(sig, c->dp_sig.p, nt * sizeof(bmbs_dup_sig), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BMBS_OK;
}

static int lane_text_sorted_dup(Lane* c, bmbs_dup_sig* sig, int64_t sig_cap, int64_t* n_sig, uint32_t* tmpl, int64_t cap, int64_t* n)
{
    Lane::SortedText& t = c->st;
    const int64_t nt = t.lines >> (t.pe ? 1 : 0), nr = t.n;
    if (int rc = fetch_begin(c, "sorted dup", {{n_sig, &nt, sig_cap, sig}, {n, &nr, cap, tmpl}}, t.lines >= 0 && t.n >= 0,
                             "the context's last text call was not a BMBS_TEXT_BAM_SORTED call that returned records, or another call has used its buffers since",
                             "an array is too small (n_sig and n tell what is needed)")) return rc;
    if (!nt) return BMBS_OK;
    HIPCHK(c, hipSetDevice(c->dev));
    if (!t.sigs_done) {
        const int rc = dup_sig_device(c, c->bam_raw.as<char>(), c->sam_off.as<u64>(), c->sam_len.as<u32>(), t.pe, (u64)nt);
        if (rc) return rc;
        if (nr) {
            ENS(c, c->dp_tmpl, (u64)nr * 4 + 64);
            hipLaunchKernelGGL(k_dup_tmpl, dim3(nblk((u64)nr, 256)), dim3(256), 0, c->stream, c->bs_idx2.as<u32>(), (long)nr, t.pe ? 1 : 0, c->dp_tmpl.as<u32>());
        }
        t.sigs_done = true;
    }
    HIPCHK(c, hipMemcpyAsync(sig, c->dp_sig.p, (u64)nt * sizeof(bmbs_dup_sig), hipMemcpyDeviceToHost, c->stream));
    if (nr) HIPCHK(c, hipMemcpyAsync(tmpl, c->dp_tmpl.p, (u64)nr * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BMBS_OK;
}

static int lane_dup_select(Lane* c, const bmbs_dup_sig* sig, int64_t n_in, uint8_t* dup, int64_t* n_dup)
{
    if (n_dup) *n_dup = 0;
    if (n_in < 0 || n_in >= (1ll << 31)) { c->err = "dup select: bad argument"; return BMBS_EINVAL; }
    if (!n_in) return BMBS_OK;
    if (!sig || !dup) { c->err = "dup select: NULL buffer"; return BMBS_EINVAL; }
    const u64 n = (u64)n_in;
    HIPCHK(c, hipSetDevice(c->dev));
    c->ends(Lane::DUP_SIGS);
    ENS(c, c->dp_sig, n * sizeof(bmbs_dup_sig) + 64); ENS(c, c->dp_key, n * 8 + 64); ENS(c, c->dp_key2, n * 8 + 64);
    ENS(c, c->dp_idx, n * 4 + 64); ENS(c, c->dp_idx2, n * 4 + 64); ENS(c, c->dp_dup, n + 64);
    {
        std::lock_guard<std::mutex> up(g_h2d_mu[c->dev & 15]);
        hipStream_t us = up_stream_of(c);
        HIPCHK(c, hipMemcpyAsync(c->dp_sig.p, sig, n * sizeof(bmbs_dup_sig), hipMemcpyHostToDevice, us));
        HIPCHK(c, hipStreamSynchronize(us));
    }
    const bmbs_dup_sig* const ds = c->dp_sig.as<bmbs_dup_sig>();
    u64* const ka = c->dp_key.as<u64>(); u64* const kb = c->dp_key2.as<u64>();
    u32* const ia = c->dp_idx.as<u32>(); u32* const ib = c->dp_idx2.as<u32>();
    u32* const info = stage_info(c);                      // three 64-bit ORs and the count of duplicates (TXI_DUP_COUNT)
    HIPCHK(c, hipMemsetAsync(info, 0, TXI_HALF_WORDS * sizeof(u32), c->stream));
    hipLaunchKernelGGL(k_dup_bits, dim3(nblk(n, 256)), dim3(256), 0, c->stream, ds, (long)n, reinterpret_cast<unsigned long long*>(info));
    HIPCHK(c, hipMemcpyAsync(c->h_info->dup_bits, info, sizeof c->h_info->dup_bits, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // each pass over the key bits that can be set only
    unsigned end_bit[3];
    size_t tmp_bytes = 0;
    for (int p = 0; p < 3; p++) {
        const u64 bits = c->h_info->dup_bits[p];
        end_bit[p] = 1;
        while (end_bit[p] < 64 && bits >> end_bit[p]) end_bit[p]++;
        size_t t = 0;
        if (int rc = pair_sort_bytes(c, "dup select", ka, kb, ia, ib, n, end_bit[p], &t)) return rc;
        tmp_bytes = std::max(tmp_bytes, t);
    }
    ENS(c, c->bs_tmp, tmp_bytes + 64);
    // (key, entry) pairs from the least significant field up; the entry numbers go back and forth between ia and ib
    prof_begin(c, "dup_pair_sorts");
    for (int p = 0; p < 3; p++) {
        u32* const in = p == 1 ? ib : ia; u32* const out = p == 1 ? ia : ib;
        hipLaunchKernelGGL(k_dup_keys, dim3(nblk(n, 256)), dim3(256), 0, c->stream, ds, p ? in : nullptr, (long)n, p, ka, in);
        if (int rc = pair_sort(c, "dup select", ka, kb, in, out, n, end_bit[p], nullptr, false, tmp_bytes)) return rc;
    }
    prof_end(c);
    prof_begin(c, "k_dup_heads");
    hipLaunchKernelGGL(k_dup_heads, dim3(nblk(n, 256)), dim3(256), 0, c->stream, ds, ib, (long)n, c->dp_dup.as<uint8_t>(), info + TXI_DUP_COUNT);
    prof_end(c);
    HIPCHK(c, hipMemcpyAsync(&c->h_info->stage[TXI_DUP_COUNT], info + TXI_DUP_COUNT, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(dup, c->dp_dup.p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    if (n_dup) *n_dup = (int64_t)c->h_info->stage[TXI_DUP_COUNT];
    return BMBS_OK;
}

// ---- methylation counts per cytosine (k_methyl.hip) -----------------------------------------------------------------------------------------
// n (key, value) pairs in ka / va (kb / vb: as large, the sort's other side) -> one entry per distinct key with the values' halves added
// up: bmbs_methyl_site at `site`, or (key, value) pairs at okey / oval; *n_out = their number
struct MethEv { u64 *ka, *kb, *va, *vb; };
static int meth_reduce(Lane* c, const MethEv& e, u64 n, int pos_bits, int key_bits, bmbs_methyl_site* site, u64* okey, u64* oval, u64* n_out)
{
    *n_out = 0;
    if (!n) return BMBS_OK;
    const u64 nw = (n + 63) / 64;
    Carve A;
    if (int rc = A.make(c, c->mt_work, {nw * 4, (nw + 1) * 8, n * 4, n * 4, (n + 1) * 8, (n + 1) * 8, n * 4})) return rc;
    u32* const wave = A.get<u32>(); u64* const hoff = A.get<u64>(); u32* const m = A.get<u32>(); u32* const u = A.get<u32>(); u64* const ms = A.get<u64>();
    u64* const us = A.get<u64>(); u32* const hpos = A.get<u32>();
    int rc = pair_sort(c, "methyl", e.ka, e.kb, e.va, e.vb, n, (unsigned)key_bits, "meth_pair_sort", true);      // (the slice's before)
    if (rc) return rc;
    prof_begin(c, "k_meth_heads");
    hipLaunchKernelGGL(k_meth_heads, dim3(nblk(n, 256)), dim3(256), 0, c->stream, e.kb, e.vb, (long)n, wave, m, u);
    prof_end(c);
    if ((rc = scan_u32(c, wave, nw, hoff, TOT_METH_HEADS))) return rc;
    if ((rc = scan_u32(c, m, n, ms, TOT_METH_M))) return rc;
    if ((rc = scan_u32(c, u, n, us, TOT_METH_U))) return rc;
    HIPCHK(c, hipMemcpyAsync(&c->h_info->meth_heads, tot_at(c, TOT_METH_HEADS), sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    hipLaunchKernelGGL(k_meth_hpos, dim3(nblk(n, 256)), dim3(256), 0, c->stream, e.kb, (long)n, hoff, hpos);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const u64 nh = c->h_info->meth_heads;
    if (nh > n) { c->err = "methyl: more run heads than entries"; return BMBS_ESTATE; }
    *n_out = nh;
    prof_begin(c, "k_meth_sites");
    hipLaunchKernelGGL(k_meth_sites, dim3(nblk(nh, 256)), dim3(256), 0, c->stream, c->ix.gen2p, c->ix.chrom_start, e.kb, hpos, (long)nh, (long)n, ms, us, pos_bits, site, okey, oval);
    prof_end(c);
    return BMBS_OK;
}
// room for n events in c->mt_ev: keys and values, each with the sort's other side
static int meth_events(Lane* c, u64 n, MethEv& e)
{
    Carve E;
    if (int rc = E.make(c, c->mt_ev, {n * 8, n * 8, n * 8, n * 8})) return rc;
    e.ka = E.get<u64>(); e.kb = E.get<u64>(); e.va = E.get<u64>(); e.vb = E.get<u64>();
    return BMBS_OK;
}

static int methyl_params_as_opts(Lane* c, const bmbs_methyl_params* par, bmbs_methyl_opts* o)
{
    *o = bmbs_methyl_opts{1, 10, 5, 0, {0, 0}, {0, 0}};
    if (!par) return BMBS_OK;
    if (par->contexts < 1 || par->contexts > 7 || par->min_mapq < 0 || par->min_mapq > 255 || par->min_phred < 0 || par->min_phred > 255 || par->reserved) {
        c->err = "methyl: bad parameters (contexts 1..7, min_mapq and min_phred 0..255, reserved 0)"; return BMBS_EINVAL;
    }
    o->contexts = par->contexts; o->min_mapq = par->min_mapq; o->min_phred = par->min_phred;
    return BMBS_OK;
}

// the options of a call: *opts if given (the _opts calls), else the old calls' parameters with no flags and no trim (NULL: the defaults).
// opposite: an opposite call, which makes no M-bias table -- its flags must be 0
static int methyl_get_opts(Lane* c, const bmbs_methyl_params* par, const bmbs_methyl_opts* opts, bool opposite, bmbs_methyl_opts* out)
{
    if (!opts) return methyl_params_as_opts(c, par, out);
    const bmbs_methyl_opts& o = *out = *opts;
    bool bad = o.contexts < 1 || o.contexts > 7 || o.min_mapq < 0 || o.min_mapq > 255 || o.min_phred < 0 || o.min_phred > 255 || (o.flags & ~BMBS_METHYL_MBIAS);
    for (int m = 0; m < 2; m++) bad = bad || o.ignore_5p[m] < 0 || o.ignore_5p[m] > 65535 || o.ignore_3p[m] < 0 || o.ignore_3p[m] > 65535;
    if (bad) { c->err = "methyl: bad parameters (contexts 1..7, min_mapq and min_phred 0..255, flags BMBS_METHYL_MBIAS or 0, ignore values 0..65535)"; return BMBS_EINVAL; }
    if (opposite && o.flags) { c->err = "methyl opposite: bad parameters (flags must be 0: an opposite call makes no M-bias table)"; return BMBS_EINVAL; }
    return BMBS_OK;
}

// a slice of records [start, *end) with at most `cap` events (a record with more is a slice of its own), events [*e0, *e1) of eoff
static int meth_slice(Lane* c, const u64* eoff, u64 start, u64 n, u64 cap, u64* end, u64* e0, u64* e1)
{
    u32* const info = stage_info(c);
    hipLaunchKernelGGL(k_meth_cut, dim3(1), dim3(64), 0, c->stream, eoff, (long)start, (long)n, cap, reinterpret_cast<u64*>(info));
    HIPCHK(c, hipMemcpyAsync(&c->h_info->meth_cut, info, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&c->h_info->meth_eoff, eoff + start, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *end = c->h_info->meth_cut; *e0 = c->h_info->meth_eoff;
    if (*end <= start || *end > n) { c->err = "methyl: bad slice"; return BMBS_ESTATE; }
    HIPCHK(c, hipMemcpyAsync(&c->h_info->meth_eoff, eoff + *end, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *e1 = c->h_info->meth_eoff;
    return BMBS_OK;
}

// the records at raw / off / len (device; off = the exclusive scan of len), their clips (device, or NULL) -> c->mt_site, c->mc.sites;
// with BMBS_METHYL_MBIAS the M-bias table of all n records -> c->mt_mbias too (once, whatever the slices).  Options: methyl_get_opts.
// opposite: the walk is the opposite-strand observation (k_methyl.hip) and its entries -> c->mt_site, c->mc.opp; flags must be 0.
// (The caller has ended the last methyl call's result: Lane::METHYL_CALL)
static int methyl_device(Lane* c, const char* raw, const u64* off, const u32* len, const u32* clip, u64 n, const bmbs_methyl_params* par_in, const bmbs_methyl_opts* opts,
                         bool opposite, int64_t* n_site)
{
    // BMBS_METHYL_EVENTS (test aid): the events a slice of records may hold
    static const u64 slice_cap = [] { const char* e = getenv("BMBS_METHYL_EVENTS"); const long long v = e ? atoll(e) : 0; return v > 0 ? (u64)v : (u64)1 << 26; }();
    bmbs_methyl_opts pp;
    if (int rc = methyl_get_opts(c, par_in, opts, opposite, &pp)) return rc;
    MethPar par;
    par.contexts = (u32)pp.contexts; par.min_mapq = (u32)pp.min_mapq; par.min_phred = (u32)pp.min_phred; par.n_chrom = c->ix.n_chrom;
    for (int m = 0; m < 2; m++) { par.ig5[m] = (u32)pp.ignore_5p[m]; par.ig3[m] = (u32)pp.ignore_3p[m]; }
    const bool trim = par.ig5[0] || par.ig5[1] || par.ig3[0] || par.ig3[1];
    const bool mbias = (pp.flags & BMBS_METHYL_MBIAS) != 0;
    int pos_bits = 1, ref_bits = 1;
    while (pos_bits < 40 && c->ix.G >> pos_bits) pos_bits++;
    while (ref_bits < 24 && (u64)c->ix.n_chrom >> ref_bits) ref_bits++;
    par.pos_bits = pos_bits;
    ENS(c, c->mt_cnt, n * 4 + 64); ENS(c, c->mt_eoff, (n + 1) * 8 + 64);
    u32* const info = stage_info(c);
    HIPCHK(c, hipMemsetAsync(info, 0, TXI_HALF_WORDS * sizeof(u32), c->stream));
    const unsigned grid = nblk(n * METH_GROUP, 256);
    // (without a trim: the kernels as they were before there was one)
    auto k_count = trim ? k_meth_events<false, true> : k_meth_events<false, false>;
    auto k_emit = trim ? k_meth_events<true, true> : k_meth_events<true, false>;
    if (opposite) {
        k_count = trim ? k_meth_events<false, true, true> : k_meth_events<false, false, true>;
        k_emit = trim ? k_meth_events<true, true, true> : k_meth_events<true, false, true>;
    }
    prof_begin(c, opposite ? "k_meth_opp_count" : "k_meth_count");
    hipLaunchKernelGGL(k_count, dim3(grid), dim3(256), 0, c->stream, c->ix.gen2p, c->ix.chrom_start, raw, off, len, clip, 0l,
                       (long)n, par, c->mt_cnt.as<u32>(), (const u64*)nullptr, (u64*)nullptr, (u64*)nullptr, info);
    prof_end(c);
    int rc = scan_u32(c, c->mt_cnt.as<u32>(), n, c->mt_eoff.as<u64>(), TOT_METH_EVENTS);
    if (rc) return rc;
    const u32* const got = c->h_info->stage;
    HIPCHK(c, hipMemcpyAsync(c->h_info->stage, info, 4 * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&c->h_info->meth_events, tot_at(c, TOT_METH_EVENTS), sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    if (got[0]) { c->err = "methyl: the length given for record " + std::to_string(~got[0]) + " is not its block_size + 4 (or is below the 36 bytes every BAM record has)"; return BMBS_EINVAL; }
    if (got[1]) { c->err = "methyl: the read name, CIGAR, sequence and qualities of record " + std::to_string(~got[1]) + " do not fit its length"; return BMBS_EINVAL; }
    if (got[2]) { c->err = "methyl: the refID of record " + std::to_string(~got[2]) + " is beyond the " + std::to_string(c->ix.n_chrom) + " sequences of the index"; return BMBS_EINVAL; }
    if (got[3]) { c->err = "methyl: the reference span of record " + std::to_string(~got[3]) + " runs off its sequence"; return BMBS_EINVAL; }
    if (mbias) {
        // 6 blocks per CU, each with its own tally in LDS (k_methyl.hip): the 6 waves per SIMD its registers allow, and 144 of the CU's 160
        // KiB of LDS -- the walk waits on memory most of its time, so resident waves are what it runs on.  The count pass above has
        // found nothing to refuse
        if (!c->mt_cus) { int cus = 0; HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->dev)); c->mt_cus = cus > 0 ? cus : 1; }
        ENS(c, c->mt_mbias, METH_MBIAS_ROWS * BMBS_MBIAS_CYCLES * 8 + 64);
        HIPCHK(c, hipMemsetAsync(c->mt_mbias.p, 0, METH_MBIAS_ROWS * BMBS_MBIAS_CYCLES * 8, c->stream));
        const unsigned mgrid = (unsigned)std::min<u64>((u64)c->mt_cus * 6, nblk(n * METH_GROUP, 256));
        prof_begin(c, "k_meth_mbias");
        hipLaunchKernelGGL(k_meth_mbias, dim3(mgrid), dim3(256), 0, c->stream, c->ix.gen2p, c->ix.chrom_start, raw, off, len, clip, (long)n, par,
                           c->mt_mbias.as<unsigned long long>());
        prof_end(c);
    }
    const u64 n_ev = c->h_info->meth_events;
    const u64* const eoff = c->mt_eoff.as<u64>();
    u64 n_acc = 0, n_sites = 0;
    bool sliced = false;
    MethEv e;
    for (u64 start = 0; start < n && n_ev;) {
        u64 end = n, e0 = 0, e1 = n_ev;
        if (n_ev > slice_cap) {
            sliced = true;
            if ((rc = meth_slice(c, eoff, start, n, slice_cap, &end, &e0, &e1))) return rc;
        }
        const u64 ne = e1 - e0;
        if (ne >= (1ull << 32)) { c->err = "methyl: a record with 2^32 events and more"; return BMBS_EINVAL; }
        if (ne) {
            if ((rc = meth_events(c, ne, e))) return rc;
            prof_begin(c, opposite ? "k_meth_opp_emit" : "k_meth_emit");
            hipLaunchKernelGGL(k_emit, dim3(nblk((end - start) * METH_GROUP, 256)), dim3(256), 0, c->stream, c->ix.gen2p,
                               c->ix.chrom_start, raw, off, len, clip, (long)start, (long)(end - start), par, (u32*)nullptr, eoff + start, e.ka, e.va, info + TXI_METH_EMIT);
            prof_end(c);
            u64 got = 0;
            if (!sliced) {
                ENS(c, c->mt_site, ne * sizeof(bmbs_methyl_site) + 64);
                if ((rc = meth_reduce(c, e, ne, pos_bits, pos_bits + ref_bits, c->mt_site.as<bmbs_methyl_site>(), nullptr, nullptr, &got))) return rc;
                n_sites = got;
            } else {
                // the slice's sites as pairs behind those of the slices before (the buffer grows: what it holds is copied over)
                if (c->mt_acc.cap < (n_acc + ne) * 16 + 64) {
                    DevBuf grown;
                    ENS(c, grown, (n_acc + ne) * 16 * 2 + 64);
                    if (n_acc) HIPCHK(c, hipMemcpyAsync(grown.p, c->mt_acc.p, n_acc * 16, hipMemcpyDeviceToDevice, c->stream));
                    HIPCHK(c, hipStreamSynchronize(c->stream));
                    release(c->mt_acc); c->mt_acc = grown;
                }
                // (pairs interleaved as key, value would need another kernel: keys in the first half of each slice's piece, values behind)
                ENS(c, c->mt_site, ne * 16 + 64);
                u64* const sk = c->mt_site.as<u64>(); u64* const sv = sk + ne;
                if ((rc = meth_reduce(c, e, ne, pos_bits, pos_bits + ref_bits, nullptr, sk, sv, &got))) return rc;
                HIPCHK(c, hipMemcpyAsync(c->mt_acc.as<u64>() + 2 * n_acc, sk, got * 8, hipMemcpyDeviceToDevice, c->stream));
                HIPCHK(c, hipMemcpyAsync(c->mt_acc.as<u64>() + 2 * n_acc + got, sv, got * 8, hipMemcpyDeviceToDevice, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                c->mt_slice.push_back({n_acc, got});
                n_acc += got;
            }
        }
        start = end;
    }
    if (sliced) {
        // the slices' sites, one more reduction: keys and values gathered into the two sides of the event buffer
        if ((rc = meth_events(c, n_acc, e))) return rc;
        for (const auto& s : c->mt_slice) {
            HIPCHK(c, hipMemcpyAsync(e.ka + s.first, c->mt_acc.as<u64>() + 2 * s.first, s.second * 8, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(e.va + s.first, c->mt_acc.as<u64>() + 2 * s.first + s.second, s.second * 8, hipMemcpyDeviceToDevice, c->stream));
        }
        c->mt_slice.clear();
        ENS(c, c->mt_site, n_acc * sizeof(bmbs_methyl_site) + 64);
        if ((rc = meth_reduce(c, e, n_acc, pos_bits, pos_bits + ref_bits, c->mt_site.as<bmbs_methyl_site>(), nullptr, nullptr, &n_sites))) return rc;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    if (opposite) c->mc.opp = (int64_t)n_sites;
    else { c->mc.sites = (int64_t)n_sites; c->mc.has_mbias = mbias; }
    if (n_site) *n_site = (int64_t)n_sites;
    return BMBS_OK;
}

// opposite: bmbs_bam_methyl_opposite (opts NULL: the defaults)
static int lane_bam_methyl(Lane* c, const char* records, uint64_t bytes, const uint32_t* len, int64_t n_in, const uint32_t* clip, const bmbs_methyl_params* par,
                           const bmbs_methyl_opts* opts, bool opposite, int64_t* n_site)
{
    if (n_site) *n_site = 0;
    c->ends(Lane::METHYL_CALL);
    c->mt_slice.clear();
    if (!c->attached) { c->err = "methyl: no index attached"; return BMBS_ESTATE; }
    if (int rc = records_check(c, "methyl", records, bytes, len, n_in, true, false)) return rc;
    const u64 n = (u64)n_in;
    if (!n) {
        // (no record: no device work; an _opts call still has its options checked, and its table is all zero)
        bmbs_methyl_opts pp;
        if (opts) { if (int rc = methyl_get_opts(c, par, opts, opposite, &pp)) return rc; c->mc.has_mbias = c->mc.mbias_zero = (pp.flags & BMBS_METHYL_MBIAS) != 0; }
        (opposite ? c->mc.opp : c->mc.sites) = 0;
        return BMBS_OK;
    }
    if (bytes && !records) { c->err = "methyl: NULL buffer"; return BMBS_EINVAL; }
    HIPCHK(c, hipSetDevice(c->dev));
    RecIn& r = c->mt_in;
    if (int rc = records_stage(c, r, records, bytes, len, n, TOT_RECS_IN, clip, &c->mt_clip)) return rc;
    return methyl_device(c, r.in.as<char>(), r.off.as<u64>(), r.len.as<u32>(), clip ? c->mt_clip.as<u32>() : nullptr, n, par, opts, opposite, n_site);
}

static int lane_bam_sort_methyl(Lane* c, const uint32_t* clip, const bmbs_methyl_params* par, const bmbs_methyl_opts* opts, bool opposite, int64_t* n_site)
{
    if (n_site) *n_site = 0;
    c->ends(Lane::METHYL_CALL);
    c->mt_slice.clear();
    if (!c->attached) { c->err = "sort methyl: no index attached"; return BMBS_ESTATE; }
    if (c->sc.n < 0) {
        c->err = "sort methyl: no bmbs_bam_sort call's records are resident (none yet, no records, or it failed), or another call has used its buffers since";
        return BMBS_ESTATE;
    }
    const u64 n = (u64)c->sc.n;
    HIPCHK(c, hipSetDevice(c->dev));
    if (clip) {
        ENS(c, c->mt_clip, n * 4 + 64);
        std::lock_guard<std::mutex> up(g_h2d_mu[c->dev & 15]);
        hipStream_t us = up_stream_of(c);
        HIPCHK(c, hipMemcpyAsync(c->mt_clip.p, clip, n * 4, hipMemcpyHostToDevice, us));
        HIPCHK(c, hipStreamSynchronize(us));
    }
    const RecIn& r = c->sc.in;
    return methyl_device(c, r.in.as<char>(), r.off.as<u64>(), r.len.as<u32>(), clip ? c->mt_clip.as<u32>() : nullptr, n, par, opts, opposite, n_site);
}

static int lane_methyl_sites(Lane* c, bmbs_methyl_site* site, int64_t cap, int64_t* n)
{
    if (int rc = fetch_begin(c, "methyl sites", {{n, &c->mc.sites, cap, site}}, c->mc.sites >= 0,
                             c->mc.opp >= 0 ? "the context's last methylation call was an opposite call: its entries are fetched with bmbs_methyl_opposite"
                                            : "the context's last bmbs_bam_methyl / bmbs_bam_sort_methyl call left no result",
                             "the array is too small (n tells what is needed)")) return rc;
    if (!c->mc.sites) return BMBS_OK;
    HIPCHK(c, hipSetDevice(c->dev));
    hipStream_t ds = down_stream_of(c);
    HIPCHK(c, hipMemcpyAsync(site, c->mt_site.p, (size_t)c->mc.sites * sizeof(bmbs_methyl_site), hipMemcpyDeviceToHost, ds));
    HIPCHK(c, hipStreamSynchronize(ds));
    return BMBS_OK;
}

static int lane_methyl_opposite(Lane* c, bmbs_methyl_site* entry, int64_t cap, int64_t* n)
{
    if (int rc = fetch_begin(c, "methyl opposite", {{n, &c->mc.opp, cap, entry}}, c->mc.opp >= 0,
                             c->mc.sites >= 0 ? "the context's last methylation call was not an opposite call: its sites are fetched with bmbs_methyl_sites"
                                              : "the context's last bmbs_bam_methyl_opposite / bmbs_bam_sort_methyl_opposite call left no result",
                             "the array is too small (n tells what is needed)")) return rc;
    if (!c->mc.opp) return BMBS_OK;
    HIPCHK(c, hipSetDevice(c->dev));
    hipStream_t ds = down_stream_of(c);
    HIPCHK(c, hipMemcpyAsync(entry, c->mt_site.p, (size_t)c->mc.opp * sizeof(bmbs_methyl_site), hipMemcpyDeviceToHost, ds));
    HIPCHK(c, hipStreamSynchronize(ds));
    return BMBS_OK;
}

// bmbs_methyl_drop_variants (host only): the rule is in include/bmbs.h
static int methyl_drop_variants(bmbs_methyl_site* site, int64_t n_site, const bmbs_methyl_site* opp, int64_t n_opp, int32_t min_depth, int32_t max_ppm, int64_t* n_kept)
{
    if (n_kept) *n_kept = 0;
    if (n_site < 0 || n_opp < 0 || (n_site && !site) || (n_opp && !opp) || !n_kept || min_depth < 1 || max_ppm < 0 || max_ppm > 1000000) return BMBS_EINVAL;
    const auto less = [](const bmbs_methyl_site& a, const bmbs_methyl_site& b) { return a.ref != b.ref ? a.ref < b.ref : a.pos < b.pos; };
    for (int64_t i = 1; i < n_site; i++) if (!less(site[i - 1], site[i])) return BMBS_EINVAL;
    for (int64_t j = 1; j < n_opp; j++) if (!less(opp[j - 1], opp[j])) return BMBS_EINVAL;
    int64_t kept = 0, j = 0;
    for (int64_t i = 0; i < n_site; i++) {
        while (j < n_opp && less(opp[j], site[i])) j++;
        bool drop = false;
        if (j < n_opp && !less(site[i], opp[j])) {
            const uint64_t variant = opp[j].meth, depth = (uint64_t)opp[j].meth + opp[j].unmeth;      // (below 2^33; times 10^6: below 2^53)
            drop = depth >= (uint64_t)min_depth && variant * 1000000ull > (uint64_t)max_ppm * depth;
        }
        if (!drop) site[kept++] = site[i];
    }
    *n_kept = kept;
    return BMBS_OK;
}

static int lane_methyl_mbias(Lane* c, uint64_t* table, int64_t cap, int64_t* n)
{
    const int64_t entries = (int64_t)METH_MBIAS_ROWS * BMBS_MBIAS_CYCLES;
    if (int rc = fetch_begin(c, "methyl mbias", {{n, &entries, cap, table}}, c->mc.sites >= 0 && c->mc.has_mbias,
                             "the context's last bmbs_bam_methyl_opts / bmbs_bam_sort_methyl_opts call left no table (none yet, it failed, or BMBS_METHYL_MBIAS was not set)",
                             "the array is too small (n tells what is needed)")) return rc;
    if (c->mc.mbias_zero) { memset(table, 0, (size_t)entries * 8); return BMBS_OK; }
    HIPCHK(c, hipSetDevice(c->dev));
    hipStream_t ds = down_stream_of(c);
    HIPCHK(c, hipMemcpyAsync(table, c->mt_mbias.p, (size_t)entries * 8, hipMemcpyDeviceToHost, ds));
    HIPCHK(c, hipStreamSynchronize(ds));
    return BMBS_OK;
}

static int lane_text_sorted_clip(Lane* c, uint32_t* clip, int64_t cap, int64_t* n)
{
    const Lane::SortedText& t = c->st;
    if (int rc = fetch_begin(c, "sorted clip", {{n, &t.n, cap, clip}}, t.lines >= 0 && t.n >= 0,
                             "the context's last text call was not a BMBS_TEXT_BAM_SORTED call that returned records, or another call has used its buffers since",
                             "the array is too small (n tells what is needed)")) return rc;
    const u64 nr = (u64)t.n;
    if (!nr) return BMBS_OK;
    HIPCHK(c, hipSetDevice(c->dev));
    ENS(c, c->mt_cl2, nr * 4 + 64);
    u32* const info = stage_info(c);
    HIPCHK(c, hipMemsetAsync(info, 0, TXI_HALF_WORDS * sizeof(u32), c->stream));
    prof_begin(c, "k_meth_clip");
    hipLaunchKernelGGL(k_meth_clip, dim3(nblk(nr, 256)), dim3(256), 0, c->stream, c->bam_raw.as<char>(), c->sam_off.as<u64>(), c->sam_len.as<u32>(), c->bs_idx2.as<u32>(), (long)nr,
                       t.pe ? 1 : 0, c->mt_cl2.as<u32>(), info);
    prof_end(c);
    HIPCHK(c, hipMemcpyAsync(c->h_info->stage, info, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(clip, c->mt_cl2.p, nr * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    if (c->h_info->stage[0]) { c->err = "sorted clip: the overlap of record " + std::to_string(~c->h_info->stage[0]) + " (in sorted order) with its mate does not fit 16 bits"; return BMBS_EINVAL; }
    return BMBS_OK;
}

// ---- reads the bisulfite treatment did not convert (k_nonconv.hip): the rule is in include/bmbs.h -------------------------------------------------
// Neither call touches a methyl call's result (Lane::mc, mt_*) or what a sort left (Lane::st, Lane::sc): the records of bmbs_bam_nonconv
// go to nc_in, everything the kernels write to nc_work.
static int nonconv_get_params(Lane* c, const bmbs_nonconv_params* in, NonconvPar* out)
{
    const bmbs_nonconv_params p = in ? *in : bmbs_nonconv_params{3, 0, 5, 0};
    if (p.threshold < 0 || p.percent < 0 || p.percent > 100 || p.min_count < 0 || p.min_phred < 0 || p.min_phred > 255) {
        c->err = "nonconv: bad parameters (threshold and min_count 0 and above, percent 0..100, min_phred 0..255)"; return BMBS_EINVAL;
    }
    out->threshold = (u32)p.threshold; out->percent = (u32)p.percent; out->min_count = (u32)p.min_count; out->min_phred = (u32)p.min_phred;
    out->n_chrom = c->ix.n_chrom;
    return BMBS_OK;
}

// the n entries at raw / off / len (device; off = the exclusive scan of len), n_tmpl templates of them -> in c->nc_work the counts (if
// wanted), the templates' verdicts and the tally; n_out more bytes are carved for the caller (the verdicts in sorted order).  The tally
// comes back in tally[NONCONV_TALLY]; the refusals are those of methyl_device, word for word
struct NonconvOut { bmbs_nonconv_count* count; uint8_t* fail; uint8_t* out; };
static int nonconv_device(Lane* c, const char* raw, const u64* off, const u32* len, u64 n, bool paired, u64 n_tmpl, const NonconvPar& par, bool want_count, u64 n_out,
                          NonconvOut* o, u64 tally[NONCONV_TALLY])
{
    Carve A;
    if (int rc = A.make(c, c->nc_work, {NONCONV_TALLY * 8, want_count ? n * sizeof(bmbs_nonconv_count) : 0, n_tmpl, n_out})) return rc;
    unsigned long long* const d_tally = A.get<unsigned long long>();
    o->count = A.get<bmbs_nonconv_count>(); o->fail = A.get<uint8_t>(); o->out = A.get<uint8_t>();
    if (!want_count) o->count = nullptr;
    u32* const info = stage_info(c);
    HIPCHK(c, hipMemsetAsync(info, 0, TXI_HALF_WORDS * sizeof(u32), c->stream));
    HIPCHK(c, hipMemsetAsync(d_tally, 0, NONCONV_TALLY * 8, c->stream));
    // as many blocks as stay resident (7 per CU: the 7 waves per SIMD the kernel's registers allow -- the walk waits on memory most of its
    // time, as k_meth_mbias does), each with its own tally, striding over the records
    if (!c->mt_cus) { int cus = 0; HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->dev)); c->mt_cus = cus > 0 ? cus : 1; }
    const unsigned grid = (unsigned)std::min<u64>((u64)c->mt_cus * 7, nblk(n * METH_GROUP, 256));
    prof_begin(c, "k_nonconv_walk");
    hipLaunchKernelGGL(k_nonconv_walk, dim3(grid), dim3(256), 0, c->stream, c->ix.gen2p, c->ix.chrom_start, raw, off, len, (long)n, paired ? 1 : 0, par, o->count, o->fail,
                       d_tally, info);
    prof_end(c);
    const u32* const got = c->h_info->stage;
    HIPCHK(c, hipMemcpyAsync(c->h_info->stage, info, 4 * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(tally, d_tally, NONCONV_TALLY * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    if (got[0]) { c->err = "nonconv: the length given for record " + std::to_string(~got[0]) + " is not its block_size + 4 (or is below the 36 bytes every BAM record has)"; return BMBS_EINVAL; }
    if (got[1]) { c->err = "nonconv: the read name, CIGAR, sequence and qualities of record " + std::to_string(~got[1]) + " do not fit its length"; return BMBS_EINVAL; }
    if (got[2]) { c->err = "nonconv: the refID of record " + std::to_string(~got[2]) + " is beyond the " + std::to_string(c->ix.n_chrom) + " sequences of the index"; return BMBS_EINVAL; }
    if (got[3]) { c->err = "nonconv: the reference span of record " + std::to_string(~got[3]) + " runs off its sequence"; return BMBS_EINVAL; }
    return BMBS_OK;
}

static int lane_bam_nonconv(Lane* c, const char* records, uint64_t bytes, const uint32_t* len, int64_t n_in, int32_t paired, const bmbs_nonconv_params* par_in,
                            bmbs_nonconv_count* count, uint8_t* fail, int64_t fail_cap, int64_t* n_tmpl, int64_t* n_fail, uint64_t* totals)
{
    if (!n_tmpl || !n_fail) { c->err = "nonconv: NULL argument"; return BMBS_EINVAL; }
    *n_tmpl = *n_fail = 0;
    if (totals) memset(totals, 0, 12 * sizeof(uint64_t));
    if (!c->attached) { c->err = "nonconv: no index attached"; return BMBS_ESTATE; }
    NonconvPar par;
    if (int rc = nonconv_get_params(c, par_in, &par)) return rc;
    if (int rc = records_check(c, "nonconv", records, bytes, len, n_in, true, paired != 0)) return rc;
    const u64 n = (u64)n_in, nt = paired ? n / 2 : n;
    *n_tmpl = (int64_t)nt;
    if ((int64_t)nt > fail_cap) { c->err = "nonconv: the array is too small (n_tmpl tells what is needed)"; return BMBS_ENOMEM; }
    if (!nt) return BMBS_OK;
    if (!fail || (bytes && !records)) { c->err = "nonconv: NULL buffer"; return BMBS_EINVAL; }
    HIPCHK(c, hipSetDevice(c->dev));
    RecIn& r = c->nc_in;
    if (int rc = records_stage(c, r, records, bytes, len, n, TOT_RECS_IN)) return rc;
    NonconvOut o;
    u64 tally[NONCONV_TALLY];
    if (int rc = nonconv_device(c, r.in.as<char>(), r.off.as<u64>(), r.len.as<u32>(), n, paired != 0, nt, par, count != nullptr, 0, &o, tally)) return rc;
    hipStream_t ds = down_stream_of(c);
    if (count) HIPCHK(c, hipMemcpyAsync(count, o.count, n * sizeof(bmbs_nonconv_count), hipMemcpyDeviceToHost, ds));
    HIPCHK(c, hipMemcpyAsync(fail, o.fail, nt, hipMemcpyDeviceToHost, ds));
    HIPCHK(c, hipStreamSynchronize(ds));
    *n_fail = (int64_t)tally[12];
    if (totals) memcpy(totals, tally, 12 * sizeof(uint64_t));
    return BMBS_OK;
}

static int lane_text_sorted_nonconv(Lane* c, const bmbs_nonconv_params* par_in, uint8_t* fail, int64_t cap, int64_t* n, int64_t* n_tmpl_failed, uint64_t* totals)
{
    if (!n || !n_tmpl_failed) { c->err = "sorted nonconv: NULL argument"; return BMBS_EINVAL; }
    *n = *n_tmpl_failed = 0;
    if (totals) memset(totals, 0, 12 * sizeof(uint64_t));
    if (!c->attached) { c->err = "sorted nonconv: no index attached"; return BMBS_ESTATE; }
    NonconvPar par;
    if (int rc = nonconv_get_params(c, par_in, &par)) return rc;
    const Lane::SortedText& t = c->st;
    if (t.lines < 0 || t.n < 0) {
        c->err = "sorted nonconv: the context's last text call was not a BMBS_TEXT_BAM_SORTED call that returned records, or another call has used its buffers since";
        return BMBS_ESTATE;
    }
    *n = t.n;
    if (t.n > cap) { c->err = "sorted nonconv: the array is too small (n tells what is needed)"; return BMBS_ENOMEM; }
    const u64 nr = (u64)t.n, lines = (u64)t.lines, nt = lines >> (t.pe ? 1 : 0);
    if (!nr || !nt) return BMBS_OK;
    if (!fail) { c->err = "sorted nonconv: NULL argument"; return BMBS_EINVAL; }
    HIPCHK(c, hipSetDevice(c->dev));
    NonconvOut o;
    u64 tally[NONCONV_TALLY];
    if (int rc = nonconv_device(c, c->bam_raw.as<char>(), c->sam_off.as<u64>(), c->sam_len.as<u32>(), lines, t.pe, nt, par, false, nr, &o, tally)) return rc;
    prof_begin(c, "k_nonconv_order");
    hipLaunchKernelGGL(k_nonconv_order, dim3(nblk(nr, 256)), dim3(256), 0, c->stream, o.fail, c->bs_idx2.as<u32>(), (long)nr, t.pe ? 1 : 0, o.out);
    prof_end(c);
    HIPCHK(c, hipMemcpyAsync(fail, o.out, nr, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    *n_tmpl_failed = (int64_t)tally[12];
    if (totals) memcpy(totals, tally, 12 * sizeof(uint64_t));
    return BMBS_OK;
}

// ---- the genome-wide cytosine report (k_cytosine.hip): the rule is in include/bmbs.h ------------------------------------------------------------
// The sites and runs go up, k_cyt_check looks at the sites, k_cyt_count at every genome word of the window, the scan says where each
// word's text goes (64-bit offsets: a window's text may pass 4 GB), and one wait brings back the refusals, the bytes and the lines.
// k_cyt_emit runs only when the caller's buffer holds the text.  Nothing of a methyl call's is read or written (Lane::mc, mt_*)
static int lane_methyl_report(Lane* c, int32_t ref, int64_t beg, int64_t end, const bmbs_methyl_site* site, int64_t n_site, const int64_t* run, int64_t n_run,
                              int32_t contexts, char* out, uint64_t cap, uint64_t* out_bytes, int64_t* n_line)
{
    if (out_bytes) *out_bytes = 0;
    if (n_line) *n_line = 0;
    if (!c->attached) { c->err = "methyl report: no index attached"; return BMBS_ESTATE; }
    if (c->n_refs != c->ix.n_chrom) { c->err = "methyl report: bmbs_sam_refs has not been given the index's reference names"; return BMBS_ESTATE; }
    if (!out_bytes || !n_line || n_site < 0 || n_run < 0 || (n_site && !site) || (n_run && !run)) { c->err = "methyl report: bad argument"; return BMBS_EINVAL; }
    if (ref < 0 || ref >= c->ix.n_chrom) { c->err = "methyl report: ref " + std::to_string(ref) + " is outside the " + std::to_string(c->ix.n_chrom) + " sequences of the index"; return BMBS_EINVAL; }
    HIPCHK(c, hipSetDevice(c->dev));
    u64 cs[2] = {0, 0}; u32 co[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(cs, c->ix.chrom_start + ref, sizeof cs, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(co, c->chrom_off.as<u32>() + ref, sizeof co, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t length = (int64_t)(cs[1] - cs[0]);
    if (beg < 0 || beg > end || end > length) {
        c->err = "methyl report: the window [" + std::to_string(beg) + ", " + std::to_string(end) + ") does not lie in the " + std::to_string(length) + " bases of sequence " + std::to_string(ref);
        return BMBS_EINVAL;
    }
    if (contexts < 1 || contexts > 7) { c->err = "methyl report: contexts " + std::to_string(contexts) + " is outside 1..7 (1 CpG | 2 CHG | 4 CHH)"; return BMBS_EINVAL; }
    for (int64_t r = 0; r < n_run; r++)
        if (run[2 * r] >= run[2 * r + 1] || run[2 * r] < (r ? run[2 * r - 1] : 0)) { c->err = "methyl report: run " + std::to_string(r) + " is empty, out of order or overlaps its predecessor"; return BMBS_EINVAL; }
    if (n_site >= (1ll << 31)) { c->err = "methyl report: 2^31 sites and more"; return BMBS_EINVAL; }
    CytPar P;
    P.gen2p = c->ix.gen2p; P.s_lo = (long)cs[0]; P.s_hi = (long)cs[1]; P.a0 = P.s_lo + beg; P.a1 = P.s_lo + end;
    P.W0 = P.a0 >> 5; P.nW = end > beg ? ((P.a1 - 1) >> 5) - P.W0 + 1 : 0;
    P.n_site = n_site; P.n_run = n_run; P.name = c->chrom_chars.as<char>() + co[0]; P.name_len = co[1] - co[0]; P.contexts = (u32)contexts;
    const u64 nW = (u64)P.nW;
    ENS(c, c->cy_site, (u64)n_site * sizeof(bmbs_methyl_site) + 64); ENS(c, c->cy_run, (u64)n_run * 16 + 64);
    ENS(c, c->cy_cnt, nW * 4 + 64); ENS(c, c->cy_off, (nW + 1) * 8 + 64);
    P.site = c->cy_site.as<bmbs_methyl_site>(); P.run = c->cy_run.as<long>();
    if (n_site || n_run) {
        std::lock_guard<std::mutex> up(g_h2d_mu[c->dev & 15]);
        hipStream_t us = up_stream_of(c);
        if (n_site) HIPCHK(c, hipMemcpyAsync(c->cy_site.p, site, (size_t)n_site * sizeof(bmbs_methyl_site), hipMemcpyHostToDevice, us));
        if (n_run) HIPCHK(c, hipMemcpyAsync(c->cy_run.p, run, (size_t)n_run * 16, hipMemcpyHostToDevice, us));
        HIPCHK(c, hipStreamSynchronize(us));
    }
    u32* const info = stage_info(c);
    HostInfo* const hi = c->h_info;
    HIPCHK(c, hipMemsetAsync(info, 0, TXI_HALF_WORDS * sizeof(u32), c->stream));
    HIPCHK(c, hipMemsetAsync(tot_at(c, TOT_CYT_BYTES), 0, sizeof hi->cyt, c->stream));
    if (n_site) hipLaunchKernelGGL(k_cyt_check, dim3(nblk((u64)n_site, 256)), dim3(256), 0, c->stream, P, (int)ref, info);
    if (nW) {
        hipLaunchKernelGGL(k_cyt_count, dim3(nblk(nW, 256)), dim3(256), 0, c->stream, P, c->cy_cnt.as<u32>(), reinterpret_cast<unsigned long long*>(tot_at(c, TOT_CYT_LINES)));
        if (int rc = scan_u32(c, c->cy_cnt.as<u32>(), nW, c->cy_off.as<u64>(), TOT_CYT_BYTES)) return rc;
    }
    HIPCHK(c, hipMemcpyAsync(hi->stage, info, TXI_CYT_WORDS * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hi->cyt, tot_at(c, TOT_CYT_BYTES), sizeof hi->cyt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    // the first offender among the sites, and of its faults the first in the order of the list
    static const char* const fault[TXI_CYT_WORDS] = {
        "has another ref than the call", "lies outside the window [beg, end)", "does not sit at a larger pos than its predecessor",
        "has a kind that is not what the genome says at its position", "is of a context that is not selected", "has a window that touches a run"};
    int64_t bad = -1; int why = 0;
    for (int x = 0; x < TXI_CYT_WORDS; x++) if (hi->stage[x] && (bad < 0 || (int64_t)~hi->stage[x] < bad)) { bad = (int64_t)~hi->stage[x]; why = x; }
    if (bad >= 0) { c->err = "methyl report: site " + std::to_string(bad) + " " + fault[why]; return BMBS_EINVAL; }
    const u64 total = hi->cyt[0];
    *out_bytes = total; *n_line = (int64_t)hi->cyt[1];
    if (total > cap) { c->err = "methyl report: the output buffer is too small (out_bytes tells what is needed)"; return BMBS_ENOMEM; }
    if (!total) return BMBS_OK;
    if (!out) { c->err = "methyl report: NULL buffer"; return BMBS_EINVAL; }
    ENS(c, c->cy_out, total + 64);
    hipLaunchKernelGGL(k_cyt_emit, dim3(nblk(nW, CYT_WPB)), dim3(256), 0, c->stream, P, c->cy_off.as<u64>(), c->cy_out.as<char>());
    HIPCHK(c, hipGetLastError());
    return download_locked(c, out, c->cy_out.as<char>(), total, c->stream, nullptr);
}

extern "C" int bmbs_methyl_report(bmbs_ctx* X, int32_t ref, int64_t beg, int64_t end, const bmbs_methyl_site* site, int64_t n_site, const int64_t* run, int64_t n_run,
                                  int32_t contexts, char* out, uint64_t cap, uint64_t* out_bytes, int64_t* n_line)
{ ON_LANE0(lane_methyl_report(c, ref, beg, end, site, n_site, run, n_run, contexts, out, cap, out_bytes, n_line)); }
extern "C" int bmbs_text_sorted_index(bmbs_ctx* X, uint64_t* key, uint32_t* len, int64_t cap, int64_t* n) { ON_LANE0(lane_text_sorted_index(c, key, len, cap, n)); }
extern "C" int bmbs_bam_sort(bmbs_ctx* X, const char* records, uint64_t bytes, const uint32_t* len, int64_t n, int32_t flags, char* out, uint64_t out_cap, uint64_t* out_bytes)
{ ON_LANE0(lane_bam_sort(c, records, bytes, len, n, flags, out, out_cap, out_bytes)); }
extern "C" int bmbs_bam_sort_index(bmbs_ctx* X, bmbs_bai_chunk* chunk, int64_t chunk_cap, int64_t* n_chunk, bmbs_bai_win* win, int64_t win_cap, int64_t* n_win,
                                   bmbs_bai_ref* ref, int64_t ref_cap, int64_t* n_ref, uint64_t* n_no_coor)
{ ON_LANE0(lane_bam_sort_index(c, chunk, chunk_cap, n_chunk, win, win_cap, n_win, ref, ref_cap, n_ref, n_no_coor)); }
extern "C" int bmbs_bam_dup_sigs(bmbs_ctx* X, const char* records, uint64_t bytes, const uint32_t* len, int64_t n, int32_t paired, bmbs_dup_sig* sig, int64_t sig_cap,
                                 int64_t* n_sig)
{ ON_LANE0(lane_bam_dup_sigs(c, records, bytes, len, n, paired, sig, sig_cap, n_sig)); }
extern "C" int bmbs_text_sorted_dup(bmbs_ctx* X, bmbs_dup_sig* sig, int64_t sig_cap, int64_t* n_sig, uint32_t* tmpl, int64_t cap, int64_t* n)
{ ON_LANE0(lane_text_sorted_dup(c, sig, sig_cap, n_sig, tmpl, cap, n)); }
extern "C" int bmbs_dup_select(bmbs_ctx* X, const bmbs_dup_sig* sig, int64_t n, uint8_t* dup, int64_t* n_dup) { ON_LANE0(lane_dup_select(c, sig, n, dup, n_dup)); }
extern "C" int bmbs_bam_methyl(bmbs_ctx* X, const char* records, uint64_t bytes, const uint32_t* len, int64_t n, const uint32_t* clip, const bmbs_methyl_params* par, int64_t* n_site)
{ ON_LANE0(lane_bam_methyl(c, records, bytes, len, n, clip, par, nullptr, false, n_site)); }
extern "C" int bmbs_bam_sort_methyl(bmbs_ctx* X, const uint32_t* clip, const bmbs_methyl_params* par, int64_t* n_site) { ON_LANE0(lane_bam_sort_methyl(c, clip, par, nullptr, false, n_site)); }
extern "C" int bmbs_bam_methyl_opts(bmbs_ctx* X, const char* records, uint64_t bytes, const uint32_t* len, int64_t n, const uint32_t* clip, const bmbs_methyl_opts* opts, int64_t* n_site)
{ ON_LANE0(lane_bam_methyl(c, records, bytes, len, n, clip, nullptr, opts, false, n_site)); }
extern "C" int bmbs_bam_sort_methyl_opts(bmbs_ctx* X, const uint32_t* clip, const bmbs_methyl_opts* opts, int64_t* n_site) { ON_LANE0(lane_bam_sort_methyl(c, clip, nullptr, opts, false, n_site)); }
extern "C" int bmbs_methyl_mbias(bmbs_ctx* X, uint64_t* table, int64_t cap, int64_t* n) { ON_LANE0(lane_methyl_mbias(c, table, cap, n)); }
extern "C" int bmbs_methyl_sites(bmbs_ctx* X, bmbs_methyl_site* site, int64_t cap, int64_t* n) { ON_LANE0(lane_methyl_sites(c, site, cap, n)); }
extern "C" int bmbs_bam_methyl_opposite(bmbs_ctx* X, const char* records, uint64_t bytes, const uint32_t* len, int64_t n, const uint32_t* clip, const bmbs_methyl_opts* opts, int64_t* n_entry)
{ ON_LANE0(lane_bam_methyl(c, records, bytes, len, n, clip, nullptr, opts, true, n_entry)); }
extern "C" int bmbs_bam_sort_methyl_opposite(bmbs_ctx* X, const uint32_t* clip, const bmbs_methyl_opts* opts, int64_t* n_entry) { ON_LANE0(lane_bam_sort_methyl(c, clip, nullptr, opts, true, n_entry)); }
extern "C" int bmbs_methyl_opposite(bmbs_ctx* X, bmbs_methyl_site* entry, int64_t cap, int64_t* n) { ON_LANE0(lane_methyl_opposite(c, entry, cap, n)); }
extern "C" int bmbs_methyl_drop_variants(bmbs_methyl_site* site, int64_t n_site, const bmbs_methyl_site* opp, int64_t n_opp, int32_t min_opposite_depth, int32_t max_variant_ppm, int64_t* n_kept)
{ return methyl_drop_variants(site, n_site, opp, n_opp, min_opposite_depth, max_variant_ppm, n_kept); }
extern "C" int bmbs_text_sorted_clip(bmbs_ctx* X, uint32_t* clip, int64_t cap, int64_t* n) { ON_LANE0(lane_text_sorted_clip(c, clip, cap, n)); }
extern "C" int bmbs_bam_nonconv(bmbs_ctx* X, const char* records, uint64_t bytes, const uint32_t* len, int64_t n, int32_t paired, const bmbs_nonconv_params* par,
                                bmbs_nonconv_count* count, uint8_t* fail, int64_t fail_cap, int64_t* n_tmpl, int64_t* n_fail, uint64_t* totals)
{ ON_LANE0(lane_bam_nonconv(c, records, bytes, len, n, paired, par, count, fail, fail_cap, n_tmpl, n_fail, totals)); }
extern "C" int bmbs_text_sorted_nonconv(bmbs_ctx* X, const bmbs_nonconv_params* par, uint8_t* fail, int64_t cap, int64_t* n, int64_t* n_tmpl_failed, uint64_t* totals)
{ ON_LANE0(lane_text_sorted_nonconv(c, par, fail, cap, n, n_tmpl_failed, totals)); }
