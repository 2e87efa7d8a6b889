// bitmapperbs_amd/csrc/bmbs_api.hip -- C-ABI (include/bmbs.h) over the gfx950 kernels.
// Owns the device buffers, the stream, the HIP-event profile and the per-ctx counters.  There is no
// CPU fallback anywhere in this library: without a HIP device every entry point fails with
// BMBS_ENODEV.
#include "bmbs_host.h"
#include "bmbs_kernels.hip"



// zero: the buffer is cleared when it is (re)allocated (packed rows: the mask words behind a row's last piece are never written)
int ensure(Lane* c, DevBuf& b, size_t bytes, bool zero)
{
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return BMBS_OK;
    size_t want = bytes + bytes / 8 + 256;
    if (want <= ((size_t)256 << 20)) {              // larger ones keep a hipMalloc of their own (freed when they grow)
        // an arena buffer leaves its old region behind when it grows: growing by half bounds what a stream of slowly rising needs strands
        if (b.cap) want = std::min<size_t>(std::max(want, b.cap + b.cap / 2), (size_t)256 << 20);
        void* p = c->arena.alloc(want);
        if (!p) { c->err = "out of device memory (lane arena)"; return BMBS_ENOMEM; }
        if (b.p && !b.arena) (void)hipFree(b.p);
        b.p = p; b.cap = want; b.arena = true;
    } else {
        if (b.p && !b.arena) (void)hipFree(b.p);
        b.p = nullptr; b.cap = 0; b.arena = false;
        hipError_t e = hipMalloc(&b.p, want);
        if (e != hipSuccess) { c->err = std::string("hipMalloc: ") + hipGetErrorString(e); b.p = nullptr; return BMBS_ENOMEM; }
        b.cap = want;
    }
    if (zero && hipMemsetAsync(b.p, 0, want, c->stream) != hipSuccess) { c->err = "hipMemsetAsync failed"; return BMBS_ESTATE; }
    return BMBS_OK;
}
void release(DevBuf& b) { if (b.p && !b.arena) (void)hipFree(b.p); b.p = nullptr; b.cap = 0; b.arena = false; }

void prof_begin(Lane* c, const char* name)
{
    std::vector<Prof>& set = c->profset[c->cur_slot];
    int& used = c->prof_used[c->cur_slot];
    if ((size_t)used == set.size()) {
        Prof p; p.name = name; p.used = false;
        (void)hipEventCreate(&p.a); (void)hipEventCreate(&p.b);
        set.push_back(p);
    }
    Prof& p = set[(size_t)used];
    p.name = name; p.used = true;
    (void)hipEventRecord(p.a, c->stream);
}
void prof_end(Lane* c) { (void)hipEventRecord(c->profset[c->cur_slot][(size_t)c->prof_used[c->cur_slot]].b, c->stream); c->prof_used[c->cur_slot]++; }
// the time between two events of completed work -> the running sums
float prof_add(Lane* c, const char* name, hipEvent_t a, hipEvent_t b)
{
    float t = 0;
    if (hipEventElapsedTime(&t, a, b) != hipSuccess) t = 0.f;
    for (auto& s : c->acc) if (s.name == name || !strcmp(s.name, name)) { s.ms += t; return t; }
    c->acc.push_back({name, (double)t});
    return t;
}
// the events of a call whose stream work has completed -> `last` and the running sums
void prof_collect(Lane* c, int slot)
{
    c->last.clear();
    for (int i = 0; i < c->prof_used[slot]; i++) {
        const Prof& p = c->profset[slot][(size_t)i];
        c->last.push_back({p.name, (double)prof_add(c, p.name, p.a, p.b)});
    }
    c->acc_calls++;
}

// exclusive scan u32[n] -> u64[n+1], total left in the lane's word `slot` (bmbs_words.h); n_dev: a device-side count that bounds n (see k_scan_partial)
// Two launches (tile sums, offsets) by default; BMBS_SCAN_CHAIN=1: one (k_scan_chain).
int scan_u32(Lane* c, const u32* in, u64 n, u64* out, Tot slot, u32* list, int nz, const u64* n_dev)
{
    const u64 per = (u64)SCAN_BLOCK * SCAN_ITEMS;
    const u64 nb = n ? (n + per - 1) / per : 1;
    if (!c->kn.scan_chain) {
        ENS(c, c->scan_tmp, (nb + 1) * 8);
        u64* bs = c->scan_tmp.as<u64>();
        hipLaunchKernelGGL(k_scan_partial, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, c->stream, in, n, bs, nz, n_dev);
        hipLaunchKernelGGL(k_scan_final, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, c->stream, in, n, bs, out, list, nz, n_dev, tot_at(c, slot));
        return BMBS_OK;
    }
    // status words: zeroed when the buffer is (re)allocated and when the epoch wraps, so no word of an earlier scan carries this scan's epoch
    const u64 nt = (nb + SCAN_SUB - 1) / SCAN_SUB;                  // a ticket per SCAN_SUB tiles
    { int rc = ensure(c, c->scan_tmp, (nb + 1) * 8, true); if (rc) return rc; }
    { int rc = ensure(c, c->scan_ticket, 64, true); if (rc) return rc; }
    if (++c->scan_epoch >= SCAN_EPOCH_MAX) {
        if (hipMemsetAsync(c->scan_tmp.p, 0, c->scan_tmp.cap, c->stream) != hipSuccess) { c->err = "hipMemsetAsync failed"; return BMBS_ESTATE; }
        c->scan_epoch = 1;
    }
    hipLaunchKernelGGL(k_scan_chain, dim3((unsigned)nt), dim3(SCAN_BLOCK), 0, c->stream, in, n, out, list, nz, n_dev, tot_at(c, slot),
                       c->scan_ticket.as<unsigned int>(), c->scan_ticket_base, c->scan_tmp.as<u64>(), c->scan_epoch);
    c->scan_ticket_base += (u32)nt;
    return BMBS_OK;
}

// capacity for a device-side count of a call that does not wait for it: what earlier calls needed per read, plus a margin
inline u64 cap_from(double need_per_read, u64 n_reads, u64 floor_, double scale = 1.0)
{
    const u64 c = (u64)(scale * (need_per_read * 1.25 * (double)n_reads + 64.0 * std::sqrt((double)n_reads + 1.0) + 1024.0));
    return c > floor_ ? c : floor_;
}

// MismatchPenaltyByQuality (ksw.h:148-161): mp_min + (int)(min(Q - q_base, 40) / 40 * (mp_max - mp_min)), every step in IEEE double
// as the reference evaluates it (the product is tabulated once per context: pen_lut)
int mismatch_penalty(const bmbs_params& P, int Q)
{
    const double phred = std::min<double>(Q - P.q_base, 40.0) / 40;
    return (int)(phred * (P.mp_max - P.mp_min)) + P.mp_min;
}

// The smallest and the largest penalty a mismatching cell can take: mismatch_penalty over all 256 quality bytes.  Not [mp_min, mp_max]:
// nothing keeps mp_min below mp_max (then the largest is mp_min or more), and a byte below q_base (--phred64 on Phred+33 data) takes
// the formula outside both ends, below zero too -- such a mismatch RAISES the score.
void mismatch_penalty_range(const bmbs_params& P, int* lo, int* hi)
{
    *lo = *hi = mismatch_penalty(P, 0);
    for (int b = 1; b < 256; b++) { const int p = mismatch_penalty(P, b); *lo = std::min(*lo, p); *hi = std::max(*hi, p); }
}

// The penalty classes of the quality bytes (bmbs_qual_classes): the distinct values of mismatch_penalty over the 256 bytes, largest
// first, the 16 largest numbered 0..15; class_of[b] = 0xFF for a byte whose penalty is not among them.  rep[c] (may be null) = the
// smallest byte of class c, what k_qual_expand writes for it (classes that do not exist: rep[0]).
void qual_class_table(const bmbs_params& P, uint8_t class_of[256], int32_t penalty_of[16], int32_t* n_classes, uint8_t rep[16])
{
    int pen[256];
    for (int b = 0; b < 256; b++) pen[b] = mismatch_penalty(P, b);
    std::vector<int> v(pen, pen + 256);
    std::sort(v.begin(), v.end(), [](int a, int b) { return a > b; });
    v.erase(std::unique(v.begin(), v.end()), v.end());
    const int nc = (int)std::min<size_t>(16, v.size());
    for (int c = 0; c < 16; c++) penalty_of[c] = c < nc ? v[(size_t)c] : 0;
    for (int b = 255; b >= 0; b--) {
        class_of[b] = 0xFF;
        for (int c = 0; c < nc; c++) if (pen[b] == v[(size_t)c]) { class_of[b] = (uint8_t)c; if (rep) rep[c] = (uint8_t)b; break; }
    }
    if (rep) for (int c = nc; c < 16; c++) rep[c] = rep[0];
    *n_classes = nc;
}

// MAP_Calculation (Schema.cpp:168-405) as data.  The reference's ladder of `if`s compares two ratios -- the runner-up's distance in
// edits over the threshold (rank_error) and the winner's score above the worst admissible score over that range (rank) -- with
// fixed cut points; the tables below are those cut points and the MAPQ each cell returns.  The ratios are formed and compared in
// double exactly as there; the result is tabulated per threshold on the host (prepare_luts) and only looked up on the device.
int map_calculation(const bmbs_params& P, unsigned second_best_diff, unsigned error_threshold, int best_score)
{
    const int unit = std::max(P.gap_open + P.gap_ext, P.mp_max);
    const int worst = -unit * (int)error_threshold;                 // scoreMax of the reference
    const double rank = (double)std::max(best_score - worst, 0) / (double)(-worst);
    const unsigned ediff = second_best_diff > error_threshold ? error_threshold + 1 : second_best_diff;
    if (ediff > error_threshold) {
        // no runner-up within the threshold: the score alone decides
        static const struct { double at; int q; } alone[] = {{0.8, 42}, {0.7, 40}, {0.6, 24}, {0.5, 23}, {0.4, 8}, {0.3, 3}};
        for (const auto& r : alone) if (rank >= r.at) return r.q;
        return 0;
    }
    const double rerr = (double)(int)ediff / (double)error_threshold;
    const bool perfect = best_score == 0;
    // rows: rank_error >= at; `zero` for a perfect winner, otherwise the first column whose rank cut is reached (hi, mid), else lo
    static const struct { double at; int zero; double hi_cut; int hi; double mid_cut; int mid; int lo; } rows[] = {
        {0.9, 39, 0.0, 33, 0.0, 33, 33}, {0.8, 38, 0.0, 27, 0.0, 27, 27}, {0.7, 37, 0.0, 26, 0.0, 26, 26}, {0.6, 36, 0.0, 22, 0.0, 22, 22},
        {0.5, 35, 0.84, 25, 0.68, 16, 5}, {0.4, 34, 0.84, 21, 0.68, 14, 4},
        {0.3, 32, 0.88, 18, 0.67, 15, 3}, {0.2, 31, 0.88, 17, 0.67, 11, 0}, {0.1, 30, 0.88, 12, 0.67, 7, 0},
    };
    for (const auto& r : rows)
        if (rerr >= r.at) return perfect ? r.zero : rank >= r.hi_cut ? r.hi : rank >= r.mid_cut ? r.mid : r.lo;
    // runner-up (almost) as good as the winner
    return ediff == 0 ? (rank >= 0.67 ? 1 : 0) : (rank >= 0.67 ? 6 : 2);
}

int threshold_k(const bmbs_params& P, int L)
{
    u64 k = (u64)(P.e_f * L);            // error_threshold1 = thread_e_f * length (Schema.cpp:24546)
    if (k >= 31) k = 31;
    return (int)k;
}

// CIGAR operations one alignment can have, + slack: the slots per job in the cigar pool.  The DP (ksw.cpp:1850-2045) maximises the
// score inside the band; the alignment with <= k edits that the Myers filter found lies inside the band and scores at least
// -k * max(mp_max, np, gap_open + gap_ext), and every gap run of any alignment costs at least gap_open + gap_ext, so the optimum
// holds at most k * max(...) / (gap_open + gap_ext) gap runs and twice that + 1 operations.  With the default penalties (6, 1,
// 5 + 3) that is the 2k + 8 this code used for every parameter set -- until a random-parameter soak (tools/fuzz_parity.py) ran
// --gap_open 1 with mismatches at 8-9: gaps cheaper than mismatches, alignments with more runs than slots.
int cigar_ops_bound(const bmbs_params& P, int L, int k)
{
    const long goe = (long)P.gap_open + P.gap_ext;
    // the dearest mismatch is the largest entry of the penalty table, which is mp_max only while mp_min <= mp_max (the default penalties
    // and every set with mp_min <= mp_max give the same bound as before)
    int pen_lo, pen_hi;
    mismatch_penalty_range(P, &pen_lo, &pen_hi);
    const long worst = std::max<long>(std::max<long>(pen_hi, P.np), goe);
    long gaps = (long)L + 2 * k;
    if (goe > 0) gaps = std::min<long>(gaps, (long)k * worst / goe);
    return (int)std::min<long>(2 * gaps + 8, 1 << 20);
}
// n_cigar of a record is 8 bits, 255 marks "more operations than slots" (cannot happen with the bound above)
#define BMBS_MAX_RECORD_OPS 254

// MAP_Calculation tables for every error_threshold 0..62 (k for single-end, k1+k2 for pairs), concatenated:
// table t = (t+2) x (unit*t+2) bytes at mapq_off[t]; plus klut[L] = the threshold of a read of length L.  Built once.
int prepare_luts(Lane* c)
{
    if (c->luts_ready) return BMBS_OK;
    int unit = c->prm.gap_open + c->prm.gap_ext;
    if (unit < c->prm.mp_max) unit = c->prm.mp_max;
    c->mapq_unit = unit;
    std::vector<u32> off(64, 0);
    std::vector<u8> lut;
    for (int k = 0; k <= 62; k++) {
        const int range = unit * k;
        off[k] = (u32)lut.size();
        // column range + 1 stands for every score above 0 (mismatches whose penalty is negative): all of them reach every rank cut
        // as score 0 does, but none is "perfect", so one column serves them all
        lut.resize(lut.size() + (size_t)(k + 2) * (range + 2));
        u8* t = lut.data() + off[k];
        for (int ed = 0; ed <= k + 1; ed++)
            for (int sd = 0; sd <= range + 1; sd++)
                t[(size_t)ed * (range + 2) + sd] = (u8)map_calculation(c->prm, (unsigned)ed, (unsigned)k, sd - range);
    }
    std::vector<u8> kl(1002);
    for (int L = 0; L <= 1001; L++) kl[L] = (u8)threshold_k(c->prm, L);
    ENS(c, c->mapq_lut, lut.size()); ENS(c, c->mapq_off, off.size() * 4); ENS(c, c->klut, kl.size());
    HIPCHK(c, hipMemcpyAsync(c->mapq_lut.p, lut.data(), lut.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->mapq_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->klut.p, kl.data(), kl.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->luts_ready = true;
    return BMBS_OK;
}

// geometry of a batch: fixed length (d_len == nullptr) or per-read lengths with L = the longest
ReadGeom geom(Lane* c, int L, const u16* d_len)
{
    ReadGeom g;
    g.len = d_len; g.klut = c->klut.as<u8>(); g.L = L; g.k = threshold_k(c->prm, L);
    return g;
}

int per_read_workspace(Lane* c, u64 n)
{
    ENS(c, c->verdict, n); ENS(c, c->n_seeds, n); ENS(c, c->multi, n); ENS(c, c->mm_site, n * 2);
    ENS(c, c->exit_site, n * 8); ENS(c, c->seeds, n * BMBS_MAX_SEEDS * sizeof(SeedRec));
    ENS(c, c->n_cand, n * 4); ENS(c, c->cand_off, (n + 1) * 8); ENS(c, c->n_votes, n * 4);
    ENS(c, c->best_site, n * 8); ENS(c, c->best_end, n * 4); ENS(c, c->best_err, n * 4); ENS(c, c->sbd, n * 4);
    ENS(c, c->red_status, n); ENS(c, c->job_flag, n * 4); ENS(c, c->job_off, (n + 1) * 8);
    return BMBS_OK;
}

ReadState read_state(Lane* c)
{
    ReadState s;
    s.verdict = c->verdict.as<u8>(); s.n_seeds = c->n_seeds.as<u8>(); s.multi = c->multi.as<u8>();
    s.mm_site = c->mm_site.as<u16>(); s.exit_site = c->exit_site.as<u64>(); s.seeds = c->seeds.as<SeedRec>();
    s.n_cand = c->n_cand.as<u32>(); s.cand_off = c->cand_off.as<u64>(); s.n_votes = c->n_votes.as<u32>();
    s.best_site = c->best_site.as<u64>(); s.best_end = c->best_end.as<int32_t>(); s.best_err = c->best_err.as<u32>();
    s.sbd = c->sbd.as<u32>(); s.red_status = c->red_status.as<u8>(); s.job_flag = c->job_flag.as<u32>();
    s.job_off = c->job_off.as<u64>();
    return s;
}

// trace slots of the register-band DP kernel: one per launched thread (<= 1 M: 16 k waves fill the chip several times over)
inline u64 sw_trace_slots(u64 n_jobs) { const u64 t = (u64)nblk(n_jobs, 64) * 64; return t < (1ull << 20) ? t : (1ull << 20); }

// LDS of the register-band DP kernels: the window words of every lane's alignment(s) (LdsWin)
inline size_t sw_window_lds(const ReadGeom& gm, int jobs_per_lane) { return (size_t)jobs_per_lane * ((gm.L + 2 * gm.k + 62) / 32 + 1) * 64 * 8; }

template <int KB>
void launch_sw(Lane* c, const char* d_seq, const char* d_qual, const char* d_qual2, const ReadGeom& gm, int stride, u64 n_jobs,
               const Jobs& jobs, u32 rev_from, u32* d_cigar_pool, int max_ops, const PackedRows& prw)
{
    const u64 slots = sw_trace_slots(n_jobs);
    const size_t lds = sw_window_lds(gm, 1);
    auto kern = gm.len ? k_align_sw<KB, false> : gm.k == KB ? k_align_sw<KB, true, true> : k_align_sw<KB, true, false>;
    for (u64 base = 0; base < n_jobs; base += slots)
        hipLaunchKernelGGL(kern, dim3((unsigned)(slots / 64)), dim3(64), lds, c->stream, c->ix, c->sp, c->pen_lut.as<int>(), d_seq,
                           d_qual, d_qual2, gm, stride, tot_at(c, TOT_SW), c->sw_job.as<u32>(), jobs, rev_from, c->trace.as<u64>(),
                           slots, base, d_cigar_pool, max_ops, c->a_start.as<int>(), c->a_end.as<int>(), c->a_nm.as<u32>(),
                           c->a_score.as<int>(), c->a_nops.as<int>(), prw);
}

// the packed form: two jobs per lane, so a launch of `slots` threads covers 2 * slots jobs
template <int KB>
void launch_sw2(Lane* c, const char* d_seq, const char* d_qual, const char* d_qual2, const ReadGeom& gm, int stride, u64 n_jobs,
                const Jobs& jobs, u32 rev_from, u32* d_cigar_pool, int max_ops, const PackedRows& prw)
{
    const u64 slots = sw_trace_slots((n_jobs + 1) / 2);
    auto kern = !prw.base ? k_align_sw2<KB, false, false> : gm.k == KB ? k_align_sw2<KB, true, true> : k_align_sw2<KB, false, true>;
    for (u64 base = 0; base < n_jobs; base += 2 * slots)
        hipLaunchKernelGGL(kern, dim3((unsigned)(slots / 64)), dim3(64), sw_window_lds(gm, 2), c->stream, c->ix, c->sp, c->pen_lut.as<int>(), d_seq,
                           d_qual, d_qual2, gm, stride, tot_at(c, TOT_SW), c->sw_job.as<u32>(), jobs, rev_from, c->trace.as<u64>(),
                           slots, base, d_cigar_pool, max_ops, c->a_start.as<int>(), c->a_end.as<int>(), c->a_nm.as<u32>(),
                           c->a_score.as<int>(), c->a_nops.as<int>(), prw);
}

// the band bounds the register-band DP kernels are instantiated for: f gets the smallest one that holds k, as a compile-time constant.
// The band loop is unrolled for KB: a tighter bound wastes fewer masked cells (k = 6 in a KB = 8 kernel idles 4 of 17)
template <class F>
void with_band_bound(int k, F&& f)
{
    if (k <= 2) f(std::integral_constant<int, 2>());
    else if (k <= 4) f(std::integral_constant<int, 4>());
    else if (k <= 6) f(std::integral_constant<int, 6>());
    else if (k <= 8) f(std::integral_constant<int, 8>());
    else if (k <= 10) f(std::integral_constant<int, 10>());
    else if (k <= 12) f(std::integral_constant<int, 12>());
    else if (k <= 16) f(std::integral_constant<int, 16>());
    else if (k <= 20) f(std::integral_constant<int, 20>());
    else if (k <= 24) f(std::integral_constant<int, 24>());
    else f(std::integral_constant<int, 31>());
}

// K11-K13 over n_jobs jobs: un-gapped recheck for all, scan-compact the ones that need the DP, run the
// register-band DP kernel instantiated for the smallest KB >= k.  No host round-trip inside.
// d_qual2: the qualities of the rows from rev_from on (mate 2), or nullptr; pr: the packed copy of the rows -- the empty one: ASCII rows.
// n_jobs bounds the job arrays and grids; n_jobs_dev (or nullptr) is where the device keeps the real count; sw_bound = the DP jobs the
// DP launches cover (a call that does not wait for its counts passes capacities here and lets k_guard_count check the last one;
// ~0: all of them)
int run_align(Lane* c, const char* d_seq, const char* d_qual, const char* d_qual2, const ReadGeom& gm, int stride, u64 n_jobs, const Jobs& jobs,
              u32 rev_from, u32* d_cigar_pool, int max_ops, const PackedRows& pr, const u64* n_jobs_dev, u64 sw_bound)
{
    if (sw_bound > n_jobs) sw_bound = n_jobs;
    const int L = gm.L, k = gm.k;              // the longest read and the largest threshold size the workspace
    const u64 nj = n_jobs ? n_jobs : 1;
    const u64 nwk = (u64)((2 * k + 1 + 15) / 16);
    ENS(c, c->a_start, nj * 4); ENS(c, c->a_end, nj * 4); ENS(c, c->a_nm, nj * 4); ENS(c, c->a_score, nj * 4); ENS(c, c->a_nops, nj * 4);
    ENS(c, c->need_sw, nj * 4); ENS(c, c->sw_off, (nj + 1) * 8); ENS(c, c->sw_job, nj * 4);
    if (!n_jobs) return BMBS_OK;
    // Three forms of the DP (BMBS_SW=reg2|reg|wave), all with identical results:
    //  reg2 (default for k >= 5; it was k >= 9 until the row loop lost a third of its instructions: k = 6 now 0.69 vs 0.73 ms):
    //        one PAIR of jobs per lane in packed 16-bit arithmetic, band in registers, trace bytes in HBM
    //        (k_align_sw2) -- the DP is VALU-issue bound, so instructions per cell is what counts: 30 per cell against 52.  Needs
    //        one read length per batch and scores that fit 16 bits.  Measured against `reg` on 10 M-pair / 10 M-read batches:
    //        k = 20 (250 bp) 2.63 vs 3.50 ms, k = 12 2.53 vs 2.69 ms, k = 6 1.02 vs 0.83 ms (narrow bands: the per-row work of two
    //        jobs outweighs the packed cells, and half as many waves balance worse) -- hence the threshold;
    //  reg:  one job per lane, 32-bit (k_align_sw) -- batches of mixed lengths, extreme penalties;
    //  wave: one job per 16 / 32 / 64 lanes, a band row per step, trace + CIGAR in LDS, nothing but the ops written to HBM
    //        (north_star (c)); measured 6.4x the instructions per job of `reg` (lanes beyond the band idle, the F prefix scan and
    //        its DPP wait states), so it only pays when there are too few jobs to fill the lanes.
    const int swm = c->kn.sw_form;
    const bool wave_form = swm == 3;
    // what one cell can move a score by, either way: the extremes of the penalty table (not mp_max: mismatch_penalty_range), np, one gap
    int pen_lo, pen_hi;
    mismatch_penalty_range(c->prm, &pen_lo, &pen_hi);
    int maxpen = std::max(std::max(std::max(pen_hi, -pen_lo), c->prm.np), c->prm.gap_open + c->prm.gap_ext);
    // The bound holds for ANY job, a stage call's with a window that fits nowhere included (every cell then costs np): L * maxpen.  Jobs
    // the filter accepted stay far inside it (H is a maximum over paths next to one with <= k edits), so a set like mp_max 2, mp_min 60
    // at 998 bases takes the 32-bit form although its accepted jobs would fit.  (gap_ext < 256 keeps the packed gap constants in their
    // halves; with gap_open >= 0 the product test already excludes it, it decides only if that test is ever loosened.)
    const bool packed = !wave_form && swm != 1 && (k >= 5 || swm == 2) && !gm.len && c->prm.gap_ext < 256 && (L + 64) * maxpen < 12000 &&
                        c->prm.mp_min >= 0 && c->prm.gap_ext >= 0 && c->prm.gap_open >= 0 && c->prm.np >= 0;
    const bool reg_form = !wave_form;
    if (reg_form) {
        const u64 nwords = packed ? (u64)((2 * k + 1 + 7) / 8) : nwk;
        const u64 slots = packed ? sw_trace_slots((sw_bound + 1) / 2) : sw_trace_slots(sw_bound);
        ENS(c, c->trace, slots * (u64)L * nwords * 8);
    }
    unsigned long long* cnt = c->counters.as<unsigned long long>();
    prof_begin(c, "k_align_ungapped");
    if (pr.base)
        hipLaunchKernelGGL(k_align_ungapped_p, dim3(nblk(n_jobs, 256)), dim3(256), 0, c->stream, c->ix, c->sp, c->pen_lut.as<int>(), d_seq, pr,
                           d_qual, d_qual2, gm, stride, n_jobs, n_jobs_dev, jobs, rev_from, c->a_start.as<int>(), c->a_end.as<int>(), c->a_nm.as<u32>(),
                           c->a_score.as<int>(), c->a_nops.as<int>(), c->need_sw.as<u32>(), cnt);
    else
        hipLaunchKernelGGL(k_align_ungapped, dim3(nblk(n_jobs, 256)), dim3(256), 0, c->stream, c->ix, c->sp, c->pen_lut.as<int>(), d_seq,
                           d_qual, d_qual2, gm, stride, n_jobs, n_jobs_dev, jobs, rev_from, c->a_start.as<int>(), c->a_end.as<int>(), c->a_nm.as<u32>(),
                           c->a_score.as<int>(), c->a_nops.as<int>(), c->need_sw.as<u32>(), cnt);
    prof_end(c);
    prof_begin(c, "scan_sw");
    int rc = scan_u32(c, c->need_sw.as<u32>(), n_jobs, c->sw_off.as<u64>(), TOT_SW, c->sw_job.as<u32>(), 0, n_jobs_dev);
    if (rc) return rc;
    prof_end(c);
    if (n_jobs_dev && reg_form && sw_bound < n_jobs)
        hipLaunchKernelGGL(k_guard_count, dim3(1), dim3(1), 0, c->stream, tot_at(c, TOT_SW), sw_bound, c->flags.as<u32>(), BMBS_FLAG_SW);
    prof_begin(c, "k_align_sw");
    if (!reg_form) {
        // one alignment per 16 / 32 / 64 lanes (band of 2k+1 cells), trace + CIGAR in LDS
        const size_t words = (size_t)sww_lds_words(L, k);
#define SWW_LAUNCH(LANES)                                                                                                             \
        hipLaunchKernelGGL((k_align_sw_wave<LANES>), dim3(nblk(n_jobs, 64 / LANES)), dim3(64), words * 4 * (64 / LANES), c->stream, c->ix, \
                           c->sp, c->pen_lut.as<int>(), d_seq, d_qual, d_qual2, gm, stride, tot_at(c, TOT_SW), c->sw_job.as<u32>(),   \
                           jobs, rev_from, d_cigar_pool, max_ops, c->a_start.as<int>(), c->a_end.as<int>(), c->a_nm.as<u32>(),          \
                           c->a_score.as<int>(), c->a_nops.as<int>(), pr)
        if (k <= 7) SWW_LAUNCH(16);
        else if (k <= 15) SWW_LAUNCH(32);
        else SWW_LAUNCH(64);
#undef SWW_LAUNCH
        prof_end(c);
        return BMBS_OK;
    }
    with_band_bound(k, [&](auto kb) {
        if (packed) launch_sw2<decltype(kb)::value>(c, d_seq, d_qual, d_qual2, gm, stride, sw_bound, jobs, rev_from, d_cigar_pool, max_ops, pr);
        else launch_sw<decltype(kb)::value>(c, d_seq, d_qual, d_qual2, gm, stride, sw_bound, jobs, rev_from, d_cigar_pool, max_ops, pr);
    });
    prof_end(c);
    return BMBS_OK;
}

// K1-K5: the four seeding kernels with their two work-list compactions (no host round-trip)
SeedCarry seed_carry(Lane* c)
{
    SeedCarry sc;
    sc.sp0 = c->sd_sp0.as<u64>(); sc.hits0 = c->sd_hits0.as<u32>(); sc.ml0 = c->sd_ml0.as<u16>(); sc.tm = c->sd_tm.as<u16>();
    sc.seed_id = c->sd_seed_id.as<u8>(); sc.clen = c->sd_clen.as<u32>(); sc.first_ml = c->sd_first_ml.as<u16>();
    sc.flag_c = c->sd_flag_c.as<u32>(); sc.flag_d = c->sd_flag_d.as<u32>(); sc.off_c = c->sd_off_c.as<u64>(); sc.off_d = c->sd_off_d.as<u64>();
    sc.list_c = c->sd_list_c.as<u32>(); sc.list_d = c->sd_list_d.as<u32>();
    return sc;
}

// packed copy of the read rows for the seeding kernels, k_seed_decide and the un-gapped recheck (default); BMBS_LEGACY=1 keeps the
// round-1 forms for A/B runs.  Paired end: the copy is a by-product of k_pe_prepare (+2.5 %); single end: a kernel of its own
// (k_pack_rows, 0.53 ms per 10 M reads) that the consumers win back (+1.8 %: 1463 -> 1489 M reads/s on configs[1]).
bool use_packed_rows(const Lane* c) { return !c->kn.rows_ascii; }
// the lane's packed rows (c->prow once it has been sized for the call) as the kernels take them; the empty one under BMBS_LEGACY=1,
// which every consumer reads as "ASCII rows"
PackedRows packed_rows(const Lane* c, const ReadGeom& gm)
{
    if (!use_packed_rows(c)) return PackedRows{nullptr, nullptr, 0, 0};
    return PackedRows{c->prow.as<u64>(), c->prow_dirty.as<u8>(), pack_words(gm.L), pack_base_words(gm.L)};
}

// trigram rank table: three backward extensions per gather pair (bmbs_dev.h: occ3).  4.5 bytes per row; built from the full SA and
// the 2-bit text on a stream of its own, checked against three single steps on a million rows before it is used.
// margin: HBM that has to stay free behind the table (the work buffers of calls still to come)
// -> false: there was no room for it this time (the caller may ask again behind a later call, when other contexts have gone)
bool occ3_build(Occ3Shared& o, u64 margin)
{
    const u64 rows = o.rows, nb = rows / 96 + 2, need = 27 * nb * 16;
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    if (free_b <= need + margin) return false;
    const u64 n_chunks = (nb + OCC3_CHUNK - 1) / OCC3_CHUNK;
    void *t3 = nullptr, *c3 = nullptr, *sums = nullptr;
    hipStream_t st = nullptr;
    bool ok = hipMalloc(&t3, need) == hipSuccess && hipMalloc(&c3, 64 * 8) == hipSuccess && hipMalloc(&sums, 27 * n_chunks * 8 + 64) == hipSuccess &&
              hipStreamCreate(&st) == hipSuccess;
    if (ok) {
        u32* flag = reinterpret_cast<u32*>(c3) + 2 * 60;                       // two spare words behind the 27 entries: overflow, mismatches
        (void)hipMemsetAsync(c3, 0, 64 * 8, st);
        hipLaunchKernelGGL(k_occ3_planes, dim3(8192), dim3(256), 0, st, o.base, rows, nb, reinterpret_cast<uint4*>(t3));
        hipLaunchKernelGGL(k_occ3_chunk_sums, dim3(nblk(27 * n_chunks, 256)), dim3(256), 0, st, reinterpret_cast<uint4*>(t3), nb, n_chunks, reinterpret_cast<u64*>(sums));
        hipLaunchKernelGGL(k_occ3_chunk_scan, dim3(1), dim3(64), 0, st, reinterpret_cast<u64*>(sums), n_chunks, flag);
        hipLaunchKernelGGL(k_occ3_apply, dim3(nblk(27 * n_chunks, 256)), dim3(256), 0, st, reinterpret_cast<uint4*>(t3), nb, n_chunks, reinterpret_cast<u64*>(sums));
        hipLaunchKernelGGL(k_occ3_c3, dim3(1), dim3(64), 0, st, o.base, reinterpret_cast<u64*>(c3));
        DevIndex probe = o.base;
        probe.occ3 = reinterpret_cast<const uint4*>(t3); probe.c3 = reinterpret_cast<const u64*>(c3); probe.nb3 = nb;
        const u64 n_check = 1u << 20;
        hipLaunchKernelGGL(k_occ3_check, dim3(nblk(n_check, 256)), dim3(256), 0, st, probe, rows, n_check, flag + 1);
        u32 h[2] = {1, 1};
        ok = hipMemcpyAsync(h, flag, 8, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess && h[0] == 0 && h[1] == 0;
        if (!ok && getenv("BMBS_VERBOSE")) fprintf(stderr, "[bmbs] trigram table not used: count overflow %u, differences from three single steps %u\n", h[0], h[1]);
    }
    if (st) (void)hipStreamDestroy(st);
    if (sums) (void)hipFree(sums);
    if (ok) { o.occ3 = t3; o.c3 = c3; o.nb3 = nb; }
    else { if (t3) (void)hipFree(t3); if (c3) (void)hipFree(c3); }
    return true;
}
// called where a lane decides which seeding kernels to launch, and when a settled call has told it how long its chains are: builds the
// table once for all users of the index when this lane would use it, and adopts it when someone has built it
void occ3_want(Lane* c, bool behind_a_call)
{
    if (c->ix.occ3 || !c->o3 || c->kn.kgram < 1 || !use_packed_rows(c)) return;
    const bool wants = c->kn.kgram >= 2 || c->lr_chain >= 3.0;
    std::lock_guard<std::mutex> l(c->o3->mu);
    // (behind a settled call the lane's work buffers exist already -- the table needs little room beside itself; in front of a context's
    // first call, BMBS_KGRAM=2, room for them is left)
    // (`tried` stays clear when the build was skipped for lack of room -- at most eight such attempts, so a device that stays full is not
    // asked for its free memory behind every call.  A lane that sizes its work buffers AFTER the table was built can still meet
    // BMBS_ENOMEM on a device this full: bmbs_reserve() in front of the first call takes the buffers first.)
    if (!c->o3->occ3 && wants && !c->o3->tried) {
        (void)hipSetDevice(c->dev);
        const bool attempted = occ3_build(*c->o3, behind_a_call ? (8ull << 30) : (40ull << 30));
        if (attempted || ++c->o3->skipped >= 8) c->o3->tried = true;
    }
    if (c->o3->occ3) { c->ix.occ3 = reinterpret_cast<const uint4*>(c->o3->occ3); c->ix.c3 = reinterpret_cast<const u64*>(c->o3->c3); c->ix.nb3 = c->o3->nb3; }
}

int launch_seeding(Lane* c, const char* d_seq, const ReadGeom& gm, int stride, u64 n, int pe_mode, bool prepacked)
{
    ENS(c, c->sd_sp0, n * 8); ENS(c, c->sd_hits0, n * 4); ENS(c, c->sd_ml0, n * 2); ENS(c, c->sd_tm, n * 2); ENS(c, c->sd_seed_id, n);
    ENS(c, c->sd_clen, n * 4); ENS(c, c->sd_first_ml, n * 2); ENS(c, c->sd_flag_c, n * 4); ENS(c, c->sd_flag_d, n * 4);
    ENS(c, c->sd_off_c, (n + 1) * 8); ENS(c, c->sd_off_d, (n + 1) * 8); ENS(c, c->sd_list_c, n * 4); ENS(c, c->sd_list_d, n * 4);
    SeedCarry sc = seed_carry(c);
    ReadState st = read_state(c);
    unsigned long long* cnt = c->counters.as<unsigned long long>();
    const unsigned chunks = nblk(n, SEED_CHUNK);
    const unsigned chunks_min = nblk(n, SEED_CHUNK_MIN);      // grid for the device-sized chunks of the two work lists
    const int target_waves = c->kn.seed_waves;
    // packed copy of the rows (2 bits per base + a not-ACGT bit plane, whole 64-byte lines: one for 150 bases): what the seeding engine and
    // k_seed_decide read instead of the ASCII rows; BMBS_LEGACY=1 keeps the round-1 forms (A/B runs)
    const bool packed = use_packed_rows(c);
    if (packed && !prepacked) {
        const int pwords = pack_words(gm.L), W = pack_base_words(gm.L);
        { int rz_ = ensure(c, c->prow, n * (u64)pwords * 8 + 64, true); if (rz_) return rz_; } ENS(c, c->prow_dirty, n + 64);
        HIPCHK(c, hipMemsetAsync(c->prow_dirty.p, 0, n + 64, c->stream));
        prof_begin(c, "k_pack_rows");
        hipLaunchKernelGGL(k_pack_rows, dim3(nblk(n * (u64)(stride / 16), 256)), dim3(256), 0, c->stream, d_seq, gm, stride, (long)n,
                           c->prow.as<u64>(), pwords, W, c->prow_dirty.as<u32>());
        prof_end(c);
    }
    const PackedRows pr = packed_rows(c, gm);
    prof_begin(c, "k_seed_first");
    // three-letter index steps (DevIndex::occ3): their kernels hold more registers (one or two waves per SIMD fewer), which costs a
    // few per cent where chains are short -- so they are used once the context has seen long ones (BMBS_KGRAM=2: always, 0: never)
    occ3_want(c, false);
    const bool kg = c->ix.occ3 && packed && (c->kn.kgram >= 2 || (c->kn.kgram == 1 && c->lr_chain >= 3.0));
    // BMBS_SEED_STAGE=1 (default): k_seed_first's results written coalesced through LDS, k_seed_decide_p's exit-A record not stored (0: the round-6 forms)
    const int stage = c->kn.seed_stage;
    if (packed && kg && stage) hipLaunchKernelGGL((k_seed_first<true, true, true>), dim3(chunks), dim3(64), 0, c->stream, c->ix, d_seq, pr, gm, stride, (long)n, sc, cnt);
    else if (packed && kg) hipLaunchKernelGGL((k_seed_first<true, true>), dim3(chunks), dim3(64), 0, c->stream, c->ix, d_seq, pr, gm, stride, (long)n, sc, cnt);
    else if (packed && stage) hipLaunchKernelGGL((k_seed_first<true, false, true>), dim3(chunks), dim3(64), 0, c->stream, c->ix, d_seq, pr, gm, stride, (long)n, sc, cnt);
    else if (packed) hipLaunchKernelGGL(k_seed_first<true>, dim3(chunks), dim3(64), 0, c->stream, c->ix, d_seq, pr, gm, stride, (long)n, sc, cnt);
    else hipLaunchKernelGGL(k_seed_first<false>, dim3(chunks), dim3(64), 0, c->stream, c->ix, d_seq, pr, gm, stride, (long)n, sc, cnt);
    prof_end(c);
    prof_begin(c, "k_seed_decide");
    // rows staged through LDS (each read fetched from HBM exactly once, coalesced) + 8 characters per compare step.  (An
    // 8-lanes-per-read form without staging was measured at 2.07 ms against 1.36 ms; the un-staged and the one-character forms of
    // round 1 were removed in round 4.)
    const bool lds_ok = (size_t)64 * (stride + 8) <= 48 * 1024;
    if (packed)
        hipLaunchKernelGGL(k_seed_decide_p, dim3(nblk(n, 64)), dim3(64), (size_t)64 * (pr.pwords + 1) * 8, c->stream, c->ix, d_seq, pr, gm, stride,
                           (long)n, c->prm.seed_len, pe_mode, (stage && !(pe_mode && c->prm.sensitive)) ? 1 : 0, st, sc, cnt);   // k_pes_reseed reads it
    else if (lds_ok)
        hipLaunchKernelGGL((k_seed_decide<true, true>), dim3(nblk(n, 64)), dim3(64), (size_t)64 * (stride + 8), c->stream, c->ix, d_seq, gm,
                           stride, (long)n, c->prm.seed_len, pe_mode, st, sc, cnt);
    else
        hipLaunchKernelGGL((k_seed_decide<false, true>), dim3(nblk(n, 256)), dim3(256), 0, c->stream, c->ix, d_seq, gm, stride, (long)n,
                           c->prm.seed_len, pe_mode, st, sc, cnt);
    prof_end(c);
    prof_begin(c, "list_second");
    int rc = scan_u32(c, sc.flag_c, n, sc.off_c, TOT_SEED_SECOND, sc.list_c);          // scan + list in one pass
    if (rc) return rc;
    prof_end(c);
    prof_begin(c, "k_seed_second");
    if (packed && kg) hipLaunchKernelGGL((k_seed_second<true, true>), dim3(chunks_min), dim3(64), 0, c->stream, c->ix, d_seq, pr, gm, stride, tot_at(c, TOT_SEED_SECOND), target_waves, pe_mode, st, sc, cnt);
    else if (packed) hipLaunchKernelGGL(k_seed_second<true>, dim3(chunks_min), dim3(64), 0, c->stream, c->ix, d_seq, pr, gm, stride, tot_at(c, TOT_SEED_SECOND), target_waves, pe_mode, st, sc, cnt);
    else hipLaunchKernelGGL(k_seed_second<false>, dim3(chunks_min), dim3(64), 0, c->stream, c->ix, d_seq, pr, gm, stride, tot_at(c, TOT_SEED_SECOND), target_waves, pe_mode, st, sc, cnt);
    prof_end(c);
    prof_begin(c, "list_extra");
    rc = scan_u32(c, sc.flag_d, n, sc.off_d, TOT_SEED_EXTRA, sc.list_d);
    if (rc) return rc;
    prof_end(c);
    prof_begin(c, "k_seed_extra");
    {
        // the rows of a wave's 64 reads staged in LDS (k_seed_extra); rows too long for 64 KB stay in global memory
        const size_t lds = 64 * (size_t)(stride + 16);
        // ... and, measured, only while the index gathers are short: on a GRCh38-size index (wide forms) every gather is an HBM
        // round trip and the 11 KB of LDS per wave cost more occupancy (3.5 instead of 8 waves per SIMD) than the coalesced rows
        // save: 4.20 ms with LDS rows, 3.93 ms without on the configs[2] batch
        const bool wide_ix = c->ix.sa64 != nullptr;
        const int rows_in_lds = lds <= 48 * 1024 && !wide_ix;
        // packed rows: the lane's row in its LDS slot (4.6 KB per wave at 150 bases: no occupancy lost); rows too long for 16 KB: from global memory
        const size_t plds = (size_t)64 * (pr.pwords + 1) * 8;
        if (packed && plds <= 16 * 1024 && kg)
            hipLaunchKernelGGL((k_seed_extra<false, true, true, true>), dim3(chunks_min), dim3(64), plds, c->stream, c->ix, d_seq, pr, gm, stride, tot_at(c, TOT_SEED_EXTRA),
                               target_waves, c->prm.seed_len, pe_mode, st, sc, cnt);
        else if (packed && plds <= 16 * 1024)
            hipLaunchKernelGGL((k_seed_extra<false, true, true>), dim3(chunks_min), dim3(64), plds, c->stream, c->ix, d_seq, pr, gm, stride, tot_at(c, TOT_SEED_EXTRA),
                               target_waves, c->prm.seed_len, pe_mode, st, sc, cnt);
        else if (packed)
            hipLaunchKernelGGL((k_seed_extra<false, true>), dim3(chunks_min), dim3(64), 0, c->stream, c->ix, d_seq, pr, gm, stride, tot_at(c, TOT_SEED_EXTRA),
                               target_waves, c->prm.seed_len, pe_mode, st, sc, cnt);
        else if (rows_in_lds)
            hipLaunchKernelGGL((k_seed_extra<true, false>), dim3(chunks_min), dim3(64), lds, c->stream, c->ix, d_seq, pr, gm, stride, tot_at(c, TOT_SEED_EXTRA),
                               target_waves, c->prm.seed_len, pe_mode, st, sc, cnt);
        else
            hipLaunchKernelGGL((k_seed_extra<false, false>), dim3(chunks_min), dim3(64), 0, c->stream, c->ix, d_seq, pr, gm, stride, tot_at(c, TOT_SEED_EXTRA),
                               target_waves, c->prm.seed_len, pe_mode, st, sc, cnt);
    }
    prof_end(c);
    return BMBS_OK;
}

// the candidate total behind scan_cand: waited for (exact), or bounded by a capacity with a guard behind the scan (k_guard_cand)
int cand_total(Lane* c, const ReadState& st, u64 n, bool exact, u64* tot_out)
{
    if (exact) {
        u64 tot = 0;
        HIPCHK(c, hipMemcpyAsync(&tot, tot_at(c, TOT_CAND), sizeof tot, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        *tot_out = tot;
        return BMBS_OK;
    }
    const u64 cap = cap_from(c->lr_cand, n, n, c->kn.cap_scale);
    hipLaunchKernelGGL(k_guard_cand, dim3(nblk(n, 256)), dim3(256), 0, c->stream, tot_at(c, TOT_CAND), cap, c->flags.as<u32>(), (long)n, st.verdict,
                       st.n_cand, st.cand_off);
    hipLaunchKernelGGL(k_guard_done, dim3(1), dim3(1), 0, c->stream, tot_at(c, TOT_CAND), c->flags.as<u32>(), BMBS_FLAG_CAND);
    *tot_out = cap;
    return BMBS_OK;
}

// stages K1-K6 + votes; leaves the vote segments in c->votes / c->slot_read
int run_seed_stages(Lane* c, const char* d_seq, const ReadGeom& gm, int stride, u64 n, u64* total_cand, int pe_mode, bool exact, bool prepacked)
{
    ReadState st = read_state(c);
    int rc = launch_seeding(c, d_seq, gm, stride, n, pe_mode, prepacked);
    if (rc) return rc;
    prof_begin(c, "scan_cand");
    rc = scan_u32(c, st.n_cand, n, st.cand_off, TOT_CAND);
    if (rc) return rc;
    prof_end(c);
    u64 tot = 0;
    rc = cand_total(c, st, n, exact, &tot);
    if (rc) return rc;
    *total_cand = tot;
    const u64 t1 = exact ? std::max<u64>(tot, cap_from((double)tot / (double)n, n, n)) : tot;     // buffers as the next call (which does not wait) will want them
    ENS(c, c->cand, t1 * 8); ENS(c, c->votes, t1 * sizeof(bmbs_vote)); ENS(c, c->slot_read, t1 * 4);
    ENS(c, c->ferr, t1 * 4); ENS(c, c->fend, t1 * 4);
    // locate + sort + votes in one kernel per list-size class (the two-kernel form of round 1, k_locate + k_vote, was removed in round 4)
    ENS(c, c->long_flag, n * 4); ENS(c, c->long_off, (n + 1) * 8); ENS(c, c->long_list, n * 4); ENS(c, c->vote_list, n * 4);
    prof_begin(c, "k_vote_fused");
    // the reads that have candidates, compacted (the scan's list mode on n_cand != 0), so that the vote kernel's waves are dense
    HIPCHK(c, hipMemsetAsync(c->long_flag.p, 0, n * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(st.n_votes, 0, n * 4, c->stream));
    rc = scan_u32(c, st.n_cand, n, c->long_off.as<u64>(), TOT_VOTE_READS, c->vote_list.as<u32>(), 1);
    if (rc) return rc;
    // long reads (up to 25 seeds): lists of 17..32 candidates are the rule, not the repeat case -- they get a kernel of their
    // own (k_vote_mid); its flag and list live in the seeding work-list buffers, free by now
    // ... and on a repeat-rich genome also for short reads (seeds with many hits): taken when the last call left more than 0.5 % of
    // its reads to the long-list kernels (a wave per read)
    const bool use_mid = gm.L / 10 - 1 > VOTE_REG || c->lr_long > 0.005;
    u32* mid_flag = use_mid ? c->sd_flag_c.as<u32>() : nullptr;
    if (use_mid) HIPCHK(c, hipMemsetAsync(mid_flag, 0, n * 4, c->stream));
    hipLaunchKernelGGL(k_vote_fused, dim3(nblk(n, 64)), dim3(64), 0, c->stream, c->ix, (long)n, gm, st, c->cand.as<u64>(),
                       c->votes.as<bmbs_vote>(), c->slot_read.as<u32>(), c->long_flag.as<u32>(), tot_at(c, TOT_VOTE_READS),
                       c->vote_list.as<u32>(), mid_flag);
    prof_end(c);
    if (use_mid) {
        prof_begin(c, "k_vote_mid");
        rc = scan_u32(c, mid_flag, n, c->long_off.as<u64>(), TOT_MID, c->sd_list_c.as<u32>());
        if (rc) return rc;
        hipLaunchKernelGGL(k_vote_mid, dim3(nblk(n, 64)), dim3(64), 0, c->stream, c->ix, gm, st, tot_at(c, TOT_MID), c->sd_list_c.as<u32>(),
                           c->cand.as<u64>(), c->votes.as<bmbs_vote>(), c->slot_read.as<u32>(), c->counters.as<unsigned long long>());
        prof_end(c);
    }
    // reads with more than 16 candidates (repeats): one block per read
    prof_begin(c, "k_vote_long");
    rc = scan_u32(c, c->long_flag.as<u32>(), n, c->long_off.as<u64>(), TOT_LONG, c->long_list.as<u32>());
    if (rc) return rc;
    // the wave form (lists of up to 256 candidates) walks the list and hands the longer ones to a list of their own (TOT_BIG)
    ENS(c, c->big_list, n * 4 + 64);
    unsigned long long* big_count = c->totals.as<unsigned long long>() + TOT_BIG;
    HIPCHK(c, hipMemsetAsync(big_count, 0, 8, c->stream));
    hipLaunchKernelGGL((k_vote_long<VM_CAP, VM_BLOCK, VOTE_REG>), dim3(32768), dim3(VM_BLOCK), 0, c->stream, c->ix, gm, st, tot_at(c, TOT_LONG),
                       c->long_list.as<u32>(), c->cand.as<u64>(), c->votes.as<bmbs_vote>(), c->slot_read.as<u32>(), c->big_list.as<u32>(), big_count, c->counters.as<unsigned long long>());
    prof_end(c);
    prof_begin(c, "k_vote_big");
    // the handed-over lists in two size classes (as k_vote_pe_long): the <= 1024-key form needs 14 KB of LDS instead of 57 KB, so five
    // times as many reads are in flight -- the vote order (std::sort's permutation, one partition pass after the other) is a
    // chain of barriers, not work
    hipLaunchKernelGGL((k_vote_long<1024, 128, VM_CAP>), dim3(8192), dim3(128), 0, c->stream, c->ix, gm, st, tot_at(c, TOT_BIG),
                       c->big_list.as<u32>(), c->cand.as<u64>(), c->votes.as<bmbs_vote>(), c->slot_read.as<u32>(), (u32*)nullptr, (unsigned long long*)nullptr, c->counters.as<unsigned long long>());
    hipLaunchKernelGGL((k_vote_long<2048, 256, 1024>), dim3(4096), dim3(256), 0, c->stream, c->ix, gm, st, tot_at(c, TOT_BIG),
                       c->big_list.as<u32>(), c->cand.as<u64>(), c->votes.as<bmbs_vote>(), c->slot_read.as<u32>(), (u32*)nullptr, (unsigned long long*)nullptr, c->counters.as<unsigned long long>());
    hipLaunchKernelGGL((k_vote_long<VL_CAP, VL_BLOCK, 2048>), dim3(2048), dim3(VL_BLOCK), 0, c->stream, c->ix, gm, st, tot_at(c, TOT_BIG),
                       c->big_list.as<u32>(), c->cand.as<u64>(), c->votes.as<bmbs_vote>(), c->slot_read.as<u32>(), (u32*)nullptr, (unsigned long long*)nullptr, c->counters.as<unsigned long long>());
    prof_end(c);
    return BMBS_OK;
}

// host rows (stride bytes apart) -> device rows padded to a multiple of 16 bytes
int upload_rows(Lane* c, DevBuf& dst, const char* src, int L, int stride, u64 n, int* dstride, hipStream_t st = nullptr)
{
    if (!st) st = c->stream;
    const int ds = (L + 15) / 16 * 16;
    *dstride = ds;
    ENS(c, dst, n * (u64)ds + 64);
    // rows that are already `ds` bytes apart go over as ONE block (the bytes past L are ignored by every kernel); a 2-D copy of
    // 150-byte rows out of a 160-byte pitch ran at half the link rate
    if (n && stride == ds) { HIPCHK(c, hipMemcpyAsync(dst.p, src, n * (u64)ds, hipMemcpyHostToDevice, st)); return BMBS_OK; }
    HIPCHK(c, hipMemsetAsync(dst.p, 0, n * (u64)ds + 64, st));
    if (n) HIPCHK(c, hipMemcpy2DAsync(dst.p, ds, src, stride, L, n, hipMemcpyHostToDevice, st));
    return BMBS_OK;
}

// ================================================================================================
extern "C" void bmbs_default_params(bmbs_params* p)
{
    p->e_f = 0.08; p->mp_max = 6; p->mp_min = 2; p->np = 1; p->gap_open = 5; p->gap_ext = 3; p->q_base = 33;
    p->seed_len = 30; p->min_ins = 0; p->max_ins = 500; p->sensitive = 0; p->ambiguous_out = 0;
}

void lane_destroy(Lane* c);

Lane* lane_create(int device_id, const bmbs_params& prm, const Knobs& kn, bool first)
{
    Lane* c = new Lane();
    c->dev = device_id;
    c->prm = prm; c->kn = kn;
    c->sp.mp_max = c->prm.mp_max; c->sp.mp_min = c->prm.mp_min; c->sp.np = c->prm.np;
    c->sp.gap_open = c->prm.gap_open; c->sp.gap_ext = c->prm.gap_ext; c->sp.q_base = c->prm.q_base;
    c->sp.seed_len = c->prm.seed_len;
    if (hipStreamCreate(&c->stream) != hipSuccess) { delete c; return nullptr; }
    // (the copy streams are created by lane_copy_streams once every lane of the context has its kernel stream: see there)
    (void)hipEventCreateWithFlags(&c->ev_up, hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&c->ev_k, hipEventDisableTiming);
    int lut[256];
    for (int q = 0; q < 256; q++) lut[q] = mismatch_penalty(c->prm, q);
    {
        uint8_t class_of[256], rep[16]; int32_t penalty_of[16], nc = 0;
        qual_class_table(c->prm, class_of, penalty_of, &nc, rep);
        for (int k = 0; k < 8; k++) { c->qrep_lo |= (u64)rep[k] << (8 * k); c->qrep_hi |= (u64)rep[8 + k] << (8 * k); }
    }
    const size_t shard_bytes = BMBS_SHARDS * BMBS_SHARD_WORDS * 8;
    if (ensure(c, c->pen_lut, sizeof(lut)) || ensure(c, c->stats, shard_bytes) || ensure(c, c->call_stats, shard_bytes) || ensure(c, c->counters, shard_bytes) ||
        ensure(c, c->totals, TOT_WORDS * sizeof(u64)) || ensure(c, c->flags, BMBS_FLAG_WORDS * sizeof(u32)) || ensure(c, c->tx_info, TXI_WORDS * sizeof(u32)) ||
        hipHostMalloc((void**)&c->h_info, sizeof(HostInfo), hipHostMallocPortable) != hipSuccess ||
        hipHostMalloc((void**)&c->h_tot, BMBS_SLOTS * sizeof(CallWords), hipHostMallocPortable) != hipSuccess) { lane_destroy(c); return nullptr; }
    memset(c->h_tot, 0, BMBS_SLOTS * sizeof(CallWords));
    (void)hipMemcpy(c->pen_lut.p, lut, sizeof(lut), hipMemcpyHostToDevice);
    (void)hipMemset(c->stats.p, 0, shard_bytes);
    (void)hipMemset(c->call_stats.p, 0, shard_bytes);
    (void)hipMemset(c->counters.p, 0, shard_bytes);
    textpath_device_init(c);
    (void)hipMemset(c->totals.p, 0, TOT_WORDS * sizeof(u64));
    (void)hipMemset(c->flags.p, 0, BMBS_FLAG_WORDS * sizeof(u32));
    // diagnostic: per-wave timeline of the kernels that call wavelog_begin/_end (one context at a time; tools/wavelog.py)
    if (first)
    if (const char* wl = getenv("BMBS_WAVELOG")) {
        const unsigned cap = 1u << 21;
        if (*wl && !ensure(c, c->wavelog_buf, (u64)cap * 32) && !ensure(c, c->wavelog_count, 64)) {
            (void)hipMemset(c->wavelog_count.p, 0, 64);
            WaveLogDev d = {c->wavelog_buf.as<unsigned long long>(), c->wavelog_count.as<unsigned int>(), cap};
            if (hipMemcpyToSymbol(HIP_SYMBOL(g_wavelog), &d, sizeof(d)) == hipSuccess) c->wavelog_path = wl;
        }
    }
    return c;
}

// The runtime multiplexes a process's streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 unless the environment says otherwise),
// each new stream taking the queue with the fewest users, and two streams on one queue run one behind the other.  With a lane's three
// streams created together, the kernel streams of a context's two lanes ended up on ONE queue in some processes and not in others --
// the lanes did not overlap there (round 5 took it for slow hosts; round 6: the same binary 1108 or 1248 M reads/s from one process
// to the next, 1255 every time with GPU_MAX_HW_QUEUES=8; profiles/HISTORY.md).  So: all kernel streams first, then the upload streams,
// then the download streams (a lane's download follows its kernels anyway: sharing a queue with them costs nothing), and bmbs_env_init
// asks for eight queues unless the process has set the variable itself.
void lane_copy_streams(std::vector<Lane*>& lanes)
{
    for (Lane* c : lanes) (void)hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking);
    for (Lane* c : lanes) (void)hipStreamCreateWithFlags(&c->down_stream, hipStreamNonBlocking);
}
// runs when the library is loaded: before the HIP runtime reads its environment, if nothing in the process has touched the GPU yet
__attribute__((constructor)) static void bmbs_env_init() { setenv("GPU_MAX_HW_QUEUES", "8", 0); }

void lane_destroy(Lane* c)
{
    if (!c) return;
    (void)hipSetDevice(c->dev);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (!c->wavelog_path.empty()) {
        (void)hipDeviceSynchronize();
        unsigned cnt = 0;
        (void)hipMemcpy(&cnt, c->wavelog_count.p, 4, hipMemcpyDeviceToHost);
        if (cnt > (1u << 21)) cnt = 1u << 21;
        std::vector<unsigned long long> h((size_t)cnt * 4);
        if (cnt) (void)hipMemcpy(h.data(), c->wavelog_buf.p, (size_t)cnt * 32, hipMemcpyDeviceToHost);
        if (FILE* f = fopen(c->wavelog_path.c_str(), "wb")) { fwrite(h.data(), 32, cnt, f); fclose(f); }
        WaveLogDev d = {nullptr, nullptr, 0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wavelog), &d, sizeof(d));
        release(c->wavelog_buf); release(c->wavelog_count);
    }
    DevBuf* all[] = {&c->occ, &c->hash, &c->sa, &c->gen2, &c->gen2p, &c->chrom_start, &c->t20, &c->pen_lut, &c->mapq_lut, &c->verdict,
                     &c->n_seeds, &c->multi, &c->mm_site, &c->exit_site, &c->seeds, &c->n_cand, &c->cand_off,
                     &c->n_votes, &c->best_site, &c->best_end, &c->best_err, &c->sbd, &c->red_status, &c->job_flag,
                     &c->job_off, &c->scan_tmp, &c->scan_ticket, &c->totals, &c->cand, &c->votes, &c->slot_read, &c->vote_off, &c->votes_dense, &c->dense_read, &c->ferr, &c->fend,
                     &c->job_read, &c->job_site, &c->job_end, &c->job_err, &c->need_sw, &c->sw_off, &c->sw_job, &c->trace, &c->a_start, &c->a_end, &c->a_nm, &c->a_score, &c->a_nops,
                     &c->in_seq, &c->in_qual, &c->out_res, &c->cig_pool, &c->in_a, &c->in_b, &c->in_c, &c->in_d,
                     &c->stats, &c->call_stats, &c->flags, &c->counters, &c->pe_seq, &c->pe_B, &c->pe_occ, &c->pe_len, &c->pe_cur,
                     &c->sd_sp0, &c->sd_hits0, &c->sd_ml0, &c->sd_tm, &c->sd_seed_id, &c->sd_clen, &c->sd_first_ml, &c->sd_flag_c, &c->sd_flag_d,
                     &c->sd_off_c, &c->sd_off_d, &c->sd_list_c, &c->sd_list_d, &c->pe_vround, &c->pe_dead, &c->pe_both, &c->pe_npair, &c->pe_sbd, &c->in_seq2, &c->in_qual2,
                     &c->pe_first, &c->pe_full, &c->pe_R, &c->pe_roff, &c->pe_rflag, &c->pe_rscan, &c->pe_rlist, &c->pe_rcnt, &c->pe_ritem_off, &c->pe_rcand, &c->long_flag, &c->long_off, &c->long_list, &c->vote_list,
                     &c->mapq_off, &c->klut, &c->in_len, &c->fq_text1, &c->fq_text2, &c->fq_idx, &c->pk_in1, &c->pk_in2, &c->pq_in1, &c->pq_in2, &c->pk_ascii, &c->prow, &c->prow_dirty, &c->pe_mid_flag, &c->pe_mid_list};
    for (DevBuf* b : all) release(*b);
    for (auto& set : c->profset) for (auto& p : set) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    c->arena.free_all();
    if (c->h_tot) (void)hipHostFree(c->h_tot);
    if (c->h_info) (void)hipHostFree(c->h_info);
    { DevBuf* tx[] = {&c->tx_tilecnt, &c->tx_tileoff, &c->tx_nl[0], &c->tx_nl[1], &c->tx_rec[0], &c->tx_rec[1], &c->tx_info, &c->sam_len, &c->sam_off, &c->sam_out, &c->chrom_chars, &c->chrom_off, &c->big_list,
                     &c->bam_raw, &c->bam_slots, &c->bam_slot_len, &c->bam_off, &c->stats_snap, &c->z_comp, &c->z_off, &c->z_text, &c->z_err, &c->z_nl, &c->z_comp2, &c->z_off2, &c->z_err2,
                     &c->bs_key, &c->bs_key2, &c->bs_idx, &c->bs_idx2, &c->bs_slen, &c->bs_soff, &c->bs_tmp, &c->sc.in.in, &c->sc.in.len, &c->sc.in.off, &c->bs_sorted, &c->bai_a, &c->bai_b, &c->bai_out,
                     &c->dp_in.in, &c->dp_in.len, &c->dp_in.off, &c->dp_sig, &c->dp_key, &c->dp_key2, &c->dp_idx, &c->dp_idx2, &c->dp_dup, &c->dp_tmpl,
                     &c->mt_in.in, &c->mt_in.len, &c->mt_in.off, &c->mt_clip, &c->mt_cnt, &c->mt_eoff, &c->mt_ev, &c->mt_work, &c->mt_acc, &c->mt_site, &c->mt_cl2, &c->mt_mbias,
                     &c->cy_site, &c->cy_run, &c->cy_cnt, &c->cy_off, &c->cy_out, &c->nc_in.in, &c->nc_in.len, &c->nc_in.off, &c->nc_work,
                     &c->tr_rec[0], &c->tr_rec[1], &c->tr_keep, &c->tr_flag, &c->tr_off, &c->tr_words};
      for (DevBuf* b : tx) release(*b); }
    if (c->ev_up) (void)hipEventDestroy(c->ev_up);
    if (c->ev_k) (void)hipEventDestroy(c->ev_k);
    if (c->ev_qx_a) (void)hipEventDestroy(c->ev_qx_a);
    if (c->ev_qx_b) (void)hipEventDestroy(c->ev_qx_b);
    if (c->up_stream) (void)hipStreamDestroy(c->up_stream);
    if (c->down_stream) (void)hipStreamDestroy(c->down_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" bmbs_ctx* bmbs_create(int device_id, const bmbs_params* params)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev) return nullptr;
    if (hipSetDevice(device_id) != hipSuccess) return nullptr;
    bmbs_ctx* X = new bmbs_ctx();
    X->dev = device_id;
    if (params) X->prm = *params; else bmbs_default_params(&X->prm);
    X->kn.read();                                  // the A/B environment is read here, once; the launch path never calls getenv
    for (int i = 0; i < X->kn.host_lanes; i++) {          // (the first kn.lanes of them take the chunks of the *_device calls)
        Lane* c = lane_create(device_id, X->prm, X->kn, i == 0);
        if (!c) { bmbs_destroy(X); return nullptr; }
        X->lanes.push_back(c);
    }
    lane_copy_streams(X->lanes);
    return X;
}

extern "C" void bmbs_destroy(bmbs_ctx* X)
{
#ifdef VOTE_PROF
    {
        unsigned long long h[4][8];
        if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_vote_prof), sizeof h) == hipSuccess)
            for (int q = 0; q < 4; q++)
                fprintf(stderr, "[vote_prof] class %d: lists %llu candidates %llu sites %llu | Mcycles: locate+sort %.1f run-ends %.1f vote-order %.1f write %.1f | one-lane fallbacks %llu\n",
                        q, h[q][0], h[q][1], h[q][2], h[q][3] / 1e6, h[q][4] / 1e6, h[q][5] / 1e6, h[q][6] / 1e6, h[q][7]);
    }
#endif
    if (!X) return;
    (void)hipSetDevice(X->dev);
    for (size_t i = X->lanes.size(); i-- > 0;) lane_destroy(X->lanes[i]);      // lane 0 (the index owner) last
    delete X;
}

extern "C" int32_t bmbs_max_cigar_ops(const bmbs_params* params, int32_t L)
{
    if (L <= 0 || L > BMBS_MAX_READ) return -1;
    bmbs_params P;
    if (params) P = *params; else bmbs_default_params(&P);
    return cigar_ops_bound(P, L, threshold_k(P, L));
}

extern "C" int64_t bmbs_outcome_index(uint64_t bases, uint32_t not_acgt, int32_t len, int32_t bits, int32_t* depth)
{
    if (bits != 32 && bits != 33) return -2;
    static const std::vector<u16> tab = [] { std::vector<u16> t(256); for (int v = 0; v < 256; v++) t[v] = th_tab_entry(v); return t; }();
    int D = 0;
    u64 idx = 0;
    const bool ok = th_slot(bases, not_acgt, len, bits, tab.data(), idx, D);
    if (depth) *depth = D;
    return ok ? (int64_t)idx : -1;
}

extern "C" const char* bmbs_last_error(const bmbs_ctx* X) { return X ? X->err.c_str() : "no context (no HIP device?)"; }

static int lane_index_attach(Lane* c, const bmbs_index_view* v)
{
    if (!c || !v) return BMBS_EINVAL;
    HIPCHK(c, hipSetDevice(c->dev));
    const u64 G = v->ref_len, n = 2 * G, rows = n + 1;
    if (v->sa_length != rows) { c->err = "index view: sa_length != 2*ref_len + 1"; return BMBS_EINVAL; }
    if (rows >= (1ull << 36)) { c->err = "genome too large: rows must fit the 36-bit fields of the 16-mer table"; return BMBS_EINVAL; }
    if (v->n_chrom < 1) { c->err = "index view: n_chrom must be at least 1"; return BMBS_EINVAL; }
    // texts of 2^32 symbols and more (GRCh38) take the wide forms: 64-bit suffix array, Occ counts relative to super-blocks of 2^31
    // symbols whose sums travel in the DevIndex; BMBS_WIDE=1 forces them on a small index and BMBS_SUPER_SHIFT=s (>= 16) makes the
    // super-blocks small enough for such an index to have several (tests)
    const char* wide_env = getenv("BMBS_WIDE");
    const bool wide = rows >= (1ull << 32) || (wide_env && !strcmp(wide_env, "1"));
    SuperSums sup; sup.shift = 0;
    for (int q = 0; q < 4; q++) { sup.T[q] = 0; sup.A[q] = 0; }
    if (wide) {
        const char* ss = getenv("BMBS_SUPER_SHIFT");
        sup.shift = ss ? atoi(ss) : 31;
        if (sup.shift < 16 || sup.shift > 31 || (n >> sup.shift) >= 4) { c->err = "index attach: the text needs more than four Occ super-blocks"; return BMBS_EINVAL; }
        for (u64 S = 0; S < 4 && (S << sup.shift) <= n; S++) {
            const u64 e = ((S << sup.shift) >> 16) * 2;
            if (e + 1 >= v->high_occ_words) break;
            sup.T[S] = v->high_occ[e]; sup.A[S] = v->high_occ[e + 1];
        }
    }
    // upload the reference layouts verbatim, re-pack on the device, drop the originals
    DevBuf t_bwt, t_ho, t_hh, t_hl, t_sa, t_fl, t_pac;
    // the staging copies are released on every path out of this function (also the HIPCHK early returns)
    struct Staging {
        DevBuf* b[7];
        ~Staging() { for (DevBuf* x : b) release(*x); }
    } staging = {{&t_bwt, &t_ho, &t_hh, &t_hl, &t_sa, &t_fl, &t_pac}};
    (void)staging;
    auto up = [&](DevBuf& b, const void* src, size_t bytes) -> int {
        int rc = ensure(c, b, bytes + 64);
        if (rc) return rc;
        if (hipMemsetAsync(b.p, 0, b.cap, c->stream) != hipSuccess) return BMBS_ENODEV;
        if (hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) return BMBS_ENODEV;
        return BMBS_OK;
    };
    int rc = 0;
    rc |= up(t_bwt, v->bwt, v->bwt_words * 8);
    rc |= up(t_ho, v->high_occ, v->high_occ_words * 8);
    rc |= up(t_hh, v->hash_hi, v->hash_entries * 4);
    rc |= up(t_hl, v->hash_lo, v->hash_entries);
    rc |= up(t_sa, v->sa, v->sa_entries * 4);
    rc |= up(t_fl, v->sa_flag, v->sa_flag_words * 8);
    rc |= up(t_pac, v->pac, v->pac_bytes);
    if (rc) { c->err = "index upload failed"; return BMBS_ENOMEM; }
    RefIndexDev R;
    R.bwt = t_bwt.as<u64>(); R.high_occ = t_ho.as<u64>(); R.hash_hi = t_hh.as<u32>(); R.hash_lo = t_hl.as<u8>();
    R.sa = t_sa.as<u32>(); R.sa_flag = t_fl.as<u64>(); R.pac = t_pac.as<u8>();
    const u64 n_blk = n / 32 + 2;
    const u64 gen_words = ((n + 63) / 64 + 3) * 2;          // whole 16-byte pieces plus spare ones for the look-ahead loads
    std::vector<u64> cs(v->n_chrom + 1, 0);
    for (int i = 0; i < v->n_chrom; i++) cs[i + 1] = cs[i] + v->chrom_len[i];
    if (ensure(c, c->occ, n_blk * 16) || ensure(c, c->hash, v->hash_entries * 8) || ensure(c, c->sa, rows * (wide ? 8 : 4)) ||
        ensure(c, c->gen2, gen_words * 8) || ensure(c, c->gen2p, gen_words * 8) || ensure(c, c->chrom_start, cs.size() * 8)) return BMBS_ENOMEM;
    HIPCHK(c, hipMemcpyAsync(c->chrom_start.p, cs.data(), cs.size() * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_repack_occ, dim3(nblk(n_blk, 256)), dim3(256), 0, c->stream, R, n, n_blk, sup, c->occ.as<uint4>());
    hipLaunchKernelGGL(k_repack_hash, dim3(nblk(v->hash_entries, 256)), dim3(256), 0, c->stream, R, v->hash_entries, c->hash.as<u64>());
    hipLaunchKernelGGL(k_build_gen2, dim3(nblk(gen_words, 256)), dim3(256), 0, c->stream, R, G, gen_words, c->gen2.as<u64>());
    hipLaunchKernelGGL(k_build_gen2p, dim3(nblk(gen_words, 256)), dim3(256), 0, c->stream, c->gen2.as<u64>(), gen_words, c->gen2p.as<u64>());
    DevIndex ix;
    ix.occ = c->occ.as<uint4>(); ix.hash = c->hash.as<u64>(); ix.gen2 = c->gen2.as<u64>(); ix.gen2p = c->gen2p.as<u64>();
    ix.sa = wide ? nullptr : c->sa.as<u32>(); ix.sa64 = wide ? c->sa.as<u64>() : nullptr;
    ix.sup_shift = sup.shift;
    for (int q = 0; q < 4; q++) { ix.supT[q] = sup.T[q]; ix.supA[q] = sup.A[q]; }
    ix.chrom_start = c->chrom_start.as<u64>(); ix.G = G; ix.total = n; ix.shapline = v->shapline;
    ix.C[0] = v->nacgt[0]; ix.C[1] = v->nacgt[1]; ix.C[2] = v->nacgt[2]; ix.n_chrom = v->n_chrom;
    hipLaunchKernelGGL(k_expand_sa, dim3(nblk(std::min<u64>(rows, 1ull << 30), 256)), dim3(256), 0, c->stream, ix, R, rows, wide ? nullptr : c->sa.as<u32>(),
                       wide ? c->sa.as<u64>() : nullptr);
    // outcome table.  Texts of 2^32 symbols and more: the balanced table of 2^33 entries (68.7 GB) when the device has the room, else the
    // ternary one at E = 5 (3^21 entries, 83.7 GB), else E = 4 (3^20 entries, 27.9 GB), else none; smaller texts: E = 4.  BMBS_T20=0 turns it off, BMBS_TDEPTH=20|21 forces a ternary depth and BMBS_TDEPTH=h32|h33 the balanced
    // table of that many bits on any text (A/B runs, tests)
    ix.t20 = nullptr; ix.t_e = 4; ix.t_b = 0;
    {
        const char* t20_env = getenv("BMBS_T20");
        const char* td_env = getenv("BMBS_TDEPTH");
        const u64 n_keys = v->hash_entries - 1;                 // 3^16
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        int want_e = wide ? 5 : 4, want_b = wide ? 33 : 0;
        if (td_env) {
            want_b = !strcmp(td_env, "h33") ? 33 : !strcmp(td_env, "h32") ? 32 : 0;
            want_e = atoi(td_env) == 21 || want_b ? 5 : 4;
        }
        const u64 room = 48ull << 30;
        if (!(t20_env && !strcmp(t20_env, "0")) && n_keys == 43046721ull) {
            if (want_b && free_b > (8ull << want_b) + room && ensure(c, c->t20, 8ull << want_b) == BMBS_OK) {
                ix.t_b = want_b; ix.t_e = TH_MAX_E;             // (t_e: the most letters a lookup reads ahead)
                const u64 n_chunks = (1ull << want_b) / TH_CHUNK;
                hipLaunchKernelGGL(k_build_th, dim3(nblk(std::min<u64>(n_chunks, 1ull << 24), 256)), dim3(256), 0, c->stream, ix, want_b, n_chunks, c->t20.as<u64>());
                ix.t20 = c->t20.as<u64>();
            }
            for (int e5 = want_e; e5 >= 4 && !ix.t20; e5--) {
                const u64 need = n_keys * t20_width(e5) * 8;
                if (free_b > need + room && ensure(c, c->t20, need) == BMBS_OK) {
                    ix.t_e = e5;
                    hipLaunchKernelGGL(k_build_t20, dim3(nblk(n_keys, 256)), dim3(256), 0, c->stream, ix, n_keys, c->t20.as<u64>());
                    ix.t20 = c->t20.as<u64>();
                }
            }
        }
    }
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { c->err = std::string("index re-pack: ") + hipGetErrorString(e); return BMBS_ENODEV; }
    // the trigram rank table is built when it is wanted (occ3_want): BMBS_KGRAM=2 at the first call, 1 (default) once long chains were seen
    ix.occ3 = nullptr; ix.c3 = nullptr; ix.nb3 = 0;
    c->o3 = std::make_shared<Occ3Shared>();
    c->o3->dev = c->dev; c->o3->base = ix; c->o3->rows = rows;
    c->ix = ix; c->rows = rows; c->attached = true;
    return BMBS_OK;
}

// ------------------------------------------------------------------------------------------------
// A mapping call on a lane: call_begin, the launch sequence, call_end.  call_end adds the call's five counters to the lane's
// (unless a guard flag says the call is going to be repeated) and copies the stage counts and the flags into page-locked
// words; lane_settle waits for the lane and reads them.
int call_begin(Lane* c, int slot)
{
    c->cur_slot = slot; c->prof_used[slot] = 0;
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, BMBS_SHARDS * BMBS_SHARD_WORDS * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(c->flags.p, 0, BMBS_FLAG_WORDS * sizeof(u32), c->stream));
    HIPCHK(c, hipMemsetAsync(c->totals.p, 0, TOT_CALL_WORDS * sizeof(u64), c->stream));
    return BMBS_OK;
}
int call_end(Lane* c, int slot)
{
    CallWords* h = c->h_tot + slot;
    const int words = BMBS_SHARDS * BMBS_SHARD_WORDS;
    hipLaunchKernelGGL(k_stats_commit, dim3(nblk(words, 256)), dim3(256), 0, c->stream, c->flags.as<u32>(), c->call_stats.as<unsigned long long>(),
                       c->stats.as<unsigned long long>(), words);
    hipLaunchKernelGGL(k_call_chain_counts, dim3(1), dim3(64), 0, c->stream, c->counters.as<unsigned long long>(), c->totals.as<u64>());      // (the array: TOT_CHAIN_*)
    HIPCHK(c, hipMemcpyAsync(h->tot, c->totals.p, sizeof h->tot, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h->flags, c->flags.p, sizeof h->flags, hipMemcpyDeviceToHost, c->stream));
    return BMBS_OK;
}

// the caller's packed rows (bmbs_map_*_packed) -> the lane's: prow / prow_dirty, and `ascii` (rows `stride` apart) gets the text of the
// pieces that hold an 'N'.  rc: the rows are reverse-complemented on the way (mate 2).  row0: where these rows sit in the batch
// (call_open has checked that hw words hold a row of this length)
void rows_from_packed(Lane* c, const u64* src, int hw, const ReadGeom& gm, u64 row0, u64 n, bool rc, char* ascii, int stride)
{
    const int pwords = pack_words(gm.L), W = pack_base_words(gm.L);
    const unsigned g = nblk(n * (u64)W, 256);
    hipLaunchKernelGGL((rc ? k_rows_from_packed<true> : k_rows_from_packed<false>), dim3(g), dim3(256), 0, c->stream, src, hw, gm, (long)row0, (long)n, c->prow.as<u64>(),
                       pwords, W, c->prow_dirty.as<u32>(), ascii, stride);
}

// host lengths -> device (u16 per read)
int upload_lens(Lane* c, const uint16_t* len, u64 n, u64 at, u64 total, int L, hipStream_t st = nullptr)
{
    if (!st) st = c->stream;
    for (u64 i = 0; i < n; i++) if (len[i] == 0 || len[i] > L) { c->err = "read length 0 or longer than L_max"; return BMBS_EINVAL; }
    ENS(c, c->in_len, total * 2 + 16);           // sized for the whole batch up front: growing would drop the first part
    HIPCHK(c, hipMemcpyAsync(c->in_len.as<u16>() + at, len, n * 2, hipMemcpyHostToDevice, st));
    return BMBS_OK;
}

// ---- the launch sequence of a mapping call ----------------------------------------------------------------------------------------
// A call is its Pending (bmbs_host.h): the launch sequence reads it and never changes it -- a call whose counts did not fit its
// capacities is issued again from the same Pending with exact = true (lane_settle).
//   a[0], a[1]: rows and qualities (mate 1); a[2], a[3]: mate 2 as in the FASTQ file.  packed_hw > 0: a[0] / a[2] hold the caller's
//   packed rows (packed_hw words apart) instead of ASCII rows.  d_len: NULL, or u16 per row (pairs: the n first mates, then the n second)

// What every call begins with: the argument checks, the tables, the geometry and the CIGAR bound, the per-row workspace of its
// `reads` rows (n, pairs: 2n) and call_begin.  A call of no reads gets BMBS_OK with nothing set up: the caller returns on P.n == 0.
int call_open(Lane* c, const Pending& P, u64 reads, ReadGeom* gm, int* max_ops)
{
    if (!c) return BMBS_EINVAL;
    if (!c->attached) { c->err = "no index attached"; return BMBS_ESTATE; }
    if (P.L <= 0 || P.L > BMBS_MAX_READ || P.stride < P.L || P.n < 0) { c->err = "bad read geometry"; return BMBS_EINVAL; }
    const uint64_t ptrs = P.a[0] | P.a[1] | (P.pe ? P.a[2] | P.a[3] : 0);
    if ((P.stride & 15) || (ptrs & 15)) { c->err = "device read buffers must be 16-byte aligned with a stride that is a multiple of 16"; return BMBS_EINVAL; }
    HIPCHK(c, hipSetDevice(c->dev));
    // prepared: c->pe_seq already holds the 2n rows (mate 1, then reverse-complemented mate 2) -- the FASTQ-text entry point writes
    // them there straight from the text
    if (P.pe && P.prepared && c->pe_seq.cap < reads * (u64)P.stride + 64) { c->err = "internal: prepared rows missing"; return BMBS_ESTATE; }
    if (P.n == 0) return BMBS_OK;
    int rc = prepare_luts(c);
    if (rc) return rc;
    *gm = geom(c, P.L, P.d_len);
    *max_ops = cigar_ops_bound(c->prm, P.L, gm->k);
    c->last_max_ops = *max_ops;
    if (*max_ops > BMBS_MAX_RECORD_OPS) { c->err = "these gap / mismatch penalties allow alignments with more CIGAR operations than a record holds (254)"; return BMBS_EINVAL; }
    rc = per_read_workspace(c, reads);
    if (rc) return rc;
    if (P.pe) {
        const u64 n = (u64)P.n;
        ENS(c, c->pe_seq, reads * (u64)P.stride + 64);
        ENS(c, c->pe_occ, reads * 4); ENS(c, c->pe_len, reads * 4); ENS(c, c->pe_cur, reads); ENS(c, c->pe_vround, reads);
        ENS(c, c->pe_dead, n); ENS(c, c->pe_both, n); ENS(c, c->pe_npair, n * 4); ENS(c, c->pe_sbd, n * 4);
    }
    if (P.packed_hw && !use_packed_rows(c)) { c->err = "packed reads need the packed-row kernels (BMBS_LEGACY is set)"; return BMBS_EINVAL; }
    if (P.packed_hw && P.packed_hw < pack_base_words(gm->L) + (gm->L + 63) / 64) { c->err = "packed rows: pwords is smaller than a row of this length takes"; return BMBS_EINVAL; }
    return call_begin(c, P.slot);
}

// What every call ends with, over its `reads` rows: the alignment jobs the reduce / pairing stage flagged -- scan, list, K11-K13.
// jobs: the count (exact), or one slot per read with the device-side count bounding every kernel and a guard on the caller's pool.
// Rows from rev_from on (mate 2; 0xffffffff: none) carry FASTQ-order qualities in qual2 for a reverse-complemented read
// (need_reverse_quality = 1)
int align_jobs(Lane* c, const Pending& P, const ReadGeom& gm, const ReadState& st, const char* seq, const char* qual1, const char* qual2, u64 reads,
               u32 rev_from, int max_ops)
{
    prof_begin(c, "scan_jobs");
    int rc = scan_u32(c, st.job_flag, reads, st.job_off, TOT_JOBS);
    if (rc) return rc;
    prof_end(c);
    u64 n_jobs = reads, sw_bound = ~0ull;
    const u64* n_jobs_dev = nullptr;
    if (P.exact) {
        HIPCHK(c, hipMemcpyAsync(&n_jobs, tot_at(c, TOT_JOBS), sizeof n_jobs, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if ((u64)P.cigar_cap < n_jobs * (u64)max_ops) { c->err = "cigar pool too small (it takes bmbs_max_cigar_ops() slots per read)"; return BMBS_ENOMEM; }
    } else {
        n_jobs_dev = tot_at(c, TOT_JOBS);
        sw_bound = cap_from(c->lr_sw, reads, c->kn.cap_scale < 1.0 ? 64 : 16384, c->kn.cap_scale);
        if ((u64)P.cigar_cap < reads * (u64)max_ops) {
            hipLaunchKernelGGL(k_guard_jobs, dim3(nblk(reads, 256)), dim3(256), 0, c->stream, n_jobs_dev, (u64)max_ops, (u64)P.cigar_cap, c->flags.as<u32>(), (long)reads, st.job_flag);
            hipLaunchKernelGGL(k_guard_done, dim3(1), dim3(1), 0, c->stream, tot_at(c, TOT_JOBS), c->flags.as<u32>(), BMBS_FLAG_CIGAR);
        }
    }
    c->last_n_jobs = n_jobs;
    const u64 nj = n_jobs ? n_jobs : 1;
    ENS(c, c->job_read, nj * 4); ENS(c, c->job_site, nj * 8); ENS(c, c->job_end, nj * 4); ENS(c, c->job_err, nj * 4);
    if (n_jobs) {
        prof_begin(c, "k_job_list");
        hipLaunchKernelGGL(k_job_list, dim3(nblk(reads, 256)), dim3(256), 0, c->stream, (long)reads, st, c->job_read.as<u32>(),
                           c->job_site.as<u64>(), c->job_end.as<int>(), c->job_err.as<u32>());
        prof_end(c);
    }
    const Jobs jobs = {c->job_read.as<u32>(), c->job_site.as<u64>(), c->job_end.as<int>(), c->job_err.as<u32>()};
    return run_align(c, seq, qual1, qual2, gm, P.stride, n_jobs, jobs, rev_from, reinterpret_cast<u32*>(P.d_cigar_pool), max_ops, packed_rows(c, gm),
                     n_jobs_dev, sw_bound);
}

// ---- single end -------------------------------------------------------------------------------------------------------------------
// the votes compacted to a dense list, Myers on every candidate (k_filter), the best site(s) of every read (k_reduce).
// tot: candidate slots -- the count itself (exact) or the capacity the buffers and grids are sized for
int se_filter_reduce(Lane* c, const ReadGeom& gm, const ReadState& st, const char* d_seq, int stride, u64 n, u64 tot, bool exact)
{
    ENS(c, c->vote_off, (n + 1) * 8);
    {
        const u64 t1 = exact ? std::max<u64>(tot, cap_from((double)tot / (double)n, n, n)) : (tot ? tot : 1);
        ENS(c, c->votes_dense, t1 * sizeof(bmbs_vote)); ENS(c, c->dense_read, t1 * 4);
    }
    prof_begin(c, "vote_compact");
    int rc = scan_u32(c, st.n_votes, n, c->vote_off.as<u64>(), TOT_VOTES);
    if (rc) return rc;
    if (tot)
        hipLaunchKernelGGL(k_vote_compact, dim3(nblk(tot, 256)), dim3(256), 0, c->stream, tot, exact ? (const u64*)nullptr : tot_at(c, TOT_CAND), st,
                           c->vote_off.as<u64>(), c->slot_read.as<u32>(), c->votes.as<bmbs_vote>(), c->votes_dense.as<bmbs_vote>(), c->dense_read.as<u32>());
    prof_end(c);
    if (tot) {
        prof_begin(c, "k_filter");
        hipLaunchKernelGGL(k_filter, dim3(nblk(tot, 256)), dim3(256), 0, c->stream, c->ix, d_seq, packed_rows(c, gm), gm, stride, tot_at(c, TOT_VOTES),
                           c->dense_read.as<u32>(), c->votes_dense.as<bmbs_vote>(), c->ferr.as<u32>(), c->fend.as<int>(), c->counters.as<unsigned long long>());
        prof_end(c);
    }
    prof_begin(c, "k_reduce");
    // over the compacted list of reads with candidates the vote stage built
    HIPCHK(c, hipMemsetAsync(st.job_flag, 0, n * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(st.red_status, 0, n, c->stream));
    hipLaunchKernelGGL(k_reduce, dim3(nblk(n, 256)), dim3(256), 0, c->stream, (long)n, c->prm.ambiguous_out, st, c->vote_off.as<u64>(),
                       c->votes_dense.as<bmbs_vote>(), c->ferr.as<u32>(), c->fend.as<int>(), tot_at(c, TOT_VOTE_READS), c->vote_list.as<u32>());
    prof_end(c);
    return BMBS_OK;
}

int map_se_dev(Lane* c, const Pending& P)
{
    ReadGeom gm = {};
    int max_ops = 0;
    int rc = call_open(c, P, (u64)P.n, &gm, &max_ops);
    if (rc || P.n == 0) return rc;
    const u64 n = (u64)P.n;
    const char* d_seq = reinterpret_cast<const char*>(P.a[0]);
    const char* d_qual = reinterpret_cast<const char*>(P.a[1]);
    if (P.packed_hw) {
        // the ASCII rows exist only where a piece holds an 'N' (written by k_rows_from_packed into the lane's own buffer)
        ENS(c, c->pk_ascii, n * (u64)P.stride + 64);
        { int rz_ = ensure(c, c->prow, n * (u64)pack_words(gm.L) * 8 + 64, true); if (rz_) return rz_; } ENS(c, c->prow_dirty, n + 64);
        HIPCHK(c, hipMemsetAsync(c->prow_dirty.p, 0, n + 64, c->stream));
        prof_begin(c, "k_rows_from_packed");
        rows_from_packed(c, reinterpret_cast<const u64*>(P.a[0]), P.packed_hw, gm, 0, n, false, c->pk_ascii.as<char>(), P.stride);
        prof_end(c);
        d_seq = c->pk_ascii.as<char>();
    }
    const ReadState st = read_state(c);
    u64 tot = 0;
    rc = run_seed_stages(c, d_seq, gm, P.stride, n, &tot, 0, P.exact, P.packed_hw > 0);
    if (rc) return rc;
    c->last_total_cand = tot;
    rc = se_filter_reduce(c, gm, st, d_seq, P.stride, n, tot, P.exact);
    if (rc) return rc;
    rc = align_jobs(c, P, gm, st, d_seq, d_qual, nullptr, n, 0xffffffffu, max_ops);
    if (rc) return rc;
    prof_begin(c, "k_finalize");
    hipLaunchKernelGGL(k_finalize, dim3(nblk(n, 256)), dim3(256), 0, c->stream, c->ix, c->sp, c->pen_lut.as<int>(),
                       c->mapq_lut.as<u8>(), c->mapq_off.as<u32>(), c->mapq_unit, d_seq, d_qual, gm, P.stride, (long)n, st, c->a_start.as<int>(),
                       c->a_end.as<int>(), c->a_nm.as<u32>(), c->a_score.as<int>(), c->a_nops.as<int>(), max_ops, P.cigar_base,
                       c->prm.ambiguous_out, c->sd_sp0.as<u64>(), c->sd_hits0.as<u32>(),
                       reinterpret_cast<bmbs_result_dev*>(P.d_results), c->call_stats.as<unsigned long long>());
    prof_end(c);
    return call_end(c, P.slot);
}

// ---- paired end (fast mode: Map_Pair_Seq_end_to_end_fast, Schema.cpp:18570; --sensitive: Map_Pair_Seq_end_to_end) -----------------
// what the stages of a paired-end call share: n pairs = n2 rows in seq_all (mate 1, then reverse-complemented mate 2), the candidate
// lists in A / B (ps.cur says which), tot = candidate slots -- the count itself (exact) or the capacity buffers and grids are sized for
struct PeCall {
    Lane* c; ReadGeom gm; PeIns pi; ReadState st; PeState ps; PeCand *A, *B; char* seq_all; u64 n, n2; int stride; bool exact; u64 tot;
    bool prepacked;              // the lane's packed rows are filled by the row stage (the seeding stage does not pack them itself)
    int rows(const Pending& P);
    int seed();
    int votes();
    int verify_round(int round, u64 cap, const char* name_f, const char* name_c);
    int verify_round_pairs(int round, u64 cap, const u32* cnt, const char* name_f, const char* name_c);
    int verify_fast();
    int verify_sensitive();
};

// the 2n rows in seq_all and their packed copy: from the caller's packed rows, or by k_pe_prepare[_p], or there already (prepared).
int PeCall::rows(const Pending& P)
{
    prepacked = false;
    if (P.packed_hw) {
        // the caller's packed rows: mate 1 as it is, mate 2 reverse-complemented (bmbs_map_pe_packed); no ASCII rows to read at all
        { int rz_ = ensure(c, c->prow, n2 * (u64)pack_words(gm.L) * 8 + 64, true); if (rz_) return rz_; } ENS(c, c->prow_dirty, n2 + 64);
        HIPCHK(c, hipMemsetAsync(c->prow_dirty.p, 0, n2 + 64, c->stream));
        prof_begin(c, "k_rows_from_packed");
        rows_from_packed(c, reinterpret_cast<const u64*>(P.a[0]), P.packed_hw, gm, 0, n, false, seq_all, stride);
        rows_from_packed(c, reinterpret_cast<const u64*>(P.a[2]), P.packed_hw, gm, n, n, true, seq_all, stride);
        prof_end(c);
        prepacked = true;
    } else if (!P.prepared) {
        u64* prow = nullptr; u32* pdirty = nullptr;
        const int pwords = pack_words(gm.L), W = pack_base_words(gm.L);
        if (use_packed_rows(c)) {
            { int rz_ = ensure(c, c->prow, n2 * (u64)pwords * 8 + 64, true); if (rz_) return rz_; } ENS(c, c->prow_dirty, n2 + 64);
            HIPCHK(c, hipMemsetAsync(c->prow_dirty.p, 0, n2 + 64, c->stream));
            prow = c->prow.as<u64>(); pdirty = c->prow_dirty.as<u32>(); prepacked = true;
        }
        // on packed rows nothing reads the ASCII rows except under a set bit of the mask plane, so only those pieces are written
        // (BMBS_LEGACY=1: no packed rows, the complete ASCII copy)
        const int sparse = prow != nullptr;
        const char* seq1 = reinterpret_cast<const char*>(P.a[0]);
        const char* seq2 = reinterpret_cast<const char*>(P.a[2]);
        prof_begin(c, "k_pe_prepare");
        const int ppr = stride / 16;
        if (sparse && ppr <= 256) {
            const int rpb = 256 / ppr;
            hipLaunchKernelGGL(k_pe_prepare_p, dim3(std::min<u64>(nblk(n, rpb), 2048)), dim3(256), (size_t)rpb * (ppr + 1) * 16, c->stream,
                               seq1, seq2, gm, stride, (long)n, seq_all, prow, pwords, W, pdirty);
        } else
        hipLaunchKernelGGL(k_pe_prepare, dim3(nblk(n * (stride / 16), 256)), dim3(256), 0, c->stream, seq1, seq2, gm, stride, (long)n, seq_all,
                           prow, pwords, W, pdirty, sparse);
        prof_end(c);
    }
    return BMBS_OK;
}

// the per-row and per-pair state (call_open has sized it; --sensitive: and its buffers), seeding of all 2n reads; candidate slots by
// scan -> tot, and the per-candidate buffers (A, B)
int PeCall::seed()
{
    ps.occ = c->pe_occ.as<int>(); ps.len = c->pe_len.as<u32>(); ps.cur = c->pe_cur.as<u8>(); ps.vround = c->pe_vround.as<u8>();
    ps.dead = c->pe_dead.as<u8>(); ps.both = c->pe_both.as<u8>(); ps.npair = c->pe_npair.as<int>(); ps.sbd = c->pe_sbd.as<u32>();
    if (c->prm.sensitive) {
        ENS(c, c->pe_first, n); ENS(c, c->pe_full, n2); ENS(c, c->pe_roff, n2 * 8); ENS(c, c->pe_rflag, n * 4); ENS(c, c->pe_rscan, (n + 1) * 8);
        ENS(c, c->pe_rlist, n * 4); ENS(c, c->pe_rcnt, n * 4); ENS(c, c->pe_ritem_off, (n + 1) * 8);
    }
    ps.first = c->pe_first.as<u8>(); ps.full = c->pe_full.as<u8>(); ps.R = c->pe_R.as<PeCand>(); ps.roff = c->pe_roff.as<u64>();
    c->last_reseeded = 0; c->last_reseed_cand = 0;
    int rc = launch_seeding(c, seq_all, gm, stride, n2, 1, prepacked);
    if (rc) return rc;
    prof_begin(c, "scan_cand");
    rc = scan_u32(c, st.n_cand, n2, st.cand_off, TOT_CAND);
    if (rc) return rc;
    prof_end(c);
    rc = cand_total(c, st, n2, exact, &tot);
    if (rc) return rc;
    c->last_total_cand = tot;
    const u64 t1 = exact ? std::max<u64>(tot, cap_from((double)tot / (double)n2, n2, n2)) : (tot ? tot : 1);
    ENS(c, c->cand, t1 * 8); ENS(c, c->votes, t1 * sizeof(PeCand)); ENS(c, c->pe_B, t1 * sizeof(PeCand)); ENS(c, c->slot_read, t1 * 4);
    ENS(c, c->dense_read, t1 * 4); ENS(c, c->ferr, t1 * 4);
    A = c->votes.as<PeCand>();
    B = c->pe_B.as<PeCand>();
    return BMBS_OK;
}

// locate + sort + votes of every read's candidates, one kernel per list-size class
int PeCall::votes()
{
    unsigned long long* cnt = c->counters.as<unsigned long long>();
    ENS(c, c->long_flag, n2 * 4); ENS(c, c->long_off, (n2 + 1) * 8); ENS(c, c->long_list, n2 * 4);
    // reads of 180 bases and more place up to 25 seeds: lists of 17..32 candidates are the rule there and get a kernel of their own
    // (k_vote_pe_mid; buffers of its own: --sensitive still reads the seeding flags afterwards)
    // (on a repeat-rich genome also for short reads: when the last call left more than 0.5 % of its reads to the long-list kernels)
    const bool use_mid = gm.L / 10 - 1 > VOTE_REG || c->lr_long > 0.005;
    if (use_mid) { ENS(c, c->pe_mid_flag, n2 * 4); ENS(c, c->pe_mid_list, n2 * 4); }
    u32* mid_flag = use_mid ? c->pe_mid_flag.as<u32>() : nullptr;
    if (use_mid) HIPCHK(c, hipMemsetAsync(mid_flag, 0, n2 * 4, c->stream));
    prof_begin(c, "k_vote_pe_fused");
    // the reads that have lists are compacted onto dense lanes inside each block of 256 (BMBS_VOTE_DENSE=0: one lane per read)
    if (c->kn.vote_dense)
        hipLaunchKernelGGL(k_vote_pe_dense, dim3(nblk(n2, VOTE_DENSE_BLOCK)), dim3(VOTE_DENSE_BLOCK), 0, c->stream, c->ix, (long)n2, gm, st, ps, A, c->long_flag.as<u32>(), mid_flag);
    else
        hipLaunchKernelGGL(k_vote_pe_fused, dim3(nblk(n2, 64)), dim3(64), 0, c->stream, c->ix, (long)n2, gm, st, ps, A, c->long_flag.as<u32>(), mid_flag);
    prof_end(c);
    if (use_mid) {
        prof_begin(c, "k_vote_pe_mid");
        int rc = scan_u32(c, mid_flag, n2, c->long_off.as<u64>(), TOT_MID, c->pe_mid_list.as<u32>());
        if (rc) return rc;
        hipLaunchKernelGGL(k_vote_pe_mid, dim3(nblk(n2, 64)), dim3(64), 0, c->stream, c->ix, gm, st, ps, tot_at(c, TOT_MID), c->pe_mid_list.as<u32>(), A, cnt);
        prof_end(c);
    }
    prof_begin(c, "k_vote_pe_long");
    // fast mode: located sites without a partner on the mate's finished list are dropped before the sort (k_pe_fast.hip; --sensitive
    // uses the lists differently, Schema.cpp:19953-21459).  BMBS_PREFILTER=0: off (A/B runs, tests)
    const int prefilter = (!c->prm.sensitive && c->kn.prefilter) ? 1 : 0;
    int rc = scan_u32(c, c->long_flag.as<u32>(), n2, c->long_off.as<u64>(), TOT_LONG, c->long_list.as<u32>());
    if (rc) return rc;
    ENS(c, c->big_list, n2 * 4 + 64);
    unsigned long long* big_count = c->totals.as<unsigned long long>() + TOT_BIG;
    HIPCHK(c, hipMemsetAsync(big_count, 0, 8, c->stream));
    hipLaunchKernelGGL((k_vote_pe_long<VM_CAP, VM_BLOCK, VOTE_REG>), dim3(32768), dim3(VM_BLOCK), 0, c->stream, c->ix, gm, st, ps,
                       tot_at(c, TOT_LONG), c->long_list.as<u32>(), A, c->big_list.as<u32>(), big_count, c->cand.as<u64>(), cnt, (long)n, pi, prefilter, c->long_flag.as<u32>());
    prof_end(c);
    prof_begin(c, "k_vote_pe_big");
    // the handed-over lists in two size classes: up to 1024 candidates (10 KB of LDS per block: twice the blocks per CU of the
    // 4096-key form; on the GRCh38-like genome 88 % of the handed-over lists), and the rest
    hipLaunchKernelGGL((k_vote_pe_long<1024, 128, VM_CAP>), dim3(8192), dim3(128), 0, c->stream, c->ix, gm, st, ps,
                       tot_at(c, TOT_BIG), c->big_list.as<u32>(), A, (u32*)nullptr, (unsigned long long*)nullptr, c->cand.as<u64>(), cnt, (long)n, pi, prefilter, c->long_flag.as<u32>());
    hipLaunchKernelGGL((k_vote_pe_long<2048, 256, 1024>), dim3(4096), dim3(256), 0, c->stream, c->ix, gm, st, ps,
                       tot_at(c, TOT_BIG), c->big_list.as<u32>(), A, (u32*)nullptr, (unsigned long long*)nullptr, c->cand.as<u64>(), cnt, (long)n, pi, prefilter, c->long_flag.as<u32>());
    hipLaunchKernelGGL((k_vote_pe_long<VL_CAP, VL_BLOCK, 2048>), dim3(2048), dim3(VL_BLOCK), 0, c->stream, c->ix, gm, st, ps,
                       tot_at(c, TOT_BIG), c->big_list.as<u32>(), A, (u32*)nullptr, (unsigned long long*)nullptr, c->cand.as<u64>(), cnt, (long)n, pi, prefilter, c->long_flag.as<u32>());
    prof_end(c);
    return BMBS_OK;
}

// one verification round: dense (read, list index) work list of the mates scheduled in `round`, Myers, compaction.
// cap: the candidates the Myers grid covers (0: none to verify); name_f / name_c: the profile names of the two halves (literals)
int PeCall::verify_round(int round, u64 cap, const char* name_f, const char* name_c)
{
    if (cap) {
        prof_begin(c, name_f);
        u32* wcnt = c->sd_flag_c.as<u32>();
        u64* woff = c->sd_off_c.as<u64>();
        hipLaunchKernelGGL(k_pe_count, dim3(nblk(n2, 256)), dim3(256), 0, c->stream, (long)n, (long)n2, round, ps, wcnt);
        int rc = scan_u32(c, wcnt, n2, woff, TOT_PE_WORK);
        if (rc) return rc;
        hipLaunchKernelGGL(k_pe_worklist, dim3(nblk(n2, 256)), dim3(256), 0, c->stream, (long)n2, wcnt, woff, c->dense_read.as<u32>(),
                           c->ferr.as<u32>());
        hipLaunchKernelGGL(k_filter_pe, dim3(nblk(cap, 256)), dim3(256), 0, c->stream, c->ix, seq_all, packed_rows(c, gm), gm, stride, st, ps, A, B,
                           tot_at(c, TOT_PE_WORK), c->dense_read.as<u32>(), c->ferr.as<u32>(), c->counters.as<unsigned long long>());
        prof_end(c);
    }
    prof_begin(c, name_c);
    hipLaunchKernelGGL(k_pe_compact, dim3(nblk(n2, 64)), dim3(64), 0, c->stream, (long)n, (long)n2, gm, round, st, ps, A, B);
    prof_end(c);
    return BMBS_OK;
}

// The same round in fast mode (BMBS_PE_ROUNDS=1), where a round verifies at most one mate of a pair: cnt holds per PAIR the entries of
// the mate scheduled in `round`, left there by the kernel before the round (k_pe_filter_pairs[_long], k_pe_prune); a scan over the n
// pairs whose second launch writes the work list itself (k_scan_expand -- always the two-launch form), Myers, compaction with one lane
// per pair.  The same candidates as verify_round's list, in the order of the pairs
int PeCall::verify_round_pairs(int round, u64 cap, const u32* cnt, const char* name_f, const char* name_c)
{
    if (cap) {
        prof_begin(c, name_f);
        const u64 per = (u64)SCAN_BLOCK * SCAN_ITEMS;
        const u64 nb = n ? (n + per - 1) / per : 1;
        // (under BMBS_SCAN_CHAIN=1 scan_tmp holds the chained scans' status words: tile sums never carry a live epoch, fresh memory might)
        { int rc = ensure(c, c->scan_tmp, (nb + 1) * 8, c->kn.scan_chain != 0); if (rc) return rc; }
        u64* bs = c->scan_tmp.as<u64>();
        hipLaunchKernelGGL(k_scan_partial, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, c->stream, cnt, n, bs, 0, (const u64*)nullptr);
        hipLaunchKernelGGL(k_scan_expand, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, c->stream, cnt, n, bs, ps.vround, round,
                           c->dense_read.as<u32>(), c->ferr.as<u32>(), tot_at(c, TOT_PE_WORK));
        hipLaunchKernelGGL(k_filter_pe, dim3(nblk(cap, 256)), dim3(256), 0, c->stream, c->ix, seq_all, packed_rows(c, gm), gm, stride, st, ps, A, B,
                           tot_at(c, TOT_PE_WORK), c->dense_read.as<u32>(), c->ferr.as<u32>(), c->counters.as<unsigned long long>());
        prof_end(c);
    }
    prof_begin(c, name_c);
    hipLaunchKernelGGL(k_pe_compact_pair, dim3(nblk(n, 64)), dim3(64), 0, c->stream, (long)n, gm, round, st, ps, A, B);
    prof_end(c);
    return BMBS_OK;
}

// fast mode: the lists cut down to sites with a partner on the mate's list, verified in two rounds
int PeCall::verify_fast()
{
    // BMBS_PE_ROUNDS=1: the rounds' per-pair counts, written by the kernels before them into a buffer the seeding stage is done with
    // (n2 words; round 1 has read its counts when k_pe_prune writes round 2's).  0: the rounds count for themselves (verify_round)
    u32* rcnt = c->kn.pe_rounds ? c->sd_flag_c.as<u32>() : nullptr;
    prof_begin(c, "k_pe_filter_pairs");
    // pairs with long candidate lists (repeats) are left to a second kernel, one wave per pair -- on repeat-rich input only (the last
    // call left more than 0.5 % of its reads to the long-list vote kernels): flag array, scan and the extra launch cost 0.3 ms per
    // 10 M pairs, 4 % of a launch on a repeat-poor genome.  BMBS_PEF_LONG=0: never, =2: always
    u32* pef_flag = (c->kn.pef_long == 2 || (c->kn.pef_long == 1 && c->lr_long > 0.005)) ? c->long_flag.as<u32>() : nullptr;
    if (pef_flag) HIPCHK(c, hipMemsetAsync(pef_flag, 0, n * 4, c->stream));
    hipLaunchKernelGGL(k_pe_filter_pairs, dim3(nblk(n, 64)), dim3(64), 0, c->stream, (long)n, gm, pi, st, ps, A, B, pef_flag,
                       c->counters.as<unsigned long long>(), rcnt);
    if (pef_flag) {
        int rc = scan_u32(c, pef_flag, n, c->long_off.as<u64>(), TOT_PEF_LONG, c->long_list.as<u32>());
        if (rc) return rc;
        hipLaunchKernelGGL(k_pe_filter_pairs_long, dim3((unsigned)std::min<u64>(n, 65536)), dim3(64), 0, c->stream, (long)n, gm, pi, st, ps, tot_at(c, TOT_PEF_LONG),
                           c->long_list.as<u32>(), A, B, rcnt);
    }
    prof_end(c);
    int rc = rcnt ? verify_round_pairs(1, tot, rcnt, "k_filter_pe_r1", "k_pe_compact_r1") : verify_round(1, tot, "k_filter_pe_r1", "k_pe_compact_r1");
    if (rc) return rc;
    prof_begin(c, "k_pe_prune");
    hipLaunchKernelGGL(k_pe_prune, dim3(nblk(n, 64)), dim3(64), 0, c->stream, (long)n, gm, pi, st, ps, A, B, rcnt);
    prof_end(c);
    return rcnt ? verify_round_pairs(2, tot, rcnt, "k_filter_pe_r2", "k_pe_compact_r2") : verify_round(2, tot, "k_filter_pe_r2", "k_pe_compact_r2");
}

// --sensitive (Map_Pair_Seq_end_to_end): first mate verified in full, second mate filtered by it, rescue by re-seeding (a third round)
int PeCall::verify_sensitive()
{
    unsigned long long* cnt = c->counters.as<unsigned long long>();
    prof_begin(c, "k_pes_order");
    hipLaunchKernelGGL(k_pes_order, dim3(nblk(n, 256)), dim3(256), 0, c->stream, (long)n, st, seed_carry(c), ps);
    prof_end(c);
    int rc = verify_round(1, tot, "k_filter_pe_r1", "k_pe_compact_r1");
    if (rc) return rc;
    prof_begin(c, "k_pes_second");
    hipLaunchKernelGGL(k_pes_second, dim3(nblk(n, 64)), dim3(64), 0, c->stream, (long)n, gm, pi, st, ps, A, B);
    prof_end(c);
    rc = verify_round(2, tot, "k_filter_pe_r2", "k_pe_compact_r2");
    if (rc) return rc;
    prof_begin(c, "k_pes_reseed");
    u32* rflag = c->pe_rflag.as<u32>();
    u32* rlist = c->pe_rlist.as<u32>();
    u32* rcnt = c->pe_rcnt.as<u32>();
    u64* n_reseed = tot_at(c, TOT_RESEED);
    hipLaunchKernelGGL(k_pes_reseed_flag, dim3(nblk(n, 256)), dim3(256), 0, c->stream, (long)n, ps, rflag);
    rc = scan_u32(c, rflag, n, c->pe_rscan.as<u64>(), TOT_RESEED, rlist);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(rcnt, 0, n * 4, c->stream));
    {
        const PackedRows prs = packed_rows(c, gm);
        const bool kg = c->ix.occ3 && prs.base && (c->kn.kgram >= 2 || (c->kn.kgram == 1 && c->lr_chain >= 3.0));
        hipLaunchKernelGGL((kg ? k_pes_reseed<true, true> : prs.base ? k_pes_reseed<true> : k_pes_reseed<false>), dim3(nblk(n, 64)), dim3(64), 0, c->stream, c->ix, seq_all, prs, gm, stride,
                           (long)n, n_reseed, rlist, st, ps, rcnt, cnt);
    }
    rc = scan_u32(c, rcnt, n, c->pe_ritem_off.as<u64>(), TOT_RCAND);
    if (rc) return rc;
    prof_end(c);
    u64 rt[2] = {0, 0};          // pairs to re-seed, their candidates (TOT_RESEED, TOT_RCAND): counts (exact) or capacities with a guard
    if (exact) {
        HIPCHK(c, hipMemcpyAsync(rt, tot_at(c, TOT_RESEED), sizeof rt, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else {
        rt[0] = n; rt[1] = cap_from(c->lr_rcand, n2, c->kn.cap_scale < 1.0 ? 64 : 65536, c->kn.cap_scale);
        hipLaunchKernelGGL(k_guard_rcand, dim3(nblk(n, 256)), dim3(256), 0, c->stream, tot_at(c, TOT_RCAND), rt[1], c->flags.as<u32>(), (long)n, rcnt,
                           c->pe_ritem_off.as<u64>());
        hipLaunchKernelGGL(k_guard_done, dim3(1), dim3(1), 0, c->stream, tot_at(c, TOT_RCAND), c->flags.as<u32>(), BMBS_FLAG_RCAND);
    }
    c->last_reseeded = rt[0]; c->last_reseed_cand = rt[1];
    if (!rt[0]) return BMBS_OK;
    const u64 rtot = exact ? std::max<u64>(rt[1], cap_from((double)rt[1] / (double)n2, n2, 65536)) : (rt[1] ? rt[1] : 1);
    ENS(c, c->pe_R, rtot * sizeof(PeCand)); ENS(c, c->pe_rcand, rtot * 8);
    ENS(c, c->dense_read, rtot * 4); ENS(c, c->ferr, rtot * 4);
    ps.R = c->pe_R.as<PeCand>();
    prof_begin(c, "k_pes_vote");
    // mates with more than PESV_LONG candidates are flagged, listed (TOT_PESV_LONG) and sorted by a block each
    u32* pv_flag = c->long_flag.as<u32>();                                  // n2 words: free again after the vote stage
    hipLaunchKernelGGL(k_pes_vote, dim3(nblk(rt[0], 64)), dim3(64), 0, c->stream, c->ix, (long)n, gm, pi, n_reseed, rlist,
                       c->pe_ritem_off.as<u64>(), st, ps, c->pe_rcand.as<u64>(), A, B, pv_flag, cnt);
    rc = scan_u32(c, pv_flag, rt[0], c->long_off.as<u64>(), TOT_PESV_LONG, c->long_list.as<u32>(), 0, n_reseed);
    if (rc) return rc;
    hipLaunchKernelGGL((k_pes_vote_long<1024, 128, PESV_LONG>), dim3(8192), dim3(128), 0, c->stream, c->ix, (long)n, gm, pi, tot_at(c, TOT_PESV_LONG),
                       c->long_list.as<u32>(), rlist, c->pe_ritem_off.as<u64>(), st, ps, c->pe_rcand.as<u64>(), A, B);
    // (three size classes, as the vote kernels: a re-seeded mate of 1 025 .. 2 048 candidates in the 4 096-key form held 41 KB of
    // LDS -- three lists per CU; r6)
    hipLaunchKernelGGL((k_pes_vote_long<2048, 256, 1024>), dim3(4096), dim3(256), 0, c->stream, c->ix, (long)n, gm, pi, tot_at(c, TOT_PESV_LONG),
                       c->long_list.as<u32>(), rlist, c->pe_ritem_off.as<u64>(), st, ps, c->pe_rcand.as<u64>(), A, B);
    hipLaunchKernelGGL((k_pes_vote_long<VL_CAP, VL_BLOCK, 2048>), dim3(2048), dim3(VL_BLOCK), 0, c->stream, c->ix, (long)n, gm, pi, tot_at(c, TOT_PESV_LONG),
                       c->long_list.as<u32>(), rlist, c->pe_ritem_off.as<u64>(), st, ps, c->pe_rcand.as<u64>(), A, B);
    prof_end(c);
    return verify_round(3, rt[1], "k_filter_pe_r3", "k_pe_compact_r3");
}

int map_pe_dev(Lane* c, const Pending& P)
{
    ReadGeom gm = {};
    int max_ops = 0;
    int rc = call_open(c, P, 2 * (u64)P.n, &gm, &max_ops);
    if (rc || P.n == 0) return rc;
    PeCall x = {};
    x.c = c; x.gm = gm; x.pi = {c->prm.min_ins, c->prm.max_ins}; x.st = read_state(c);
    x.seq_all = c->pe_seq.as<char>(); x.n = (u64)P.n; x.n2 = 2 * x.n; x.stride = P.stride; x.exact = P.exact;
    // the qualities are read where the caller put them (qual_row): mate 1 rows in a[1], mate 2 rows in a[3]
    const char* qual_1 = reinterpret_cast<const char*>(P.a[1]);
    const char* qual_2 = reinterpret_cast<const char*>(P.a[3]);
    rc = x.rows(P);
    if (!rc) rc = x.seed();
    if (!rc) rc = x.votes();
    if (!rc) rc = c->prm.sensitive ? x.verify_sensitive() : x.verify_fast();
    if (rc) return rc;
    prof_begin(c, "k_pe_pair");
    hipLaunchKernelGGL(k_pe_pair, dim3(nblk(x.n, 64)), dim3(64), 0, c->stream, c->ix, (long)x.n, gm, x.pi, c->prm.ambiguous_out, x.st, x.ps, x.A, x.B);
    prof_end(c);
    rc = align_jobs(c, P, gm, x.st, x.seq_all, qual_1, qual_2, x.n2, (u32)x.n, max_ops);
    if (rc) return rc;
    prof_begin(c, "k_finalize_pe");
    hipLaunchKernelGGL(k_finalize_pe, dim3(nblk(x.n, 256)), dim3(256), 0, c->stream, c->ix, c->sp, c->pen_lut.as<int>(), x.seq_all, qual_1, qual_2, P.stride,
                       c->mapq_lut.as<u8>(), c->mapq_off.as<u32>(), c->mapq_unit, gm,
                       c->prm.min_ins, c->prm.max_ins, c->prm.ambiguous_out, (long)x.n, x.st, x.ps, c->a_start.as<int>(), c->a_end.as<int>(), c->a_nm.as<u32>(),
                       c->a_score.as<int>(), c->a_nops.as<int>(), max_ops, P.cigar_base, reinterpret_cast<bmbs_result_dev*>(P.d_results),
                       c->call_stats.as<unsigned long long>());
    prof_end(c);
    return call_end(c, P.slot);
}

// ---- calls in flight on a lane ------------------------------------------------------------------------------------------------
int lane_issue(Lane* c, const Pending& P) { return P.pe ? map_pe_dev(c, P) : map_se_dev(c, P); }

// Wait for the lane, then read what its calls left in their page-locked words: the stage counts (they size the next calls) and the
// guard flags.  A call whose counts did not fit its capacities has done no harm (the guards took its work away and its counters
// were not committed): it is issued again with exact sizes.  The caller's buffers of a *_device call have to stay untouched until
// bmbs_sync() for exactly this reason.
int lane_settle(Lane* c)
{
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int rc_all = BMBS_OK;
    while (!c->inflight.empty()) {
        Pending P = c->inflight.front();
        c->inflight.pop_front();
        for (int attempt = 0; attempt < 2; attempt++) {
            const u64* t = c->h_tot[P.slot].tot;
            const u32* f = c->h_tot[P.slot].flags;
            if (f[BMBS_FLAG_CIGAR]) { c->err = "cigar pool too small (it takes bmbs_max_cigar_ops() slots per read)"; rc_all = BMBS_ENOMEM; break; }
            if (!(f[BMBS_FLAG_CAND] | f[BMBS_FLAG_SW] | f[BMBS_FLAG_RCAND])) {
                const double nr = (double)(P.pe ? 2 * P.n : P.n);
                if (nr > 0) {
                    c->lr_cand = std::max(c->lr_cand, std::max(1e-9, (double)t[TOT_CAND] / nr));
                    c->lr_sw = std::max(c->lr_sw, (double)t[TOT_SW] / nr);
                    c->lr_rcand = std::max(c->lr_rcand, (double)t[TOT_RCAND] / nr);
                    c->lr_long = ((double)t[TOT_LONG] + (double)t[TOT_MID]) / nr;             // reads whose candidate lists went to the mid / long kernels
                    if (t[TOT_CHAIN_LOOKUPS]) { c->lr_chain = (double)t[TOT_CHAIN_EXT] / (double)t[TOT_CHAIN_LOOKUPS]; occ3_want(c, true); }      // (the table is built here, behind the call that showed the chains)
                }
                c->last_total_cand = t[TOT_CAND]; c->last_n_jobs = t[TOT_JOBS];
                prof_collect(c, P.slot);
                break;
            }
            if (attempt == 1) { c->err = "internal error: a call issued with exact sizes raised a capacity flag"; rc_all = BMBS_ESTATE; break; }
            c->n_retries++;
            P.exact = true;
            const int rc = lane_issue(c, P);
            if (rc) { rc_all = rc; break; }
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
    }
    return rc_all;
}

// P.staged: the call reads lane-owned staging buffers (host entry points, re-laid length arrays), which the next call overwrites
int lane_enqueue(Lane* c, Pending P, bool staged)
{
    if (!c->inflight.empty() && (c->lr_cand == 0 || (int)c->inflight.size() >= BMBS_SLOTS || c->inflight.back().staged || c->inflight.back().prepared || staged)) {
        const int rc = lane_settle(c);
        if (rc) return rc;
    }
    P.exact = c->kn.exact || c->lr_cand == 0;          // nothing learned yet: wait for the counts this once
    P.slot = c->next_slot;
    c->next_slot = (c->next_slot + 1) % BMBS_SLOTS;
    const int rc = lane_issue(c, P);
    if (rc) return rc;
    P.staged = staged;
    c->inflight.push_back(P);
    return BMBS_OK;
}

// what earlier calls needed per read is shared by the lanes of a context
void share_needs(bmbs_ctx* X)
{
    double a = 0, b = 0, d = 0, g = 0, ch = 0;
    for (Lane* c : X->lanes) { a = std::max(a, c->lr_cand); b = std::max(b, c->lr_sw); d = std::max(d, c->lr_rcand); g = std::max(g, c->lr_long); ch = std::max(ch, c->lr_chain); }
    for (Lane* c : X->lanes) { c->lr_cand = a; c->lr_sw = b; c->lr_rcand = d; c->lr_long = g; c->lr_chain = ch; }
}

int settle_all(bmbs_ctx* X)
{
    int rc_all = BMBS_OK;
    for (Lane* c : X->lanes) { const int rc = lane_settle(c); if (rc) { X->err = c->err; rc_all = rc; } }
    return rc_all;
}

// lanes a device call is dealt to.  Measured on one box, lanes overlapping (round 6; M reads/s at 2 / 3 / 4 lanes): uniform-random genome
// 1249 / 1211-vs-1201 / 1179 -- the seeding kernels there sit at the gather ceiling and a fourth lane only adds contention --;
// GRCh38-like pairs 622 / 640 / 646, single-end 412 / 419 / 421, --sensitive 428 / 440 / 450 -- the list kernels wait on their own
// chains and fill with whatever else is resident.  Three it is.  (Four on repeat-rich input, chosen from what
// settled calls had shown, was built and taken out again: a call's chunk boundaries -- and with them the records' cigar_off -- then
// differed between the first and the second call of a context on the same input.)
int device_lanes(const bmbs_ctx* X) { return std::min<int>((int)X->lanes.size(), X->kn.lanes); }
// ---- the chunk plan of a mapping call: how its n units (reads, or pairs: rpu records each) are cut into chunks of ch, and the one
// place that says where chunk k starts, how long it is, which lane takes it and which part of the caller's CIGAR pool is its own
struct ChunkPlan {
    bool pe = false, whole = true;               // whole: the call runs as one chunk on lane 0, on the caller's pool as it is
    int32_t L = 0; int rpu = 1, max_ops = 0, used_lanes = 1;
    int64_t n = 0, ch = 0, n_chunks = 0, cigar_cap = 0;
    int64_t off(int64_t k) const { return k * ch; }
    int64_t units(int64_t k) const { return std::min(ch, n - off(k)); }
    int lane(int64_t k) const { return (int)(k % used_lanes); }
    int64_t worst_case(int64_t k) const { return units(k) * rpu * (int64_t)max_ops; }      // CIGAR words if every read of chunk k needs K12
    u64 cigar_base(int64_t k) const { return whole ? 0 : (u64)off(k) * rpu * (u64)max_ops; }
    int64_t cigar_room(int64_t k) const { return whole ? cigar_cap : worst_case(k); }       // what of the caller's pool belongs to chunk k
};
// host_copies: a host call -- its chunks carry their own H2D / D2H copies and are dealt to every lane of the context, not to device_lanes of them
ChunkPlan plan_chunks(const bmbs_ctx* X, bool pe, int32_t L, int64_t n, int64_t cigar_cap, bool host_copies)
{
    ChunkPlan p;
    p.pe = pe; p.L = L; p.rpu = pe ? 2 : 1; p.max_ops = cigar_ops_bound(X->prm, L, threshold_k(X->prm, L)); p.n = p.ch = n; p.cigar_cap = cigar_cap;
    const int64_t nl = host_copies ? (int64_t)X->lanes.size() : device_lanes(X);
    // a small call is not cut, and neither is one whose pool has no room for every chunk's worst case
    if (nl >= 2 && n >= 2 * X->kn.split_min && cigar_cap >= n * p.rpu * (int64_t)p.max_ops) {
        p.ch = X->kn.chunk > 0 ? X->kn.chunk : (n + nl - 1) / nl;            // one chunk per lane (BMBS_CHUNK overrides)
        // ... and smaller ones where they carry copies: a shorter tail behind the last upload (a call of 2 M pairs: 126 M reads/s in
        // chunks of 500 k, 133-138 in chunks of 250 k -- the first upload and the last chunk's kernels and download are not hidden
        // behind anything; tools/hostbuf_ab.py)
        if (host_copies && X->kn.chunk <= 0) p.ch = std::min<int64_t>(p.ch, std::min<int64_t>(500000, std::max<int64_t>(250000, n / 8)));
        p.ch = std::max<int64_t>(p.ch, X->kn.split_min);
    }
    p.whole = p.ch >= n;
    if (p.whole) p.ch = n;
    p.n_chunks = n > 0 ? (n + p.ch - 1) / p.ch : 0;
    p.used_lanes = (int)std::min<int64_t>(nl, p.n_chunks);
    return p;
}
// chunk k as the launch sequences take it: its rows at a[] (seq 1, qual 1, seq 2, qual 2; `stride` bytes apart), its lengths, where its records and CIGAR words go
Pending chunk_pending(const ChunkPlan& p, int64_t k, int32_t stride, const uint64_t a[4], const u16* d_len, uint64_t d_results, uint64_t d_cigar_pool, int64_t pool_cap)
{
    Pending P;
    P.pe = p.pe; P.L = p.L; P.stride = stride; P.n = p.units(k); P.d_len = d_len;
    for (int i = 0; i < (p.pe ? 4 : 2); i++) P.a[i] = a[i];
    P.d_results = d_results; P.d_cigar_pool = d_cigar_pool; P.cigar_cap = pool_cap; P.cigar_base = (u32)p.cigar_base(k);
    return P;
}
// *_device entry points: the call is cut into chunks dealt to the lanes in turn; nothing waits (bmbs_sync does)
struct DevIn { uint64_t seq1 = 0, qual1 = 0, seq2 = 0, qual2 = 0; const u16* len = nullptr; };      // len: [n first mates][n second mates]
int dispatch_device(bmbs_ctx* X, bool pe, const DevIn& in, int32_t L, int32_t stride, int64_t n, uint64_t d_results, uint64_t d_cigar_pool, int64_t cigar_cap)
{
    if (!X || X->lanes.empty()) return BMBS_EINVAL;
    if (L <= 0 || L > BMBS_MAX_READ || stride < L || n < 0) { X->err = "bad read geometry"; return BMBS_EINVAL; }
    if (n == 0) return BMBS_OK;
    share_needs(X);
    const ChunkPlan p = plan_chunks(X, pe, L, n, cigar_cap, false);        // (fixed for the call, whatever a lane that settles meanwhile learns)
    for (int64_t k = 0; k < p.n_chunks; k++) {
        Lane* c = X->lanes[(size_t)p.lane(k)];
        const int64_t off = p.off(k), m = p.units(k);
        const uint64_t ro = (uint64_t)off * (uint64_t)stride;
        const uint64_t a[4] = {in.seq1 + ro, in.qual1 + ro, in.seq2 + ro, in.qual2 + ro};
        const u16* len = in.len && !p.whole ? in.len + off : in.len;
        const bool staged = in.len && !p.whole && pe;
        if (staged) {
            // a chunk of pairs wants its lengths as [m first mates][m second mates]: re-laid into the lane's own array
            HIPCHK(c, hipSetDevice(c->dev));
            if (!c->inflight.empty()) { const int rs = lane_settle(c); if (rs) { X->err = c->err; return rs; } }
            ENS(c, c->in_len, (u64)m * 4 + 16);
            HIPCHK(c, hipMemcpyAsync(c->in_len.as<u16>(), in.len + off, (size_t)m * 2, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->in_len.as<u16>() + m, in.len + n + off, (size_t)m * 2, hipMemcpyDeviceToDevice, c->stream));
            len = c->in_len.as<u16>();
        }
        const Pending P = chunk_pending(p, k, stride, a, len, d_results + (uint64_t)off * p.rpu * 32, d_cigar_pool + p.cigar_base(k) * 4, p.cigar_room(k));
        const int rc = lane_enqueue(c, P, staged);
        if (rc) { X->err = c->err; return rc; }
    }
    X->used_lanes = p.used_lanes;
    return BMBS_OK;
}

// host entry points: chunk k is uploaded, mapped and read back on lane k % lanes -- its copies run beside the kernels of the
// chunks on the other lanes (one direction of the link each: 48 GB/s both ways at once on the MI355X boxes, tools/pcie_probe).
// Per mate: ASCII rows or (hw > 0) packed rows hw words apart, quality bytes or (qw > 0) packed quality classes qw words apart, lengths or none
struct HostMate { const char *seq = nullptr, *qual = nullptr; const uint16_t* len = nullptr; const uint64_t *rows = nullptr, *qrows = nullptr; };
struct HostIn { HostMate m[2]; int hw = 0, qw = 0; };
// a host-buffer call, stage by stage: issue (upload, expand_quals, enqueue) puts chunk k on its lane, finish takes it off again
struct HostCall {
    bmbs_ctx* X; const HostIn& in; int32_t stride; bmbs_result* results; uint32_t* cigar_pool; const ChunkPlan p;
    const int ds = (p.L + 15) / 16 * 16;                                        // stride of the rows on the device: what upload_rows gives them
    std::vector<int64_t> open = std::vector<int64_t>(X->lanes.size(), -1);      // per lane: the chunk in flight (-1: none)
    std::atomic<int64_t> extent{0};                                             // words of the caller's CIGAR pool in use
    int rc = BMBS_OK; std::mutex err_mu; std::atomic<int> stop{0};
    static hipStream_t up_of(const Lane* c) { return copy_streams(c) ? c->up_stream : c->stream; }
    static hipStream_t down_of(const Lane* c) { return copy_streams(c) ? c->down_stream : c->stream; }
    // chunk k of an array of w words per read (packed rows, packed quality classes): it goes over as it is, one block per mate
    int upload_words(Lane* c, DevBuf& dst, const uint64_t* src, int w, int64_t k)
    {
        ENS(c, dst, (u64)p.units(k) * (u64)w * 8 + 64);
        HIPCHK(c, hipMemcpyAsync(dst.p, src + (size_t)p.off(k) * (size_t)w, (u64)p.units(k) * (u64)w * 8, hipMemcpyHostToDevice, up_of(c)));
        return BMBS_OK;
    }
    int upload_bytes(Lane* c, DevBuf& dst, const char* src, int64_t k)
    { int to = 0; return upload_rows(c, dst, src + (size_t)p.off(k) * (size_t)stride, p.L, stride, (u64)p.units(k), &to, up_of(c)); }
    // everything chunk k reads, on the upload stream: rows, qualities, lengths; the kernel stream waits for the last of them
    int upload(Lane* c, int64_t k)
    {
        const HostMate &m1 = in.m[0], &m2 = in.m[1];
        const u64 um = (u64)p.units(k); int r = BMBS_OK;
        if (in.hw) { r = upload_words(c, c->pk_in1, m1.rows, in.hw, k); if (!r && p.pe) r = upload_words(c, c->pk_in2, m2.rows, in.hw, k); }
        else r = upload_bytes(c, c->in_seq, m1.seq, k);
        if (r) return r;
        if (in.qw) {                                // (the byte rows expand_quals writes are sized here, with the upload buffers)
            ENS(c, c->in_qual, um * (u64)ds + 64);
            r = upload_words(c, c->pq_in1, m1.qrows, in.qw, k);
            if (!r && p.pe) { ENS(c, c->in_qual2, um * (u64)ds + 64); r = upload_words(c, c->pq_in2, m2.qrows, in.qw, k); }
        } else r = upload_bytes(c, c->in_qual, m1.qual, k);
        if (r) return r;
        if (p.pe && !in.hw) { r = upload_bytes(c, c->in_seq2, m2.seq, k); if (r) return r; }
        if (p.pe && !in.qw) { r = upload_bytes(c, c->in_qual2, m2.qual, k); if (r) return r; }
        if (m1.len) {
            r = upload_lens(c, m1.len + p.off(k), um, 0, um * p.rpu, p.L, up_of(c));
            if (!r && p.pe) r = upload_lens(c, m2.len + p.off(k), um, um, um * p.rpu, p.L, up_of(c));
            if (r) return r;
        }
        if (copy_streams(c)) { HIPCHK(c, hipEventRecord(c->ev_up, c->up_stream)); HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_up, 0)); }
        return BMBS_OK;
    }
    // packed quality classes -> the byte rows, at the stride upload_rows would have given them: on the kernel stream, in front of the call, so that a
    // chunk issued again with exact sizes finds them in place.  Its two events stand outside the call's event set: finish adds their time to the running sums
    int expand_quals(Lane* c, int64_t k)
    {
        const int Wq = ds / 16;
        const u64 words = (u64)p.units(k) * (u64)Wq * (u64)p.rpu;
        if (!c->ev_qx_a) { HIPCHK(c, hipEventCreate(&c->ev_qx_a)); HIPCHK(c, hipEventCreate(&c->ev_qx_b)); }
        const QualRep rep = {c->qrep_lo, c->qrep_hi};
        HIPCHK(c, hipEventRecord(c->ev_qx_a, c->stream));
        hipLaunchKernelGGL(k_qual_expand, dim3(std::min<unsigned>(nblk(words, 256), 4096u)), dim3(256), 0, c->stream, c->pq_in1.as<u64>(),
                           p.pe ? c->pq_in2.as<u64>() : (const u64*)nullptr, in.qw, Wq, (long)p.units(k), rep, c->in_qual.as<uint4>(),
                           p.pe ? c->in_qual2.as<uint4>() : (uint4*)nullptr);
        HIPCHK(c, hipEventRecord(c->ev_qx_b, c->stream));
        c->qx_timed = true;
        return BMBS_OK;
    }
    // the call on the lane's staging buffers, and the records' download behind it
    int enqueue(Lane* c, int64_t k)
    {
        const uint64_t a[4] = {(uint64_t)(in.hw ? c->pk_in1.p : c->in_seq.p), (uint64_t)c->in_qual.p, (uint64_t)(in.hw ? c->pk_in2.p : c->in_seq2.p), (uint64_t)c->in_qual2.p};
        Pending P = chunk_pending(p, k, ds, a, in.m[0].len ? c->in_len.as<u16>() : nullptr, (uint64_t)c->out_res.p, (uint64_t)c->cig_pool.p, p.worst_case(k));
        P.packed_hw = in.hw;
        { const int r = lane_enqueue(c, P, true); if (r) return r; }
        if (copy_streams(c)) { HIPCHK(c, hipEventRecord(c->ev_k, c->stream)); HIPCHK(c, hipStreamWaitEvent(c->down_stream, c->ev_k, 0)); }
        HIPCHK(c, hipMemcpyAsync(results + p.off(k) * p.rpu, c->out_res.p, (u64)p.units(k) * p.rpu * 32, hipMemcpyDeviceToHost, down_of(c)));
        return BMBS_OK;
    }
    // upload, kernels and the records' download of chunk k on its lane (whose previous chunk has been finished)
    int issue(Lane* c, int64_t k)
    {
        HIPCHK(c, hipSetDevice(c->dev));
        ENS(c, c->out_res, (u64)p.units(k) * p.rpu * 32);
        ENS(c, c->cig_pool, (u64)p.worst_case(k) * 4);
        // One upload at a time per device (the text calls' rule, bmbs_textpath.hip): four lanes that upload side by side share the
        // link, finish together, compute together and leave the link idle meanwhile -- in turn, each chunk goes up at the full
        // rate and its kernels run beside the next lane's upload.  The lock is held until this chunk's copies have ended; the
        // kernels are queued behind them meanwhile.  BMBS_UP_TURNS=0: the round-5 form.  (ONE upload stream shared by the lanes --
        // copies back to back with no host in between -- measured no better than side-by-side uploads: 172 against 174 / 165 M
        // reads/s, turns 186 / 192; 2 M pairs per call, profiles/HISTORY.md)
        std::unique_lock<std::mutex> up_turn(g_h2d_mu[c->dev & 15], std::defer_lock);
        if (copy_streams(c) && p.used_lanes > 1 && c->kn.up_turns) up_turn.lock();
        int r = upload(c, k);
        if (!r && in.qw) r = expand_quals(c, k);
        if (!r) r = enqueue(c, k);
        if (r) return r;
        if (up_turn.owns_lock()) HIPCHK(c, hipEventSynchronize(c->ev_up));          // this chunk is up: the next lane's turn
        return BMBS_OK;
    }
    // the chunk in flight on lane li: its counts, then exactly the CIGAR operations it produced
    int finish(int li)
    {
        const int64_t k = std::exchange(open[(size_t)li], -1);
        if (k < 0) return BMBS_OK;
        Lane* c = X->lanes[(size_t)li];
        const u64 retries0 = c->n_retries;
        { const int r = lane_settle(c); if (r) return r; }
        if (c->qx_timed) { c->qx_timed = false; prof_add(c, "k_qual_expand", c->ev_qx_a, c->ev_qx_b); }
        if (c->n_retries != retries0)               // the chunk was issued again with exact sizes: the records copied behind the first attempt are stale
            HIPCHK(c, hipMemcpyAsync(results + p.off(k) * p.rpu, c->out_res.p, (u64)p.units(k) * p.rpu * 32, hipMemcpyDeviceToHost, down_of(c)));
        const u64 used = c->last_n_jobs * (u64)p.max_ops, base = p.cigar_base(k);
        if (base + used > (u64)p.cigar_cap) { c->err = "host cigar pool too small"; return BMBS_ENOMEM; }
        if (used) {
            HIPCHK(c, hipMemcpyAsync(cigar_pool + base, c->cig_pool.p, used * 4, hipMemcpyDeviceToHost, down_of(c)));
            int64_t seen = extent.load();
            while ((int64_t)(base + used) > seen && !extent.compare_exchange_weak(seen, (int64_t)(base + used))) {}
        }
        HIPCHK(c, hipStreamSynchronize(down_of(c)));
        return BMBS_OK;
    }
    // the chunks of lane li, one behind the other; the first error of the call wins rc and X->err and stops the other lanes
    void run_lane(int li)
    {
        Lane* c = X->lanes[(size_t)li];
        (void)hipSetDevice(c->dev);
        int r = BMBS_OK;
        for (int64_t k = li; k < p.n_chunks && !r && !stop.load(); k += p.used_lanes) {
            r = finish(li);
            if (!r) r = issue(c, k);
            if (!r) open[(size_t)li] = k;
        }
        if (!r) r = finish(li);
        if (r) { stop.store(1); std::lock_guard<std::mutex> l(err_mu); if (!rc) { rc = r; X->err = c->err; } }
    }
    // One host thread per lane: a chunk is ~110 kernel launches and a handful of waits, and with all of them issued by one thread the
    // call was bound by that thread on boxes with slower cores (2 M pairs through bmbs_map_pe_packed: 137 M reads/s where the link
    // would give 200).  Chunk k goes to lane k % lanes whoever issues it: the results do not depend on the threads.
    int run()
    {
        std::vector<std::thread> th;
        for (int t = 1; t < p.used_lanes; t++) th.emplace_back(&HostCall::run_lane, this, t);
        run_lane(0);
        for (auto& t : th) t.join();
        if (rc) for (Lane* c : X->lanes) { (void)hipStreamSynchronize(c->stream); if (c->down_stream) (void)hipStreamSynchronize(c->down_stream); c->inflight.clear(); }
        return rc;
    }
};
int dispatch_host(bmbs_ctx* X, bool pe, const HostIn& in, int32_t L, int32_t stride, int64_t n, bmbs_result* results, uint32_t* pool, int64_t cigar_cap, int64_t* n_cigar_used)
{
    static_assert(sizeof(bmbs_result) == 32 && sizeof(bmbs_result_dev) == 32, "result record is 32 bytes");
    if (!X || X->lanes.empty()) return BMBS_EINVAL;
    if (n_cigar_used) *n_cigar_used = 0;
    if (n <= 0) return BMBS_OK;
    if (L <= 0 || L > BMBS_MAX_READ || stride < L) { X->err = "bad read geometry"; return BMBS_EINVAL; }
    share_needs(X);
    HostCall call{X, in, stride, results, pool, plan_chunks(X, pe, L, n, cigar_cap, true)};
    { const int rc = call.run(); if (rc) return rc; }
    X->used_lanes = call.p.used_lanes;
    if (n_cigar_used) *n_cigar_used = call.extent.load();
    return BMBS_OK;
}

extern "C" int bmbs_sync(bmbs_ctx* X) { return X ? settle_all(X) : BMBS_EINVAL; }

extern "C" int bmbs_map_se_device(bmbs_ctx* X, uint64_t d_seq, uint64_t d_qual, int32_t L, int32_t stride,
                                  int64_t n_reads, uint64_t d_results, uint64_t d_cigar_pool, int64_t cigar_cap)
{
    DevIn in; in.seq1 = d_seq; in.qual1 = d_qual;
    return dispatch_device(X, false, in, L, stride, n_reads, d_results, d_cigar_pool, cigar_cap);
}
extern "C" int bmbs_map_se_var_device(bmbs_ctx* X, uint64_t d_seq, uint64_t d_qual, uint64_t d_len, int32_t L_max, int32_t stride,
                                      int64_t n_reads, uint64_t d_results, uint64_t d_cigar_pool, int64_t cigar_cap)
{
    if (X && !d_len) { X->err = "d_len is NULL"; return BMBS_EINVAL; }
    DevIn in; in.seq1 = d_seq; in.qual1 = d_qual; in.len = reinterpret_cast<const u16*>(d_len);
    return dispatch_device(X, false, in, L_max, stride, n_reads, d_results, d_cigar_pool, cigar_cap);
}
extern "C" int bmbs_map_se(bmbs_ctx* X, const char* seq, const char* qual, int32_t L, int32_t stride, int64_t n_reads,
                           bmbs_result* results, uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used)
{
    HostIn in; in.m[0].seq = seq; in.m[0].qual = qual;
    return dispatch_host(X, false, in, L, stride, n_reads, results, cigar_pool, cigar_cap, n_cigar_used);
}
extern "C" int bmbs_map_se_var(bmbs_ctx* X, const char* seq, const char* qual, const uint16_t* len, int32_t L_max, int32_t stride,
                               int64_t n_reads, bmbs_result* results, uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used)
{
    if (X && !len) { X->err = "len is NULL"; return BMBS_EINVAL; }
    HostIn in; in.m[0].seq = seq; in.m[0].qual = qual; in.m[0].len = len;
    return dispatch_host(X, false, in, L_max, stride, n_reads, results, cigar_pool, cigar_cap, n_cigar_used);
}
extern "C" int bmbs_map_pe_device(bmbs_ctx* X, uint64_t d_seq1, uint64_t d_qual1, uint64_t d_seq2, uint64_t d_qual2, int32_t L, int32_t stride,
                                  int64_t n_pairs, uint64_t d_results, uint64_t d_cigar_pool, int64_t cigar_cap)
{
    DevIn in; in.seq1 = d_seq1; in.qual1 = d_qual1; in.seq2 = d_seq2; in.qual2 = d_qual2;
    return dispatch_device(X, true, in, L, stride, n_pairs, d_results, d_cigar_pool, cigar_cap);
}
extern "C" int bmbs_map_pe_var_device(bmbs_ctx* X, uint64_t d_seq1, uint64_t d_qual1, uint64_t d_seq2, uint64_t d_qual2, uint64_t d_len,
                                      int32_t L_max, int32_t stride, int64_t n_pairs, uint64_t d_results, uint64_t d_cigar_pool, int64_t cigar_cap)
{
    if (X && !d_len) { X->err = "d_len is NULL"; return BMBS_EINVAL; }
    DevIn in; in.seq1 = d_seq1; in.qual1 = d_qual1; in.seq2 = d_seq2; in.qual2 = d_qual2; in.len = reinterpret_cast<const u16*>(d_len);
    return dispatch_device(X, true, in, L_max, stride, n_pairs, d_results, d_cigar_pool, cigar_cap);
}
extern "C" int bmbs_map_pe(bmbs_ctx* X, const char* seq1, const char* qual1, const char* seq2, const char* qual2, int32_t L, int32_t stride,
                           int64_t n_pairs, bmbs_result* results, uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used)
{
    HostIn in; in.m[0].seq = seq1; in.m[0].qual = qual1; in.m[1].seq = seq2; in.m[1].qual = qual2;
    return dispatch_host(X, true, in, L, stride, n_pairs, results, cigar_pool, cigar_cap, n_cigar_used);
}
extern "C" int bmbs_map_pe_var(bmbs_ctx* X, const char* seq1, const char* qual1, const char* seq2, const char* qual2, const uint16_t* len1, const uint16_t* len2,
                               int32_t L_max, int32_t stride, int64_t n_pairs, bmbs_result* results, uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used)
{
    if (X && (!len1 || !len2)) { X->err = "len1 / len2 is NULL"; return BMBS_EINVAL; }
    HostIn in; in.m[0].seq = seq1; in.m[0].qual = qual1; in.m[0].len = len1; in.m[1].seq = seq2; in.m[1].qual = qual2; in.m[1].len = len2;
    return dispatch_host(X, true, in, L_max, stride, n_pairs, results, cigar_pool, cigar_cap, n_cigar_used);
}

// ---- packed reads (include/bmbs.h): 2 bits per base + an 'N' plane instead of a byte per base ---------------------------------------------
extern "C" int bmbs_map_se_packed(bmbs_ctx* X, const uint64_t* rows, int32_t pwords, const char* qual, const uint16_t* len, int32_t L_max, int32_t stride,
                                  int64_t n_reads, bmbs_result* results, uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used)
{
    if (X && (!rows || !qual || pwords <= 0)) { X->err = "packed reads: NULL rows / qualities or pwords <= 0"; return BMBS_EINVAL; }
    HostIn in; in.hw = pwords; in.m[0].rows = rows; in.m[0].qual = qual; in.m[0].len = len;
    return dispatch_host(X, false, in, L_max, stride, n_reads, results, cigar_pool, cigar_cap, n_cigar_used);
}
extern "C" int bmbs_map_pe_packed(bmbs_ctx* X, const uint64_t* rows1, const uint64_t* rows2, int32_t pwords, const char* qual1, const char* qual2,
                                  const uint16_t* len1, const uint16_t* len2, int32_t L_max, int32_t stride, int64_t n_pairs, bmbs_result* results,
                                  uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used)
{
    if (X && (!rows1 || !rows2 || !qual1 || !qual2 || pwords <= 0 || (len1 != nullptr) != (len2 != nullptr))) { X->err = "packed reads: NULL rows / qualities, pwords <= 0, or only one of len1 / len2"; return BMBS_EINVAL; }
    HostIn in; in.hw = pwords;
    in.m[0].rows = rows1; in.m[0].qual = qual1; in.m[0].len = len1;
    in.m[1].rows = rows2; in.m[1].qual = qual2; in.m[1].len = len2;
    return dispatch_host(X, true, in, L_max, stride, n_pairs, results, cigar_pool, cigar_cap, n_cigar_used);
}
// ---- packed quality classes (include/bmbs.h): a 4-bit penalty class per base instead of the quality byte ------------------------------------
extern "C" int bmbs_qual_classes(const bmbs_params* params, uint8_t class_of[256], int32_t penalty_of[16], int32_t* n_classes)
{
    if (!class_of || !penalty_of || !n_classes) return BMBS_EINVAL;
    bmbs_params P;
    if (params) P = *params; else bmbs_default_params(&P);
    qual_class_table(P, class_of, penalty_of, n_classes, nullptr);
    return BMBS_OK;
}
extern "C" int bmbs_map_se_packedq(bmbs_ctx* X, const uint64_t* rows, int32_t pwords, const uint64_t* qrows, int32_t qwords, const uint16_t* len, int32_t L_max,
                                   int64_t n_reads, bmbs_result* results, uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used)
{
    if (X && (!rows || !qrows || pwords <= 0 || qwords <= 0)) { X->err = "packed reads: NULL rows / quality classes or pwords / qwords <= 0"; return BMBS_EINVAL; }
    if (X && L_max > 0 && qwords < (L_max + 15) / 16) { X->err = "packed quality classes: qwords is smaller than a row of this length takes"; return BMBS_EINVAL; }
    HostIn in; in.hw = pwords; in.qw = qwords; in.m[0].rows = rows; in.m[0].qrows = qrows; in.m[0].len = len;
    return dispatch_host(X, false, in, L_max, std::max(L_max, 0), n_reads, results, cigar_pool, cigar_cap, n_cigar_used);
}
extern "C" int bmbs_map_pe_packedq(bmbs_ctx* X, const uint64_t* rows1, const uint64_t* rows2, int32_t pwords, const uint64_t* qrows1, const uint64_t* qrows2,
                                   int32_t qwords, const uint16_t* len1, const uint16_t* len2, int32_t L_max, int64_t n_pairs, bmbs_result* results,
                                   uint32_t* cigar_pool, int64_t cigar_cap, int64_t* n_cigar_used)
{
    if (X && (!rows1 || !rows2 || !qrows1 || !qrows2 || pwords <= 0 || qwords <= 0 || (len1 != nullptr) != (len2 != nullptr))) {
        X->err = "packed reads: NULL rows / quality classes, pwords / qwords <= 0, or only one of len1 / len2"; return BMBS_EINVAL;
    }
    if (X && L_max > 0 && qwords < (L_max + 15) / 16) { X->err = "packed quality classes: qwords is smaller than a row of this length takes"; return BMBS_EINVAL; }
    HostIn in; in.hw = pwords; in.qw = qwords;
    in.m[0].rows = rows1; in.m[0].qrows = qrows1; in.m[0].len = len1;
    in.m[1].rows = rows2; in.m[1].qrows = qrows2; in.m[1].len = len2;
    return dispatch_host(X, true, in, L_max, std::max(L_max, 0), n_pairs, results, cigar_pool, cigar_cap, n_cigar_used);
}
// quality bytes -> packed classes on the host's threads (once per batch, like bmbs_pack_rows).  -> BMBS_OK, or BMBS_EINVAL with *bad_row = the
// first row that holds a byte without a class (or whose length is 0 or beyond L_max)
extern "C" int bmbs_pack_quals(const bmbs_params* params, const char* qual, int32_t L_max, int32_t stride, int64_t n, const uint16_t* len, uint64_t* qrows,
                               int32_t qwords, int32_t threads, int64_t* bad_row)
{
    const int Wq = (L_max + 15) / 16;
    if (bad_row) *bad_row = -1;
    if (!qual || !qrows || L_max <= 0 || L_max > BMBS_MAX_READ || stride < L_max || qwords < Wq || n < 0) return BMBS_EINVAL;
    bmbs_params P;
    if (params) P = *params; else bmbs_default_params(&P);
    uint8_t cls[256]; int32_t penalty_of[16], nc = 0;
    qual_class_table(P, cls, penalty_of, &nc, nullptr);
    // the 256-byte class table, squared: two quality bytes -> their two nibbles in one lookup (the pairs real qualities form touch a few
    // dozen lines of it); a byte without a class sets the entry's high byte.  One byte at a time the packer ran at 1.3 GB/s per thread
    std::vector<uint16_t> pair_((size_t)65536);
    uint16_t* pair = pair_.data();
    for (int b1 = 0; b1 < 256; b1++)
        for (int b0 = 0; b0 < 256; b0++)
            pair[(b1 << 8) | b0] = (uint16_t)((cls[b0] & 15) | ((cls[b1] & 15) << 4) | ((cls[b0] | cls[b1]) & 0xF0 ? 0x100 : 0));
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(threads > 0 ? threads : 1, n / 4096 + 1));
    std::vector<int64_t> bad((size_t)T, -1);
    auto work = [&](int t) {
        const int64_t a = n * t / T, e = n * (t + 1) / T;
        for (int64_t r = a; r < e; r++) {
            const unsigned char* s = reinterpret_cast<const unsigned char*>(qual) + (size_t)r * (size_t)stride;
            uint64_t* o = qrows + (size_t)r * (size_t)qwords;
            const int Lr = len ? (int)len[r] : L_max;
            if (Lr <= 0 || Lr > L_max) { for (int q = 0; q < qwords; q++) o[q] = 0; if (bad[(size_t)t] < 0) bad[(size_t)t] = r; continue; }
            unsigned seen = 0;
            const int full = Lr >> 4;
            for (int w = 0; w < full; w++, s += 16) {
                uint64_t in[2], x = 0;
                memcpy(in, s, 16);
                for (int h = 0; h < 2; h++)
                    for (int k = 0; k < 4; k++) { const unsigned c = pair[(in[h] >> (16 * k)) & 0xffffu]; seen |= c; x |= (uint64_t)(c & 0xffu) << (32 * h + 8 * k); }
                o[w] = x;
            }
            int w = full;
            if (Lr & 15) {
                uint64_t x = 0;
                for (int k = 0; k < (Lr & 15); k++) { const unsigned c = cls[s[k]]; seen |= c >> 4 ? 0x100u : 0u; x |= (uint64_t)(c & 15u) << (4 * k); }
                o[w++] = x;
            }
            for (; w < qwords; w++) o[w] = 0;
            if ((seen & 0x100u) && bad[(size_t)t] < 0) bad[(size_t)t] = r;
        }
    };
    if (T == 1) work(0);
    else { std::vector<std::thread> th; for (int t = 0; t < T; t++) th.emplace_back(work, t); for (auto& x : th) x.join(); }
    for (int t = 0; t < T; t++) if (bad[(size_t)t] >= 0) { if (bad_row) *bad_row = bad[(size_t)t]; return BMBS_EINVAL; }
    return BMBS_OK;
}
// ASCII rows -> packed rows on the host's threads (what a caller's reader does once per batch).  -> BMBS_OK, or BMBS_EINVAL with *bad_row =
// the first row that holds a character other than A C G T N
extern "C" int bmbs_pack_rows(const char* seq, int32_t L_max, int32_t stride, int64_t n, const uint16_t* len, uint64_t* rows, int32_t pwords, int32_t threads,
                              int64_t* bad_row)
{
    const int W = (L_max + 31) / 32, M = (L_max + 63) / 64;
    if (bad_row) *bad_row = -1;
    if (!seq || !rows || L_max <= 0 || L_max > BMBS_MAX_READ || stride < L_max || pwords < W + M || n < 0) return BMBS_EINVAL;
    static unsigned char code[256]; static std::once_flag once;
    std::call_once(once, [] { for (int i = 0; i < 256; i++) code[i] = 5; code[(int)'A'] = 0; code[(int)'C'] = 1; code[(int)'G'] = 2; code[(int)'T'] = 3; code[(int)'N'] = 4; });
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(threads > 0 ? threads : 1, n / 4096 + 1));
    std::vector<int64_t> bad((size_t)T, -1);
    auto work = [&](int t) {
        const int64_t a = n * t / T, e = n * (t + 1) / T;
        for (int64_t r = a; r < e; r++) {
            const unsigned char* s = reinterpret_cast<const unsigned char*>(seq) + (size_t)r * (size_t)stride;
            uint64_t* o = rows + (size_t)r * (size_t)pwords;
            const int Lr = len ? (int)len[r] : L_max;
            for (int q = 0; q < pwords; q++) o[q] = 0;
            // (the rule upload_lens applies later: a length of 0 or beyond L_max would read past the row and write past its words)
            if (Lr <= 0 || Lr > L_max) { if (bad[(size_t)t] < 0) bad[(size_t)t] = r; continue; }
            for (int j = 0; j < Lr; j++) {
                const unsigned c = code[s[j]];
                if (c < 4) o[j >> 5] |= (uint64_t)c << (2 * (j & 31));
                else if (c == 4) o[W + (j >> 6)] |= 1ull << (j & 63);
                else if (bad[(size_t)t] < 0) bad[(size_t)t] = r;
            }
        }
    };
    if (T == 1) work(0);
    else { std::vector<std::thread> th; for (int t = 0; t < T; t++) th.emplace_back(work, t); for (auto& x : th) x.join(); }
    for (int t = 0; t < T; t++) if (bad[(size_t)t] >= 0) { if (bad_row) *bad_row = bad[(size_t)t]; return BMBS_EINVAL; }
    return BMBS_OK;
}

// ------------------------------------------------------------------------------------------------
static int lane_locate_batch(Lane* c, const uint64_t* row, int64_t n_rows, uint64_t* pos)
{
    if (!c) return BMBS_EINVAL;
    if (!c->attached) { c->err = "no index attached"; return BMBS_ESTATE; }
    if (n_rows <= 0) return BMBS_OK;
    HIPCHK(c, hipSetDevice(c->dev));
    const u64 m = (u64)n_rows;
    ENS(c, c->in_a, m * 8); ENS(c, c->in_b, m * 8);
    HIPCHK(c, hipMemcpyAsync(c->in_a.p, row, m * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_locate_rows, dim3(nblk(m, 256)), dim3(256), 0, c->stream, c->ix, c->in_a.as<u64>(), (long)m, c->in_b.as<u64>());
    HIPCHK(c, hipMemcpyAsync(pos, c->in_b.p, m * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BMBS_OK;
}

// A second context on the index of another one (same device): it takes the device pointers, owns none of the index memory and
// has its own stream and work buffers.  Two such contexts driven by two host threads keep two batches in flight: the kernels of
// one hide the memory waits and the low-occupancy phases of the other's.
extern "C" int bmbs_index_share(bmbs_ctx* X, const bmbs_ctx* owner)
{
    if (!X || !owner || X->lanes.empty() || owner->lanes.empty()) return BMBS_EINVAL;
    const Lane* o = owner->lanes[0];
    if (!o->attached) { X->err = "index share: the owner has no index attached"; return BMBS_ESTATE; }
    if (X->dev != owner->dev) { X->err = "index share: contexts on different devices"; return BMBS_EINVAL; }
    if (X->lanes[0]->attached) { X->err = "index share: this context already has an index"; return BMBS_ESTATE; }
    for (Lane* c : X->lanes) { c->ix = o->ix; c->rows = o->rows; c->o3 = o->o3; c->attached = true; }
    return BMBS_OK;
}

static int lane_vote_order_batch(Lane* c, const uint8_t* vote, const int64_t* seg_off, int64_t n_seg, int32_t form,
                                     uint32_t* perm)
{
    if (!c) return BMBS_EINVAL;
    if (n_seg <= 0) return BMBS_OK;
    if (form != 0 && form != 1) { c->err = "vote order: form is 0 (wave) or 1 (block)"; return BMBS_EINVAL; }
    const int64_t cap = form ? VL_CAP : VM_CAP;
    for (int64_t s = 0; s < n_seg; s++)
        if (seg_off[s + 1] < seg_off[s] || seg_off[s + 1] - seg_off[s] > cap) { c->err = "vote order: list longer than the form's capacity"; return BMBS_EINVAL; }
    const u64 m = (u64)seg_off[n_seg] - (u64)seg_off[0];
    if (m == 0) return BMBS_OK;
    HIPCHK(c, hipSetDevice(c->dev));
    ENS(c, c->in_a, ((u64)n_seg + 1) * 8); ENS(c, c->in_b, m * 4); ENS(c, c->in_seq, (u64)seg_off[n_seg] + 64);
    HIPCHK(c, hipMemcpyAsync(c->in_a.p, seg_off, ((u64)n_seg + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->in_seq.p, vote, (u64)seg_off[n_seg], hipMemcpyHostToDevice, c->stream));
    const u64 grid = (u64)n_seg < 65536 ? (u64)n_seg : 65536;
    // perm is indexed like vote (seg_off[0] may be > 0): the kernel writes perm[a + j], so shift the base
    u32* dperm = c->in_b.as<u32>() - seg_off[0];
    if (form) hipLaunchKernelGGL((k_vote_order<VL_CAP, VL_BLOCK>), dim3(grid), dim3(VL_BLOCK), 0, c->stream, c->in_seq.as<uint8_t>(), c->in_a.as<long>(), (long)n_seg, dperm);
    else hipLaunchKernelGGL((k_vote_order<VM_CAP, VM_BLOCK>), dim3(grid), dim3(VM_BLOCK), 0, c->stream, c->in_seq.as<uint8_t>(), c->in_a.as<long>(), (long)n_seg, dperm);
    HIPCHK(c, hipMemcpyAsync(perm + seg_off[0], c->in_b.p, m * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BMBS_OK;
}

static int lane_window_batch(Lane* c, const uint64_t* site, int64_t n_sites, int32_t len, char* out)
{
    if (!c) return BMBS_EINVAL;
    if (!c->attached) { c->err = "no index attached"; return BMBS_ESTATE; }
    if (n_sites <= 0) return BMBS_OK;
    if (len <= 0 || len > 1024) { c->err = "window length out of range"; return BMBS_EINVAL; }
    HIPCHK(c, hipSetDevice(c->dev));
    const u64 m = (u64)n_sites;
    ENS(c, c->in_b, m * 8); ENS(c, c->in_seq, m * (u64)len + 64);
    HIPCHK(c, hipMemcpyAsync(c->in_b.p, site, m * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_window, dim3(nblk(m, 256)), dim3(256), 0, c->stream, c->ix, c->in_b.as<u64>(), (long)m, len, c->in_seq.as<char>());
    HIPCHK(c, hipMemcpyAsync(out, c->in_seq.p, m * (u64)len, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BMBS_OK;
}

// the packed stage entries (bmbs_filter_batch_packed, bmbs_align_batch_packed): the uploaded rows c->in_seq packed on the device
// exactly as the mapping calls pack them (k_pack_rows: 2 bits per base + the not-ACGT plane and the per-row dirty byte)
static int pack_stage_rows(Lane* c, const ReadGeom& gm, int stride, u64 n_reads, PackedRows* pr)
{
    const int pwords = pack_words(gm.L), W = pack_base_words(gm.L);
    { int rz_ = ensure(c, c->prow, n_reads * (u64)pwords * 8 + 64, true); if (rz_) return rz_; } ENS(c, c->prow_dirty, n_reads + 64);
    HIPCHK(c, hipMemsetAsync(c->prow_dirty.p, 0, n_reads + 64, c->stream));
    hipLaunchKernelGGL(k_pack_rows, dim3(nblk(n_reads * (u64)(stride / 16), 256)), dim3(256), 0, c->stream, c->in_seq.as<char>(), gm, stride, (long)n_reads,
                       c->prow.as<u64>(), pwords, W, c->prow_dirty.as<u32>());
    pr->base = c->prow.as<u64>(); pr->dirty = c->prow_dirty.as<u8>(); pr->pwords = pwords; pr->W = W;
    return BMBS_OK;
}

static int lane_filter_batch(Lane* c, const char* seq, int32_t L, int32_t stride, int64_t n_reads,
                                 const uint32_t* read_of, const uint64_t* site, int64_t n_cand, uint32_t* err,
                                 int32_t* end_site, bool packed)
{
    if (!c) return BMBS_EINVAL;
    if (!c->attached) { c->err = "no index attached"; return BMBS_ESTATE; }
    HIPCHK(c, hipSetDevice(c->dev));
    if (n_cand <= 0) return BMBS_OK;
    if (L <= 0 || L > BMBS_MAX_READ || stride < L || n_reads < 0) { c->err = "bad read geometry"; return BMBS_EINVAL; }
    if (!seq || !read_of || !site || !err || !end_site) { c->err = "filter batch: NULL buffer"; return BMBS_EINVAL; }
    for (int64_t i = 0; i < n_cand; i++) if ((int64_t)read_of[i] >= n_reads) { c->err = "filter batch: read_of out of range"; return BMBS_EINVAL; }
    const u64 bytes = (u64)n_reads * stride, m = (u64)n_cand;
    { const int r0 = prepare_luts(c); if (r0) return r0; }
    ENS(c, c->in_a, m * 4); ENS(c, c->in_b, m * 8); ENS(c, c->ferr, m * 4); ENS(c, c->fend, m * 4);
    { int ds = 0; int r1 = upload_rows(c, c->in_seq, seq, L, stride, (u64)n_reads, &ds); if (r1) return r1; stride = ds; (void)bytes; }
    HIPCHK(c, hipMemcpyAsync(c->in_a.p, read_of, m * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->in_b.p, site, m * 8, hipMemcpyHostToDevice, c->stream));
    PackedRows pr = {nullptr, nullptr, 0, 0};
    const ReadGeom gm = geom(c, L, nullptr);
    // packed: the Myers form the mapping calls run (bpm_planes<W, true>)
    if (packed) { const int rp = pack_stage_rows(c, gm, stride, (u64)n_reads, &pr); if (rp) return rp; }
    hipLaunchKernelGGL(k_filter_pairs, dim3(nblk(m, 256)), dim3(256), 0, c->stream, c->ix, c->in_seq.as<char>(), pr, gm, stride, m,
                       c->in_a.as<u32>(), c->in_b.as<u64>(), c->ferr.as<u32>(), c->fend.as<int>());
    HIPCHK(c, hipMemcpyAsync(err, c->ferr.p, m * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(end_site, c->fend.p, m * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BMBS_OK;
}

static int lane_align_batch(Lane* c, const char* seq, const char* qual, int32_t L, int32_t stride, int64_t n_reads,
                                const uint32_t* read_of, const uint64_t* site, const int32_t* end_site_in,
                                const uint32_t* err_in, int64_t n_jobs, int32_t* start_site, int32_t* end_site,
                                uint32_t* nm, int32_t* score, uint32_t* cigar_ops, int32_t* n_ops, int32_t max_ops, bool packed, uint32_t rev_from)
{
    if (!c) return BMBS_EINVAL;
    if (!c->attached) { c->err = "no index attached"; return BMBS_ESTATE; }
    HIPCHK(c, hipSetDevice(c->dev));
    if (n_jobs <= 0) return BMBS_OK;
    if (L <= 0 || L > BMBS_MAX_READ || stride < L || n_reads < 0) { c->err = "bad read geometry"; return BMBS_EINVAL; }
    if (max_ops < cigar_ops_bound(c->prm, L, threshold_k(c->prm, L))) { c->err = "align batch: max_ops must be at least bmbs_max_cigar_ops(L)"; return BMBS_EINVAL; }
    for (int64_t i = 0; i < n_jobs; i++) if ((int64_t)read_of[i] >= n_reads) { c->err = "align batch: read_of out of range"; return BMBS_EINVAL; }
    const u64 bytes = (u64)n_reads * stride, m = (u64)n_jobs;
    { const int r0 = prepare_luts(c); if (r0) return r0; }
    ENS(c, c->in_a, m * 4); ENS(c, c->in_b, m * 8); ENS(c, c->in_c, m * 4); ENS(c, c->in_d, m * 4);
    ENS(c, c->cig_pool, m * (u64)max_ops * 4);
    {
        int ds = 0;
        int r1 = upload_rows(c, c->in_seq, seq, L, stride, (u64)n_reads, &ds); if (r1) return r1;
        r1 = upload_rows(c, c->in_qual, qual, L, stride, (u64)n_reads, &ds); if (r1) return r1;
        stride = ds; (void)bytes;
    }
    HIPCHK(c, hipMemcpyAsync(c->in_a.p, read_of, m * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->in_b.p, site, m * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->in_c.p, end_site_in, m * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->in_d.p, err_in, m * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->cig_pool.p, 0, m * (u64)max_ops * 4, c->stream));
    c->cur_slot = 0; c->prof_used[0] = 0;
    Jobs jobs = {c->in_a.as<u32>(), c->in_b.as<u64>(), c->in_c.as<int>(), c->in_d.as<u32>()};
    PackedRows pr = {nullptr, nullptr, 0, 0};                                        // the empty one: on the ASCII rows
    const ReadGeom gm = geom(c, L, nullptr);
    if (packed) { const int rp = pack_stage_rows(c, gm, stride, (u64)n_reads, &pr); if (rp) return rp; }
    int rc = run_align(c, c->in_seq.as<char>(), c->in_qual.as<char>(), nullptr, gm, stride, m, jobs, packed ? rev_from : 0xffffffffu, c->cig_pool.as<u32>(),
                       max_ops, pr, nullptr, ~0ull);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(start_site, c->a_start.p, m * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(end_site, c->a_end.p, m * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(nm, c->a_nm.p, m * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(score, c->a_score.p, m * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(n_ops, c->a_nops.p, m * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cigar_ops, c->cig_pool.p, m * (u64)max_ops * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c, 0);
    return BMBS_OK;
}

static int lane_seed_batch(Lane* c, const char* seq, int32_t L, int32_t stride, int64_t n_reads, uint8_t* verdict,
                               uint64_t* exit_site, uint64_t* seg_off, uint32_t* n_votes, uint64_t* vote_site,
                               uint32_t* vote_cnt, int64_t vote_cap, int64_t* total_slots)
{
    if (!c) return BMBS_EINVAL;
    if (!c->attached) { c->err = "no index attached"; return BMBS_ESTATE; }
    HIPCHK(c, hipSetDevice(c->dev));
    const u64 n = (u64)n_reads, bytes = n * (u64)stride;
    if (total_slots) *total_slots = 0;
    if (n == 0) return BMBS_OK;
    if (L <= 0 || L > BMBS_MAX_READ || stride < L || n_reads < 0) { c->err = "bad read geometry"; return BMBS_EINVAL; }
    { const int r0 = prepare_luts(c); if (r0) return r0; }
    c->cur_slot = 0; c->prof_used[0] = 0;
    int rc = per_read_workspace(c, n);
    if (rc) return rc;
    { int ds = 0; int r1 = upload_rows(c, c->in_seq, seq, L, stride, n, &ds); if (r1) return r1; stride = ds; (void)bytes; }
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, BMBS_SHARDS * BMBS_SHARD_WORDS * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(c->exit_site.p, 0, n * 8, c->stream));
    u64 tot = 0;
    rc = run_seed_stages(c, c->in_seq.as<char>(), geom(c, L, nullptr), stride, n, &tot, 0, true, false);
    if (rc) return rc;
    if (total_slots) *total_slots = (int64_t)tot;
    if ((u64)vote_cap < tot) { c->err = "vote buffers too small"; (void)hipStreamSynchronize(c->stream); return BMBS_ENOMEM; }
    HIPCHK(c, hipMemcpyAsync(verdict, c->verdict.p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(exit_site, c->exit_site.p, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(seg_off, c->cand_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(n_votes, c->n_votes.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    std::vector<bmbs_vote> hv(tot ? tot : 1);
    if (tot) HIPCHK(c, hipMemcpyAsync(hv.data(), c->votes.p, tot * sizeof(bmbs_vote), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (u64 i = 0; i < tot; i++) { vote_site[i] = hv[i].site; vote_cnt[i] = hv[i].vote; }
    return BMBS_OK;
}

// ------------------------------------------------------------------------------------------------
extern "C" int bmbs_stats_get(bmbs_ctx* X, int64_t stats[5])
{
    if (!X) return BMBS_EINVAL;
    { const int rc = settle_all(X); if (rc) return rc; }
    static_assert(sizeof(unsigned long long) == 8, "");
    for (int j = 0; j < 5; j++) stats[j] = 0;
    for (Lane* c : X->lanes) {
        uint64_t all[BMBS_SHARDS * BMBS_SHARD_WORDS];
        HIPCHK(c, hipSetDevice(c->dev));
        HIPCHK(c, hipMemcpy(all, c->stats.p, sizeof(all), hipMemcpyDeviceToHost));
        for (int j = 0; j < 5; j++) { uint64_t t = 0; for (int sdx = 0; sdx < BMBS_SHARDS; sdx++) t += all[sdx * BMBS_SHARD_WORDS + j]; stats[j] += (int64_t)t; }
    }
    return BMBS_OK;
}
extern "C" int bmbs_stats_reset(bmbs_ctx* X)
{
    if (!X) return BMBS_EINVAL;
    { const int rc = settle_all(X); if (rc) return rc; }
    for (Lane* c : X->lanes) {
        HIPCHK(c, hipSetDevice(c->dev));
        HIPCHK(c, hipMemsetAsync(c->stats.p, 0, BMBS_SHARDS * BMBS_SHARD_WORDS * 8, c->stream));
    }
    return BMBS_OK;
}
extern "C" int bmbs_stats_allreduce(bmbs_ctx** ctxs, int n, int64_t stats[5])
{
    for (int j = 0; j < 5; j++) stats[j] = 0;
    for (int i = 0; i < n; i++) {
        int64_t s[5];
        int rc = bmbs_stats_get(ctxs[i], s);
        if (rc) return rc;
        for (int j = 0; j < 5; j++) stats[j] += s[j];
    }
    return BMBS_OK;
}

// the kernels of the last mapping call, lane by lane (a split call has every kernel once per lane it ran on: the caller adds them up)
extern "C" int bmbs_profile_last(bmbs_ctx* X, const char** names, float* ms, int* n)
{
    if (!X || !n) return BMBS_EINVAL;
    { const int rc = settle_all(X); if (rc) return rc; }
    int cap = *n, cntp = 0;
    for (int li = 0; li < X->used_lanes && li < (int)X->lanes.size(); li++) {
        Lane* c = X->lanes[(size_t)li];
        for (size_t i = 0; i < c->last.size() && cntp < cap; i++) { names[cntp] = c->last[i].name; ms[cntp] = (float)c->last[i].ms; cntp++; }
    }
    *n = cntp;
    return BMBS_OK;
}

// sums over every mapping call settled since the last bmbs_profile_reset (all lanes): the bench reads per-kernel averages from
// here once per timed region instead of waiting for the device after every call
extern "C" int bmbs_profile_total(bmbs_ctx* X, const char** names, double* ms, int* n, int64_t* calls)
{
    if (!X || !n) return BMBS_EINVAL;
    { const int rc = settle_all(X); if (rc) return rc; }
    int cap = *n, cntp = 0;
    int64_t nc = 0;
    for (Lane* c : X->lanes) {
        nc += (int64_t)c->acc_calls;
        for (const auto& a : c->acc) {
            int at = -1;
            for (int j = 0; j < cntp; j++) if (!strcmp(names[j], a.name)) { at = j; break; }
            if (at < 0) { if (cntp >= cap) continue; at = cntp++; names[at] = a.name; ms[at] = 0; }
            ms[at] += a.ms;
        }
    }
    *n = cntp;
    if (calls) *calls = nc;
    return BMBS_OK;
}
extern "C" int bmbs_profile_reset(bmbs_ctx* X)
{
    if (!X) return BMBS_EINVAL;
    { const int rc = settle_all(X); if (rc) return rc; }
    for (Lane* c : X->lanes) { c->acc.clear(); c->acc_calls = 0; }
    return BMBS_OK;
}

extern "C" int bmbs_counters_last(bmbs_ctx* X, uint64_t out[8])
{
    uint64_t all[32];
    int rc = bmbs_counters_all(X, all);
    if (rc) return rc;
    for (int i = 0; i < 8; i++) out[i] = all[i];
    return BMBS_OK;
}

extern "C" int bmbs_counters_all(bmbs_ctx* X, uint64_t out[32])
{
    if (!X) return BMBS_EINVAL;
    { const int rc = settle_all(X); if (rc) return rc; }
    for (int j = 0; j < 32; j++) out[j] = 0;
    uint64_t cand = 0, jobs = 0;
    for (int li = 0; li < X->used_lanes && li < (int)X->lanes.size(); li++) {
        Lane* c = X->lanes[(size_t)li];
        uint64_t all[BMBS_SHARDS * BMBS_SHARD_WORDS];
        HIPCHK(c, hipSetDevice(c->dev));
        HIPCHK(c, hipMemcpy(all, c->counters.p, sizeof(all), hipMemcpyDeviceToHost));
        for (int j = 0; j < 32; j++) { uint64_t t = 0; for (int sdx = 0; sdx < BMBS_SHARDS; sdx++) t += all[sdx * BMBS_SHARD_WORDS + j]; out[j] += t; }
        cand += c->last_total_cand; jobs += c->last_n_jobs;
    }
    out[6] = cand;
    out[7] = jobs;
    return BMBS_OK;
}

// room for the work buffers of later calls, taken now (a lane's buffers are carved out of large slabs; the first slab costs a
// device-wide hipMalloc): a driver calls this while it loads, so that its first batches do not pay for it
extern "C" int bmbs_reserve(bmbs_ctx* X, uint64_t bytes_per_lane)
{
    if (!X) return BMBS_EINVAL;
    for (Lane* c : X->lanes) {
        HIPCHK(c, hipSetDevice(c->dev));
        size_t have = 0;
        for (const auto& sl : c->arena.slabs) have += sl.cap - sl.used;
        if (have >= bytes_per_lane) continue;
        const size_t cap = (size_t)bytes_per_lane;
        void* p = nullptr;
        if (hipMalloc(&p, cap) != hipSuccess) { X->err = "bmbs_reserve: out of device memory"; return BMBS_ENOMEM; }
        c->arena.slabs.push_back({(char*)p, cap, 0});
        c->arena.total += cap;
    }
    return BMBS_OK;
}

// first use of a page-locked buffer by the device is slow (the first 361 MB download into a fresh buffer took 44 ms instead of 7 on
// the MI355X boxes): a driver lets every staging buffer be touched once in each direction while it loads
extern "C" int bmbs_host_prefault(bmbs_ctx* X, void* p, uint64_t bytes, int32_t kind)
{
    Lane* c = lane0(X);
    if (!c || !p) return BMBS_EINVAL;
    HIPCHK(c, hipSetDevice(c->dev));
    const u64 piece = 64ull << 20;
    DevBuf tmp;
    void* d = nullptr;
    if (hipMalloc(&d, piece) != hipSuccess) return BMBS_ENOMEM;
    hipStream_t st = down_stream_of(c);
    hipError_t e = hipSuccess;
    for (u64 o = 0; o < bytes && e == hipSuccess; o += piece) {
        const u64 m = std::min(piece, bytes - o);
        if (kind != 2) e = hipMemcpyAsync(d, (char*)p + o, m, hipMemcpyHostToDevice, st);
        if (kind != 1 && e == hipSuccess) e = hipMemcpyAsync((char*)p + o, d, m, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(d);
    (void)tmp;
    return e == hipSuccess ? BMBS_OK : BMBS_ESTATE;
}

// diagnostic: calls that were issued again with exact sizes because a stage count did not fit the capacity learned so far
extern "C" int64_t bmbs_retries(bmbs_ctx* X)
{
    int64_t t = 0;
    if (X) for (Lane* c : X->lanes) t += (int64_t)c->n_retries;
    return t;
}

// ---- the stage entry points and the FASTQ-text calls run on lane 0 -----------------------------------------------------------
extern "C" int bmbs_index_attach(bmbs_ctx* X, const bmbs_index_view* v)
{
    Lane* c = lane0(X);
    if (!c) return BMBS_EINVAL;
    const int rc = lane_index_attach(c, v);
    if (rc) return fin(X, c, rc);
    for (size_t i = 1; i < X->lanes.size(); i++) { Lane* o = X->lanes[i]; o->ix = c->ix; o->rows = c->rows; o->o3 = c->o3; o->attached = true; }
    return BMBS_OK;
}
extern "C" int bmbs_locate_batch(bmbs_ctx* X, const uint64_t* row, int64_t n_rows, uint64_t* pos) { ON_LANE0(lane_locate_batch(c, row, n_rows, pos)); }
extern "C" int bmbs_vote_order_batch(bmbs_ctx* X, const uint8_t* vote, const int64_t* seg_off, int64_t n_seg, int32_t form, uint32_t* perm)
{ ON_LANE0(lane_vote_order_batch(c, vote, seg_off, n_seg, form, perm)); }
extern "C" int bmbs_window_batch(bmbs_ctx* X, const uint64_t* site, int64_t n_sites, int32_t len, char* out) { ON_LANE0(lane_window_batch(c, site, n_sites, len, out)); }
extern "C" int bmbs_filter_batch(bmbs_ctx* X, const char* seq, int32_t L, int32_t stride, int64_t n_reads, const uint32_t* read_of, const uint64_t* site,
                                 int64_t n_cand, uint32_t* err, int32_t* end_site)
{ ON_LANE0(lane_filter_batch(c, seq, L, stride, n_reads, read_of, site, n_cand, err, end_site, false)); }
extern "C" int bmbs_filter_batch_packed(bmbs_ctx* X, const char* seq, int32_t L, int32_t stride, int64_t n_reads, const uint32_t* read_of, const uint64_t* site,
                                        int64_t n_cand, uint32_t* err, int32_t* end_site)
{ ON_LANE0(lane_filter_batch(c, seq, L, stride, n_reads, read_of, site, n_cand, err, end_site, true)); }
extern "C" int bmbs_align_batch(bmbs_ctx* X, const char* seq, const char* qual, int32_t L, int32_t stride, int64_t n_reads, const uint32_t* read_of,
                                const uint64_t* site, const int32_t* end_site_in, const uint32_t* err_in, int64_t n_jobs, int32_t* start_site,
                                int32_t* end_site, uint32_t* nm, int32_t* score, uint32_t* cigar_ops, int32_t* n_ops, int32_t max_ops)
{ ON_LANE0(lane_align_batch(c, seq, qual, L, stride, n_reads, read_of, site, end_site_in, err_in, n_jobs, start_site, end_site, nm, score, cigar_ops, n_ops, max_ops, false, 0xffffffffu)); }
extern "C" int bmbs_align_batch_packed(bmbs_ctx* X, const char* seq, const char* qual, int32_t L, int32_t stride, int64_t n_reads, const uint32_t* read_of,
                                       const uint64_t* site, const int32_t* end_site_in, const uint32_t* err_in, int64_t n_jobs, int32_t* start_site,
                                       int32_t* end_site, uint32_t* nm, int32_t* score, uint32_t* cigar_ops, int32_t* n_ops, int32_t max_ops, uint32_t rev_from)
{ ON_LANE0(lane_align_batch(c, seq, qual, L, stride, n_reads, read_of, site, end_site_in, err_in, n_jobs, start_site, end_site, nm, score, cigar_ops, n_ops, max_ops, true, rev_from)); }
extern "C" int bmbs_seed_batch(bmbs_ctx* X, const char* seq, int32_t L, int32_t stride, int64_t n_reads, uint8_t* verdict, uint64_t* exit_site,
                               uint64_t* seg_off, uint32_t* n_votes, uint64_t* vote_site, uint32_t* vote_cnt, int64_t vote_cap, int64_t* total_slots)
{ ON_LANE0(lane_seed_batch(c, seq, L, stride, n_reads, verdict, exit_site, seg_off, n_votes, vote_site, vote_cnt, vote_cap, total_slots)); }

// BMBS_HOST_INTERLEAVE=1: the pages of page-locked buffers are spread over all NUMA nodes of the host (set_mempolicy around the
// allocation): a file-to-file run moves ~1.3 KB per read through host memory, and one node of a 4-nodes-per-socket host has a
// quarter of the socket's bandwidth
static long set_policy_interleave(bool on)
{
#ifdef SYS_set_mempolicy
    unsigned long mask[16];
    memset(mask, 0, sizeof mask);
    int nodes = 0;
    if (FILE* f = fopen("/sys/devices/system/node/online", "r")) {
        int a = 0, b = 0;
        const int k = fscanf(f, "%d-%d", &a, &b);
        fclose(f);
        nodes = k == 2 ? b + 1 : 1;
    }
    if (nodes < 2) return -1;
    for (int i = 0; i < nodes && i < 1024; i++) mask[i / (8 * sizeof(long))] |= 1ul << (i % (8 * sizeof(long)));
    return syscall(SYS_set_mempolicy, on ? 3 /* MPOL_INTERLEAVE */ : 0 /* MPOL_DEFAULT */, on ? mask : nullptr, on ? (unsigned long)(nodes + 1) : 0ul);
#else
    (void)on; return -1;
#endif
}
static void* host_alloc_flags(uint64_t bytes, unsigned extra);
extern "C" void* bmbs_host_alloc(uint64_t bytes) { return host_alloc_flags(bytes, 0); }
// kind 1: written by the host, read by the device (FASTQ windows); kind 2: written by the device, read by the host (SAM text).
// The HIP flags of either kind can be set from the environment for experiments (BMBS_PIN_IN_FLAGS / BMBS_PIN_OUT_FLAGS, numeric:
// 0x40000000 hipHostMallocNonCoherent, 0x4 hipHostMallocWriteCombined)
extern "C" void* bmbs_host_alloc_kind(uint64_t bytes, int32_t kind)
{
    static const unsigned in_flags = [] { const char* e = getenv("BMBS_PIN_IN_FLAGS"); return e ? (unsigned)strtoul(e, nullptr, 0) : 0u; }();
    static const unsigned out_flags = [] { const char* e = getenv("BMBS_PIN_OUT_FLAGS"); return e ? (unsigned)strtoul(e, nullptr, 0) : 0u; }();
    return host_alloc_flags(bytes, kind == 1 ? in_flags : kind == 2 ? out_flags : 0u);
}
static void* host_alloc_flags(uint64_t bytes, unsigned extra)
{
    static const bool interleave = [] { const char* e = getenv("BMBS_HOST_INTERLEAVE"); return e && !strcmp(e, "1"); }();
    void* p = nullptr;
    unsigned flags = hipHostMallocPortable | extra;                           // portable: contexts on several devices copy from it
    bool pol = false;
    if (interleave && set_policy_interleave(true) == 0) { pol = true; flags |= hipHostMallocNumaUser; }
    const hipError_t e = hipHostMalloc(&p, bytes ? bytes : 16, flags);
    if (pol) (void)set_policy_interleave(false);
    if (e != hipSuccess) return nullptr;
    return p;
}
extern "C" void bmbs_host_free(void* p) { if (p) (void)hipHostFree(p); }
