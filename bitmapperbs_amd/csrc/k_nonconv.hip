// bitmapperbs_amd/csrc/k_nonconv.hip -- reads the bisulfite treatment did not convert, found on the device (`--bam --sort
// --filter-non-conversion`, bmbs_bam_nonconv, bmbs_text_sorted_nonconv).  The rule is in include/bmbs.h; tests/nonconv_spec.py restates it.
//
// Record i = len[i] bytes at raw + off[i] (len 0: no record), the layout of k_methyl.hip.  A record is EXAMINED when it is mapped with a
// CIGAR and neither secondary nor supplementary; its CALLS are those of k_meth_events without a clip, a trim, a MAPQ bound or the
// proper-pair rule, in all three contexts.  nm / nu = its methylated / unmethylated calls outside CpG decide whether it FAILS; a template
// (one entry, or entries 2p and 2p + 1) fails when one of its records does.
//   k_nonconv_walk    a group of METH_GROUP lanes per record: checks it, counts its calls by context, decides the record and -- where the
//                     two records of a pair are neighbouring groups of one wave -- the template; tallies the calls of all examined
//                     records by (strand, context, methylated) and the failed templates in the block's LDS, 64 bits a counter
//   k_nonconv_order   the verdict of the template of every record of a sorted text call, in sorted order
// The walk is the THIRD copy of k_meth_events' (k_methyl.hip; k_meth_mbias holds the second): a change to the record checks or to the
// walk there has to be made here too.  Every store is an ordinary vector store, every add an atomicAdd of plain C++; there is no inline
// assembly.
#ifndef K_NONCONV_HIP
#define K_NONCONV_HIP

#define NONCONV_TALLY 13                  // 12 totals, [2 strand][3 context][2 (unmethylated, methylated)], and the failed templates

struct NonconvPar { u32 threshold, percent, min_count, min_phred; int n_chrom; };

// nm methylated and nu unmethylated calls outside CpG: does the record fail?  (64-bit: 100 * nm does not fit 32 bits for every record)
DEVI bool nonconv_fails(u32 nm, u32 nu, const NonconvPar& par)
{
    if (par.threshold && nm >= par.threshold) return true;
    const u64 all = (u64)nm + nu;
    return par.percent && all >= par.min_count && 100ull * nm >= (u64)par.percent * all;
}

// info[0..3]: the four refusal words of k_meth_events, for the same reasons.  Nothing is read behind a record.
// count (or NULL): count[i] = the (methylated, unmethylated) calls outside CpG of entry i, 0, 0 when it is not examined.
// fail[t] = 1 when template t fails, else 0: t = i, or with `paired` i / 2 for the entries i and i + 1 (n is even then).
// tally[NONCONV_TALLY] (global, zeroed by the caller): += the calls of every examined record, += the failed templates.
// A fixed grid strides over the records, 256 / METH_GROUP of them per block and step: an even number, and the stride is even too, so the
// two records of a pair are always the groups 2 g and 2 g + 1 of one wave -- lanes that differ in bit METH_GROUP only.  Each block
// tallies in LDS and adds its non-zero counters to the global table once, when it is through.  Integer adds: the table does not depend
// on their order.
__global__ void __launch_bounds__(256)
k_nonconv_walk(const u64* __restrict__ gen2p, const u64* __restrict__ chrom_start, const char* __restrict__ raw, const u64* __restrict__ off,
               const u32* __restrict__ len, long n, int paired, NonconvPar par, bmbs_nonconv_count* __restrict__ count, uint8_t* __restrict__ fail,
               unsigned long long* __restrict__ tally, u32* __restrict__ info)
{
    static_assert(METH_GROUP == 16 && 256 % (2 * METH_GROUP) == 0, "a pair's two groups share a wave");
    __shared__ unsigned long long block_tally[NONCONV_TALLY];
    if (threadIdx.x < NONCONV_TALLY) block_tally[threadIdx.x] = 0;
    __syncthreads();
    const int gl = threadIdx.x % METH_GROUP;
    const long per_block = 256 / METH_GROUP, step = (long)gridDim.x * per_block;
    for (long first = (long)blockIdx.x * per_block; first < n; first += step) {          // (uniform within the block)
        const long i = first + threadIdx.x / METH_GROUP;
        bool live = i < n;
        const u32 l = live ? len[i] : 0;
        if (l == 0) live = false;
        if (live && l < 36) { if (gl == 0) atomicMax(&info[0], ~(u32)i); live = false; }
        const char* const p = raw + (live ? off[i] : 0);
        if (live && bs_ld32(p) + 4u != l) { if (gl == 0) atomicMax(&info[0], ~(u32)i); live = false; }
        int ref = -1, pos = 0;
        u32 l_name = 0, n_cig = 0, flag = 4, l_seq = 0;
        if (live) {
            ref = (int)bs_ld32(p + 4); pos = (int)bs_ld32(p + 8);
            l_name = (u32)(unsigned char)p[12];
            n_cig = (u32)(unsigned char)p[16] | ((u32)(unsigned char)p[17] << 8);
            flag = (u32)(unsigned char)p[18] | ((u32)(unsigned char)p[19] << 8);
            l_seq = bs_ld32(p + 20);
            if (36ull + l_name + 4ull * n_cig + ((u64)l_seq + 1) / 2 + l_seq > (u64)l) { if (gl == 0) atomicMax(&info[1], ~(u32)i); live = false; }
        }
        if (live && ref >= par.n_chrom) { if (gl == 0) atomicMax(&info[2], ~(u32)i); live = false; }
        const bool mapped = live && ref >= 0 && !(flag & 4u) && n_cig > 0;
        const char* const cg = p + 36 + l_name;
        // the reference span, the lanes' shares added up within the group (every lane of the wave takes part)
        u64 span = 0;
        if (mapped)
            for (u32 k = (u32)gl; k < n_cig; k += METH_GROUP) { const u32 c = bs_ld32(cg + 4 * (u64)k); if ((0x18du >> (c & 15u)) & 1u) span += c >> 4; }
        for (int d = METH_GROUP / 2; d; d >>= 1) {
            const u32 lo = (u32)__shfl_xor((int)(u32)span, d), hi = (u32)__shfl_xor((int)(u32)(span >> 32), d);
            span += ((u64)hi << 32) | lo;
        }
        long s_lo = 0, s_hi = 0;
        bool examined = mapped;
        if (mapped) {
            s_lo = (long)chrom_start[ref]; s_hi = (long)chrom_start[ref + 1];
            if (pos < 0 || (u64)pos + span > (u64)(s_hi - s_lo)) { if (gl == 0) atomicMax(&info[3], ~(u32)i); examined = false; }
        }
        examined = examined && !(flag & 0x900u);                                // secondary and supplementary records are not looked at
        // paired: read 1 reverse or read 2 forward is OB; single: reverse is OB
        const bool ob = (flag & 1u) ? (((flag & 0x40u) && (flag & 0x10u)) || ((flag & 0x80u) && !(flag & 0x10u))) : (flag & 0x10u) != 0;
        const long a0 = s_lo + pos, a1 = a0 + (long)span;                       // the span in genome coordinates
        const bool all_m = examined && n_cig == 1 && ((0x181u >> (bs_ld32(cg) & 15u)) & 1u);      // one M, = or X: a constant shift
        const char* const sq = cg + 4 * (u64)n_cig;
        const char* const ql = sq + ((u64)l_seq + 1) / 2;
        const u32 want_m = ob ? 4u : 2u, want_u = ob ? 1u : 8u;                 // G / A for OB, C / T for OT (BAM's 4-bit codes)
        const long W0 = a0 >> 5, W1 = examined && span ? (a1 - 1) >> 5 : W0 - 1;
        u32 cu[3] = {0, 0, 0}, cm[3] = {0, 0, 0};                               // this lane's unmethylated / methylated calls by context
        for (long W = W0 + gl; W <= W1; W += METH_GROUP) {
            u32 m[6];
            meth_masks(gen2p, W, s_lo, s_hi, m);
            const u32 in = (u32)meth_range(32 * W, a0, a1, 32);
            const u32 m0 = m[ob ? 3 : 0] & in, m1 = m[ob ? 4 : 1] & in, m2 = m[ob ? 5 : 2] & in;
            u32 sel = m0 | m1 | m2;
            // the read base against each position that is left: bits ascend, so the CIGAR is walked once per word
            u32 mb = 0, ub = 0;
            u32 k = 0; long r_at = 0, i_at = 0;
            while (sel) {
                const int b = __ffs((int)sel) - 1;
                sel &= sel - 1;
                const long ro = 32 * W + b - a0;                                 // offset in the record's reference span
                long ri = -1;
                if (all_m) ri = ro;
                else {
                    while (k < n_cig) {
                        const u32 c = bs_ld32(cg + 4 * (u64)k);
                        const u32 op = c & 15u; const long ln = (long)(c >> 4);
                        const bool on_ref = (0x18du >> op) & 1u, on_read = (0x193u >> op) & 1u;      // M D N = X / M I S = X
                        if (on_ref && ro < r_at + ln) { if (on_read) ri = i_at + (ro - r_at); break; }
                        if (on_ref) r_at += ln;
                        if (on_read) i_at += ln;
                        k++;
                    }
                }
                if (ri < 0 || ri >= (long)l_seq) continue;
                const u32 q = (u32)(unsigned char)ql[ri];
                if ((q == 255u ? 0u : q) < par.min_phred) continue;
                const u32 by = (u32)(unsigned char)sq[ri >> 1];
                const u32 code = (ri & 1) ? (by & 15u) : (by >> 4);
                if (code == want_m) mb |= 1u << b;
                else if (code == want_u) ub |= 1u << b;
            }
            cm[0] += (u32)__popc(mb & m0); cm[1] += (u32)__popc(mb & m1); cm[2] += (u32)__popc(mb & m2);
            cu[0] += (u32)__popc(ub & m0); cu[1] += (u32)__popc(ub & m1); cu[2] += (u32)__popc(ub & m2);
        }
        // the record's six counts: the lanes' added up within the group (a record has fewer calls than bases: 32 bits hold them)
#pragma unroll
        for (int x = 0; x < 3; x++)
            for (int d = METH_GROUP / 2; d; d >>= 1) { cm[x] += (u32)__shfl_xor((int)cm[x], d); cu[x] += (u32)__shfl_xor((int)cu[x], d); }
        const u32 nm = cm[1] + cm[2], nu = cu[1] + cu[2];
        const bool rec_fails = examined && nonconv_fails(nm, nu, par);
        // the other record of the pair: the same lane of the neighbouring group (single end: not looked at)
        const bool mate_fails = __shfl_xor((int)rec_fails, METH_GROUP) != 0;
        if (gl == 0 && i < n) {
            if (count) { bmbs_nonconv_count c; c.meth = nm; c.unmeth = nu; count[i] = c; }
            if (examined) {
#pragma unroll
                for (int x = 0; x < 3; x++) {
                    if (cu[x]) atomicAdd(&block_tally[((ob ? 3 : 0) + x) * 2], (unsigned long long)cu[x]);
                    if (cm[x]) atomicAdd(&block_tally[((ob ? 3 : 0) + x) * 2 + 1], (unsigned long long)cm[x]);
                }
            }
            const bool tmpl_fails = rec_fails || (paired && mate_fails);
            if (!paired || !(i & 1)) {
                fail[paired ? i >> 1 : i] = tmpl_fails ? 1 : 0;
                if (tmpl_fails) atomicAdd(&block_tally[12], 1ull);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < NONCONV_TALLY) { const unsigned long long v = block_tally[threadIdx.x]; if (v) atomicAdd(&tally[threadIdx.x], v); }
}

// out[j] = the verdict of the template of the j-th record of a sorted text call (idx[j] = its output line; lines 2p and 2p + 1 are the
// records of pair p: shift 1, else 0)
__global__ void __launch_bounds__(256)
k_nonconv_order(const uint8_t* __restrict__ fail, const u32* __restrict__ idx, long n, int shift, uint8_t* __restrict__ out)
{
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[j] = fail[idx[j] >> shift];
}
#endif
