// bitmapperbs_amd/csrc/k_bai.hip -- the pieces of a .bai index (SAM specification section 5.2) of the records bmbs_bam_sort has just sorted and
// deflated (bmbs_bam_sort_index).  The sorted records (bs_sorted), their offsets in the uncompressed stream (bs_soff) and the compressed
// offset of every BGZF block (bam_off) are still on the device; what goes back over the link is a few kilobytes.
//   k_bai_records    record j -> rb[j] = refID << 16 | bin, rw[j] = first window | last window << 15 | mapped << 30; per-reference counts
//   k_bai_heads      rb[j] against rb[j - 1]: run heads counted per wave (ballot + popcount), window candidates counted per record, the
//                    first record of every reference and the record behind its last
//   k_bai_emit       head j -> its place in the list of heads (scan of the wave counts + rank in the wave); window candidates (key, j)
//   k_bai_chunks     head i -> (ref << 16 | bin, i), virtual offsets of the run's first record and of the next head
//   (pair sort)      stable, by ref << 16 | bin: chunks of one bin stay in file order
//   k_bai_chunk_out  the sorted chunks as bmbs_bai_chunk
//   (pair sort)      the window candidates, stable, by ref << 15 | window: the first of a key is the record with the smallest offset
//   k_bai_win_flag / k_bai_win_out   the first candidate of every key as bmbs_bai_win
//   k_bai_ref_out    the references that have records as bmbs_bai_ref
// Windows: the records are sorted by position, so a mapped record can hold the minimum of its START window only when its predecessor
// is not a mapped record of the same reference with the same start window; it is a candidate for every further window it reaches
// into.  Reads of a few hundred bases give about one candidate per 16 kb of covered genome -- no table over the references' lengths
// (which the call does not know).
#ifndef K_BAI_HIP
#define K_BAI_HIP

#define BAI_NOCOOR  (~0ull)               // rb of a record with refID -1
#define BAI_MAX_END (1u << 29)            // BAI: 5 levels of bins below 2^29

struct BaiVoff { const u64* soff; const u64* bam_off; u64 total, nb; };
// virtual offset of sorted record j's first byte (j = n: the first byte behind the call), relative to the call's first block
DEVI u64 bai_voff(const BaiVoff& v, u64 j)
{
    const u64 u = v.soff[j];
    if (u >= v.total) return v.bam_off[v.nb] << 16;
    return (v.bam_off[u / BGZF_IN] << 16) | (u % BGZF_IN);
}

DEVI u32 bai_reg2bin(u32 beg, u32 end)
{
    --end;
    if (beg >> 14 == end >> 14) return 4681u + (beg >> 14);
    if (beg >> 17 == end >> 17) return 585u + (beg >> 17);
    if (beg >> 20 == end >> 20) return 73u + (beg >> 20);
    if (beg >> 23 == end >> 23) return 9u + (beg >> 23);
    if (beg >> 26 == end >> 26) return 1u + (beg >> 26);
    return 0u;
}

// info[0] = ~(the first record that ends behind 2^29), info[1] = ~(the first record whose read name and CIGAR do not fit its length)
// (0: none), info[2] = records with refID -1.  cnt[2 r] / cnt[2 r + 1] = mapped / unmapped records of reference r (r < n_ref).
__global__ void __launch_bounds__(256)
k_bai_records(const char* __restrict__ rec, const u64* __restrict__ soff, long n, u32 n_ref, u64* __restrict__ rb, u32* __restrict__ rw, u32* __restrict__ cnt,
              u32* __restrict__ info)
{
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = j < n;
    u32 far = 0, bad = 0, ref = 0xffffffffu, mapped = 0;
    if (active) {
        const u64 so = soff[j];
        const char* p = rec + so;
        const u64 len = soff[j + 1] - so;
        ref = bs_ld32(p + 4);
        const int pos = (int)bs_ld32(p + 8);
        const u32 l_name = (u32)(unsigned char)p[12];
        u32 n_cig = (u32)(unsigned char)p[16] | ((u32)(unsigned char)p[17] << 8);
        const u32 flag = (u32)(unsigned char)p[18] | ((u32)(unsigned char)p[19] << 8);
        u64 b = BAI_NOCOOR; u32 w = 0;
        if (ref != 0xffffffffu) {
            if (36ull + l_name + 4ull * n_cig > len) { bad = ~(u32)j; n_cig = 0; }       // (nothing is read behind the record)
            mapped = (flag & 4u) ? 0u : 1u;
            u64 rl = 0;
            if (mapped) {
                const char* q = p + 36 + l_name;
                for (u32 k = 0; k < n_cig; k++) {
                    const u32 c = bs_ld32(q + 4 * k);
                    if ((0x18du >> (c & 15u)) & 1u) rl += c >> 4;                         // M D N = X consume reference
                }
            }
            const u64 beg = pos < 0 ? 0 : (u64)pos, end = beg + (rl ? rl : 1);
            if (end > BAI_MAX_END) { far = ~(u32)j; b = (u64)ref << 16; }
            else {
                b = ((u64)ref << 16) | bai_reg2bin((u32)beg, (u32)end);
                w = (u32)(beg >> 14) | ((u32)((end - 1) >> 14) << 15) | (mapped << 30);
            }
        }
        rb[j] = b; rw[j] = w;
    }
    for (int d = 32; d; d >>= 1) {
        const u32 f = (u32)__shfl_xor((int)far, d), g = (u32)__shfl_xor((int)bad, d);
        far = far > f ? far : f; bad = bad > g ? bad : g;
    }
    const int lane = threadIdx.x & 63;
    if (lane == 0) { if (far) atomicMax(&info[0], far); if (bad) atomicMax(&info[1], bad); }
    // the counts: one atomic per wave, reference in it (the records are sorted: mostly one) and word
    u64 pend = __ballot(active);
    while (pend) {
        const int lead = __ffsll((long long)pend) - 1;
        const u32 r = (u32)__shfl((int)ref, lead);
        const u64 same = __ballot(active && ref == r);
        const u32 nt = (u32)__popcll(same), nm = (u32)__popcll(__ballot(active && ref == r && mapped));
        if (lane == lead) {
            if (r == 0xffffffffu) atomicAdd(&info[2], nt);
            else if (r < n_ref) { if (nm) atomicAdd(&cnt[2 * (u64)r], nm); if (nt - nm) atomicAdd(&cnt[2 * (u64)r + 1], nt - nm); }
        }
        pend &= ~same;
    }
}

// is record j (rb / rw = b / w; its predecessor's: pb / pw) a candidate for its start window?
DEVI bool bai_start_cand(long j, u64 b, u32 w, u64 pb, u32 pw)
{
    return j == 0 || (pb >> 16) != (b >> 16) || !((pw >> 30) & 1u) || (pw & 0x7fffu) != (w & 0x7fffu);
}
DEVI u32 bai_n_cand(long j, u64 b, u32 w, u64 pb, u32 pw)
{
    if (b == BAI_NOCOOR || !((w >> 30) & 1u)) return 0;
    return (bai_start_cand(j, b, w, pb, pw) ? 1u : 0u) + (((w >> 15) & 0x7fffu) - (w & 0x7fffu));
}

// wave_heads[v] = run heads among the records of wave v (the first record with refID -1 counts as one: it ends the last run);
// wc[j] = window candidates of record j; has[r] = 1, first[r] / last[r] = the first record of reference r / the record behind its last
__global__ void __launch_bounds__(256)
k_bai_heads(const u64* __restrict__ rb, const u32* __restrict__ rw, long n, u32 n_ref, u32* __restrict__ wave_heads, u32* __restrict__ wc, u32* __restrict__ has,
            u32* __restrict__ first, u32* __restrict__ last)
{
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = j < n;
    bool head = false;
    if (active) {
        const u64 b = rb[j], pb = j ? rb[j - 1] : 0;
        const u32 w = rw[j], pw = j ? rw[j - 1] : 0;
        head = j == 0 || b != pb;
        wc[j] = bai_n_cand(j, b, w, pb, pw);
        const u64 r = b >> 16, pr = pb >> 16;
        if (j == 0 || r != pr) {
            if (b != BAI_NOCOOR && r < n_ref) { first[r] = (u32)j; has[r] = 1u; }
            if (j && pr < n_ref) last[pr] = (u32)j;
        }
        if (j == n - 1 && b != BAI_NOCOOR && r < n_ref) last[r] = (u32)n;
    }
    const u64 hm = __ballot(head);
    if ((threadIdx.x & 63) == 0 && active) wave_heads[j >> 6] = (u32)__popcll(hm);
}

// hj[] = the run heads' record numbers, in order; the window candidates of record j at woff[j]
__global__ void __launch_bounds__(256)
k_bai_emit(const u64* __restrict__ rb, const u32* __restrict__ rw, long n, const u64* __restrict__ hoff, const u64* __restrict__ woff, u32* __restrict__ hj,
           u64* __restrict__ wkey, u32* __restrict__ wval)
{
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = j < n;
    bool head = false;
    u64 b = 0, pb = 0; u32 w = 0, pw = 0;
    if (active) {
        b = rb[j]; w = rw[j];
        if (j) { pb = rb[j - 1]; pw = rw[j - 1]; }
        head = j == 0 || b != pb;
    }
    const u64 hm = __ballot(head);
    const int lane = threadIdx.x & 63;
    if (head) hj[hoff[j >> 6] + (u64)__popcll(hm & ((1ull << lane) - 1ull))] = (u32)j;
    if (active && bai_n_cand(j, b, w, pb, pw)) {
        u64 at = woff[j];
        const u64 r = (b >> 16) << 15;
        const u32 w0 = w & 0x7fffu, w1 = (w >> 15) & 0x7fffu;
        if (bai_start_cand(j, b, w, pb, pw)) { wkey[at] = r | w0; wval[at] = (u32)j; at++; }
        for (u32 x = w0 + 1; x <= w1; x++, at++) { wkey[at] = r | x; wval[at] = (u32)j; }
    }
}

// chunk i = the run from head i to the next head (or the call's end); be[2 i], be[2 i + 1] = its virtual offsets
__global__ void __launch_bounds__(256)
k_bai_chunks(const u32* __restrict__ hj, long m, long n, const u64* __restrict__ rb, BaiVoff v, u64* __restrict__ ckey, u32* __restrict__ cidx, u64* __restrict__ be)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const u64 j = hj[i], jn = i + 1 < m ? (u64)hj[i + 1] : (u64)n;
    ckey[i] = rb[j]; cidx[i] = (u32)i;
    be[2 * i] = bai_voff(v, j); be[2 * i + 1] = bai_voff(v, jn);
}

__global__ void __launch_bounds__(256)
k_bai_chunk_out(const u64* __restrict__ ckey, const u32* __restrict__ cidx, const u64* __restrict__ be, long m, bmbs_bai_chunk* __restrict__ out)
{
    const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= m) return;
    const u64 k = ckey[s]; const u64 i = cidx[s];
    bmbs_bai_chunk c;
    c.ref = (int32_t)(u32)(k >> 16); c.bin = (u32)(k & 0xffffu); c.beg = be[2 * i]; c.end = be[2 * i + 1];
    out[s] = c;
}

__global__ void __launch_bounds__(256)
k_bai_win_flag(const u64* __restrict__ wkey, long t_n, u32* __restrict__ flag)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < t_n) flag[t] = (t == 0 || wkey[t] != wkey[t - 1]) ? 1u : 0u;
}

// list[] = the first candidate of every (ref, window), *n_list of them (a count the scan in front of this kernel left on the device)
__global__ void __launch_bounds__(256)
k_bai_win_out(const u32* __restrict__ list, const u64* __restrict__ n_list, const u64* __restrict__ wkey, const u32* __restrict__ wval, BaiVoff v, bmbs_bai_win* __restrict__ out)
{
    const u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= *n_list) return;
    const u32 t = list[s];
    const u64 k = wkey[t];
    bmbs_bai_win o;
    o.ref = (int32_t)(u32)(k >> 15); o.win = (u32)(k & 0x7fffu); o.off = bai_voff(v, wval[t]);
    out[s] = o;
}

__global__ void __launch_bounds__(256)
k_bai_ref_out(const u32* __restrict__ list, long n_list, const u32* __restrict__ first, const u32* __restrict__ last, const u32* __restrict__ cnt, BaiVoff v,
              bmbs_bai_ref* __restrict__ out)
{
    const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_list) return;
    const u32 r = list[s];
    bmbs_bai_ref o;
    o.ref = (int32_t)r; o.pad = 0; o.beg = bai_voff(v, first[r]); o.end = bai_voff(v, last[r]);
    o.n_mapped = cnt[2 * (u64)r]; o.n_unmapped = cnt[2 * (u64)r + 1];
    out[s] = o;
}
#endif
