// bitmapperbs_amd/csrc/k_bamsort.hip -- coordinate sort of BAM records on the device (`--bam --sort`, bmbs_bam_sort).
//
// The records of a batch sit one behind the other in device memory, record i at off[i] (the exclusive scan of the record lengths).
//   k_bam_keys    record -> key[i] = refID << 32 | (pos + 1) << 1 | reverse-strand bit (include/bmbs.h), idx[i] = i; checks the lengths
//   (pair sort)   rocPRIM radix_sort_pairs over (key, idx): an LSD radix sort, stable, over the key bits that can be set only
//   k_bam_slen    the lengths in sorted order (their scan = where every record goes)
//   k_bam_gather  the records into sorted order: the one kernel here that moves the records themselves (twice their bytes)
// Deflation of the sorted stream is k_bgzf_block / k_bgzf_gather (bmbs_bam.hip), unchanged.
#ifndef K_BAMSORT_HIP
#define K_BAMSORT_HIP
#include <rocprim/device/device_radix_sort.hpp>

DEVI u32 bs_ld32(const char* p)
{
    return (u32)(unsigned char)p[0] | ((u32)(unsigned char)p[1] << 8) | ((u32)(unsigned char)p[2] << 16) | ((u32)(unsigned char)p[3] << 24);
}

// info[0] = ~(the first record whose length is below 36 or is not its block_size + 4) (0: none), info[1] = the largest refID other than
// -1, info[2] = entries of length 0.  skip_empty (the text calls: output lines that print nothing have length 0): such an entry is no
// record, gets the all-ones key -- behind every real key, the unmapped records' included -- and is counted, not reported.
__global__ void __launch_bounds__(256)
k_bam_keys(const char* __restrict__ raw, const u64* __restrict__ off, const u32* __restrict__ len, long n, int skip_empty, u64* __restrict__ key,
           u32* __restrict__ idx, u32* __restrict__ info)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    u32 bad = 0, ref_max = 0, empty = 0;
    if (i < n) {
        const u32 l = len[i];
        u64 k = ~0ull;
        if (l == 0 && skip_empty) empty = 1;
        else if (l < 36) bad = ~(u32)i;
        else {
            const char* p = raw + off[i];
            if (bs_ld32(p) + 4u != l) bad = ~(u32)i;
            const u32 ref = bs_ld32(p + 4), pos1 = bs_ld32(p + 8) + 1u;
            const u32 flag = (u32)(unsigned char)p[18] | ((u32)(unsigned char)p[19] << 8);
            k = ((u64)ref << 32) | ((u64)pos1 << 1) | (u64)((flag >> 4) & 1u);
            if (ref != 0xffffffffu) ref_max = ref;
        }
        key[i] = k; idx[i] = (u32)i;
    }
    // one atomic per wave and word
    for (int d = 32; d; d >>= 1) {
        const u32 b = (u32)__shfl_xor((int)bad, d), r = (u32)__shfl_xor((int)ref_max, d);
        bad = bad > b ? bad : b; ref_max = ref_max > r ? ref_max : r;
    }
    const u32 n_empty = (u32)__popcll(__ballot(empty));
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicMax(&info[0], bad);
        if (ref_max) atomicMax(&info[1], ref_max);
        if (n_empty) atomicAdd(&info[2], n_empty);
    }
}

__global__ void __launch_bounds__(256)
k_bam_slen(const u32* __restrict__ len, const u32* __restrict__ idx, long n, u32* __restrict__ slen)
{
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) slen[j] = len[idx[j]];
}

// ---- the records into sorted order: one workgroup per piece of the output ------------------------------------------------------------
// k_line_write's scheme with scattered sources.  A workgroup owns `rpb` consecutive OUTPUT records = one contiguous piece of the output,
// soff[r0] .. soff[r0 + nr) (soff: the scan of the sorted lengths).  Output record j is input record idx[j]; source and destination
// start at arbitrary bytes.
//   1. 16 lanes per record pull it with 16-byte loads at SOURCE alignment and write it into the LDS image of the piece.  The image is
//      laid out at DESTINATION alignment (its byte `lead` is the piece's first), so a lane's 16 bytes land 4-aligned only after a
//      shift by sh = (destination - source) mod 4 bytes: dword k of the lane's unit = the top sh bytes of source dword k - 1 and the
//      low 4 - sh bytes of dword k (dword -1: the last dword of the previous unit, loaded again -- a hit in the line the neighbouring
//      lane has just fetched).  One unit more than the record has carries the bytes shifted out of its last one.  Dwords that lie
//      inside the record are stored whole, the ragged ones at its two ends byte-wise (the neighbouring record owns the other bytes).
//   2. the image goes out with 16-byte stores, its first and last unit byte-wise (the neighbouring pieces own the rest).
// A piece larger than the image (`cap` bytes; records of many kilobytes) takes the plain path: a wave per record, byte by byte.
#define BSG_THREADS 256
#define BSG_CAP     32768                // image bytes: 4 workgroups per CU beside each other (4 x 32.8 KB of the CU's 160 KB)
#define BSG_GROUP   16

__global__ void __launch_bounds__(BSG_THREADS)
k_bam_gather(const char* __restrict__ raw, const u64* __restrict__ off, const u32* __restrict__ idx, const u64* __restrict__ soff, long n, int rpb, u32 cap,
             char* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) char img[BSG_CAP + 32];
    const int tid = threadIdx.x;
    const long r0 = (long)blockIdx.x * rpb;
    const int nr = (int)((n - r0) < (long)rpb ? (n - r0) : (long)rpb);
    const u64 o0 = soff[r0], o1 = soff[r0 + nr];
    if (o1 == o0) return;
    if (o1 - o0 <= (u64)cap) {
        const u32 piece = (u32)(o1 - o0);
        const u32 lead = (u32)((uintptr_t)(out + o0) & 15u);
        char* const gout = out + o0 - lead;                        // 16-byte aligned; byte `lead` of the image is the piece's first
        const int grp = tid / BSG_GROUP, gl = tid % BSG_GROUP;
        for (int j = grp; j < nr; j += BSG_THREADS / BSG_GROUP) {
            const u64 so = soff[r0 + j];
            const int len = (int)(soff[r0 + j + 1] - so);
            if (!len) continue;
            const char* const src = raw + off[idx[r0 + j]];
            const int sl = (int)((uintptr_t)src & 15u);
            const char* const sa = src - sl;                       // the record's first 16-byte unit
            const int d0 = (int)lead + (int)(so - o0), dend = d0 + len;       // the record's place in the image
            const int nu = (sl + len + 15) >> 4;
            const int sh = (d0 - sl) & 3;
            const int db = d0 - sl - sh;                           // image offset of unit 0's first dword: a multiple of 4, may be below 0
            for (int u = gl; u <= nu; u += BSG_GROUP) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                u32 p = 0;
                if (u < nu) v = *reinterpret_cast<const uint4*>(sa + 16 * u);
                if (u > 0) p = *reinterpret_cast<const u32*>(sa + 16 * u - 4);
                const u32 s[5] = {p, v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const u32 w = sh ? (u32)((((u64)s[k + 1] << 32) | (u64)s[k]) >> (32 - 8 * sh)) : s[k + 1];
                    const int a = db + 16 * u + 4 * k;
                    if (a >= d0 && a + 4 <= dend) *reinterpret_cast<u32*>(img + a) = w;
                    else
#pragma unroll
                        for (int b = 0; b < 4; b++) if (a + b >= d0 && a + b < dend) img[a + b] = (char)(w >> (8 * b));
                }
            }
        }
        __syncthreads();
        const u32 end = lead + piece;
        const int n16 = (int)((end + 15u) >> 4);
        for (int c = tid; c < n16; c += BSG_THREADS) {
            const u32 b = (u32)c << 4;
            if (b >= lead && b + 16u <= end) *reinterpret_cast<uint4*>(gout + b) = *reinterpret_cast<const uint4*>(img + b);
            else for (u32 i = b; i < b + 16u; i++) if (i >= lead && i < end) gout[i] = img[i];
        }
        return;
    }
    const int wave = tid >> 6, lane = tid & 63;
    for (int j = wave; j < nr; j += BSG_THREADS / 64) {
        const u64 so = soff[r0 + j];
        const u64 len = soff[r0 + j + 1] - so;
        if (!len) continue;
        const char* const src = raw + off[idx[r0 + j]];
        char* const dst = out + so;
        for (u64 t = (u64)lane; t < len; t += 64) dst[t] = src[t];
    }
}
#endif
