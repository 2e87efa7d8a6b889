// bitmapperbs_amd/csrc/k_trim.hip -- adapter and quality trimming of the reads of a text call on the device (bmbs_set_trim, `--trim`).
// The rule is include/bmbs.h's (tests/trim_spec.py restates it): the BWA quality rule at the 3' end, the leftmost accepted start of a 3'
// adapter without indels, fixed clips, a length filter.  Every consumer of a read in a text call takes it from the four per-record
// arrays of FqRec (seq_off, qual_off, seq_len, qual_len), so the stage sits behind k_fq_records and rewrites them:
//   k_fq_trim      one launch per file.  TRIM_GROUP lanes per record, four records per wave; the record's four fields in place, a keep
//                  byte per record (its length passes the filter), the step counters of the file's mate (TrimWord, bmbs_words.h)
//   k_trim_keep    the keep bytes of the file(s) -> one u32 flag per template (pairs: both mates pass), what scan_u32 reads
//   k_fq_compact   the six arrays of a file scattered into a second set (a parallel compaction in place is not safe); the longest and
//                  the shortest read that stays, and their bases
// k_fq_trim stages the upper-cased sequence of its 16 records in LDS (1 KiB each) for the adapter step and tallies its counters there;
// every store to memory is an ordinary vector store or a 64-bit atomic add.
#ifndef K_TRIM_HIP
#define K_TRIM_HIP

#define TRIM_GROUP 16                              // lanes per record (k_dup_sig's: a line goes in 16-byte units at source alignment)
#define TRIM_BLOCK 256
#define TRIM_RECS (TRIM_BLOCK / TRIM_GROUP)        // records per workgroup
#define TRIM_LDS_REC 1024                          // staged bytes per record: up to 15 bytes of alignment + BMBS_MAX_READ, in whole units
#define TRIM_UNITS 4                               // units per lane at most: (15 + BMBS_MAX_READ + 15) / 16 = 64 units per record
static_assert(15 + BMBS_MAX_READ + 15 < TRIM_LDS_REC + 16 && TRIM_LDS_REC == 16 * TRIM_GROUP * TRIM_UNITS, "a record's units fit its lanes and its LDS");

// what k_fq_trim is told, by value: the adapter of the file's mate (upper case, alen letters, 0: no adapter step), the quality cutoff
// (0: no quality step) and the Phred base, the acceptance test of a start, the clips of the mate, the length filter
struct TrimArgs {
    uint4 ad[2];
    int alen, quality, base, min_overlap, error_permille, clip5, clip3, min_length;
};

// the four bytes of w upper-cased ('a'..'z' only)
DEVI u32 trim_up4(u32 w)
{
    const u32 lo7 = w & 0x7f7f7f7fu;
    const u32 m = (lo7 + 0x1f1f1f1fu) & ~(lo7 + 0x05050505u) & ~w & 0x80808080u;      // bytes in 0x61 .. 0x7a
    return w - (m >> 2);
}
DEVI u32 trim_word(const uint4& v, int w) { return w == 0 ? v.x : w == 1 ? v.y : w == 2 ? v.z : v.w; }

__global__ void __launch_bounds__(TRIM_BLOCK)
k_fq_trim(const char* __restrict__ text, FqRec o, long n, TrimArgs a, u8* __restrict__ keep, unsigned long long* __restrict__ cnt)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_seq[TRIM_RECS][TRIM_LDS_REC];
    __shared__ __attribute__((aligned(16))) unsigned char s_ad[32];
    __shared__ unsigned long long s_cnt[TRW_TRIM_COUNTERS];
    const int g = threadIdx.x / TRIM_GROUP, gl = threadIdx.x % TRIM_GROUP;
    const long r = (long)blockIdx.x * TRIM_RECS + g;
    if (threadIdx.x < 2) reinterpret_cast<uint4*>(s_ad)[threadIdx.x] = threadIdx.x ? a.ad[1] : a.ad[0];
    if (threadIdx.x < TRW_TRIM_COUNTERS) s_cnt[threadIdx.x] = 0;
    const bool live = r < n;
    u32 so = 0, qo = 0;
    int L = 0, ql = 0;
    if (live) { so = o.seq_off[r]; qo = o.qual_off[r]; L = o.seq_len[r]; ql = o.qual_len[r]; }
    const int L0 = L;

    // ---- 1. quality (cutadapt -q, the BWA rule): v_i = cutoff - (q_i - base), S_i its suffix sums; b = the largest i with S_i < 0;
    // stop = the largest i > b where S_i is largest, if that is > 0.  The lanes take consecutive units of the quality line, read at
    // source alignment: a unit reaches into the bytes around the line, which do not count; a character missing from a short line is ' '
    if (a.quality > 0) {
        const int lead = (int)((uintptr_t)(text + qo) & 15u);
        const char* const qa = text + qo - lead;
        const int nu = (lead + L + 15) >> 4;
        const int per = (nu + TRIM_GROUP - 1) / TRIM_GROUP;
        const int u0 = gl * per;
        uint4 v[TRIM_UNITS];
        int P = 0;
#pragma unroll
        for (int k = 0; k < TRIM_UNITS; k++) {
            const int u = u0 + k;
            v[k] = make_uint4(0x20202020u, 0x20202020u, 0x20202020u, 0x20202020u);
            if (k < per && u < nu) {
                if (16 * u - lead < ql) v[k] = *reinterpret_cast<const uint4*>(qa + 16 * u);
#pragma unroll
                for (int t = 0; t < 16; t++) {
                    const int i = 16 * u - lead + t;
                    const int q = i < ql ? (int)((trim_word(v[k], t >> 2) >> (8 * (t & 3))) & 255u) : (int)' ';
                    if (i >= 0 && i < L) P += a.quality - (q - a.base);
                }
            }
        }
        // T = the sum of the lanes to the right (a suffix scan across the group)
        int inc = P;
        for (int d = 1; d < TRIM_GROUP; d <<= 1) { const int x = __shfl_down(inc, d, TRIM_GROUP); if (gl + d < TRIM_GROUP) inc += x; }
        int s = inc - P;
        // the lane's own positions from the right: its first negative sum, and the largest sum (rightmost on ties) in front of it
        const int NONE = -(1 << 30);
        int neg = -1, mx = NONE, am = -1, lo = L;
#pragma unroll
        for (int k = TRIM_UNITS - 1; k >= 0; k--) {
            const int u = u0 + k;
            if (k < per && u < nu) {
#pragma unroll
                for (int t = 15; t >= 0; t--) {
                    const int i = 16 * u - lead + t;
                    const int q = i < ql ? (int)((trim_word(v[k], t >> 2) >> (8 * (t & 3))) & 255u) : (int)' ';
                    if (i >= 0 && i < L) {
                        s += a.quality - (q - a.base);
                        lo = i;
                        if (neg < 0) {
                            if (s < 0) neg = i;
                            else if (s > mx) { mx = s; am = i; }
                        }
                    }
                }
            }
        }
        int b = neg;
        for (int d = TRIM_GROUP / 2; d; d >>= 1) { const int x = __shfl_xor(b, d, TRIM_GROUP); b = x > b ? x : b; }
        // lanes to the left of b do not count; b's own lane stopped there
        if (neg != b && lo <= b) mx = NONE;
        for (int d = TRIM_GROUP / 2; d; d >>= 1) {
            const int xm = __shfl_xor(mx, d, TRIM_GROUP), xa = __shfl_xor(am, d, TRIM_GROUP);
            if (xm > mx || (xm == mx && xa > am)) { mx = xm; am = xa; }
        }
        if (mx > 0) L = am;
    }
    const int L1 = L;

    // ---- 2. 3' adapter (cutadapt -a, --no-indels' acceptance test): the leftmost start i at which the overlap o = min(|A|, L - i)
    // is at least min_overlap and has at most o * error_permille / 1000 mismatches.  The upper-cased sequence is staged once; the lanes
    // take the starts i, i + 16, ... and leave a start as soon as its mismatches exceed the bound
    if (a.alen > 0) {
        const int lead = (int)((uintptr_t)(text + so) & 15u);
        const char* const sa = text + so - lead;
        const int nu = (lead + L + 15) >> 4;
        uint4* const dst = reinterpret_cast<uint4*>(s_seq[g]);
        for (int u = gl; u < nu; u += TRIM_GROUP) {
            uint4 w = *reinterpret_cast<const uint4*>(sa + 16 * u);
            w.x = trim_up4(w.x); w.y = trim_up4(w.y); w.z = trim_up4(w.z); w.w = trim_up4(w.w);
            dst[u] = w;
        }
        __syncthreads();
        const unsigned char* const sq = s_seq[g] + lead;
        int best = L;
        for (int i = gl; i < L; i += TRIM_GROUP) {
            const int ov = a.alen < L - i ? a.alen : L - i;
            if (ov < a.min_overlap) break;                       // (the overlap only shrinks from here on)
            const int bound = ov * a.error_permille / 1000;
            int mm = 0;
            for (int j = 0; j < ov; j++) { mm += sq[i + j] != s_ad[j] ? 1 : 0; if (mm > bound) break; }
            if (mm <= bound) { best = i; break; }
        }
        for (int d = TRIM_GROUP / 2; d; d >>= 1) { const int x = __shfl_xor(best, d, TRIM_GROUP); best = x < best ? x : best; }
        L = best;
    } else __syncthreads();                                      // (s_cnt is zero before the first add)
    const int L2 = L;

    // ---- 3. fixed clips: the 3' end first, then the 5' end (both lines begin k characters later)
    L -= L < a.clip3 ? L : a.clip3;
    const int k5 = L < a.clip5 ? L : a.clip5;
    L -= k5;
    if (live && gl == 0) {
        int nq = ql - k5;
        nq = nq < 0 ? 0 : nq > L ? L : nq;
        o.seq_off[r] = so + (u32)k5; o.qual_off[r] = qo + (u32)k5; o.seq_len[r] = (u16)L; o.qual_len[r] = (u16)nq;
        keep[r] = L >= a.min_length ? 1 : 0;
        atomicAdd(&s_cnt[TRW_RECORDS_IN], 1ull); atomicAdd(&s_cnt[TRW_BASES_IN], (unsigned long long)L0);
        if (L1 < L0) { atomicAdd(&s_cnt[TRW_Q_RECORDS], 1ull); atomicAdd(&s_cnt[TRW_Q_BASES], (unsigned long long)(L0 - L1)); }
        if (L2 < L1) { atomicAdd(&s_cnt[TRW_A_RECORDS], 1ull); atomicAdd(&s_cnt[TRW_A_BASES], (unsigned long long)(L1 - L2)); }
        if (L < L2) { atomicAdd(&s_cnt[TRW_C_RECORDS], 1ull); atomicAdd(&s_cnt[TRW_C_BASES], (unsigned long long)(L2 - L)); }
    }
    __syncthreads();
    if (threadIdx.x < TRW_TRIM_COUNTERS && s_cnt[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], s_cnt[threadIdx.x]);
}

// flag[r] = 1 where template r stays: its record passed the length filter (pairs: both mates')
__global__ void __launch_bounds__(256)
k_trim_keep(const u8* __restrict__ keep0, const u8* __restrict__ keep1, long n, u32* __restrict__ flag)
{
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    flag[r] = (u32)(keep0[r] & (keep1 ? keep1[r] : (u8)1));
}

// the records that stay, in input order: record r of `src` becomes record off[r] of `dst`.  bases: the file's TRW_BASES_OUT; lens: the
// words TRW_MAX_LEN, TRW_MIN_LEN_C of the call (both files add to them)
__global__ void __launch_bounds__(256)
k_fq_compact(FqRec src, FqRec dst, const u32* __restrict__ flag, const u64* __restrict__ off, long n, unsigned long long* __restrict__ bases,
             unsigned long long* __restrict__ lens)
{
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    u32 L = 0, Lc = 0, sum = 0;
    if (r < n && flag[r]) {
        const u64 d = off[r];
        const u32 sl = src.seq_len[r];
        dst.seq_off[d] = src.seq_off[r]; dst.qual_off[d] = src.qual_off[r]; dst.name_off[d] = src.name_off[r];
        dst.seq_len[d] = (u16)sl; dst.qual_len[d] = src.qual_len[r]; dst.name_len[d] = src.name_len[r];
        L = sl; Lc = ~sl; sum = sl;
    }
    for (int of = 32; of > 0; of >>= 1) {
        const u32 x = __shfl_down(L, of, 64), y = __shfl_down(Lc, of, 64);
        L = x > L ? x : L; Lc = y > Lc ? y : Lc; sum += __shfl_down(sum, of, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (sum) atomicAdd(bases, (unsigned long long)sum);
        if (Lc) { atomicMax(&lens[0], (unsigned long long)L); atomicMax(&lens[1], (unsigned long long)Lc); }
    }
}
#endif
