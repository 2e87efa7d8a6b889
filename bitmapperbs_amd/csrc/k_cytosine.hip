// bitmapperbs_amd/csrc/k_cytosine.hip -- the genome-wide cytosine report on the device (`--methyl <prefix> --cytosine-report`,
// bmbs_methyl_report): one line of text for every cytosine of a selected context in a window [beg, end) of one sequence, on both strands,
// covered or not.  The rule is in include/bmbs.h; tests/cytosine_spec.py restates it.  A line is
//     name \t pos + 1 \t + | - \t methylated \t unmethylated \t CG | CHG | CHH \t three letters \n
//   k_cyt_check   one lane per site of the caller's: its sequence, the window, the order, its kind against the genome, the selection,
//                 contact with a run of bases the FASTA does not spell A, C, G or T
//   k_cyt_count   one lane per 32-base genome word of the window: the bytes and lines of the word
//   (scan_u32)    where each word's text goes: 64-bit offsets
//   k_cyt_emit    CYT_WPB consecutive words per block = one contiguous piece of the text, four lanes per word (eight positions each):
//                 the piece is formatted into LDS and goes out in whole aligned 16-byte stores, its ragged ends byte by byte
//                 (k_line_write's scheme, bmbs_bam.hip); a piece above CYT_LDS bytes is written straight to memory
// Which positions are cytosines of which context is meth_masks' word (k_methyl.hip), nothing of this file's: what is added here is the
// window, the runs, the join against the sites and the text.  The sites are ordered by position, so a lane finds the first site of its
// positions with one binary search and walks on from there.  Every store is an ordinary vector store, every add an atomicAdd /
// atomicMax of plain C++; there is no inline assembly.
#ifndef K_CYTOSINE_HIP
#define K_CYTOSINE_HIP

#define CYT_WPB 64                        // genome words per block of k_cyt_emit (256 lanes, four per word)
#define CYT_LDS 49152                     // bytes of the block's image of its piece of the text (three blocks a CU)

// the sequence [s_lo, s_hi) and the window [a0, a1) in genome coordinates; word i of the call is genome word W0 + i; sites and runs in
// sequence coordinates (run r = [run[2 r], run[2 r + 1])); the sequence's name
struct CytPar {
    const u64* gen2p; long s_lo, s_hi, a0, a1, W0, nW;
    const bmbs_methyl_site* site; long n_site;
    const long* run; long n_run;
    const char* name; u32 name_len, contexts;
};

// the bits of the 36-base window of word W (bit k = genome position 32 W - 2 + k) that lie in a run
DEVI u64 cyt_run_bits(const CytPar& P, long W)
{
    const long r_lo = 32 * W - 2 - P.s_lo;                                  // bit 0 in sequence coordinates
    long lo = 0, hi = P.n_run;                                              // the first run that ends behind r_lo
    while (lo < hi) { const long mid = (lo + hi) >> 1; if (P.run[2 * mid + 1] > r_lo) hi = mid; else lo = mid + 1; }
    u64 R = 0;
    for (long r = lo; r < P.n_run && P.run[2 * r] < r_lo + 36; r++) R |= meth_range(r_lo, P.run[2 * r], P.run[2 * r + 1], 36);
    return R;
}

// What word W says: sel = the positions that get a line unless a site says otherwise (a cytosine of a selected context inside the
// window whose own window touches no run), rev = those that are a forward G, cpg / chg = the positions of these contexts (else CHH);
// b0 / b1 = the two planes of the 36-base window, unk = its positions that print as N (off the sequence, or in a run)
struct CytWord { u32 sel, rev, cpg, chg; u64 b0, b1, unk; };
DEVI CytWord cyt_word(const CytPar& P, long W)
{
    u32 m[6];
    meth_masks(P.gen2p, W, P.s_lo, P.s_hi, m);
    const u64 wp = W > 0 ? P.gen2p[W - 1] : 0, wc = P.gen2p[W], wn = P.gen2p[W + 1];
    CytWord w;
    w.b0 = ((u64)(u32)wp >> 30) | ((u64)(u32)wc << 2) | (((u64)(u32)wn & 3u) << 34);
    w.b1 = ((u64)(u32)(wp >> 32) >> 30) | ((u64)(u32)(wc >> 32) << 2) | (((u64)(u32)(wn >> 32) & 3u) << 34);
    const u64 R = P.n_run ? cyt_run_bits(P, W) : 0;
    w.unk = ~meth_range(32 * W - 2, P.s_lo, P.s_hi, 36) | R;
    // a forward C at bit b reads b, b + 1 (CpG) and b + 2 (CHG, CHH); a forward G reads b, b - 1 and b - 2: bit b of R is position b - 2
    const u64 Ra = R >> 2;
    const u32 tf2 = (u32)(Ra | (Ra >> 1)), tf3 = tf2 | (u32)(Ra >> 2);
    const u32 tr2 = (u32)(Ra | (R >> 1)), tr3 = tr2 | (u32)R;
    u32 fw = 0, rv = 0;
    if (P.contexts & 1u) { fw |= m[0] & ~tf2; rv |= m[3] & ~tr2; }
    if (P.contexts & 2u) { fw |= m[1] & ~tf3; rv |= m[4] & ~tr3; }
    if (P.contexts & 4u) { fw |= m[2] & ~tf3; rv |= m[5] & ~tr3; }
    w.sel = (fw | rv) & (u32)meth_range(32 * W, P.a0, P.a1, 32);
    w.rev = rv; w.cpg = m[0] | m[3]; w.chg = m[1] | m[4];
    return w;
}

// decimal digits of v, by comparisons
DEVI u32 cyt_digits(u64 v) { u32 d = 1; for (u64 t = 10; d < 20 && v >= t; t *= 10) d++; return d; }
// v in d digits at p
DEVI char* cyt_put(char* p, u64 v, u32 d) { for (u32 k = d; k-- > 0;) { p[k] = (char)('0' + (u32)(v % 10)); v /= 10; } return p + d; }
// the letter of bit k of the word's 36-base window, on the forward strand or complemented ("ACGT" / "TGCA", one byte each)
DEVI char cyt_letter(const CytWord& w, int k, bool comp)
{
    if ((w.unk >> k) & 1u) return 'N';
    const u32 code = (u32)((w.b0 >> k) & 1u) | ((u32)((w.b1 >> k) & 1u) << 1);
    return (char)(((comp ? 0x41434754u : 0x54474341u) >> (8 * code)) & 0xffu);
}

// The lines of the positions `mask` of word W: their bytes, *n_lines their number; EMIT: written at dst.  A site with BMBS_REPORT_OMIT
// takes its position's line away.  The sites need not be what k_cyt_check accepts for this to stay inside the arrays.
template <bool EMIT>
DEVI u32 cyt_lines(const CytPar& P, const CytWord& w, long W, u32 mask, char* dst, u32* n_lines)
{
    u32 sel = w.sel & mask, bytes = 0, lines = 0;
    *n_lines = 0;
    if (!sel) return 0;
    const long p0 = 32 * W - P.s_lo;                                        // bit 0 in sequence coordinates
    long j = 0, hi = P.n_site;                                              // the first site at or behind the first position
    { const long first = p0 + __ffs((int)sel) - 1; while (j < hi) { const long mid = (j + hi) >> 1; if ((long)P.site[mid].pos < first) j = mid + 1; else hi = mid; } }
    while (sel) {
        const int b = __ffs((int)sel) - 1;
        sel &= sel - 1;
        const long p = p0 + b;
        while (j < P.n_site && (long)P.site[j].pos < p) j++;
        u32 me = 0, un = 0;
        if (j < P.n_site && (long)P.site[j].pos == p) {
            const bmbs_methyl_site s = P.site[j];
            if (s.kind & BMBS_REPORT_OMIT) continue;
            me = s.meth; un = s.unmeth;
        }
        const bool cpg = (w.cpg >> b) & 1u, rev = (w.rev >> b) & 1u;
        const u32 dp = cyt_digits((u64)p + 1), dm = cyt_digits(me), du = cyt_digits(un);
        bytes += P.name_len + dp + dm + du + (cpg ? 2u : 3u) + 11u;          // six tabs, the strand, three letters, the newline
        lines++;
        if (EMIT) {
            char* q = dst;
            for (u32 k = 0; k < P.name_len; k++) q[k] = P.name[k];
            q += P.name_len;
            *q++ = '\t'; q = cyt_put(q, (u64)p + 1, dp);
            *q++ = '\t'; *q++ = rev ? '-' : '+';
            *q++ = '\t'; q = cyt_put(q, me, dm);
            *q++ = '\t'; q = cyt_put(q, un, du);
            *q++ = '\t'; *q++ = 'C';
            if (cpg) *q++ = 'G'; else { *q++ = 'H'; *q++ = ((w.chg >> b) & 1u) ? 'G' : 'H'; }
            *q++ = '\t';
            for (int k = 0; k < 3; k++) *q++ = cyt_letter(w, rev ? b + 2 - k : b + 2 + k, rev);
            *q++ = '\n';
            dst = q;
        }
    }
    *n_lines = lines;
    return bytes;
}

// info[x] = ~(the first site that ...), 0: none.  x = 0: has another ref; 1: lies outside [beg, end); 2: does not sit at a larger
// position than its predecessor; 3: kind & 7 is not what the genome says at its position (or kind has bits above BMBS_REPORT_OMIT);
// 4: its context is not selected; 5: its window touches a run.  beg / end in sequence coordinates (P.a0 - P.s_lo, P.a1 - P.s_lo); the
// genome is looked at only for a site inside the window
__global__ void __launch_bounds__(256)
k_cyt_check(CytPar P, int ref, u32* __restrict__ info)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n_site) return;
    const bmbs_methyl_site s = P.site[i];
    if (s.ref != ref) atomicMax(&info[0], ~(u32)i);
    if (i > 0 && P.site[i - 1].pos >= s.pos) atomicMax(&info[2], ~(u32)i);
    const long a = P.s_lo + (long)s.pos;
    if (s.pos < 0 || a < P.a0 || a >= P.a1) { atomicMax(&info[1], ~(u32)i); return; }
    u32 m[6];
    meth_masks(P.gen2p, a >> 5, P.s_lo, P.s_hi, m);
    u32 kind = 0xffffffffu;
#pragma unroll
    for (int x = 0; x < 6; x++) if ((m[x] >> (a & 31)) & 1u) kind = (u32)(x % 3) | ((u32)(x / 3) << 2);
    if (kind != (s.kind & ~(u32)BMBS_REPORT_OMIT)) { atomicMax(&info[3], ~(u32)i); return; }
    if (!((P.contexts >> (kind & 3u)) & 1u)) atomicMax(&info[4], ~(u32)i);
    // the window [lo, hi] of the site and the last run that begins at or in front of hi (methyl_touches, search_sort.h)
    const long w = (kind & 3u) == 0 ? 1 : 2;
    const long lo = (kind & 4u) ? (long)s.pos - w : (long)s.pos, hi = (kind & 4u) ? (long)s.pos : (long)s.pos + w;
    long r0 = 0, r1 = P.n_run;
    while (r0 < r1) { const long mid = (r0 + r1) >> 1; if (P.run[2 * mid] <= hi) r0 = mid + 1; else r1 = mid; }
    if (r0 > 0 && P.run[2 * (r0 - 1) + 1] > lo) atomicMax(&info[5], ~(u32)i);
}

// cnt[i] = the bytes of word i of the call; *n_lines += its lines (the wave's, added up first)
__global__ void __launch_bounds__(256)
k_cyt_count(CytPar P, u32* __restrict__ cnt, unsigned long long* __restrict__ n_lines)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    u32 lines = 0;
    if (i < P.nW) {
        const CytWord w = cyt_word(P, P.W0 + i);
        cnt[i] = cyt_lines<false>(P, w, P.W0 + i, 0xffffffffu, nullptr, &lines);
    }
    for (int d = 32; d; d >>= 1) lines += (u32)__shfl_xor((int)lines, d);
    if ((threadIdx.x & 63) == 0 && lines) atomicAdd(n_lines, (unsigned long long)lines);
}

// the text: word i at out + off[i] (off = the exclusive scan of cnt, nW + 1 entries)
__global__ void __launch_bounds__(256)
k_cyt_emit(CytPar P, const u64* __restrict__ off, char* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) char img[CYT_LDS + 16];
    const int tid = (int)threadIdx.x;
    const long w0 = (long)blockIdx.x * CYT_WPB;
    const int nw = (int)(P.nW - w0 < CYT_WPB ? P.nW - w0 : CYT_WPB);      // words of this block
    const u64 o0 = off[w0], piece = off[w0 + nw] - o0;
    if (!piece) return;                                                     // (uniform within the block)
    const int wi = tid >> 2, q = tid & 3;
    const bool live = wi < nw;
    const long W = P.W0 + w0 + wi;
    const u32 mask = 0xffu << (8 * q);
    CytWord w = {0, 0, 0, 0, 0, 0, 0};
    u32 mine = 0, lines = 0;
    if (live) { w = cyt_word(P, W); mine = cyt_lines<false>(P, w, W, mask, nullptr, &lines); }
    // where the lane's eight positions go: the bytes of the word's lanes in front of it (every lane of the wave takes part)
    u32 incl = mine;
    for (int d = 1; d < 4; d <<= 1) { const u32 v = (u32)__shfl_up((int)incl, d, 4); if (q >= d) incl += v; }
    const u64 at = live ? off[w0 + wi] - o0 + (incl - mine) : 0;
    if (piece > CYT_LDS) {                                                  // (uniform) long names, many cytosines, long counts: straight to memory
        if (mine) cyt_lines<true>(P, w, W, mask, out + o0 + at, &lines);
        return;
    }
    const u32 lead = (u32)((uintptr_t)(out + o0) & 15u);
    char* const gout = out + o0 - lead;                                     // 16-byte aligned; byte `lead` of the image is the piece's first
    if (mine) cyt_lines<true>(P, w, W, mask, img + lead + (u32)at, &lines);
    __syncthreads();
    const u32 end = lead + (u32)piece;
    const int n16 = (int)((end + 15u) >> 4);
    for (int c = tid; c < n16; c += 256) {
        const u32 b = (u32)c << 4;
        if (b >= lead && b + 16u <= end) *reinterpret_cast<uint4*>(gout + b) = *reinterpret_cast<const uint4*>(img + b);
        else for (u32 i = b; i < b + 16u; i++) if (i >= lead && i < end) gout[i] = img[i];
    }
}
#endif
