// bitmapperbs_amd/csrc/k_methyl.hip -- per-cytosine methylation counts from BAM records on the device (`--bam --sort --methyl`,
// bmbs_bam_methyl[_opts], bmbs_bam_sort_methyl[_opts], bmbs_methyl_sites, bmbs_methyl_mbias, bmbs_text_sorted_clip,
// bmbs_bam_methyl_opposite, bmbs_bam_sort_methyl_opposite, bmbs_methyl_opposite).  The rule is in include/bmbs.h; tests/methyl_spec.py
// restates the sites, tests/mbias_spec.py the read-end trim and the M-bias table, tests/variant_spec.py the opposite-strand observation.
//
// Record i = len[i] bytes at raw + off[i] (len 0: no record), the layout of k_markdup.hip.  An EVENT is one call of one read base:
// key = refID << pos_bits | pos, value = 1 << 32 (methylated) or 1 (unmethylated) -- the same (key, value) form a SITE has once its
// events are added up, so that one reduction serves the events of a slice of records and the sites of several slices.
//   k_meth_events<false>  a group of METH_GROUP lanes per record: checks it, decides whether it counts, and counts its events
//   (scan_u32)            where each record's events go
//   k_meth_events<true>   the same walk again, writing the events  (<.., true>: both passes leave out the calls of trimmed cycles)
//   k_meth_events<.., .., true>  the OPPOSITE-strand observation (bmbs_bam_methyl_opposite, bmbs_bam_sort_methyl_opposite; tests/
//                         variant_spec.py): the same two passes, but an OB record is looked at where the genome has a forward C of a
//                         selected context and an OT record where it has a forward G -- where the other strand's records are called.  A
//                         read base that passes the filters of a call is a MATCH (value 1) when its code is the genome's base there
//                         (C = 2, G = 4), a VARIANT (value 1 << 32) when it is one of the other three of A C G T, else nothing
//   k_meth_mbias          the same walk once more when the M-bias table is asked for: a histogram of the calls by (mate, strand,
//                         context, methylated, cycle), trimmed or not
//   k_meth_cut            where a slice of records ends that holds at most a given number of events
//   (pair sort)           rocPRIM radix_sort_pairs over (key, value), stable, over the key bits that can be set only
//   k_meth_heads          run heads of equal keys per wave by ballot + popcount; the two halves of the values as 32-bit words for the scans
//   k_meth_hpos           the position of every run head, from the scan of the waves' head counts
//   k_meth_sites          per head the sums of its run from the two scans: a bmbs_methyl_site (context and strand looked up in the genome
//                         again) or a (key, value) pair for the merge of slices
//   k_meth_clip           the mate-overlap clip of every record of a sorted text call, in sorted order
// The context masks are bit-parallel on the planes of DevIndex::gen2p, 32 reference bases a word; read bases and qualities are fetched
// only where a mask bit is set.  k_meth_mbias keeps a block's tally in LDS; no other kernel here uses LDS.  Every store is an ordinary
// vector store, every add an atomicAdd of plain C++; there is no inline assembly.
#ifndef K_METHYL_HIP
#define K_METHYL_HIP

#define METH_GROUP 16                     // lanes per record: a lane takes one 32-base word of the record's reference span at a time

#define METH_MBIAS_ROWS 24                // mate x strand x context x (unmethylated, methylated)
#define METH_MBIAS_LDS 256                // k_meth_mbias: cycles below this are tallied in the block's LDS table

// ig5 / ig3: the cycles left out at the 5' / 3' end of a record of mate 0 / 1 (read only where TRIM is set)
struct MethPar { u32 contexts, min_mapq, min_phred; int n_chrom, pos_bits; u32 ig5[2], ig3[2]; };

// mate of a record: 1 for read 2 of a pair (flags 0x1 and 0x80), else 0
DEVI u32 meth_mate(u32 flag) { return (flag & 0x81u) == 0x81u ? 1u : 0u; }
// cycle of read base ri: its position in sequencing order (SEQ is stored reversed for flag 0x10)
DEVI long meth_cycle(u32 flag, u32 l_seq, long ri) { return (flag & 0x10u) ? (long)l_seq - 1 - ri : ri; }

// bits k of a 64-bit window whose bit 0 is position b0, for the positions in [lo, hi)  (the window is at most 63 bits wide in use)
DEVI u64 meth_range(long b0, long lo, long hi, int width)
{
    long kl = lo - b0, kh = hi - b0;
    kl = kl < 0 ? 0 : (kl > width ? width : kl);
    kh = kh < 0 ? 0 : (kh > width ? width : kh);
    return kh > kl ? (((u64)1 << kh) - 1) & ~(((u64)1 << kl) - 1) : 0;
}

// The cytosines with a context among the 32 forward positions of genome word W (absolute positions 32 W .. 32 W + 31), as far as they
// lie in the sequence [lo, hi): m[ctx] forward-strand C, m[3 + ctx] forward-strand G (a cytosine of the reverse strand), ctx 0 CpG,
// 1 CHG, 2 CHH.  With A0 C1 G2 T3: C = b0 & ~b1, G = ~b0 & b1; the neighbours two positions to either side come from words W - 1 and
// W + 1 (the planes hold the doubled genome: W + 1 exists for every forward word), positions outside [lo, hi) are neither C nor G.
DEVI void meth_masks(const u64* __restrict__ gen2p, long W, long lo, long hi, u32 m[6])
{
    const u64 wp = W > 0 ? gen2p[W - 1] : 0, wc = gen2p[W], wn = gen2p[W + 1];
    // 36-bit windows, bit k = position 32 W - 2 + k
    const u64 b0 = ((u64)(u32)wp >> 30) | ((u64)(u32)wc << 2) | (((u64)(u32)wn & 3u) << 34);
    const u64 b1 = ((u64)(u32)(wp >> 32) >> 30) | ((u64)(u32)(wc >> 32) << 2) | (((u64)(u32)(wn >> 32) & 3u) << 34);
    const u64 I = meth_range(32 * W - 2, lo, hi, 36);
    const u64 Cm = b0 & ~b1 & I, Gm = ~b0 & b1 & I;
    const u64 cpg = Cm & (Gm >> 1), chg = Cm & ~cpg & (Gm >> 2), chh = Cm & ~cpg & ~chg & (I >> 2);
    const u64 gpc = Gm & (Cm << 1), ghc = Gm & ~gpc & (Cm << 2), ghh = Gm & ~gpc & ~ghc & (I << 2);
    m[0] = (u32)(cpg >> 2); m[1] = (u32)(chg >> 2); m[2] = (u32)(chh >> 2);
    m[3] = (u32)(gpc >> 2); m[4] = (u32)(ghc >> 2); m[5] = (u32)(ghh >> 2);
}

// info[0] = ~(the first record whose length is below 36 or is not its block_size + 4), info[1] = ~(the first whose read name, CIGAR,
// sequence and qualities do not fit its length), info[2] = ~(the first whose refID is beyond the index's sequences), info[3] = ~(the
// first mapped record whose reference span runs off its sequence) (0: none).  Nothing is read behind a record.
// EMIT false: cnt[i - first] = the events of record i.  EMIT true: they are written at eoff[i - first] - eoff[0].
// TRIM: a call of cycle c of a record of mate m is an event only if par.ig5[m] <= c < l_seq - par.ig3[m]; both passes of a call run
// the same TRIM.  <.., false> is the kernel as it was before there was a trim: none of this is compiled into it.
// OPP: the opposite-strand observation (the header of this file): the other half of the masks, and match / variant in the place of
// unmethylated / methylated.  Its record checks are those of the calls and report through the same four words, nothing of its own.
// <.., .., false> (the default) is the kernel as it was before there was one: none of this is compiled into it, and its code is the
// same instruction for instruction -- which a template parameter guarantees and a walk shared through a function does not.
// k_meth_mbias below holds a COPY of the record checks and of the walk: a change to the rule here has to be made there too.
// k_nonconv_walk (k_nonconv.hip) holds a third copy, with the non-conversion filter's own rule for which records it looks at.
template <bool EMIT, bool TRIM, bool OPP = false>
__global__ void __launch_bounds__(256)
k_meth_events(const u64* __restrict__ gen2p, const u64* __restrict__ chrom_start, const char* __restrict__ raw, const u64* __restrict__ off,
              const u32* __restrict__ len, const u32* __restrict__ clip, long first, long n, MethPar par, u32* __restrict__ cnt,
              const u64* __restrict__ eoff, u64* __restrict__ key, u64* __restrict__ val, u32* __restrict__ info)
{
    const long t = ((long)blockIdx.x * blockDim.x + threadIdx.x) / METH_GROUP;
    const int gl = threadIdx.x % METH_GROUP;
    const long i = first + t;
    bool live = t < n;
    const u32 l = live ? len[i] : 0;
    if (l == 0) live = false;
    if (live && l < 36) { if (!EMIT && gl == 0) atomicMax(&info[0], ~(u32)i); live = false; }
    const char* const p = raw + (live ? off[i] : 0);
    if (live && bs_ld32(p) + 4u != l) { if (!EMIT && gl == 0) atomicMax(&info[0], ~(u32)i); live = false; }
    int ref = -1, pos = 0;
    u32 l_name = 0, mapq = 0, n_cig = 0, flag = 4, l_seq = 0;
    if (live) {
        ref = (int)bs_ld32(p + 4); pos = (int)bs_ld32(p + 8);
        l_name = (u32)(unsigned char)p[12]; mapq = (u32)(unsigned char)p[13];
        n_cig = (u32)(unsigned char)p[16] | ((u32)(unsigned char)p[17] << 8);
        flag = (u32)(unsigned char)p[18] | ((u32)(unsigned char)p[19] << 8);
        l_seq = bs_ld32(p + 20);
        if (36ull + l_name + 4ull * n_cig + ((u64)l_seq + 1) / 2 + l_seq > (u64)l) { if (!EMIT && gl == 0) atomicMax(&info[1], ~(u32)i); live = false; }
    }
    if (live && ref >= par.n_chrom) { if (!EMIT && gl == 0) atomicMax(&info[2], ~(u32)i); live = false; }
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
    bool counts = mapped;
    if (mapped) {
        s_lo = (long)chrom_start[ref]; s_hi = (long)chrom_start[ref + 1];
        if (pos < 0 || (u64)pos + span > (u64)(s_hi - s_lo)) { if (!EMIT && gl == 0) atomicMax(&info[3], ~(u32)i); counts = false; }
    }
    counts = counts && !(flag & 0xF00u) && mapq >= par.min_mapq && (!(flag & 1u) || (flag & 2u));
    u32 total = 0;
    const u64 ebase = (EMIT && t < n) ? eoff[t] - eoff[0] : 0;
    // paired: read 1 reverse or read 2 forward is OB; single: reverse is OB
    const bool ob = (flag & 1u) ? (((flag & 0x40u) && (flag & 0x10u)) || ((flag & 0x80u) && !(flag & 0x10u))) : (flag & 0x10u) != 0;
    const long a0 = s_lo + pos, a1 = a0 + (long)span;                       // the span in genome coordinates
    const u32 cw = (counts && clip) ? clip[i] : 0;
    const long c_lo = a0 + (long)(cw >> 16), c_hi = c_lo + (long)(cw & 0xffffu);
    const bool all_m = counts && n_cig == 1 && ((0x181u >> (bs_ld32(cg) & 15u)) & 1u);      // one M, = or X: a constant shift
    const char* const sq = cg + 4 * (u64)n_cig;
    const char* const ql = sq + ((u64)l_seq + 1) / 2;
    // G / A for OB, C / T for OT (BAM's 4-bit codes); OPP: want_u = the genome's own base where the record is looked at, C for OB, G for OT
    const u32 want_m = OPP ? 0u : ob ? 4u : 2u, want_u = OPP ? (ob ? 2u : 4u) : ob ? 1u : 8u;
    const bool at_g = OPP ? !ob : ob;                                       // the record is looked at where the genome has a forward G
    const long W0 = a0 >> 5, W1 = counts && span ? (a1 - 1) >> 5 : W0 - 1;
    const long t_lo = TRIM ? (long)par.ig5[meth_mate(flag)] : 0, t_hi = TRIM ? (long)l_seq - (long)par.ig3[meth_mate(flag)] : 0;
    for (long base = W0; base <= W1; base += METH_GROUP) {                  // (uniform within the group)
        const long W = base + gl;
        u32 mb = 0, ub = 0;
        if (W <= W1) {
            u32 m[6];
            meth_masks(gen2p, W, s_lo, s_hi, m);
            u32 sel = 0;
#pragma unroll
            for (int x = 0; x < 3; x++) if ((par.contexts >> x) & 1u) sel |= m[(at_g ? 3 : 0) + x];
            sel &= (u32)meth_range(32 * W, a0, a1, 32) & ~(u32)meth_range(32 * W, c_lo, c_hi, 32);
            // the read base against each position that is left: bits ascend, so the CIGAR is walked once per word
            u32 k = 0; long r_at = 0, i_at = 0;
            while (sel) {
                const int b = __ffs((int)sel) - 1;
                sel &= sel - 1;
                const long ro = 32 * W + b - a0;                             // offset in the record's reference span
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
                if (TRIM) { const long cy = meth_cycle(flag, l_seq, ri); if (cy < t_lo || cy >= t_hi) continue; }
                const u32 q = (u32)(unsigned char)ql[ri];
                if ((q == 255u ? 0u : q) < par.min_phred) continue;
                const u32 by = (u32)(unsigned char)sq[ri >> 1];
                const u32 code = (ri & 1) ? (by & 15u) : (by >> 4);
                if (OPP) {                                                   // a match, or one of the other three of A C G T: a variant
                    if (code == want_u) ub |= 1u << b;
                    else if ((0x116u >> code) & 1u) mb |= 1u << b;
                }
                else if (code == want_m) mb |= 1u << b;
                else if (code == want_u) ub |= 1u << b;
            }
        }
        // where this lane's events go: the group's counts added up from lane 0 on
        const u32 mine = (u32)__popc(mb | ub);
        u32 incl = mine;
        for (int d = 1; d < METH_GROUP; d <<= 1) { const u32 v = (u32)__shfl_up((int)incl, d, METH_GROUP); if (gl >= d) incl += v; }
        const u32 all = (u32)__shfl((int)incl, METH_GROUP - 1, METH_GROUP);
        if (EMIT) {
            u64 e = ebase + total + (incl - mine);
            u32 both = mb | ub;
            const u64 kref = (u64)(u32)ref << par.pos_bits;
            while (both) {
                const int b = __ffs((int)both) - 1;
                both &= both - 1;
                key[e] = kref | (u64)(32 * W + b - s_lo);
                val[e] = ((mb >> b) & 1u) ? (u64)1 << 32 : (u64)1;
                e++;
            }
        }
        total += all;
    }
    if (!EMIT && t < n && gl == 0) cnt[t] = total;
}

// The M-bias table: table[row * BMBS_MBIAS_CYCLES + min(cycle, BMBS_MBIAS_CYCLES - 1)] += 1 for every call of records 0 .. n - 1, with
// row = ((mate * 2 + strand) * 3 + context) * 2 + methylated.  A call is what k_meth_events<.., false> makes an event of: the trim is
// not looked at.  The walk is that kernel's, written out again: the tally needs the read index and the context of a call where the
// innermost loop has them, and a walk shared through a function would have to leave k_meth_events' code as it is.  It
// runs behind a count pass that found nothing to refuse; the checks stay, so that nothing is read behind a record, and report nothing.
// A fixed grid strides over the records, a group of METH_GROUP lanes per record.  Each block tallies the cycles below METH_MBIAS_LDS in
// its own u32 table in LDS (24 rows x 256 x 4 B = 24 KiB) with adds that return nothing, and adds its non-zero counters to the global
// table when it is through; later cycles go to the global table at once.  A record has every cycle once, so it adds at most 1 to any
// one counter: with n < 2^31 records no u32 counter of a block can wrap.  Integer adds: the table does not depend on their order.
__global__ void __launch_bounds__(256)
k_meth_mbias(const u64* __restrict__ gen2p, const u64* __restrict__ chrom_start, const char* __restrict__ raw, const u64* __restrict__ off,
             const u32* __restrict__ len, const u32* __restrict__ clip, long n, MethPar par, unsigned long long* __restrict__ table)
{
    __shared__ u32 tally[METH_MBIAS_ROWS * METH_MBIAS_LDS];
    for (int x = (int)threadIdx.x; x < METH_MBIAS_ROWS * METH_MBIAS_LDS; x += 256) tally[x] = 0;
    __syncthreads();
    const int gl = threadIdx.x % METH_GROUP;
    const long per_block = 256 / METH_GROUP, step = (long)gridDim.x * per_block;
    for (long first = (long)blockIdx.x * per_block; first < n; first += step) {          // (uniform within the block)
        const long i = first + threadIdx.x / METH_GROUP;
        bool live = i < n;
        const u32 l = live ? len[i] : 0;
        if (l < 36) live = false;
        const char* const p = raw + (live ? off[i] : 0);
        if (live && bs_ld32(p) + 4u != l) live = false;
        int ref = -1, pos = 0;
        u32 l_name = 0, mapq = 0, n_cig = 0, flag = 4, l_seq = 0;
        if (live) {
            ref = (int)bs_ld32(p + 4); pos = (int)bs_ld32(p + 8);
            l_name = (u32)(unsigned char)p[12]; mapq = (u32)(unsigned char)p[13];
            n_cig = (u32)(unsigned char)p[16] | ((u32)(unsigned char)p[17] << 8);
            flag = (u32)(unsigned char)p[18] | ((u32)(unsigned char)p[19] << 8);
            l_seq = bs_ld32(p + 20);
            if (36ull + l_name + 4ull * n_cig + ((u64)l_seq + 1) / 2 + l_seq > (u64)l) live = false;
        }
        if (live && ref >= par.n_chrom) live = false;
        const bool mapped = live && ref >= 0 && !(flag & 4u) && n_cig > 0;
        const char* const cg = p + 36 + l_name;
        u64 span = 0;
        if (mapped)
            for (u32 k = (u32)gl; k < n_cig; k += METH_GROUP) { const u32 c = bs_ld32(cg + 4 * (u64)k); if ((0x18du >> (c & 15u)) & 1u) span += c >> 4; }
        for (int d = METH_GROUP / 2; d; d >>= 1) {
            const u32 lo = (u32)__shfl_xor((int)(u32)span, d), hi = (u32)__shfl_xor((int)(u32)(span >> 32), d);
            span += ((u64)hi << 32) | lo;
        }
        long s_lo = 0, s_hi = 0;
        bool counts = mapped;
        if (mapped) {
            s_lo = (long)chrom_start[ref]; s_hi = (long)chrom_start[ref + 1];
            if (pos < 0 || (u64)pos + span > (u64)(s_hi - s_lo)) counts = false;
        }
        counts = counts && !(flag & 0xF00u) && mapq >= par.min_mapq && (!(flag & 1u) || (flag & 2u));
        const bool ob = (flag & 1u) ? (((flag & 0x40u) && (flag & 0x10u)) || ((flag & 0x80u) && !(flag & 0x10u))) : (flag & 0x10u) != 0;
        const long a0 = s_lo + pos, a1 = a0 + (long)span;
        const u32 cw = (counts && clip) ? clip[i] : 0;
        const long c_lo = a0 + (long)(cw >> 16), c_hi = c_lo + (long)(cw & 0xffffu);
        const bool all_m = counts && n_cig == 1 && ((0x181u >> (bs_ld32(cg) & 15u)) & 1u);
        const char* const sq = cg + 4 * (u64)n_cig;
        const char* const ql = sq + ((u64)l_seq + 1) / 2;
        const u32 want_m = ob ? 4u : 2u, want_u = ob ? 1u : 8u;
        const u32 row0 = (meth_mate(flag) * 2u + (ob ? 1u : 0u)) * 6u;              // + 2 context + methylated
        const long W0 = a0 >> 5, W1 = counts && span ? (a1 - 1) >> 5 : W0 - 1;
        for (long W = W0 + gl; W <= W1; W += METH_GROUP) {
            u32 m[6];
            meth_masks(gen2p, W, s_lo, s_hi, m);
            const u32 m0 = m[ob ? 3 : 0], m1 = m[ob ? 4 : 1];
            u32 sel = 0;
#pragma unroll
            for (int x = 0; x < 3; x++) if ((par.contexts >> x) & 1u) sel |= m[(ob ? 3 : 0) + x];
            sel &= (u32)meth_range(32 * W, a0, a1, 32) & ~(u32)meth_range(32 * W, c_lo, c_hi, 32);
            u32 k = 0; long r_at = 0, i_at = 0;
            while (sel) {
                const int b = __ffs((int)sel) - 1;
                sel &= sel - 1;
                const long ro = 32 * W + b - a0;
                long ri = -1;
                if (all_m) ri = ro;
                else {
                    while (k < n_cig) {
                        const u32 c = bs_ld32(cg + 4 * (u64)k);
                        const u32 op = c & 15u; const long ln = (long)(c >> 4);
                        const bool on_ref = (0x18du >> op) & 1u, on_read = (0x193u >> op) & 1u;
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
                if (code != want_m && code != want_u) continue;
                const u32 row = row0 + 2u * (((m0 >> b) & 1u) ? 0u : ((m1 >> b) & 1u) ? 1u : 2u) + (code == want_m ? 1u : 0u);
                const long cy = meth_cycle(flag, l_seq, ri);                        // 0 .. l_seq - 1
                if (cy < METH_MBIAS_LDS) atomicAdd(&tally[row * METH_MBIAS_LDS + (u32)cy], 1u);
                else atomicAdd(&table[row * BMBS_MBIAS_CYCLES + (u32)(cy < BMBS_MBIAS_CYCLES ? cy : BMBS_MBIAS_CYCLES - 1)], 1ull);
            }
        }
    }
    __syncthreads();
    for (int x = (int)threadIdx.x; x < METH_MBIAS_ROWS * METH_MBIAS_LDS; x += 256) {
        const u32 v = tally[x];
        if (v) atomicAdd(&table[(x / METH_MBIAS_LDS) * BMBS_MBIAS_CYCLES + x % METH_MBIAS_LDS], (unsigned long long)v);
    }
}

// *end = the largest r in (start, n] with eoff[r] - eoff[start] <= cap, start + 1 at the least (one thread)
__global__ void k_meth_cut(const u64* __restrict__ eoff, long start, long n, u64 cap, u64* __restrict__ end)
{
    if (threadIdx.x || blockIdx.x) return;
    const u64 lim = eoff[start] + cap;
    long lo = start + 1, hi = n;                                           // eoff[lo] may exceed lim (a single record's events)
    while (lo < hi) { const long mid = (lo + hi + 1) >> 1; if (eoff[mid] <= lim) lo = mid; else hi = mid - 1; }
    *end = (u64)lo;
}

// sorted (key, value): wave[w] = the run heads among entries 64 w .. 64 w + 63, m[i] / u[i] = the two halves of value i
__global__ void __launch_bounds__(256)
k_meth_heads(const u64* __restrict__ key, const u64* __restrict__ val, long n, u32* __restrict__ wave, u32* __restrict__ m, u32* __restrict__ u)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool head = false;
    if (i < n) {
        head = i == 0 || key[i] != key[i - 1];
        const u64 v = val[i];
        m[i] = (u32)(v >> 32); u[i] = (u32)v;
    }
    const u64 bal = __ballot(head);
    if ((threadIdx.x & 63) == 0 && i < n) wave[i >> 6] = (u32)__popcll(bal);
}

// hpos[h] = the entry of run head h: hoff = the exclusive scan of wave[]
__global__ void __launch_bounds__(256)
k_meth_hpos(const u64* __restrict__ key, long n, const u64* __restrict__ hoff, u32* __restrict__ hpos)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool head = i < n && (i == 0 || key[i] != key[i - 1]);
    const u64 bal = __ballot(head);
    if (head) hpos[hoff[i >> 6] + (u64)__popcll(bal & (((u64)1 << (threadIdx.x & 63)) - 1))] = (u32)i;
}

// site h = the run from hpos[h] to the next head (n behind the last): its sums from the scans ms / us of m[] / u[] (clamped to 32 bits).
// site != NULL: the bmbs_methyl_site, its context and strand from the genome; else the (key, value) pair at okey / oval
__global__ void __launch_bounds__(256)
k_meth_sites(const u64* __restrict__ gen2p, const u64* __restrict__ chrom_start, const u64* __restrict__ key, const u32* __restrict__ hpos, long n_heads, long n,
             const u64* __restrict__ ms, const u64* __restrict__ us, int pos_bits, bmbs_methyl_site* __restrict__ site, u64* __restrict__ okey, u64* __restrict__ oval)
{
    const long h = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= n_heads) return;
    const long a = hpos[h], b = h + 1 < n_heads ? (long)hpos[h + 1] : n;
    const u64 k = key[a];
    u64 me = ms[b] - ms[a], un = us[b] - us[a];
    me = me > 0xffffffffull ? 0xffffffffull : me; un = un > 0xffffffffull ? 0xffffffffull : un;
    if (!site) { okey[h] = k; oval[h] = (me << 32) | un; return; }
    const int ref = (int)(k >> pos_bits);
    const long pos = (long)(k & (((u64)1 << pos_bits) - 1));
    const long lo = (long)chrom_start[ref], hi = (long)chrom_start[ref + 1];
    u32 m[6];
    meth_masks(gen2p, (lo + pos) >> 5, lo, hi, m);
    u32 kind = 0;
#pragma unroll
    for (int x = 0; x < 6; x++) if ((m[x] >> ((lo + pos) & 31)) & 1u) kind = (u32)(x % 3) | ((u32)(x / 3) << 2);
    bmbs_methyl_site s;
    s.ref = ref; s.pos = (int)pos; s.meth = (u32)me; s.unmeth = (u32)un; s.kind = kind; s.pad = 0;
    site[h] = s;
}

// What one thread learns of output line `line` of a text call (bam_raw / sam_off / sam_len): ok = there, mapped, with a CIGAR that
// lies inside the record; its refID, position and reference span
struct MethLine { bool ok; int ref; long pos, span; u32 flag; };
DEVI MethLine meth_line(const char* __restrict__ raw, const u64* __restrict__ off, const u32* __restrict__ len, long line)
{
    MethLine r = {false, -1, 0, 0, 0};
    const u32 l = len[line];
    if (l < 36) return r;
    const char* const p = raw + off[line];
    const u32 l_name = (u32)(unsigned char)p[12];
    const u32 n_cig = (u32)(unsigned char)p[16] | ((u32)(unsigned char)p[17] << 8);
    r.flag = (u32)(unsigned char)p[18] | ((u32)(unsigned char)p[19] << 8);
    r.ref = (int)bs_ld32(p + 4); r.pos = (long)(int)bs_ld32(p + 8);
    if ((r.flag & 4u) || n_cig == 0 || r.ref < 0 || 36ull + l_name + 4ull * n_cig > (u64)l) return r;
    for (u32 k = 0; k < n_cig; k++) { const u32 c = bs_ld32(p + 36 + l_name + 4 * (u64)k); if ((0x18du >> (c & 15u)) & 1u) r.span += (long)(c >> 4); }
    r.ok = true;
    return r;
}

// clip[j] of the j-th record in sorted order (idx[j] = its output line; lines 2p and 2p + 1 are the records of pair p):
// (beg - pos) << 16 | (end - beg) for the intersection [beg, end) of its reference span with its mate's, for a read-2 record (flag 0x80)
// only and only when both are usable and share refID, else 0.  info[0] = ~(the first j whose offset or length does not fit 16 bits)
__global__ void __launch_bounds__(256)
k_meth_clip(const char* __restrict__ raw, const u64* __restrict__ off, const u32* __restrict__ len, const u32* __restrict__ idx, long n, int paired,
            u32* __restrict__ clip, u32* __restrict__ info)
{
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    u32 c = 0;
    if (paired) {
        const long line = (long)idx[j];
        const MethLine me = meth_line(raw, off, len, line);
        if (me.ok && (me.flag & 0x80u)) {
            const MethLine ma = meth_line(raw, off, len, line ^ 1);
            if (ma.ok && ma.ref == me.ref) {
                const long beg = me.pos > ma.pos ? me.pos : ma.pos;
                const long e1 = me.pos + me.span, e2 = ma.pos + ma.span;
                const long end = e1 < e2 ? e1 : e2;
                if (end > beg) {
                    if (beg - me.pos >= 65536 || end - beg >= 65536) atomicMax(&info[0], ~(u32)j);
                    else c = ((u32)(beg - me.pos) << 16) | (u32)(end - beg);
                }
            }
        }
    }
    clip[j] = c;
}
#endif
