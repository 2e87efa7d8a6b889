// bitmapperbs_amd/csrc/k_markdup.hip -- PCR duplicate marking of BAM records on the device (`--bam --sort --markdup`, bmbs_bam_dup_sigs,
// bmbs_text_sorted_dup, bmbs_dup_select).  The rule is Picard's pair-level one (include/bmbs.h; tests/markdup_spec.py restates it).
//
// A template is one record (single end) or the two records 2p, 2p + 1 of a pair; record i = len[i] bytes at raw + off[i] (len 0: no
// record), exactly the layout a text call leaves behind (bam_raw / sam_off / sam_len) before the sort tears the mates apart.
//   k_dup_sig     template -> its 24-byte signature: both 5' ends, orientation, the sum of the base qualities >= 15
//   k_dup_bits    the OR of every sort key of the three passes below: which key bits can be set at all
//   k_dup_keys    the key of one pass, read through the order the previous pass left
//   (pair sort)   rocPRIM radix_sort_pairs over (key, template), stable, three passes from the least significant field up:
//                 orient << 32 | ~score  (best score first, equal scores in input order), then (ref_hi, pos_hi), then (ref_lo, pos_lo)
//   k_dup_heads   every entry against its predecessor: the first of a run of equal signatures stays, the others are duplicates
//   k_dup_tmpl    the template of every record of a sorted text call, in sorted order
// No kernel here uses LDS; every store is an ordinary vector store.
#ifndef K_MARKDUP_HIP
#define K_MARKDUP_HIP

#define DUP_GROUP 16                      // lanes per template (k_bam_gather's: a record's qualities go in 16-byte units, one per lane)

// the qualities that count among the 4 bytes of w, which are bytes i0 .. i0 + 3 of a record's n qualities (bytes outside 0 .. n - 1
// belong to its neighbours): those >= 15 (Picard's SUM_OF_BASE_QUALITIES); 0xff = "no quality" counts as 0
DEVI u32 dup_q4(u32 w, long i0, long n)
{
    u32 s = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const u32 q = (w >> (8 * b)) & 255u;
        const long i = i0 + b;
        s += (i >= 0 && i < n && q >= 15u && q != 255u) ? q : 0u;
    }
    return s;
}

// What the DUP_GROUP lanes of a template learn of one of its records.  ok: the record is there, mapped, primary and has a CIGAR.
// rl / sc: THIS lane's share of the reference length and of the score (the caller adds the lanes up); lead / trail: the clipped
// lengths at the two ends (lane 0 of the group only).
struct DupRec { bool ok; u32 ref, pos, rev, r1, rl, sc, lead, trail; };

// info[0] = ~(the first record whose length is below 36 or is not its block_size + 4), info[1] = ~(the first record whose read name,
// CIGAR, sequence and qualities do not fit its length) (0: none): nothing is read behind a record
DEVI DupRec dup_record(const char* __restrict__ raw, const u64* __restrict__ off, const u32* __restrict__ len, long i, int gl, u32* __restrict__ info)
{
    DupRec r = {false, 0, 0, 0, 0, 0, 0, 0, 0};
    const u32 l = len[i];
    if (l == 0) return r;
    if (l < 36) { if (gl == 0) atomicMax(&info[0], ~(u32)i); return r; }
    const char* const p = raw + off[i];
    if (bs_ld32(p) + 4u != l) { if (gl == 0) atomicMax(&info[0], ~(u32)i); return r; }
    r.ref = bs_ld32(p + 4); r.pos = bs_ld32(p + 8);
    const u32 l_name = (u32)(unsigned char)p[12];
    const u32 n_cig = (u32)(unsigned char)p[16] | ((u32)(unsigned char)p[17] << 8);
    const u32 flag = (u32)(unsigned char)p[18] | ((u32)(unsigned char)p[19] << 8);
    const u32 l_seq = bs_ld32(p + 20);
    const u64 q_at = 36ull + l_name + 4ull * n_cig + ((u64)l_seq + 1) / 2;
    if (q_at + l_seq > (u64)l) { if (gl == 0) atomicMax(&info[1], ~(u32)i); return r; }
    if ((flag & 0x904u) || n_cig == 0) return r;             // unmapped, secondary, supplementary, no CIGAR: no part in a signature
    r.ok = true;
    r.rev = (flag >> 4) & 1u; r.r1 = (flag >> 6) & 1u;
    const char* const cg = p + 36 + l_name;
    for (u32 k = (u32)gl; k < n_cig; k += DUP_GROUP) {
        const u32 c = bs_ld32(cg + 4 * (u64)k);
        if ((0x18du >> (c & 15u)) & 1u) r.rl += c >> 4;      // M D N = X consume reference
    }
    if (gl == 0) {
        if (!r.rev) {
            for (u32 k = 0; k < n_cig; k++) { const u32 c = bs_ld32(cg + 4 * (u64)k); if ((c & 15u) != 4u && (c & 15u) != 5u) break; r.lead += c >> 4; }
        } else {
            for (u32 k = n_cig; k > 0; k--) { const u32 c = bs_ld32(cg + 4 * (u64)(k - 1)); if ((c & 15u) != 4u && (c & 15u) != 5u) break; r.trail += c >> 4; }
        }
    }
    // the qualities in 16-byte units at SOURCE alignment, a unit per lane; the first and the last unit reach into the neighbouring
    // bytes (the sequence in front, the next record or the buffer's padding behind), which dup_q4 leaves out
    const char* const q = p + q_at;
    const long lead = (long)((uintptr_t)q & 15u);
    const char* const qa = q - lead;
    const long nu = (lead + (long)l_seq + 15) >> 4;
    for (long u = gl; u < nu; u += DUP_GROUP) {
        const uint4 v = *reinterpret_cast<const uint4*>(qa + 16 * u);
        const long i0 = 16 * u - lead;
        r.sc += dup_q4(v.x, i0, (long)l_seq) + dup_q4(v.y, i0 + 4, (long)l_seq) + dup_q4(v.z, i0 + 8, (long)l_seq) + dup_q4(v.w, i0 + 12, (long)l_seq);
    }
    return r;
}

// the 5' end of a usable record (rl summed over the group): forward pos - leading clips, reverse pos + reference length + trailing clips - 1
DEVI int dup_five_prime(const DupRec& r) { return (int)(r.rev ? r.pos + r.rl + r.trail - 1u : r.pos - r.lead); }

// the signature of a template from its record(s), rl and sc summed over the group (b: the second record of a pair, !ok otherwise)
DEVI bmbs_dup_sig dup_compose(const DupRec& a, const DupRec& b)
{
    bmbs_dup_sig s;
    s.ref_lo = s.pos_lo = s.ref_hi = s.pos_hi = -1; s.orient = BMBS_DUP_NONE; s.score = 0;
    if (a.ok && b.ok) {
        const int ca = dup_five_prime(a), cb = dup_five_prime(b);
        // lo = the smaller end by (refID, 5' coordinate); a tie goes to the forward strand, a further tie to read 1
        bool a_lo;
        if ((int)a.ref != (int)b.ref) a_lo = (int)a.ref < (int)b.ref;
        else if (ca != cb) a_lo = ca < cb;
        else if (a.rev != b.rev) a_lo = !a.rev;
        else a_lo = a.r1 || !b.r1;
        const DupRec& lo = a_lo ? a : b; const DupRec& hi = a_lo ? b : a;
        s.ref_lo = (int)lo.ref; s.pos_lo = a_lo ? ca : cb; s.ref_hi = (int)hi.ref; s.pos_hi = a_lo ? cb : ca;
        s.orient = lo.rev | (hi.rev << 1) | (lo.r1 << 2) | 8u;
        s.score = a.sc + b.sc;
    } else if (a.ok || b.ok) {
        const DupRec& r = a.ok ? a : b;
        s.ref_lo = (int)r.ref; s.pos_lo = dup_five_prime(r); s.orient = r.rev; s.score = r.sc;
    }
    return s;
}

__global__ void __launch_bounds__(256)
k_dup_sig(const char* __restrict__ raw, const u64* __restrict__ off, const u32* __restrict__ len, int paired, long n_tmpl, bmbs_dup_sig* __restrict__ sig,
          u32* __restrict__ info)
{
    const long t = ((long)blockIdx.x * blockDim.x + threadIdx.x) / DUP_GROUP;
    const int gl = threadIdx.x % DUP_GROUP;
    DupRec a = {false, 0, 0, 0, 0, 0, 0, 0, 0}, b = a;
    if (t < n_tmpl) {
        a = dup_record(raw, off, len, paired ? 2 * t : t, gl, info);
        if (paired) b = dup_record(raw, off, len, 2 * t + 1, gl, info);
    }
    // the lanes' shares added up within the group (every lane of the wave takes part)
    for (int d = DUP_GROUP / 2; d; d >>= 1) {
        a.rl += (u32)__shfl_xor((int)a.rl, d); a.sc += (u32)__shfl_xor((int)a.sc, d);
        b.rl += (u32)__shfl_xor((int)b.rl, d); b.sc += (u32)__shfl_xor((int)b.sc, d);
    }
    if (t >= n_tmpl || gl != 0) return;
    sig[t] = dup_compose(a, b);
}

DEVI u64 dup_key(const bmbs_dup_sig& s, int pass)
{
    if (pass == 0) return ((u64)s.orient << 32) | (u64)(0xffffffffu - s.score);
    if (pass == 1) return ((u64)(u32)s.ref_hi << 32) | (u64)(u32)s.pos_hi;
    return ((u64)(u32)s.ref_lo << 32) | (u64)(u32)s.pos_lo;
}

// bits[pass] = the OR of the pass's keys over all entries: one atomic per wave and word
__global__ void __launch_bounds__(256)
k_dup_bits(const bmbs_dup_sig* __restrict__ sig, long n, unsigned long long* __restrict__ bits)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    u64 k[3] = {0, 0, 0};
    if (i < n) { const bmbs_dup_sig s = sig[i]; k[0] = dup_key(s, 0); k[1] = dup_key(s, 1); k[2] = dup_key(s, 2); }
    for (int d = 32; d; d >>= 1)
#pragma unroll
        for (int p = 0; p < 3; p++) {
            const u32 lo = (u32)__shfl_xor((int)(u32)k[p], d), hi = (u32)__shfl_xor((int)(u32)(k[p] >> 32), d);
            k[p] |= ((u64)hi << 32) | lo;
        }
    if ((threadIdx.x & 63) == 0)
        for (int p = 0; p < 3; p++) if (k[p]) atomicOr(&bits[p], (unsigned long long)k[p]);
}

// key[j] = the pass's key of entry order[j] (order NULL: j itself, and idx[j] = j is written)
__global__ void __launch_bounds__(256)
k_dup_keys(const bmbs_dup_sig* __restrict__ sig, const u32* __restrict__ order, long n, int pass, u64* __restrict__ key, u32* __restrict__ idx)
{
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const u32 i = order ? order[j] : (u32)j;
    key[j] = dup_key(sig[i], pass);
    if (!order) idx[j] = (u32)j;
}

// order[]: the entries sorted by (ref_lo, pos_lo, ref_hi, pos_hi, orient, best score first, input order).  dup[i] = 1 when entry i has
// its predecessor's signature (the first of a run stays); entries without a signature are never marked.  *n_dup: one atomic per wave
__global__ void __launch_bounds__(256)
k_dup_heads(const bmbs_dup_sig* __restrict__ sig, const u32* __restrict__ order, long n, uint8_t* __restrict__ dup, u32* __restrict__ n_dup)
{
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool d = false;
    if (j < n) {
        const u32 i = order[j];
        const bmbs_dup_sig s = sig[i];
        if (j > 0 && !(s.orient & BMBS_DUP_NONE)) {
            const bmbs_dup_sig p = sig[order[j - 1]];
            d = s.ref_lo == p.ref_lo && s.pos_lo == p.pos_lo && s.ref_hi == p.ref_hi && s.pos_hi == p.pos_hi && s.orient == p.orient;
        }
        dup[i] = d ? 1 : 0;
    }
    const u32 nd = (u32)__popcll(__ballot(d));
    if ((threadIdx.x & 63) == 0 && nd) atomicAdd(n_dup, nd);
}

// tmpl[j] = the template of the j-th record of a sorted text call: its line, shifted right by one for pairs
__global__ void __launch_bounds__(256)
k_dup_tmpl(const u32* __restrict__ idx, long n, int shift, u32* __restrict__ tmpl)
{
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) tmpl[j] = idx[j] >> shift;
}
#endif
