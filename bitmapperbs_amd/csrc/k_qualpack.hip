// bitmapperbs_amd/csrc/k_qualpack.hip -- packed quality classes (bmbs_map_*_packedq) -> the quality bytes the mapping kernels read
// (one stage of the mapping path; included by bmbs_kernels.hip: no translation unit of its own)
// ================================================================================================
// A quality byte means one thing to the mapping path: the index of pen_lut[256] (mismatch_penalty).  That table takes few distinct
// values, so the caller's reader sends a 4-bit penalty CLASS per base (bmbs_pack_quals: 16 classes per u64, 80 bytes for a 150-base
// read instead of 160) and this kernel writes, once per chunk, the byte rows the alignment and finalize kernels have always read:
// for class c the representative byte rep[c], the smallest byte with pen_lut[rep[c]] == penalty_of[c].  None of those kernels
// changes.
//
// Streaming shape: the device stride of a quality row is ds = 16 * Wq bytes (Wq = ceil(L / 16) words per packed row), so one thread
// takes one u64 and writes one 16-byte piece, and thread j's piece is out[j] -- the output of both mates is one dense run each.  The
// caller's rows may be further apart than Wq words (qwords): only the read address knows.  rep[16] travels as two u64 kernel
// arguments (scalar registers); a byte is picked by v_perm_b32 out of the low / high eight entries and the class's top bit chooses
// between the two.  No LDS, no scratch.
struct QualRep { u64 lo, hi; };      // rep[c] = byte c of lo (c < 8), byte c - 8 of hi

// four classes (16 bits) -> their four representative bytes
DEVI u32 qual_rep4(u32 x16, const QualRep& rep)
{
    u32 v = x16 & 0xffffu;
    v = (v | (v << 8)) & 0x00ff00ffu;
    v = (v | (v << 4)) & 0x0f0f0f0fu;                         // one class per byte
    const u32 sel = v & 0x07070707u;
    const u32 top = ((v >> 3) & 0x01010101u) * 0xffu;         // 0xff where the class is 8..15
    const u32 a = __builtin_amdgcn_perm((u32)(rep.lo >> 32), (u32)rep.lo, sel);
    const u32 b = __builtin_amdgcn_perm((u32)(rep.hi >> 32), (u32)rep.hi, sel);
    return (a & ~top) | (b & top);
}

// q1 / q2: n packed rows each, qwords words apart (q2 null: single end); out1 / out2: n rows of Wq 16-byte pieces
__global__ void __launch_bounds__(256) k_qual_expand(const u64* __restrict__ q1, const u64* __restrict__ q2, int qwords, int Wq, long n, QualRep rep,
                                                     uint4* __restrict__ out1, uint4* __restrict__ out2)
{
    const u64 per = (u64)n * (u64)Wq;
    const u64 total = q2 ? 2 * per : per;
    const u64 step = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const bool second = i >= per;
        const u64 j = second ? i - per : i;
        u64 at = j;                                               // rows exactly Wq words apart: the input is one dense run too
        if (qwords != Wq) { const u64 r = j / (u32)Wq; at = r * (u64)qwords + (j - r * (u32)Wq); }
        const u64 x = (second ? q2 : q1)[at];
        uint4 o;
        o.x = qual_rep4((u32)x, rep);
        o.y = qual_rep4((u32)(x >> 16), rep);
        o.z = qual_rep4((u32)(x >> 32), rep);
        o.w = qual_rep4((u32)(x >> 48), rep);
        (second ? out2 : out1)[j] = o;
    }
}
