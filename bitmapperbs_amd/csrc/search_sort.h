// bitmapperbs_amd/csrc/search_sort.h -- the host side of --bam --sort: the store of pass 1, the plan and the staging of pass 2, the .bai
// index and the methylation files (bmbs_search.cpp)
#pragma once
#include "search_util.h"
#include <zlib.h>
#include <algorithm>
#include <cctype>
#include <cstdint>
#include <map>
#include <cstdio>
#include <utility>

// BGZF: independent gzip members of at most 0xff00 input bytes with the BC extra field (SAM spec 4.1)
inline void bgzf_append(const char* in, size_t n, std::vector<char>& out)
{
    size_t done = 0;
    do {
        const size_t chunk = std::min<size_t>(n - done, 0xff00);
        const size_t at = out.size();
        out.resize(at + 18 + compressBound((uLong)chunk) + 8);
        z_stream zs; memset(&zs, 0, sizeof(zs));
        deflateInit2(&zs, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
        zs.next_in = (Bytef*)(in + done); zs.avail_in = (uInt)chunk;
        zs.next_out = (Bytef*)(out.data() + at + 18); zs.avail_out = (uInt)(out.size() - at - 18 - 8);
        deflate(&zs, Z_FINISH);
        const size_t clen = zs.total_out;
        deflateEnd(&zs);
        static const unsigned char hdr[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        memcpy(out.data() + at, hdr, 16);
        const uint16_t bsize = (uint16_t)(clen + 25);
        out[at + 16] = (char)bsize; out[at + 17] = (char)(bsize >> 8);
        const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef*)(in + done), (uInt)chunk);
        char* t = out.data() + at + 18 + clen;
        t[0] = (char)crc; t[1] = (char)(crc >> 8); t[2] = (char)(crc >> 16); t[3] = (char)(crc >> 24);
        t[4] = (char)chunk; t[5] = (char)(chunk >> 8); t[6] = (char)(chunk >> 16); t[7] = (char)(chunk >> 24);
        out.resize(at + 18 + clen + 8);
        done += chunk;
    } while (done < n);
}

// ---- --bam --sort: one coordinate-sorted BAM file.  The device sorts (k_bamsort.hip); the host only cuts and concatenates. --------------
// Pass 1 (while mapping): every batch comes back as uncompressed records sorted by key (BMBS_TEXT_BAM_SORTED) with its key and length
// arrays (bmbs_text_sorted_index).  The key space is cut into fine bins of equal genomic length plus one for records without a
// reference; a batch is cut at the bin edges by binary search over its keys and every slice is appended to its bin's store, in
// Batch.seq order (the writer takes the batches in that order), so a bin holds its records in the order of the unsorted file.
// Pass 2 (after the last batch): bins in key order, grouped into calls of at most a byte budget, go through bmbs_bam_sort -- a stable
// sort, so equal keys keep the unsorted file's order whichever context mapped them first -- and come back as BGZF blocks.
inline uint64_t bam_key_of(const char* r)
{
    uint32_t ref, pos; uint16_t flag;
    memcpy(&ref, r + 4, 4); memcpy(&pos, r + 8, 4); memcpy(&flag, r + 18, 2);
    return ((uint64_t)ref << 32) | ((uint64_t)(uint32_t)(pos + 1u) << 1) | (uint64_t)((flag >> 4) & 1u);
}
// --markdup: beside every record the id of its template (the batch's running template base + the template's index in the batch, batches
// in Batch.seq order), and a second store of the templates' signatures (bmbs_text_sorted_dup), cut at the SAME edges by the key of
// (ref_lo, pos_lo) -- templates with equal signatures share a bin, in input order.  Between the passes bmbs_dup_select runs over groups
// of signature bins and sets a bit per losing template; pass 2 ORs 0x04 into byte 19 (flag 0x400) of the staged copy of its records.
// --methyl, pairs: beside every record its mate-overlap clip (bmbs_text_sorted_clip), which pass 2 hands to bmbs_bam_sort_methyl.
struct SortBin { std::vector<char> rec; std::vector<uint32_t> len; std::vector<uint64_t> tid; std::vector<uint32_t> clip; };
struct SigBin { std::vector<bmbs_dup_sig> sig; std::vector<uint64_t> gid; };
struct SortStore {
    std::vector<uint64_t> edge;                  // bin k holds the keys in [edge[k], edge[k + 1]); the last bin: refID -1
    std::vector<SortBin> bin;
    std::vector<SigBin> sbin;                    // --markdup: the signatures, by the same edges
    size_t bytes = 0, cap = 0;                   // record bytes + 4 per record (--markdup: + 8, and 32 per signature; --methyl of pairs: + 4) held / allowed (--sort-mem)
    long records = 0, templates = 0, with_sig = 0;
    void init(const bmbs_index_view& v, long want_bins)
    {
        uint64_t G = 0;
        for (int i = 0; i < v.n_chrom; i++) G += v.chrom_len[i];
        const uint64_t nb = (uint64_t)std::max(1l, std::min(want_bins, 1l << 20));
        const uint64_t W = std::max<uint64_t>(1, (G + nb - 1) / nb);
        int ref = 0; uint64_t ref_start = 0;
        edge.clear();
        for (uint64_t lin = 0; lin < G || edge.empty(); lin += W) {
            while (ref + 1 < v.n_chrom && lin >= ref_start + v.chrom_len[ref]) { ref_start += v.chrom_len[ref]; ref++; }
            edge.push_back(lin == 0 ? 0 : ((uint64_t)(uint32_t)ref << 32) | ((lin - ref_start + 1) << 1));
        }
        edge.push_back((uint64_t)0xffffffffu << 32);
        bin.assign(edge.size(), SortBin());
        sbin.assign(edge.size(), SigBin());
        edge.push_back(~(uint64_t)0);
    }
    size_t bin_of(uint64_t key) const { return (size_t)(std::upper_bound(edge.begin(), edge.end() - 1, key) - edge.begin()) - 1; }
    // the sorted records of one batch (tmpl: the template of each within the batch, base: the batch's first template id; --markdup;
    // clip: the clip of each; --methyl of pairs); false: the store's cap would be exceeded
    bool add(Pool& pool, const char* recs, size_t nbytes, const uint64_t* key, const uint32_t* len, size_t n, const uint32_t* tmpl = nullptr, uint64_t base = 0,
             const uint32_t* clip = nullptr)
    {
        const size_t per = (tmpl ? 12 : 4) + (clip ? 4 : 0);
        if (bytes + nbytes + per * n > cap) return false;
        struct Slice { size_t k, lo, hi; };
        std::vector<Slice> sl;
        for (size_t i = 0; i < n;) {
            const size_t k = bin_of(key[i]);
            const size_t hi = k + 1 < bin.size() ? (size_t)(std::lower_bound(key + i, key + n, edge[k + 1]) - key) : n;
            sl.push_back({k, i, hi});
            i = hi;
        }
        std::vector<uint64_t> off(n + 1);
        off[0] = 0;
        for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + len[i];
        const int T = std::max(1, std::min<int>(pool.size(), (int)sl.size()));
        pool.run(T, [&](int t) {
            for (size_t j = (size_t)t; j < sl.size(); j += (size_t)T) {
                SortBin& b = bin[sl[j].k];
                b.rec.insert(b.rec.end(), recs + off[sl[j].lo], recs + off[sl[j].hi]);
                b.len.insert(b.len.end(), len + sl[j].lo, len + sl[j].hi);
                if (tmpl) for (size_t i = sl[j].lo; i < sl[j].hi; i++) b.tid.push_back(base + tmpl[i]);
                if (clip) b.clip.insert(b.clip.end(), clip + sl[j].lo, clip + sl[j].hi);
            }
        });
        bytes += nbytes + per * n; records += (long)n;
        return true;
    }
    // the signatures of one batch's templates, in batch order; those without a signature are counted and not kept
    bool add_sigs(Pool& pool, const bmbs_dup_sig* sig, size_t nt, uint64_t base)
    {
        std::vector<uint32_t> bi(nt);
        const int T = std::max(1, std::min<int>(pool.size(), (int)(nt / 4096) + 1));
        std::vector<size_t> kept((size_t)T, 0);
        pool.run(T, [&](int t) {
            for (size_t i = nt * (size_t)t / (size_t)T; i < nt * ((size_t)t + 1) / (size_t)T; i++) {
                if (sig[i].orient & BMBS_DUP_NONE) { bi[i] = ~0u; continue; }
                bi[i] = (uint32_t)bin_of(((uint64_t)(uint32_t)sig[i].ref_lo << 32) | ((uint64_t)(uint32_t)(sig[i].pos_lo + 1) << 1));
                kept[(size_t)t]++;
            }
        });
        size_t ns = 0;
        for (size_t k : kept) ns += k;
        if (bytes + 32 * ns > cap) return false;
        pool.run(T, [&](int t) {
            for (size_t i = 0; i < nt; i++)
                if (bi[i] != ~0u && bi[i] % (uint32_t)T == (uint32_t)t) { SigBin& b = sbin[bi[i]]; b.sig.push_back(sig[i]); b.gid.push_back(base + i); }
        });
        bytes += 32 * ns; templates += (long)nt; with_sig += (long)ns;
        return true;
    }
};
// ---- --bam --sort --bai: the .bai index (SAM specification section 5.2) of the sorted file, from the same run ------------------------------
// Every pass-2 call leaves the pieces of its own blocks on the device side (bmbs_bam_sort_index: chunks, 16 kb windows, per-reference
// totals; virtual offsets relative to the call's first block).  The writing thread knows the file offset B at which it appends a
// call's blocks, adds B << 16 and merges in call order:
//   chunks of one (ref, bin) one behind the other; two are joined when the earlier one's end is the later one's beg (a run of records
//   of one bin that went on across the call boundary); a window keeps the first call's offset; a reference keeps the first beg, the
//   last end and the summed counts.
// The file written is the NORMAL FORM, so that a BAM file has exactly one index: n_ref of the header; bins in ascending number with
// their chunks in file order, then the pseudo-bin 37450 with (ref.beg, ref.end) and (n_mapped, n_unmapped); a linear index of 1 + the
// last window touched, empty windows filled with the previous window's value, leading ones with ref.beg (htslib's update_loff); the
// count of records without a reference.  Sequences without records: n_bin = 0, n_intv = 0.  htslib's compress_binning (folding small
// bins into their parents, a size optimisation no reader depends on) is not done.
struct BaiPieces {
    std::vector<bmbs_bai_chunk> chunk; std::vector<bmbs_bai_win> win; std::vector<bmbs_bai_ref> ref;
    int64_t n_chunk = 0, n_win = 0, n_ref = 0; uint64_t n_no_coor = 0;
    // the pieces of ctx's last bmbs_bam_sort call
    bool fetch(bmbs_ctx* ctx)
    {
        for (int attempt = 0; attempt < 2; attempt++) {
            const int rc = bmbs_bam_sort_index(ctx, chunk.data(), (int64_t)chunk.size(), &n_chunk, win.data(), (int64_t)win.size(), &n_win, ref.data(), (int64_t)ref.size(),
                                               &n_ref, &n_no_coor);
            if (rc == BMBS_OK) return true;
            if (rc != BMBS_ENOMEM || attempt) return false;
            if ((size_t)n_chunk > chunk.size()) chunk.resize((size_t)n_chunk + (size_t)n_chunk / 8);
            if ((size_t)n_win > win.size()) win.resize((size_t)n_win + (size_t)n_win / 8);
            if ((size_t)n_ref > ref.size()) ref.resize((size_t)n_ref);
        }
        return false;
    }
};
struct BaiIndex {
    struct Ref {
        std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins;
        std::vector<uint64_t> lin;                   // window -> offset; ~0: no mapped record overlaps it
        bool any = false; uint64_t beg = 0, end = 0, n_mapped = 0, n_unmapped = 0;
    };
    std::vector<Ref> refs;
    uint64_t n_no_coor = 0;
    void init(size_t n_ref) { refs.assign(n_ref, Ref()); }
    // the pieces of the call whose blocks start at file offset B; false: a reference index outside the header's
    bool add(const BaiPieces& p, uint64_t B)
    {
        const uint64_t sh = B << 16;
        for (int64_t i = 0; i < p.n_chunk; i++) {
            const bmbs_bai_chunk& c = p.chunk[(size_t)i];
            if (c.ref < 0 || (size_t)c.ref >= refs.size()) return false;
            auto& v = refs[(size_t)c.ref].bins[c.bin];
            if (!v.empty() && v.back().second == c.beg + sh) v.back().second = c.end + sh;
            else v.push_back({c.beg + sh, c.end + sh});
        }
        for (int64_t i = 0; i < p.n_win; i++) {
            const bmbs_bai_win& w = p.win[(size_t)i];
            if (w.ref < 0 || (size_t)w.ref >= refs.size()) return false;
            auto& lin = refs[(size_t)w.ref].lin;
            if (lin.size() <= w.win) lin.resize((size_t)w.win + 1, ~(uint64_t)0);
            if (lin[w.win] == ~(uint64_t)0) lin[w.win] = w.off + sh;
        }
        for (int64_t i = 0; i < p.n_ref; i++) {
            const bmbs_bai_ref& r = p.ref[(size_t)i];
            if (r.ref < 0 || (size_t)r.ref >= refs.size()) return false;
            Ref& R = refs[(size_t)r.ref];
            if (!R.any) { R.any = true; R.beg = r.beg + sh; }
            R.end = r.end + sh; R.n_mapped += r.n_mapped; R.n_unmapped += r.n_unmapped;
        }
        n_no_coor += p.n_no_coor;
        return true;
    }
    size_t n_chunks() const { size_t n = 0; for (const Ref& r : refs) for (const auto& b : r.bins) n += b.second.size(); return n; }
    size_t n_windows() const { size_t n = 0; for (const Ref& r : refs) n += r.lin.size(); return n; }
    void serialize(std::string& o) const
    {
        auto p32 = [&](uint32_t v) { for (int i = 0; i < 4; i++) o.push_back((char)(v >> (8 * i))); };
        auto p64 = [&](uint64_t v) { for (int i = 0; i < 8; i++) o.push_back((char)(v >> (8 * i))); };
        o.assign("BAI\1", 4);
        p32((uint32_t)refs.size());
        for (const Ref& r : refs) {
            if (!r.any) { p32(0); p32(0); continue; }
            p32((uint32_t)r.bins.size() + 1);
            for (const auto& b : r.bins) {
                p32(b.first); p32((uint32_t)b.second.size());
                for (const auto& c : b.second) { p64(c.first); p64(c.second); }
            }
            p32(37450); p32(2); p64(r.beg); p64(r.end); p64(r.n_mapped); p64(r.n_unmapped);
            p32((uint32_t)r.lin.size());
            uint64_t prev = r.beg;
            for (uint64_t v : r.lin) { if (v != ~(uint64_t)0) prev = v; p64(prev); }
        }
        p64(n_no_coor);
    }
};
// one bmbs_bam_sort call of pass 2: whole bins first .. last, or -- a bin larger than the call budget -- the records of that bin whose
// keys lie in [k_lo, k_hi], in the bin's order; a single key that is larger than the budget on its own is cut anywhere (`skip` of its
// records left out, `n` taken): equal keys need no sorting, their order is the bin's
struct SortUnit { size_t first = 0, last = 0; bool sub = false; uint64_t k_lo = 0, k_hi = 0; size_t skip = 0; size_t bytes = 0, n = 0; };
inline void sort_plan(const SortStore& st, size_t budget, std::vector<SortUnit>& units)
{
    SortUnit cur; bool open = false;
    auto flush = [&] { if (open) units.push_back(cur); open = false; };
    for (size_t k = 0; k < st.bin.size(); k++) {
        const SortBin& b = st.bin[k];
        if (b.len.empty()) continue;
        if (b.rec.size() <= budget) {
            if (open && cur.bytes + b.rec.size() > budget) flush();
            if (!open) { cur = SortUnit(); cur.first = k; open = true; }
            cur.last = k; cur.bytes += b.rec.size(); cur.n += b.len.size();
            continue;
        }
        // skew: this bin alone is over the budget.  Its key range is cut again, at the finest edges there are -- between distinct
        // keys, wherever the bytes counted in key order reach the budget
        flush();
        const size_t n = b.len.size();
        std::vector<std::pair<uint64_t, uint32_t>> kl(n);
        { size_t at = 0; for (size_t i = 0; i < n; i++) { kl[i] = {bam_key_of(b.rec.data() + at), b.len[i]}; at += b.len[i]; } }
        std::vector<std::pair<uint64_t, uint32_t>> in_order = kl;
        std::sort(kl.begin(), kl.end(), [](const std::pair<uint64_t, uint32_t>& x, const std::pair<uint64_t, uint32_t>& y) { return x.first < y.first; });
        SortUnit u; bool uopen = false;
        auto uflush = [&] { if (uopen) units.push_back(u); uopen = false; };
        for (size_t i = 0; i < n;) {
            size_t j = i, gb = 0;
            while (j < n && kl[j].first == kl[i].first) gb += kl[j++].second;
            const uint64_t key = kl[i].first;
            if (gb <= budget) {
                if (uopen && u.bytes + gb > budget) uflush();
                if (!uopen) { u = SortUnit(); u.first = u.last = k; u.sub = true; u.k_lo = key; uopen = true; }
                u.k_hi = key; u.bytes += gb; u.n += j - i;
            } else {
                uflush();
                SortUnit one; one.first = one.last = k; one.sub = true; one.k_lo = one.k_hi = key;
                size_t seen = 0;
                for (size_t r = 0; r < n; r++) {
                    if (in_order[r].first != key) continue;
                    if (one.n && one.bytes + in_order[r].second > budget) { units.push_back(one); one.skip = seen; one.bytes = 0; one.n = 0; }
                    one.bytes += in_order[r].second; one.n++; seen++;
                }
                if (one.n) units.push_back(one);
            }
            i = j;
        }
        uflush();
    }
    flush();
}
// the records and lengths of a unit, one behind the other, into a staging buffer
// dup (--markdup, else NULL): a bit per template id; the copy of every record of a marked template gets flag 0x400 (byte 19 |= 0x04)
// clip (--methyl of pairs, else NULL): the records' clips, laid out like the lengths
inline void sort_stage(const SortStore& st, const SortUnit& u, Pool& pool, char* dst, uint32_t* len, const uint64_t* dup, uint32_t* clip)
{
    auto marked = [&](uint64_t t) { return (dup[t >> 6] >> (t & 63)) & 1; };
    if (!u.sub) {
        std::vector<size_t> at(u.last - u.first + 2, 0), ln(u.last - u.first + 2, 0);
        for (size_t k = u.first; k <= u.last; k++) { at[k - u.first + 1] = at[k - u.first] + st.bin[k].rec.size(); ln[k - u.first + 1] = ln[k - u.first] + st.bin[k].len.size(); }
        const int nb = (int)(u.last - u.first + 1), T = std::max(1, std::min(pool.size(), nb));
        pool.run(T, [&](int t) {
            for (int j = t; j < nb; j += T) {
                const SortBin& b = st.bin[u.first + (size_t)j];
                if (b.len.empty()) continue;
                memcpy(dst + at[(size_t)j], b.rec.data(), b.rec.size());
                memcpy(len + ln[(size_t)j], b.len.data(), b.len.size() * 4);
                if (clip) memcpy(clip + ln[(size_t)j], b.clip.data(), b.clip.size() * 4);
                if (dup) { size_t o = at[(size_t)j]; for (size_t i = 0; i < b.len.size(); o += b.len[i], i++) if (marked(b.tid[i])) dst[o + 19] |= 0x04; }
            }
        });
        return;
    }
    const SortBin& b = st.bin[u.first];
    size_t at = 0, seen = 0, taken = 0;
    for (size_t i = 0; i < b.len.size() && taken < u.n; at += b.len[i], i++) {
        const uint64_t key = bam_key_of(b.rec.data() + at);
        if (key < u.k_lo || key > u.k_hi) continue;
        if (seen++ < u.skip) continue;
        memcpy(dst, b.rec.data() + at, b.len[i]);
        if (dup && marked(b.tid[i])) dst[19] |= 0x04;
        dst += b.len[i];
        if (clip) clip[taken] = b.clip[i];
        len[taken++] = b.len[i];
    }
}

// ---- --bam --sort --methyl <prefix>: methylation counts per cytosine of the sorted file's records -----------------------------------------
// Every pass-2 call leaves the sites of its own records on the device (bmbs_bam_sort_methyl behind bmbs_bam_sort: the records are still
// there, duplicates already carry 0x400); only the sites come back.  Calls go in key order and a record reaches at most its span behind
// its position, so a call's sites overlap only the tail of what the calls before it left: the writing thread merges the two sorted
// lists from the first new position on and adds the counts of equal (ref, pos).  The result does not depend on how the records were
// cut into calls.  The files are written once the BAM is complete.
inline bool site_less(const bmbs_methyl_site& a, const bmbs_methyl_site& b) { return a.ref != b.ref ? a.ref < b.ref : a.pos < b.pos; }
inline void methyl_merge(std::vector<bmbs_methyl_site>& all, const bmbs_methyl_site* add, size_t n)
{
    if (!n) return;
    const size_t from = (size_t)(std::lower_bound(all.begin(), all.end(), add[0], site_less) - all.begin());
    std::vector<bmbs_methyl_site> tail(all.begin() + (long)from, all.end());
    all.resize(from);
    size_t i = 0, j = 0;
    while (i < tail.size() || j < n) {
        if (j == n || (i < tail.size() && site_less(tail[i], add[j]))) all.push_back(tail[i++]);
        else if (i == tail.size() || site_less(add[j], tail[i])) all.push_back(add[j++]);
        else { bmbs_methyl_site s = tail[i++]; s.meth += add[j].meth; s.unmeth += add[j].unmeth; j++; all.push_back(s); }
    }
}
// The index holds a pseudo-random letter for every base of the FASTA that is not A, C, G or T: a site whose position or context window
// (CpG: the two bases, CHG / CHH: the three) touches such a base says nothing about the genome.  runs[ref] = the [beg, end) runs of
// such bases of sequence ref, read from the FASTA the way the index builder reads it; false: the file cannot be read, or its
// sequences are not the index's
inline bool non_acgt_runs(const std::string& fasta, const bmbs_index_view& v, std::vector<std::vector<std::pair<int64_t, int64_t>>>& runs)
{
    FILE* f = fopen(fasta.c_str(), "rb");
    if (!f) return false;
    runs.clear();
    std::vector<char> buf(1 << 22);
    bool hdr = false, bol = true;
    int64_t pos = 0;
    size_t got;
    while ((got = fread(buf.data(), 1, buf.size(), f)) > 0)
        for (size_t i = 0; i < got; i++) {
            const unsigned char c = (unsigned char)buf[i];
            if (hdr) { if (c == '\n') { hdr = false; bol = true; } continue; }
            if (c == '\n') { bol = true; continue; }
            if (bol && c == '>') { hdr = true; runs.emplace_back(); if (runs.size() > 1 && pos != (int64_t)v.chrom_len[runs.size() - 2]) { fclose(f); return false; } pos = 0; continue; }
            bol = false;
            if (c <= ' ') continue;
            if (runs.empty()) { fclose(f); return false; }
            const int u = toupper(c);
            if (u != 'A' && u != 'C' && u != 'G' && u != 'T') {
                auto& r = runs.back();
                if (!r.empty() && r.back().second == pos) r.back().second = pos + 1; else r.push_back({pos, pos + 1});
            }
            pos++;
        }
    fclose(f);
    return (int)runs.size() == v.n_chrom && pos == (int64_t)v.chrom_len[runs.size() - 1];
}
inline bool methyl_touches(const std::vector<std::pair<int64_t, int64_t>>& runs, const bmbs_methyl_site& s)
{
    const int64_t w = (s.kind & 3u) == 0 ? 1 : 2;
    const int64_t lo = (s.kind & 4u) ? s.pos - w : s.pos, hi = (s.kind & 4u) ? s.pos : s.pos + w;       // the window [lo, hi]
    auto it = std::upper_bound(runs.begin(), runs.end(), std::make_pair(hi, INT64_MAX));                 // the first run that begins behind hi
    return it != runs.begin() && (it - 1)->second > lo;
}
// --methyl-max-variant-frac: a plain decimal in [0, 1] -> parts per million without floating point.  Digits, or digits '.' digits with
// the first digits optional; at most 6 digits behind the point; no sign, no exponent, nothing else
inline bool methyl_parse_frac(const char* text, int32_t* ppm)
{
    const char* q = text;
    uint64_t whole = 0, frac = 0;
    int nw = 0, nf = 0;
    for (; *q >= '0' && *q <= '9'; q++, nw++) whole = std::min<uint64_t>(whole * 10 + (uint64_t)(*q - '0'), 1000);
    if (*q == '.') {
        for (q++; *q >= '0' && *q <= '9'; q++, nf++) { if (nf >= 6) return false; frac = frac * 10 + (uint64_t)(*q - '0'); }
        if (!nf) return false;
    }
    if (*q || nw + nf == 0) return false;
    for (int k = nf; k < 6; k++) frac *= 10;
    const uint64_t v = whole * 1000000 + frac;
    if (v > 1000000) return false;
    *ppm = (int32_t)v;
    return true;
}
// <prefix>_<context>.bedGraph in MethylDackel's column layout; the percentage is rounded half up in integers.
// merge (--methyl-merge-context): a CpG site is written with the interval of its dinucleotide (strand 0 at p: [p, p + 2), strand 1:
// [p - 1, p + 1)), a CHG site with that of its trinucleotide ([p, p + 3) / [p - 2, p + 1)), and the sites of the context with the same
// interval -- the two strands of one CpG or CHG -- are added; a site without its partner (absent, dropped before, or of another context:
// in CCG the G is a CpG cytosine) stands alone with its interval; CHH is never merged.  Among the sites of ONE context in (ref, pos)
// order the intervals ascend and only partners share one (a C directly in front of a G is a CpG on both strands, so no CHG of strand 0
// lies between a CHG of strand 1 and its interval's start): one pending line is enough.
// min_depth (--methyl-min-depth): a line is written iff meth + unmeth >= min_depth, *shallow += the lines that are not
inline bool methyl_write(const std::string& path, const std::string& prefix, const char* ctx_name, unsigned ctx, const std::vector<bmbs_methyl_site>& sites, const bmbs_index_file* ixf,
                         bool merge, uint64_t min_depth, size_t* shallow)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "track type=\"bedGraph\" description=\"%s %s methylation levels\"\n", prefix.c_str(), ctx_name);
    struct Line { int32_t ref; int64_t beg, end; uint64_t m, u; } cur = {-1, 0, 0, 0, 0};
    const auto flush = [&] {
        if (cur.ref < 0) return;
        if (cur.m + cur.u < min_depth) { ++*shallow; return; }
        fprintf(f, "%s\t%lld\t%lld\t%llu\t%llu\t%llu\n", bmbs_index_file_chrom_name(ixf, cur.ref), (long long)cur.beg, (long long)cur.end,
                (unsigned long long)((200 * cur.m + cur.m + cur.u) / (2 * (cur.m + cur.u))), (unsigned long long)cur.m, (unsigned long long)cur.u);
    };
    const int64_t w = !merge || ctx == 2 ? 1 : ctx == 0 ? 2 : 3;
    for (const bmbs_methyl_site& s : sites) {
        if ((s.kind & 3u) != ctx) continue;
        const int64_t beg = (s.kind & 4u) ? (int64_t)s.pos - w + 1 : (int64_t)s.pos;
        if (cur.ref == s.ref && cur.beg == beg) { cur.m += s.meth; cur.u += s.unmeth; continue; }
        flush();
        cur = Line{s.ref, beg, beg + w, s.meth, s.unmeth};
    }
    flush();
    const bool ok = !ferror(f);
    return fclose(f) == 0 && ok;
}
// <prefix>_mbias.tsv (--mbias): the M-bias table, table[2 mate][2 strand][3 context][2 (unmethylated, methylated)][BMBS_MBIAS_CYCLES] --
// the pass-2 calls' tables (bmbs_methyl_mbias) added up, which does not depend on how the records were cut into calls.  One line per
// (context, strand, read, cycle) with calls, in that order, cycles 1-based, the percentage rounded as in the bedGraphs
inline bool mbias_write(const std::string& path, const std::vector<uint64_t>& table)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    static const char* const ctx_name[3] = {"CpG", "CHG", "CHH"};
    fputs("#context\tstrand\tread\tcycle\tmethylated\tunmethylated\tpercent\n", f);
    for (size_t ctx = 0; ctx < 3; ctx++)
        for (size_t strand = 0; strand < 2; strand++)
            for (size_t mate = 0; mate < 2; mate++) {
                const uint64_t* const un = table.data() + (((mate * 2 + strand) * 3 + ctx) * 2) * BMBS_MBIAS_CYCLES, * const me = un + BMBS_MBIAS_CYCLES;
                for (size_t cy = 0; cy < BMBS_MBIAS_CYCLES; cy++) {
                    const uint64_t m = me[cy], u = un[cy];
                    if (m + u) fprintf(f, "%s\t%s\t%zu\t%zu\t%llu\t%llu\t%llu\n", ctx_name[ctx], strand ? "OB" : "OT", mate + 1, cy + 1, (unsigned long long)m, (unsigned long long)u,
                                       (unsigned long long)((200 * m + m + u) / (2 * (m + u))));
                }
            }
    const bool ok = !ferror(f);
    return fclose(f) == 0 && ok;
}
