// bitmapperbs_amd/csrc/bmbs_search.cpp -- C++ host driver over the C-ABI: the `bitmapperBS --search`
// command line (Process_CommandLines.cpp:88-132), FASTQ in (Process_Reads.cpp:155-317, 810-890), SAM out
// (Process_sam_out.cpp:1137-1153, Schema.cpp:11989-12039, 10537-10640, 11494-11590), mapstats
// (Bitmapper_main.cpp:266-308) -- with the per-read mapping loops of Schema.cpp replaced by batch calls into
// libbmbs_hip.so.  Record order is the input order (== the reference at -t 1).
//
//   bmbs_search --search <index prefix | dir> --seq r.fq[.gz] [-o out.sam] [-e 0.08] [--mapstats f]
//   bmbs_search --search <index> --seq1 a.fq --seq2 b.fq [--min 0] [--max 500] [--sensitive] ...
//   output variants (Process_CommandLines.cpp:93-105): --pbat, --unmapped_out, --ambiguous_out, --bam (BGZF-compressed BAM)
//   extra: --device N | --devices a,b,... (one index copy per listed device, batches dealt to whichever context is free, output
//          order kept), --contexts S (contexts per device sharing its index: S batches in flight per GPU so that the copies of
//          one overlap the kernels of another; default 4), --batch N (records per GPU batch, default 500 k), -t N (host I/O
//          threads), --out-parts N (the input is cut into N contiguous record ranges, each written to its own file
//          <out>.part000 ... concurrently; `cat` of the parts in order == the one-file output), --verbose,
//          --bam --sort [--sort-mem GiB] (ONE coordinate-sorted BAM: its records are the stable sort, by reference / position /
//          strand, of the records --bam writes; sorted on the device, see "--bam --sort" below; needs --out-parts 1)
//          --bam --sort --markdup (PCR duplicates get flag 0x400 in that file: Picard's pair-level rule, decided on the device, see
//          "--markdup" below; nothing else in any record changes)
//          --bam --sort --methyl <prefix> [--CpG] [--CHG] [--CHH] (per-cytosine methylation counts of that file's records, computed on the
//          device while its blocks are written: <prefix>_CpG.bedGraph ..., see "--methyl" below)
//
// The reference has ONE reader thread and ONE fprintf sink (Process_Reads.cpp:2057-2260, Process_sam_out.cpp:954-1006), which is
// what limits it.  Round 2 of this driver indexed the lines and formatted the SAM text with the host's
// I/O threads; those two stages were as long as the GPU stage.  Now the host touches file bytes only to move them:
//   stage R  pread of a window of the FASTQ file(s) into a page-locked buffer (parallel; .gz: one inflate thread per file); the
//            reader COUNTS the newlines (SWAR over the bytes it has just read) to know how many whole records the window holds
//   stage G  one bmbs_map_se_text / bmbs_map_pe_text call per batch: text up, newline index + rows + mapping + SAM formatting on
//            the device (bmbs_text.hip), finished SAM text down into a page-locked buffer; one worker thread per context
//   stage W  pwrite of the SAM text at the part's running offset (--bam: the text is converted to BAM records and BGZF blocks by
//            the I/O threads first, bam_prase.cpp:201-221)
// Buffered writes to ONE file serialise on its inode lock at the speed of one memcpy (~10 GB/s = 28 M SAM records/s on the MI355X
// boxes): --out-parts N gives N inodes.  Every part is a pipeline of its own (reader -> shared GPU workers -> writer) over its own
// record range of the input; for pairs the ranges are cut at the same record in both files (found by the read names, by counting
// lines when the names do not tell).
#include "../../include/bmbs.h"
#include "pgz.h"
#if defined(__x86_64__)
#include <emmintrin.h>
#endif
#include <zlib.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/vfs.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <cctype>
#include <cstdint>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <string>
#include <thread>
#include <vector>

namespace {

// ---- a small persistent thread pool: run(n, f) executes f(0..n-1) and returns when all are done -------------
class Pool {
public:
    explicit Pool(int extra_threads)
    {
        for (int i = 0; i < extra_threads; i++) th_.emplace_back([this] { loop(); });
    }
    ~Pool()
    {
        { std::lock_guard<std::mutex> l(m_); stop_ = true; }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    int size() const { return (int)th_.size() + 1; }
    void run(int n, const std::function<void(int)>& f)
    {
        if (n <= 0) return;
        if (th_.empty() || n == 1) { for (int i = 0; i < n; i++) f(i); return; }
        {
            std::lock_guard<std::mutex> l(m_);
            fn_ = &f; ntask_ = n; next_ = 0; pending_ = n; gen_++;
        }
        cv_.notify_all();
        work();                                   // the caller helps
        std::unique_lock<std::mutex> l(m_);
        done_.wait(l, [this] { return pending_ == 0; });
        fn_ = nullptr;
    }
private:
    void work()
    {
        for (;;) {
            int i;
            const std::function<void(int)>* f;
            {
                std::lock_guard<std::mutex> l(m_);
                if (!fn_ || next_ >= ntask_) return;
                i = next_++; f = fn_;
            }
            (*f)(i);
            {
                std::lock_guard<std::mutex> l(m_);
                if (--pending_ == 0) done_.notify_all();
            }
        }
    }
    void loop()
    {
        unsigned long seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> l(m_);
                cv_.wait(l, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
            }
            work();
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    bool stop_ = false;
    unsigned long gen_ = 0;
    int pending_ = 0, next_ = 0, ntask_ = 0;
    const std::function<void(int)>* fn_ = nullptr;
};

template <class T> class Chan {                  // hand-over queue between the pipeline stages
public:
    void put(T v) { { std::lock_guard<std::mutex> l(m_); q_.push(v); } cv_.notify_one(); }
    T get() { std::unique_lock<std::mutex> l(m_); cv_.wait(l, [this] { return !q_.empty(); }); T v = q_.front(); q_.pop(); return v; }
private:
    std::mutex m_; std::condition_variable cv_; std::queue<T> q_;
};

template <class T> class OrderedChan {           // hands items out in sequence-number order whatever order they arrive in
public:
    void put(long seq, T v) { { std::lock_guard<std::mutex> l(m_); q_[seq] = v; } cv_.notify_all(); }
    T get()
    {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [this] { return q_.count(next_) != 0; });
        T v = q_[next_]; q_.erase(next_); next_++;
        return v;
    }
private:
    std::mutex m_; std::condition_variable cv_; std::map<long, T> q_; long next_ = 0;
};


// ---- newline counting: 64 bytes per step (SSE2: compare, move mask, one population count per 64 bytes) -----------------------------
// (the 8-bytes-per-step SWAR form this replaces ran at 2.4 GB/s per core -- without -mpopcnt every population count is a library
// call -- and sixteen cores' worth of it was what the readers of a FASTQ -> SAM run were busy with; this form: 18 GB/s per core)
inline size_t count_nl(const char* p, size_t n)
{
    size_t c = 0, i = 0;
#if defined(__x86_64__)
    const __m128i nl = _mm_set1_epi8('\n');
    for (; i + 64 <= n; i += 64) {
        const uint64_t a = (unsigned)_mm_movemask_epi8(_mm_cmpeq_epi8(_mm_loadu_si128(reinterpret_cast<const __m128i*>(p + i)), nl));
        const uint64_t b = (unsigned)_mm_movemask_epi8(_mm_cmpeq_epi8(_mm_loadu_si128(reinterpret_cast<const __m128i*>(p + i + 16)), nl));
        const uint64_t d = (unsigned)_mm_movemask_epi8(_mm_cmpeq_epi8(_mm_loadu_si128(reinterpret_cast<const __m128i*>(p + i + 32)), nl));
        const uint64_t e = (unsigned)_mm_movemask_epi8(_mm_cmpeq_epi8(_mm_loadu_si128(reinterpret_cast<const __m128i*>(p + i + 48)), nl));
        c += (size_t)__builtin_popcountll(a | (b << 16) | (d << 32) | (e << 48));
    }
#endif
    for (; i < n; i++) c += p[i] == '\n';                 // (the whole buffer on a host without SSE2)
    return c;
}
// offset just behind the k-th newline (k >= 1) of p[0, n), n when there are fewer
inline size_t after_kth_nl(const char* p, size_t n, size_t k)
{
    const char* q = p; const char* e = p + n;
    while (k && q < e) { const char* h = (const char*)memchr(q, '\n', (size_t)(e - q)); if (!h) return n; q = h + 1; k--; }
    return k ? n : (size_t)(q - p);
}

struct Pinned {                                  // page-locked staging (bmbs_host_alloc_kind)
    char* p = nullptr; size_t cap = 0; int kind = 0;
    bool need(size_t bytes)
    {
        if (bytes <= cap) return true;
        if (p) bmbs_host_free(p);
        cap = bytes + bytes / 4 + 4096;
        p = (char*)bmbs_host_alloc_kind(cap, kind);
        if (!p) { cap = 0; return false; }
        return true;
    }
    void release() { if (p) bmbs_host_free(p); p = nullptr; cap = 0; }
};

// ---- FASTQ text source over a byte range of a file.  Plain files: parallel pread()s straight into the batch's page-locked window,
// the newlines counted per 64 KiB block by the thread that has just read it.  .gz: a thread of its own inflates into a queue of
// chunks (so that the two files of a paired-end run inflate side by side) and the window is assembled from them. ---------------
#define SUB_BLOCK ((size_t)1 << 16)
// --loop-input N (measurement aid; plain FASTQ, and BGZF input that is inflated on the device): a part's byte range is read N times over, so that a run lasts seconds on an input
// that fits the page cache (the pipeline's fill and the contexts' first calls then weigh what they weigh in a real run)
static int g_loop_input = 1;
struct Source {
    bool gz = false;
    size_t lo0 = 0; int loops_left = 0;
    int fd = -1;
    size_t size = 0, off = 0, end = 0;           // plain: the part's byte range [off, end)
    std::string err;
    // .gz: inflated text arrives as numbered chunks; `ready` hands them to window() in order
    std::vector<std::thread> inflaters;
    std::mutex m; std::condition_variable cv_data, cv_room;
    std::map<long, std::vector<char>> ready;     // chunk number -> text
    int zdev = -1;                               // >= 0: BGZF blocks are inflated on this HIP device (bmbs_inflate_bgzf)
    // ... a window at a time, straight into the batch's page-locked window: no inflater threads, no chunk queue, and the newline counts
    // come back with the text -- the host moves the compressed bytes into a staging buffer and nothing else
    bool zdirect = false;
    bmbs_ctx* zc = nullptr;
    Pinned zstage;
    std::vector<uint64_t> zblk, zout;
    long next_chunk = 0;                         // the chunk window() takes next
    long want_chunk = 0;                         // the chunk window() is waiting for (always admitted by push_chunk)
    size_t queued = 0, front_used = 0;
    bool gz_done = false, gz_stop = false;
    int live_inflaters = 0;
    std::vector<char> carry;
    // BGZF (bgzip): independent deflate blocks of <= 64 KiB with their compressed size in the header -- inflated by several threads
    bool bgzf = false;
    const unsigned char* zmap = nullptr; size_t zsize = 0, znext = 0;     // the compressed file, mapped; next unassigned block
    long zjob = 0;                                                        // number of the next job
    // ordinary gzip (one deflate stream per member): block-parallel inflate, pgz.h
    std::unique_ptr<pgz::Engine> pgz_eng;
    std::thread pgz_watch;
    int gz_threads_ = 1;

    static bool is_gz(const char* path)
    {
        FILE* f = fopen(path, "rb");
        if (!f) return false;
        unsigned char mg[2] = {0, 0};
        const size_t got = fread(mg, 1, 2, f);
        fclose(f);
        return got == 2 && mg[0] == 0x1f && mg[1] == 0x8b;
    }
    // compressed size of the BGZF block at p (0: not a BGZF block header)
    static size_t bgzf_block(const unsigned char* p, size_t avail)
    {
        if (avail < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4) || p[10] != 6 || p[11] != 0 || p[12] != 'B' || p[13] != 'C' || p[14] != 2 || p[15] != 0) return 0;
        const size_t bs = (size_t)(p[16] | (p[17] << 8)) + 1;
        return bs >= 26 && bs <= avail ? bs : 0;
    }
    static size_t bgzf_isize(const unsigned char* p, size_t bs) { return (size_t)p[bs - 4] | ((size_t)p[bs - 3] << 8) | ((size_t)p[bs - 2] << 16) | ((size_t)p[bs - 1] << 24); }
    // the gzip members from byte `at` of the mapped file on, chunk numbers from `first_id` (called with `m` held)
    void start_pgz(size_t at, long first_id)
    {
        if (gz_stop || pgz_eng) return;
        pgz::Options o; o.threads = gz_threads_; o.span = (size_t)1 << 20;
        if (const char* sp = getenv("BMBS_GZ_SPAN")) { const long v = atol(sp); if (v >= 1024) o.span = (size_t)v; }      // tests: many spans in a small file
        pgz_eng.reset(new pgz::Engine(zmap, zsize, at, first_id, o, [this](long id, std::vector<char>&& c) { push_chunk(id, std::move(c)); }));
        live_inflaters++;
        pgz_eng->start();
        pgz_watch = std::thread([this] {
            const std::string e = pgz_eng->wait();
            if (!e.empty()) { std::lock_guard<std::mutex> l(m); if (err.empty()) err = e; }
            inflater_exit();
        });
    }
    void push_chunk(long id, std::vector<char>&& c)
    {
        std::unique_lock<std::mutex> l(m);
        // the chunk window() is waiting for always gets in; the others wait for room (text inflated ahead of its turn is bounded)
        cv_room.wait(l, [&] { return id == want_chunk || queued < ((size_t)768 << 20) || gz_stop; });
        if (gz_stop) return;
        queued += c.size();
        ready[id] = std::move(c);
        cv_data.notify_all();
    }
    void inflater_exit()
    {
        std::lock_guard<std::mutex> l(m);
        if (--live_inflaters == 0) { gz_done = true; cv_data.notify_all(); }
    }
    // a one-member .gz file that is not taken by the device path after all: the host's block-parallel inflater from its first byte
    void host_stream() { std::lock_guard<std::mutex> l(m); start_pgz(0, 0); }
    bool open(const char* path, size_t lo, size_t hi, int gz_threads = 1, int device = -1)
    {
        zdev = device;
        gz = is_gz(path);
        if (gz) {
            const int zfd = ::open(path, O_RDONLY);
            struct stat zsb;
            bool zmap_keep = false;
            if (zfd >= 0 && fstat(zfd, &zsb) == 0 && zsb.st_size >= 18) {
                void* mp = mmap(nullptr, (size_t)zsb.st_size, PROT_READ, MAP_PRIVATE, zfd, 0);
                if (mp != MAP_FAILED) {
                    zmap = (const unsigned char*)mp; zsize = (size_t)zsb.st_size; zmap_keep = true;
                    (void)madvise(mp, zsize, MADV_SEQUENTIAL);
                    bgzf = bgzf_block(zmap, zsize) != 0;
                }
            }
            if (zfd >= 0) ::close(zfd);
            if (!zmap_keep) return false;
            gz_threads_ = std::max(1, gz_threads);
            if (bgzf) {
                const char* zd = getenv("BMBS_GZ_DEVICE");
                if (zd && !strcmp(zd, "0")) zdev = -1;
                if (zdev >= 0) { zdirect = true; zstage.kind = 1; loops_left = g_loop_input - 1; return true; }      // inflated on the device, a window at a time (no threads here)
                const int n_inflaters = gz_threads_;
                live_inflaters = n_inflaters;                   // (the threads count it down as they finish: not the loop bound)
                for (int t = 0; t < n_inflaters; t++)
                    inflaters.emplace_back([this] {
                        // every block is a gzip member of its own: the driver's own inflater (pgz.h) on known bytes -- no window in
                        // front of a block, no markers -- and the member's CRC-32 checked by carry-less multiplication
                        pgz::OutBuf<pgz::u8> ob;
                        std::unique_ptr<pgz::Tables> dyn(new pgz::Tables);
                        std::vector<pgz::MemberEnd> ends;
                        for (;;) {
                            // a job = the blocks of the next ~2 MiB of the compressed file
                            size_t a, e; long id;
                            {
                                std::lock_guard<std::mutex> l(m);
                                if (gz_stop || znext >= zsize) break;
                                a = znext; id = zjob;
                                size_t q = a;
                                while (q < zsize && q - a < ((size_t)2 << 20)) { const size_t bs = bgzf_block(zmap + q, zsize - q); if (!bs) break; q += bs; }
                                if (q == a) {
                                    // not a BGZF block: a file whose later members are ordinary gzip goes on through the stream inflater
                                    znext = zsize;
                                    if (pgz::gzip_header(zmap, zsize, a)) start_pgz(a, id);
                                    else err = "corrupt BGZF block header in the .gz input";
                                    break;
                                }
                                zjob++; e = q; znext = q;
                            }
                            bool bad = false;
                            std::vector<char> out;
                            try {
                                size_t total = 0;
                                for (size_t q = a; q < e;) { const size_t bs = bgzf_block(zmap + q, zsize - q); const size_t isz = bgzf_isize(zmap + q, bs); if (isz > 65536) bad = true; total += isz; q += bs; }
                                if (!bad) out.resize(total);
                                size_t at = 0;
                                for (size_t q = a; q < e && !bad;) {
                                    const size_t bs = bgzf_block(zmap + q, zsize - q);
                                    const size_t isz = bgzf_isize(zmap + q, bs);
                                    if (isz) {
                                        if (!ob.mem) { if (!ob.reserve(70000)) throw std::bad_alloc(); memset(ob.mem, 0, pgz::WIN); }
                                        ob.n = 0; ob.mstart = 0; ob.reach = 0; ends.clear();      // (a member of its own: nothing in front of it)
                                        // (the deflate data starts behind the WHOLE member header: a block may carry a name, a comment or a header CRC too)
                                        const size_t body = pgz::gzip_header(zmap, q + bs, q);
                                        pgz::DecodeResult r; r.st = pgz::ST_ERROR; r.end_bit = 0; r.why = "";
                                        if (body) r = pgz::decode_blocks<pgz::u8>(zmap, q + bs, (pgz::u64)body * 8, ~(pgz::u64)0, ob, ends, *dyn);
                                        if (r.st != pgz::ST_END || ob.n != isz || ends.size() != 1 || ends[0].isize != (pgz::u32)isz ||
                                            ends[0].crc != pgz::crc32_fast(0, ob.out(), isz)) bad = true;
                                        else memcpy(out.data() + at, ob.out(), isz);
                                    }
                                    at += isz; q += bs;
                                }
                            } catch (const std::exception&) { bad = true; }
                            if (bad) { std::lock_guard<std::mutex> l(m); err = "corrupt BGZF block in the .gz input"; znext = zsize; break; }
                            push_chunk(id, std::move(out));
                        }
                        inflater_exit();
                    });
                return true;
            }
            host_stream();
            return true;
        }
        fd = ::open(path, O_RDONLY);
        if (fd < 0) return false;
        struct stat sb;
        if (fstat(fd, &sb)) return false;
        size = (size_t)sb.st_size;
        off = std::min(lo, size); end = std::min(hi, size);
        lo0 = off; loops_left = g_loop_input - 1;
        (void)posix_fadvise(fd, 0, 0, POSIX_FADV_SEQUENTIAL);
        return true;
    }
    // up to `cap` bytes of text starting at the current record boundary into dst (which has 64 spare bytes behind cap); `last` when
    // they reach the end of the range; counts[i] = newlines of dst[i * SUB_BLOCK ...).  false: I/O error (err says which)
    bool window(Pool& pool, char* dst, size_t cap, size_t& len_out, bool& last, std::vector<uint32_t>& counts)
    {
        size_t len = 0;
        if (!gz) {
            if (off == end && loops_left > 0) { off = lo0; loops_left--; }
            len = std::min(cap, end - off);
            const size_t nsb = (len + SUB_BLOCK - 1) / SUB_BLOCK;
            counts.assign(nsb, 0);
            const int T = pool.size() * 2;
            const size_t per = ((nsb + (size_t)T - 1) / (size_t)T) * SUB_BLOCK;
            std::atomic<int> bad(0);
            pool.run(T, [&](int t) {
                size_t a = std::min(len, per * (size_t)t);
                const size_t e = std::min(len, a + per);
                while (a < e) {
                    const size_t stop = std::min(e, a + SUB_BLOCK);            // read one block, count it while it is in cache
                    size_t at = a;
                    while (at < stop) {
                        const ssize_t g = pread(fd, dst + at, stop - at, (off_t)(off + at));
                        if (g <= 0) { bad = g < 0 ? errno : EIO; return; }
                        at += (size_t)g;
                    }
                    counts[a / SUB_BLOCK] = (uint32_t)count_nl(dst + a, stop - a);
                    a = stop;
                }
            });
            if (bad) { err = std::string("read error on the FASTQ input: ") + strerror(bad); return false; }
            last = off + len == end && loops_left == 0;
        } else if (zdirect) {
            if (!zc) {
                // (only when the driver's two-phase path is not in use: a context of this source's own inflates into the host window)
                bmbs_params P0; bmbs_default_params(&P0);
                zc = bmbs_create(zdev, &P0);
                if (!zc) { err = "cannot create a context on the device for the BGZF input (BMBS_GZ_DEVICE=0 inflates on the host)"; return false; }
            }
            size_t have = carry.size();
            if (have > cap) { err = "internal: carried text larger than the window"; return false; }
            if (have) memcpy(dst, carry.data(), have);
            carry.clear();
            // the BGZF blocks whose text fits behind the carried bytes
            const size_t a = znext;
            size_t q = a; uint64_t text = 0;
            zblk.clear(); zout.clear(); zblk.push_back(0); zout.push_back(0);
            bool foreign = false;
            while (q < zsize) {
                const size_t bs = bgzf_block(zmap + q, zsize - q);
                if (!bs) { foreign = true; break; }
                const size_t isz = bgzf_isize(zmap + q, bs);
                if (isz > 65536) { err = "corrupt BGZF block in the .gz input"; return false; }
                if (have + text + isz > cap) break;
                q += bs; text += isz;
                zblk.push_back(q - a); zout.push_back(text);
            }
            if (foreign && q == a) {
                // a member that is not a BGZF block: the rest of the file goes through the host's stream inflater (chunks)
                if (!pgz::gzip_header(zmap, zsize, a)) { err = "corrupt BGZF block header in the .gz input"; return false; }
                zdirect = false;
                { std::lock_guard<std::mutex> l(m); znext = zsize; start_pgz(a, 0); }
                carry.assign(dst, dst + have);
                return window(pool, dst, cap, len_out, last, counts);
            }
            if (q == a && q < zsize) { err = "a BGZF block larger than the window"; return false; }
            znext = q;
            len = have + (size_t)text;
            last = znext >= zsize;
            const size_t nsb = (len + SUB_BLOCK - 1) / SUB_BLOCK;
            counts.assign(nsb + 1, 0);
            if (q > a) {
                const size_t zbytes = q - a;
                if (!zstage.need(zbytes + 64)) { err = "cannot allocate page-locked staging memory"; return false; }
                const int T = pool.size() * 2;
                const size_t per = ((zbytes + (size_t)T - 1) / (size_t)T + 4095) & ~(size_t)4095;
                pool.run(T, [&](int t) { const size_t x = std::min(zbytes, per * (size_t)t), y = std::min(zbytes, x + per); if (x < y) memcpy(zstage.p + x, zmap + a + x, y - x); });
                const int rc = bmbs_inflate_bgzf(zc, zstage.p, zbytes, zblk.data(), zout.data(), (int64_t)zblk.size() - 1, dst + have, (uint64_t)text, counts.data(), (uint64_t)have);
                if (rc) { err = bmbs_last_error(zc); return false; }
            }
            counts.resize(nsb);
            for (size_t i = 0; i * SUB_BLOCK < have; i++) counts[i] += (uint32_t)count_nl(dst + i * SUB_BLOCK, std::min(SUB_BLOCK, have - i * SUB_BLOCK));
        } else {
            size_t have = std::min(carry.size(), cap);
            if (carry.size() > cap) { err = "internal: carried text larger than the window"; return false; }
            // which pieces of which chunks make up the window (waiting for the inflaters as needed) ...
            struct Piece { const char* src; size_t len, dst; };
            std::vector<Piece> pieces;
            if (have) pieces.push_back(Piece{carry.data(), have, 0});
            bool done = false;
            long chunk = next_chunk; size_t used = front_used;
            std::vector<long> finished;
            while (have < cap) {
                std::unique_lock<std::mutex> l(m);
                if (want_chunk != chunk) { want_chunk = chunk; cv_room.notify_all(); }
                cv_data.wait(l, [&] { return ready.count(chunk) != 0 || gz_done; });
                auto it = ready.find(chunk);
                if (it == ready.end()) { done = true; if (!err.empty()) return false; break; }
                std::vector<char>& f = it->second;                                  // (only this thread erases: the chunk stays put)
                l.unlock();
                const size_t take = std::min(cap - have, f.size() - used);
                pieces.push_back(Piece{f.data() + used, take, have});
                have += take; used += take;
                if (used == f.size()) { finished.push_back(chunk); chunk++; used = 0; }
            }
            len = have;
            last = done;
            // ... then every thread copies its share of the window and counts the newlines of what it has just written (one thread
            // copying 300 MB windows of two files was the whole run time of gzipped input once the inflate ran on many threads)
            const size_t nsb = (len + SUB_BLOCK - 1) / SUB_BLOCK;
            counts.assign(nsb, 0);
            const int T = (int)std::min<size_t>(std::max<size_t>(nsb, 1), (size_t)pool.size() * 2);
            const size_t per = ((nsb + (size_t)T - 1) / (size_t)T) * SUB_BLOCK;
            pool.run(T, [&](int t) {
                const size_t a = std::min(len, per * (size_t)t), e = std::min(len, a + per);
                if (a >= e) return;
                size_t lo = 0, hi = pieces.size();                                  // first piece that reaches beyond a
                while (lo < hi) { const size_t mid = (lo + hi) / 2; if (pieces[mid].dst + pieces[mid].len <= a) lo = mid + 1; else hi = mid; }
                for (size_t i = lo; i < pieces.size() && pieces[i].dst < e; i++) {
                    const size_t x = std::max(a, pieces[i].dst), y = std::min(e, pieces[i].dst + pieces[i].len);
                    if (x < y) memcpy(dst + x, pieces[i].src + (x - pieces[i].dst), y - x);
                }
                for (size_t q = a; q < e; q += SUB_BLOCK) counts[q / SUB_BLOCK] = (uint32_t)count_nl(dst + q, std::min(SUB_BLOCK, e - q));
            });
            carry.clear();
            {
                std::lock_guard<std::mutex> l(m);
                for (long id : finished) { auto it = ready.find(id); if (it != ready.end()) { queued -= it->second.size(); ready.erase(it); } }
                next_chunk = chunk; want_chunk = chunk; front_used = used;
                cv_room.notify_all();
            }
        }
        // an unterminated last line counts as a line: the device wants every line closed
        if (last && len && dst[len - 1] != '\n') { dst[len] = '\n'; len++; if ((len - 1) / SUB_BLOCK >= counts.size()) counts.push_back(0); counts[(len - 1) / SUB_BLOCK]++; }
        len_out = len;
        return true;
    }
    void consumed(const char* p, size_t len, size_t used)
    {
        if (!gz) { off += std::min(used, end - off); return; }
        carry.assign(p + used, p + len);
    }
    void close()
    {
        if (gz) {
            { std::lock_guard<std::mutex> l(m); gz_stop = true; }
            cv_room.notify_all();
            if (pgz_eng) pgz_eng->stop();
            for (auto& t : inflaters) t.join();
            inflaters.clear();
            if (pgz_watch.joinable()) pgz_watch.join();
            pgz_eng.reset();
        }
        ready.clear();
        if (zmap) munmap((void*)zmap, zsize);
        zmap = nullptr;
        if (fd >= 0) ::close(fd);
        fd = -1; gz = false;
    }
    // the next BGZF blocks whose text fits into `room` bytes (at least one): their bytes are zmap[a, q); tables relative to a.
    // foreign: the file goes on with a member that is not a BGZF block.  false: corrupt header
    bool next_blocks(size_t room, size_t& a, size_t& q, bool& foreign)
    {
        a = znext; q = a; foreign = false;
        uint64_t text = 0;
        zblk.clear(); zout.clear(); zblk.push_back(0); zout.push_back(0);
        while (q < zsize) {
            const size_t bs = bgzf_block(zmap + q, zsize - q);
            if (!bs) { foreign = true; break; }
            const size_t isz = bgzf_isize(zmap + q, bs);
            if (isz > 65536) { err = "corrupt BGZF block in the .gz input"; return false; }
            if (text + isz > room && q > a) break;
            q += bs; text += isz;
            zblk.push_back(q - a); zout.push_back(text);
            if (text >= room) break;
        }
        if (foreign && q == a && !pgz::gzip_header(zmap, zsize, a)) { err = "corrupt BGZF block header in the .gz input"; return false; }
        return true;
    }
    // the device side of a compressed source (context, staging): released apart from close(), outside a driver's timed region
    void release_device()
    {
        if (zc) bmbs_destroy(zc);
        zc = nullptr;
        zstage.release();
    }
    ~Source() { close(); release_device(); }
};

// offset just behind the k-th newline of a window whose blocks have been counted
size_t after_kth_nl_blocks(const char* p, size_t len, const std::vector<uint32_t>& counts, size_t k)
{
    size_t acc = 0;
    for (size_t i = 0; i < counts.size(); i++) {
        if (acc + counts[i] >= k) { const size_t a = i * SUB_BLOCK; return a + after_kth_nl(p + a, std::min(SUB_BLOCK, len - a), k - acc); }
        acc += counts[i];
    }
    return len;
}

// ---- where the parts begin: record boundaries of plain FASTQ files ----------------------------------------------------------------
// first record start at or after `guess`: a line that begins with '@' whose second successor begins with '+' (a quality line may
// begin with '@', but then the line two further on is a sequence line, which cannot begin with '+')
size_t record_start_at(int fd, size_t size, size_t guess)
{
    if (guess == 0) return 0;
    if (guess >= size) return size;
    for (size_t span = (size_t)1 << 20; ; span *= 4) {
        const size_t a = guess - 1, n = std::min(span, size - a);           // from the byte before: a newline there makes `guess` a line start
        std::vector<char> buf(n);
        size_t got = 0;
        while (got < n) { const ssize_t g = pread(fd, buf.data() + got, n - got, (off_t)(a + got)); if (g <= 0) break; got += (size_t)g; }
        std::vector<size_t> ls;                                                // line starts inside the buffer
        for (size_t i = 0; i + 1 < got; i++) if (buf[i] == '\n') ls.push_back(i + 1);
        for (size_t i = 0; i + 2 < ls.size(); i++)
            if (buf[ls[i]] == '@' && buf[ls[i + 2]] == '+' && (i + 4 >= ls.size() || buf[ls[i + 4]] == '@')) return a + ls[i];
        if (a + n >= size) return size;
    }
}
// name of the record at `at`, cut like the paired-end reader does (first ' ' or '/')
std::string cut_name_at(int fd, size_t size, size_t at)
{
    char b[4096];
    const size_t n = std::min(sizeof b, size - at);
    const ssize_t g = pread(fd, b, n, (off_t)at);
    std::string s;
    for (ssize_t i = 0; i < g && b[i] != '\n' && b[i] != ' ' && b[i] != '/'; i++) s += b[i];
    return s;
}
size_t next_record(int fd, size_t size, size_t at)       // start of the record after the one at `at`
{
    size_t pos = at; int lines = 0;
    char b[1 << 16];
    while (pos < size && lines < 4) {
        const ssize_t g = pread(fd, b, sizeof b, (off_t)pos);
        if (g <= 0) break;
        for (ssize_t i = 0; i < g; i++) if (b[i] == '\n' && ++lines == 4) return pos + (size_t)i + 1;
        pos += (size_t)g;
    }
    return size;
}
size_t count_lines(Pool& pool, int fd, size_t a, size_t b)                 // newlines of file bytes [a, b)
{
    const size_t blk = (size_t)16 << 20, nb = (b - a + blk - 1) / blk;
    std::vector<size_t> c(nb, 0);
    const int T = (int)std::min<size_t>(nb, (size_t)pool.size() * 2);
    pool.run(T, [&](int t) {
        std::vector<char> buf(blk);
        for (size_t i = (size_t)t; i < nb; i += (size_t)T) {
            const size_t lo = a + i * blk, n = std::min(blk, b - lo);
            size_t got = 0;
            while (got < n) { const ssize_t g = pread(fd, buf.data() + got, n - got, (off_t)(lo + got)); if (g <= 0) break; got += (size_t)g; }
            c[i] = count_nl(buf.data(), got);
        }
    });
    size_t s = 0;
    for (size_t x : c) s += x;
    return s;
}
size_t offset_of_line(Pool& pool, int fd, size_t size, size_t line)          // offset of the first byte of line `line` (0-based)
{
    if (line == 0) return 0;
    const size_t blk = (size_t)16 << 20, nb = (size + blk - 1) / blk;
    std::vector<size_t> c(nb, 0);
    const int T = (int)std::min<size_t>(nb, (size_t)pool.size() * 2);
    pool.run(T, [&](int t) {
        std::vector<char> buf(blk);
        for (size_t i = (size_t)t; i < nb; i += (size_t)T) {
            const size_t lo = i * blk, n = std::min(blk, size - lo);
            size_t got = 0;
            while (got < n) { const ssize_t g = pread(fd, buf.data() + got, n - got, (off_t)(lo + got)); if (g <= 0) break; got += (size_t)g; }
            c[i] = count_nl(buf.data(), got);
        }
    });
    size_t acc = 0;
    for (size_t i = 0; i < nb; i++) {
        if (acc + c[i] >= line) {
            const size_t lo = i * blk, n = std::min(blk, size - lo);
            std::vector<char> buf(n);
            size_t got = 0;
            while (got < n) { const ssize_t g = pread(fd, buf.data() + got, n - got, (off_t)(lo + got)); if (g <= 0) break; got += (size_t)g; }
            return lo + after_kth_nl(buf.data(), got, line - acc);
        }
        acc += c[i];
    }
    return size;
}
// the record of file 2 that pairs with the record starting at b1 of file 1: looked for by name around the proportional offset
// (two consecutive names have to agree and the match has to be the only one in the window); counted when the names do not tell
size_t mate_boundary(Pool& pool, int fd1, size_t size1, size_t b1, int fd2, size_t size2)
{
    if (b1 == 0) return 0;
    if (b1 >= size1) return size2;
    const std::string n0 = cut_name_at(fd1, size1, b1);
    const size_t b1n = next_record(fd1, size1, b1);
    const std::string n1 = b1n < size1 ? cut_name_at(fd1, size1, b1n) : std::string();
    const size_t g2 = (size_t)((double)size2 * ((double)b1 / (double)size1));
    for (size_t W = (size_t)2 << 20; W <= ((size_t)64 << 20) && !n0.empty(); W *= 4) {
        size_t lo = g2 > W ? record_start_at(fd2, size2, g2 - W) : 0;
        const size_t hi = std::min(size2, g2 + W);
        size_t found = size2 + 1; int hits = 0;
        for (size_t at = lo; at < hi && at < size2; at = next_record(fd2, size2, at)) {
            if (cut_name_at(fd2, size2, at) != n0) continue;
            const size_t nx = next_record(fd2, size2, at);
            if (!n1.empty() && (nx >= size2 || cut_name_at(fd2, size2, nx) != n1)) continue;
            hits++; found = at;
        }
        if (hits == 1) return found;
        if (hits > 1) break;                                                  // names repeat: they do not identify a record
    }
    const size_t lines = count_lines(pool, fd1, 0, b1);                       // b1 is a record start: lines % 4 == 0
    return offset_of_line(pool, fd2, size2, lines);
}

inline void put_uint(std::string& s, unsigned long long v)
{
    char b[24]; int i = 24;
    do { b[--i] = (char)('0' + v % 10); v /= 10; } while (v);
    s.append(b + i, (size_t)(24 - i));
}

// ---- --bam (Process_CommandLines.cpp:94; the reference hands each SAM line to htslib's sam_parse1 and bam_write1,
// bam_prase.cpp:201-221): the records are built and deflated into BGZF blocks ON THE DEVICE (BMBS_TEXT_BAM, bmbs_bam.hip); the host
// writes the BAM header (below) and the end-of-file block, and moves the device's bytes into the file ----------
inline void put_le32(std::vector<char>& o, uint32_t v) { char b[4] = {(char)v, (char)(v >> 8), (char)(v >> 16), (char)(v >> 24)}; o.insert(o.end(), b, b + 4); }

// BGZF: independent gzip members of at most 0xff00 input bytes with the BC extra field (SAM spec 4.1)
void bgzf_append(const char* in, size_t n, std::vector<char>& out)
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
void sort_plan(const SortStore& st, size_t budget, std::vector<SortUnit>& units)
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
void sort_stage(const SortStore& st, const SortUnit& u, Pool& pool, char* dst, uint32_t* len, const uint64_t* dup, uint32_t* clip)
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
void methyl_merge(std::vector<bmbs_methyl_site>& all, const bmbs_methyl_site* add, size_t n)
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
bool non_acgt_runs(const std::string& fasta, const bmbs_index_view& v, std::vector<std::vector<std::pair<int64_t, int64_t>>>& runs)
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
// <prefix>_<context>.bedGraph in MethylDackel's column layout; the percentage is rounded half up in integers
bool methyl_write(const std::string& path, const std::string& prefix, const char* ctx_name, unsigned ctx, const std::vector<bmbs_methyl_site>& sites, const bmbs_index_file* ixf)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "track type=\"bedGraph\" description=\"%s %s methylation levels\"\n", prefix.c_str(), ctx_name);
    for (const bmbs_methyl_site& s : sites) {
        if ((s.kind & 3u) != ctx) continue;
        const uint64_t m = s.meth, u = s.unmeth;
        fprintf(f, "%s\t%d\t%d\t%llu\t%u\t%u\n", bmbs_index_file_chrom_name(ixf, s.ref), s.pos, s.pos + 1, (unsigned long long)((200 * m + m + u) / (2 * (m + u))), s.meth, s.unmeth);
    }
    const bool ok = !ferror(f);
    return fclose(f) == 0 && ok;
}

void print_stats(FILE* o, const int64_t st[5])
{
    long long reads = st[0], uniq = st[1], amb = st[2], unm = st[0] - st[1] - st[2];
    fprintf(o, "%-48s%lld\n", "No. of Reads:", reads);
    fprintf(o, "%-48s%lld (%0.2f%%)\n", "No. of Unique Mapped Reads:", uniq, ((double)uniq / (double)reads) * 100);
    fprintf(o, "%-48s%lld (%0.2f%%)\n", "No. of Ambiguous Mapped Reads:", amb, ((double)amb / (double)reads) * 100);
    fprintf(o, "%-48s%lld (%0.2f%%)\n", "No. of Unmapped Reads:", unm, ((double)unm / (double)reads) * 100);
    fprintf(o, "%-47s %0.2f%%\n", "Mismatch and Indel Rate:", ((double)st[4] / (double)st[3]) * 100);
}

bool is_dir(const std::string& p) { struct stat sb; return stat(p.c_str(), &sb) == 0 && S_ISDIR(sb.st_mode); }

double now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }

struct Part;
struct Batch {
    Part* part = nullptr;
    long seq = 0;                                // position within the part (output order)
    long n = 0;                                  // records (pairs)
    bool end = false;                            // the part's input ends with this batch
    Pinned text1, text2, sam;                    // FASTQ windows in, SAM text out
    size_t used1 = 0, used2 = 0;
    uint64_t sam_bytes = 0;
    std::vector<uint64_t> skey; std::vector<uint32_t> slen; int64_t n_sorted = 0;      // --sort: key and length of each record in `sam`
    std::vector<bmbs_dup_sig> sig; std::vector<uint32_t> tmpl; int64_t n_sig = 0;      // --markdup: the batch's signatures, the template of each record in `sam`
    std::vector<uint32_t> clip;                                                         // --methyl of pairs: the mate-overlap clip of each record in `sam`
    std::vector<uint32_t> counts1, counts2;
    bmbs_ctx* open_ctx = nullptr;                // compressed input kept on the device: the context that holds this batch's open window
};

struct Part {                                    // one contiguous record range of the input -> one output file
    int id = 0;
    Source s1, s2;
    int ofd = -1;
    size_t out_off = 0;
    size_t alloc_end = 0;                        // the file's blocks are reserved up to here (fallocate ahead of the writers)
    bool can_alloc = true, regular = false;
    OrderedChan<Batch*> out_q;
    long next_seq = 0;
    std::thread reader, writer;
    double t_read = 0, t_write = 0, t_format = 0, t_wait_r = 0, t_wait_w = 0;
    long records = 0;
};

}  // namespace

#ifdef BMBS_SOURCE_TEST
// reader self-test (no GPU): bmbs_reader_test <file> <window bytes> <threads> -- the text the driver's reader hands on, window by
// window, to stdout; what is left of a window behind its last complete record is carried into the next one as in the real pipeline
int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    Source s;
    const size_t cap = (size_t)atol(argv[2]);
    if (!s.open(argv[1], 0, ~(size_t)0, atoi(argv[3]))) { fprintf(stderr, "cannot open\n"); return 1; }
    Pool pool(3);
    std::vector<char> buf(cap + 64 + ((size_t)64 << 20));
    std::vector<uint32_t> counts;
    for (;;) {
        size_t n = 0; bool last = false;
        const size_t want = std::max(cap, s.carry.size() + 1024);
        if (!s.window(pool, buf.data(), want, n, last, counts)) { fprintf(stderr, "%s\n", s.err.c_str()); return 1; }
        size_t lines = 0;
        for (uint32_t c : counts) lines += c;
        const size_t nrec = lines / 4;
        if (nrec == 0 && !last) { fprintf(stderr, "record larger than the window\n"); return 1; }
        const size_t used = nrec ? after_kth_nl_blocks(buf.data(), n, counts, nrec * 4) : 0;
        fwrite(buf.data(), 1, used, stdout);
        s.consumed(buf.data(), n, used);
        if (last && used == n) break;
        if (last && nrec == 0) break;
    }
    s.close();
    return 0;
}
#else
int main(int argc, char** argv)
{
    bmbs_params P; bmbs_default_params(&P);
    std::string index, seq, seq1, seq2, out = "output", mapstats, build_fasta, index_folder;
    int device = 0, io_threads = 0, contexts = 4, parts = 1, reader_threads = 0;
    std::vector<int> devices;
    long batch = 500000;
    bool verbose = false, unmapped_out = false, pbat = false, bam = false, print_parts = false, print_plan = false, sort_out = false, bai_out = false, markdup = false;
    std::string methyl;                          // --methyl <prefix>: <prefix>_CpG.bedGraph ... from the sorted file's records
    bmbs_methyl_params mpar = {0, 10, 5, 0};     // --CpG (the default) --CHG --CHH, --methyl-min-mapq, --methyl-min-phred
    double sort_mem_gib = 0;                     // --sort-mem: cap of the in-memory record store of --sort (0: half of the machine's memory)
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto val = [&]() -> const char* { if (i + 1 >= argc) { fprintf(stderr, "missing value for %s\n", a.c_str()); exit(2); } return argv[++i]; };
        if (a == "--search") index = val();
        else if (a == "--index") build_fasta = val();                 // Process_CommandLines.cpp:107, 364-381
        else if (a == "--index_folder") index_folder = val();
        else if (a == "--seq") seq = val();
        else if (a == "--seq1") seq1 = val();
        else if (a == "--seq2") seq2 = val();
        else if (a == "-o") out = val();
        else if (a == "-e") P.e_f = atof(val());
        else if (a == "--min") P.min_ins = atoi(val());
        else if (a == "--max") P.max_ins = atoi(val());
        else if (a == "--mp_max") P.mp_max = atoi(val());
        else if (a == "--mp_min") P.mp_min = atoi(val());
        else if (a == "--np") P.np = atoi(val());
        else if (a == "--gap_open") P.gap_open = atoi(val());
        else if (a == "--gap_extension") P.gap_ext = atoi(val());
        else if (a == "--seed") P.seed_len = atoi(val());
        else if (a == "--phred33") P.q_base = 33;
        else if (a == "--phred64") P.q_base = 64;
        else if (a == "--sensitive") P.sensitive = 1;
        else if (a == "--fast") P.sensitive = 0;
        else if (a == "--pe") {}
        else if (a == "-t") io_threads = atoi(val());    // the reference's mapping threads; here: host I/O threads (the GPU maps)
        else if (a == "--mapstats") mapstats = val();
        else if (a == "--device") device = atoi(val());
        else if (a == "--devices") {                                  // comma-separated device ids, one index copy each
            const char* v = val();
            devices.clear();
            for (const char* q = v; *q;) { devices.push_back(atoi(q)); while (*q && *q != ',') q++; if (*q == ',') q++; }
        }
        else if (a == "--contexts") contexts = atoi(val());
        else if (a == "--batch") batch = atol(val());
        else if (a == "--loop-input") g_loop_input = std::max(1, atoi(val()));
        else if (a == "--out-parts") parts = atoi(val());
        else if (a == "--print-plan") print_parts = print_plan = true;           // ... and how the parts are worked off: devices, contexts, workers (no GPU needed: tests)
        else if (a == "--print-parts") print_parts = true;                   // the record ranges --out-parts would use, then exit (no GPU needed: tests)
        else if (a == "--reader-threads") reader_threads = atoi(val());     // pread threads per part (default: -t / (2 x parts))
        else if (a == "--verbose") verbose = true;
        else if (a == "--unmapped_out") unmapped_out = true;          // Process_CommandLines.cpp:104-105
        else if (a == "--ambiguous_out") P.ambiguous_out = 1;
        else if (a == "--pbat") pbat = true;                          // Process_CommandLines.cpp:93
        else if (a == "--bam") bam = true;                            // Process_CommandLines.cpp:94-95
        else if (a == "--sam") bam = false;
        else if (a == "--sort") sort_out = true;                      // --bam --sort: one coordinate-sorted BAM file (sorted on the device)
        else if (a == "--sort-mem") sort_mem_gib = atof(val());
        else if (a == "--markdup") markdup = true;                   // --bam --sort --markdup: flag 0x400 on PCR duplicates, decided on the device
        else if (a == "--bai") bai_out = true;                        // --bam --sort --bai: <out>.bai beside the sorted file, from the same run
        else if (a == "--methyl") methyl = val();                     // --bam --sort --methyl <prefix>: methylation counts per cytosine, from the device
        else if (a == "--CpG") mpar.contexts |= 1;                    // (the reference's names for the contexts of its own extractor)
        else if (a == "--CHG") mpar.contexts |= 2;
        else if (a == "--CHH") mpar.contexts |= 4;
        else if (a == "--methyl-min-mapq") mpar.min_mapq = atoi(val());
        else if (a == "--methyl-min-phred") mpar.min_phred = atoi(val());
        else { fprintf(stderr, "bmbs_search: unsupported option %s\n", a.c_str()); return 2; }
    }
    if (sort_out && !bam) { fprintf(stderr, "bmbs_search: --sort needs --bam\n"); return 2; }
    if (sort_out && parts > 1) { fprintf(stderr, "bmbs_search: --sort writes one file (--out-parts 1)\n"); return 2; }
    if (bai_out && !sort_out) { fprintf(stderr, "bmbs_search: --bai needs --sort\n"); return 2; }
    if (markdup && !sort_out) { fprintf(stderr, "bmbs_search: --markdup needs --sort\n"); return 2; }
    const bool methyl_out = !methyl.empty();
    if (methyl_out && !sort_out) { fprintf(stderr, "bmbs_search: --methyl needs --sort\n"); return 2; }
    if (!methyl_out && (mpar.contexts || mpar.min_mapq != 10 || mpar.min_phred != 5)) { fprintf(stderr, "bmbs_search: --CpG, --CHG, --CHH, --methyl-min-mapq and --methyl-min-phred need --methyl\n"); return 2; }
    if (mpar.min_mapq < 0 || mpar.min_mapq > 255 || mpar.min_phred < 0 || mpar.min_phred > 255) { fprintf(stderr, "bmbs_search: --methyl-min-mapq and --methyl-min-phred take 0..255\n"); return 2; }
    if (!mpar.contexts) mpar.contexts = 1;
    if (bai_out) {
        // the index lies beside a file: a device or a pipe has no such place
        struct stat osb;
        if (stat(out.c_str(), &osb) == 0 && !S_ISREG(osb.st_mode)) { fprintf(stderr, "bmbs_search: --bai needs a regular output file (-o %s is none)\n", out.c_str()); return 2; }
    }
    if (!build_fasta.empty()) {
        // bitmapperBS --index <fasta> [--index_folder <dir>]: <fasta>.index* or <dir>/genome.index* (Index.cpp:832-938)
        std::string prefix = build_fasta;
        if (!index_folder.empty()) {
            while (index_folder.size() > 1 && index_folder.back() == '/') index_folder.pop_back();
            ::mkdir(index_folder.c_str(), 0755);
            prefix = index_folder + "/genome";
        }
        if (io_threads <= 0) io_threads = (int)std::thread::hardware_concurrency();
        const double t0 = now();
        const int rc = bmbs_index_build(build_fasta.c_str(), prefix.c_str(), io_threads < 1 ? 1 : io_threads);
        if (rc) { fprintf(stderr, "bmbs_search: index build failed (%d)\n", rc); return 1; }
        fprintf(stderr, "index written to %s.index* in %.1f s\n", prefix.c_str(), now() - t0);
        return 0;
    }
    if (index.empty() || (seq.empty() && (seq1.empty() || seq2.empty()))) {
        fprintf(stderr, "usage: bmbs_search --index <genome.fa> [--index_folder dir] [-t threads]\n       bmbs_search --search <index> (--seq r.fq | --seq1 a.fq --seq2 b.fq) [-o out.sam] [-e f] [--min n] [--max n] [--sensitive] [--pbat] [--unmapped_out] [--ambiguous_out] [--bam [--sort [--sort-mem GiB] [--markdup] [--bai] [--methyl prefix [--CpG] [--CHG] [--CHH] [--methyl-min-mapq n] [--methyl-min-phred n]]]] [--mapstats f] [-t io_threads] [--out-parts n]\n");
        return 2;
    }
    if (batch < 1) batch = 1;
    if (io_threads <= 0) {
        // plain text needs few threads to read at memory speed; compressed input is inflated by them (csrc/pgz.h): more pay off
        const bool zin = Source::is_gz(seq.empty() ? seq1.c_str() : seq.c_str());
        const int hw = (int)std::thread::hardware_concurrency();
        // what the process may actually use: a container's CPU quota (cgroup v2 cpu.max "quota period") is often far below the hardware
        // threads it can see -- 16 cores' worth of 256 on the MI355X boxes -- and inflating on four times as many threads as that is slower
        int eff = hw;
        if (FILE* cf = fopen("/sys/fs/cgroup/cpu.max", "r")) {
            long long quota = 0, period = 0;
            if (fscanf(cf, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0) eff = (int)std::max<long long>(1, std::min<long long>(hw, (quota + period - 1) / period));
            fclose(cf);
        }
        io_threads = zin ? std::min(std::max(1, eff), 64) : std::min(hw, 32);
    }
    if (io_threads < 1) io_threads = 1;
    if (parts < 1) parts = 1;
    if (parts > 64) parts = 64;
    const double t_start = now();
    if (devices.empty()) devices.push_back(device);
    if (contexts < 1) contexts = 1;
    const bool pe = seq.empty();
    // --pbat: single-end reads are mapped as their reverse complement with mirrored qualities (inputReads_single_directly_pbat,
    // Process_Reads.cpp:986-1075; Schema.cpp:15102 need_reverse_quality = 1); paired-end input files swap roles
    // (exchange_two_reads, Process_Reads.cpp:1628, called from Bitmapper_main.cpp:169)
    if (pbat && pe) std::swap(seq1, seq2);
    const std::string& in1 = pe ? seq1 : seq;
    const bool gz_in = Source::is_gz(in1.c_str()) || (pe && Source::is_gz(seq2.c_str()));
    // a .gz stream cannot be entered in the middle: everything goes through part 0, the other part files stay empty
    const int live_parts = gz_in ? 1 : parts;
    // where the parts begin: byte offsets of record starts, the same record in both files of a pair (plain files; a .gz stream cannot
    // be entered in the middle)
    auto compute_cuts = [&](std::vector<size_t>& cut1, std::vector<size_t>& cut2) -> bool {
        cut1.assign((size_t)live_parts + 1, 0); cut2.assign((size_t)live_parts + 1, 0);
        if (gz_in) { cut1[1] = cut2[1] = ~(size_t)0; return true; }
        Pool pool(std::max(1, io_threads / 2) - 1);
        const int fd1 = ::open(in1.c_str(), O_RDONLY), fd2 = pe ? ::open(seq2.c_str(), O_RDONLY) : -1;
        struct stat sb1, sb2;
        if (fd1 < 0 || fstat(fd1, &sb1) || (pe && (fd2 < 0 || fstat(fd2, &sb2)))) return false;
        const size_t size1 = (size_t)sb1.st_size, size2 = pe ? (size_t)sb2.st_size : 0;
        cut1[(size_t)live_parts] = size1; cut2[(size_t)live_parts] = size2;
        for (int p = 1; p < live_parts; p++) {
            cut1[(size_t)p] = std::max(cut1[(size_t)p - 1], record_start_at(fd1, size1, (size_t)((double)size1 * p / live_parts)));
            if (pe) cut2[(size_t)p] = std::max(cut2[(size_t)p - 1], mate_boundary(pool, fd1, size1, cut1[(size_t)p], fd2, size2));
        }
        ::close(fd1); if (fd2 >= 0) ::close(fd2);
        return true;
    };
    if (print_parts) {
        std::vector<size_t> cut1, cut2;
        if (!compute_cuts(cut1, cut2)) { fprintf(stderr, "Cannot open the read file(s)\n"); return 1; }
        for (int p = 0; p <= live_parts; p++) printf("%d\t%zu\t%zu\n", p, cut1[(size_t)p], cut2[(size_t)p]);
        if (print_plan) {
            // record ranges of the input -> GPUs, index replicated, no exchange step, output concatenated in range order.
            // Here a range is a part; its batches go to whichever context is free (one worker thread per context, `contexts` contexts
            // on every listed device sharing that device's index copy) and come back in order through the part's own queue.
            printf("plan\tdevices\t%zu\tcontexts_per_device\t%d\tworkers\t%zu\tparts\t%d\tbatches_in_flight\t%zu\tbatch\t%ld\n",
                   devices.size(), contexts, devices.size() * (size_t)contexts, live_parts, (size_t)live_parts + devices.size() * (size_t)contexts + 2, batch);
            for (size_t d = 0; d < devices.size(); d++) printf("device\t%d\tindex_copy\t1\tcontexts\t%d\n", devices[d], contexts);
            printf("stats\tsum over %zu contexts (bmbs_stats_allreduce)\n", devices.size() * (size_t)contexts);
        }
        return 0;
    }
    // the drivers' contexts run one batch at a time each: one lane per context is enough (BMBS_LANES is only read by bmbs_create)
    setenv("BMBS_LANES", "1", 0);
    const int n_ctx = (int)devices.size() * contexts;
    const int n_batches = live_parts + n_ctx + 2;
    std::vector<Batch> batches((size_t)n_batches);
    for (auto& b : batches) { b.text1.kind = 1; b.text2.kind = 1; b.sam.kind = 2; }
    // bytes per record of the input, from its first records (plain text): sizes the page-locked windows, which cost ~0.2 ms per MB
    // to pin and are therefore allocated once, by several threads, while the index loads
    size_t est0 = 400;
    {
        char head[1 << 16];
        FILE* fp = fopen(in1.c_str(), "rb");
        const size_t got = fp ? fread(head, 1, sizeof head, fp) : 0;
        if (fp) fclose(fp);
        if (got > 2 && !((unsigned char)head[0] == 0x1f && (unsigned char)head[1] == 0x8b)) {
            size_t lines = 0, last = 0;
            for (size_t i = 0; i < got; i++) if (head[i] == '\n') { lines++; if (lines % 4 == 0) last = i + 1; }
            if (lines >= 4) est0 = std::max<size_t>(est0, last / (lines / 4) + 32);
        }
    }
    if (is_dir(index)) index += "/genome";           // Index.cpp:1048-1069
    bmbs_index_file* ixf = bmbs_index_file_load(index.c_str());
    if (!ixf) { fprintf(stderr, "Cannot open index %s.index*\n", index.c_str()); return 1; }
    bmbs_index_view view; bmbs_index_file_view(ixf, &view);
    std::vector<std::string> chrom_names;
    size_t max_chrom = 0;
    for (int i = 0; i < view.n_chrom; i++) { chrom_names.push_back(bmbs_index_file_chrom_name(ixf, i)); max_chrom = std::max(max_chrom, chrom_names.back().size()); }
    if (bai_out)
        for (int i = 0; i < view.n_chrom; i++)
            if (view.chrom_len[i] > (1ull << 29)) {
                fprintf(stderr, "bmbs_search: --bai: sequence %s is longer than 2^29 bases: a BAI index cannot hold it (CSI is not written)\n", chrom_names[(size_t)i].c_str());
                return 2;
            }
    // SAM bytes a batch can need: QNAME + SEQ + QUAL come out of the text, the other columns are bounded per line
    const int L_est = (int)std::min<size_t>(1000, (est0 / 2) + (est0 / 4));
    auto sam_bound = [&](size_t text_bytes, size_t lines, int L) {
        return text_bytes + lines * (max_chrom + 5 * (size_t)std::max(8, (int)bmbs_max_cigar_ops(&P, std::max(1, std::min(1000, L)))) + 96) + 4096;
    };
    auto window_bytes = [&](size_t est) { return std::min<size_t>((size_t)batch * est + (1u << 16), (size_t)4000 << 20); };
    // BGZF input that is inflated on the device: the compressed bytes of a window, staged (block tables and a page-locked copy per
    // file).  Two of them: while a context opens one window, a helper thread stages the next
    struct Staged {
        Pinned buf[2]; std::vector<uint64_t> blk[2], out[2];
        size_t a[2] = {0, 0}, q[2] = {0, 0};
        bool foreign_any = false, ok = true; std::string err;
        bool last[2] = {false, false};               // the window ends its file (--loop-input: for the last time)
    } zst[2];
    for (auto& x : zst) { x.buf[0].kind = 1; x.buf[1].kind = 1; }
    std::thread prealloc([&] {
        const size_t want = window_bytes(est0) + 64;
        std::vector<std::thread> th;
        if (gz_in)
            for (auto& x : zst)
                for (int f = 0; f < (pe ? 2 : 1); f++) {
                    struct stat sb;
                    const size_t fsize = stat((f ? seq2 : in1).c_str(), &sb) == 0 ? (size_t)sb.st_size : 0;
                    Pinned* pb = &x.buf[f];
                    th.emplace_back([pb, fsize, want] { pb->need(std::min(fsize + 64, want / 2)); });
                }
        for (auto& b : batches)
            th.emplace_back([&, want] {
                Batch* bb = &b;
                bb->text1.need(want); if (pe) bb->text2.need(want);
                bb->sam.need(sam_bound(want * (pe ? 2 : 1), (size_t)batch * (pe ? 2 : 1), L_est));
            });
        for (auto& t : th) t.join();
    });
    struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } prealloc_guard{prealloc};     // error returns below must not leave it running
    // one owner context per listed device (attached in parallel: each uploads and re-packs its own index copy), plus
    // contexts-1 further contexts per device on the owner's index (bmbs_index_share)
    std::vector<bmbs_ctx*> ctxs;                  // owners first
    for (int d : devices) {
        bmbs_ctx* c = bmbs_create(d, &P);
        if (!c) { fprintf(stderr, "bmbs_search: no usable HIP device %d (this driver has no CPU mapping path)\n", d); return 1; }
        ctxs.push_back(c);
    }
    {
        std::vector<int> rcs(ctxs.size(), 0);
        std::vector<std::thread> th;
        for (size_t i = 0; i < ctxs.size(); i++) th.emplace_back([&, i] { rcs[i] = bmbs_index_attach(ctxs[i], &view); });
        for (auto& t : th) t.join();
        for (size_t i = 0; i < ctxs.size(); i++) if (rcs[i]) { fprintf(stderr, "%s\n", bmbs_last_error(ctxs[i])); return 1; }
    }
    const size_t n_owner = ctxs.size();
    for (size_t i = 0; i < n_owner; i++)
        for (int s = 1; s < contexts; s++) {
            bmbs_ctx* c = bmbs_create(devices[i], &P);
            if (!c || bmbs_index_share(c, ctxs[i])) { fprintf(stderr, "bmbs_search: cannot create a shared context on device %d\n", devices[i]); return 1; }
            ctxs.push_back(c);
        }
    {
        std::vector<const char*> nm;
        for (const auto& s : chrom_names) nm.push_back(s.c_str());
        for (bmbs_ctx* c : ctxs) if (bmbs_sam_refs(c, nm.data(), (int32_t)nm.size())) { fprintf(stderr, "%s\n", bmbs_last_error(c)); return 1; }
    }
    // device memory for the work buffers of a batch, taken while the index loads instead of inside the first calls
    for (bmbs_ctx* c : ctxs) (void)bmbs_reserve(c, (uint64_t)batch * (pe ? 2 : 1) * (1200 + 3 * (uint64_t)std::max<size_t>(est0 / 2, 100)));
    // ---- the parts: record ranges of the input, one output file each
    std::vector<std::unique_ptr<Part>> P_(static_cast<size_t>(parts));
    for (int p = 0; p < parts; p++) { P_[(size_t)p].reset(new Part()); P_[(size_t)p]->id = p; }
    {
        std::vector<size_t> cut1, cut2;
        if (!compute_cuts(cut1, cut2)) { fprintf(stderr, "Cannot open the read file(s)\n"); return 1; }
        for (int p = 0; p < live_parts; p++) {
            Part& pt = *P_[(size_t)p];
            const int zt = std::max(1, io_threads / (pe ? 2 : 1));          // compressed input: inflate threads per file
            if (!pt.s1.open(in1.c_str(), cut1[(size_t)p], cut1[(size_t)p + 1], zt, devices[(size_t)p % devices.size()]) ||
                (pe && !pt.s2.open(seq2.c_str(), cut2[(size_t)p], cut2[(size_t)p + 1], zt, devices[(size_t)p % devices.size()]))) {
                fprintf(stderr, "Cannot open the read file(s)\n"); return 1;
            }
        }
    }
    for (int p = 0; p < parts; p++) {
        Part& pt = *P_[(size_t)p];
        std::string path = out;
        if (parts > 1) { char suf[32]; snprintf(suf, sizeof suf, ".part%03d", p); path += suf; }
        pt.ofd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (pt.ofd < 0) { fprintf(stderr, "Cannot open %s\n", path.c_str()); return 1; }
        {
            struct stat osb; pt.regular = fstat(pt.ofd, &osb) == 0 && S_ISREG(osb.st_mode);
            // blocks are reserved ahead only where that is a table entry (extent file systems): tmpfs answers fallocate by taking and
            // clearing the pages (4 GiB ahead of eight parts: slower than the writes, then ENOSPC), overlayfs refuses it
            struct statfs fsb;
            pt.can_alloc = pt.regular && fstatfs(pt.ofd, &fsb) == 0 &&
                           ((unsigned long)fsb.f_type == 0xEF53ul || (unsigned long)fsb.f_type == 0x58465342ul || (unsigned long)fsb.f_type == 0x9123683Eul);
        }
        if (p == 0) {
            // OutPutSAM_Nounheader (Process_sam_out.cpp:1137-1153)
            std::string h = sort_out ? "@HD\tVN:1.4\tSO:coordinate\n" : "@HD\tVN:1.4\tSO:unsorted\n";
            for (int i = 0; i < view.n_chrom; i++) { h += "@SQ\tSN:" + chrom_names[(size_t)i] + "\tLN:"; put_uint(h, view.chrom_len[i]); h += '\n'; }
            h += "@PG\tID:BitMapperBS\tVN:1.0.2.3\tCL:";
            // (--methyl and its options shape no byte of this file, so they stay out of its header: the BAM and its .bai are the same
            // bytes with and without them)
            for (int i = 0; i < argc; i++) {
                const std::string a = argv[i];
                if (a == "--methyl" || a == "--methyl-min-mapq" || a == "--methyl-min-phred") { i++; continue; }
                if (a == "--CpG" || a == "--CHG" || a == "--CHH") continue;
                h += a; h += ' ';
            }
            h += '\n';
            if (bam) {
                // BAM header: magic, the same text, the reference dictionary; one BGZF block series
                std::vector<char> hb = {'B', 'A', 'M', 1}, z;
                put_le32(hb, (uint32_t)h.size()); hb.insert(hb.end(), h.begin(), h.end());
                put_le32(hb, (uint32_t)view.n_chrom);
                for (int i = 0; i < view.n_chrom; i++) {
                    const std::string& nm = chrom_names[(size_t)i];
                    put_le32(hb, (uint32_t)nm.size() + 1); hb.insert(hb.end(), nm.begin(), nm.end()); hb.push_back(0);
                    put_le32(hb, (uint32_t)view.chrom_len[i]);
                }
                bgzf_append(hb.data(), hb.size(), z);
                h.assign(z.begin(), z.end());
            }
            if (pwrite(pt.ofd, h.data(), h.size(), 0) != (ssize_t)h.size()) { fprintf(stderr, "write error on %s\n", path.c_str()); return 1; }
            pt.out_off = h.size();
        }
    }
    prealloc.join();
    // the device touches every staging buffer once now (BMBS_NO_PREFAULT=1 skips it)
    if (!getenv("BMBS_NO_PREFAULT")) {
        std::vector<std::thread> th;
        for (size_t i = 0; i < batches.size(); i++)
            th.emplace_back([&, i] {
                Batch& b = batches[i];
                bmbs_ctx* c = ctxs[i % ctxs.size()];
                if (b.text1.p) (void)bmbs_host_prefault(c, b.text1.p, b.text1.cap, 1);
                if (b.text2.p) (void)bmbs_host_prefault(c, b.text2.p, b.text2.cap, 1);
                if (b.sam.p) (void)bmbs_host_prefault(c, b.sam.p, b.sam.cap, 2);
            });
        for (auto& t : th) t.join();
    }
    const int32_t flags = (pbat && !pe ? BMBS_TEXT_PBAT : 0) | (unmapped_out ? BMBS_TEXT_UNMAPPED : 0) | (bam ? BMBS_TEXT_BAM : 0) | (sort_out ? BMBS_TEXT_BAM_SORTED : 0);
    // --sort: the store of pass 1.  Bins: BMBS_SORT_BINS, by default 4096 of equal genomic length (0.76 Mbp of a human genome each) + one
    // for records without a reference; its cap: --sort-mem, by default half of the machine's memory
    SortStore sort_store;
    if (sort_out) {
        const char* e = getenv("BMBS_SORT_BINS");
        sort_store.init(view, e ? atol(e) : 4096);
        const double phys = (double)sysconf(_SC_PHYS_PAGES) * (double)sysconf(_SC_PAGE_SIZE);
        sort_store.cap = (size_t)(sort_mem_gib > 0 ? sort_mem_gib * 1073741824.0 : phys / 2);
    }
    const double t_loaded = now();

    Chan<Batch*> free_q, gpu_q;
    for (auto& b : batches) free_q.put(&b);
    std::atomic<bool> failed(false);
    std::mutex err_mu;
    auto fail = [&](const std::string& why) { std::lock_guard<std::mutex> l(err_mu); if (!failed.exchange(true)) fprintf(stderr, "bmbs_search: %s\n", why.c_str()); };
    // the writers only pwrite (SAM text or finished BGZF blocks), every I/O thread reads
    const int r_threads = reader_threads > 0 ? reader_threads : std::max(1, io_threads / live_parts);

    // ---------------- stage R (one per part): text window + newline count -> how many whole records ----------------------------
    // BGZF input that stays on the device (bmbs_text_open_bgzf / bmbs_text_map_open): the reader hands the compressed blocks of a window
    // to a context, learns how many whole records they held and what is left over (the next window's prefix), and passes the context on
    // to a worker for the mapping.  The inflated text never crosses the link -- the host moves compressed bytes and tails only.
    Chan<bmbs_ctx*> ctx_pool;
    auto z_mode = [&](Part* pt) { return pt->s1.zdirect && (!pe || pt->s2.zdirect); };
    if (live_parts == 1 && z_mode(P_[0].get())) for (bmbs_ctx* c : ctxs) ctx_pool.put(c);
    // true: the input is finished (or failed); false: go on with the host-window reader (a member that is not a BGZF block turned up)
    auto reader_z = [&](Part* pt, Pool& pool, Pool& pool2) -> bool {
        size_t est = est0;
        Pinned tails[2]; tails[0].kind = 2; tails[1].kind = 2;
        // (what a window leaves over is a partial record, plus -- when the mates' records differ in size -- the surplus of one file, which the
        // next window's smaller block count evens out: never more than a window)
        // in practice a fraction of a record; the buffers grow when a call says so (page-locked memory is slow to get: ~0.1 ms per MB)
        size_t tail_cap = (size_t)4 << 20;
        if (const char* tv = getenv("BMBS_Z_TAIL")) { const long v = atol(tv); if (v >= 1) tail_cap = (size_t)v; }      // tests: the growth path
        if (!tails[0].need(tail_cap) || (pe && !tails[1].need(tail_cap))) { fail("cannot allocate page-locked staging memory"); return true; }
        Source* S[2] = {&pt->s1, &pt->s2};
        const int nf = pe ? 2 : 1;
        // (zst: the two staged windows -- while a context opens one (upload, inflate, index: the reader waits for the device), a helper
        // thread stages the next)
        Staged* st = zst;
        auto stage = [&](Staged& g, size_t room0, size_t room1) {
            g.foreign_any = false; g.ok = true;
            const size_t room[2] = {room0, room1};
            for (int f = 0; f < nf && g.ok; f++) {
                Source& s = *S[f];
                bool foreign = false;
                if (!s.next_blocks(room[f], g.a[f], g.q[f], foreign)) { g.ok = false; g.err = s.err; break; }
                if (foreign && g.q[f] == g.a[f]) { g.foreign_any = true; continue; }
                g.blk[f] = s.zblk; g.out[f] = s.zout;
                const size_t zbytes = g.q[f] - g.a[f];
                if (zbytes) {
                    if (!g.buf[f].need(zbytes + 64)) { g.ok = false; g.err = "cannot allocate page-locked staging memory"; break; }
                    Pool& pl = f ? pool2 : pool;
                    const int T = pl.size() * 2;
                    const size_t per = ((zbytes + (size_t)T - 1) / (size_t)T + 4095) & ~(size_t)4095;
                    char* dst = g.buf[f].p; const unsigned char* src = s.zmap + g.a[f];
                    pl.run(T, [&](int t) { const size_t x = std::min(zbytes, per * (size_t)t), y = std::min(zbytes, x + per); if (x < y) memcpy(dst + x, src + x, y - x); });
                }
                s.znext = g.q[f];
                g.last[f] = g.q[f] >= s.zsize && s.loops_left == 0;
                if (g.q[f] >= s.zsize && s.loops_left > 0) { s.znext = 0; s.loops_left--; }      // --loop-input: the file once more
            }
        };
        auto room_for = [&](size_t est_now, int f) {
            const size_t target = std::min<size_t>((size_t)batch * est_now + (1u << 16), (size_t)3500 << 20);
            return target > S[f]->carry.size() ? target - S[f]->carry.size() : (size_t)0;
        };
        int cur = 0;
        stage(st[0], room_for(est, 0), pe ? room_for(est, 1) : 0);
        std::thread ahead;
        auto join_ahead = [&] { if (ahead.joinable()) ahead.join(); };
        struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{ahead};
        for (;;) {
            const double tw0 = now();
            Batch* b = free_q.get();
            bmbs_ctx* ctx = ctx_pool.get();
            const double t0 = now();
            pt->t_wait_r += t0 - tw0;
            b->part = pt; b->seq = pt->next_seq++; b->n = 0; b->end = false; b->used1 = b->used2 = 0; b->sam_bytes = 0; b->open_ctx = nullptr;
            auto bail = [&](const std::string& why) { join_ahead(); fail(why); b->end = true; b->n = 0; ctx_pool.put(ctx); gpu_q.put(b); };
            if (failed) { join_ahead(); b->end = true; ctx_pool.put(ctx); gpu_q.put(b); return true; }
            join_ahead();
            Staged& g = st[cur];
            if (!g.ok) { bail(g.err); return true; }
            const size_t target = std::min<size_t>((size_t)batch * est + (1u << 16), (size_t)3500 << 20);
            bmbs_ztext z[2]; memset(z, 0, sizeof z);
            if (g.foreign_any) {
                // the rest of such a file goes through the host's stream inflater; blocks already taken for this window are given back
                for (int f = 0; f < nf; f++) {
                    Source& s = *S[f];
                    s.znext = g.a[f];
                    if (s.znext < s.zsize && !s.bgzf_block(s.zmap + s.znext, s.zsize - s.znext)) { std::lock_guard<std::mutex> l(s.m); s.zdirect = false; const size_t at = s.znext; s.znext = s.zsize; s.start_pgz(at, 0); }
                }
                pt->next_seq--;                                     // (the batch was not used)
                free_q.put(b);
                // every window opened so far has to be mapped before the workers go back to contexts of their own
                for (size_t i = 1; i < ctxs.size(); i++) (void)ctx_pool.get();
                return false;
            }
            size_t text_bytes = 0;
            for (int f = 0; f < nf; f++) {
                Source& s = *S[f];
                z[f].prefix = s.carry.empty() ? nullptr : s.carry.data(); z[f].prefix_bytes = s.carry.size();
                z[f].comp = g.buf[f].p; z[f].comp_bytes = g.q[f] - g.a[f]; z[f].blk_off = g.blk[f].data(); z[f].out_off = g.out[f].data(); z[f].n_blocks = (int64_t)g.blk[f].size() - 1;
                text_bytes += s.carry.size() + (size_t)g.out[f].back();
            }
            const bool last1 = g.last[0], last2 = pe && g.last[1];
            // the window behind this one is staged while the device works on this one (what this window will leave over is not known
            // yet: the last window's leftover stands in for it when the room is measured)
            {
                const size_t r0 = room_for(est, 0), r1 = pe ? room_for(est, 1) : 0;
                Staged* nx = &st[cur ^ 1];
                ahead = std::thread([&stage, nx, r0, r1] { stage(*nx, r0, r1); });
                cur ^= 1;
            }
            int64_t nrec = 0; uint64_t tb[2] = {0, 0};
            // every whole record of the window is taken (the window is what bounds a batch here: --batch records by the running estimate of a record's size)
            int rc = bmbs_text_open_bgzf(ctx, &z[0], pe ? &z[1] : nullptr, 4 * (int64_t)batch, last1 ? 1 : 0, last2 ? 1 : 0, &nrec, tails[0].p, tail_cap, &tb[0],
                                         pe ? tails[1].p : nullptr, &tb[1]);
            if (rc == BMBS_ENOMEM && std::max(tb[0], tb[1]) > tail_cap) {
                // more text behind the window's records than the tail buffers hold (the mates' records differ in size): once more with room
                tail_cap = (size_t)std::max(tb[0], tb[1]) + ((size_t)4 << 20);
                if (!tails[0].need(tail_cap) || (pe && !tails[1].need(tail_cap))) { bail("cannot allocate page-locked staging memory"); return true; }
                rc = bmbs_text_open_bgzf(ctx, &z[0], pe ? &z[1] : nullptr, 4 * (int64_t)batch, last1 ? 1 : 0, last2 ? 1 : 0, &nrec, tails[0].p, tail_cap, &tb[0],
                                         pe ? tails[1].p : nullptr, &tb[1]);
            }
            if (rc) { bail(bmbs_last_error(ctx)); return true; }
            for (int f = 0; f < nf; f++) S[f]->carry.assign(tails[f].p, tails[f].p + tb[f]);
            // the part's input ends with this batch when a file has nothing left behind it (PE: the shorter file decides)
            b->end = (last1 && tb[0] == 0) || (pe && last2 && tb[1] == 0);
            if (nrec == 0) {
                if (!b->end && (last1 || (pe && last2))) b->end = true;            // a trailing fragment that is not a whole record
                if (!b->end) { bail("FASTQ record larger than the " + std::to_string(target) + "-byte window"); return true; }
                ctx_pool.put(ctx); gpu_q.put(b);
                return true;
            }
            est = std::max<size_t>(64, text_bytes / (size_t)nf / (size_t)nrec + 16);
            b->n = nrec; b->open_ctx = ctx;
            const int Lg = (int)std::min<size_t>(1000, est / 2);
            if (!b->sam.need(sam_bound(text_bytes, (size_t)nrec * (pe ? 2 : 1), Lg))) { bail("cannot allocate page-locked staging memory"); return true; }
            pt->t_read += now() - t0;
            pt->records += nrec;
            const bool end = b->end;
            gpu_q.put(b);
            if (end) return true;
        }
    };
    auto reader_fn = [&](Part* pt) {
        Pool pool(r_threads - 1);
        Pool pool2(pe && pt->s2.gz ? std::max(1, r_threads / 2) - 1 : 0);          // second mate's window of compressed input
        if (live_parts == 1 && z_mode(pt) && reader_z(pt, pool, pool2)) return;
        size_t est = est0;
        for (;;) {
            const double tw0 = now();
            Batch* b = free_q.get();
            const double t0 = now();
            pt->t_wait_r += t0 - tw0;
            b->part = pt; b->seq = pt->next_seq++; b->n = 0; b->end = false; b->used1 = b->used2 = 0; b->sam_bytes = 0;
            auto bail = [&](const std::string& why) { fail(why); b->end = true; b->n = 0; gpu_q.put(b); };
            if (failed) { b->end = true; gpu_q.put(b); return; }
            // (.gz: what the previous window left over is copied in first and must fit whatever the new estimate says)
            const size_t want = std::max(window_bytes(est), std::max(pt->s1.carry.size(), pt->s2.carry.size()) + (1u << 16));
            if (!b->text1.need(want + 64) || (pe && !b->text2.need(want + 64))) { bail("cannot allocate page-locked staging memory"); return; }
            bool last1 = true, last2 = true;
            size_t n1 = 0, n2 = 0;
            if (pe && pt->s2.gz) {
                // compressed input: the two windows are assembled side by side (each waits for its own inflaters)
                bool ok2 = true;
                std::thread w2([&] { ok2 = pt->s2.window(pool2, b->text2.p, want, n2, last2, b->counts2); });
                const bool ok1 = pt->s1.window(pool, b->text1.p, want, n1, last1, b->counts1);
                w2.join();
                if (!ok1) { bail(pt->s1.err); return; }
                if (!ok2) { bail(pt->s2.err); return; }
            } else {
                if (!pt->s1.window(pool, b->text1.p, want, n1, last1, b->counts1)) { bail(pt->s1.err); return; }
                if (pe && !pt->s2.window(pool, b->text2.p, want, n2, last2, b->counts2)) { bail(pt->s2.err); return; }
            }
            size_t l1 = 0, l2 = 0;
            for (uint32_t c : b->counts1) l1 += c;
            for (uint32_t c : b->counts2) l2 += c;
            const long avail1 = (long)(l1 / 4), avail2 = pe ? (long)(l2 / 4) : 0;
            long nrec = pe ? std::min(avail1, avail2) : avail1;
            if (nrec > batch) nrec = batch;
            // the part's input ends with this batch when a file has no complete record left after it (PE: the shorter file decides)
            b->end = (last1 && avail1 == nrec) || (pe && last2 && avail2 == nrec);
            if (nrec == 0) {
                if (!b->end) { bail("FASTQ record larger than the " + std::to_string(want) + "-byte window"); return; }
                gpu_q.put(b);
                return;
            }
            b->used1 = after_kth_nl_blocks(b->text1.p, n1, b->counts1, (size_t)nrec * 4);
            pt->s1.consumed(b->text1.p, n1, b->used1);
            if (pe) { b->used2 = after_kth_nl_blocks(b->text2.p, n2, b->counts2, (size_t)nrec * 4); pt->s2.consumed(b->text2.p, n2, b->used2); }
            est = std::max<size_t>(64, std::max(b->used1, b->used2) / (size_t)nrec + 16);
            b->n = nrec;
            const int Lg = (int)std::min<size_t>(1000, est / 2);
            if (!b->sam.need(sam_bound(b->used1 + b->used2, (size_t)nrec * (pe ? 2 : 1), Lg))) { bail("cannot allocate page-locked staging memory"); return; }
            pt->t_read += now() - t0;
            pt->records += nrec;
            const bool end = b->end;
            gpu_q.put(b);
            if (end) return;
        }
    };

    // ---------------- stage W (one per part): the SAM text (or its BAM form) goes into the part's file, in order -----------------
    uint64_t tmpl_base = 0;                      // --markdup: template ids run over the batches in Batch.seq order (--sort: one part, one writer)
    auto writer_fn = [&](Part* pt) {
        Pool wpool(std::max(1, std::min(8, io_threads / (2 * live_parts))) - 1);       // slices of a batch written side by side
        for (;;) {
            const double tw0 = now();
            Batch* b = pt->out_q.get();
            const double t0 = now();
            pt->t_wait_w += t0 - tw0;
            const bool end = b->end;
            if (sort_out) {
                bool room = true;
                if (b->n && !failed && markdup) room = sort_store.add_sigs(wpool, b->sig.data(), (size_t)b->n_sig, tmpl_base);
                if (b->n && !failed && b->sam_bytes && room)
                    room = sort_store.add(wpool, b->sam.p, (size_t)b->sam_bytes, b->skey.data(), b->slen.data(), (size_t)b->n_sorted, markdup ? b->tmpl.data() : nullptr, tmpl_base,
                                          methyl_out && pe ? b->clip.data() : nullptr);
                if (b->n && markdup) tmpl_base += (uint64_t)b->n_sig;
                if (!room) {
                    char msg[256];
                    snprintf(msg, sizeof msg, "--sort-mem: the record store of --sort is used up (%.3f GiB allowed): %ld records fit, the run has more (spilling to disk is not implemented)",
                             (double)sort_store.cap / 1073741824.0, sort_store.records);
                    fail(msg);
                }
            } else if (b->n && !failed && b->sam_bytes) {
                const char* text = b->sam.p;
                const size_t len = (size_t)b->sam_bytes;
                // One buffered pwrite per batch extends the file under its inode lock at the speed of one memcpy (10 GB/s = 28 M SAM
                // records/s on the MI355X boxes).  With the blocks reserved ahead (fallocate in 4 GiB steps, cut back to the true size
                // at the end) several slices of a batch go into the page cache side by side: 17 GB/s (profiles/r02_write_probe.txt)
                if (pt->can_alloc && pt->out_off + len > pt->alloc_end) {
                    const size_t step = std::max<size_t>((size_t)4 << 30, 2 * len);
                    if (fallocate(pt->ofd, 0, (off_t)pt->alloc_end, (off_t)(pt->out_off + len + step - pt->alloc_end)) == 0) pt->alloc_end = pt->out_off + len + step;
                    else { pt->can_alloc = false; if (verbose && pt->alloc_end == 0) fprintf(stderr, "[bmbs_search] part %d: fallocate not available on the output (%s): one writer per batch\n", pt->id, strerror(errno)); }      // not a regular file (/dev/null, a pipe), or a file system without it
                }
                // (no fallocate -- overlayfs says ENODEV: four slices still extend a regular file a little faster than one, 12.8 against 10 GB/s)
                const int T = pt->can_alloc ? wpool.size() : (pt->regular ? std::min(4, wpool.size()) : 1);
                const size_t per = ((len + (size_t)T - 1) / (size_t)T + 4095) & ~(size_t)4095;
                wpool.run(T, [&](int t) {
                    size_t done = std::min(len, per * (size_t)t);
                    const size_t stop = std::min(len, done + per);
                    while (done < stop) {
                        const ssize_t w = pwrite(pt->ofd, text + done, stop - done, (off_t)(pt->out_off + done));
                        if (w <= 0) { fail(std::string("write error: ") + strerror(errno)); break; }
                        done += (size_t)w;
                    }
                });
                pt->out_off += len;
            }
            pt->t_write += now() - t0;
            free_q.put(b);
            if (end) return;
        }
    };

    // ---------------- stage G: one worker per context, one library call per batch ---------------------------------------
    double t_gpu = 0, t_wait_g = 0;
    std::mutex g_mu;
    auto g_worker = [&](bmbs_ctx* own_ctx) {
        for (;;) {
            bmbs_ctx* ctx = own_ctx;
            const double tw0 = now();
            Batch* b = gpu_q.get();
            if (!b) return;
            const double t0 = now();
            bmbs_ctx* octx = b->open_ctx;                                        // compressed input on the device: the batch's window is open on this context
            b->open_ctx = nullptr;
            if (octx) ctx = octx;
            if (!failed && b->n) {
                for (int attempt = 0; attempt < 2; attempt++) {
                    uint64_t bytes = 0; int64_t lines = 0;
                    const int rc = octx ? bmbs_text_map_open(ctx, flags, b->sam.p, b->sam.cap, &bytes, &lines)
                                 : pe ? bmbs_map_pe_text(ctx, b->text1.p, b->used1, b->text2.p, b->used2, b->n, flags, b->sam.p, b->sam.cap, &bytes, &lines)
                                      : bmbs_map_se_text(ctx, b->text1.p, b->used1, b->n, flags, b->sam.p, b->sam.cap, &bytes, &lines);
                    if (rc == BMBS_ENOMEM && bytes > b->sam.cap && attempt == 0 && b->sam.need((size_t)bytes + 64)) continue;   // reads longer than guessed
                    if (rc) fail(bmbs_last_error(ctx));
                    b->sam_bytes = rc ? 0 : bytes;
                    if (sort_out && !rc) {
                        b->skey.resize((size_t)lines + 1); b->slen.resize((size_t)lines + 1);
                        if (bmbs_text_sorted_index(ctx, b->skey.data(), b->slen.data(), lines, &b->n_sorted)) { fail(bmbs_last_error(ctx)); b->sam_bytes = 0; }
                        b->n_sig = 0;
                        if (markdup && !failed) {
                            int64_t nt = 0;
                            b->sig.resize((size_t)b->n + 1); b->tmpl.resize((size_t)lines + 1);
                            if (bmbs_text_sorted_dup(ctx, b->sig.data(), b->n, &b->n_sig, b->tmpl.data(), lines, &nt)) { fail(bmbs_last_error(ctx)); b->sam_bytes = 0; }
                            else if (nt != b->n_sorted || b->n_sig != b->n) { fail("--markdup: the batch's templates do not match its records"); b->sam_bytes = 0; }
                        }
                        if (methyl_out && pe && !failed) {
                            int64_t nc = 0;
                            b->clip.resize((size_t)lines + 1);
                            if (bmbs_text_sorted_clip(ctx, b->clip.data(), lines, &nc)) { fail(bmbs_last_error(ctx)); b->sam_bytes = 0; }
                            else if (nc != b->n_sorted) { fail("--methyl: the batch's clips do not match its records"); b->sam_bytes = 0; }
                        }
                    }
                    break;
                }
            }
            { std::lock_guard<std::mutex> l(g_mu); t_wait_g += t0 - tw0; t_gpu += now() - t0; }
            if (octx) ctx_pool.put(octx);
            b->part->out_q.put(b->seq, b);
        }
    };
    std::vector<std::thread> workers;
    for (bmbs_ctx* c : ctxs) workers.emplace_back(g_worker, c);
    for (int p = 0; p < live_parts; p++) { Part* pt = P_[(size_t)p].get(); pt->writer = std::thread(writer_fn, pt); pt->reader = std::thread(reader_fn, pt); }
    for (int p = 0; p < live_parts; p++) P_[(size_t)p]->reader.join();
    for (int p = 0; p < live_parts; p++) P_[(size_t)p]->writer.join();           // every batch has passed its writer: the workers are idle
    for (size_t i = 0; i < workers.size(); i++) gpu_q.put(nullptr);
    for (auto& t : workers) t.join();
    long total_records = 0;
    double t_read = 0, t_write = 0, t_format = 0, t_wait_r = 0, t_wait_w = 0;
    for (int p = 0; p < live_parts; p++) {
        const Part& pt = *P_[(size_t)p];
        total_records += pt.records; t_read += pt.t_read; t_write += pt.t_write; t_format += pt.t_format; t_wait_r += pt.t_wait_r; t_wait_w += pt.t_wait_w;
    }
    // ---------------- --sort, pass 2: bins in key order -> bmbs_bam_sort -> BGZF blocks behind the header ------------------------------
    // Calls of at most BMBS_SORT_CALL_BYTES (default 1 GiB) of records; staged by the I/O threads into page-locked buffers, sorted and
    // deflated on the device, appended by this thread in call order.  BMBS_SORT_SLOTS staging slots (default 2) on as many contexts:
    // the staging and upload of one call run beside the kernels and the download of the other.
    const double t_pass1 = now();
    size_t sort_calls = 0, select_calls = 0, n_dup = 0;
    std::vector<uint64_t> dup_bits;              // --markdup: a bit per template id, set for duplicates
    double t_select = t_pass1;
    BaiIndex bai;
    bai.init((size_t)view.n_chrom);
    std::vector<bmbs_methyl_site> meth_sites;    // --methyl: the sites of the calls so far, merged
    if (sort_out && !failed) {
        Part& pt = *P_[0];
        const char* e = getenv("BMBS_SORT_CALL_BYTES");
        const size_t budget = (size_t)std::max(1l, e ? atol(e) : 1l << 30);
        // --markdup, between the passes: bmbs_dup_select over groups of consecutive signature bins of at most the call budget (a template's
        // group lies in one bin, in input order: bins are filled in Batch.seq order), a bit per losing template
        if (markdup) {
            dup_bits.assign(((size_t)sort_store.templates + 63) / 64 + 1, 0);
            const size_t lim = std::max<size_t>(1, budget / sizeof(bmbs_dup_sig));
            std::vector<bmbs_dup_sig> gs; std::vector<uint64_t> gg; std::vector<uint8_t> gd;
            auto run = [&] {
                if (gs.empty() || failed) { gs.clear(); gg.clear(); return; }
                gd.assign(gs.size(), 0);
                int64_t nd = 0;
                if (bmbs_dup_select(ctxs[0], gs.data(), (int64_t)gs.size(), gd.data(), &nd)) fail(bmbs_last_error(ctxs[0]));
                else for (size_t i = 0; i < gs.size(); i++) if (gd[i]) dup_bits[gg[i] >> 6] |= (uint64_t)1 << (gg[i] & 63);
                if (!failed) n_dup += (size_t)nd;
                select_calls++; gs.clear(); gg.clear();
            };
            for (SigBin& sb : sort_store.sbin) {
                if (sb.sig.empty()) continue;
                if (!gs.empty() && gs.size() + sb.sig.size() > lim) run();
                gs.insert(gs.end(), sb.sig.begin(), sb.sig.end()); gg.insert(gg.end(), sb.gid.begin(), sb.gid.end());
                std::vector<bmbs_dup_sig>().swap(sb.sig); std::vector<uint64_t>().swap(sb.gid);
            }
            run();
        }
        t_select = now();
        std::vector<SortUnit> units;
        sort_plan(sort_store, budget, units);
        sort_calls = units.size();
        size_t max_bytes = 0, max_n = 0;
        for (const SortUnit& u : units) { max_bytes = std::max(max_bytes, u.bytes); max_n = std::max(max_n, u.n); }
        e = getenv("BMBS_SORT_SLOTS");
        const int n_slots = (int)std::max<size_t>(1, std::min<size_t>({(size_t)(e ? atoi(e) : 2), ctxs.size(), units.size(), (size_t)4}));
        struct Slot { Pinned in, out; std::vector<uint32_t> len, clip; size_t unit = 0; uint64_t out_bytes = 0; BaiPieces bai; std::vector<bmbs_methyl_site> site; int64_t n_site = 0; };
        std::vector<Slot> slots((size_t)n_slots);
        if (!units.empty()) {
            // (the mapping's page-locked windows are of no use here: a call is larger than a batch)
            for (auto& b : batches) { b.text1.release(); b.text2.release(); b.sam.release(); }
            std::vector<std::thread> th;
            std::atomic<bool> ok(true);
            for (Slot& sl : slots) {
                sl.in.kind = 1; sl.out.kind = 2; sl.len.resize(max_n + 1);
                if (methyl_out && pe) sl.clip.resize(max_n + 1);
                th.emplace_back([&] { if (!sl.in.need(max_bytes + 64)) ok = false; });
                th.emplace_back([&] { if (!sl.out.need((max_bytes / 0xff00 + 1) * 65536 + 64)) ok = false; });
            }
            for (auto& t : th) t.join();
            if (!ok) fail("cannot allocate page-locked staging memory");
        }
        if (!failed && !units.empty()) {
            Chan<Slot*> free_s, staged_s;
            OrderedChan<Slot*> done_s;
            for (Slot& sl : slots) free_s.put(&sl);
            std::thread stager([&] {
                Pool spool(std::max(1, std::min(16, io_threads)) - 1);
                for (size_t i = 0; i < units.size(); i++) {
                    Slot* sl = free_s.get();
                    sl->unit = i;
                    if (!failed) sort_stage(sort_store, units[i], spool, sl->in.p, sl->len.data(), markdup ? dup_bits.data() : nullptr, methyl_out && pe ? sl->clip.data() : nullptr);
                    staged_s.put(sl);
                }
                for (int i = 0; i < n_slots; i++) staged_s.put(nullptr);
            });
            std::vector<std::thread> sorters;
            for (int w = 0; w < n_slots; w++)
                sorters.emplace_back([&, w] {
                    bmbs_ctx* ctx = ctxs[(size_t)w];
                    for (;;) {
                        Slot* sl = staged_s.get();
                        if (!sl) return;
                        const SortUnit& u = units[sl->unit];
                        sl->out_bytes = 0;
                        for (int attempt = 0; attempt < 2 && !failed; attempt++) {
                            const int rc = bmbs_bam_sort(ctx, sl->in.p, u.bytes, sl->len.data(), (int64_t)u.n, 0, sl->out.p, sl->out.cap, &sl->out_bytes);
                            if (rc == BMBS_ENOMEM && attempt == 0 && sl->out_bytes > sl->out.cap && sl->out.need((size_t)sl->out_bytes + 64)) continue;
                            if (rc) { fail(bmbs_last_error(ctx)); sl->out_bytes = 0; }
                            break;
                        }
                        if (bai_out && !failed && !sl->bai.fetch(ctx)) { fail(bmbs_last_error(ctx)); sl->out_bytes = 0; }
                        // --methyl: the call's records are still on the device (the staged copies: duplicates carry 0x400)
                        sl->n_site = 0;
                        if (methyl_out && !failed) {
                            int64_t ns = 0;
                            if (bmbs_bam_sort_methyl(ctx, pe ? sl->clip.data() : nullptr, &mpar, &ns)) { fail(bmbs_last_error(ctx)); sl->out_bytes = 0; }
                            else {
                                if ((size_t)ns > sl->site.size()) sl->site.resize((size_t)ns + (size_t)ns / 8);
                                if (bmbs_methyl_sites(ctx, sl->site.data(), (int64_t)sl->site.size(), &sl->n_site)) { fail(bmbs_last_error(ctx)); sl->out_bytes = 0; sl->n_site = 0; }
                            }
                        }
                        done_s.put((long)sl->unit, sl);
                    }
                });
            for (size_t i = 0; i < units.size(); i++) {
                Slot* sl = done_s.get();
                size_t done = 0;
                while (!failed && done < sl->out_bytes) {
                    const ssize_t w = pwrite(pt.ofd, sl->out.p + done, (size_t)sl->out_bytes - done, (off_t)(pt.out_off + done));
                    if (w <= 0) { fail(std::string("write error: ") + strerror(errno)); break; }
                    done += (size_t)w;
                }
                if (bai_out && !failed && !bai.add(sl->bai, (uint64_t)pt.out_off)) fail("--bai: a record names a sequence the header does not have");
                if (methyl_out && !failed) methyl_merge(meth_sites, sl->site.data(), (size_t)sl->n_site);
                pt.out_off += (size_t)sl->out_bytes;
                free_s.put(sl);
            }
            stager.join();
            for (auto& t : sorters) t.join();
        }
        for (Slot& sl : slots) { sl.in.release(); sl.out.release(); }
    }
    const double t_pass2 = now();
    if (bam && !failed) {
        static const unsigned char eof_block[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        Part& lastp = *P_[(size_t)parts - 1];
        if (pwrite(lastp.ofd, eof_block, 28, (off_t)lastp.out_off) != 28) failed = true;
        lastp.out_off += 28;
    }
    const double t_joined = now();
    for (int p = 0; p < parts; p++) { Part& pt = *P_[(size_t)p]; if (pt.alloc_end > pt.out_off && ftruncate(pt.ofd, (off_t)pt.out_off) != 0) failed = true; ::close(pt.ofd); if (p < live_parts) { pt.s1.close(); if (pe) pt.s2.close(); } }
    // the index: written once the file is complete
    size_t bai_bytes = 0;
    if (bai_out && !failed) {
        if (!P_[0]->regular) { fprintf(stderr, "bmbs_search: --bai needs a regular output file (-o %s is none)\n", out.c_str()); failed = true; }
        else {
            std::string ix;
            bai.serialize(ix);
            bai_bytes = ix.size();
            const int fd = ::open((out + ".bai").c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
            size_t done = 0;
            while (fd >= 0 && done < ix.size()) { const ssize_t w = ::write(fd, ix.data() + done, ix.size() - done); if (w <= 0) break; done += (size_t)w; }
            if (fd < 0 || done < ix.size() || ::close(fd) != 0) { fprintf(stderr, "bmbs_search: cannot write %s.bai: %s\n", out.c_str(), strerror(errno)); failed = true; }
        }
    }
    // --methyl: the files, written once the BAM is complete; sites that touch a base the FASTA does not spell A, C, G or T are left out
    static const char* const ctx_names[3] = {"CpG", "CHG", "CHH"};
    size_t meth_n[3] = {0, 0, 0}, meth_calls[3] = {0, 0, 0}, meth_dropped = 0;
    if (methyl_out && !failed) {
        std::vector<std::vector<std::pair<int64_t, int64_t>>> runs;
        if (!non_acgt_runs(index, view, runs)) fprintf(stderr, "bmbs_search: --methyl: cannot read the sequences of the index from %s: sites at bases other than A, C, G and T are not filtered out\n", index.c_str());
        else {
            size_t kept = 0;
            for (const bmbs_methyl_site& s : meth_sites) if (runs[(size_t)s.ref].empty() || !methyl_touches(runs[(size_t)s.ref], s)) meth_sites[kept++] = s;
            meth_dropped = meth_sites.size() - kept;
            meth_sites.resize(kept);
        }
        for (const bmbs_methyl_site& s : meth_sites) { meth_n[s.kind & 3u]++; meth_calls[s.kind & 3u] += (size_t)s.meth + s.unmeth; }
        for (unsigned x = 0; x < 3 && !failed; x++) {
            if (!((mpar.contexts >> x) & 1)) continue;
            const std::string path = methyl + "_" + ctx_names[x] + ".bedGraph";
            if (!methyl_write(path, methyl, ctx_names[x], x, meth_sites, ixf)) { fprintf(stderr, "bmbs_search: cannot write %s: %s\n", path.c_str(), strerror(errno)); failed = true; }
        }
    }
    if (failed && methyl_out) for (unsigned x = 0; x < 3; x++) if ((mpar.contexts >> x) & 1) ::unlink((methyl + "_" + ctx_names[x] + ".bedGraph").c_str());
    if (failed && sort_out && P_[0]->regular) ::unlink(out.c_str());      // a sorted file is whole or absent (a device or a pipe is left alone)
    if (failed && bai_out && P_[0]->regular) ::unlink((out + ".bai").c_str());      // ... and so is its index
    if (failed) { fprintf(stderr, "bmbs_search: failed\n"); return 1; }
    int64_t st[5];
    bmbs_stats_allreduce(ctxs.data(), (int)ctxs.size(), st);      // get_mapping_informations: the counters of every worker summed
    print_stats(stderr, st);
    if (!mapstats.empty()) { FILE* m = fopen(mapstats.c_str(), "w"); if (m) { print_stats(m, st); fclose(m); } }
    const double t_end = now();
    for (int p = 0; p < live_parts; p++) { P_[(size_t)p]->s1.release_device(); P_[(size_t)p]->s2.release_device(); }
    if (verbose)
        fprintf(stderr, "[bmbs_search] records %ld  load+attach %.3fs  mapping wall %.3fs  (pipeline %.3fs; stage busy, summed over %d part(s): read + newline count %.3fs, gpu calls %.3fs over %d context(s), host format %.3fs, write %.3fs)  %d I/O threads, batch %ld, %zu device(s) x %d context(s), %d output part(s)\n",
                total_records, t_loaded - t_start, t_end - t_loaded, t_joined - t_loaded, live_parts, t_read, t_gpu, n_ctx, t_format, t_write, io_threads, batch,
                n_owner, contexts, parts);
    if (verbose && sort_out) {
        char ixs[640] = "";
        if (bai_out) snprintf(ixs, sizeof ixs, ", index: chunks %zu, windows %zu, %zu bytes", bai.n_chunks(), bai.n_windows(), bai_bytes);
        if (markdup)
            snprintf(ixs + strlen(ixs), sizeof ixs - strlen(ixs), ", markdup: templates %ld, with signature %ld, duplicates %zu (select calls %zu, %.3fs of pass 2)", sort_store.templates,
                     sort_store.with_sig, n_dup, select_calls, t_select - t_pass1);
        if (methyl_out)
            snprintf(ixs + strlen(ixs), sizeof ixs - strlen(ixs), ", methyl: sites CpG %zu CHG %zu CHH %zu, calls CpG %zu CHG %zu CHH %zu, sites left out at bases other than ACGT %zu", meth_n[0],
                     meth_n[1], meth_n[2], meth_calls[0], meth_calls[1], meth_calls[2], meth_dropped);
        fprintf(stderr, "[bmbs_search] sort: bins %zu (one of them for records without a reference), pass-2 calls %zu, store bytes %zu (%ld records), pass 1 %.3fs (mapping, binning), pass 2 %.3fs (sort, deflate, write)%s\n",
                sort_store.bin.size(), sort_calls, sort_store.bytes, sort_store.records, t_pass1 - t_loaded, t_pass2 - t_pass1, ixs);
    }
    if (verbose)
        fprintf(stderr, "[bmbs_search] stage idle (waiting for a batch, summed): readers %.3fs, gpu workers %.3fs, writers %.3fs\n", t_wait_r, t_wait_g, t_wait_w);
    if (verbose) {
        // what bounds the run: the link's busy time per direction (copies of the text calls, summed over the contexts: one copy per direction
        // and device at a time) and the workers' busy time against the mapping wall
        double up = 0, down = 0, in_calls = 0, calls = 0;
        for (bmbs_ctx* c : ctxs) { double t4[4]; if (bmbs_text_times(c, t4) == 0) { up += t4[0]; down += t4[1]; in_calls += t4[2]; calls += t4[3]; } }
        const double wall_s = t_end - t_loaded, nd = (double)std::max<size_t>(1, n_owner);
        fprintf(stderr, "[bmbs_search] busy fractions of the mapping wall: link up %.3f, link down %.3f (per device), gpu workers %.3f, readers %.3f, writers %.3f  (text calls %.0f, %.3fs inside them)\n",
                up / nd / wall_s, down / nd / wall_s, t_gpu / std::max(1, n_ctx) / wall_s, t_read / std::max(1, live_parts) / wall_s, t_write / std::max(1, live_parts) / wall_s, calls, in_calls);
    }
    const double t0 = now();
    for (auto& b : batches) { b.text1.release(); b.text2.release(); b.sam.release(); }
    const double t1 = now();
    for (size_t i = ctxs.size(); i-- > 0;) bmbs_destroy(ctxs[i]);     // the sharing contexts go before their owners
    const double t2 = now();
    bmbs_index_file_free(ixf);
    if (verbose) fprintf(stderr, "[bmbs_search] teardown: unpin %.3fs, destroy ctx %.3fs, free index %.3fs\n", t1 - t0, t2 - t1, now() - t2);
    return 0;
}
#endif
