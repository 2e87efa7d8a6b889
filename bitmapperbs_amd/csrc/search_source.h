// bitmapperbs_amd/csrc/search_source.h -- the driver's FASTQ reader (plain, gzip and BGZF input, window by window) and the cutting of
// plain input into parts at record boundaries (bmbs_search.cpp, bmbs_reader_test.cpp)
#pragma once
#include "search_util.h"
#include "pgz.h"
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <memory>

// ---- FASTQ text source over a byte range of a file.  Plain files: parallel pread()s straight into the batch's page-locked window,
// the newlines counted per 64 KiB block by the thread that has just read it.  .gz: a thread of its own inflates into a queue of
// chunks (so that the two files of a paired-end run inflate side by side) and the window is assembled from them. ---------------
#define SUB_BLOCK ((size_t)1 << 16)
// --loop-input N (measurement aid; plain FASTQ, and BGZF input that is inflated on the device): a part's byte range is read N times over, so that a run lasts seconds on an input
// that fits the page cache (the pipeline's fill and the contexts' first calls then weigh what they weigh in a real run)
inline int g_loop_input = 1;
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
inline size_t after_kth_nl_blocks(const char* p, size_t len, const std::vector<uint32_t>& counts, size_t k)
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
inline size_t record_start_at(int fd, size_t size, size_t guess)
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
inline std::string cut_name_at(int fd, size_t size, size_t at)
{
    char b[4096];
    const size_t n = std::min(sizeof b, size - at);
    const ssize_t g = pread(fd, b, n, (off_t)at);
    std::string s;
    for (ssize_t i = 0; i < g && b[i] != '\n' && b[i] != ' ' && b[i] != '/'; i++) s += b[i];
    return s;
}
inline size_t next_record(int fd, size_t size, size_t at)       // start of the record after the one at `at`
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
inline size_t count_lines(Pool& pool, int fd, size_t a, size_t b)                 // newlines of file bytes [a, b)
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
inline size_t offset_of_line(Pool& pool, int fd, size_t size, size_t line)          // offset of the first byte of line `line` (0-based)
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
inline size_t mate_boundary(Pool& pool, int fd1, size_t size1, size_t b1, int fd2, size_t size2)
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
