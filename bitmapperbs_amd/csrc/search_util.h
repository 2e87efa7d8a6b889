// bitmapperbs_amd/csrc/search_util.h -- what the driver's stages are built from: the thread pool, the hand-over queues between the
// stages, page-locked staging buffers, newline counting, and a few byte-level helpers (bmbs_search.cpp, bmbs_reader_test.cpp)
#pragma once
#include "../../include/bmbs.h"
#if defined(__x86_64__)
#include <emmintrin.h>
#endif
#include <unistd.h>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <ctime>
#include <functional>
#include <map>
#include <mutex>
#include <queue>
#include <string>
#include <thread>
#include <vector>

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

// joins a thread when the scope that started it is left, whichever way
struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } };

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

// all of p[0, n) to file offset off; false: the write failed (errno says why) or made no progress
inline bool pwrite_all(int fd, const char* p, size_t n, size_t off)
{
    size_t done = 0;
    while (done < n) {
        const ssize_t w = pwrite(fd, p + done, n - done, (off_t)(off + done));
        if (w <= 0) return false;
        done += (size_t)w;
    }
    return true;
}

inline void put_uint(std::string& s, unsigned long long v)
{
    char b[24]; int i = 24;
    do { b[--i] = (char)('0' + v % 10); v /= 10; } while (v);
    s.append(b + i, (size_t)(24 - i));
}
inline void put_le32(std::vector<char>& o, uint32_t v) { char b[4] = {(char)v, (char)(v >> 8), (char)(v >> 16), (char)(v >> 24)}; o.insert(o.end(), b, b + 4); }

inline double now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
