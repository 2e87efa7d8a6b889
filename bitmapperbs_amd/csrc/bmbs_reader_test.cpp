// bitmapperbs_amd/csrc/bmbs_reader_test.cpp -- the driver's FASTQ reader on its own (no GPU)
#include "search_source.h"

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
