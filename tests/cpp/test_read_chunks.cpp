// The chunk rule of the chunked host-buffer calls (sbwt_amd/csrc/sbwt_read_chunks.h) against a literal restatement of the loop
// that read hits, colours, screen and walks each carried before they shared it, and against a brute-force recount.
// No GPU, no library: g++ -std=c++17 -O1 -fsanitize=address,undefined tests/cpp/test_read_chunks.cpp && ./a.out
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../sbwt_amd/csrc/sbwt_read_chunks.h"

static int n_cases = 0;
#define CHECK(cond)                                                                                            \
    do {                                                                                                       \
        if (!(cond)) {                                                                                         \
            fprintf(stderr, "%s:%d: case %d: CHECK(%s) failed\n", __FILE__, __LINE__, n_cases, #cond);         \
            exit(1);                                                                                           \
        }                                                                                                      \
    } while (0)

// the loop as the four entry points had it (the walks' copy: it is the one that counts windows), offsets known to be good
struct Old {
    std::vector<int64_t> cuts{0};
    int64_t max_bases = 0, max_reads = 0, max_windows = 0;
};
static Old old_loop(const int64_t *read_off, int64_t n_reads, int64_t budget, int64_t CH_READS, int64_t k) {
    Old o;
    int64_t windows = 0;
    for (int64_t lo = 0, r = 0; r < n_reads; r++) {
        if (r > lo && (read_off[r + 1] - read_off[lo] > budget || r - lo >= CH_READS)) {
            o.cuts.push_back(r);
            lo = r;
            windows = 0;
        }
        windows += std::max<int64_t>(0, read_off[r + 1] - read_off[r] - k + 1);
        o.max_bases = std::max(o.max_bases, read_off[r + 1] - read_off[lo]);
        o.max_reads = std::max(o.max_reads, r + 1 - lo);
        o.max_windows = std::max(o.max_windows, windows);
    }
    o.cuts.push_back(n_reads);
    return o;
}

static void check_case(const std::vector<int64_t> &off, int64_t budget, int64_t cap, int64_t k) {
    n_cases++;
    const int64_t n = (int64_t)off.size() - 1;
    const SbwtReadChunks ch = sbwt_cut_read_chunks(off.data(), n, budget, cap, k);
    CHECK(ch.bad == SbwtReadChunks::NONE && ch.bad_read == -1);
    const Old o = old_loop(off.data(), n, budget, cap, k);
    CHECK(ch.cuts == o.cuts);
    CHECK(ch.max_bases == o.max_bases && ch.max_reads == o.max_reads && ch.max_windows == o.max_windows);
    // a partition of [0, n) into chunks of at least one read; only a chunk of one read may exceed a limit
    CHECK(ch.n_chunks() >= 1 && ch.cuts.front() == 0 && ch.cuts.back() == n);
    int64_t mb = 0, mr = 0, mw = 0, total = 0;
    for (int64_t c = 0; c < ch.n_chunks(); c++) {
        const int64_t lo = ch.cuts[(size_t)c], hi = ch.cuts[(size_t)c + 1];
        CHECK(hi > lo);
        if (hi - lo > 1) CHECK(off[(size_t)hi] - off[(size_t)lo] <= budget && hi - lo <= cap);
        // (greedy: the next read would not have fitted)
        if (hi < n) CHECK(off[(size_t)hi + 1] - off[(size_t)lo] > budget || hi - lo >= cap);
        int64_t w = 0;
        for (int64_t r = lo; r < hi; r++) w += std::max<int64_t>(0, off[(size_t)r + 1] - off[(size_t)r] - k + 1);
        mb = std::max(mb, off[(size_t)hi] - off[(size_t)lo]);
        mr = std::max(mr, hi - lo);
        mw = std::max(mw, w);
        total += w;
    }
    CHECK(ch.max_bases == mb && ch.max_reads == mr && ch.max_windows == mw && ch.windows == total);
}

int main() {
    std::mt19937_64 rng(20240607);
    for (const int64_t n : {1, 2, 3, 1000})
        for (const int64_t first : {(int64_t)0, (int64_t)12345}) {                 // offsets that do not start at 0
            std::vector<int64_t> off{first};
            for (int64_t r = 0; r < n; r++) off.push_back(off.back() + (rng() % 5 == 0 ? 0 : (int64_t)(rng() % 401)));
            if (n >= 2) {                                                           // one read longer than every small budget
                const int64_t grow = 500 - (off[2] - off[1]);
                for (size_t t = 2; t < off.size(); t++) off[t] += grow;
            }
            const int64_t total = off.back() - off.front();
            for (const int64_t budget : {(int64_t)1, (int64_t)40, total, total + 1})
                for (const int64_t cap : {(int64_t)1, (int64_t)2, (int64_t)1 << 24})
                    for (const int64_t k : {1, 31}) check_case(off, budget, cap, k);
        }
    {   // no read at all: one empty chunk table entry, nothing counted (the entry points return before they cut)
        const int64_t off0[1] = {7};
        const SbwtReadChunks ch = sbwt_cut_read_chunks(off0, 0, 40, 2, 31);
        CHECK(ch.bad == SbwtReadChunks::NONE && ch.cuts == std::vector<int64_t>({0, 0}) && ch.max_reads == 0 && ch.windows == 0);
    }
    {   // refused lengths: the first bad read and its kind, whatever comes after it
        const int64_t dec[] = {5, 10, 30, 29, 40, 35};
        SbwtReadChunks ch = sbwt_cut_read_chunks(dec, 5, 40, 2, 31);
        CHECK(ch.bad == SbwtReadChunks::DECREASING && ch.bad_read == 2);
        const int64_t two31 = (int64_t)1 << 31;
        const int64_t lng[] = {3, 3 + two31 - 1, 3 + two31 - 1 + two31, 3 + 3 * two31};
        ch = sbwt_cut_read_chunks(lng, 3, 40, 2, 31);
        CHECK(ch.bad == SbwtReadChunks::TOO_LONG && ch.bad_read == 1);
        ch = sbwt_cut_read_chunks(lng, 1, 40, 2, 31);                               // 2^31 - 1 bases: the longest read there is
        CHECK(ch.bad == SbwtReadChunks::NONE && ch.max_bases == two31 - 1 && ch.windows == two31 - 31);
        const int64_t mixed[] = {0, two31, two31 - 1};                              // too long first, decreasing second
        ch = sbwt_cut_read_chunks(mixed, 2, 40, 2, 31);
        CHECK(ch.bad == SbwtReadChunks::TOO_LONG && ch.bad_read == 0);
    }
    printf("read chunks: %d cases ok\n", n_cases);
    return 0;
}
