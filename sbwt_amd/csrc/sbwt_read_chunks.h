// sbwt_read_chunks.h -- how the chunked host-buffer calls (read hits, colours and pseudoalignment, screen, walks) cut a batch
// of reads into chunks.  Plain C++: no HIP, no C ABI, so the rule is tested on its own (tests/cpp/test_read_chunks.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <new>
#include <vector>

struct SbwtReadChunks {
    enum Bad { NONE = 0, DECREASING, TOO_LONG, NO_MEMORY };     // TOO_LONG: a read of 2^31 bases or more
    std::vector<int64_t> cuts;      // chunk c holds the reads cuts[c] .. cuts[c + 1] - 1
    int64_t max_bases = 0, max_reads = 0, max_windows = 0;      // the largest of any one chunk
    int64_t windows = 0;            // k-mer windows of the whole batch
    Bad bad = NONE;
    int64_t bad_read = -1;          // DECREASING, TOO_LONG: the first read whose length is refused
    int64_t n_chunks() const { return (int64_t)cuts.size() - 1; }
};

// Chunks of whole reads: a chunk ends before read r when it holds a read already and r would take it past `budget` bases or
// `max_chunk_reads` reads, so a chunk always takes at least one read, however long.  Only differences of offsets are used.
// (hidden: an inline function of a header is no part of the library's interface)
__attribute__((visibility("hidden"))) inline SbwtReadChunks sbwt_cut_read_chunks(const int64_t *read_off, int64_t n_reads, int64_t budget, int64_t max_chunk_reads, int64_t k) {
    SbwtReadChunks ch;
    try {
        ch.cuts.push_back(0);
        int64_t chunk_windows = 0;
        for (int64_t lo = 0, r = 0; r < n_reads; r++) {
            const int64_t len = read_off[r + 1] - read_off[r];
            if (len < 0 || len >= ((int64_t)1 << 31)) {
                ch.bad = len < 0 ? SbwtReadChunks::DECREASING : SbwtReadChunks::TOO_LONG;
                ch.bad_read = r;
                return ch;
            }
            if (r > lo && (read_off[r + 1] - read_off[lo] > budget || r - lo >= max_chunk_reads)) {
                ch.cuts.push_back(r);
                lo = r;
                chunk_windows = 0;
            }
            const int64_t w = std::max<int64_t>(0, len - k + 1);
            chunk_windows += w;
            ch.windows += w;
            ch.max_bases = std::max(ch.max_bases, read_off[r + 1] - read_off[lo]);
            ch.max_reads = std::max(ch.max_reads, r + 1 - lo);
            ch.max_windows = std::max(ch.max_windows, chunk_windows);
        }
        ch.cuts.push_back(n_reads);
    } catch (const std::bad_alloc &) {
        ch.bad = SbwtReadChunks::NO_MEMORY;
    }
    return ch;
}
