// sbwt_colors.h -- the colour matrix of an index and pseudoalignment over it (sbwt_colors.hip): what the C-ABI host code launches.
#pragma once
#include <hip/hip_runtime.h>
#include "sbwt_device.h"

// the record of a read (sbwtgpu_pseudoalignment of include/sbwtgpu.h)
struct SbwtPseudoalignment { unsigned long long colors; int n_kmers, n_found; };
static_assert(sizeof(SbwtPseudoalignment) == 16, "a read's record is 16 bytes");
// the record of a read over a wide matrix (sbwtgpu_read_found): its colours are `words` words of their own
struct SbwtReadFound { int n_kmers, n_found; };
static_assert(sizeof(SbwtReadFound) == 8, "a read's wide record is 8 bytes");

// Where the parts of a pseudoalignment (and colouring) workspace lie, in bytes from its start (every part 256-byte aligned).
// The search workspace comes first, so the search's status word is where sbwtgpu_workspace_status looks for it.
struct SbwtPaLayout {
    long long hdr;      // SbwtPaHeader
    long long res;      // int32 search results of the forward batch: 4 bytes per base
    long long cnt;      // windows per read (n_reads entries)
    long long ooff;     // their exclusive scan (n_reads + 1)
    long long bsum;     // the scan's block sums
    long long res2;     // two strands: the int32 results of the mirrored batch ...
    long long rc;       // ... the reverse complement of the whole base buffer ...
    long long roff2;    // ... the mirrored read offsets ...
    long long ooff2;    // ... and the mirrored result offsets
    long long total;
};
struct SbwtPaHeader {
    int status;                         // the first non-zero status word of this call's searches (SbwtWorkHeader::status)
    int pad0;
    unsigned long long n_hit;           // colouring: windows with a hit on either strand
    int pad[60];
};
static_assert(sizeof(SbwtPaHeader) == 256, "pseudoalignment header is 256 bytes");

SbwtPaLayout sbwt_pa_layout(long long search_ws_bytes, long long total_bases, long long n_reads, int strands);

// hdr->status = the search's status word unless an earlier search of the call left one (one thread, after each search)
void sbwt_launch_pa_note_status(const SbwtWorkHeader *search_ws, SbwtPaHeader *hdr, hipStream_t stream);

// The matrix: n_nodes x words 64-bit words, row-major; colour c is bit c & 63 of word c >> 6 (words = 1: one word per column).
// Bit `color` of row res[i] is set for every result res[i] >= 0 of the W = d_out_off[n_reads] results (max_results bounds W for
// the grid).  count != 0: hdr->n_hit += the number of i with res[i] >= 0 or, when d_other is given, other[W - 1 - i] >= 0 (the
// mirrored batch's result of the same window).
void sbwt_launch_col_mark(const int *d_res, const int *d_other, const long long *d_out_off, long long n_reads, long long max_results,
                          unsigned long long *d_rows, long long n_nodes, int words, int color, int count, SbwtPaHeader *hdr,
                          hipStream_t stream);

// d_stats[c] = rows with bit c set (c < 64 words), d_stats[64 words] = rows that are not 0 in some word; the caller zeroes the
// 64 words + 1 entries first
void sbwt_launch_col_stats(const unsigned long long *d_rows, long long n_nodes, int words, unsigned long long *d_stats,
                           hipStream_t stream);

// An uploaded matrix (of ceil(n_colors / 64) words per row) made to obey the definition: bits >= n_colors and the rows of dummy columns (k-1 rounds down the dummy tree
// from the root: sbwt_colwalk.h) are cleared.  Scratch of one byte per column, freed before it returns; synchronises `stream`.
hipError_t sbwt_colors_clean(const SbwtIndexView &ix, unsigned long long *d_rows, int n_colors, hipStream_t stream);

// One record per read from the int32 results, the rows and d_out_off; d_res2 (may be NULL): the mirrored batch's results, window
// p's at W - 1 - p.  d_counts (may be NULL): n_reads x n_colors int32.
void sbwt_launch_pa_reduce(const int *d_res, const int *d_res2, const long long *d_out_off, long long n_reads,
                           const unsigned long long *d_rows, long long n_nodes, int n_colors, int threshold_ppm, int denominator,
                           SbwtPseudoalignment *d_out, int *d_counts, hipStream_t stream);

// The same over rows of `words` words: d_out[r] = {n_kmers, n_found}, d_colors: n_reads x words, d_counts (may be NULL): n_reads x
// n_colors int32.  Dynamic LDS: 4 waves x (words - 1) x 64 int32 (none for words = 1, 63 KiB for 64).
void sbwt_launch_pa_reduce_wide(const int *d_res, const int *d_res2, const long long *d_out_off, long long n_reads,
                                const unsigned long long *d_rows, long long n_nodes, int words, int n_colors, int threshold_ppm,
                                int denominator, SbwtReadFound *d_out, unsigned long long *d_colors, int *d_counts, hipStream_t stream);
