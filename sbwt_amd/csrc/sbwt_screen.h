// sbwt_screen.h -- screening a read set against the references: per-colour k-mer containment (sbwt_screen.hip, DESIGN.md
// section 23; include/sbwtgpu.h, "screen").  What the C-ABI host code launches.
#pragma once
#include <hip/hip_runtime.h>

// The counters of a screen object, on the device: every add adds to them with atomics, nothing else writes them.
struct SbwtScreenCounters {
    unsigned long long n_windows;       // the sample's size, misses counted (two strands: twice the windows)
    unsigned long long n_hits;          // results >= 0
    unsigned long long pad[6];
};
static_assert(sizeof(SbwtScreenCounters) == 64, "the screen counters are eight words");

// One launch per add.  d_res: the W = d_out_off[n_reads] int32 results of the batch, d_res2 (may be NULL): the W results of
// the mirrored batch (max_results bounds W for the grid).  Every result v with 0 <= v < n_nodes is a hit: bit v of d_seen is
// set, d_set_hits[ids[v]] and ctr->n_hits grow by one; ctr->n_windows grows by W (2 W with d_res2).  An id >= n_sets (never:
// ids stay below n_sets) counts as a hit of no set.
void sbwt_launch_screen_add(const int *d_res, const int *d_res2, const long long *d_out_off, long long n_reads, long long max_results,
                            const unsigned *d_ids, long long n_nodes, long long n_sets, unsigned long long *d_seen,
                            unsigned long long *d_set_hits, SbwtScreenCounters *ctr, hipStream_t stream);

// d_set_kmers[t] = the columns whose id is t, d_set_seen[t] = those of them whose bit of d_seen is set (n_sets int64 each,
// zeroed here first): sbwt_launch_gm_sizes' histogram and the same weighted by a bit, in one pass over ids and the bitmap.
void sbwt_launch_screen_sets(const unsigned *d_ids, long long n_nodes, long long n_sets, const unsigned long long *d_seen,
                             unsigned long long *d_set_kmers, unsigned long long *d_set_seen, hipStream_t stream);

// *d_out = the set bits of the n_words words of d_seen
void sbwt_launch_screen_popcount(const unsigned long long *d_seen, long long n_words, unsigned long long *d_out, hipStream_t stream);

// d_ref[x * n_colors + c] = the sum of d_vec[x][t] over the sets t >= 1 whose table row holds colour c, for the three
// per-set int64 vectors d_vec0 .. d_vec2 (3 * n_colors int64, zeroed here first).  One pass over the table.
void sbwt_launch_screen_expand(const unsigned long long *d_table, long long n_sets, int words, int n_colors,
                               const unsigned long long *d_vec0, const unsigned long long *d_vec1, const unsigned long long *d_vec2,
                               unsigned long long *d_ref, hipStream_t stream);
