// sbwt_positions.h -- reference positions per column and read mapping by diagonal voting (sbwt_positions.hip, DESIGN.md
// section 26; include/sbwtgpu.h, "positions").  What the C-ABI host code launches.
#pragma once
#include <hip/hip_runtime.h>

#define SBWT_PM_TABLE 256       // distinct placements a wave keeps in LDS per read (the compiled T)
#define SBWT_POS_NONE (~0ull)   // first[v]: no position

// The counters of a positions object, on the device: the adds add to them with atomics.
struct SbwtPosCounters {
    unsigned long long n_windows;       // windows offered, once per strand searched
    unsigned long long n_hits;          // results >= 0
    unsigned long long bad;             // upload: an entry that is neither SBWT_POS_NONE nor a key with seq < 2^30
    unsigned long long pad[5];
};
static_assert(sizeof(SbwtPosCounters) == 64, "the position counters are eight words");

// the record of a read (sbwtgpu_read_map of include/sbwtgpu.h)
struct SbwtReadMap { long long start; int seq, strand, votes, votes2, n_found, n_anchored; };
static_assert(sizeof(SbwtReadMap) == 32, "a read's map record is 32 bytes");

// The head of the map calls' own part of the workspace, behind the pseudoalignment layout: the length of the list of reads
// whose placements outgrew the LDS table, then the list (4 bytes per read).
struct SbwtPosMapHeader { unsigned n_slow; unsigned pad[63]; };
static_assert(sizeof(SbwtPosMapHeader) == 256, "the map header is 256 bytes");

// One launch per add.  d_res: the W = d_out_off[n_reads] int32 results of the batch, d_res2 (may be NULL): the W results of
// the mirrored batch, window p's at W - 1 - p (max_results bounds W for the grid).  Every result v with 0 <= v < n_nodes
// offers the key ((first_seq + r) << 32) | (pos << 1) | t to d_first[v] (64-bit atomicMin, skipped when the value there is
// smaller already), r and pos found from d_out_off by bisection; ctr->n_windows grows by W (2 W with d_res2), ctr->n_hits by
// the hits, *d_n_hit_windows by the windows with a hit on either strand.
void sbwt_launch_pos_add(const int *d_res, const int *d_res2, const long long *d_out_off, long long n_reads, long long max_results,
                         long long first_seq, long long n_nodes, unsigned long long *d_first, SbwtPosCounters *ctr,
                         unsigned long long *d_n_hit_windows, hipStream_t stream);

// ctr->bad = 1 when an entry of d_first is neither SBWT_POS_NONE nor a key with seq < 2^30
void sbwt_launch_pos_check(const unsigned long long *d_first, long long n_nodes, SbwtPosCounters *ctr, hipStream_t stream);

// *d_out = the entries of d_first that hold a position
void sbwt_launch_pos_count(const unsigned long long *d_first, long long n_nodes, unsigned long long *d_out, hipStream_t stream);

// One record per read from the int32 results, d_first and d_out_off; d_res2 (may be NULL) as above.  Two launches: one wave per
// read with a table of `cap` (1 .. SBWT_PM_TABLE) placements in LDS, which appends the reads that outgrow it to d_slow, and a
// grid-stride kernel over that list which recomputes them exactly.  hdr is zeroed here first.
void sbwt_launch_pos_map(const int *d_res, const int *d_res2, const long long *d_out_off, long long n_reads,
                         const unsigned long long *d_first, long long n_nodes, int cap, SbwtReadMap *d_out, SbwtPosMapHeader *hdr,
                         unsigned *d_slow, hipStream_t stream);
