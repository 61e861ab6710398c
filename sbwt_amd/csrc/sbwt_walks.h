// sbwt_walks.h -- reads threaded through the unitig graph (sbwt_walks.hip): what the C-ABI host
// code launches.
#pragma once
#include <hip/hip_runtime.h>
#include "sbwt_device.h"

// the record of a step (sbwtgpu_walk_step of include/sbwtgpu.h)
struct SbwtWalkStep { unsigned unitig, offset; int read_pos, n_kmers; };
static_assert(sizeof(SbwtWalkStep) == 16, "a step's record is 16 bytes");

// Where the parts of a walks workspace lie, in bytes from its start (every part 256-byte aligned).  The search workspace
// comes first, so the search's status word is where sbwtgpu_workspace_status looks for it.
struct SbwtWalkLayout {
    long long res;      // int32 search results, one per base
    long long cnt;      // windows per read (n_reads entries)
    long long ooff;     // their exclusive scan (n_reads + 1)
    long long bsum;     // that scan's block sums
    long long rbits;    // R: one bit per window, set at the first window of every read (n_words words, below)
    long long sbits;    // S: step starts
    long long tbits;    // T: step ends
    long long wcnt;     // popcount of every S word (int64, the scan's input)
    long long wpre;     // their exclusive scan (n_words + 1)
    long long wsum;     // the block sums of either scan
    long long rcnt;     // popcount of every R word ...
    long long rpre;     // ... and their exclusive scan (n_words + 1): rank over the read starts
    long long rstart;   // the first window of every read that has one, in order (n_reads entries at most)
    long long n_words;  // total_bases / 64 + 2: bit W = out_off[n_reads] itself has a word, so rank(W) needs no special case
    long long total;
};
SbwtWalkLayout sbwt_walk_layout(long long search_ws_bytes, long long total_bases, long long n_reads);

// start[v >> 6] bit (v & 63) = (col_offset[v] == 0) for the n_nodes columns; d_start has (n_nodes + 63) / 64 words
void sbwt_launch_walk_startbits(const unsigned *d_col_offset, long long n_nodes, unsigned long long *d_start, hipStream_t stream);
// Everything after the search: R from out_off, the flags S and T from the results, step_off[0 .. n_reads] by rank over S, the
// records (those of number < steps_cap) and, with d_cov, the sum of n_kmers per unitig added onto d_cov.  total_bases
// is what L was laid out for: its n_words bound W = d_out_off[n_reads] for the grids (W = 0: d_res is not read).  Never
// synchronises.  hipSuccess; the error of clearing R, after which nothing is launched; or hipGetLastError() after the launches.
hipError_t sbwt_launch_walks(const int *d_res, const long long *d_out_off, long long n_reads, long long total_bases,
                       const unsigned long long *d_start, const unsigned *d_col_unitig, const unsigned *d_col_offset, long long n_nodes,
                       char *d_ws, const SbwtWalkLayout &L, long long *d_step_off, SbwtWalkStep *d_steps, long long steps_cap,
                       long long *d_cov, hipStream_t stream);
