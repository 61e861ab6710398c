// sbwt_setops.h -- set operations on two indexes (sbwt_setops.hip): what the C-ABI host code launches.
#pragma once
#include <hip/hip_runtime.h>
#include "sbwt_device.h"

// scratch per column while sbwt_setops_keys works (freed before it returns): 4 (pred) + 1 (dummy level) + 2 x 16 (window +
// pointer, double-buffered; the compaction's scans reuse the free half) bytes for k <= 32, 2 x 32 for 32 < k <= 64
long long sbwt_setops_scratch_bytes(long long n_nodes, int k);

// The keys of the real columns of an index, in column order = ascending key order, no duplicates: the builder's format
// (sbwt_build.hip: char i of the k-mer at bits 2i; 8 bytes each for k <= 32, 16 for 32 < k <= 64).  *d_keys is a device
// allocation of its own that the caller frees (never null on success).  Synchronises `stream`.  On failure nothing is left
// allocated.  With d_cols: *d_cols is a second allocation of the caller's, the column of every key (4 bytes each).
hipError_t sbwt_setops_keys(const SbwtIndexView &ix, void **d_keys, long long *n_keys, hipStream_t stream,
                            unsigned **d_cols = nullptr);

struct SbwtSetopCounts {
    long long n_a = 0, n_b = 0, n_both = 0, n_either = 0, n_result = 0;
};
// Two sorted duplicate-free key lists (they may be the same array) -> the counts, and with d_out != nullptr the sorted
// duplicate-free list of the operation (SBWTGPU_SETOP_*: 0 union, 1 intersection, 2 a minus b, 3 symmetric difference) as a
// device allocation of its own (never null on success).  d_out == nullptr: counts only, nothing is compacted (n_result = 0).
hipError_t sbwt_setops_merge(const void *d_a, long long n_a, const void *d_b, long long n_b, int key_bytes, int op,
                             void **d_out, SbwtSetopCounts *counts, hipStream_t stream);
