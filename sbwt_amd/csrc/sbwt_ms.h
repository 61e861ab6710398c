// sbwt_ms.h -- matching statistics and the LCS array (sbwt_ms.hip): what the C-ABI host code launches.
#pragma once
#include <hip/hip_runtime.h>
#include "sbwt_device.h"

// The matching-statistics workspace: counters of the last launch on it (cleared by the caller before each call).
struct SbwtMsWork {
    unsigned long long n_walk;      // bases walked, the k-1 warm-up bases in front of every chunk that starts inside a read included
    unsigned long long n_contract;  // contractions (d == k -> k-1, and every failed extension with d > 0)
    unsigned long long n_recompute; // contractions whose widening passed the scan bound: the interval was recomputed by LF steps
    unsigned long long n_full;      // positions answered with len == k
    unsigned long long n_out;       // positions answered
    unsigned long long pad[27];
};
static_assert(sizeof(SbwtMsWork) == 256, "matching-statistics workspace is 256 bytes");

// scratch of the LCS build: pred[] of 4 bytes per column (8 past 2^32 columns)
long long sbwt_lcs_scratch_bytes(long long n_nodes);
// d_lcs: n_nodes + 1 bytes (lcs[n_nodes] = 0 is written too) in an allocation rounded up to 64 bytes
void sbwt_launch_build_lcs(const SbwtIndexView &ix, void *d_scratch, unsigned char *d_lcs, hipStream_t stream);
// output slot of base i = i (d_bases, d_len, d_first, d_second are indexed alike); d_first == d_second == nullptr: lengths only
void sbwt_launch_ms(const SbwtIndexView &ix, const unsigned char *d_lcs, const char *d_bases, long long total_bases,
                    const long long *d_read_off, long long n_reads, unsigned char *d_len, long long *d_first,
                    long long *d_second, SbwtMsWork *ws, hipStream_t stream);
long long sbwt_ms_chunk(long long total_bases, int k);
