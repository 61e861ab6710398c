// sbwt_colormerge.h -- colour sets carried onto another index (sbwt_colormerge.hip): what the C-ABI
// host code calls.
#pragma once
#include <hip/hip_runtime.h>
#include "sbwt_device.h"

// one coloured input: its index and its colour-set object's device arrays (ids: ix.n_nodes uint32; table: n_sets x words)
struct SbwtCmSide {
    SbwtIndexView ix;
    const unsigned *d_ids = nullptr;
    const unsigned long long *d_table = nullptr;
    long long n_sets = 1;
    int words = 1;
};

struct SbwtCmInfo {
    long long n_real_u = 0, n_from_a = 0, n_from_b = 0, n_from_both = 0, n_pairs = 0, n_sets = 0;
    double pass_ms[4] = {0, 0, 0, 0};      // keys, locate and gather, pairs and rows, canonical numbering
};

// The canonical colour-set object of index `u` whose real column of k-mer x carries S_a(x) | (S_b(x) shifted up by
// color_offset_b bits), in rows of words_out words; a k-mer that a side lacks has the empty set there (include/sbwtgpu.h,
// "colour sets carried onto another index").  b == nullptr: a alone.  u_is says that u is the index of a (1) or of b (2) and
// b_is_a that both sides have one index: the keys of an index are extracted once.  *d_ids (u.n_nodes uint32, dummy columns 0)
// and *d_table (*n_sets x words_out) are allocated here and belong to the caller; on an error neither is left allocated.
// All three indexes have one k in 2 .. 64 and u fewer than 2^31 columns.
// Scratch, all freed before it returns: per index while its keys are extracted what sbwt_setops_scratch_bytes says (one
// index at a time); 12 (20 for k > 32) bytes per key of each index for keys and columns until the locate pass has run; then
// per key of u 8 (the pair) + 4 (its number) + 13 (sbwt_colorsets_compress on the pairs); per distinct pair 8 + 8 words_out
// + 4 + 13.  Synchronises `stream`.
hipError_t sbwt_colormerge(const SbwtIndexView &u, const SbwtCmSide &a, const SbwtCmSide *b, int u_is, bool b_is_a,
                           int color_offset_b, int words_out, unsigned **d_ids, unsigned long long **d_table, long long *n_sets,
                           SbwtCmInfo *info, hipStream_t stream);
