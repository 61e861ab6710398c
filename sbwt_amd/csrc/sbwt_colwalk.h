// sbwt_colwalk.h -- the two kernels that let a pass walk the columns of an index BACKWARDS from the blocks and C alone: the
// predecessor array, and the real/dummy level of every column.  Shared by the unitig pass (sbwt_unitigs.hip, DESIGN.md
// section 10) and the label extraction of the set operations (sbwt_setops.hip, section 11).  `static`: every translation
// unit that includes this gets its own copy, like the scans of sbwt_scan.h.
#pragma once
#include "sbwt_kernels_common.h"

__device__ __forceinline__ int ut_last_char(const SbwtIndexView &ix, i64 v) {
    return (v >= ix.C[1]) + (v >= ix.C[2]) + (v >= ix.C[3]);
}
__device__ __forceinline__ unsigned char ut_level(int depth) { return (unsigned char)(depth % 254 + 1); }

// pred[C[c] + rank_c(u)] = u: the one column an edge enters column w from (every column but the root has exactly one)
template <bool MEGA>
static __global__ void __launch_bounds__(256) k_ut_pred(SbwtIndexView ix, unsigned *__restrict__ pred) {
    const i64 u = (i64)blockIdx.x * 256 + threadIdx.x;
    if (u >= ix.n_nodes) return;
    if (u == 0) pred[0] = 0;                                 // nothing enters the root
    const uint4 *blk = ix.blocks + ((u >> 6) << 2);
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint4 q = blk[c];
        if ((quad_bits(q) >> (u & 63)) & 1ull) pred[quad_rank<MEGA>(ix, q, u, c)] = (unsigned)u;
    }
}

// round r: the dummies of depth r hand level r + 1 to their children; after k-1 rounds from the root a column with level 0
// is real.  A level is stored modulo 254, which a child's one depth makes unambiguous: a column that a later round takes for
// its own again only repeats the stores it made before.
template <bool MEGA>
static __global__ void __launch_bounds__(256) k_ut_level(SbwtIndexView ix, unsigned char *__restrict__ lev, int r) {
    const i64 u = (i64)blockIdx.x * 256 + threadIdx.x;
    if (u >= ix.n_nodes) return;
    if (r == 0 && u == 0) lev[0] = ut_level(0);
    if (u == 0 ? r % 254 != 0 : lev[u] != ut_level(r)) return;
    const unsigned char next = ut_level(r + 1);
    const uint4 *blk = ix.blocks + ((u >> 6) << 2);
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint4 q = blk[c];
        if ((quad_bits(q) >> (u & 63)) & 1ull) lev[quad_rank<MEGA>(ix, q, u, c)] = next;
    }
}
