// sbwt_screen.hip -- screening a read set against the references (include/sbwtgpu.h, "screen"): an
// accumulator that lives across batches -- one `seen` bit per column, one hit counter per colour set, two scalars -- and the
// passes that turn it into per-set and per-colour vectors.  Everything is an integer sum, so no result depends on the order
// in which lanes, waves, batches or host threads arrive.
//
//   k_sc_add     the search's int32 results (and the mirrored batch's) -> the accumulator, one launch per add.  A wave takes
//                SC_SPAN consecutive results at a stretch, 64 per iteration.  Per hit two gathers: the word of `seen` (a plain
//                load, the atomic OR only when the bit is clear: after a sample's first batches most bits are set) and
//                ids[col].  A read follows a path, so consecutive windows mostly carry one id: the wave keeps a pending
//                (id, count) run, peels the iteration's distinct ids as k_pa_reduce_sets peels keys (readlane, ballot,
//                popcount) and issues one add per run, not per hit; after SC_PEEL distinct ids the lanes left over add 1
//                each, so an iteration of 64 different ids costs no more trips than that.  Adds to ids below SC_LDS_IDS meet
//                in the block's LDS and reach memory once per block -- 10^9 hits on an index of 8 sets would otherwise all
//                meet at 8 addresses in L2 -- and the others are 64-bit atomics on set_hits directly.
//   k_sc_sets    ids + seen -> set_kmers[t], set_seen[t]: k_gm_sizes' histogram and the same weighted by the column's bit, in
//                one streaming pass (a sibling of that kernel, which is left as it is: it writes uint32 and takes no mask).
//   k_sc_expand  table + three per-set vectors -> three per-colour vectors: a bit matrix times vector product.  A wave keeps
//                one word of colours (lane l: colour 64 w + l) and walks the sets 64 at a time: lane i loads set i's word
//                and its three values, the non-zero words are broadcast one by one (readlane) and the lanes of their set
//                bits add.  64-bit integer adds; the block's four waves meet in LDS, then one atomic per colour and vector.
#include "sbwt_kernels_common.h"
#include "sbwt_screen.h"

#define SC_LDS_IDS 1024
#define SC_SPAN 2048            // results a wave takes at a stretch (a run is flushed at its end at the latest)
#define SC_PEEL 4               // distinct ids of an iteration that are counted by ballot before the rest adds lane by lane

__device__ __forceinline__ u64 sc_readlane64(u64 v, int src) {
    return (u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src) |
           ((u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src) << 32);
}

// ---------------------------------------------------------------------------------------------
// results -> accumulator
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void sc_flush(unsigned *lds_hits, u64 *set_hits, unsigned id, unsigned n, int lane) {
    if (lane == 0 && n) {
        if (id < SC_LDS_IDS) atomicAdd(lds_hits + id, n);
        else atomicAdd(set_hits + id, (u64)n);
    }
}

__global__ void __launch_bounds__(256) k_sc_add(const int *__restrict__ res, const int *__restrict__ res2,
                                                const i64 *__restrict__ out_off, i64 n_reads, const unsigned *__restrict__ ids,
                                                i64 n_nodes, unsigned n_sets, u64 *seen, u64 *set_hits, SbwtScreenCounters *ctr) {
    __shared__ unsigned lds_hits[SC_LDS_IDS];
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < SC_LDS_IDS; i += 256) lds_hits[i] = 0;
    __syncthreads();
    const i64 W = out_off[n_reads];
    const i64 total = res2 ? 2 * W : W;                    // the mirrored batch's results follow the forward ones
    if (blockIdx.x == 0 && threadIdx.x == 0 && total > 0) atomicAdd(&ctr->n_windows, (u64)total);
    const i64 n_spans = (total + SC_SPAN - 1) / SC_SPAN;
    u64 hits = 0;                                          // of this lane's wave (the same in every lane)
    unsigned pend_id = 0, pend_n = 0;                      // the pending run, the same in every lane; nothing pending: pend_n = 0
    for (i64 g = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); g < n_spans; g += (i64)gridDim.x * 4) {
        const i64 base = g * SC_SPAN;
        for (int it = 0; it < SC_SPAN / 64 && base + it * 64 < total; it++) {
            const i64 i = base + it * 64 + lane;
            i64 v = -1;
            if (i < total) v = i < W ? res[i] : res2[i - W];
            const bool hit = v >= 0 && v < n_nodes;
            unsigned id = 0;
            bool counted = false;
            if (hit) {
                const u64 bit = 1ull << (v & 63);
                u64 *word = seen + (v >> 6);
                if (!(*word & bit)) atomicOr(word, bit);
                id = ids[v];
                counted = id < n_sets;                     // (always: ids stay below n_sets)
            }
            hits += (u64)__popcll(__ballot(hit));
            u64 live = __ballot(counted);
            for (int round = 0; round < SC_PEEL && live; round++) {
                const int src = __ffsll((i64)live) - 1;
                const unsigned k0 = (unsigned)__builtin_amdgcn_readlane((int)id, src);
                const u64 eq = __ballot(counted && id == k0);
                live &= ~eq;
                const unsigned c = (unsigned)__popcll(eq);
                if (pend_n != 0 && k0 == pend_id) {
                    pend_n += c;
                } else {
                    sc_flush(lds_hits, set_hits, pend_id, pend_n, lane);
                    pend_id = k0;
                    pend_n = c;
                }
            }
            if ((live >> lane) & 1ull) {
                if (id < SC_LDS_IDS) atomicAdd(lds_hits + id, 1u);
                else atomicAdd(set_hits + id, 1ull);
            }
        }
    }
    sc_flush(lds_hits, set_hits, pend_id, pend_n, lane);
    if (lane == 0 && hits) atomicAdd(&ctr->n_hits, hits);
    __syncthreads();
    for (unsigned i = threadIdx.x; i < SC_LDS_IDS && i < n_sets; i += 256) {
        const unsigned c = lds_hits[i];
        if (c) atomicAdd(set_hits + i, (u64)c);
    }
}

void sbwt_launch_screen_add(const int *d_res, const int *d_res2, const long long *d_out_off, long long n_reads, long long max_results,
                            const unsigned *d_ids, long long n_nodes, long long n_sets, unsigned long long *d_seen,
                            unsigned long long *d_set_hits, SbwtScreenCounters *ctr, hipStream_t stream) {
    // a block's four waves take 4 x SC_SPAN results per round; a block's 32-bit LDS counters hold what it sees (the cap leaves
    // a block of the largest batch, 2 x 2^36 results, 2^26 of them)
    const i64 total = d_res2 ? 2 * max_results : max_results;
    const i64 gb = (total + 4 * SC_SPAN - 1) / (4 * SC_SPAN);
    const dim3 grid((unsigned)(gb < 1 ? 1 : gb > 2048 ? 2048 : gb)), block(256);
    hipLaunchKernelGGL(k_sc_add, grid, block, 0, stream, d_res, d_res2, d_out_off, (i64)n_reads, d_ids, (i64)n_nodes, (unsigned)n_sets,
                       (u64 *)d_seen, (u64 *)d_set_hits, ctr);
}

// ---------------------------------------------------------------------------------------------
// ids + seen -> per-set k-mers and seen k-mers
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_sc_sets(const unsigned *__restrict__ ids, i64 n, unsigned n_sets, const u64 *__restrict__ seen,
                                                 u64 *__restrict__ set_kmers, u64 *__restrict__ set_seen) {
    __shared__ unsigned lds_cnt[SC_LDS_IDS], lds_seen[SC_LDS_IDS];
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < SC_LDS_IDS; i += 256) lds_cnt[i] = lds_seen[i] = 0;
    __syncthreads();
    // (whole waves go round together: the bound is rounded up to the wave, and a lane past n sits the ballots out)
    for (i64 j0 = (i64)blockIdx.x * 256 + (threadIdx.x & ~63u); j0 < n; j0 += (i64)gridDim.x * 256) {
        const i64 j = j0 + lane;
        bool on = j < n;
        const unsigned id = on ? ids[j] : 0;
        if (id >= n_sets) on = false;                      // (never: ids stay below n_sets)
        const u64 sw = seen[j0 >> 6];                      // the wave's 64 columns are one word of the bitmap (j0 < n: it exists)
        u64 live = __ballot(on);
        for (int round = 0; round < 2 && live; round++) {
            const int src = __ffsll((i64)live) - 1;
            const unsigned k0 = (unsigned)__builtin_amdgcn_readlane((int)id, src);
            const u64 eq = __ballot(on && id == k0);
            live &= ~eq;
            if (lane == 0) {
                const unsigned c = (unsigned)__popcll(eq), s = (unsigned)__popcll(eq & sw);
                if (k0 < SC_LDS_IDS) {
                    atomicAdd(lds_cnt + k0, c);
                    if (s) atomicAdd(lds_seen + k0, s);
                } else {
                    atomicAdd(set_kmers + k0, (u64)c);
                    if (s) atomicAdd(set_seen + k0, (u64)s);
                }
            }
        }
        if ((live >> lane) & 1ull) {
            const bool s = (sw >> lane) & 1ull;
            if (id < SC_LDS_IDS) {
                atomicAdd(lds_cnt + id, 1u);
                if (s) atomicAdd(lds_seen + id, 1u);
            } else {
                atomicAdd(set_kmers + id, 1ull);
                if (s) atomicAdd(set_seen + id, 1ull);
            }
        }
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < SC_LDS_IDS && i < n_sets; i += 256) {
        const unsigned c = lds_cnt[i], s = lds_seen[i];
        if (c) atomicAdd(set_kmers + i, (u64)c);
        if (s) atomicAdd(set_seen + i, (u64)s);
    }
}

void sbwt_launch_screen_sets(const unsigned *d_ids, long long n_nodes, long long n_sets, const unsigned long long *d_seen,
                             unsigned long long *d_set_kmers, unsigned long long *d_set_seen, hipStream_t stream) {
    (void)hipMemsetAsync(d_set_kmers, 0, (size_t)n_sets * 8, stream);
    (void)hipMemsetAsync(d_set_seen, 0, (size_t)n_sets * 8, stream);
    const i64 g = (n_nodes + 255) / 256;
    hipLaunchKernelGGL(k_sc_sets, dim3((unsigned)(g < 1 ? 1 : g > 2048 ? 2048 : g)), dim3(256), 0, stream, d_ids, (i64)n_nodes,
                       (unsigned)n_sets, (const u64 *)d_seen, (u64 *)d_set_kmers, (u64 *)d_set_seen);
}

// *out += the set bits of the bitmap (the caller zeroes it first)
__global__ void __launch_bounds__(256) k_sc_popcount(const u64 *__restrict__ seen, i64 n_words, u64 *__restrict__ out) {
    u64 mine = 0;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (i64)gridDim.x * 256) mine += (u64)__popcll(seen[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(out, mine);
}

void sbwt_launch_screen_popcount(const unsigned long long *d_seen, long long n_words, unsigned long long *d_out, hipStream_t stream) {
    (void)hipMemsetAsync(d_out, 0, 8, stream);
    const i64 g = (n_words + 255) / 256;
    hipLaunchKernelGGL(k_sc_popcount, dim3((unsigned)(g < 1 ? 1 : g > 1024 ? 1024 : g)), dim3(256), 0, stream, (const u64 *)d_seen,
                       (i64)n_words, (u64 *)d_out);
}

// ---------------------------------------------------------------------------------------------
// per-set vectors -> per-colour vectors
// ---------------------------------------------------------------------------------------------
// grid: x slices the sets, y = the word of colours
__global__ void __launch_bounds__(256) k_sc_expand(const u64 *__restrict__ table, i64 n_sets, int words, int n_colors,
                                                   const u64 *__restrict__ vec0, const u64 *__restrict__ vec1,
                                                   const u64 *__restrict__ vec2, u64 *__restrict__ ref) {
    __shared__ u64 part[3][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w = blockIdx.y;
    u64 a0 = 0, a1 = 0, a2 = 0;                            // lane l: colour 64 w + l
    for (i64 t0 = ((i64)blockIdx.x * 4 + wave) * 64; t0 < n_sets; t0 += (i64)gridDim.x * 256) {
        const i64 t = t0 + lane;
        u64 word = 0, x0 = 0, x1 = 0, x2 = 0;
        if (t >= 1 && t < n_sets) {                        // (set 0 is the empty set whatever its row says)
            word = table[t * words + w];
            if (word) { x0 = vec0[t]; x1 = vec1[t]; x2 = vec2[t]; }
        }
        u64 left = __ballot(word != 0);
        while (left) {                                     // one trip per set of the 64 that holds a colour of this word
            const int src = __ffsll((i64)left) - 1;
            left &= left - 1;
            const u64 bits = sc_readlane64(word, src);
            const u64 y0 = sc_readlane64(x0, src), y1 = sc_readlane64(x1, src), y2 = sc_readlane64(x2, src);
            if ((bits >> lane) & 1ull) { a0 += y0; a1 += y1; a2 += y2; }
        }
    }
    part[0][wave][lane] = a0;
    part[1][wave][lane] = a1;
    part[2][wave][lane] = a2;
    __syncthreads();
    if (threadIdx.x < 192) {
        const int x = threadIdx.x >> 6;                    // wave x adds up vector x
        const u64 s = part[x][0][lane] + part[x][1][lane] + part[x][2][lane] + part[x][3][lane];
        const int c = w * 64 + lane;
        if (c < n_colors && s) atomicAdd(ref + (i64)x * n_colors + c, s);
    }
}

void sbwt_launch_screen_expand(const unsigned long long *d_table, long long n_sets, int words, int n_colors,
                               const unsigned long long *d_vec0, const unsigned long long *d_vec1, const unsigned long long *d_vec2,
                               unsigned long long *d_ref, hipStream_t stream) {
    (void)hipMemsetAsync(d_ref, 0, (size_t)3 * (size_t)n_colors * 8, stream);
    const i64 need = (n_sets + 255) / 256, cap = 1024 / words < 1 ? 1 : 1024 / words;
    const dim3 grid((unsigned)(need < 1 ? 1 : need > cap ? cap : need), (unsigned)words), block(256);
    hipLaunchKernelGGL(k_sc_expand, grid, block, 0, stream, (const u64 *)d_table, (i64)n_sets, words, n_colors, (const u64 *)d_vec0,
                       (const u64 *)d_vec1, (const u64 *)d_vec2, (u64 *)d_ref);
}
