// sbwt_positions.hip -- reference positions per column, and reads placed on the references by diagonal voting
// (include/sbwtgpu.h, "positions").  Everything is an integer minimum, sum or maximum, so no result
// depends on the order in which lanes, waves, batches or host threads arrive.
//
//   k_pos_add    the search's int32 results (and the mirrored batch's) -> first[v], one launch per add.  A lane takes one
//                result; a hit finds its sequence and offset by bisecting the window offsets (a reference is ONE read of
//                millions of windows, so nothing here is per read), forms the key and offers it with a 64-bit atomicMin --
//                after a plain load, and only when the value there is larger.
//   k_pos_map    results + first -> one record per read: k_pa_reduce_sets' frame (one wave per read, lane l window 64 it + l).
//                Per hit one 8-byte gather of first[v]; the placement key (seq, o, start) as one 63-bit integer whose order is
//                the tie rule's; the iteration's distinct keys are peeled (readlane, ballot, popcount) into a pending
//                (key, count) run that lives across iterations, and a run that ends goes into the wave's table in LDS:
//                PM_T keys and counts, found by a wave-wide compare.  A read that follows a reference makes one or two
//                entries.  A read whose placements outgrow the table is appended to a list instead of written.
//   k_pos_map_slow  grid-stride over that list, its length read on the device: every hit's key is compared with every other
//                (quadratic in the read's windows, 64 keys per trip: for the odd junk read), which needs no table at all.
#include "sbwt_kernels_common.h"
#include "sbwt_positions.h"
#include "sbwt_posmap.h"

#define PM_T SBWT_PM_TABLE

// ---------------------------------------------------------------------------------------------
// results -> first
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pos_add(const int *__restrict__ res, const int *__restrict__ res2,
                                                 const i64 *__restrict__ out_off, i64 n_reads, i64 first_seq, i64 n_nodes,
                                                 u64 *first, SbwtPosCounters *ctr, u64 *n_hit_windows) {
    pm_for_each_result(res, res2, out_off, n_reads, first_seq, n_nodes, &ctr->n_windows, &ctr->n_hits, n_hit_windows,
                       [&](bool hit, i64 v, u64 key) { if (hit && first[v] > key) atomicMin(first + v, key); });
}

void sbwt_launch_pos_add(const int *d_res, const int *d_res2, const long long *d_out_off, long long n_reads, long long max_results,
                         long long first_seq, long long n_nodes, unsigned long long *d_first, SbwtPosCounters *ctr,
                         unsigned long long *d_n_hit_windows, hipStream_t stream) {
    hipLaunchKernelGGL(k_pos_add, dim3(pm_grid(d_res2 ? 2 * max_results : max_results, 256, 4096)), dim3(256), 0, stream, d_res, d_res2,
                       d_out_off, (i64)n_reads, (i64)first_seq, (i64)n_nodes, (u64 *)d_first, ctr, (u64 *)d_n_hit_windows);
}

__global__ void __launch_bounds__(256) k_pos_check(const u64 *__restrict__ first, i64 n, SbwtPosCounters *ctr) {
    bool bad = false;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        const u64 f = first[i];
        if (f != SBWT_POS_NONE && (f >> 62) != 0) bad = true;      // seq = f >> 32 must stay below 2^30
    }
    if (bad) ctr->bad = 1;
}

void sbwt_launch_pos_check(const unsigned long long *d_first, long long n_nodes, SbwtPosCounters *ctr, hipStream_t stream) {
    hipLaunchKernelGGL(k_pos_check, dim3(pm_grid(n_nodes, 256, 1024)), dim3(256), 0, stream, (const u64 *)d_first, (i64)n_nodes, ctr);
}

// *out += the entries with a position (the caller zeroes it first)
__global__ void __launch_bounds__(256) k_pos_count(const u64 *__restrict__ first, i64 n, u64 *__restrict__ out) {
    u64 mine = 0;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) mine += first[i] != SBWT_POS_NONE;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(out, mine);
}

void sbwt_launch_pos_count(const unsigned long long *d_first, long long n_nodes, unsigned long long *d_out, hipStream_t stream) {
    (void)hipMemsetAsync(d_out, 0, 8, stream);
    hipLaunchKernelGGL(k_pos_count, dim3(pm_grid(n_nodes, 256, 1024)), dim3(256), 0, stream, (const u64 *)d_first, (i64)n_nodes,
                       (u64 *)d_out);
}

// ---------------------------------------------------------------------------------------------
// results + first -> one record per read
// ---------------------------------------------------------------------------------------------
// the key of search s of window q of the read whose windows start at `at` (PM_NOKEY: no hit, or a hit without a position)
__device__ __forceinline__ u64 pm_window_key(const int *__restrict__ res, const int *__restrict__ res2, i64 W, i64 at, i64 q, i64 m,
                                             unsigned s, const u64 *__restrict__ first, i64 n_nodes, bool &hit) {
    const i64 p = at + q;
    const i64 v = s ? res2[W - 1 - p] : res[p];
    hit = v >= 0 && v < n_nodes;
    if (!hit) return PM_NOKEY;
    const u64 f = first[v];
    return f == SBWT_POS_NONE ? PM_NOKEY : pm_key(f, q, m, s);
}

template <bool TWO>
__global__ void __launch_bounds__(256) k_pos_map(const int *__restrict__ res, const int *__restrict__ res2,
                                                 const i64 *__restrict__ out_off, i64 n_reads, const u64 *__restrict__ first,
                                                 i64 n_nodes, int cap, SbwtReadMap *__restrict__ out, SbwtPosMapHeader *hdr,
                                                 unsigned *__restrict__ slow) {
    __shared__ u64 lds_keys[4][PM_T];
    __shared__ int lds_cnt[4][PM_T];
    const int lane = threadIdx.x & 63;
    u64 *keys = lds_keys[threadIdx.x >> 6];
    int *cnt = lds_cnt[threadIdx.x >> 6];
    const i64 n_waves = (i64)gridDim.x * 4;
    const i64 W = out_off[n_reads];
    for (i64 r = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); r < n_reads; r += n_waves) {
        const i64 at = out_off[r];
        const i64 m = out_off[r + 1] - at;                // (< 2^30: the entry points refuse longer reads)
        int found = 0, anchored = 0, n_ent = 0;           // the same in every lane
        u64 pend_key = 0;                                 // the pending run; nothing pending: pend_n = 0
        int pend_n = 0;
        bool fits = true;
        for (i64 q0 = 0; q0 < m && fits; q0 += 64) {
            const i64 q = q0 + lane;
            u64 key[2] = {PM_NOKEY, PM_NOKEY};
            bool hit0 = false, hit1 = false;
            if (q < m) {
                key[0] = pm_window_key(res, res2, W, at, q, m, 0, first, n_nodes, hit0);
                if (TWO) key[1] = pm_window_key(res, res2, W, at, q, m, 1, first, n_nodes, hit1);
            }
            found += __popcll(__ballot(hit0)) + (TWO ? __popcll(__ballot(hit1)) : 0);
#pragma unroll
            for (int s = 0; s < (TWO ? 2 : 1); s++) {
                anchored += __popcll(__ballot(key[s] != PM_NOKEY));
                pm_peel_pending(key[s], pend_key, pend_n, keys, cnt, n_ent, cap, fits, lane);
            }
        }
        if (pend_n != 0 && fits) fits = pm_put(keys, cnt, n_ent, cap, pend_key, pend_n, lane);
        pm_end_read(fits, keys, cnt, n_ent, found, anchored, r, out, hdr, slow, lane);
    }
}

// The reads of the list, exactly and without a table: lane l holds the key of hit slot a0 + l and counts the slots of the
// whole read that carry the same key, 64 of them per trip.  Slot a is search a % S of window a / S (S searches per window).
template <bool TWO>
__global__ void __launch_bounds__(256) k_pos_map_slow(const int *__restrict__ res, const int *__restrict__ res2,
                                                      const i64 *__restrict__ out_off, i64 n_reads, const u64 *__restrict__ first,
                                                      i64 n_nodes, SbwtReadMap *__restrict__ out, const SbwtPosMapHeader *hdr,
                                                      const unsigned *__restrict__ slow) {
    const int lane = threadIdx.x & 63;
    const int S = TWO ? 2 : 1;
    const i64 W = out_off[n_reads];
    i64 n_slow = hdr->n_slow;
    if (n_slow > n_reads) n_slow = n_reads;               // (never: a read is listed once)
    for (i64 e = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); e < n_slow; e += (i64)gridDim.x * 4) {
        const i64 r = slow[e];
        if (r >= n_reads) continue;                       // (never)
        const i64 at = out_off[r];
        const i64 m = out_off[r + 1] - at;
        const i64 n_slots = m * S;
        int found = 0, anchored = 0;
        PmBest best = {PM_NOKEY, 0, 0};
        for (i64 a0 = 0; a0 < n_slots; a0 += 64) {
            const i64 a = a0 + lane;
            bool hit = false;
            u64 mine = PM_NOKEY;
            if (a < n_slots) mine = pm_window_key(res, res2, W, at, a / S, m, (unsigned)(a % S), first, n_nodes, hit);
            found += __popcll(__ballot(hit));
            const u64 have = __ballot(mine != PM_NOKEY);
            anchored += __popcll(have);
            if (!have) continue;
            int c = 0;
            for (i64 b0 = 0; b0 < n_slots; b0 += 64) {
                const i64 b = b0 + lane;
                bool hit_b = false;
                u64 other = PM_NOKEY;
                if (b < n_slots) other = pm_window_key(res, res2, W, at, b / S, m, (unsigned)(b % S), first, n_nodes, hit_b);
                u64 left = __ballot(other != PM_NOKEY);
                while (left) {
                    const int src = __ffsll((i64)left) - 1;
                    left &= left - 1;
                    c += pm_readlane64(other, src) == mine;
                }
            }
            if (mine != PM_NOKEY) pm_offer(best, mine, c);
        }
        pm_write(best, found, anchored, out + r, lane);
    }
}

void sbwt_launch_pos_map(const int *d_res, const int *d_res2, const long long *d_out_off, long long n_reads,
                         const unsigned long long *d_first, long long n_nodes, int cap, SbwtReadMap *d_out, SbwtPosMapHeader *hdr,
                         unsigned *d_slow, hipStream_t stream) {
    if (cap < 1 || cap > PM_T) cap = PM_T;
    (void)hipMemsetAsync(hdr, 0, sizeof(SbwtPosMapHeader), stream);
    // a block's four waves take four reads per round
    const dim3 grid(pm_grid(n_reads, 4, 1 << 20)), slow_grid(pm_grid(n_reads, 4, 1024)), block(256);
    pm_strands(d_res2 != nullptr, [&](auto two) {
        constexpr bool TWO = decltype(two)::value;
        hipLaunchKernelGGL((k_pos_map<TWO>), grid, block, 0, stream, d_res, d_res2, d_out_off, (i64)n_reads, (const u64 *)d_first,
                           (i64)n_nodes, cap, d_out, hdr, d_slow);
        hipLaunchKernelGGL((k_pos_map_slow<TWO>), slow_grid, block, 0, stream, d_res, d_res2, d_out_off, (i64)n_reads,
                           (const u64 *)d_first, (i64)n_nodes, d_out, hdr, d_slow);
    });
}
