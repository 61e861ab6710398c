// sbwt_occurrences.hip -- every reference occurrence of every column's k-mer as CSR arrays (off, occ), and reads placed on the
// references by diagonal voting over ALL occurrences (include/sbwtgpu.h, "occurrences").  Everything is
// an integer sum, minimum or maximum over a SET of (column, key) pairs, so no result depends on the order in which lanes,
// waves, batches or host threads arrive.
//
//   k_occ_add    the search's int32 results (and the mirrored batch's) -> (column, key) appended to the builder's log: k_pos_add's
//                frame (a lane per result, sequence and offset by bisecting the window offsets), and instead of an atomic
//                minimum a wave-aggregated append: ballot, ONE atomic per wave on the log's length, prefix popcount.
//   finish       sort the log by (column, key) with two stable rocPRIM radix sorts, k_occ_flag marks the first entry of every
//                run of equal pairs and counts them per column, an exclusive scan makes off, a flagged select makes occ.
//   k_occ_map    results + (off, occ) -> one record per read: k_pos_map's frame.  Per hit one gather of off[v], off[v + 1]
//                (adjacent), then trip j = 0, 1, ... loads occ[off[v] + j] in the lanes whose column has more than j
//                occurrences.  The keys of a column ascend by (seq, pos): a read in a stretch shared by C references sees the
//                same C placements window after window, one per j, so the kernel carries a pending (key, count) run PER j for
//                j < OM_NP in registers -- lane j of one register pair and one count holds rank j's run, read with readlane --
//                and the table in LDS is touched once per placement, not once per iteration.  Runs of j >= OM_NP go
//                straight to the table.  A read whose placements outgrow the table is appended to a list.
//   k_occ_map_slow  grid-stride over that list: the read's votes are enumerated again in P slices of the key space (a hash
//                of the key modulo P), only the current slice's keys enter the table, P doubles until every slice fits; the
//                slices' (best, runner-up) fold with pm_offer, exactly, because slices hold disjoint keys.  A read that no
//                P up to SBWT_OM_MAX_SLICES fits is marked on the list.
//   k_occ_map_last  grid-stride over the marked entries: key by key in ascending order with no table at all.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include "sbwt_kernels_common.h"
#include "sbwt_occurrences.h"
#include "sbwt_posmap.h"

#define OM_T SBWT_OM_TABLE
#define OM_NP SBWT_OM_PENDING

// ---------------------------------------------------------------------------------------------
// results -> log
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_occ_add(const int *__restrict__ res, const int *__restrict__ res2,
                                                 const i64 *__restrict__ out_off, i64 n_reads, i64 first_seq, i64 n_nodes,
                                                 unsigned *__restrict__ log_col, u64 *__restrict__ log_key, u64 log_cap,
                                                 SbwtOccCounters *ctr, u64 *n_hit_windows) {
    const int lane = threadIdx.x & 63;
    pm_for_each_result(res, res2, out_off, n_reads, first_seq, n_nodes, &ctr->n_windows, &ctr->n_hits, n_hit_windows,
                       [&](bool hit, i64 v, u64 key) {
        const u64 hm = __ballot(hit);
        if (!hm) return;                                   // one atomic per wave, then every hit its own slot
        u64 base = 0;
        if (lane == 0) base = atomicAdd(&ctr->log_len, (u64)__popcll(hm));
        base = pm_readlane64(base, 0);
        if (hit) {
            const u64 e = base + (u64)__popcll(hm & ((1ull << lane) - 1ull));
            if (e < log_cap) { log_col[e] = (unsigned)v; log_key[e] = key; }
            else ctr->bad_kind = 1;                        // (never: the host makes room for every result before the launch)
        }
    });
}

void sbwt_launch_occ_add(const int *d_res, const int *d_res2, const long long *d_out_off, long long n_reads, long long max_results,
                         long long first_seq, long long n_nodes, unsigned *d_log_col, unsigned long long *d_log_key,
                         unsigned long long log_cap, SbwtOccCounters *ctr, unsigned long long *d_n_hit_windows, hipStream_t stream) {
    hipLaunchKernelGGL(k_occ_add, dim3(pm_grid(d_res2 ? 2 * max_results : max_results, 256, 4096)), dim3(256), 0, stream, d_res, d_res2,
                       d_out_off, (i64)n_reads, (i64)first_seq, (i64)n_nodes, d_log_col, (u64 *)d_log_key, (u64)log_cap, ctr,
                       (u64 *)d_n_hit_windows);
}

// ---------------------------------------------------------------------------------------------
// log -> (off, occ)
// ---------------------------------------------------------------------------------------------
size_t sbwt_occ_sort_tmp_bytes(long long n) {
    size_t a = 0, b = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a, (const u64 *)nullptr, (u64 *)nullptr, (const unsigned *)nullptr, (unsigned *)nullptr,
                                    (size_t)n, 0u, 64u, (hipStream_t) nullptr);
    (void)rocprim::radix_sort_pairs(nullptr, b, (const unsigned *)nullptr, (unsigned *)nullptr, (const u64 *)nullptr, (u64 *)nullptr,
                                    (size_t)n, 0u, 32u, (hipStream_t) nullptr);
    return (a > b ? a : b) + 256;
}

hipError_t sbwt_occ_sort(unsigned *d_log_col, unsigned long long *d_log_key, unsigned *d_alt_col, unsigned long long *d_alt_key,
                         long long n, int key_bits, int col_bits, void *tmp, size_t tmp_bytes, hipStream_t stream) {
    if (key_bits < 1) key_bits = 1;
    if (key_bits > 64) key_bits = 64;
    if (col_bits < 1) col_bits = 1;
    if (col_bits > 32) col_bits = 32;
    size_t bytes = tmp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(tmp, bytes, (const u64 *)d_log_key, (u64 *)d_alt_key, (const unsigned *)d_log_col, d_alt_col,
                                             (size_t)n, 0u, (unsigned)key_bits, stream);
    if (e != hipSuccess) return e;
    bytes = tmp_bytes;
    return rocprim::radix_sort_pairs(tmp, bytes, (const unsigned *)d_alt_col, d_log_col, (const u64 *)d_alt_key, (u64 *)d_log_key, (size_t)n,
                                     0u, (unsigned)col_bits, stream);
}

__global__ void __launch_bounds__(256) k_occ_flag(const unsigned *__restrict__ col, const u64 *__restrict__ key, i64 n,
                                                  unsigned char *__restrict__ flag, u64 *off, SbwtOccCounters *ctr) {
    const int lane = threadIdx.x & 63;
    u64 mine = 0;                                          // of this lane's wave
    for (i64 i0 = (i64)blockIdx.x * 256 + (threadIdx.x & ~63u); i0 < n; i0 += (i64)gridDim.x * 256) {
        const i64 i = i0 + lane;
        bool f = false;
        if (i < n) {
            f = i == 0 || col[i] != col[i - 1] || key[i] != key[i - 1];
            flag[i] = f;
            if (f) atomicAdd(off + col[i], 1ull);
        }
        mine += (u64)__popcll(__ballot(f));
    }
    if (lane == 0 && mine) atomicAdd(&ctr->n_unique, mine);
}

void sbwt_launch_occ_flag(const unsigned *d_col, const unsigned long long *d_key, long long n, unsigned char *d_flag,
                          unsigned long long *d_off, long long n_nodes, SbwtOccCounters *ctr, hipStream_t stream) {
    (void)hipMemsetAsync(d_off, 0, (size_t)(n_nodes + 1) * 8, stream);
    (void)hipMemsetAsync(&ctr->n_unique, 0, 8, stream);
    if (n > 0)
        hipLaunchKernelGGL(k_occ_flag, dim3(pm_grid(n, 256, 4096)), dim3(256), 0, stream, d_col, (const u64 *)d_key, (i64)n, d_flag,
                           (u64 *)d_off, ctr);
}

size_t sbwt_occ_scan_tmp_bytes(long long n_nodes) {
    size_t a = 0;
    (void)rocprim::exclusive_scan(nullptr, a, (const u64 *)nullptr, (u64 *)nullptr, (u64)0, (size_t)n_nodes + 1, rocprim::plus<u64>(),
                                  (hipStream_t) nullptr);
    return a + 256;
}
hipError_t sbwt_occ_scan(unsigned long long *d_off, long long n_nodes, void *tmp, size_t tmp_bytes, hipStream_t stream) {
    return rocprim::exclusive_scan(tmp, tmp_bytes, (const u64 *)d_off, (u64 *)d_off, (u64)0, (size_t)n_nodes + 1, rocprim::plus<u64>(), stream);
}

size_t sbwt_occ_select_tmp_bytes(long long n) {
    size_t a = 0;
    (void)rocprim::select(nullptr, a, (const u64 *)nullptr, (const unsigned char *)nullptr, (u64 *)nullptr, (u64 *)nullptr, (size_t)n,
                          (hipStream_t) nullptr);
    return a + 256;
}
hipError_t sbwt_occ_select(const unsigned long long *d_key, const unsigned char *d_flag, long long n, unsigned long long *d_occ,
                           unsigned long long *d_count, void *tmp, size_t tmp_bytes, hipStream_t stream) {
    return rocprim::select(tmp, tmp_bytes, (const u64 *)d_key, d_flag, (u64 *)d_occ, (u64 *)d_count, (size_t)n, stream);
}

__global__ void __launch_bounds__(256) k_occ_stats(const u64 *__restrict__ off, i64 n, SbwtOccCounters *ctr) {
    u64 pos = 0, mx = 0;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        const u64 c = off[i + 1] - off[i];
        pos += c != 0;
        if (c > mx) mx = c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        pos += __shfl_down(pos, o);
        const u64 om = __shfl_down(mx, o);
        if (om > mx) mx = om;
    }
    if ((threadIdx.x & 63) == 0) {
        if (pos) atomicAdd(&ctr->n_positioned, pos);
        if (mx) atomicMax(&ctr->max_count, mx);
    }
}

void sbwt_launch_occ_stats(const unsigned long long *d_off, long long n_nodes, SbwtOccCounters *ctr, hipStream_t stream) {
    (void)hipMemsetAsync(&ctr->n_positioned, 0, 16, stream);       // (n_positioned and max_count are neighbours)
    hipLaunchKernelGGL(k_occ_stats, dim3(pm_grid(n_nodes, 256, 1024)), dim3(256), 0, stream, (const u64 *)d_off, (i64)n_nodes, ctr);
}

__device__ __forceinline__ void occ_bad(SbwtOccCounters *ctr, i64 column, u64 kind) {
    const u64 before = atomicMin(&ctr->bad_column, (u64)column);
    if ((u64)column < before) ctr->bad_kind = kind;        // (two kinds on one column: either names it)
}

__global__ void __launch_bounds__(256) k_occ_check_off(const u64 *__restrict__ off, i64 n, u64 n_occ, SbwtOccCounters *ctr) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i <= n; i += (i64)gridDim.x * 256) {
        if (i == 0 && off[0] != 0) occ_bad(ctr, 0, SBWT_OCC_BAD_OFF0);
        if (i < n && off[i] > off[i + 1]) occ_bad(ctr, i, SBWT_OCC_BAD_MONOTONE);
        if (i == n && off[n] != n_occ) occ_bad(ctr, n > 0 ? n - 1 : 0, SBWT_OCC_BAD_TOTAL);
    }
}
// (after k_occ_check_off passed: 0 = off[0] <= ... <= off[n] = n_occ, so every index below is inside occ)
__global__ void __launch_bounds__(256) k_occ_check_keys(const u64 *__restrict__ off, const u64 *__restrict__ occ, i64 n,
                                                        SbwtOccCounters *ctr) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        const u64 lo = off[i], hi = off[i + 1];
        u64 kind = 0;
        for (u64 e = lo; e < hi && !kind; e++) {
            const u64 f = occ[e];
            if ((f >> 62) != 0) kind = SBWT_OCC_BAD_SEQ;   // seq = f >> 32 must stay below 2^30
            else if (e > lo && occ[e - 1] >= f) kind = SBWT_OCC_BAD_ORDER;
        }
        if (kind) occ_bad(ctr, i, kind);
    }
}
void sbwt_launch_occ_check_off(const unsigned long long *d_off, long long n_nodes, unsigned long long n_occ, SbwtOccCounters *ctr,
                               hipStream_t stream) {
    hipLaunchKernelGGL(k_occ_check_off, dim3(pm_grid(n_nodes + 1, 256, 1024)), dim3(256), 0, stream, (const u64 *)d_off, (i64)n_nodes,
                       (u64)n_occ, ctr);
}
void sbwt_launch_occ_check_keys(const unsigned long long *d_off, const unsigned long long *d_occ, long long n_nodes, SbwtOccCounters *ctr,
                                hipStream_t stream) {
    hipLaunchKernelGGL(k_occ_check_keys, dim3(pm_grid(n_nodes, 256, 1024)), dim3(256), 0, stream, (const u64 *)d_off, (const u64 *)d_occ,
                       (i64)n_nodes, ctr);
}

__global__ void __launch_bounds__(256) k_occ_first(const u64 *__restrict__ off, const u64 *__restrict__ occ, i64 n,
                                                   u64 *__restrict__ first) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        const u64 lo = off[i];
        first[i] = off[i + 1] > lo ? occ[lo] : SBWT_POS_NONE;
    }
}
void sbwt_launch_occ_first(const unsigned long long *d_off, const unsigned long long *d_occ, long long n_nodes, unsigned long long *d_first,
                           hipStream_t stream) {
    hipLaunchKernelGGL(k_occ_first, dim3(pm_grid(n_nodes, 256, 1024)), dim3(256), 0, stream, (const u64 *)d_off, (const u64 *)d_occ,
                       (i64)n_nodes, (u64 *)d_first);
}

// ---------------------------------------------------------------------------------------------
// results + (off, occ) -> one record per read
// ---------------------------------------------------------------------------------------------
// A lane's hit of search s of window q: the column's first occurrence index and its count (0: no hit, an empty column, or
// more than max_occ occurrences -- found, not anchored).
__device__ __forceinline__ void om_window(const int *__restrict__ res, const int *__restrict__ res2, i64 W, i64 at, i64 q, i64 m,
                                          unsigned s, const u64 *__restrict__ off, i64 n_nodes, u64 max_occ, bool &hit, u64 &base,
                                          int &c) {
    hit = false; base = 0; c = 0;
    if (q >= m) return;
    const i64 p = at + q;
    const i64 v = s ? res2[W - 1 - p] : res[p];
    hit = v >= 0 && v < n_nodes;
    if (!hit) return;
    base = off[v];
    const u64 cc = off[v + 1] - base;
    c = cc > max_occ ? 0 : (int)cc;
}

template <bool TWO>
__global__ void __launch_bounds__(256) k_occ_map(const int *__restrict__ res, const int *__restrict__ res2,
                                                 const i64 *__restrict__ out_off, i64 n_reads, const u64 *__restrict__ off,
                                                 const u64 *__restrict__ occ, i64 n_nodes, u64 max_occ, int cap,
                                                 SbwtReadMap *__restrict__ out, SbwtPosMapHeader *hdr, unsigned *__restrict__ slow) {
    __shared__ u64 lds_keys[4][OM_T];
    __shared__ int lds_cnt[4][OM_T];
    const int lane = threadIdx.x & 63;
    u64 *keys = lds_keys[threadIdx.x >> 6];
    int *cnt = lds_cnt[threadIdx.x >> 6];
    const i64 n_waves = (i64)gridDim.x * 4;
    const i64 W = out_off[n_reads];
    for (i64 r = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); r < n_reads; r += n_waves) {
        const i64 at = out_off[r];
        const i64 m = out_off[r + 1] - at;                // (< 2^30: the entry points refuse longer reads)
        int found = 0, anchored = 0, n_ent = 0;           // the same in every lane
        u64 pend_key = 0;                                 // LANE j holds the pending run of occurrence rank j < OM_NP (one
        int pend_n = 0;                                   // register pair and a count for all of them); nothing pending: 0
        bool fits = true;
        for (i64 q0 = 0; q0 < m && fits; q0 += 64) {
            const i64 q = q0 + lane;
#pragma unroll 1
            for (int s = 0; s < (TWO ? 2 : 1); s++) {
                bool hit;
                u64 base;
                int c;
                om_window(res, res2, W, at, q, m, (unsigned)s, off, n_nodes, max_occ, hit, base, c);
                found += __popcll(__ballot(hit));
                anchored += __popcll(__ballot(c > 0));
                for (int j = 0; fits && __ballot(c > j); j++) {
                    const u64 mine = c > j ? pm_key(occ[base + j], q, m, (unsigned)s) : PM_NOKEY;
                    if (j < OM_NP) {
                        u64 pk = pm_readlane64(pend_key, j);
                        int pn = __builtin_amdgcn_readlane(pend_n, j);
                        pm_peel_pending(mine, pk, pn, keys, cnt, n_ent, cap, fits, lane);
                        if (lane == j) { pend_key = pk; pend_n = pn; }
                    } else {
                        pm_peel_put(mine, keys, cnt, n_ent, cap, fits, lane);
                    }
                }
            }
        }
        for (int j = 0; j < OM_NP && fits; j++) {
            const u64 pk = pm_readlane64(pend_key, j);
            const int pn = __builtin_amdgcn_readlane(pend_n, j);
            if (pn != 0) fits = pm_put(keys, cnt, n_ent, cap, pk, pn, lane);
        }
        pm_end_read(fits, keys, cnt, n_ent, found, anchored, r, out, hdr, slow, lane);
    }
}

// Every vote of the read, 64 at a time: f(mine) once per (iteration, search, trip) with the lanes' keys (PM_NOKEY: none), in
// the order k_occ_map takes them; f returns false to stop (the same in every lane).  found and anchored are set, in every lane
// to the read's totals (they are summed per lane and folded at the end: the second kernels are short of scalar registers).
template <bool TWO, typename F>
__device__ __forceinline__ bool om_enumerate(const int *__restrict__ res, const int *__restrict__ res2, i64 W, i64 at, i64 m,
                                             const u64 *__restrict__ off, const u64 *__restrict__ occ, i64 n_nodes, u64 max_occ, int lane,
                                             int &found, int &anchored, F f) {
    int nf = 0, na = 0;                                   // this lane's
    bool go = true;
    for (i64 q0 = 0; q0 < m && go; q0 += 64) {
        const i64 q = q0 + lane;
#pragma unroll 1
        for (int s = 0; s < (TWO ? 2 : 1) && go; s++) {
            bool hit;
            u64 base;
            int c;
            om_window(res, res2, W, at, q, m, (unsigned)s, off, n_nodes, max_occ, hit, base, c);
            nf += hit;
            na += c > 0;
            for (int j = 0; go && __ballot(c > j); j++) {
                const u64 mine = c > j ? pm_key(occ[base + j], q, m, (unsigned)s) : PM_NOKEY;
                go = f(mine);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nf += __shfl_xor(nf, o);
        na += __shfl_xor(na, o);
    }
    found = nf;
    anchored = na;
    return go;
}

__device__ __forceinline__ unsigned om_slice(u64 key, unsigned P) { return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 48) & (P - 1u); }

#define OM_LAST 0x80000000u     // on a list entry: no slicing up to SBWT_OM_MAX_SLICES fitted, k_occ_map_last writes the record

// The reads of the list in slices of the key space: slice sl of P into the table, the slices' candidates folded per lane; a
// slice that outgrows the table starts the read again with 2 P slices.
template <bool TWO>
__global__ void __launch_bounds__(256) k_occ_map_slow(const int *__restrict__ res, const int *__restrict__ res2,
                                                      const i64 *__restrict__ out_off, i64 n_reads, const u64 *__restrict__ off,
                                                      const u64 *__restrict__ occ, i64 n_nodes, u64 max_occ, int cap,
                                                      SbwtReadMap *__restrict__ out, const SbwtPosMapHeader *hdr, unsigned *slow) {
    __shared__ u64 lds_keys[4][OM_T];
    __shared__ int lds_cnt[4][OM_T];
    const int lane = threadIdx.x & 63;
    u64 *keys = lds_keys[threadIdx.x >> 6];
    int *cnt = lds_cnt[threadIdx.x >> 6];
    const i64 W = out_off[n_reads];
    i64 n_slow = hdr->n_slow;
    if (n_slow > n_reads) n_slow = n_reads;               // (never: a read is listed once)
    for (i64 e = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); e < n_slow; e += (i64)gridDim.x * 4) {
        const i64 r = slow[e];
        if (r >= n_reads) continue;                       // (never)
        const i64 at = out_off[r];
        const i64 m = out_off[r + 1] - at;
        int found = 0, anchored = 0;
        PmBest best = {PM_NOKEY, 0, 0};
        bool fits = false;
        for (unsigned P = 2; P <= SBWT_OM_MAX_SLICES && !fits; P <<= 1) {
            best = {PM_NOKEY, 0, 0};
            fits = true;
            for (unsigned sl = 0; sl < P && fits; sl++) {
                int n_ent = 0;
                om_enumerate<TWO>(res, res2, W, at, m, off, occ, n_nodes, max_occ, lane, found, anchored, [&](u64 mine) {
                    if (mine != PM_NOKEY && om_slice(mine, P) != sl) mine = PM_NOKEY;
                    pm_peel_put(mine, keys, cnt, n_ent, cap, fits, lane);
                    return fits;
                });
                if (fits)
                    for (int j = lane; j < n_ent; j += 64) pm_offer(best, keys[j], cnt[j]);
                __builtin_amdgcn_wave_barrier();          // (the next slice's first entry comes after these loads)
            }
        }
        if (fits) pm_write(best, found, anchored, out + r, lane);
        else if (lane == 0) slow[e] = (unsigned)r | OM_LAST;
    }
}

// The marked reads of the list without a table: the keys one by one in ascending order.  A pass counts the votes of the
// current key and finds the smallest key above it; every lane ends with the same candidates.  One enumeration of the read's
// votes per distinct placement.
template <bool TWO>
__global__ void __launch_bounds__(256) k_occ_map_last(const int *__restrict__ res, const int *__restrict__ res2,
                                                      const i64 *__restrict__ out_off, i64 n_reads, const u64 *__restrict__ off,
                                                      const u64 *__restrict__ occ, i64 n_nodes, u64 max_occ,
                                                      SbwtReadMap *__restrict__ out, const SbwtPosMapHeader *hdr,
                                                      const unsigned *__restrict__ slow) {
    const int lane = threadIdx.x & 63;
    const i64 W = out_off[n_reads];
    i64 n_slow = hdr->n_slow;
    if (n_slow > n_reads) n_slow = n_reads;               // (never)
    for (i64 e = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); e < n_slow; e += (i64)gridDim.x * 4) {
        const unsigned x = slow[e];
        if (!(x & OM_LAST)) continue;
        const i64 r = x & ~OM_LAST;
        if (r >= n_reads) continue;                       // (never)
        const i64 at = out_off[r];
        const i64 m = out_off[r + 1] - at;
        int found = 0, anchored = 0;
        PmBest best = {PM_NOKEY, 0, 0};
        u64 cur = 0;
        bool have = false;
        for (;;) {
            u64 nxt = PM_NOKEY;
            int c = 0;
            om_enumerate<TWO>(res, res2, W, at, m, off, occ, n_nodes, max_occ, lane, found, anchored, [&](u64 mine) {
                if (mine != PM_NOKEY) {
                    if (have && mine == cur) c++;
                    else if ((!have || mine > cur) && mine < nxt) nxt = mine;
                }
                return true;
            });
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                c += __shfl_xor(c, o);
                const u64 on = __shfl_xor(nxt, o);
                if (on < nxt) nxt = on;
            }
            if (have) pm_offer(best, cur, c);
            if (nxt == PM_NOKEY) break;
            cur = nxt;
            have = true;
        }
        pm_write(best, found, anchored, out + r, lane);
    }
}

void sbwt_launch_occ_map(const int *d_res, const int *d_res2, const long long *d_out_off, long long n_reads,
                         const unsigned long long *d_off, const unsigned long long *d_occ, long long n_nodes, int max_occ, int cap,
                         SbwtReadMap *d_out, SbwtPosMapHeader *hdr, unsigned *d_slow, hipStream_t stream) {
    if (cap < 1 || cap > OM_T) cap = OM_T;
    (void)hipMemsetAsync(hdr, 0, sizeof(SbwtPosMapHeader), stream);
    // a block's four waves take four reads per round
    const dim3 grid(pm_grid(n_reads, 4, 1 << 20)), slow_grid(pm_grid(n_reads, 4, 1024)), block(256);
    const u64 *off = (const u64 *)d_off, *occ = (const u64 *)d_occ;
    pm_strands(d_res2 != nullptr, [&](auto two) {
        constexpr bool TWO = decltype(two)::value;
        hipLaunchKernelGGL((k_occ_map<TWO>), grid, block, 0, stream, d_res, d_res2, d_out_off, (i64)n_reads, off, occ, (i64)n_nodes,
                           (u64)max_occ, cap, d_out, hdr, d_slow);
        hipLaunchKernelGGL((k_occ_map_slow<TWO>), slow_grid, block, 0, stream, d_res, d_res2, d_out_off, (i64)n_reads, off, occ,
                           (i64)n_nodes, (u64)max_occ, cap, d_out, hdr, d_slow);
        hipLaunchKernelGGL((k_occ_map_last<TWO>), slow_grid, block, 0, stream, d_res, d_res2, d_out_off, (i64)n_reads, off, occ,
                           (i64)n_nodes, (u64)max_occ, d_out, hdr, d_slow);
    });
}
