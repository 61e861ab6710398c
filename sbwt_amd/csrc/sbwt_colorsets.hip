// sbwt_colorsets.hip -- deduplicated colour sets: a pan-genome's columns carry few distinct colour rows, so a column keeps a
// 4-byte id and the distinct rows of `words` 64-bit words lie once in a table (include/sbwtgpu.h, "colour sets"; DESIGN.md
// section 15).  The object means the wide matrix rows[j * words + w] = table[ids[j] * words + w] of sbwt_colors.hip.
//
//   k_cs_insert    matrix -> hash table of representative columns: a lane hashes its column's row and probes an
//                  open-addressing table of 2 n + 1 uint32 slots.  An empty slot is taken by compare-and-swap; a taken one is
//                  compared with the FULL row of its representative (never by hash) -- equal: atomicMin towards the smaller
//                  column (loaded first, the atomic skipped when it would not lower it), different: the next slot.  Every
//                  representative a slot ever holds carries the same row and the matrix does not change, so the compare has
//                  no race, and at the end a slot holds its class's smallest column whatever the order of arrival.  The
//                  column keeps its slot in ids[] for k_cs_assign; a zero row keeps CS_EMPTY and never touches the table.
//   k_cs_insert_wave  the same for rows of more than two words: a wave per column, lane w word w, so that rows are read coalesced
//   k_cs_flag      slots -> one byte per column: 1 for a representative
//   (rocPRIM)      exclusive scan of the flags: a class's id is 1 + the scan value of its representative -- the classes in the
//                  order of their smallest columns, which is the canonical form
//   k_cs_assign    every column turns its slot into its id; the representative copies its row into the table
//   k_cs_expand    ids + table -> wide matrix, grid-stride over the n x words words
//   k_cs_check_ids, k_cs_check_table   an uploaded object: dummy columns' ids to 0, ids < n_sets, row 0 zero, no other row
//                  zero, no bit >= n_colors
//   k_pa_reduce_sets  results + ids + table -> records: k_pa_reduce_wide's frame (one wave per read, lane l window 64 it + l,
//                  word 0's counters in a register, the others in LDS at [wave][w - 1][lane]) with a 4-byte gather per lane.
//                  A window's key is its id (two strands: the ordered pair of its two ids); the wave keeps a pending
//                  (key, count) in scalar registers, the distinct keys of an iteration are peeled one ballot each, and only a
//                  change of key loads a table row: lane w loads word w, the non-zero words are broadcast one by one and the
//                  lanes of their set bits add the count.  No per-colour ballot anywhere.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include "sbwt_colwalk.h"
#include "sbwt_colorsets.h"

#define CS_EMPTY 0xFFFFFFFFu

// grid for a grid-stride loop over n items: enough blocks to fill the chip, no more
static inline unsigned cs_stride_grid(i64 n) {
    const i64 g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : g > 8192 ? 8192 : g);
}

// ---------------------------------------------------------------------------------------------
// matrix -> ids + table
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 cs_mix(u64 h, u64 x) {
    h = (h ^ x) * 0xff51afd7ed558ccdull;
    return h ^ (h >> 32);
}

__global__ void __launch_bounds__(256) k_cs_insert(const u64 *__restrict__ rows, i64 n, int words, unsigned *slots, u64 n_slots,
                                                   unsigned *__restrict__ ids) {
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < n; j += (i64)gridDim.x * 256) {
        const u64 *row = rows + j * (i64)words;
        u64 any = 0, h = 0x9e3779b97f4a7c15ull;
        for (int w = 0; w < words; w++) {
            const u64 x = row[w];
            any |= x;
            h = cs_mix(h, x);
        }
        if (!any) { ids[j] = CS_EMPTY; continue; }
        u64 s = __umul64hi(cs_mix(h, (u64)words), n_slots);          // (uniform over [0, n_slots))
        for (;;) {
            unsigned cur = slots[s];
            if (cur == CS_EMPTY) {
                cur = atomicCAS(slots + s, CS_EMPTY, (unsigned)j);
                if (cur == CS_EMPTY) break;                           // this column is the slot's first representative
            }
            bool same = cur == (unsigned)j;
            if (!same) {
                const u64 *other = rows + (i64)cur * (i64)words;
                same = true;
                for (int w = 0; w < words && same; w++) same = row[w] == other[w];
            }
            if (same) {
                if ((unsigned)j < cur) atomicMin(slots + s, (unsigned)j);
                break;
            }
            s = s + 1 == n_slots ? 0 : s + 1;
        }
        ids[j] = (unsigned)s;
    }
}

// The same with one wave per column, for rows of more than CS_LANE_WORDS words: lane w holds word w (one coalesced load of the
// row, one of a representative's), the row's hash is the XOR of the lanes' position-dependent hashes, and lane 0 does the
// slot's atomics.  Which of the two kernels ran does not show in the result: the slots end with the classes' smallest columns.
#define CS_LANE_WORDS 2
__global__ void __launch_bounds__(256) k_cs_insert_wave(const u64 *__restrict__ rows, i64 n, int words, unsigned *slots, u64 n_slots,
                                                        unsigned *__restrict__ ids) {
    const int lane = threadIdx.x & 63;
    const i64 n_waves = (i64)gridDim.x * 4;
    for (i64 j = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); j < n; j += n_waves) {
        const u64 x = lane < words ? rows[j * (i64)words + lane] : 0;
        if (!__ballot(x != 0)) {
            if (lane == 0) ids[j] = CS_EMPTY;
            continue;
        }
        u64 h = x ? cs_mix(0x9e3779b97f4a7c15ull + (u64)lane, x) : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) h ^= (u64)__shfl_xor((long long)h, off);
        u64 s = __umul64hi(cs_mix(h, (u64)words), n_slots);          // (the same in every lane)
        for (;;) {
            unsigned cur = 0;
            if (lane == 0) {
                cur = slots[s];
                if (cur == CS_EMPTY) {
                    cur = atomicCAS(slots + s, CS_EMPTY, (unsigned)j);
                    if (cur == CS_EMPTY) cur = (unsigned)j;          // this column is the slot's first representative
                }
            }
            cur = (unsigned)__builtin_amdgcn_readfirstlane((int)cur);
            if (cur == (unsigned)j) break;
            const u64 y = lane < words ? rows[(i64)cur * (i64)words + lane] : 0;
            if (!__ballot(x != y)) {
                if (lane == 0 && (unsigned)j < cur) atomicMin(slots + s, (unsigned)j);
                break;
            }
            s = s + 1 == n_slots ? 0 : s + 1;
        }
        if (lane == 0) ids[j] = (unsigned)s;
    }
}

__global__ void __launch_bounds__(256) k_cs_flag(const unsigned *__restrict__ slots, u64 n_slots, unsigned char *__restrict__ flags) {
    for (u64 s = (u64)blockIdx.x * 256 + threadIdx.x; s < n_slots; s += (u64)gridDim.x * 256) {
        const unsigned c = slots[s];
        if (c != CS_EMPTY) flags[c] = 1;
    }
}

__global__ void __launch_bounds__(256) k_cs_assign(const u64 *__restrict__ rows, i64 n, int words, const unsigned *__restrict__ slots,
                                                   const unsigned *__restrict__ rank, unsigned *__restrict__ ids,
                                                   u64 *__restrict__ table) {
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < n; j += (i64)gridDim.x * 256) {
        const unsigned s = ids[j];
        if (s == CS_EMPTY) { ids[j] = 0; continue; }
        const unsigned rep = slots[s];
        const unsigned id = 1u + rank[rep];
        ids[j] = id;
        if (rep == (unsigned)j)
            for (int w = 0; w < words; w++) table[(i64)id * words + w] = rows[j * (i64)words + w];
    }
}

struct CsByteToU32 {
    __host__ __device__ unsigned operator()(unsigned char b) const { return b; }
};

hipError_t sbwt_colorsets_compress(const unsigned long long *d_rows, long long n, int words, unsigned **d_ids,
                                   unsigned long long **d_table, long long *n_sets, hipStream_t stream) {
    const u64 n_slots = 2ull * (u64)n + 1;                  // (n < 2^31: fewer than 2^32 - 1 slots, so CS_EMPTY is no slot number)
    unsigned *ids = nullptr, *slots = nullptr, *rank = nullptr;
    unsigned char *flags = nullptr;
    void *tmp = nullptr;
    u64 *table = nullptr;
    size_t tmp_bytes = 0;
    unsigned total = 0;
    *d_ids = nullptr;
    *d_table = nullptr;
    *n_sets = 0;
    const unsigned g = cs_stride_grid(n);
    hipError_t e = hipMalloc((void **)&ids, (size_t)n * 4 + 16);
    if (e == hipSuccess) e = hipMalloc((void **)&slots, (size_t)n_slots * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&flags, (size_t)n + 1);
    if (e == hipSuccess) e = hipMalloc((void **)&rank, ((size_t)n + 1) * 4);
    const auto flags_in = rocprim::make_transform_iterator((const unsigned char *)flags, CsByteToU32());
    if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, tmp_bytes, flags_in, rank, 0u, (size_t)n + 1, rocprim::plus<unsigned>(), stream);
    if (e == hipSuccess) e = hipMalloc(&tmp, tmp_bytes + 16);
    if (e == hipSuccess) e = hipMemsetAsync(slots, 0xFF, (size_t)n_slots * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(flags, 0, (size_t)n + 1, stream);
    if (e == hipSuccess) {
        if (words > CS_LANE_WORDS) {
            const i64 gb = ((i64)n + 3) / 4;
            hipLaunchKernelGGL(k_cs_insert_wave, dim3((unsigned)(gb < 1 ? 1 : gb > 16384 ? 16384 : gb)), dim3(256), 0, stream,
                               (const u64 *)d_rows, (i64)n, words, slots, n_slots, ids);
        } else {
            hipLaunchKernelGGL(k_cs_insert, dim3(g), dim3(256), 0, stream, (const u64 *)d_rows, (i64)n, words, slots, n_slots, ids);
        }
        hipLaunchKernelGGL(k_cs_flag, dim3(cs_stride_grid((i64)n_slots)), dim3(256), 0, stream, (const unsigned *)slots, n_slots, flags);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = rocprim::exclusive_scan(tmp, tmp_bytes, flags_in, rank, 0u, (size_t)n + 1, rocprim::plus<unsigned>(), stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&total, rank + n, 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = hipMalloc((void **)&table, ((size_t)total + 1) * (size_t)words * 8);
    if (e == hipSuccess) e = hipMemsetAsync(table, 0, (size_t)words * 8, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_cs_assign, dim3(g), dim3(256), 0, stream, (const u64 *)d_rows, (i64)n, words, (const unsigned *)slots,
                           (const unsigned *)rank, ids, table);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = e2;
    (void)hipFree(tmp);
    (void)hipFree(rank);
    (void)hipFree(flags);
    (void)hipFree(slots);
    if (e != hipSuccess) {
        (void)hipFree(ids);
        (void)hipFree(table);
        return e;
    }
    *d_ids = ids;
    *d_table = (unsigned long long *)table;
    *n_sets = (long long)total + 1;
    return hipSuccess;
}

// ---------------------------------------------------------------------------------------------
// ids + table -> matrix, counts, checks
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_cs_expand(const unsigned *__restrict__ ids, const u64 *__restrict__ table, i64 n, int words,
                                                   u64 *__restrict__ rows) {
    const i64 total = n * (i64)words;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < total; i += (i64)gridDim.x * 256) {
        const i64 j = i / words;
        rows[i] = table[(i64)ids[j] * words + (i - j * words)];
    }
}

__global__ void __launch_bounds__(256) k_cs_count(const unsigned *__restrict__ ids, i64 n, u64 *__restrict__ count) {
    u64 mine = 0;
    // (whole waves go round together: the bound is rounded up to the wave, and a lane past n sits the ballot out)
    for (i64 j0 = (i64)blockIdx.x * 256 + (threadIdx.x & ~63u); j0 < n; j0 += (i64)gridDim.x * 256) {
        const i64 j = j0 + (threadIdx.x & 63);
        mine += (u64)__popcll(__ballot(j < n && ids[j] != 0));
    }
    if (mine && (threadIdx.x & 63) == 0) atomicAdd(count, mine);
}

// report[0]: the smallest real column whose id is not below n_sets
__global__ void __launch_bounds__(256) k_cs_check_ids(unsigned *__restrict__ ids, i64 n, const unsigned char *__restrict__ lev,
                                                      u64 n_sets, u64 *__restrict__ report) {
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < n; j += (i64)gridDim.x * 256) {
        const unsigned id = ids[j];
        if (j == 0 || lev[j] != 0) {                         // (the root is a dummy whatever k is)
            if (id != 0) ids[j] = 0;
        } else if ((u64)id >= n_sets) {
            atomicMin(report, (u64)j);
        }
    }
}

// report[1]: (row << 8 | kind) of the first violation; a lane takes a table row; `keep` masks the last word
__global__ void __launch_bounds__(256) k_cs_check_table(const u64 *__restrict__ table, i64 n_sets, int words, u64 keep,
                                                        u64 *__restrict__ report) {
    for (i64 r = (i64)blockIdx.x * 256 + threadIdx.x; r < n_sets; r += (i64)gridDim.x * 256) {
        u64 any = 0;
        for (int w = 0; w < words; w++) any |= table[r * words + w];
        const u64 high = table[r * words + words - 1] & ~keep;
        const int kind = r == 0 && any ? SBWT_CS_ROW0_NOT_ZERO : r != 0 && !any ? SBWT_CS_ZERO_ROW : high ? SBWT_CS_HIGH_BIT : SBWT_CS_OK;
        if (kind != SBWT_CS_OK) atomicMin(report + 1, ((u64)r << 8) | (u64)kind);
    }
}

void sbwt_launch_cs_expand(const unsigned *d_ids, const unsigned long long *d_table, long long n, int words,
                           unsigned long long *d_rows, hipStream_t stream) {
    hipLaunchKernelGGL(k_cs_expand, dim3(cs_stride_grid(n * words)), dim3(256), 0, stream, d_ids, (const u64 *)d_table, (i64)n, words,
                       (u64 *)d_rows);
}

void sbwt_launch_cs_count(const unsigned *d_ids, long long n, unsigned long long *d_count, hipStream_t stream) {
    hipLaunchKernelGGL(k_cs_count, dim3(cs_stride_grid(n)), dim3(256), 0, stream, d_ids, (i64)n, (u64 *)d_count);
}

hipError_t sbwt_colorsets_validate(const SbwtIndexView &ix, unsigned *d_ids, const unsigned long long *d_table, long long n_sets,
                                   int n_colors, unsigned long long h_report[2], hipStream_t stream) {
    const bool mega = ix.n_mega > 1 || ix.force_mega;
    const i64 n = ix.n_nodes;
    const unsigned g = grid_for(n);
    unsigned char *lev = nullptr;
    u64 *report = nullptr;
    hipError_t e = hipMalloc((void **)&lev, (size_t)(n + 256));
    if (e == hipSuccess) e = hipMalloc((void **)&report, 16);
    if (e == hipSuccess) e = hipMemsetAsync(lev, 0, (size_t)(n + 256), stream);
    if (e == hipSuccess) e = hipMemsetAsync(report, 0xFF, 16, stream);
    if (e == hipSuccess) {
        for (int r = 0; r + 1 < ix.k; r++) {
            if (mega) hipLaunchKernelGGL(k_ut_level<true>, dim3(g), dim3(256), 0, stream, ix, lev, r);
            else hipLaunchKernelGGL(k_ut_level<false>, dim3(g), dim3(256), 0, stream, ix, lev, r);
        }
        const int words = (n_colors + 63) / 64;
        const u64 keep = (n_colors & 63) == 0 ? ~0ull : ((1ull << (n_colors & 63)) - 1ull);
        hipLaunchKernelGGL(k_cs_check_ids, dim3(cs_stride_grid(n)), dim3(256), 0, stream, d_ids, n, (const unsigned char *)lev,
                           (u64)n_sets, report);
        hipLaunchKernelGGL(k_cs_check_table, dim3(cs_stride_grid(n_sets)), dim3(256), 0, stream, (const u64 *)d_table, (i64)n_sets, words,
                           keep, report);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_report, report, 16, hipMemcpyDeviceToHost, stream);
    const hipError_t e2 = hipStreamSynchronize(stream);
    (void)hipFree(lev);
    (void)hipFree(report);
    return e != hipSuccess ? e : e2;
}

// ---------------------------------------------------------------------------------------------
// results + ids + table -> records
// ---------------------------------------------------------------------------------------------
// `cnt` (dynamic LDS): [4 waves][words - 1][64 lanes] int32, as in k_pa_reduce_wide: a lane reads and writes its own entries
// only, so the waves of a block need no barrier.
//
// The (key, n) pair goes into the counters: the row is table[x] | table[y] (x = 0: table[y]), `words` <= 64 words at a
// wave-uniform address, word w in lane w by one coalesced load; every non-zero word is broadcast and the lanes of its set bits
// add n.
__device__ __forceinline__ void cs_flush(const u64 *__restrict__ table, int words, u64 key, int n, int lane, int &count0, int *cnt) {
    const unsigned x = (unsigned)(key >> 32), y = (unsigned)key;
    u64 word = 0;
    if (lane < words) {
        word = table[(i64)y * words + lane];
        if (x) word |= table[(i64)x * words + lane];
    }
    u64 left = __ballot(word != 0);
    while (left) {
        const int w = __ffsll((i64)left) - 1;
        left &= left - 1;
        const u64 bits = (u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)word, w) |
                         ((u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(word >> 32), w) << 32);
        if ((bits >> lane) & 1ull) {
            if (w == 0) count0 += n;
            else cnt[(w - 1) * 64] += n;
        }
    }
}

template <bool TWO>
__global__ void __launch_bounds__(256) k_pa_reduce_sets(const int *__restrict__ res, const int *__restrict__ res2,
                                                        const i64 *__restrict__ out_off, i64 n_reads, const unsigned *__restrict__ ids,
                                                        const u64 *__restrict__ table, i64 n_nodes, unsigned n_sets, int words,
                                                        int n_colors, int ppm, int denominator, int2 *__restrict__ out,
                                                        u64 *__restrict__ colors, int *__restrict__ counts) {
    extern __shared__ int pa_sets_cnt[];
    const int lane = threadIdx.x & 63;
    int *cnt = pa_sets_cnt + (size_t)(threadIdx.x >> 6) * (size_t)(words - 1) * 64 + lane;        // [w - 1] at cnt[(w - 1) * 64]
    const i64 n_waves = (i64)gridDim.x * 4;
    const i64 W = out_off[n_reads];
    for (i64 r = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); r < n_reads; r += n_waves) {
        const i64 s = out_off[r];
        const i64 m = out_off[r + 1] - s;                 // (< 2^31: a read has fewer bases than that)
        int count0 = 0, found = 0;                        // lane c: count_c of word 0; every lane: n_found
        for (int w = 1; w < words; w++) cnt[(w - 1) * 64] = 0;
        u64 pend_key = 0;                                 // the pending run, the same in every lane; nothing pending: pend_n = 0
        int pend_n = 0;
        for (i64 q0 = 0; q0 < m; q0 += 64) {
            const i64 q = q0 + lane;
            unsigned x = 0, y = 0;                        // the key of this lane's window: x <= y, x = 0 when one id says it all
            if (q < m) {
                const i64 p = s + q;
                const i64 v = res[p];
                if (v >= 0 && v < n_nodes) y = ids[v];
                if (y >= n_sets) y = 0;
                if (TWO) {
                    const i64 v2 = res2[W - 1 - p];
                    if (v2 >= 0 && v2 < n_nodes) x = ids[v2];
                    if (x >= n_sets || x == y) x = 0;
                    if (x > y) { const unsigned t = x; x = y; y = t; }
                }
            }
            const u64 key = ((u64)x << 32) | (u64)y;      // found exactly when y != 0: no row is read for n_found
            u64 live = __ballot(y != 0);
            found += __popcll(live);
            while (live) {                                // one trip per distinct key of the iteration
                const int src = __ffsll((i64)live) - 1;
                const u64 k0 = (u64)(unsigned)__builtin_amdgcn_readlane((int)y, src) |
                               ((u64)(unsigned)__builtin_amdgcn_readlane((int)x, src) << 32);
                const u64 eq = __ballot(key == k0);
                live &= ~eq;
                if (pend_n != 0 && k0 == pend_key) {
                    pend_n += __popcll(eq);
                } else {
                    if (pend_n != 0) cs_flush(table, words, pend_key, pend_n, lane, count0, cnt);
                    pend_key = k0;
                    pend_n = __popcll(eq);
                }
            }
        }
        if (pend_n != 0) cs_flush(table, words, pend_key, pend_n, lane, count0, cnt);
        const i64 D = denominator ? m : (i64)found;
        u64 mine = 0;                                     // lane w: word w of the read's colours
        for (int w = 0; w < words; w++) {
            const int count = w == 0 ? count0 : cnt[(w - 1) * 64];
            const bool livec = w * 64 + lane < n_colors;
            const u64 b = __ballot(livec && D > 0 && (u64)count * 1000000ull >= (u64)ppm * (u64)D);
            if (lane == w) mine = b;
            if (counts && livec) __builtin_nontemporal_store(count, counts + r * n_colors + w * 64 + lane);
        }
        if (lane < words) __builtin_nontemporal_store(mine, colors + r * words + lane);
        if (lane == 0) out[r] = make_int2((int)m, found);
    }
}

void sbwt_launch_pa_reduce_sets(const int *d_res, const int *d_res2, const long long *d_out_off, long long n_reads,
                                const unsigned *d_ids, const unsigned long long *d_table, long long n_nodes, long long n_sets,
                                int words, int n_colors, int threshold_ppm, int denominator, SbwtReadFound *d_out,
                                unsigned long long *d_colors, int *d_counts, hipStream_t stream) {
    // a block's four waves take four reads per round
    const i64 gb = (n_reads + 3) / 4;
    const dim3 grid((unsigned)(gb < 1 ? 1 : gb > (1 << 20) ? (1 << 20) : gb)), block(256);
    const size_t lds = (size_t)4 * 64 * (size_t)(words - 1) * sizeof(int);      // at most 63 KiB (words <= 64)
    if (d_res2)
        hipLaunchKernelGGL((k_pa_reduce_sets<true>), grid, block, lds, stream, d_res, d_res2, d_out_off, (i64)n_reads, d_ids,
                           (const u64 *)d_table, (i64)n_nodes, (unsigned)n_sets, words, n_colors, threshold_ppm, denominator, (int2 *)d_out,
                           (u64 *)d_colors, d_counts);
    else
        hipLaunchKernelGGL((k_pa_reduce_sets<false>), grid, block, lds, stream, d_res, d_res2, d_out_off, (i64)n_reads, d_ids,
                           (const u64 *)d_table, (i64)n_nodes, (unsigned)n_sets, words, n_colors, threshold_ppm, denominator, (int2 *)d_out,
                           (u64 *)d_colors, d_counts);
}
