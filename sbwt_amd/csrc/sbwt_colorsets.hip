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

// ---------------------------------------------------------------------------------------------
// the builder: colour sets made one colour at a time, without the wide matrix
// ---------------------------------------------------------------------------------------------
// State (SbwtCsbState): ids[n], table[cap x words] with row 0 zero, cnt[cap] = the columns that carry each id, and a mark
// bitmap of one bit per column, 64 columns a word.  A colour is marked into the bitmap by any number of searches and then
// CLOSED: every marked column's set becomes its old set + the colour.  A closed colour is in no row of the table, so
//   k_csb_count   bitmap -> hit[old id] = the marked columns that carry it.  A wave takes a bitmap word, lane l its column
//                 64 w + l; ids are gathered for set bits only and the distinct ids of the word are peeled as k_pa_reduce_sets
//                 peels keys (readlane, ballot, popcount): one add per distinct id and word, into the block's LDS counters
//                 for ids below CSB_LDS_IDS -- a strain's millions of columns share a handful of ids, which would otherwise
//                 all meet at a few addresses in L2 -- and into `hit` directly above that.
//   k_csb_plan    a lane per old id: hit == cnt and id != 0 -> every column of the set moves: the colour's bit is set in the
//                 row in place and hit becomes 0 ("stays"); any other hit != 0 -> the set splits, counted in ctr[1].
//                 The host reads ctr and grows table and cnt when old sets + splits pass the capacity.
//   k_csb_assign  a lane per old id that splits: a new id from an atomic counter (any order: finish fixes the numbering),
//                 cnt[new] = hit, cnt[old] -= hit, hit[old] = the new id -- the array now is the remap, 0 = stays.
//   k_csb_rows    grid-stride over old sets x words: table[new] = table[old] | the colour's bit
//   k_csb_move    bitmap -> ids: marked columns of split sets take remap[id]; the word is cleared
// The table's rows stay pairwise distinct and every row but 0 stays in use: new rows hold the colour and surviving old rows
// do not, distinct old rows give distinct new ones, and a row that would become unused is the one changed in place.
//   finish:  k_csb_first (atomicMin of the columns that carry each id, the atomic skipped when it would not lower it; ids below
//            CSB_LDS_IDS in the block's LDS first),
//            k_csb_flag, rocPRIM's exclusive scan over the n flags, k_csb_renumber, k_csb_permute -- compress's flag / scan /
//            assign passes over again, so the result is the canonical form.
#define CSB_LDS_IDS 1024

// grid for a loop in which a wave takes one bitmap word per round
static inline unsigned csb_word_grid(i64 n_words) {
    const i64 g = (n_words + 3) / 4;
    return (unsigned)(g < 1 ? 1 : g > 2048 ? 2048 : g);
}

// k_col_mark with a bit per column for a row of words: the same window count
__global__ void __launch_bounds__(256) k_csb_mark(const int *__restrict__ res, const int *__restrict__ other,
                                                  const i64 *__restrict__ out_off, i64 n_reads, u64 *marks, i64 n_nodes, int count,
                                                  SbwtPaHeader *__restrict__ hdr) {
    const i64 W = out_off[n_reads];
    u64 mine = 0;                                          // windows with a hit, of this lane's wave (kept by its lane 0)
    for (i64 i0 = (i64)blockIdx.x * 256 + (threadIdx.x & ~63u); i0 < W; i0 += (i64)gridDim.x * 256) {
        const i64 i = i0 + (threadIdx.x & 63);
        bool hit = false;
        if (i < W) {
            const i64 v = res[i];
            if (v >= 0 && v < n_nodes) {
                hit = true;
                const u64 bit = 1ull << (v & 63);
                u64 *word = marks + (v >> 6);
                if (!(*word & bit)) atomicOr(word, bit);
            }
            if (count && !hit && other) hit = other[W - 1 - i] >= 0;
        }
        if (count) mine += (u64)__popcll(__ballot(hit));
    }
    if (count && mine && (threadIdx.x & 63) == 0) atomicAdd(&hdr->n_hit, mine);
}

// ctr[0] += the marked columns
__global__ void __launch_bounds__(256) k_csb_count(const u64 *__restrict__ marks, i64 n_words, i64 n, const unsigned *__restrict__ ids,
                                                   unsigned n_sets, unsigned *__restrict__ hit, u64 *__restrict__ ctr) {
    __shared__ unsigned lds_hit[CSB_LDS_IDS];
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < CSB_LDS_IDS; i += 256) lds_hit[i] = 0;
    __syncthreads();
    u64 mine = 0;
    for (i64 w = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); w < n_words; w += (i64)gridDim.x * 4) {
        const u64 bits = marks[w];                         // (the same address, and so the same value, in every lane)
        if (!bits) continue;
        const i64 j = w * 64 + lane;
        const bool on = ((bits >> lane) & 1ull) && j < n;
        unsigned id = on ? ids[j] : 0;
        if (id >= n_sets) id = 0;                          // (never: ids stay below n_sets)
        u64 live = __ballot(on);
        mine += (u64)__popcll(live);
        while (live) {                                     // one trip per distinct id of the word
            const int src = __ffsll((i64)live) - 1;
            const unsigned k0 = (unsigned)__builtin_amdgcn_readlane((int)id, src);
            const u64 eq = __ballot(on && id == k0);
            live &= ~eq;
            if (lane == 0) {
                if (k0 < CSB_LDS_IDS) atomicAdd(lds_hit + k0, (unsigned)__popcll(eq));
                else atomicAdd(hit + k0, (unsigned)__popcll(eq));
            }
        }
    }
    if (mine && lane == 0) atomicAdd(ctr, mine);
    __syncthreads();
    for (unsigned i = threadIdx.x; i < CSB_LDS_IDS && i < n_sets; i += 256) {
        const unsigned v = lds_hit[i];
        if (v) atomicAdd(hit + i, v);
    }
}

// ctr[1] += the sets that split; ctr[2] = hit[0], the columns that were not coloured and now are
__global__ void __launch_bounds__(256) k_csb_plan(unsigned *__restrict__ hit, const unsigned *__restrict__ cnt, unsigned n_sets,
                                                  u64 *__restrict__ table, int words, int color, u64 *__restrict__ ctr) {
    u64 mine = 0;
    for (unsigned r0 = blockIdx.x * 256 + (threadIdx.x & ~63u); r0 < n_sets; r0 += gridDim.x * 256) {
        const unsigned r = r0 + (threadIdx.x & 63);
        bool split = false;
        if (r < n_sets) {
            const unsigned h = hit[r];
            if (r == 0) ctr[2] = h;
            if (h != 0 && r != 0 && h == cnt[r]) {
                table[(i64)r * words + (color >> 6)] |= 1ull << (color & 63);
                hit[r] = 0;
            } else {
                split = h != 0;
            }
        }
        mine += (u64)__popcll(__ballot(split));
    }
    if (mine && (threadIdx.x & 63) == 0) atomicAdd(ctr + 1, mine);
}

// ctr[3]: the new ids handed out so far
__global__ void __launch_bounds__(256) k_csb_assign(unsigned *__restrict__ hit, unsigned *__restrict__ cnt, unsigned n_sets,
                                                    u64 *__restrict__ ctr) {
    for (unsigned r = blockIdx.x * 256 + threadIdx.x; r < n_sets; r += gridDim.x * 256) {
        const unsigned h = hit[r];
        if (h == 0) continue;
        const unsigned fresh = n_sets + (unsigned)atomicAdd(ctr + 3, 1ull);
        cnt[fresh] = h;
        cnt[r] -= h;
        hit[r] = fresh;
    }
}

__global__ void __launch_bounds__(256) k_csb_rows(const unsigned *__restrict__ remap, unsigned n_sets, u64 *table, int words, int color) {
    const i64 total = (i64)n_sets * words;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < total; i += (i64)gridDim.x * 256) {
        const i64 r = i / words;
        const int w = (int)(i - r * words);
        const unsigned fresh = remap[r];
        if (fresh) table[(i64)fresh * words + w] = table[i] | (w == (color >> 6) ? 1ull << (color & 63) : 0ull);
    }
}

__global__ void __launch_bounds__(256) k_csb_move(u64 *__restrict__ marks, i64 n_words, i64 n, unsigned *__restrict__ ids,
                                                  const unsigned *__restrict__ remap, unsigned n_sets) {
    const int lane = threadIdx.x & 63;
    for (i64 w = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); w < n_words; w += (i64)gridDim.x * 4) {
        const u64 bits = marks[w];
        if (!bits) continue;                               // (the same in every lane)
        const i64 j = w * 64 + lane;
        if (((bits >> lane) & 1ull) && j < n) {
            const unsigned id = ids[j];
            const unsigned fresh = id < n_sets ? remap[id] : 0;
            if (fresh) ids[j] = fresh;
        }
        if (lane == 0) marks[w] = 0;
    }
}

// first[id] = the smallest column that carries id (first[] starts as CS_EMPTY).  Columns come to a block in ascending order, so
// a minimum is loaded first and the atomic skipped when it would not lower it: after a block's first round nearly all skip.
// Ids below CSB_LDS_IDS meet in the block's LDS and reach `first` once per block and id -- the few sets that millions of
// columns share would otherwise send every wave of the first round to the same few addresses in L2.
__global__ void __launch_bounds__(256) k_csb_first(const unsigned *__restrict__ ids, i64 n, unsigned n_sets, unsigned *first) {
    __shared__ unsigned lds_min[CSB_LDS_IDS];
    for (int i = threadIdx.x; i < CSB_LDS_IDS; i += 256) lds_min[i] = CS_EMPTY;
    __syncthreads();
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < n; j += (i64)gridDim.x * 256) {
        const unsigned id = ids[j];
        if (id == 0 || id >= n_sets) continue;
        if (id < CSB_LDS_IDS) {
            if ((unsigned)j < lds_min[id]) atomicMin(lds_min + id, (unsigned)j);
        } else if ((unsigned)j < first[id]) {
            atomicMin(first + id, (unsigned)j);
        }
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < CSB_LDS_IDS && i < n_sets; i += 256) {
        const unsigned v = lds_min[i];
        if (v != CS_EMPTY && v < first[i]) atomicMin(first + i, v);
    }
}

__global__ void __launch_bounds__(256) k_csb_flag(const unsigned *__restrict__ first, unsigned n_sets, i64 n, unsigned char *__restrict__ flags) {
    for (unsigned r = 1 + blockIdx.x * 256 + threadIdx.x; r < n_sets; r += gridDim.x * 256) {
        const unsigned f = first[r];
        if ((i64)f < n) flags[f] = 1;
    }
}

__global__ void __launch_bounds__(256) k_csb_renumber(unsigned *__restrict__ ids, i64 n, unsigned n_sets, const unsigned *__restrict__ first,
                                                      const unsigned *__restrict__ rank) {
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < n; j += (i64)gridDim.x * 256) {
        const unsigned id = ids[j];
        if (id == 0) continue;
        const unsigned f = id < n_sets ? first[id] : CS_EMPTY;
        ids[j] = (i64)f < n ? 1u + rank[f] : 0u;
    }
}

__global__ void __launch_bounds__(256) k_csb_permute(const u64 *__restrict__ table, unsigned n_sets, int words, i64 n,
                                                     const unsigned *__restrict__ first, const unsigned *__restrict__ rank,
                                                     u64 *__restrict__ out) {
    const i64 total = (i64)n_sets * words;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < total; i += (i64)gridDim.x * 256) {
        const i64 r = i / words;
        if (r == 0) { out[i] = 0; continue; }
        const unsigned f = first[r];
        if ((i64)f < n) out[(i64)(1u + rank[f]) * words + (i - r * words)] = table[i];
    }
}

void sbwt_launch_csb_mark(const int *d_res, const int *d_other, const long long *d_out_off, long long n_reads, long long max_results,
                          unsigned long long *d_marks, long long n_nodes, int count, SbwtPaHeader *hdr, hipStream_t stream) {
    hipLaunchKernelGGL(k_csb_mark, dim3(cs_stride_grid(max_results)), dim3(256), 0, stream, d_res, d_other, d_out_off, (i64)n_reads,
                       (u64 *)d_marks, (i64)n_nodes, count, hdr);
}

static inline i64 csb_mark_words(i64 n) { return (n + 63) / 64; }

long long sbwt_csb_device_bytes(const SbwtCsbState *b) {
    if (!b->d_ids) return 0;
    return b->n * 4 + csb_mark_words(b->n) * 8 + b->cap * ((i64)b->words * 8 + 4);
}

void sbwt_csb_free(SbwtCsbState *b) {
    (void)hipFree(b->d_ids);
    (void)hipFree(b->d_table);
    (void)hipFree(b->d_cnt);
    (void)hipFree(b->d_marks);
    b->d_ids = b->d_cnt = nullptr;
    b->d_table = b->d_marks = nullptr;
    b->cap = 0;
}

hipError_t sbwt_csb_init(SbwtCsbState *b, long long n, int words, hipStream_t stream) {
    b->n = n;
    b->words = words;
    b->cap = SBWT_CSB_FIRST_CAPACITY;
    b->n_sets = 1;
    b->n_colored = 0;
    b->d_ids = b->d_cnt = nullptr;
    b->d_table = b->d_marks = nullptr;
    const size_t mark_bytes = (size_t)csb_mark_words(n) * 8, table_bytes = (size_t)b->cap * (size_t)words * 8;
    const unsigned all = (unsigned)n;
    hipError_t e = hipMalloc((void **)&b->d_ids, (size_t)n * 4 + 16);
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_marks, mark_bytes + 16);
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_table, table_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_cnt, (size_t)b->cap * 4);
    if (e == hipSuccess) e = hipMemsetAsync(b->d_ids, 0, (size_t)n * 4 + 16, stream);
    if (e == hipSuccess) e = hipMemsetAsync(b->d_marks, 0, mark_bytes + 16, stream);
    if (e == hipSuccess) e = hipMemsetAsync(b->d_table, 0, table_bytes, stream);
    if (e == hipSuccess) e = hipMemsetAsync(b->d_cnt, 0, (size_t)b->cap * 4, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b->d_cnt, &all, 4, hipMemcpyHostToDevice, stream);
    const hipError_t e2 = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) sbwt_csb_free(b);
    return e;
}

// table and cnt of at least `need` rows: the capacity doubles, the rows in use are copied on the device
static hipError_t csb_grow(SbwtCsbState *b, i64 need, hipStream_t stream) {
    i64 cap = b->cap;
    while (cap < need) cap *= 2;
    if (cap == b->cap) return hipSuccess;
    u64 *table = nullptr;
    unsigned *cnt = nullptr;
    const size_t row = (size_t)b->words * 8;
    hipError_t e = hipMalloc((void **)&table, (size_t)cap * row);
    if (e == hipSuccess) e = hipMalloc((void **)&cnt, (size_t)cap * 4);
    if (e == hipSuccess) e = hipMemcpyAsync(table, b->d_table, (size_t)b->n_sets * row, hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(cnt, b->d_cnt, (size_t)b->n_sets * 4, hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipMemsetAsync(cnt + b->n_sets, 0, (size_t)(cap - b->n_sets) * 4, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
        (void)hipFree(table);
        (void)hipFree(cnt);
        return e;
    }
    (void)hipFree(b->d_table);
    (void)hipFree(b->d_cnt);
    b->d_table = (unsigned long long *)table;
    b->d_cnt = cnt;
    b->cap = cap;
    return hipSuccess;
}

hipError_t sbwt_csb_close(SbwtCsbState *b, int color, long long *n_marked, hipStream_t stream) {
    const i64 n_words = csb_mark_words(b->n);
    const unsigned old = (unsigned)b->n_sets;
    const unsigned gw = csb_word_grid(n_words), gs = cs_stride_grid((i64)old);
    unsigned *hit = nullptr;                                // hit, then remap: one uint32 per old set; the four counters behind
    u64 h_ctr[4] = {0, 0, 0, 0};
    *n_marked = 0;
    const size_t hit_bytes = ((size_t)old * 4 + 15) & ~(size_t)15;
    hipError_t e = hipMalloc((void **)&hit, hit_bytes + 32);
    u64 *ctr = reinterpret_cast<u64 *>(reinterpret_cast<char *>(hit) + hit_bytes);
    if (e == hipSuccess) e = hipMemsetAsync(hit, 0, hit_bytes + 32, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_csb_count, dim3(gw), dim3(256), 0, stream, (const u64 *)b->d_marks, n_words, (i64)b->n,
                           (const unsigned *)b->d_ids, old, hit, ctr);
        hipLaunchKernelGGL(k_csb_plan, dim3(gs), dim3(256), 0, stream, hit, (const unsigned *)b->d_cnt, old, (u64 *)b->d_table, b->words,
                           color, ctr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_ctr, ctr, 32, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    const i64 fresh = (i64)h_ctr[1];
    if (e == hipSuccess && fresh > 0 && (i64)old + fresh > (i64)0xFFFFFFFFll) e = hipErrorOutOfMemory;          // (ids are uint32)
    if (e == hipSuccess && fresh > 0) e = csb_grow(b, (i64)old + fresh, stream);
    if (e == hipSuccess && h_ctr[0] != 0) {
        if (fresh > 0) {
            hipLaunchKernelGGL(k_csb_assign, dim3(gs), dim3(256), 0, stream, hit, b->d_cnt, old, ctr);
            hipLaunchKernelGGL(k_csb_rows, dim3(cs_stride_grid((i64)old * b->words)), dim3(256), 0, stream, (const unsigned *)hit, old,
                               (u64 *)b->d_table, b->words, color);
        }
        hipLaunchKernelGGL(k_csb_move, dim3(gw), dim3(256), 0, stream, (u64 *)b->d_marks, n_words, (i64)b->n, b->d_ids,
                           (const unsigned *)hit, old);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = e2;
    (void)hipFree(hit);
    if (e != hipSuccess) return e;
    b->n_sets = (i64)old + fresh;
    b->n_colored += (i64)h_ctr[2];
    *n_marked = (long long)h_ctr[0];
    return hipSuccess;
}

hipError_t sbwt_csb_finish(SbwtCsbState *b, unsigned **d_ids, unsigned long long **d_table, long long *n_sets, hipStream_t stream) {
    const i64 n = b->n;
    const unsigned sets = (unsigned)b->n_sets;
    unsigned *first = nullptr, *rank = nullptr;
    unsigned char *flags = nullptr;
    void *tmp = nullptr;
    u64 *table = nullptr;
    size_t tmp_bytes = 0;
    unsigned total = 0;
    *d_ids = nullptr;
    *d_table = nullptr;
    *n_sets = 0;
    const unsigned g = cs_stride_grid(n), gs = cs_stride_grid((i64)sets);
    hipError_t e = hipMalloc((void **)&first, (size_t)sets * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&flags, (size_t)n + 1);
    if (e == hipSuccess) e = hipMalloc((void **)&rank, ((size_t)n + 1) * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&table, (size_t)sets * (size_t)b->words * 8);
    const auto flags_in = rocprim::make_transform_iterator((const unsigned char *)flags, CsByteToU32());
    if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, tmp_bytes, flags_in, rank, 0u, (size_t)n + 1, rocprim::plus<unsigned>(), stream);
    if (e == hipSuccess) e = hipMalloc(&tmp, tmp_bytes + 16);
    if (e == hipSuccess) e = hipMemsetAsync(first, 0xFF, (size_t)sets * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(flags, 0, (size_t)n + 1, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_csb_first, dim3(g > 2048 ? 2048 : g), dim3(256), 0, stream, (const unsigned *)b->d_ids, n, sets, first);
        hipLaunchKernelGGL(k_csb_flag, dim3(gs), dim3(256), 0, stream, (const unsigned *)first, sets, n, flags);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = rocprim::exclusive_scan(tmp, tmp_bytes, flags_in, rank, 0u, (size_t)n + 1, rocprim::plus<unsigned>(), stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&total, rank + n, 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_csb_renumber, dim3(g), dim3(256), 0, stream, b->d_ids, n, sets, (const unsigned *)first, (const unsigned *)rank);
        hipLaunchKernelGGL(k_csb_permute, dim3(cs_stride_grid((i64)sets * b->words)), dim3(256), 0, stream, (const u64 *)b->d_table, sets,
                           b->words, n, (const unsigned *)first, (const unsigned *)rank, table);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = e2;
    if (e == hipSuccess && total + 1u != sets) e = hipErrorAssert;          // (every row but 0 is in use: never)
    (void)hipFree(tmp);
    (void)hipFree(rank);
    (void)hipFree(flags);
    (void)hipFree(first);
    if (e != hipSuccess) {
        (void)hipFree(table);
        return e;
    }
    *d_ids = b->d_ids;
    *d_table = (unsigned long long *)table;
    *n_sets = (long long)sets;
    b->d_ids = nullptr;
    sbwt_csb_free(b);
    return hipSuccess;
}
