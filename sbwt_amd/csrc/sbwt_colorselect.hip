// sbwt_colorselect.hip -- k-mers selected by a predicate over their colour sets (include/sbwtgpu.h, "colour select"; DESIGN.md
// section 20).  The keys of the real columns come from sbwt_setops_keys with their columns; what leaves this file goes to the
// builder's tail like the result of a set operation: sorted distinct keys, no text, no sort.
//
//   k_csel_verdict<G>  table -> one byte per set.  G = the smallest power of two >= words lanes share a row: lane g of a group
//                   loads word g, the popcount of row & include and the flag of row & exclude are reduced over the group by
//                   xor-shuffles, the group's first lane tests the two bounds and stores the byte.  words = 1: a lane per
//                   row, 64 rows per wave; words = 64: a wave per row, 512 contiguous bytes per load instruction; a wave's
//                   loads are contiguous for every words in between (its 64 / G rows follow each other; the lanes past
//                   words in each group load nothing).
//   (k_gm_sizes)    ids -> size[t], the histogram of sbwt_colormatrix.hip
//   k_csel_tally    verdicts and sizes -> the coloured columns, the coloured selected columns, keep[t] = set t >= 1 matches and
//                   is carried, and the number of such sets; sums per wave by xor-shuffles, one atomic per wave and counter
//   (rocPRIM, k_csel_rows, sbwt_colorsets_compress)  only when more than one non-empty set is kept: their numbers
//                   selected in order, their rows gathered, and the rows deduplicated by content -- an uploaded object may
//                   hold a row twice, and the count is one of what the object means
//   k_csel_flags    flag[i] = verdict[ids[cols[i]]], every index guarded; the flags are counted per wave, so that the host
//                   knows the output's size before anything is written to it
//   (rocPRIM)       select of the keys by flag: order-preserving, 8- or 16-byte keys
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include "sbwt_kernels_common.h"
#include "sbwt_colormatrix.h"
#include "sbwt_colorsets.h"
#include "sbwt_colorselect.h"

typedef __uint128_t u128;

// grid for a grid-stride loop over n work-items: enough blocks to fill the chip, no more
static inline unsigned csel_stride_grid(i64 n) {
    const i64 g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : g > 2048 ? 2048 : g);
}

template <int G>
__global__ void __launch_bounds__(256) k_csel_verdict(const u64 *__restrict__ table, i64 n_sets, int words, const u64 *__restrict__ masks,
                                                      int min_in, int max_in, unsigned char *__restrict__ verdict) {
    const int g = threadIdx.x & (G - 1);
    const u64 inc = g < words ? masks[g] : 0, exc = g < words ? masks[words + g] : 0;
    // (whole waves go round together: the bound is rounded up to the block's rows, and a lane without a word adds nothing)
    const i64 rows_per_block = 256 / G;
    for (i64 t0 = (i64)blockIdx.x * rows_per_block; t0 < n_sets; t0 += (i64)gridDim.x * rows_per_block) {
        const i64 t = t0 + threadIdx.x / G;
        const u64 x = (t < n_sets && g < words) ? table[t * (i64)words + g] : 0;
        int pop = __popcll(x & inc);
        int bad = (x & exc) != 0 ? 1 : 0;
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) {
            pop += __shfl_xor(pop, off);
            bad |= __shfl_xor(bad, off);
        }
        if (t < n_sets && g == 0) verdict[t] = (!bad && pop >= min_in && pop <= max_in) ? 1 : 0;
    }
}

void sbwt_launch_csel_verdict(const unsigned long long *d_table, long long n_sets, int words, const unsigned long long *d_masks,
                              int min_in, int max_in, unsigned char *d_verdict, hipStream_t stream) {
#define CSEL_VERDICT(G)                                                                                                              \
    hipLaunchKernelGGL(k_csel_verdict<G>, dim3(csel_stride_grid((i64)n_sets * G)), dim3(256), 0, stream, (const u64 *)d_table, (i64)n_sets, \
                       words, (const u64 *)d_masks, min_in, max_in, d_verdict)
    if (words <= 1) CSEL_VERDICT(1);
    else if (words <= 2) CSEL_VERDICT(2);
    else if (words <= 4) CSEL_VERDICT(4);
    else if (words <= 8) CSEL_VERDICT(8);
    else if (words <= 16) CSEL_VERDICT(16);
    else if (words <= 32) CSEL_VERDICT(32);
    else CSEL_VERDICT(64);
#undef CSEL_VERDICT
}

// acc[0] += the columns with a set t >= 1, acc[1] += those whose set matches, acc[2] += the sets t >= 1 that match and have a column
__global__ void __launch_bounds__(256) k_csel_tally(const unsigned char *__restrict__ verdict, const unsigned *__restrict__ sizes, i64 n_sets,
                                                    unsigned char *__restrict__ keep, u64 *__restrict__ acc) {
    u64 colored = 0, sel = 0, kept = 0;
    for (i64 t0 = (i64)blockIdx.x * 256 + (threadIdx.x & ~63u); t0 < n_sets; t0 += (i64)gridDim.x * 256) {
        const i64 t = t0 + (threadIdx.x & 63);
        const bool on = t < n_sets && t != 0;
        const u64 sz = on ? sizes[t] : 0;
        const bool v = on && verdict[t] != 0;
        colored += sz;
        sel += v ? sz : 0;
        const bool kp = v && sz != 0;
        if (t < n_sets) keep[t] = kp ? 1 : 0;
        kept += (u64)__popcll(__ballot(kp));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        colored += (u64)__shfl_xor((long long)colored, off);
        sel += (u64)__shfl_xor((long long)sel, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (colored) atomicAdd(acc + 0, colored);
        if (sel) atomicAdd(acc + 1, sel);
        if (kept) atomicAdd(acc + 2, kept);
    }
}

// rows[r * words + w] = table[list[r] * words + w] for r < m
__global__ void __launch_bounds__(256) k_csel_rows(const unsigned *__restrict__ list, i64 m, const u64 *__restrict__ table, i64 n_sets, int words,
                                                   u64 *__restrict__ rows) {
    const i64 total = m * (i64)words;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < total; i += (i64)gridDim.x * 256) {
        const i64 r = i / words;
        const u64 t = list[r];
        rows[i] = t < (u64)n_sets ? table[(i64)t * words + (i - r * words)] : 0;
    }
}

__global__ void __launch_bounds__(256) k_csel_flags(const unsigned *__restrict__ cols, i64 n_keys, const unsigned *__restrict__ ids, i64 n_nodes,
                                                    const unsigned char *__restrict__ verdict, i64 n_sets, unsigned char *__restrict__ flags,
                                                    u64 *__restrict__ n_flagged) {
    u64 mine = 0;
    for (i64 i0 = (i64)blockIdx.x * 256 + (threadIdx.x & ~63u); i0 < n_keys; i0 += (i64)gridDim.x * 256) {
        const i64 i = i0 + (threadIdx.x & 63);
        bool f = false;
        if (i < n_keys) {
            const u64 c = cols[i];
            if (c < (u64)n_nodes) {
                const u64 id = ids[c];
                if (id < (u64)n_sets) f = verdict[id] != 0;
            }
            flags[i] = f ? 1 : 0;
        }
        mine += (u64)__popcll(__ballot(f));
    }
    if (mine && (threadIdx.x & 63) == 0) atomicAdd(n_flagged, mine);
}

#define CSEL_TRY(expr)                    \
    do {                                  \
        e = (expr);                       \
        if (e != hipSuccess) goto done;   \
    } while (0)

template <typename KT>
static hipError_t colorselect_t(const unsigned *d_ids, i64 n_nodes, const u64 *d_table, i64 n_sets, int words, const u64 *d_masks, int min_in,
                                int max_in, const KT *d_keys, const unsigned *d_cols, i64 n_keys, void **d_out, SbwtCselCounts *counts,
                                hipStream_t stream) {
    hipError_t e = hipSuccess;
    unsigned char *verdict = nullptr, *keep = nullptr, *flags = nullptr;
    unsigned *sizes = nullptr, *list = nullptr, *cids = nullptr;
    u64 *acc = nullptr, *rows = nullptr, *ctable = nullptr;          // acc: coloured, selected coloured, kept sets, flagged keys, selected count
    KT *out = nullptr;
    void *tmp = nullptr;
    size_t tmp_bytes = 0;
    u64 h_acc[5] = {0, 0, 0, 0, 0};
    unsigned char v0 = 0;
    i64 real0 = 0, n_sel = 0, n_kept = 0, distinct = 0;
    *counts = SbwtCselCounts();
    if (d_out) *d_out = nullptr;
    CSEL_TRY(hipMalloc((void **)&verdict, (size_t)n_sets));
    CSEL_TRY(hipMalloc((void **)&keep, (size_t)n_sets));
    CSEL_TRY(hipMalloc((void **)&sizes, (size_t)n_sets * 4));
    CSEL_TRY(hipMalloc((void **)&acc, sizeof(h_acc)));
    CSEL_TRY(hipMemsetAsync(acc, 0, sizeof(h_acc), stream));
    sbwt_launch_csel_verdict(d_table, n_sets, words, d_masks, min_in, max_in, verdict, stream);
    sbwt_launch_gm_sizes(d_ids, n_nodes, n_sets, sizes, stream);
    hipLaunchKernelGGL(k_csel_tally, dim3(csel_stride_grid(n_sets)), dim3(256), 0, stream, (const unsigned char *)verdict,
                       (const unsigned *)sizes, n_sets, keep, acc);
    CSEL_TRY(hipGetLastError());
    CSEL_TRY(hipMemcpyAsync(h_acc, acc, sizeof(h_acc), hipMemcpyDeviceToHost, stream));
    CSEL_TRY(hipMemcpyAsync(&v0, verdict, 1, hipMemcpyDeviceToHost, stream));
    CSEL_TRY(hipStreamSynchronize(stream));
    // size[0] holds the dummy columns too: the uncoloured REAL columns are the keys that no set t >= 1 accounts for
    real0 = n_keys - (i64)h_acc[0];
    if (real0 < 0) { e = hipErrorUnknown; goto done; }
    n_sel = (i64)h_acc[1] + (v0 ? real0 : 0);
    n_kept = (i64)h_acc[2];
    distinct = n_kept;
    if (n_kept > 1) {
        CSEL_TRY(hipMalloc((void **)&list, (size_t)n_kept * 4));
        CSEL_TRY(hipMalloc((void **)&rows, (size_t)n_kept * (size_t)words * 8));
        CSEL_TRY(rocprim::select(nullptr, tmp_bytes, rocprim::counting_iterator<unsigned>(0), (const unsigned char *)keep, list, acc + 4,
                                 (size_t)n_sets, stream));
        CSEL_TRY(hipMalloc(&tmp, tmp_bytes + 16));
        CSEL_TRY(rocprim::select(tmp, tmp_bytes, rocprim::counting_iterator<unsigned>(0), (const unsigned char *)keep, list, acc + 4,
                                 (size_t)n_sets, stream));
        hipLaunchKernelGGL(k_csel_rows, dim3(csel_stride_grid(n_kept * (i64)words)), dim3(256), 0, stream, (const unsigned *)list, n_kept,
                           d_table, n_sets, words, rows);
        CSEL_TRY(hipGetLastError());
        long long ns = 0;
        CSEL_TRY(sbwt_colorsets_compress(rows, n_kept, words, &cids, (unsigned long long **)&ctable, &ns, stream));
        distinct = ns - 1;
        (void)hipFree(tmp);
        tmp = nullptr;
    }
    if (d_out) {
        CSEL_TRY(hipMalloc((void **)&flags, (size_t)(n_keys ? n_keys : 1)));
        CSEL_TRY(hipMalloc((void **)&out, (size_t)(n_sel ? n_sel : 1) * sizeof(KT)));
        if (n_keys > 0) {
            hipLaunchKernelGGL(k_csel_flags, dim3(csel_stride_grid(n_keys)), dim3(256), 0, stream, d_cols, n_keys, d_ids, n_nodes,
                               (const unsigned char *)verdict, n_sets, flags, acc + 3);
            CSEL_TRY(hipGetLastError());
            CSEL_TRY(hipMemcpyAsync(h_acc + 3, acc + 3, 8, hipMemcpyDeviceToHost, stream));
            CSEL_TRY(hipStreamSynchronize(stream));
            // the output holds n_sel keys: nothing is written to it unless the flags say the same number
            if ((i64)h_acc[3] != n_sel) { e = hipErrorUnknown; goto done; }
            CSEL_TRY(rocprim::select(nullptr, tmp_bytes, d_keys, (const unsigned char *)flags, out, acc + 4, (size_t)n_keys, stream));
            CSEL_TRY(hipMalloc(&tmp, tmp_bytes + 16));
            CSEL_TRY(rocprim::select(tmp, tmp_bytes, d_keys, (const unsigned char *)flags, out, acc + 4, (size_t)n_keys, stream));
            CSEL_TRY(hipStreamSynchronize(stream));
        } else if (n_sel != 0) {
            e = hipErrorUnknown;
            goto done;
        }
        *d_out = out;
        out = nullptr;
    }
    counts->n_real = n_keys;
    counts->n_selected = n_sel;
    counts->n_sets_matched = distinct + ((v0 && real0 > 0) ? 1 : 0);
done:
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(stream);
        (void)hipGetLastError();
    }
    (void)hipFree(verdict); (void)hipFree(keep); (void)hipFree(flags); (void)hipFree(sizes); (void)hipFree(list); (void)hipFree(cids);
    (void)hipFree(acc); (void)hipFree(rows); (void)hipFree(ctable); (void)hipFree(tmp); (void)hipFree(out);
    return e;
}

hipError_t sbwt_colorselect(const unsigned *d_ids, long long n_nodes, const unsigned long long *d_table, long long n_sets, int words,
                            const unsigned long long *d_masks, int min_in, int max_in, const void *d_keys, const unsigned *d_cols,
                            long long n_keys, int key_bytes, void **d_out, SbwtCselCounts *counts, hipStream_t stream) {
    return key_bytes == 8 ? colorselect_t<u64>(d_ids, n_nodes, (const u64 *)d_table, n_sets, words, (const u64 *)d_masks, min_in, max_in,
                                               static_cast<const u64 *>(d_keys), d_cols, n_keys, d_out, counts, stream)
                          : colorselect_t<u128>(d_ids, n_nodes, (const u64 *)d_table, n_sets, words, (const u64 *)d_masks, min_in, max_in,
                                                static_cast<const u128 *>(d_keys), d_cols, n_keys, d_out, counts, stream);
}
