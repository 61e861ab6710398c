// sbwt_colormerge.hip -- colour sets carried onto another index (include/sbwtgpu.h, "colour sets carried onto another index";
// DESIGN.md section 17).  Index u gets, for every real column with k-mer x, the set S_a(x) | S_b(x) << color_offset_b, where
// S_a and S_b are what two colour-set objects of two other indexes say about x -- no sequence is read, no wide matrix made.
//
//   keys        sbwt_setops_keys of u, a and b: the sorted distinct keys of the real columns, each with its column
//   k_cm_locate a lane per key of u: lower-bound binary search of the key in a's keys and in b's; on a match the id of that
//               column is gathered.  Out comes one 64-bit pair (id_a << 32 | id_b) per key of u; the keys found in a, in b and
//               in both are counted by ballot and popcount, one atomic per wave and counter.
//   pairs       the pairs are a matrix of one word per row, so sbwt_colorsets_compress IS the pass that finds the distinct
//               ones (k_cs_insert: the pair itself is compared, never its hash; atomicMin on the representative with the load
//               first; the pair (0, 0) never touches the table): every key gets its pair's number, and the distinct pairs lie
//               in a table, numbered by the smallest key -- that is, column -- of u that carries them.
//   k_cm_rows   grid-stride over distinct pairs x words_out: row[w] = ta[id_a][w] | tb[id_b] shifted up by the offset
//   rows        different pairs may give one row (shared colour spaces, duplicate rows in an uploaded input), so the pairs'
//               rows go through sbwt_colorsets_compress once more.  It numbers the row classes by their smallest pair, pairs
//               are numbered by their smallest column, so the classes come out in the order of their smallest columns: its
//               table is the canonical table of the result as it stands.
//   k_cm_scatter  ids[column of key i] = class[pair[i]] into a zero-filled array: dummy columns keep 0
#include "sbwt_kernels_common.h"
#include "sbwt_setops.h"
#include "sbwt_colorsets.h"
#include "sbwt_colormerge.h"
#include <chrono>

typedef __uint128_t u128;

static inline unsigned cm_stride_grid(i64 n) {
    const i64 g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : g > 8192 ? 8192 : g);
}

// the smallest position whose key is not below x (n when there is none)
template <typename KT>
__device__ __forceinline__ i64 cm_lower_bound(const KT *__restrict__ keys, i64 n, KT x) {
    i64 lo = 0, hi = n;
    while (lo < hi) {
        const i64 mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <typename KT>
__device__ __forceinline__ bool cm_find(const KT *__restrict__ keys, const unsigned *__restrict__ cols, i64 n,
                                        const unsigned *__restrict__ ids, unsigned n_sets, KT x, unsigned &id) {
    const i64 p = cm_lower_bound(keys, n, x);
    if (p >= n || keys[p] != x) return false;
    const unsigned v = ids[cols[p]];
    id = v < n_sets ? v : 0;                               // (never: an object's ids stay below n_sets)
    return true;
}

// ctr[0] += keys of u in a, ctr[1] += in b, ctr[2] += in both.  kb == nullptr: no second side.
template <typename KT>
__global__ void __launch_bounds__(256) k_cm_locate(const KT *__restrict__ ku, i64 nu, const KT *__restrict__ ka,
                                                   const unsigned *__restrict__ ca, i64 na, const unsigned *__restrict__ ids_a,
                                                   unsigned sets_a, const KT *__restrict__ kb, const unsigned *__restrict__ cb, i64 nb,
                                                   const unsigned *__restrict__ ids_b, unsigned sets_b, u64 *__restrict__ pairs,
                                                   u64 *__restrict__ ctr) {
    u64 in_a = 0, in_b = 0, in_both = 0;
    // (whole waves go round together: the bound is rounded up to the wave, and a lane past nu sits the ballots out)
    for (i64 i0 = (i64)blockIdx.x * 256 + (threadIdx.x & ~63u); i0 < nu; i0 += (i64)gridDim.x * 256) {
        const i64 i = i0 + (threadIdx.x & 63);
        bool fa = false, fb = false;
        if (i < nu) {
            const KT x = ku[i];
            unsigned ia = 0, ib = 0;
            fa = cm_find(ka, ca, na, ids_a, sets_a, x, ia);
            if (kb) fb = cm_find(kb, cb, nb, ids_b, sets_b, x, ib);
            pairs[i] = ((u64)ia << 32) | (u64)ib;
        }
        in_a += (u64)__popcll(__ballot(fa));
        in_b += (u64)__popcll(__ballot(fb));
        in_both += (u64)__popcll(__ballot(fa && fb));
    }
    if ((threadIdx.x & 63) == 0) {
        if (in_a) atomicAdd(ctr, in_a);
        if (in_b) atomicAdd(ctr + 1, in_b);
        if (in_both) atomicAdd(ctr + 2, in_both);
    }
}

// rows[r * words + w] of pair r = ptable[r]: ta's row | tb's row shifted up by 64 q + s bits; words past a table's width are 0,
// and pair 0 = (0, 0) gives the zero row because row 0 of both tables is zero.  tb == nullptr: no second side.
__global__ void __launch_bounds__(256) k_cm_rows(const u64 *__restrict__ ptable, i64 n_pairs, const u64 *__restrict__ ta, int wa,
                                                 const u64 *__restrict__ tb, int wb, int q, int s, int words, u64 *__restrict__ rows) {
    const i64 total = n_pairs * (i64)words;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < total; i += (i64)gridDim.x * 256) {
        const i64 r = i / words;
        const int w = (int)(i - r * words);
        const u64 pair = ptable[r];
        const unsigned ia = (unsigned)(pair >> 32), ib = (unsigned)pair;
        u64 v = w < wa ? ta[(i64)ia * wa + w] : 0ull;
        if (tb) {
            const int j = w - q;
            if (j >= 0 && j < wb) v |= tb[(i64)ib * wb + j] << s;
            if (s != 0 && j >= 1 && j - 1 < wb) v |= tb[(i64)ib * wb + j - 1] >> (64 - s);
        }
        rows[i] = v;
    }
}

__global__ void __launch_bounds__(256) k_cm_scatter(const unsigned *__restrict__ cols, const unsigned *__restrict__ pid, i64 nu,
                                                    const unsigned *__restrict__ cls, unsigned *__restrict__ ids) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < nu; i += (i64)gridDim.x * 256) ids[cols[i]] = cls[pid[i]];
}

namespace {
double cm_ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
struct CmKeys {
    void *keys = nullptr;
    unsigned *cols = nullptr;
    long long n = 0;
    void release() {
        (void)hipFree(keys);
        (void)hipFree(cols);
        keys = nullptr;
        cols = nullptr;
    }
};

template <typename KT>
void cm_launch_locate(const CmKeys &ku, const CmKeys &ka, const SbwtCmSide &a, const CmKeys *kb, const SbwtCmSide *b, u64 *pairs,
                      u64 *ctr, hipStream_t stream) {
    hipLaunchKernelGGL(k_cm_locate<KT>, dim3(cm_stride_grid(ku.n)), dim3(256), 0, stream, (const KT *)ku.keys, (i64)ku.n,
                       (const KT *)ka.keys, (const unsigned *)ka.cols, (i64)ka.n, a.d_ids, (unsigned)a.n_sets,
                       (const KT *)(kb ? kb->keys : nullptr), (const unsigned *)(kb ? kb->cols : nullptr), (i64)(kb ? kb->n : 0),
                       b ? b->d_ids : nullptr, (unsigned)(b ? b->n_sets : 1), pairs, ctr);
}
}  // namespace

#define CM_TRY(expr)                      \
    do {                                  \
        e = (expr);                       \
        if (e != hipSuccess) goto done;   \
    } while (0)

hipError_t sbwt_colormerge(const SbwtIndexView &u, const SbwtCmSide &a, const SbwtCmSide *b, int u_is, bool b_is_a,
                           int color_offset_b, int words_out, unsigned **d_ids, unsigned long long **d_table, long long *n_sets,
                           SbwtCmInfo *info, hipStream_t stream) {
    hipError_t e = hipSuccess;
    CmKeys own[3];                                          // the extracted lists: of a, of b, of u -- as far as they differ
    const CmKeys *ka = &own[0], *kb = nullptr, *ku = nullptr;
    u64 *pairs = nullptr, *ctr = nullptr, *ptable = nullptr, *prows = nullptr, *table = nullptr;
    unsigned *pid = nullptr, *cls = nullptr, *ids = nullptr;
    u64 h_ctr[3] = {0, 0, 0};
    long long n_p = 0, sets = 0;
    *d_ids = nullptr;
    *d_table = nullptr;
    *n_sets = 0;
    *info = SbwtCmInfo();
    if (b && b_is_a && u_is == 2) u_is = 1;

    auto t0 = std::chrono::steady_clock::now();
    CM_TRY(sbwt_setops_keys(a.ix, &own[0].keys, &own[0].n, stream, &own[0].cols));
    if (b) {
        kb = b_is_a ? &own[0] : &own[1];
        if (!b_is_a) CM_TRY(sbwt_setops_keys(b->ix, &own[1].keys, &own[1].n, stream, &own[1].cols));
    }
    ku = u_is == 1 ? ka : (u_is == 2 && kb) ? kb : &own[2];
    if (ku == &own[2]) CM_TRY(sbwt_setops_keys(u, &own[2].keys, &own[2].n, stream, &own[2].cols));
    info->pass_ms[0] = cm_ms_since(t0);
    info->n_real_u = ku->n;

    t0 = std::chrono::steady_clock::now();
    CM_TRY(hipMalloc((void **)&pairs, (size_t)(ku->n ? ku->n : 1) * 8));
    CM_TRY(hipMalloc((void **)&ctr, 32));
    CM_TRY(hipMemsetAsync(ctr, 0, 32, stream));
    if (u.k <= 32) cm_launch_locate<u64>(*ku, *ka, a, kb, b, pairs, ctr, stream);
    else cm_launch_locate<u128>(*ku, *ka, a, kb, b, pairs, ctr, stream);
    CM_TRY(hipGetLastError());
    CM_TRY(hipMemcpyAsync(h_ctr, ctr, 24, hipMemcpyDeviceToHost, stream));
    CM_TRY(hipStreamSynchronize(stream));
    info->n_from_a = (long long)h_ctr[0];
    info->n_from_b = (long long)h_ctr[1];
    info->n_from_both = (long long)h_ctr[2];
    // (the other lists' keys and columns have done their work; u's columns are needed for the scatter)
    for (CmKeys &l : own)
        if (&l != ku) l.release();
    info->pass_ms[1] = cm_ms_since(t0);

    t0 = std::chrono::steady_clock::now();
    CM_TRY(sbwt_colorsets_compress(pairs, ku->n, 1, &pid, &ptable, &n_p, stream));
    (void)hipFree(pairs);
    pairs = nullptr;
    info->n_pairs = n_p - 1;
    CM_TRY(hipMalloc((void **)&prows, (size_t)n_p * (size_t)words_out * 8));
    hipLaunchKernelGGL(k_cm_rows, dim3(cm_stride_grid(n_p * words_out)), dim3(256), 0, stream, (const u64 *)ptable, (i64)n_p,
                       (const u64 *)a.d_table, a.words, (const u64 *)(b ? b->d_table : nullptr), b ? b->words : 0, color_offset_b >> 6,
                       color_offset_b & 63, words_out, prows);
    CM_TRY(hipGetLastError());
    CM_TRY(hipStreamSynchronize(stream));
    info->pass_ms[2] = cm_ms_since(t0);

    t0 = std::chrono::steady_clock::now();
    CM_TRY(sbwt_colorsets_compress(prows, n_p, words_out, &cls, &table, &sets, stream));
    CM_TRY(hipMalloc((void **)&ids, (size_t)u.n_nodes * 4 + 16));
    CM_TRY(hipMemsetAsync(ids, 0, (size_t)u.n_nodes * 4 + 16, stream));
    hipLaunchKernelGGL(k_cm_scatter, dim3(cm_stride_grid(ku->n)), dim3(256), 0, stream, (const unsigned *)ku->cols, (const unsigned *)pid,
                       (i64)ku->n, (const unsigned *)cls, ids);
    CM_TRY(hipGetLastError());
    CM_TRY(hipStreamSynchronize(stream));
    info->pass_ms[3] = cm_ms_since(t0);
    info->n_sets = sets;
    *d_ids = ids;
    *d_table = (unsigned long long *)table;
    *n_sets = sets;
    ids = nullptr;
    table = nullptr;
done:
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(stream);
        (void)hipGetLastError();
    }
    for (CmKeys &l : own) l.release();
    (void)hipFree(pairs); (void)hipFree(ctr); (void)hipFree(pid); (void)hipFree(ptable); (void)hipFree(prows); (void)hipFree(cls);
    (void)hipFree(ids); (void)hipFree(table);
    return e;
}
