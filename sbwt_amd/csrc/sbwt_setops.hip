// sbwt_setops.hip -- set operations on two indexes: the k-mers of an index back as the builder's sorted
// keys, and the merge of two such lists under union / intersection / difference / symmetric difference.  What comes out goes
// to the builder's tail (sbwt_build_from_keys, sbwt_build.hip), which starts from sorted distinct keys: no text, no sort.
//
// Label extraction (sbwt_setops_keys), every pass a flat launch over the columns, reading the blocks and C only:
//   1  pred[C[c] + rank_c(u)] = u                                               (k_ut_pred, sbwt_colwalk.h)
//   2  level of every dummy, k-1 rounds from the root; level 0 = real           (k_ut_level)
//   3  windows by doubling over pred.  Per column v a state { W_m(v), J_m(v) }: W_m(v) = the last m characters of v's
//      label as key bits (the oldest of them at bits 0-1), J_m(v) = pred^m(v).  Two windows combine as
//          W_{a+b}(v) = W_b(J_a(v)) | W_a(v) << 2b,      J_{a+b}(v) = J_b(J_a(v))
//      and a round follows the binary expansion of k from its top bit down: it doubles m (a = b = m: ONE random read of the
//      state of J_m(v)) and, where the expansion has a 1, appends one more character (a = 2m, b = 1: W_1(u) is u's last
//      character, which C tells without a read; J_1(u) = pred[u], one random 4-byte read).  floor(log2 k) double-buffered
//      rounds give W_k = the key -- against k dependent 4-byte reads per column for a serial walk.
//      INVARIANT: pred(0) = 0 and nothing is checked on the way: a dummy's chain reaches the root and idles there, so a
//      dummy's window holds bits that mean nothing.  A real column's k-1 predecessors never are the root (that is what real
//      means), every window of length <= k that a real column combines lies within them, so its key never contains such bits.
//      Only the real columns' keys leave this file.
//   4  real flags -> exclusive scan (sbwt_scan.h) -> the keys compacted in column order = ascending key order; on request
//      the column of every key beside it (sbwt_colormerge.hip gathers per-column data through it)
//
// Merge and select (sbwt_setops_merge): rocprim::merge by key with the origin (0 = a, 1 = b) as the value -- no sort of any
// kind.  Each list is duplicate-free, so a run of equal keys in the merged order has length 1 or 2; the first element of a run
// decides: union keeps it, intersection when the run has two, difference when it has one and comes from a, symmetric
// difference when it has one.  Flags -> scan -> compact.  The counts-only form counts the runs of two and stops.
#include <rocprim/device/device_merge.hpp>
#include "sbwt_colwalk.h"
#include "sbwt_scan.h"
#include "sbwt_setops.h"

typedef __uint128_t u128;

// window + pointer of one column: 16 bytes for 64-bit keys, 32 for 128-bit keys (one aligned read either way)
template <typename KT> struct SoState { KT w; unsigned j; };
static_assert(sizeof(SoState<u64>) == 16 && sizeof(SoState<u128>) == 32, "one or two 16-byte quads per state");

// ---- pass 3 ----
template <typename KT>
__global__ void __launch_bounds__(256) k_so_init(SbwtIndexView ix, const unsigned *__restrict__ pred, SoState<KT> *__restrict__ st) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v >= ix.n_nodes) return;
    SoState<KT> s;
    s.w = (KT)ut_last_char(ix, v);
    s.j = pred[v];
    st[v] = s;
}
// m -> 2m (+ 1 when `plus`): see the head of the file.  2m + plus <= k <= 4 * sizeof(KT), so no shift reaches the key's width.
template <typename KT>
__global__ void __launch_bounds__(256) k_so_double(SbwtIndexView ix, const unsigned *__restrict__ pred, const SoState<KT> *__restrict__ in,
                                                   SoState<KT> *__restrict__ out, int m, int plus) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v >= ix.n_nodes) return;
    const SoState<KT> s = in[v];
    const SoState<KT> q = in[s.j];
    SoState<KT> r;
    r.w = q.w | (s.w << (2 * m));
    r.j = q.j;
    if (plus) {
        r.w = (KT)ut_last_char(ix, (i64)r.j) | (r.w << 2);
        r.j = pred[r.j];
    }
    out[v] = r;
}

// ---- pass 4 ----
__global__ void __launch_bounds__(256) k_so_real(i64 n, const unsigned char *__restrict__ lev, i64 *__restrict__ flag) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v < n) flag[v] = lev[v] == 0 ? 1 : 0;
}
template <typename KT>
__global__ void __launch_bounds__(256) k_so_gather(i64 n, const SoState<KT> *__restrict__ st, const unsigned char *__restrict__ lev,
                                                   const i64 *__restrict__ pos, KT *__restrict__ keys, unsigned *__restrict__ cols) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v < n && lev[v] == 0) {
        keys[pos[v]] = st[v].w;
        if (cols) cols[pos[v]] = (unsigned)v;
    }
}

// ---- merge and select ----
// keep[i] for the operation, and the number of runs of two (= |a AND b|) summed into *n_both (one atomic per wave that has any)
template <typename KT>
__global__ void __launch_bounds__(256) k_so_select(const KT *__restrict__ m, const unsigned char *__restrict__ org, i64 n, int op,
                                                   i64 *__restrict__ keep, unsigned long long *__restrict__ n_both) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    bool pair = false;
    if (i < n) {
        const KT x = m[i];
        const bool first = i == 0 || m[i - 1] != x;
        pair = first && i + 1 < n && m[i + 1] == x;
        if (keep) {
            const bool single = first && !pair;
            bool kp;
            if (op == 0) kp = first;
            else if (op == 1) kp = pair;
            else if (op == 2) kp = single && org[i] == 0;
            else kp = single;
            keep[i] = kp ? 1 : 0;
        }
    }
    const u64 b = __ballot(pair);
    if (b && (threadIdx.x & 63) == 0) atomicAdd(n_both, (unsigned long long)__popcll(b));
}
template <typename KT>
__global__ void __launch_bounds__(256) k_so_compact(const KT *__restrict__ m, const i64 *__restrict__ keep, const i64 *__restrict__ pos,
                                                    i64 n, KT *__restrict__ out) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < n && keep[i]) out[pos[i]] = m[i];
}

// ---------------------------------------------------------------------------------------------
static inline i64 so_pad(i64 n) { return (n + 64 + 255) & ~(i64)255; }
struct SoLayout {
    i64 pred, lev, st0, st1, bsum, bytes;
    SoLayout(i64 n, int state_bytes) {
        const i64 np = so_pad(n);
        pred = 0;
        lev = pred + 4 * np;
        st0 = lev + np;
        st1 = st0 + (i64)state_bytes * np;
        bsum = st1 + (i64)state_bytes * np;
        bytes = bsum + ((8 * (np / 1024 + 4) + 255) & ~(i64)255);
    }
};
long long sbwt_setops_scratch_bytes(long long n_nodes, int k) { return SoLayout(n_nodes, k <= 32 ? 16 : 32).bytes; }

static void so_scan(const i64 *in, i64 n, i64 *bsum, i64 *out, hipStream_t stream) {
    if (n <= 0) {
        (void)hipMemsetAsync(out, 0, 8, stream);
        return;
    }
    const unsigned nb = (unsigned)((n + 1023) / 1024);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(nb), dim3(256), 0, stream, in, n, bsum);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, stream, bsum, (i64)nb);
    hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(256), 0, stream, in, n, bsum, out);
}

#define SO_TRY(expr)                      \
    do {                                  \
        e = (expr);                       \
        if (e != hipSuccess) goto done;   \
    } while (0)

template <typename KT>
static hipError_t setops_keys_t(const SbwtIndexView &ix, void **d_keys, long long *n_keys, hipStream_t stream, unsigned **d_cols) {
    const bool mega = ix.n_mega > 1 || ix.force_mega;
    const i64 n = ix.n_nodes;
    const int k = ix.k;
    const SoLayout L(n, (int)sizeof(SoState<KT>));
    const unsigned g = grid_for(n);
    hipError_t e = hipSuccess;
    char *base = nullptr;
    KT *keys = nullptr;
    unsigned *cols = nullptr;
    unsigned *pred = nullptr;
    unsigned char *lev = nullptr;
    SoState<KT> *st[2] = {nullptr, nullptr};
    i64 *bsum = nullptr, *flag = nullptr, *pos = nullptr;
    i64 nk = 0;
    int cur = 0, m = 1, top = 0;
    *d_keys = nullptr;
    *n_keys = 0;
    if (d_cols) *d_cols = nullptr;
    SO_TRY(hipMalloc((void **)&base, (size_t)L.bytes));
    pred = reinterpret_cast<unsigned *>(base + L.pred);
    lev = reinterpret_cast<unsigned char *>(base + L.lev);
    st[0] = reinterpret_cast<SoState<KT> *>(base + L.st0);
    st[1] = reinterpret_cast<SoState<KT> *>(base + L.st1);
    bsum = reinterpret_cast<i64 *>(base + L.bsum);
    // (pred cleared first: an image whose columns are not those of an SBWT may leave entries unwritten, and every pointer of
    // pass 3 comes out of this array)
    SO_TRY(hipMemsetAsync(pred, 0, (size_t)(4 * so_pad(n)), stream));
    SO_TRY(hipMemsetAsync(lev, 0, (size_t)so_pad(n), stream));
    if (mega) hipLaunchKernelGGL(k_ut_pred<true>, dim3(g), dim3(256), 0, stream, ix, pred);
    else hipLaunchKernelGGL(k_ut_pred<false>, dim3(g), dim3(256), 0, stream, ix, pred);
    for (int r = 0; r + 1 < k; r++) {
        if (mega) hipLaunchKernelGGL(k_ut_level<true>, dim3(g), dim3(256), 0, stream, ix, lev, r);
        else hipLaunchKernelGGL(k_ut_level<false>, dim3(g), dim3(256), 0, stream, ix, lev, r);
    }
    hipLaunchKernelGGL(k_so_init<KT>, dim3(g), dim3(256), 0, stream, ix, (const unsigned *)pred, st[0]);
    while ((k >> (top + 1)) != 0) top++;                     // k's highest set bit
    for (int bit = top - 1; bit >= 0; bit--) {
        const int plus = (k >> bit) & 1;
        hipLaunchKernelGGL(k_so_double<KT>, dim3(g), dim3(256), 0, stream, ix, (const unsigned *)pred, (const SoState<KT> *)st[cur],
                           st[cur ^ 1], m, plus);
        cur ^= 1;
        m = 2 * m + plus;
    }
    // the scans work in the half of the state that is free now: flag[n], pos[n + 1] (16 n + 8 bytes of at least 16 (n + 64))
    flag = reinterpret_cast<i64 *>(st[cur ^ 1]);
    pos = flag + n;
    hipLaunchKernelGGL(k_so_real, dim3(g), dim3(256), 0, stream, n, (const unsigned char *)lev, flag);
    so_scan(flag, n, bsum, pos, stream);
    SO_TRY(hipMemcpyAsync(&nk, pos + n, 8, hipMemcpyDeviceToHost, stream));
    SO_TRY(hipStreamSynchronize(stream));
    SO_TRY(hipMalloc((void **)&keys, (size_t)(nk ? nk : 1) * sizeof(KT)));
    if (d_cols) SO_TRY(hipMalloc((void **)&cols, (size_t)(nk ? nk : 1) * 4));
    hipLaunchKernelGGL(k_so_gather<KT>, dim3(g), dim3(256), 0, stream, n, (const SoState<KT> *)st[cur], (const unsigned char *)lev,
                       (const i64 *)pos, keys, cols);
    SO_TRY(hipGetLastError());
    SO_TRY(hipStreamSynchronize(stream));
    *d_keys = keys;
    *n_keys = nk;
    if (d_cols) *d_cols = cols;
    keys = nullptr;
    cols = nullptr;
done:
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(stream);
        (void)hipGetLastError();
    }
    (void)hipFree(base);
    (void)hipFree(keys);
    (void)hipFree(cols);
    return e;
}
hipError_t sbwt_setops_keys(const SbwtIndexView &ix, void **d_keys, long long *n_keys, hipStream_t stream, unsigned **d_cols) {
    return ix.k <= 32 ? setops_keys_t<u64>(ix, d_keys, n_keys, stream, d_cols) : setops_keys_t<u128>(ix, d_keys, n_keys, stream, d_cols);
}

template <typename KT>
static hipError_t setops_merge_t(const KT *a, i64 na, const KT *b, i64 nb, int op, void **d_out, SbwtSetopCounts *counts,
                                 hipStream_t stream) {
    const i64 n = na + nb;
    hipError_t e = hipSuccess;
    KT *merged = nullptr, *out = nullptr;
    unsigned char *org_in = nullptr, *org = nullptr;
    i64 *keep = nullptr, *pos = nullptr, *bsum = nullptr;
    unsigned long long *d_both = nullptr, h_both = 0;
    void *tmp = nullptr;
    size_t tmp_bytes = 0;
    i64 n_res = 0;
    *counts = SbwtSetopCounts();
    if (d_out) *d_out = nullptr;
    SO_TRY(hipMalloc((void **)&d_both, 8));
    SO_TRY(hipMemsetAsync(d_both, 0, 8, stream));
    if (n > 0) {
        SO_TRY(hipMalloc((void **)&merged, (size_t)n * sizeof(KT)));
        SO_TRY(hipMalloc((void **)&org_in, (size_t)n));
        SO_TRY(hipMalloc((void **)&org, (size_t)n));
        SO_TRY(hipMemsetAsync(org_in, 0, (size_t)na, stream));
        SO_TRY(hipMemsetAsync(org_in + na, 1, (size_t)nb, stream));
        SO_TRY(rocprim::merge(nullptr, tmp_bytes, a, b, merged, (const unsigned char *)org_in, (const unsigned char *)(org_in + na), org,
                              (size_t)na, (size_t)nb, rocprim::less<KT>(), stream));
        SO_TRY(hipMalloc(&tmp, tmp_bytes + 16));
        SO_TRY(rocprim::merge(tmp, tmp_bytes, a, b, merged, (const unsigned char *)org_in, (const unsigned char *)(org_in + na), org,
                              (size_t)na, (size_t)nb, rocprim::less<KT>(), stream));
        if (d_out) {
            SO_TRY(hipMalloc((void **)&keep, (size_t)(n + 1) * 8));
            SO_TRY(hipMalloc((void **)&pos, (size_t)(n + 2) * 8));
            SO_TRY(hipMalloc((void **)&bsum, (size_t)((n + 1023) / 1024 + 2) * 8));
        }
        hipLaunchKernelGGL(k_so_select<KT>, dim3(grid_for(n)), dim3(256), 0, stream, (const KT *)merged, (const unsigned char *)org, n, op,
                           keep, d_both);
        if (d_out) {
            so_scan(keep, n, bsum, pos, stream);
            SO_TRY(hipMemcpyAsync(&n_res, pos + n, 8, hipMemcpyDeviceToHost, stream));
        }
    }
    SO_TRY(hipMemcpyAsync(&h_both, d_both, 8, hipMemcpyDeviceToHost, stream));
    SO_TRY(hipStreamSynchronize(stream));
    if (d_out) {
        SO_TRY(hipMalloc((void **)&out, (size_t)(n_res ? n_res : 1) * sizeof(KT)));
        if (n > 0)
            hipLaunchKernelGGL(k_so_compact<KT>, dim3(grid_for(n)), dim3(256), 0, stream, (const KT *)merged, (const i64 *)keep,
                               (const i64 *)pos, n, out);
        SO_TRY(hipGetLastError());
        SO_TRY(hipStreamSynchronize(stream));
        *d_out = out;
        out = nullptr;
    }
    counts->n_a = na;
    counts->n_b = nb;
    counts->n_both = (i64)h_both;
    counts->n_either = n - (i64)h_both;
    counts->n_result = n_res;
done:
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(stream);
        (void)hipGetLastError();
    }
    (void)hipFree(merged); (void)hipFree(org_in); (void)hipFree(org); (void)hipFree(keep); (void)hipFree(pos); (void)hipFree(bsum);
    (void)hipFree(d_both); (void)hipFree(tmp); (void)hipFree(out);
    return e;
}
hipError_t sbwt_setops_merge(const void *d_a, long long n_a, const void *d_b, long long n_b, int key_bytes, int op, void **d_out,
                             SbwtSetopCounts *counts, hipStream_t stream) {
    return key_bytes == 8 ? setops_merge_t<u64>(static_cast<const u64 *>(d_a), n_a, static_cast<const u64 *>(d_b), n_b, op, d_out, counts, stream)
                          : setops_merge_t<u128>(static_cast<const u128 *>(d_a), n_a, static_cast<const u128 *>(d_b), n_b, op, d_out, counts, stream);
}
