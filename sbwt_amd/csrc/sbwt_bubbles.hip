// sbwt_bubbles.hip -- bubbles of the plain unitig graph: variant sites and the colours of each allele.
//
// A bubble is four unitigs (s, a, b, t): s has exactly the two links a, b (CSR order), a and b have one in-link and one
// out-link each, both out-links go to t, t has exactly two in-links, and neither a nor b is s or t (s = t is allowed).  In
// the plain graph every branch is a single unitig, so everything is decided on link_off / link_to alone:
//   k_bb_indeg               indeg[j] = the entries of link_to equal to j: one atomic add per link
//   k_bb_detect              one lane per unitig s applies the definition (four dependent gathers at most) and writes a flag
//   k_scan_*                 the exclusive scan of the flags (sbwt_scan.h): a bubble's number, ascending by source
//   k_bb_fill                the records, the slot table (slot[branch j of bubble i] = 2 i + j, else 0xFFFFFFFF), n_snps
//   k_bb_rows_init           inter = ones below n_colors, uni = 0
//   k_bb_colors              one lane per column: col_unitig[v] coalesced, the slot of its unitig, and for a branch column
//                            the row table[ids[v]] AND-ed into inter and OR-ed into uni with 64-bit atomics
// A branch has in-degree 1, so it belongs to one bubble and its slot is unique.  All launches are flat grid-stride loops.
#include "sbwt_kernels_common.h"
#include "sbwt_bubbles.h"
#include "sbwt_scan.h"

static inline long long bb_a256(long long x) { return (x + 255) & ~255ll; }

// grid for a grid-stride loop over n items: enough blocks to fill the chip, no more
static inline unsigned bb_stride_grid(i64 n) {
    const i64 g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : g > 8192 ? 8192 : g);
}

struct BbLayout {
    long long indeg, slot, flag, pre, bsum, ctr, total;
};
static BbLayout bb_layout(long long n_unitigs) {
    BbLayout L;
    long long p = 0;
    L.indeg = p; p += bb_a256(n_unitigs * 4 + 4);
    L.slot = p; p += bb_a256(n_unitigs * 4 + 4);
    L.flag = p; p += bb_a256(n_unitigs * 8 + 8);
    L.pre = p; p += bb_a256((n_unitigs + 1) * 8);
    L.bsum = p; p += bb_a256((n_unitigs / 1024 + 3) * 8);
    L.ctr = p; p += 256;
    L.total = p;
    return L;
}
long long sbwt_bubbles_scratch_bytes(long long n_unitigs) { return bb_layout(n_unitigs).total; }

// ---------------------------------------------------------------------------------------------
// pass 1: in-degrees
// ---------------------------------------------------------------------------------------------
// (a target that is no unitig -- never: links end at unitigs -- is skipped, so nothing outside indeg is touched)
__global__ void __launch_bounds__(256) k_bb_indeg(const unsigned *__restrict__ link_to, i64 n_links, i64 n_unitigs,
                                                  unsigned *__restrict__ indeg) {
    for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < n_links; e += (i64)gridDim.x * 256) {
        const unsigned j = __builtin_nontemporal_load(link_to + e);
        if ((i64)j < n_unitigs) atomicAdd(indeg + j, 1u);
    }
}

// ---------------------------------------------------------------------------------------------
// pass 2: detect
// ---------------------------------------------------------------------------------------------
// the definition for source s; a, b, t are what the record takes when it holds
__device__ __forceinline__ bool bb_test(const i64 *__restrict__ link_off, const unsigned *__restrict__ link_to,
                                        const unsigned *__restrict__ indeg, i64 n_unitigs, i64 s, unsigned &a, unsigned &b,
                                        unsigned &t) {
    const i64 lo = link_off[s];
    if (link_off[s + 1] - lo != 2) return false;
    a = link_to[lo];
    b = link_to[lo + 1];
    if ((i64)a >= n_unitigs || (i64)b >= n_unitigs || a == b || (i64)a == s || (i64)b == s) return false;
    if (indeg[a] != 1u || indeg[b] != 1u) return false;
    const i64 la = link_off[a], lb = link_off[b];
    if (link_off[a + 1] - la != 1 || link_off[b + 1] - lb != 1) return false;
    t = link_to[la];
    if (link_to[lb] != t || (i64)t >= n_unitigs || t == a || t == b) return false;
    return indeg[t] == 2u;
}

__global__ void __launch_bounds__(256) k_bb_detect(const i64 *__restrict__ link_off, const unsigned *__restrict__ link_to,
                                                   const unsigned *__restrict__ indeg, i64 n_unitigs, i64 *__restrict__ flag) {
    for (i64 s = (i64)blockIdx.x * 256 + threadIdx.x; s < n_unitigs; s += (i64)gridDim.x * 256) {
        unsigned a, b, t;
        flag[s] = bb_test(link_off, link_to, indeg, n_unitigs, s, a, b, t) ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------
// pass 3: records and slot table
// ---------------------------------------------------------------------------------------------
// The flagged lanes repeat the test for a, b, t (the gathers hit the cache the detect pass filled; storing them would take
// 12 bytes per unitig for the few that are sources).  n_kmers = length - k + 1 from the base offsets.  One add per wave
// counts the SNPs.  (slot is filled with 0xFFFFFFFF before.)
typedef unsigned u32x4_bb __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) k_bb_fill(const i64 *__restrict__ link_off, const unsigned *__restrict__ link_to,
                                                 const unsigned *__restrict__ indeg, const i64 *__restrict__ off, i64 n_unitigs, i64 k,
                                                 const i64 *__restrict__ flag, const i64 *__restrict__ pre, i64 n_bubbles,
                                                 SbwtBubble *__restrict__ rec, unsigned *__restrict__ slot, u64 *__restrict__ n_snps) {
    const i64 n_round = (n_unitigs + 63) & ~63ll;         // whole waves enter the loop: the ballot below needs every lane
    for (i64 s = (i64)blockIdx.x * 256 + threadIdx.x; s < n_round; s += (i64)gridDim.x * 256) {
        bool snp = false;
        unsigned a, b, t;
        if (s < n_unitigs && flag[s] && bb_test(link_off, link_to, indeg, n_unitigs, s, a, b, t)) {
            const i64 i = pre[s];
            if (i < n_bubbles) {
                const i64 na = off[a + 1] - off[a] - k + 1, nb = off[b + 1] - off[b] - k + 1;
                snp = na == k && nb == k;
                const u32x4_bb lo = {(unsigned)s, a, b, t}, hi = {(unsigned)na, (unsigned)nb, snp ? 1u : 0u, 0u};
                u32x4_bb *p = reinterpret_cast<u32x4_bb *>(rec + i);
                p[0] = lo;
                p[1] = hi;
                slot[a] = (unsigned)(2 * i);
                slot[b] = (unsigned)(2 * i + 1);
            }
        }
        const u64 m = __ballot(snp);
        if (m && (threadIdx.x & 63) == 0) atomicAdd(n_snps, (u64)__popcll(m));
    }
}

// ---------------------------------------------------------------------------------------------
// pass 4: branch colours
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bb_rows_init(u64 *__restrict__ inter, u64 *__restrict__ uni, i64 n_rows, int words,
                                                      int n_colors) {
    const i64 n = n_rows * words;
    const int last = n_colors & 63;
    for (i64 x = (i64)blockIdx.x * 256 + threadIdx.x; x < n; x += (i64)gridDim.x * 256) {
        const int w = (int)(x % words);
        inter[x] = (w == words - 1 && last) ? low_mask(last) : ~0ull;
        uni[x] = 0ull;
    }
}

// The stream is the 4 bytes per column of the map; the slot gather goes to a table of 4 bytes per unitig and only the branch
// columns (about k per branch) go on to ids, the table and the atomics.  A row has no bit at or above n_colors (an invariant
// of the object), so the words go in as they are.  (Four columns per lane and 16-byte load measured the same: the pass is
// bound by the gathers and atomics of the branch columns)
__global__ void __launch_bounds__(256) k_bb_colors(const unsigned *__restrict__ col_unitig, i64 n_nodes, i64 n_unitigs,
                                                   const unsigned *__restrict__ slot, const unsigned *__restrict__ ids,
                                                   const u64 *__restrict__ table, int words, i64 n_rows, u64 *__restrict__ inter,
                                                   u64 *__restrict__ uni) {
    for (i64 v = (i64)blockIdx.x * 256 + threadIdx.x; v < n_nodes; v += (i64)gridDim.x * 256) {
        const unsigned un = __builtin_nontemporal_load(col_unitig + v);
        if ((i64)un >= n_unitigs) continue;              // a dummy column (0xFFFFFFFF)
        const unsigned sl = slot[un];
        if ((i64)sl >= n_rows) continue;                 // no branch (0xFFFFFFFF)
        const u64 *row = table + (i64)ids[v] * words;
        u64 *pi = inter + (i64)sl * words, *pu = uni + (i64)sl * words;
        for (int w = 0; w < words; w++) {
            const u64 r = row[w];
            atomicAnd(pi + w, r);
            if (r) atomicOr(pu + w, r);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------------------------
hipError_t sbwt_bubbles_in_degrees(const unsigned *d_link_to, long long n_links, long long n_unitigs, unsigned *d_indeg,
                                   hipStream_t stream) {
    if (n_unitigs <= 0) return hipSuccess;
    const hipError_t e = hipMemsetAsync(d_indeg, 0, (size_t)n_unitigs * 4, stream);
    if (e != hipSuccess) return e;
    if (n_links > 0)
        hipLaunchKernelGGL(k_bb_indeg, dim3(bb_stride_grid(n_links)), dim3(256), 0, stream, d_link_to, (i64)n_links, (i64)n_unitigs, d_indeg);
    return hipGetLastError();
}

#define BB_TRY(x)                 \
    do {                          \
        e = (x);                  \
        if (e != hipSuccess) goto done; \
    } while (0)

hipError_t sbwt_bubbles_run(const SbwtBubbleGraph &g, SbwtBubbleRun *run, hipStream_t stream) {
    *run = SbwtBubbleRun();
    const i64 n = g.n_unitigs;
    if (n <= 0 || g.n_links <= 0) return hipSuccess;      // no link, no bubble
    const BbLayout L = bb_layout(n);
    const unsigned nb = (unsigned)((n + 1023) / 1024);
    const bool colors = g.d_ids != nullptr;
    hipError_t e = hipSuccess;
    char *ws = nullptr;
    hipEvent_t ev[SBWT_BB_N_PASSES + 1] = {};
    unsigned *indeg, *slot;
    i64 *flag, *pre, *bsum;
    u64 *ctr;
    i64 n_bubbles = 0;
    u64 n_snps = 0;
    BB_TRY(hipMalloc((void **)&ws, (size_t)L.total));
    indeg = reinterpret_cast<unsigned *>(ws + L.indeg);
    slot = reinterpret_cast<unsigned *>(ws + L.slot);
    flag = reinterpret_cast<i64 *>(ws + L.flag);
    pre = reinterpret_cast<i64 *>(ws + L.pre);
    bsum = reinterpret_cast<i64 *>(ws + L.bsum);
    ctr = reinterpret_cast<u64 *>(ws + L.ctr);
    for (int i = 0; i <= SBWT_BB_N_PASSES; i++) BB_TRY(hipEventCreate(&ev[i]));

    BB_TRY(hipEventRecord(ev[SBWT_BB_PASS_INDEG], stream));
    BB_TRY(sbwt_bubbles_in_degrees(g.d_link_to, g.n_links, n, indeg, stream));

    BB_TRY(hipEventRecord(ev[SBWT_BB_PASS_DETECT], stream));
    hipLaunchKernelGGL(k_bb_detect, dim3(bb_stride_grid(n)), dim3(256), 0, stream, (const i64 *)g.d_link_off, g.d_link_to,
                       (const unsigned *)indeg, n, flag);

    BB_TRY(hipEventRecord(ev[SBWT_BB_PASS_COMPACT], stream));
    hipLaunchKernelGGL(k_scan_block_sums, dim3(nb), dim3(256), 0, stream, (const i64 *)flag, n, bsum);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, stream, bsum, (i64)nb);
    hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(256), 0, stream, (const i64 *)flag, n, (const i64 *)bsum, pre);
    BB_TRY(hipGetLastError());
    BB_TRY(hipMemcpyAsync(&n_bubbles, pre + n, 8, hipMemcpyDeviceToHost, stream));
    BB_TRY(hipStreamSynchronize(stream));
    if (n_bubbles > 0) {
        BB_TRY(hipMalloc((void **)&run->d_rec, (size_t)n_bubbles * sizeof(SbwtBubble)));
        if (colors) {
            BB_TRY(hipMalloc((void **)&run->d_inter, (size_t)n_bubbles * 2 * g.words * 8));
            BB_TRY(hipMalloc((void **)&run->d_uni, (size_t)n_bubbles * 2 * g.words * 8));
        }
        BB_TRY(hipMemsetAsync(slot, 0xFF, (size_t)n * 4, stream));
        BB_TRY(hipMemsetAsync(ctr, 0, 8, stream));
        hipLaunchKernelGGL(k_bb_fill, dim3(bb_stride_grid(n)), dim3(256), 0, stream, (const i64 *)g.d_link_off, g.d_link_to,
                           (const unsigned *)indeg, (const i64 *)g.d_off, n, (i64)g.k, (const i64 *)flag, (const i64 *)pre, n_bubbles,
                           run->d_rec, slot, ctr);
        BB_TRY(hipGetLastError());
    }

    BB_TRY(hipEventRecord(ev[SBWT_BB_PASS_COLORS], stream));
    if (n_bubbles > 0 && colors) {
        const i64 n_rows = 2 * n_bubbles;
        hipLaunchKernelGGL(k_bb_rows_init, dim3(bb_stride_grid(n_rows * g.words)), dim3(256), 0, stream, run->d_inter, run->d_uni, n_rows,
                           g.words, g.n_colors);
        hipLaunchKernelGGL(k_bb_colors, dim3(bb_stride_grid(g.n_nodes)), dim3(256), 0, stream, g.d_col_unitig, (i64)g.n_nodes, n,
                           (const unsigned *)slot, g.d_ids, (const u64 *)g.d_table, g.words, n_rows, run->d_inter, run->d_uni);
        BB_TRY(hipGetLastError());
    }
    BB_TRY(hipEventRecord(ev[SBWT_BB_N_PASSES], stream));
    if (n_bubbles > 0) BB_TRY(hipMemcpyAsync(&n_snps, ctr, 8, hipMemcpyDeviceToHost, stream));
    BB_TRY(hipStreamSynchronize(stream));
    for (int i = 0; i < SBWT_BB_N_PASSES; i++) BB_TRY(hipEventElapsedTime(&run->ms[i], ev[i], ev[i + 1]));
    run->n_bubbles = n_bubbles;
    run->n_snps = (long long)n_snps;
done:
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(stream);
        if (run->d_rec) (void)hipFree(run->d_rec);
        if (run->d_inter) (void)hipFree(run->d_inter);
        if (run->d_uni) (void)hipFree(run->d_uni);
        *run = SbwtBubbleRun();
    }
    for (int i = 0; i <= SBWT_BB_N_PASSES; i++)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    if (ws) (void)hipFree(ws);
    return e;
}
