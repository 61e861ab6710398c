// sbwt_colormatrix.hip -- pairwise shared k-mer counts between colours (include/sbwtgpu.h, "shared k-mers"; DESIGN.md
// section 19): G = B^T diag(w) B for the n_sets x n_colors bit matrix B of a colour-set table and one weight per set, exact
// in int64.  With w[t] = the columns that carry set t, G[a][b] is the number of index k-mers that references a and b share.
//
//   k_gm_sizes      ids -> sizes[t]: a histogram.  A wave peels the two commonest ids of its 64 columns (readlane, ballot,
//                   popcount: one add each), the lanes left over add 1 each; ids below GM_LDS_IDS meet in the block's LDS and
//                   reach memory once per block -- 12.8 M columns over 8 sets would otherwise all meet at 8 addresses in L2.
//   k_gm_weights    sizes or the caller's int64 weights -> uint32 weights (set 0: 0; out of range: 0 and the set's number into
//                   the header's status by atomicMin), the sets' numbers for the sort, n_used and max_w of the header
//   --- few sets: the plain route ---
//   k_gm_plain      a wave per (colour a, word of colours b): the sets are walked once; the bit of a is wave-uniform, so a set
//                   without a costs one scalar test, and a set with it adds its weight in the lanes whose bit of b is set.
//                   Writes the matrix directly.
//   --- many sets: the matrix cores ---
//   (rocPRIM)       radix sort of (weight, set) by descending weight: the sets that count come first (compaction), and the
//                   sets whose weight has a limb l, w >= 128^l, are a prefix for every l
//   k_gm_limbs      sorted weights -> five arrays of 7-bit limbs, one byte per set, and the header's n_limb[l]
//   k_gm_transpose  table -> bit planes plane[kb][colour] = one 64-bit word: bit i says whether sorted set 64 kb + i holds the
//                   colour.  A wave takes 64 sets, lane i the row of set i; a ballot per colour gives the word, lane b keeps
//                   the ballot of colour 64 w + b, and the 64 words of a table word leave in one coalesced store.
//   k_gm_mfma       a wave per (64 x 64 tile pair ta <= tb, K chunk, limb): v_mfma_i32_16x16x64_i8, 4 x 4 tiles of 16 x 16.
//                   Lane (r = lane & 15, g = lane >> 4) holds for row/column r the 16 K values 16 g .. 16 g + 15 of a K block
//                   of 64 sets: 16 bits of a plane word, spread to 16 bytes of 0/1 (A) and ANDed as byte masks onto the 16
//                   limb bytes of those sets (B).  Both operands take their K values from the same bits in the same order,
//                   so the sum over K does not depend on how the instruction numbers K inside a lane.  The i32 tile is
//                   added into the padded int64 matrix shifted by 7 l bits, with one atomic per non-zero entry: at most
//                   flush_sets sets per wave, 127 flush_sets < 2^31.  Integer atomics commute: the bytes do not depend on
//                   the order of arrival.
//   k_gm_mirror     padded upper tiles -> the C x C result, the lower tiles read transposed
#include <chrono>
#include <rocprim/device/device_radix_sort.hpp>
#include "sbwt_kernels_common.h"
#include "sbwt_colormatrix.h"

#define GM_LDS_IDS 1024

static inline unsigned gm_stride_grid(i64 n, i64 cap) {
    const i64 g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}
static inline i64 gm_up(i64 x, i64 a) { return (x + a - 1) / a * a; }

// ---------------------------------------------------------------------------------------------
// sizes and weights
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_gm_sizes(const unsigned *__restrict__ ids, i64 n, unsigned n_sets, unsigned *__restrict__ sizes) {
    __shared__ unsigned lds_cnt[GM_LDS_IDS];
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < GM_LDS_IDS; i += 256) lds_cnt[i] = 0;
    __syncthreads();
    // (whole waves go round together: the bound is rounded up to the wave, and a lane past n sits the ballots out)
    for (i64 j0 = (i64)blockIdx.x * 256 + (threadIdx.x & ~63u); j0 < n; j0 += (i64)gridDim.x * 256) {
        const i64 j = j0 + lane;
        bool on = j < n;
        const unsigned id = on ? ids[j] : 0;
        if (id >= n_sets) on = false;                      // (never: ids stay below n_sets)
        u64 live = __ballot(on);
        for (int round = 0; round < 2 && live; round++) {
            const int src = __ffsll((i64)live) - 1;
            const unsigned k0 = (unsigned)__builtin_amdgcn_readlane((int)id, src);
            const u64 eq = __ballot(on && id == k0);
            live &= ~eq;
            if (lane == 0) {
                if (k0 < GM_LDS_IDS) atomicAdd(lds_cnt + k0, (unsigned)__popcll(eq));
                else atomicAdd(sizes + k0, (unsigned)__popcll(eq));
            }
        }
        if ((live >> lane) & 1ull) {
            if (id < GM_LDS_IDS) atomicAdd(lds_cnt + id, 1u);
            else atomicAdd(sizes + id, 1u);
        }
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < GM_LDS_IDS && i < n_sets; i += 256) {
        const unsigned v = lds_cnt[i];
        if (v) atomicAdd(sizes + i, v);
    }
}

void sbwt_launch_gm_sizes(const unsigned *d_ids, long long n, long long n_sets, unsigned *d_sizes, hipStream_t stream) {
    (void)hipMemsetAsync(d_sizes, 0, (size_t)n_sets * 4, stream);
    hipLaunchKernelGGL(k_gm_sizes, dim3(gm_stride_grid(n, 2048)), dim3(256), 0, stream, d_ids, (i64)n, (unsigned)n_sets, d_sizes);
}

// wv[t]: in (w64 == nullptr) the sizes, out the weights; iota[t] = t when it is given
__global__ void __launch_bounds__(256) k_gm_weights(const i64 *__restrict__ w64, unsigned *__restrict__ wv, unsigned *__restrict__ iota,
                                                    i64 n_sets, SbwtGmHeader *__restrict__ hdr) {
    u64 used = 0;
    unsigned top = 0;
    for (i64 t0 = (i64)blockIdx.x * 256 + (threadIdx.x & ~63u); t0 < n_sets; t0 += (i64)gridDim.x * 256) {
        const i64 t = t0 + (threadIdx.x & 63);
        unsigned v = 0;
        if (t < n_sets && t != 0) {
            if (w64) {
                const i64 x = w64[t];
                if (x < 0 || x > 0x7fffffffll) atomicMin(&hdr->status, (u64)t);
                else v = (unsigned)x;
            } else {
                v = wv[t];
            }
        }
        if (t < n_sets) {
            wv[t] = v;
            if (iota) iota[t] = (unsigned)t;
        }
        used += (u64)__popcll(__ballot(v != 0));
        top = v > top ? v : top;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)top, off);
        top = o > top ? o : top;
    }
    if ((threadIdx.x & 63) == 0 && used) {
        atomicAdd(&hdr->n_used, used);
        atomicMax(&hdr->max_w, (u64)top);
    }
}

// ---------------------------------------------------------------------------------------------
// few sets: the plain route
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_gm_plain(const u64 *__restrict__ table, const unsigned *__restrict__ wv, i64 n_sets, int words,
                                                  int n_colors, i64 *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const i64 unit = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    const i64 a = unit / words;
    if (a >= n_colors) return;
    const int wb = (int)(unit - a * words), wa = (int)(a >> 6), sa = (int)(a & 63);
    i64 acc = 0;
    for (i64 t = 1; t < n_sets; t++) {
        if (!((table[t * words + wa] >> sa) & 1ull)) continue;           // (the same in every lane)
        if ((table[t * words + wb] >> lane) & 1ull) acc += (i64)wv[t];
    }
    const int b = wb * 64 + lane;
    if (b < n_colors) out[a * n_colors + b] = acc;
}

// ---------------------------------------------------------------------------------------------
// many sets: the matrix cores
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_gm_limbs(const unsigned *__restrict__ sorted, i64 n_sets, i64 k_pad,
                                                  unsigned char *__restrict__ limbs, SbwtGmHeader *__restrict__ hdr) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < k_pad; i += (i64)gridDim.x * 256) {
        const unsigned key = i < n_sets ? sorted[i] : 0, next = i + 1 < n_sets ? sorted[i + 1] : 0;
#pragma unroll
        for (int l = 0; l < 5; l++) {
            limbs[(i64)l * k_pad + i] = (unsigned char)((key >> (7 * l)) & 127u);
            const unsigned thr = 1u << (7 * l);            // (descending weights: one position per limb sees the step)
            if (key >= thr && next < thr) hdr->n_limb[l] = (u64)(i + 1);
        }
    }
}

__global__ void __launch_bounds__(256) k_gm_transpose(const u64 *__restrict__ table, const unsigned *__restrict__ perm, int words,
                                                      int c_pad, const SbwtGmHeader *__restrict__ hdr, u64 *__restrict__ planes) {
    const int lane = threadIdx.x & 63;
    const i64 n_used = (i64)hdr->n_limb[0];
    const i64 n_kb = (n_used + 63) >> 6;
    for (i64 kb = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); kb < n_kb; kb += (i64)gridDim.x * 4) {
        const i64 i = kb * 64 + lane;
        const i64 t = i < n_used ? (i64)perm[i] : 0;       // (row 0 is the empty set: a lane past the end reads zeros)
        for (int w = 0; w < words; w++) {
            const u64 row = table[t * words + w];
            u64 mine = 0;
#pragma unroll 8
            for (int b = 0; b < 64; b++) {
                const u64 bal = __ballot((row >> b) & 1ull);
                if (lane == b) mine = bal;
            }
            planes[kb * c_pad + w * 64 + lane] = mine;
        }
    }
}

typedef int gm_v4i __attribute__((ext_vector_type(4)));

// bits 0..3 of x -> four bytes of 0 or 1
__device__ __forceinline__ unsigned gm_spread4(unsigned x) { return ((x & 15u) * 0x00204081u) & 0x01010101u; }

__device__ __forceinline__ gm_v4i gm_spread16(unsigned bits) {
    gm_v4i v;
    v.x = (int)gm_spread4(bits);
    v.y = (int)gm_spread4(bits >> 4);
    v.z = (int)gm_spread4(bits >> 8);
    v.w = (int)gm_spread4(bits >> 12);
    return v;
}

// planes16: the planes as 16-bit quarters, quarter g of a word = its bits 16 g .. 16 g + 15 (little endian)
__global__ void __launch_bounds__(256) k_gm_mfma(const unsigned short *__restrict__ planes16, const unsigned char *__restrict__ limbs,
                                                 const SbwtGmHeader *__restrict__ hdr, i64 k_pad, int c_pad, int n_tiles, i64 n_pairs,
                                                 i64 chunk_kb, i64 n_splits, u64 *__restrict__ gpad) {
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    i64 unit = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    const i64 per_limb = n_pairs * n_splits;
    if (unit >= per_limb * 5) return;
    const int l = (int)(unit / per_limb);
    unit -= (i64)l * per_limb;
    const i64 split = unit / n_pairs;
    i64 p = unit - split * n_pairs;
    const i64 kb_all = ((i64)hdr->n_limb[l] + 63) >> 6;
    const i64 kb0 = split * chunk_kb;
    const i64 kb1 = kb0 + chunk_kb < kb_all ? kb0 + chunk_kb : kb_all;
    if (kb0 >= kb1) return;
    int ta = 0;
    while (p >= n_tiles - ta) { p -= n_tiles - ta; ta++; }
    const int tb = ta + (int)p;

    gm_v4i acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = gm_v4i{0, 0, 0, 0};
    const unsigned char *lim = limbs + (i64)l * k_pad + g * 16;
    for (i64 kb = kb0; kb < kb1; kb++) {
        const unsigned short *pl = planes16 + kb * c_pad * 4 + g;
        const uint4 lw = *reinterpret_cast<const uint4 *>(lim + kb * 64);
        gm_v4i a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; i++) a[i] = gm_spread16(pl[(ta * 64 + i * 16 + r) * 4]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const gm_v4i m = gm_spread16(pl[(tb * 64 + j * 16 + r) * 4]);
            b[j].x = (int)((unsigned)m.x * 0xFFu & lw.x);
            b[j].y = (int)((unsigned)m.y * 0xFFu & lw.y);
            b[j].z = (int)((unsigned)m.z * 0xFFu & lw.z);
            b[j].w = (int)((unsigned)m.w * 0xFFu & lw.w);
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    // D[row][col]: col = lane & 15, row = 4 (lane >> 4) + register
    const int shift = 7 * l;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int v = acc[i][j][q];
                if (v != 0) atomicAdd(gpad + (i64)(ta * 64 + i * 16 + g * 4 + q) * c_pad + tb * 64 + j * 16 + r, (u64)(unsigned)v << shift);
            }
}

__global__ void __launch_bounds__(256) k_gm_mirror(const i64 *__restrict__ gpad, int c_pad, int n_colors, i64 *__restrict__ out) {
    const i64 total = (i64)n_colors * n_colors;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < total; i += (i64)gridDim.x * 256) {
        const i64 a = i / n_colors, b = i - a * n_colors;
        out[i] = (a >> 6) <= (b >> 6) ? gpad[a * c_pad + b] : gpad[b * c_pad + a];
    }
}

// ---------------------------------------------------------------------------------------------
// the call
// ---------------------------------------------------------------------------------------------
namespace {
struct GmLayout {
    i64 k_pad, c_pad, off_wv, off_iota, off_sorted, off_perm, off_limbs, off_planes, off_gpad, off_tmp, total;
    size_t tmp_bytes;
};

hipError_t gm_layout(i64 n_sets, int n_colors, GmLayout *L) {
    L->k_pad = gm_up(n_sets, 64);
    L->c_pad = gm_up(n_colors, 64);
    L->tmp_bytes = 0;
    const hipError_t e = rocprim::radix_sort_pairs_desc(nullptr, L->tmp_bytes, (const unsigned *)nullptr, (unsigned *)nullptr,
                                                        (const unsigned *)nullptr, (unsigned *)nullptr, (size_t)n_sets, 0u, 32u,
                                                        (hipStream_t)0);
    i64 o = 256;
    L->off_wv = o;      o += gm_up(L->k_pad * 4, 256);
    L->off_iota = o;    o += gm_up(L->k_pad * 4, 256);
    L->off_sorted = o;  o += gm_up(L->k_pad * 4, 256);
    L->off_perm = o;    o += gm_up(L->k_pad * 4, 256);
    L->off_limbs = o;   o += gm_up(L->k_pad * 5, 256);
    L->off_planes = o;  o += gm_up((L->k_pad / 64) * L->c_pad * 8, 256);
    L->off_gpad = o;    o += gm_up(L->c_pad * L->c_pad * 8, 256);
    L->off_tmp = o;     o += gm_up((i64)L->tmp_bytes + 16, 256);
    L->total = o;
    return e;
}

struct GmClock {
    double *ms;
    hipStream_t st;
    std::chrono::steady_clock::time_point t0;
    hipError_t lap(int i) {
        if (!ms) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(st);
        const auto t1 = std::chrono::steady_clock::now();
        ms[i] += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return e;
    }
};
}  // namespace

long long sbwt_gm_workspace_bytes(long long n_sets, int n_colors) {
    GmLayout L;
    if (gm_layout(n_sets, n_colors, &L) != hipSuccess) return -1;
    return L.total;
}

long long sbwt_gm_plain_workspace_bytes(long long n_sets) { return 256 + gm_up(gm_up(n_sets, 64) * 4, 256); }

hipError_t sbwt_gm_enqueue(const unsigned *d_ids, long long n, const unsigned long long *d_table, long long n_sets, int n_colors,
                           const long long *d_weights, long long *d_matrix, void *d_ws, long long ws_bytes, bool use_mfma,
                           long long flush_sets, double *pass_ms, hipStream_t stream) {
    GmLayout L;
    hipError_t e = gm_layout(n_sets, n_colors, &L);
    if (e != hipSuccess) return e;
    if (ws_bytes < (use_mfma ? L.total : L.off_iota)) return hipErrorInvalidValue;
    char *ws = static_cast<char *>(d_ws);
    SbwtGmHeader *hdr = reinterpret_cast<SbwtGmHeader *>(ws);
    unsigned *wv = reinterpret_cast<unsigned *>(ws + L.off_wv), *iota = reinterpret_cast<unsigned *>(ws + L.off_iota);
    unsigned *sorted = reinterpret_cast<unsigned *>(ws + L.off_sorted), *perm = reinterpret_cast<unsigned *>(ws + L.off_perm);
    unsigned char *limbs = reinterpret_cast<unsigned char *>(ws + L.off_limbs);
    u64 *planes = reinterpret_cast<u64 *>(ws + L.off_planes), *gpad = reinterpret_cast<u64 *>(ws + L.off_gpad);
    const int words = (n_colors + 63) / 64, c_pad = (int)L.c_pad;
    GmClock clock{pass_ms, stream, std::chrono::steady_clock::now()};
    if (pass_ms) pass_ms[0] = pass_ms[1] = pass_ms[2] = pass_ms[3] = 0;

    if ((e = hipMemsetAsync(hdr, 0, 256, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(&hdr->status, 0xFF, 8, stream)) != hipSuccess) return e;
    if (!d_weights) {
        sbwt_launch_gm_sizes(d_ids, n, n_sets, wv, stream);
        if ((e = clock.lap(0)) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_gm_weights, dim3(gm_stride_grid(n_sets, 2048)), dim3(256), 0, stream, (const i64 *)d_weights, wv,
                       use_mfma ? iota : (unsigned *)nullptr, (i64)n_sets, hdr);
    if (!use_mfma) {
        if ((e = clock.lap(1)) != hipSuccess) return e;
        const i64 units = (i64)n_colors * words;
        hipLaunchKernelGGL(k_gm_plain, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, stream, (const u64 *)d_table, (const unsigned *)wv,
                           (i64)n_sets, words, n_colors, (i64 *)d_matrix);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        return clock.lap(2);
    }

    e = rocprim::radix_sort_pairs_desc(ws + L.off_tmp, L.tmp_bytes, (const unsigned *)wv, sorted, (const unsigned *)iota, perm, (size_t)n_sets,
                                       0u, 32u, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_gm_limbs, dim3(gm_stride_grid(L.k_pad, 4096)), dim3(256), 0, stream, (const unsigned *)sorted, (i64)n_sets, L.k_pad,
                       limbs, hdr);
    const i64 n_kb = L.k_pad / 64;
    hipLaunchKernelGGL(k_gm_transpose, dim3((unsigned)((n_kb + 3) / 4 > 16384 ? 16384 : (n_kb + 3) / 4)), dim3(256), 0, stream,
                       (const u64 *)d_table, (const unsigned *)perm, words, c_pad, (const SbwtGmHeader *)hdr, planes);
    if ((e = hipMemsetAsync(gpad, 0, (size_t)(L.c_pad * L.c_pad * 8), stream)) != hipSuccess) return e;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = clock.lap(1)) != hipSuccess) return e;

    // a wave's K chunk: enough waves to fill the chip, no chunk so short that its 4096 adds outweigh its products, none longer
    // than the flush interval
    const int n_tiles = c_pad / 64;
    const i64 n_pairs = (i64)n_tiles * (n_tiles + 1) / 2;
    const i64 want = n_pairs >= 4096 ? 1 : 4096 / n_pairs;
    i64 chunk = gm_up((L.k_pad + want - 1) / want, 64);
    if (chunk < 1024) chunk = 1024;
    const i64 cap = flush_sets < 64 ? 64 : flush_sets / 64 * 64;      // (64 sets: one K block, 127 * 64 fits whatever was asked)
    if (chunk > cap) chunk = cap;
    const i64 chunk_kb = chunk / 64, n_splits = (n_kb + chunk_kb - 1) / chunk_kb;
    const i64 n_units = n_pairs * n_splits * 5;
    if ((n_units + 3) / 4 >= ((i64)1 << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gm_mfma, dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, stream, (const unsigned short *)planes,
                       (const unsigned char *)limbs, (const SbwtGmHeader *)hdr, L.k_pad, c_pad, n_tiles, n_pairs, chunk_kb, n_splits, gpad);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = clock.lap(2)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_gm_mirror, dim3(gm_stride_grid((i64)n_colors * n_colors, 8192)), dim3(256), 0, stream, (const i64 *)gpad, c_pad,
                       n_colors, (i64 *)d_matrix);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return clock.lap(3);
}
