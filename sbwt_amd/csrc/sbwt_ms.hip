// sbwt_ms.hip -- k-bounded matching statistics (MS) and the longest-common-suffix (LCS) array they contract with.
//
// Column j of the index has the label L_j: its k characters, '$'-padded on the left for dummies, L_0 = $^k, in colex order.
// lcs[j] (1 <= j < n) is the length of the longest common suffix of L_{j-1} and L_j, '$' never counting; lcs[0] = 0, and the
// device array holds one more entry, lcs[n] = 0, so that a contraction may read lcs[r + 1] for any interval [l, r].
//
// For a read s and each position i, MS gives len[i]: the largest d <= k such that s[i-d+1 .. i] is upper-case ACGT and a
// suffix of some label (for a string over ACGT of length <= k that is the same as being a substring of an indexed k-mer:
// every column is reachable from the root along the dummy chains, so every prefix of a k-mer ends some label), and the colex
// interval [first[i], second[i]] of the labels that end with that suffix ([0, n-1] when len[i] == 0).
//
// Both kernels read the 64-byte blocks and C only (sbwt_device.h), so they serve every image level and the big layout.
#include "sbwt_kernels_common.h"
#include "sbwt_ms.h"

// ---------------------------------------------------------------------------------------------
// LCS construction
// ---------------------------------------------------------------------------------------------
static inline unsigned stride_grid(i64 n) {
    const i64 g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : g > (1 << 20) ? (1 << 20) : g);
}

// last character of a non-root column's label: the C range that holds it
__device__ __forceinline__ int last_char(const SbwtIndexView &ix, i64 v) {
    return (v >= ix.C[1]) + (v >= ix.C[2]) + (v >= ix.C[3]);
}

// pred[C[c] + rank_c(u)] = u for every column u and every c in its set: the one column every non-root column is entered
// from.  The lanes of a wave share a block, so the four quads are one 64-byte line; the stores form four ascending streams.
template <bool MEGA, typename P>
__global__ void __launch_bounds__(256) k_lcs_pred(SbwtIndexView ix, P *__restrict__ pred) {
    const i64 n = ix.n_nodes;
    for (i64 u = (i64)blockIdx.x * 256 + threadIdx.x; u < n; u += (i64)gridDim.x * 256) {
        const uint4 *blk = ix.blocks + ((u >> 6) << 2);
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const uint4 q = blk[c];
            if ((quad_bits(q) >> (u & 63)) & 1ull) pred[quad_rank<MEGA>(ix, q, u, c)] = (P)u;
        }
    }
}

// one lane per j: walk L_{j-1} and L_j back through pred while their last characters agree.  The two columns never meet
// (colex order of the predecessors follows that of the labels), and only the smaller one can reach the root.
template <typename P>
__global__ void __launch_bounds__(256) k_lcs_walk(SbwtIndexView ix, const P *__restrict__ pred, unsigned char *__restrict__ lcs) {
    const i64 n = ix.n_nodes;
    const int cap = ix.k - 1;
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j <= n; j += (i64)gridDim.x * 256) {
        int d = 0;
        if (j >= 1 && j < n) {
            i64 a = j - 1, b = j;
            while (d < cap && a != 0 && b < n && last_char(ix, a) == last_char(ix, b)) {
                a = (i64)pred[a];
                b = (i64)pred[b];
                d++;
            }
        }
        lcs[j] = (unsigned char)d;
    }
}

long long sbwt_lcs_scratch_bytes(long long n_nodes) {
    return (n_nodes <= 0xFFFFFFFFll ? 4 : 8) * (n_nodes + 1);
}

void sbwt_launch_build_lcs(const SbwtIndexView &ix, void *d_scratch, unsigned char *d_lcs, hipStream_t stream) {
    const bool mega = ix.n_mega > 1 || ix.force_mega;
    const unsigned g1 = stride_grid(ix.n_nodes), g2 = stride_grid(ix.n_nodes + 1);
    if (ix.n_nodes <= 0xFFFFFFFFll) {
        unsigned *pred = static_cast<unsigned *>(d_scratch);
        if (mega) hipLaunchKernelGGL((k_lcs_pred<true, unsigned>), dim3(g1), dim3(256), 0, stream, ix, pred);
        else hipLaunchKernelGGL((k_lcs_pred<false, unsigned>), dim3(g1), dim3(256), 0, stream, ix, pred);
        hipLaunchKernelGGL((k_lcs_walk<unsigned>), dim3(g2), dim3(256), 0, stream, ix, (const unsigned *)pred, d_lcs);
    } else {
        u64 *pred = static_cast<u64 *>(d_scratch);
        if (mega) hipLaunchKernelGGL((k_lcs_pred<true, u64>), dim3(g1), dim3(256), 0, stream, ix, pred);
        else hipLaunchKernelGGL((k_lcs_pred<false, u64>), dim3(g1), dim3(256), 0, stream, ix, pred);
        hipLaunchKernelGGL((k_lcs_walk<u64>), dim3(g2), dim3(256), 0, stream, ix, (const u64 *)pred, d_lcs);
    }
}

// ---------------------------------------------------------------------------------------------
// Matching statistics
// ---------------------------------------------------------------------------------------------
// The bases of the batch are cut into chunks of `chunk` output positions (global base offsets, chunk-aligned); one lane
// answers one chunk.  Where a chunk starts inside a read the lane first walks up to k-1 bases before it (len[i] depends on
// s[i-k+1 .. i] only), so a 1 Mbp read is answered by a thousand lanes and 150 bp reads by one lane per few reads.
//
// Per base the state (d, l, r) -- the match length and the interval of its labels -- is updated as follows:
//   d == k: contract to k-1 first (one column holds the k-mer; its suffix group holds the edges);
//   extend: l' = C[c] + rank_c(l), r' = C[c] + rank_c(r+1) - 1 (k_update_interval);
//   on failure with d > 0: d' = max(lcs[l], lcs[r+1]), widen [l, r] to the maximal range whose inner lcs values are >= d',
//   and retry.  The widening scans at most SBWT_MS_SCAN_WORDS 8-byte words of lcs on each side; past that the interval
//   of the last d' bases is recomputed from [0, n-1] with d' LF steps (short matches have wide intervals: a 3-mer's is
//   ~n/64 columns).
#define SBWT_MS_SCAN_WORDS 16

// bit b of the result: byte b of w is < dd
__device__ __forceinline__ unsigned bytes_below(u64 w, unsigned dd) {
    unsigned m = 0;
#pragma unroll
    for (int b = 0; b < 8; b++) m |= (((unsigned)(w >> (8 * b)) & 0xFFu) < dd ? 1u : 0u) << b;
    return m;
}

// widen [l, r] to the maximal range whose inner lcs values are >= dd (1 <= dd): false if the scan bound was reached
__device__ __forceinline__ bool ms_widen(const unsigned char *__restrict__ lcs, unsigned dd, i64 &l, i64 &r) {
    const u64 *w = reinterpret_cast<const u64 *>(lcs);
    // left: the largest p <= l with lcs[p] < dd (lcs[0] = 0 stops it)
    {
        i64 wi = l >> 3;
        unsigned m = bytes_below(w[wi], dd) & ((2u << (l & 7)) - 1u);
        int s = 0;
        while (m == 0) {
            if (++s > SBWT_MS_SCAN_WORDS) return false;
            m = bytes_below(w[--wi], dd);
        }
        l = (wi << 3) + (31 - __clz(m));
    }
    // right: the smallest p >= r + 1 with lcs[p] < dd (lcs[n] = 0 stops it); r = p - 1
    {
        const i64 p0 = r + 1;
        i64 wi = p0 >> 3;
        unsigned m = bytes_below(w[wi], dd) & (0xFFu << (p0 & 7));
        int s = 0;
        while (m == 0) {
            if (++s > SBWT_MS_SCAN_WORDS) return false;
            m = bytes_below(w[++wi], dd);
        }
        r = (wi << 3) + (__ffs(m) - 1) - 1;
    }
    return true;
}

// interval of s[from .. from+len) (upper-case ACGT) from [0, n-1]
template <bool MEGA>
__device__ __forceinline__ void ms_recompute(const SbwtIndexView &ix, const char *__restrict__ bases, i64 from, int len, i64 &l, i64 &r) {
    l = 0;
    r = ix.n_nodes - 1;
    for (int t = 0; t < len && l <= r; t++) {
        const int c = (int)dna_code((unsigned char)bases[from + t]);
        const uint4 q1 = ix.blocks[((l >> 6) << 2) + c];
        const uint4 q2 = ix.blocks[(((r + 1) >> 6) << 2) + c];
        l = (i64)quad_rank<MEGA>(ix, q1, l, c);
        r = (i64)quad_rank<MEGA>(ix, q2, r + 1, c) - 1;
    }
}

// len bytes leave four at a time: one 4-byte store per aligned word the lane fills, byte stores at its chunk's edges
struct MsLenPack {
    unsigned word = 0, mask = 0;
    i64 at = -1;
    __device__ __forceinline__ void flush(unsigned char *out, bool aligned) {
        if (mask == 0xFu && aligned) {
            __builtin_nontemporal_store(word, reinterpret_cast<unsigned *>(out + at));
        } else {
            for (int b = 0; b < 4; b++)
                if ((mask >> b) & 1u) out[at + b] = (unsigned char)(word >> (8 * b));
        }
        mask = 0;
        word = 0;
    }
    __device__ __forceinline__ void put(unsigned char *out, bool aligned, i64 i, unsigned v) {
        const i64 a = i & ~(i64)3;
        if (a != at) {
            if (mask) flush(out, aligned);
            at = a;
        }
        word |= v << (8 * (i & 3));
        mask |= 1u << (i & 3);
    }
};

template <bool MEGA, bool IV>
__global__ void __launch_bounds__(256) k_ms(SbwtIndexView ix, const unsigned char *__restrict__ lcs, const char *__restrict__ bases,
                                            const i64 *__restrict__ read_off, i64 n_reads, i64 chunk, i64 n_chunks,
                                            unsigned char *__restrict__ len_out, i64 *__restrict__ first,
                                            i64 *__restrict__ second, SbwtMsWork *ws) {
    const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 b0 = read_off[0], b1 = read_off[n_reads];
    const i64 c0 = (b0 & ~(i64)63) + t * chunk;
    i64 p = c0 > b0 ? c0 : b0;
    const i64 pend = (c0 + chunk < b1) ? c0 + chunk : b1;
    u64 n_walk = 0, n_contract = 0, n_recompute = 0, n_full = 0, n_out = 0;
    if (t < n_chunks && p < pend) {
        // the read that holds p: read_off[r] <= p < read_off[r + 1]
        i64 lo = 0, hi = n_reads;
        while (hi - lo > 1) {
            const i64 mid = lo + ((hi - lo) >> 1);
            if (read_off[mid] <= p) lo = mid; else hi = mid;
        }
        i64 r = lo;
        const int k = ix.k;
        const i64 n = ix.n_nodes;
        const bool al = ((uintptr_t)len_out & 3) == 0;
        MsLenPack pk;
        while (p < pend) {
            const i64 rs = read_off[r], re = read_off[r + 1];
            const i64 stop = re < pend ? re : pend;
            i64 i = p - (k - 1) > rs ? p - (k - 1) : rs;
            int d = 0;
            i64 l = 0, rr = n - 1;
            u64 cw = ~0ull, wv = 0;
            for (; i < stop; i++) {
                // 8 bases per load: the 8-byte aligned word that holds base i (it never leaves the page of a valid byte)
                const u64 ad = (u64)(uintptr_t)(bases + i);
                if ((ad >> 3) != cw) {
                    cw = ad >> 3;
                    wv = *reinterpret_cast<const u64 *>((uintptr_t)(cw << 3));
                }
                const unsigned b = (unsigned)(wv >> (8 * (ad & 7))) & 0xFFu;
                n_walk++;
                if (!is_ACGT(b)) {
                    d = 0; l = 0; rr = n - 1;
                } else {
                    const int c = (int)dna_code(b);
                    if (d == k) {
                        n_contract++;
                        d = k - 1;
                        if (d == 0) { l = 0; rr = n - 1; }
                        else if (!ms_widen(lcs, (unsigned)d, l, rr)) { n_recompute++; ms_recompute<MEGA>(ix, bases, i - d, d, l, rr); }
                    }
                    for (;;) {
                        const uint4 q1 = ix.blocks[((l >> 6) << 2) + c];
                        const uint4 q2 = ix.blocks[(((rr + 1) >> 6) << 2) + c];
                        const i64 nl = (i64)quad_rank<MEGA>(ix, q1, l, c);
                        const i64 nr = (i64)quad_rank<MEGA>(ix, q2, rr + 1, c) - 1;
                        if (nl <= nr) { l = nl; rr = nr; d++; break; }
                        if (d == 0) break;                   // c ends no label: len 0, the full range
                        n_contract++;
                        const unsigned a = lcs[l], z = lcs[rr + 1];
                        int dd = (int)(a > z ? a : z);
                        if (dd == 0) { d = 0; l = 0; rr = n - 1; continue; }
                        // (a maximal interval has outer lcs values < d; anything else would stall the loop: recompute)
                        if (dd >= d) { dd = d - 1; n_recompute++; ms_recompute<MEGA>(ix, bases, i - dd, dd, l, rr); }
                        else if (!ms_widen(lcs, (unsigned)dd, l, rr)) { n_recompute++; ms_recompute<MEGA>(ix, bases, i - dd, dd, l, rr); }
                        d = dd;
                    }
                }
                if (i >= p) {
                    pk.put(len_out, al, i, (unsigned)d);
                    if (IV) {
                        st_stream(first + i, l);
                        st_stream(second + i, rr);
                    }
                    n_out++;
                    n_full += (d == k);
                }
            }
            p = stop;
            r++;
        }
        if (pk.mask) pk.flush(len_out, al);
    }
    // per-launch counters (ms_bench.py): one atomic per wave and counter
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        n_walk += __shfl_xor(n_walk, s);
        n_contract += __shfl_xor(n_contract, s);
        n_recompute += __shfl_xor(n_recompute, s);
        n_full += __shfl_xor(n_full, s);
        n_out += __shfl_xor(n_out, s);
    }
    if ((threadIdx.x & 63) == 0 && n_walk) {
        atomicAdd(&ws->n_walk, n_walk);
        atomicAdd(&ws->n_contract, n_contract);
        atomicAdd(&ws->n_recompute, n_recompute);
        atomicAdd(&ws->n_full, n_full);
        atomicAdd(&ws->n_out, n_out);
    }
}

long long sbwt_ms_chunk(long long total_bases, int k) {
    long long c = total_bases >= ((long long)1 << 26) ? 1024 : 256;
    while (c < 4ll * k) c *= 2;
    return c;
}

void sbwt_launch_ms(const SbwtIndexView &ix, const unsigned char *d_lcs, const char *d_bases, long long total_bases,
                    const long long *d_read_off, long long n_reads, unsigned char *d_len, long long *d_first,
                    long long *d_second, SbwtMsWork *ws, hipStream_t stream) {
    if (n_reads <= 0 || total_bases <= 0) return;
    const bool mega = ix.n_mega > 1 || ix.force_mega;
    const i64 chunk = sbwt_ms_chunk(total_bases, ix.k);
    // chunks start at multiples of `chunk` from read_off[0] rounded down to 64: one more covers the rounding
    const i64 n_chunks = (total_bases + 63) / chunk + 2;
    const unsigned g = grid_for(n_chunks);
    if (d_first) {
        if (mega) hipLaunchKernelGGL((k_ms<true, true>), dim3(g), dim3(256), 0, stream, ix, d_lcs, d_bases, d_read_off, (i64)n_reads, chunk, n_chunks, d_len, d_first, d_second, ws);
        else hipLaunchKernelGGL((k_ms<false, true>), dim3(g), dim3(256), 0, stream, ix, d_lcs, d_bases, d_read_off, (i64)n_reads, chunk, n_chunks, d_len, d_first, d_second, ws);
    } else {
        if (mega) hipLaunchKernelGGL((k_ms<true, false>), dim3(g), dim3(256), 0, stream, ix, d_lcs, d_bases, d_read_off, (i64)n_reads, chunk, n_chunks, d_len, (i64 *)nullptr, (i64 *)nullptr, ws);
        else hipLaunchKernelGGL((k_ms<false, false>), dim3(g), dim3(256), 0, stream, ix, d_lcs, d_bases, d_read_off, (i64)n_reads, chunk, n_chunks, d_len, (i64 *)nullptr, (i64 *)nullptr, ws);
    }
}
