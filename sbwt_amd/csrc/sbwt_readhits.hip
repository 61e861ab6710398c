// sbwt_readhits.hip -- per-read hit profiles: { windows, indexed windows, bases they cover, longest run of hits } per read,
// computed from the results that the search kernels write (they are not touched).
//
// Read r has m_r = max(0, len_r - k + 1) windows; hit[i] = (the search result of window i is >= 0).  The passes:
//   k_rh_counts + k_scan_*   out_off[] from read_off[] and k (the device entry point cannot look at offsets on the host)
//   (search)                 the existing int32 / int64 device route writes W = out_off[n] results
//   k_rh_bits                results -> one bit per window, one 64-bit word per 64 results (one coalesced load + a ballot)
//   k_rh_reduce              bit vector + out_off -> one 16-byte record per read
// Either strand: k_rh_revcomp writes the reverse complement of the WHOLE base buffer (rc[T-1-b] = comp(bases[b])) and
// k_rh_mirror_off the offsets T - read_off[n-j] / W - out_off[n-j]: read r becomes read n-1-r of the mirrored batch and its
// window i lands at result W-1-p (p: its forward position).  The mirrored batch is searched into the same result buffer
// and k_rh_bits ORs result W-1-p into bit p.  No lane ever looks up which read a base belongs to.
//
// The record of a stretch of windows is a monoid (RhSeg below), so a read may be cut anywhere: a lane walks a short read
// word by word, a wave takes a long one 64 words at a time and combines across its lanes.
#include "sbwt_kernels_common.h"
#include "sbwt_readhits.h"
#include "sbwt_scan.h"

static inline long long rh_a256(long long x) { return (x + 255) & ~255ll; }

SbwtRhLayout sbwt_rh_layout(long long search_ws_bytes, long long total_bases, long long n_reads, int strands) {
    SbwtRhLayout L;
    long long p = rh_a256(search_ws_bytes);
    L.hdr = p; p += (long long)sizeof(SbwtRhHeader);
    L.res = p; p += rh_a256(total_bases * 8 + 64);
    L.bits = p; p += rh_a256((total_bases / 64 + 2) * 8);
    L.cnt = p; p += rh_a256((n_reads + 1) * 8);
    L.ooff = p; p += rh_a256((n_reads + 1) * 8);
    L.bsum = p; p += rh_a256((n_reads / 1024 + 3) * 8);
    L.rc = L.roff2 = L.ooff2 = 0;
    if (strands == 2) {
        L.rc = p; p += rh_a256(total_bases + 16);
        L.roff2 = p; p += rh_a256((n_reads + 1) * 8);
        L.ooff2 = p; p += rh_a256((n_reads + 1) * 8);
    }
    L.total = p;
    return L;
}

// grid for a grid-stride loop over n items: enough blocks to fill the chip, no more
static inline unsigned rh_stride_grid(i64 n) {
    const i64 g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : g > 8192 ? 8192 : g);
}

// ---------------------------------------------------------------------------------------------
// offsets
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_rh_counts(const i64 *__restrict__ read_off, i64 n_reads, int k, i64 *__restrict__ cnt) {
    for (i64 r = (i64)blockIdx.x * 256 + threadIdx.x; r < n_reads; r += (i64)gridDim.x * 256) {
        const i64 m = read_off[r + 1] - read_off[r] - k + 1;
        cnt[r] = m > 0 ? m : 0;
    }
}

__global__ void __launch_bounds__(256) k_rh_mirror_off(const i64 *__restrict__ read_off, const i64 *__restrict__ out_off, i64 n_reads,
                                                       i64 total_bases, i64 *__restrict__ roff2, i64 *__restrict__ ooff2) {
    const i64 W = out_off[n_reads];
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j <= n_reads; j += (i64)gridDim.x * 256) {
        roff2[j] = total_bases - read_off[n_reads - j];
        ooff2[j] = W - out_off[n_reads - j];
    }
}

// A <-> T, C <-> G on upper-case bytes; every other byte stays what it is (and so stays no base)
__device__ __forceinline__ unsigned rh_comp(unsigned b) {
    return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : b;
}

// Eight bytes of rc per lane (rc is 8-byte aligned: it lies in the workspace): the source bytes come from the one or two
// aligned 8-byte words that hold them -- each holds a byte of the buffer, so it never leaves a valid byte's page.
__global__ void __launch_bounds__(256) k_rh_revcomp(const char *__restrict__ bases, i64 T, char *__restrict__ rc) {
    const i64 n8 = (T + 7) >> 3;
    for (i64 t = (i64)blockIdx.x * 256 + threadIdx.x; t < n8; t += (i64)gridDim.x * 256) {
        const i64 d = t << 3, s0 = T - 8 - d;
        if (s0 < 0) {                                     // the last lane: fewer than eight bytes are left
            for (i64 j = d; j < T; j++) rc[j] = (char)rh_comp((unsigned char)bases[T - 1 - j]);
            continue;
        }
        const uintptr_t ad = (uintptr_t)(bases + s0), al = ad & ~(uintptr_t)7;
        const int sh = (int)(ad & 7) * 8;
        u64 v = __builtin_nontemporal_load(reinterpret_cast<const u64 *>(al)) >> sh;
        if (sh) v |= __builtin_nontemporal_load(reinterpret_cast<const u64 *>(al + 8)) << (64 - sh);
        u64 o = 0;                                        // byte j of o = comp(byte 7 - j of v)
#pragma unroll
        for (int j = 0; j < 8; j++) o |= (u64)rh_comp((unsigned)(v >> (8 * (7 - j))) & 0xFFu) << (8 * j);
        *reinterpret_cast<u64 *>(rc + d) = o;
    }
}

// ---------------------------------------------------------------------------------------------
// results -> bits
// ---------------------------------------------------------------------------------------------
// A wave takes 64 consecutive words = 4096 results: one coalesced load per lane and a ballot per word, lane w keeps word w,
// and the 64 words leave with one coalesced store.  The results are streamed exactly once.
template <typename R, bool MIRROR>
__global__ void __launch_bounds__(256) k_rh_bits(const R *__restrict__ res, const i64 *__restrict__ out_off, i64 n_reads,
                                                 u64 *__restrict__ bits, const SbwtWorkHeader *__restrict__ search_ws,
                                                 SbwtRhHeader *__restrict__ hdr) {
    const i64 W = out_off[n_reads];
    const i64 n_words = (W + 63) >> 6;
    const int lane = threadIdx.x & 63;
    const i64 n_waves = (i64)gridDim.x * 4;
    if (blockIdx.x == 0 && threadIdx.x == 0 && hdr->status == 0 && search_ws->status != 0) hdr->status = search_ws->status;
    for (i64 g = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); (g << 6) < n_words; g += n_waves) {
        const i64 base = g << 12;
        u64 mine = 0;
#pragma unroll 8
        for (int w = 0; w < 64; w++) {
            const i64 p = base + ((i64)w << 6) + lane;
            bool hit = false;
            if (p < W) hit = __builtin_nontemporal_load(res + (MIRROR ? W - 1 - p : p)) >= 0;
            const u64 b = __ballot(hit);
            if (lane == w) mine = b;
        }
        const i64 wi = (g << 6) + lane;
        if (wi < n_words) bits[wi] = MIRROR ? (bits[wi] | mine) : mine;
    }
}

// ---------------------------------------------------------------------------------------------
// bits -> records
// ---------------------------------------------------------------------------------------------
// What a stretch of n consecutive windows contributes (positions are relative to the read's first window):
//   found                hits
//   pre, suf, best       hits in a row at its start, at its end, anywhere (found == n: every window is a hit)
//   first, last          position of its first and last hit (found > 0)
//   cov                  sum over its hits but the first of min(k, distance to the hit before): the bases each of them adds
//                        to the cover of the ones before.  The stretch's first hit adds k, or less once a stretch with a hit
//                        is joined in front -- that term is added by the join, and k for the read's first hit at the end.
struct RhSeg { int n, found, pre, suf, best, first, last, cov; };

__device__ __forceinline__ RhSeg rh_join(const RhSeg &A, const RhSeg &B, int k) {
    RhSeg R;
    R.n = A.n + B.n;
    R.found = A.found + B.found;
    R.pre = (A.found == A.n) ? A.n + B.pre : A.pre;
    R.suf = (B.found == B.n) ? B.n + A.suf : B.suf;
    const int mid = A.suf + B.pre;
    R.best = max(max(A.best, B.best), mid);
    R.first = A.found ? A.first : B.first;
    R.last = B.found ? B.last : A.last;
    R.cov = A.cov + B.cov + ((A.found && B.found) ? min(k, B.first - A.last) : 0);
    return R;
}

// the stretch of nb <= 64 windows whose hits are the low nb bits of x (the bits above are 0), the first at position a0
__device__ __forceinline__ RhSeg rh_of_chunk(u64 x, int nb, int a0, int k) {
    RhSeg S;
    S.n = nb;
    S.found = __popcll(x);
    S.pre = S.suf = S.best = S.first = S.last = S.cov = 0;
    if (x) {
        S.first = a0 + __ffsll((i64)x) - 1;
        S.last = a0 + 63 - __clzll((i64)x);
        S.pre = (~x) ? __ffsll((i64)~x) - 1 : 64;
        const u64 top = x << (64 - nb);                  // (nb >= 1: x has a bit)
        S.suf = (~top) ? __clzll((i64)~top) : 64;
        // run by run: a run of l hits at t adds min(k, t - previous hit) for its first and 1 for each of the others
        int prev = -1;
        u64 y = x;
        while (y) {
            const int t = __ffsll((i64)y) - 1;
            const u64 u = ~(y >> t);                     // (t zeros shifted in at the top: u != 0 unless t == 0 and y is all ones)
            const int l = u ? __ffsll((i64)u) - 1 : 64;
            if (prev >= 0) S.cov += min(k, t - prev);
            S.cov += l - 1;
            prev = t + l - 1;
            S.best = max(S.best, l);
            if (t + l >= 64) break;
            y &= ~0ull << (t + l);
        }
    }
    return S;
}

// windows [64 j, 64 j + nb) of the read whose first window is bit s of the vector: reads start anywhere inside a word
__device__ __forceinline__ u64 rh_chunk_bits(const u64 *__restrict__ bits, i64 s, int j, int nb) {
    const i64 q = s + ((i64)j << 6);
    const i64 wi = q >> 6;
    const int sh = (int)(q & 63);
    u64 x = bits[wi] >> sh;
    if (sh + nb > 64) x |= bits[wi + 1] << (64 - sh);
    if (nb < 64) x &= (1ull << nb) - 1ull;
    return x;
}

__device__ __forceinline__ RhSeg rh_shfl_down(const RhSeg &S, int off) {
    RhSeg R;
    R.n = __shfl_down(S.n, off); R.found = __shfl_down(S.found, off); R.pre = __shfl_down(S.pre, off); R.suf = __shfl_down(S.suf, off);
    R.best = __shfl_down(S.best, off); R.first = __shfl_down(S.first, off); R.last = __shfl_down(S.last, off); R.cov = __shfl_down(S.cov, off);
    return R;
}

typedef int i32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ void rh_store(SbwtReadHits *out, i64 r, const RhSeg &S, int k) {
    const i32x4_a4 v = {S.n, S.found, S.cov + (S.found ? k : 0), S.best};
    __builtin_nontemporal_store(v, reinterpret_cast<i32x4_a4 *>(out + r));
}

// One lane per read; the reads of wave_min windows or more are then taken one after the other by the whole wave that holds
// them, 64 words per iteration (lane l: chunk 64 it + l), combined by an ordered tree over the lanes.
__global__ void __launch_bounds__(256) k_rh_reduce(const u64 *__restrict__ bits, const i64 *__restrict__ out_off, i64 n_reads, int k,
                                                   int wave_min, SbwtReadHits *__restrict__ out) {
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    const bool valid = r < n_reads;
    const i64 s = valid ? out_off[r] : 0;
    const int m = valid ? (int)(out_off[r + 1] - s) : 0;
    const bool is_long = valid && m >= wave_min;
    if (valid && !is_long) {
        RhSeg acc = {0, 0, 0, 0, 0, 0, 0, 0};
        const int nc = (m + 63) >> 6;
        for (int j = 0; j < nc; j++) {
            const int nb = min(64, m - (j << 6));
            acc = rh_join(acc, rh_of_chunk(rh_chunk_bits(bits, s, j, nb), nb, j << 6, k), k);
        }
        rh_store(out, r, acc, k);
    }
    u64 todo = __ballot(is_long);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int src = __ffsll((i64)todo) - 1;
        todo &= todo - 1;
        const i64 rr = __shfl(r, src), ss = __shfl(s, src);
        const int mm = __shfl(m, src);
        const int nc = (mm + 63) >> 6;
        RhSeg acc = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int j0 = 0; j0 < nc; j0 += 64) {
            const int j = j0 + lane;
            RhSeg S = {0, 0, 0, 0, 0, 0, 0, 0};
            if (j < nc) {
                const int nb = min(64, mm - (j << 6));
                S = rh_of_chunk(rh_chunk_bits(bits, ss, j, nb), nb, j << 6, k);
            }
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) S = rh_join(S, rh_shfl_down(S, off), k);   // lane 0: chunks j0 .. j0 + 63 in order
            acc = rh_join(acc, S, k);
        }
        if (lane == 0) rh_store(out, rr, acc, k);
    }
}

// ---------------------------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------------------------
void sbwt_launch_rh_offsets(const long long *d_read_off, long long n_reads, int k, long long *d_cnt, long long *d_bsum,
                            long long *d_out_off, hipStream_t stream) {
    const unsigned nb = (unsigned)((n_reads + 1023) / 1024);
    hipLaunchKernelGGL(k_rh_counts, dim3(rh_stride_grid(n_reads)), dim3(256), 0, stream, d_read_off, (i64)n_reads, k, d_cnt);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(nb), dim3(256), 0, stream, (const i64 *)d_cnt, (i64)n_reads, d_bsum);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, stream, d_bsum, (i64)nb);
    hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(256), 0, stream, (const i64 *)d_cnt, (i64)n_reads, (const i64 *)d_bsum, d_out_off);
}

void sbwt_launch_rh_mirror(const char *d_bases, long long total_bases, const long long *d_read_off, const long long *d_out_off,
                           long long n_reads, char *d_rc, long long *d_roff2, long long *d_ooff2, hipStream_t stream) {
    if (total_bases > 0)
        hipLaunchKernelGGL(k_rh_revcomp, dim3(rh_stride_grid((total_bases + 7) / 8)), dim3(256), 0, stream, d_bases, (i64)total_bases, d_rc);
    hipLaunchKernelGGL(k_rh_mirror_off, dim3(rh_stride_grid(n_reads + 1)), dim3(256), 0, stream, d_read_off, d_out_off, (i64)n_reads,
                       (i64)total_bases, d_roff2, d_ooff2);
}

void sbwt_launch_rh_bits(const void *d_res, int wide, const long long *d_out_off, long long n_reads, long long max_results,
                         int mirrored, unsigned long long *d_bits, const SbwtWorkHeader *search_ws, SbwtRhHeader *hdr,
                         hipStream_t stream) {
    // a block's four waves take 4 x 4096 results per round
    const i64 groups = (max_results + 4095) / 4096;
    const i64 gb = (groups + 3) / 4;
    const dim3 grid((unsigned)(gb < 1 ? 1 : gb > 8192 ? 8192 : gb)), block(256);
    if (wide) {
        const i64 *res = static_cast<const i64 *>(d_res);
        if (mirrored) hipLaunchKernelGGL((k_rh_bits<i64, true>), grid, block, 0, stream, res, d_out_off, (i64)n_reads, d_bits, search_ws, hdr);
        else hipLaunchKernelGGL((k_rh_bits<i64, false>), grid, block, 0, stream, res, d_out_off, (i64)n_reads, d_bits, search_ws, hdr);
    } else {
        const int *res = static_cast<const int *>(d_res);
        if (mirrored) hipLaunchKernelGGL((k_rh_bits<int, true>), grid, block, 0, stream, res, d_out_off, (i64)n_reads, d_bits, search_ws, hdr);
        else hipLaunchKernelGGL((k_rh_bits<int, false>), grid, block, 0, stream, res, d_out_off, (i64)n_reads, d_bits, search_ws, hdr);
    }
}

void sbwt_launch_rh_reduce(const unsigned long long *d_bits, const long long *d_out_off, long long n_reads, int k, int wave_min,
                           SbwtReadHits *d_out, hipStream_t stream) {
    hipLaunchKernelGGL(k_rh_reduce, dim3(grid_for(n_reads)), dim3(256), 0, stream, (const u64 *)d_bits, d_out_off, (i64)n_reads, k,
                       wave_min, d_out);
}
