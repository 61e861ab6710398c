// sbwt_walks.hip -- reads threaded through the unitig graph: the steps of every read, computed from the
// results that the search kernels write (they are not touched) and the column map of a graph handle.
//
// Window p of the batch (p counts the windows of all reads, W = out_off[n_reads] of them) hits when its result is >= 0; a
// step is a maximal range of hits of one read along one unitig.  Inside a run of hits a step starts exactly where the
// column's offset in its unitig is 0 (section 22 has the argument), so one bit per column decides it:
//   k_wk_startbits            col_offset -> start[]: one bit per column, once per handle
//   k_rh_counts + k_scan_*    out_off[] from read_off[] and k (sbwt_readhits.hip)
//   k_wk_rstart               R: bit out_off[r] for every read with a window
//   (search)                  the int32 device route writes W results
//   k_wk_flags                results -> H (hit), S = H & (R | ~H(p-1) | start[res]) (a step starts), T = H & ~((H & ~S) >> 1)
//                             (a step ends), and the popcounts of every S word and of every R word
//   k_scan_*                  exclusive scans of the popcounts: rank over S and rank over R
//   k_wk_stepoff              step_off[r] = rank_S(out_off[r]); rstart[rank_R(out_off[r])] = out_off[r] for a read with a window
//   k_wk_starts, k_wk_ends    the records: the lane at a start writes unitig, offset, read_pos (its read's first window is
//                             rstart[rank_R(p + 1) - 1]: no search); the lane at the matching end adds what makes n_kmers
// Steps are disjoint and ordered, so the j-th set bit of S and the j-th set bit of T belong to step j, and the number of T
// bits before an end q is the number of S bits at or before q, less one: one scan serves both.  All launches are flat; the
// two fill kernels take a word per lane and its set bits in turn.
#include "sbwt_kernels_common.h"
#include "sbwt_readhits.h"
#include "sbwt_walks.h"
#include "sbwt_scan.h"

static inline long long wk_a256(long long x) { return (x + 255) & ~255ll; }

SbwtWalkLayout sbwt_walk_layout(long long search_ws_bytes, long long total_bases, long long n_reads) {
    SbwtWalkLayout L;
    L.n_words = total_bases / 64 + 2;
    long long p = wk_a256(search_ws_bytes);
    L.res = p; p += wk_a256(total_bases * 4 + 64);
    L.cnt = p; p += wk_a256((n_reads + 1) * 8);
    L.ooff = p; p += wk_a256((n_reads + 1) * 8);
    L.bsum = p; p += wk_a256((n_reads / 1024 + 3) * 8);
    L.rbits = p; p += wk_a256(L.n_words * 8);
    L.sbits = p; p += wk_a256(L.n_words * 8);
    L.tbits = p; p += wk_a256(L.n_words * 8);
    L.wcnt = p; p += wk_a256(L.n_words * 8);
    L.wpre = p; p += wk_a256((L.n_words + 1) * 8);
    L.wsum = p; p += wk_a256((L.n_words / 1024 + 3) * 8);
    L.rcnt = p; p += wk_a256(L.n_words * 8);
    L.rpre = p; p += wk_a256((L.n_words + 1) * 8);
    L.rstart = p; p += wk_a256((n_reads + 1) * 8);
    L.total = p;
    return L;
}

// grid for a grid-stride loop over n items: enough blocks to fill the chip, no more
static inline unsigned wk_stride_grid(i64 n) {
    const i64 g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : g > 8192 ? 8192 : g);
}
// a block's four waves take 4 x 4096 items per round
static inline unsigned wk_wave_grid(i64 n) {
    const i64 gb = ((n + 4095) / 4096 + 3) / 4;
    return (unsigned)(gb < 1 ? 1 : gb > 8192 ? 8192 : gb);
}

// ---------------------------------------------------------------------------------------------
// the handle's start bitmap
// ---------------------------------------------------------------------------------------------
// A wave takes 4096 columns: one coalesced load per lane and a ballot per 64 columns, lane w keeps word w, and the 64 words
// leave with one coalesced store.  A dummy column's offset is 0xFFFFFFFF: no start.
__global__ void __launch_bounds__(256) k_wk_startbits(const unsigned *__restrict__ col_offset, i64 n_nodes, u64 *__restrict__ start) {
    const i64 n_words = (n_nodes + 63) >> 6;
    const int lane = threadIdx.x & 63;
    const i64 n_waves = (i64)gridDim.x * 4;
    for (i64 g = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); (g << 6) < n_words; g += n_waves) {
        const i64 base = g << 12;
        u64 mine = 0;
#pragma unroll 8
        for (int w = 0; w < 64; w++) {
            const i64 v = base + ((i64)w << 6) + lane;
            bool z = false;
            if (v < n_nodes) z = __builtin_nontemporal_load(col_offset + v) == 0u;
            const u64 b = __ballot(z);
            if (lane == w) mine = b;
        }
        const i64 wi = (g << 6) + lane;
        if (wi < n_words) start[wi] = mine;
    }
}

// ---------------------------------------------------------------------------------------------
// read starts
// ---------------------------------------------------------------------------------------------
// (R is zeroed before; reads without a window share their out_off with the next read and set nothing)
__global__ void __launch_bounds__(256) k_wk_rstart(const i64 *__restrict__ out_off, i64 n_reads, u64 *__restrict__ R) {
    for (i64 r = (i64)blockIdx.x * 256 + threadIdx.x; r < n_reads; r += (i64)gridDim.x * 256) {
        const i64 p = out_off[r];
        if (out_off[r + 1] > p) atomicOr(R + (p >> 6), 1ull << (p & 63));
    }
}

// ---------------------------------------------------------------------------------------------
// results -> flags
// ---------------------------------------------------------------------------------------------
// whether column c starts a unitig; a value that is no column of the index counts as a start (its record then says so: the
// fill gives it 0xFFFFFFFF), so nothing outside the bitmap is read whatever the results hold
__device__ __forceinline__ bool wk_start_bit(const u64 *__restrict__ start, i64 n_nodes, int c) {
    if ((i64)c >= n_nodes) return true;
    return (start[c >> 6] >> (c & 63)) & 1ull;
}

// A wave takes 64 consecutive words = 4096 windows, in the shape of k_rh_bits.  The only gather is the start bit, and only
// for hits; it depends on the result alone, so the loads of the unrolled rounds are in flight together.  H(p-1) is the bit
// below in the ballot; the first lane of a word takes the top bit of the word before, the wave's first word reads one more
// result.  T needs S of the window after the wave's last: its last lane works that one window out.
// Words from W's on (n_words of them, a bound the host knows) are written as zeros.
__global__ void __launch_bounds__(256) k_wk_flags(const int *__restrict__ res, const i64 *__restrict__ out_off, i64 n_reads,
                                                  const u64 *__restrict__ start, i64 n_nodes, const u64 *__restrict__ R, i64 n_words,
                                                  u64 *__restrict__ S, u64 *__restrict__ T, i64 *__restrict__ wcnt, i64 *__restrict__ rcnt) {
    const i64 W = out_off[n_reads];
    const int lane = threadIdx.x & 63;
    const i64 n_waves = (i64)gridDim.x * 4;
    for (i64 g = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); (g << 6) < n_words; g += n_waves) {
        const i64 base = g << 12;
        u64 carry = 0;                                   // H of the window before the word
        if (base > 0 && base - 1 < W) carry = res[base - 1] >= 0 ? 1ull : 0ull;
        u64 Hm = 0, Sm = 0, Rm = 0;
#pragma unroll 8
        for (int w = 0; w < 64; w++) {
            const i64 wi = (base >> 6) + w;
            const i64 p = base + ((i64)w << 6) + lane;
            int c = -1;
            if (p < W) c = __builtin_nontemporal_load(res + p);
            const bool hit = c >= 0;
            const bool sb = hit ? wk_start_bit(start, n_nodes, c) : false;
            const u64 h = __ballot(hit);
            const u64 rw = wi < n_words ? R[wi] : 0ull;
            const u64 prev = (h << 1) | carry;
            carry = h >> 63;
            const u64 s = h & (rw | ~prev | __ballot(sb));
            if (lane == w) { Hm = h; Sm = s; Rm = rw; }
        }
        // N: hits that continue the step of the window before; the end of a step is a hit whose next window is not in N
        const u64 N = Hm & ~Sm;
        u64 next0 = __shfl_down(N, 1) & 1ull;
        if (lane == 63) {
            const i64 p1 = base + 4096;
            next0 = 0;
            if (p1 < W) {
                const int c1 = res[p1];
                if (c1 >= 0 && !(R[p1 >> 6] & 1ull) && !wk_start_bit(start, n_nodes, c1)) next0 = 1;
            }
        }
        const u64 Tm = Hm & ~((N >> 1) | (next0 << 63));
        const i64 wi = (g << 6) + lane;
        if (wi < n_words) {
            S[wi] = Sm;
            T[wi] = Tm;
            wcnt[wi] = __popcll(Sm);
            rcnt[wi] = __popcll(Rm);
        }
    }
}

// the number of set bits of S below bit p (wpre: the exclusive scan of the words' popcounts)
__device__ __forceinline__ i64 wk_rank(const u64 *__restrict__ S, const i64 *__restrict__ wpre, i64 p) {
    const int b = (int)(p & 63);
    return wpre[p >> 6] + __popcll(S[p >> 6] & ((1ull << b) - 1ull));
}

// step_off[r] = rank_S(out_off[r]) for r = 0 .. n_reads (out_off[n_reads] = W: its word exists and holds no bit from W on),
// and the first windows of the reads that have one, in order: the j-th set bit of R is at rstart[j]
__global__ void __launch_bounds__(256) k_wk_stepoff(const i64 *__restrict__ out_off, i64 n_reads, const u64 *__restrict__ S,
                                                    const i64 *__restrict__ wpre, const u64 *__restrict__ R, const i64 *__restrict__ rpre,
                                                    i64 *__restrict__ step_off, i64 *__restrict__ rstart) {
    for (i64 r = (i64)blockIdx.x * 256 + threadIdx.x; r <= n_reads; r += (i64)gridDim.x * 256) {
        const i64 p = out_off[r];
        step_off[r] = wk_rank(S, wpre, p);
        if (r < n_reads && out_off[r + 1] > p) rstart[wk_rank(R, rpre, p)] = p;
    }
}

// ---------------------------------------------------------------------------------------------
// flags -> records
// ---------------------------------------------------------------------------------------------
typedef int i32x4_wk __attribute__((ext_vector_type(4), aligned(4)));

// One lane per 64-window word, which takes the word's starts one after the other (a word has 2 or 3 on reads of a pan-genome,
// 64 at most): one lane per window left two or three lanes of a wave active behind a chain of four dependent loads and took
// 5.3 ms where this takes the time of its memory traffic.  The lane at a start p of step s = rank_S(p) does the only full
// gathers, one pair per step, takes its read's first window from rank over R (a binary search in out_off took 24 dependent
// loads per step and most of the call's time) and writes the record with n_kmers = -p (mod 2^32): k_wk_ends adds q + 1 for
// the end q.  (Words from W's on are zeros: no lane needs W.)
__global__ void __launch_bounds__(256) k_wk_starts(const int *__restrict__ res, i64 n_words, const u64 *__restrict__ S,
                                                   const i64 *__restrict__ wpre, const u64 *__restrict__ R, const i64 *__restrict__ rpre,
                                                   const i64 *__restrict__ rstart, const unsigned *__restrict__ col_unitig,
                                                   const unsigned *__restrict__ col_offset, i64 n_nodes, SbwtWalkStep *__restrict__ steps,
                                                   i64 steps_cap) {
    for (i64 w = (i64)blockIdx.x * 256 + threadIdx.x; w < n_words; w += (i64)gridDim.x * 256) {
        u64 x = S[w];
        if (!x) continue;
        i64 s = wpre[w];
        const u64 rw = R[w];
        const i64 j0 = rpre[w] - 1;                      // reads that start before the word, less one
        for (; x && s < steps_cap; x &= x - 1, s++) {
            const int b = __ffsll((i64)x) - 1;
            const i64 p = (w << 6) + b;
            const int c = res[p];
            unsigned un = 0xFFFFFFFFu, of = 0xFFFFFFFFu;
            if ((i64)c < n_nodes) { un = col_unitig[c]; of = col_offset[c]; }
            // (a hit lies in a read, so a read starts at or before p)
            const i64 first = rstart[j0 + __popcll(rw & (b == 63 ? ~0ull : (1ull << (b + 1)) - 1ull))];
            const i32x4_wk v = {(int)un, (int)of, (int)(p - first), (int)(0u - (unsigned)p)};
            *reinterpret_cast<i32x4_wk *>(steps + s) = v;
        }
    }
}

// One lane per word again.  The lane at an end q of step s = (S bits at or before q) - 1 completes n_kmers = q + 1 - p, exact
// in 32-bit wrapping arithmetic because a step is shorter than a read (< 2^31).  Coverage: one 64-bit add per step onto the
// unitig of the end's column, which is the step's.  A step that is not stored (s >= steps_cap) still counts: its start is
// the last S bit at or before q, found by walking the S words back from q -- for callers that gave less room than steps.
__global__ void __launch_bounds__(256) k_wk_ends(const int *__restrict__ res, i64 n_words, const u64 *__restrict__ S,
                                                 const u64 *__restrict__ T, const i64 *__restrict__ wpre,
                                                 const unsigned *__restrict__ col_unitig, i64 n_nodes, SbwtWalkStep *__restrict__ steps,
                                                 i64 steps_cap, i64 *__restrict__ cov) {
    for (i64 w = (i64)blockIdx.x * 256 + threadIdx.x; w < n_words; w += (i64)gridDim.x * 256) {
        u64 t = T[w];
        if (!t) continue;
        const u64 sw = S[w];
        const i64 s0 = wpre[w] - 1;
        for (; t; t &= t - 1) {
            const int b = __ffsll((i64)t) - 1;
            const i64 q = (w << 6) + b;
            const u64 upto = sw & (b == 63 ? ~0ull : (1ull << (b + 1)) - 1ull);
            const i64 s = s0 + __popcll(upto);
            int n;
            if (s < steps_cap) {
                n = (int)((unsigned)steps[s].n_kmers + (unsigned)(q + 1));
                steps[s].n_kmers = n;
            } else {
                if (!cov) break;                         // (the steps of the ends that follow are not stored either)
                i64 v = w;
                u64 x = upto;
                while (!x && v > 0) x = S[--v];
                n = (int)(q - ((v << 6) + 63 - __clzll((i64)x)) + 1);
            }
            if (cov) {
                const int c = res[q];
                if ((i64)c < n_nodes) {
                    const unsigned un = col_unitig[c];
                    if (un != 0xFFFFFFFFu) atomicAdd(reinterpret_cast<u64 *>(cov) + un, (u64)n);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------------------------
void sbwt_launch_walk_startbits(const unsigned *d_col_offset, long long n_nodes, unsigned long long *d_start, hipStream_t stream) {
    hipLaunchKernelGGL(k_wk_startbits, dim3(wk_wave_grid(n_nodes)), dim3(256), 0, stream, d_col_offset, (i64)n_nodes, (u64 *)d_start);
}

hipError_t sbwt_launch_walks(const int *d_res, const long long *d_out_off, long long n_reads, long long total_bases,
                       const unsigned long long *d_start, const unsigned *d_col_unitig, const unsigned *d_col_offset, long long n_nodes,
                       char *d_ws, const SbwtWalkLayout &L, long long *d_step_off, SbwtWalkStep *d_steps, long long steps_cap,
                       long long *d_cov, hipStream_t stream) {
    u64 *R = reinterpret_cast<u64 *>(d_ws + L.rbits), *S = reinterpret_cast<u64 *>(d_ws + L.sbits), *T = reinterpret_cast<u64 *>(d_ws + L.tbits);
    i64 *wcnt = reinterpret_cast<i64 *>(d_ws + L.wcnt), *wpre = reinterpret_cast<i64 *>(d_ws + L.wpre), *wsum = reinterpret_cast<i64 *>(d_ws + L.wsum);
    i64 *rcnt = reinterpret_cast<i64 *>(d_ws + L.rcnt), *rpre = reinterpret_cast<i64 *>(d_ws + L.rpre), *rstart = reinterpret_cast<i64 *>(d_ws + L.rstart);
    const i64 nw = L.n_words;
    const unsigned nb = (unsigned)((nw + 1023) / 1024);
    const hipError_t e = hipMemsetAsync(R, 0, (size_t)nw * 8, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_wk_rstart, dim3(wk_stride_grid(n_reads)), dim3(256), 0, stream, d_out_off, (i64)n_reads, R);
    hipLaunchKernelGGL(k_wk_flags, dim3(wk_wave_grid(nw * 64)), dim3(256), 0, stream, d_res, d_out_off, (i64)n_reads, (const u64 *)d_start,
                       (i64)n_nodes, (const u64 *)R, nw, S, T, wcnt, rcnt);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(nb), dim3(256), 0, stream, (const i64 *)wcnt, nw, wsum);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, stream, wsum, (i64)nb);
    hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(256), 0, stream, (const i64 *)wcnt, nw, (const i64 *)wsum, wpre);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(nb), dim3(256), 0, stream, (const i64 *)rcnt, nw, wsum);      // (wsum: free again)
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, stream, wsum, (i64)nb);
    hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(256), 0, stream, (const i64 *)rcnt, nw, (const i64 *)wsum, rpre);
    hipLaunchKernelGGL(k_wk_stepoff, dim3(wk_stride_grid(n_reads + 1)), dim3(256), 0, stream, d_out_off, (i64)n_reads, (const u64 *)S,
                       (const i64 *)wpre, (const u64 *)R, (const i64 *)rpre, d_step_off, rstart);
    hipLaunchKernelGGL(k_wk_starts, dim3(wk_stride_grid(nw)), dim3(256), 0, stream, d_res, nw, (const u64 *)S, (const i64 *)wpre, (const u64 *)R,
                       (const i64 *)rpre, (const i64 *)rstart, d_col_unitig, d_col_offset, (i64)n_nodes, d_steps, (i64)steps_cap);
    hipLaunchKernelGGL(k_wk_ends, dim3(wk_stride_grid(nw)), dim3(256), 0, stream, d_res, nw, (const u64 *)S, (const u64 *)T, (const i64 *)wpre,
                       d_col_unitig, (i64)n_nodes, d_steps, (i64)steps_cap, d_cov);
    return hipGetLastError();
}
