// sbwt_colors.hip -- the colour matrix of an index (one 64-bit row per column, bit c = "the column's k-mer was given for
// reference c") and pseudoalignment over it: which references hold a read.  The search kernels are used as they are; what is
// here turns their int32 results into bits of the matrix (colouring) and into one record per read (the query).
//
//   k_col_mark     result -> bit: one lane per result; a lane loads its row and issues the 64-bit atomic OR only when the bit is
//                  still clear (a reference's k-mers repeat, and adding is idempotent, so most lanes issue none)
//   k_col_stats    coloured columns in total and per colour, one pass over the rows
//   k_col_clean    an uploaded matrix: bits >= n_colors and the rows of dummy columns are cleared
//   k_pa_reduce    results + rows + out_off -> records (and counts): one wave per read, lane l takes window 64 it + l -- one
//                  coalesced 256-byte load of results, one 8-byte gather per lane; lane c owns count_c, which grows by the
//                  popcount of a ballot of bit c per iteration.  An iteration whose non-zero rows are all equal (reads from one
//                  strain) adds one popcount to the lanes of that row's bits instead.
//   k_pa_reduce_wide  the same for rows of `words` 64-bit words (up to 4096 colours): a lane gathers the words of its window's row
//                  one after the other; per word, lane c owns the count of colour 64 w + c -- word 0's in a register, the others
//                  in LDS at [wave][w - 1][lane]; the fast path is decided word by word
// The matrix is n x words little-endian words, row-major; words = 1 is the 64-colour matrix, and the kernels that take `words`
// do with 1 what they did before they took it.
// Either strand: the mirrored batch of sbwt_readhits.hip is searched into a second result buffer; window p's second result
// lies at W - 1 - p, and the two rows are ORed.
#include "sbwt_colwalk.h"
#include "sbwt_colors.h"

static inline long long pa_a256(long long x) { return (x + 255) & ~255ll; }

SbwtPaLayout sbwt_pa_layout(long long search_ws_bytes, long long total_bases, long long n_reads, int strands) {
    SbwtPaLayout L;
    long long p = pa_a256(search_ws_bytes);
    L.hdr = p; p += (long long)sizeof(SbwtPaHeader);
    L.res = p; p += pa_a256(total_bases * 4 + 64);
    L.cnt = p; p += pa_a256((n_reads + 1) * 8);
    L.ooff = p; p += pa_a256((n_reads + 1) * 8);
    L.bsum = p; p += pa_a256((n_reads / 1024 + 3) * 8);
    L.res2 = L.rc = L.roff2 = L.ooff2 = 0;
    if (strands == 2) {
        L.res2 = p; p += pa_a256(total_bases * 4 + 64);
        L.rc = p; p += pa_a256(total_bases + 16);
        L.roff2 = p; p += pa_a256((n_reads + 1) * 8);
        L.ooff2 = p; p += pa_a256((n_reads + 1) * 8);
    }
    L.total = p;
    return L;
}

// grid for a grid-stride loop over n items: enough blocks to fill the chip, no more
static inline unsigned col_stride_grid(i64 n) {
    const i64 g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : g > 8192 ? 8192 : g);
}

__global__ void k_pa_note_status(const SbwtWorkHeader *__restrict__ search_ws, SbwtPaHeader *__restrict__ hdr) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && hdr->status == 0 && search_ws->status != 0) hdr->status = search_ws->status;
}

// ---------------------------------------------------------------------------------------------
// colouring
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_col_mark(const int *__restrict__ res, const int *__restrict__ other,
                                                  const i64 *__restrict__ out_off, i64 n_reads, u64 *rows, i64 n_nodes, int words,
                                                  int color, int count, SbwtPaHeader *__restrict__ hdr) {
    const i64 W = out_off[n_reads];
    const u64 bit = 1ull << (color & 63);
    const i64 word = color >> 6;
    u64 mine = 0;                                          // windows with a hit, of this lane's wave (kept by its lane 0)
    // (whole waves go round together: the bound is rounded up to the wave, and a lane past W sits the ballot out)
    for (i64 i0 = (i64)blockIdx.x * 256 + (threadIdx.x & ~63u); i0 < W; i0 += (i64)gridDim.x * 256) {
        const i64 i = i0 + (threadIdx.x & 63);
        bool hit = false;
        if (i < W) {
            const i64 v = res[i];
            if (v >= 0 && v < n_nodes) {
                hit = true;
                u64 *row = rows + (v * (i64)words + word);
                if (!(*row & bit)) atomicOr(row, bit);
            }
            if (count && !hit && other) hit = other[W - 1 - i] >= 0;
        }
        if (count) mine += (u64)__popcll(__ballot(hit));
    }
    if (count && mine && (threadIdx.x & 63) == 0) atomicAdd(&hdr->n_hit, mine);
}

// One pass over the matrix.  A wave takes 64 rows, lane l row j0 + l, and walks their words: for word w, lane c gets the number
// of the 64 rows with bit c by one ballot per colour and adds it to the block's counter [w][c] in LDS (dynamic: words x 64
// uint32; a block sees fewer than 2^32 rows); the OR of a lane's words says whether its row counts as coloured.  The block's
// counters go to `stats` with one atomic add per non-zero entry at the end.
__global__ void __launch_bounds__(256) k_col_stats(const u64 *__restrict__ rows, i64 n, int words, u64 *__restrict__ stats) {
    extern __shared__ unsigned col_stats_cnt[];
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < words * 64; i += 256) col_stats_cnt[i] = 0;
    __syncthreads();
    u64 any = 0;
    for (i64 j0 = (i64)blockIdx.x * 256 + (threadIdx.x & ~63u); j0 < n; j0 += (i64)gridDim.x * 256) {
        const i64 j = j0 + lane;
        const u64 *row = rows + j * (i64)words;
        u64 all = 0;
        for (int w = 0; w < words; w++) {
            const u64 word = j < n ? row[w] : 0;
            all |= word;
            if (!__ballot(word != 0)) continue;
            unsigned mine = 0;
            for (int c = 0; c < 64; c++) {
                const u64 b = __ballot((word >> c) & 1ull);
                if (lane == c) mine = (unsigned)__popcll(b);
            }
            if (mine) atomicAdd(col_stats_cnt + w * 64 + lane, mine);
        }
        any += (u64)__popcll(__ballot(all != 0));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < words * 64; i += 256)
        if (col_stats_cnt[i]) atomicAdd(stats + i, (u64)col_stats_cnt[i]);
    if (lane == 0 && any) atomicAdd(stats + (i64)words * 64, any);
}

// grid-stride over the n x words words of the matrix (64-bit indices: n < 2^31 columns of up to 64 words); `keep` masks the last
// word of a row
__global__ void __launch_bounds__(256) k_col_clean(u64 *__restrict__ rows, i64 n, int words, const unsigned char *__restrict__ lev,
                                                   u64 keep) {
    const i64 total = n * (i64)words;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < total; i += (i64)gridDim.x * 256) {
        const i64 j = i / words;
        const u64 v = rows[i];
        const u64 w = (j == 0 || lev[j] != 0) ? 0 : (i - j * words == words - 1 ? (v & keep) : v);      // (the root is a dummy whatever k is)
        if (w != v) rows[i] = w;
    }
}

hipError_t sbwt_colors_clean(const SbwtIndexView &ix, unsigned long long *d_rows, int n_colors, hipStream_t stream) {
    const bool mega = ix.n_mega > 1 || ix.force_mega;
    const i64 n = ix.n_nodes;
    const unsigned g = grid_for(n);
    unsigned char *lev = nullptr;
    hipError_t e = hipMalloc((void **)&lev, (size_t)(n + 256));
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(lev, 0, (size_t)(n + 256), stream);
    if (e == hipSuccess) {
        for (int r = 0; r + 1 < ix.k; r++) {
            if (mega) hipLaunchKernelGGL(k_ut_level<true>, dim3(g), dim3(256), 0, stream, ix, lev, r);
            else hipLaunchKernelGGL(k_ut_level<false>, dim3(g), dim3(256), 0, stream, ix, lev, r);
        }
        const int words = (n_colors + 63) / 64;
        const u64 keep = (n_colors & 63) == 0 ? ~0ull : ((1ull << (n_colors & 63)) - 1ull);
        hipLaunchKernelGGL(k_col_clean, dim3(col_stride_grid(n * words)), dim3(256), 0, stream, (u64 *)d_rows, n, words,
                           (const unsigned char *)lev, keep);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(stream);
    (void)hipFree(lev);
    return e != hipSuccess ? e : e2;
}

// ---------------------------------------------------------------------------------------------
// results + rows -> records
// ---------------------------------------------------------------------------------------------
typedef unsigned u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));

template <bool TWO>
__global__ void __launch_bounds__(256) k_pa_reduce(const int *__restrict__ res, const int *__restrict__ res2,
                                                   const i64 *__restrict__ out_off, i64 n_reads, const u64 *__restrict__ rows,
                                                   i64 n_nodes, int n_colors, int ppm, int denominator,
                                                   SbwtPseudoalignment *__restrict__ out, int *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const i64 n_waves = (i64)gridDim.x * 4;
    const i64 W = out_off[n_reads];
    for (i64 r = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); r < n_reads; r += n_waves) {
        const i64 s = out_off[r];
        const i64 m = out_off[r + 1] - s;                 // (< 2^31: a read has fewer bases than that)
        int count = 0, found = 0;                         // lane c: count_c; every lane: n_found
        for (i64 q0 = 0; q0 < m; q0 += 64) {
            const i64 q = q0 + lane;
            u64 row = 0;
            if (q < m) {
                const i64 p = s + q;
                const i64 v = res[p];
                if (v >= 0 && v < n_nodes) row = rows[v];
                if (TWO) {
                    const i64 v2 = res2[W - 1 - p];
                    if (v2 >= 0 && v2 < n_nodes) row |= rows[v2];
                }
            }
            const u64 nz = __ballot(row != 0);
            if (!nz) continue;
            const int nf = __popcll(nz);
            found += nf;
            // the first non-zero row of the iteration, in scalar registers; are the others equal to it?
            const int src = __ffsll((i64)nz) - 1;
            const u64 first = (u64)(unsigned)__shfl((int)(unsigned)row, src) | ((u64)(unsigned)__shfl((int)(unsigned)(row >> 32), src) << 32);
            if (!__ballot(row != 0 && row != first)) {
                if ((first >> lane) & 1ull) count += nf;
            } else {
                for (int c = 0; c < n_colors; c++) {
                    const u64 b = __ballot((row >> c) & 1ull);
                    if (lane == c) count += __popcll(b);
                }
            }
        }
        const i64 D = denominator ? m : (i64)found;
        const bool set = lane < n_colors && D > 0 && (u64)count * 1000000ull >= (u64)ppm * (u64)D;
        const u64 colors = __ballot(set);
        if (lane == 0) {
            const u32x4_a8 v = {(unsigned)colors, (unsigned)(colors >> 32), (unsigned)m, (unsigned)found};
            __builtin_nontemporal_store(v, reinterpret_cast<u32x4_a8 *>(out + r));
        }
        if (counts && lane < n_colors) __builtin_nontemporal_store(count, counts + r * n_colors + lane);
    }
}

// Rows of `words` words.  `cnt` (dynamic LDS): [4 waves][words - 1][64 lanes] int32; a lane reads and writes its own entries only,
// so the waves of a block need no barrier.  Word 0's counts stay in a register, as in k_pa_reduce.
template <bool TWO>
__global__ void __launch_bounds__(256) k_pa_reduce_wide(const int *__restrict__ res, const int *__restrict__ res2,
                                                        const i64 *__restrict__ out_off, i64 n_reads, const u64 *__restrict__ rows,
                                                        i64 n_nodes, int words, int n_colors, int ppm, int denominator,
                                                        int2 *__restrict__ out, u64 *__restrict__ colors, int *__restrict__ counts) {
    extern __shared__ int pa_wide_cnt[];
    const int lane = threadIdx.x & 63;
    int *cnt = pa_wide_cnt + (size_t)(threadIdx.x >> 6) * (size_t)(words - 1) * 64 + lane;        // [w - 1] at cnt[(w - 1) * 64]
    const i64 n_waves = (i64)gridDim.x * 4;
    const i64 W = out_off[n_reads];
    for (i64 r = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); r < n_reads; r += n_waves) {
        const i64 s = out_off[r];
        const i64 m = out_off[r + 1] - s;                 // (< 2^31: a read has fewer bases than that)
        int count0 = 0, found = 0;                        // lane c: count_c of word 0; every lane: n_found
        for (int w = 1; w < words; w++) cnt[(w - 1) * 64] = 0;
        for (i64 q0 = 0; q0 < m; q0 += 64) {
            const i64 q = q0 + lane;
            const u64 *ra = nullptr, *rb = nullptr;       // the rows of this lane's window: forward hit, mirrored hit
            if (q < m) {
                const i64 p = s + q;
                const i64 v = res[p];
                if (v >= 0 && v < n_nodes) ra = rows + v * (i64)words;
                if (TWO) {
                    const i64 v2 = res2[W - 1 - p];
                    if (v2 >= 0 && v2 < n_nodes) rb = rows + v2 * (i64)words;
                }
            }
            if (!__ballot(ra != nullptr || rb != nullptr)) continue;
            u64 all = 0;                                  // the OR of the row's words: a window is found when some word is not 0
            u64 next = (ra ? ra[0] : 0) | (TWO && rb ? rb[0] : 0);
            for (int w = 0; w < words; w++) {
                const u64 word = next;
                if (w + 1 < words) next = (ra ? ra[w + 1] : 0) | (TWO && rb ? rb[w + 1] : 0);
                all |= word;
                const u64 nz = __ballot(word != 0);
                if (!nz) continue;
                // this word of the first row that has it non-zero, in scalar registers; are the others' equal to it?
                const int src = __ffsll((i64)nz) - 1;
                const u64 first = (u64)(unsigned)__shfl((int)(unsigned)word, src) | ((u64)(unsigned)__shfl((int)(unsigned)(word >> 32), src) << 32);
                int inc = 0;
                if (!__ballot(word != 0 && word != first)) {
                    if ((first >> lane) & 1ull) inc = __popcll(nz);
                } else {
                    const int nc = min(64, n_colors - w * 64);
                    for (int c = 0; c < nc; c++) {
                        const u64 b = __ballot((word >> c) & 1ull);
                        if (lane == c) inc = __popcll(b);
                    }
                }
                if (w == 0) count0 += inc;
                else if (inc) cnt[(w - 1) * 64] += inc;
            }
            found += __popcll(__ballot(all != 0));
        }
        const i64 D = denominator ? m : (i64)found;
        u64 mine = 0;                                     // lane w: word w of the read's colours
        for (int w = 0; w < words; w++) {
            const int count = w == 0 ? count0 : cnt[(w - 1) * 64];
            const bool live = w * 64 + lane < n_colors;
            const u64 b = __ballot(live && D > 0 && (u64)count * 1000000ull >= (u64)ppm * (u64)D);
            if (lane == w) mine = b;
            if (counts && live) __builtin_nontemporal_store(count, counts + r * n_colors + w * 64 + lane);
        }
        if (lane < words) __builtin_nontemporal_store(mine, colors + r * words + lane);
        if (lane == 0) out[r] = make_int2((int)m, found);
    }
}

// ---------------------------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------------------------
void sbwt_launch_pa_note_status(const SbwtWorkHeader *search_ws, SbwtPaHeader *hdr, hipStream_t stream) {
    hipLaunchKernelGGL(k_pa_note_status, dim3(1), dim3(64), 0, stream, search_ws, hdr);
}

void sbwt_launch_col_mark(const int *d_res, const int *d_other, const long long *d_out_off, long long n_reads, long long max_results,
                          unsigned long long *d_rows, long long n_nodes, int words, int color, int count, SbwtPaHeader *hdr,
                          hipStream_t stream) {
    hipLaunchKernelGGL(k_col_mark, dim3(col_stride_grid(max_results)), dim3(256), 0, stream, d_res, d_other, d_out_off, (i64)n_reads,
                       (u64 *)d_rows, (i64)n_nodes, words, color, count, hdr);
}

void sbwt_launch_col_stats(const unsigned long long *d_rows, long long n_nodes, int words, unsigned long long *d_stats,
                           hipStream_t stream) {
    hipLaunchKernelGGL(k_col_stats, dim3(col_stride_grid(n_nodes)), dim3(256), (size_t)words * 64 * sizeof(unsigned), stream,
                       (const u64 *)d_rows, (i64)n_nodes, words, (u64 *)d_stats);
}

void sbwt_launch_pa_reduce(const int *d_res, const int *d_res2, const long long *d_out_off, long long n_reads,
                           const unsigned long long *d_rows, long long n_nodes, int n_colors, int threshold_ppm, int denominator,
                           SbwtPseudoalignment *d_out, int *d_counts, hipStream_t stream) {
    // a block's four waves take four reads per round
    const i64 gb = (n_reads + 3) / 4;
    const dim3 grid((unsigned)(gb < 1 ? 1 : gb > (1 << 20) ? (1 << 20) : gb)), block(256);
    if (d_res2)
        hipLaunchKernelGGL((k_pa_reduce<true>), grid, block, 0, stream, d_res, d_res2, d_out_off, (i64)n_reads, (const u64 *)d_rows,
                           (i64)n_nodes, n_colors, threshold_ppm, denominator, d_out, d_counts);
    else
        hipLaunchKernelGGL((k_pa_reduce<false>), grid, block, 0, stream, d_res, d_res2, d_out_off, (i64)n_reads, (const u64 *)d_rows,
                           (i64)n_nodes, n_colors, threshold_ppm, denominator, d_out, d_counts);
}

void sbwt_launch_pa_reduce_wide(const int *d_res, const int *d_res2, const long long *d_out_off, long long n_reads,
                                const unsigned long long *d_rows, long long n_nodes, int words, int n_colors, int threshold_ppm,
                                int denominator, SbwtReadFound *d_out, unsigned long long *d_colors, int *d_counts, hipStream_t stream) {
    const i64 gb = (n_reads + 3) / 4;
    const dim3 grid((unsigned)(gb < 1 ? 1 : gb > (1 << 20) ? (1 << 20) : gb)), block(256);
    const size_t lds = (size_t)4 * 64 * (size_t)(words - 1) * sizeof(int);      // at most 63 KiB (words <= 64)
    if (d_res2)
        hipLaunchKernelGGL((k_pa_reduce_wide<true>), grid, block, lds, stream, d_res, d_res2, d_out_off, (i64)n_reads,
                           (const u64 *)d_rows, (i64)n_nodes, words, n_colors, threshold_ppm, denominator, (int2 *)d_out, (u64 *)d_colors,
                           d_counts);
    else
        hipLaunchKernelGGL((k_pa_reduce_wide<false>), grid, block, lds, stream, d_res, d_res2, d_out_off, (i64)n_reads,
                           (const u64 *)d_rows, (i64)n_nodes, words, n_colors, threshold_ppm, denominator, (int2 *)d_out, (u64 *)d_colors,
                           d_counts);
}
