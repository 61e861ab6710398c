// sbwt_genotype.hip -- genotyping a read set at the bubbles (include/sbwtgpu.h, "genotype"): an
// accumulator that lives across batches -- one uint64 hit counter per k-mer of every bubble branch, three scalars -- and the
// passes that turn it into per-branch vectors, calls and per-colour vectors.  Everything is an integer sum, so no result
// depends on the order in which lanes, waves, batches or host threads arrive.
//
// The build (once per object; three streaming passes and two scans):
//   k_gt_slots     records -> slot table (unitig -> slot 2 i + j, 0xFFFFFFFF elsewhere) and the n_kmers of every slot, with
//                  the check that the records fit the handle: through an error word, nothing is read back per record.
//   k_scan_*       n_kmers in slot order -> branch_off (sbwt_scan.h)
//   k_gt_bitmap    col_unitig -> the branch bitmap, one bit per column, and the popcount of every word
//   k_scan_*       popcounts -> the branch columns before every word
//   k_gt_pos       per branch column, in column order, its position p = branch_off[slot] + col_offset; the scan's int64
//                  prefix narrowed to the uint32 rank directory
// The bitmap (n / 8 bytes) and the directory (n / 16 bytes) are what an add gathers from: they stay in L2 where col_unitig
// (4 n bytes) would not.
//
//   k_gt_add       the search's int32 results (and the mirrored batch's) -> the accumulator, one launch per add, in the frame
//                  of k_sc_add: a wave takes GT_SPAN consecutive results, 64 per iteration.  Per hit one gather, the word of
//                  the bitmap; only for a set bit the directory entry plus a popcount give the rank, the rank gives p, and
//                  one 64-bit atomic adds to kmer_hits[p].  Equal positions in one iteration meet at the atomic unit: a read
//                  that runs along a branch hits consecutive positions.  The scalars are counted by ballot and popcount and
//                  added once per wave.
//   k_gt_branches  kmer_hits -> seen, hits, min_hits: one wave per slot (branches are short)
//   k_gt_calls     one lane per bubble applies the two integer tests; with colours, lane = colour within a word as in
//                  k_sc_expand: the informative words inter[2 i] ^ inter[2 i + 1] and the call are broadcast one by one, the
//                  block's four waves meet in LDS, then one atomic per colour and vector.
#include "sbwt_kernels_common.h"
#include "sbwt_genotype.h"
#include "sbwt_scan.h"

#define GT_SPAN 2048            // results a wave takes at a stretch
#define GT_NONE 0xFFFFFFFFu

__device__ __forceinline__ u64 gt_readlane64(u64 v, int src) {
    return (u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src) |
           ((u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src) << 32);
}

// ---------------------------------------------------------------------------------------------
// the build
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_gt_slots(const SbwtBubble *__restrict__ rec, i64 n_slots, const i64 *__restrict__ off,
                                                  i64 n_unitigs, i64 k, unsigned *slot_of, i64 *__restrict__ nk, unsigned *err) {
    const i64 s = (i64)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_slots) return;
    const SbwtBubble b = rec[s >> 1];
    const unsigned u = b.branch[s & 1], n = b.n_kmers[s & 1];
    nk[s] = (i64)n;
    if ((i64)u >= n_unitigs || (i64)n != off[u + 1] - off[u] - (k - 1)) {
        atomicOr(err, (unsigned)SBWT_GT_BAD_UNITIG);
        return;
    }
    if (atomicExch(slot_of + u, (unsigned)s) != GT_NONE) atomicOr(err, (unsigned)SBWT_GT_BAD_SHARED);
}

// one wave per word of the bitmap (whole waves go round together)
__global__ void __launch_bounds__(256) k_gt_bitmap(const unsigned *__restrict__ col_unitig, i64 n_nodes, i64 n_unitigs,
                                                   const unsigned *__restrict__ slot_of, u64 *__restrict__ bitmap, i64 n_words,
                                                   i64 *__restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    for (i64 w = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); w < n_words; w += (i64)gridDim.x * 4) {
        const i64 v = w * 64 + lane;
        bool on = false;
        if (v < n_nodes) {
            const unsigned cu = col_unitig[v];
            on = (i64)cu < n_unitigs && slot_of[cu] != GT_NONE;
        }
        const u64 bits = __ballot(on);
        if (lane == 0) {
            bitmap[w] = bits;
            cnt[w] = (i64)__popcll(bits);
        }
    }
}

__global__ void __launch_bounds__(256) k_gt_pos(const unsigned *__restrict__ col_unitig, const unsigned *__restrict__ col_offset,
                                                const unsigned *__restrict__ slot_of, const i64 *__restrict__ branch_off,
                                                const u64 *__restrict__ bitmap, i64 n_words, const i64 *__restrict__ pre,
                                                unsigned *__restrict__ dir, unsigned *__restrict__ pos, i64 n_positions, unsigned *err) {
    const int lane = threadIdx.x & 63;
    for (i64 w = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); w < n_words; w += (i64)gridDim.x * 4) {
        const u64 bits = bitmap[w];
        const i64 before = pre[w];
        if (lane == 0) dir[w] = (unsigned)before;
        if ((bits >> lane) & 1ull) {
            const i64 v = w * 64 + lane;
            const unsigned s = slot_of[col_unitig[v]];         // (a set bit: the column has a unitig and the unitig a slot)
            const i64 lo = branch_off[s], o = (i64)col_offset[v];
            const i64 r = before + (i64)__popcll(bits & low_mask(lane));
            if (o >= branch_off[s + 1] - lo || r >= n_positions) atomicOr(err, (unsigned)SBWT_GT_BAD_COLUMNS);
            else pos[r] = (unsigned)(lo + o);
        }
    }
}

void sbwt_genotype_free(SbwtGenotypeState *s) {
    if (s->d_acc) (void)hipFree(s->d_acc);
    if (s->d_branch_off) (void)hipFree(s->d_branch_off);
    if (s->d_bitmap) (void)hipFree(s->d_bitmap);
    if (s->d_dir) (void)hipFree(s->d_dir);
    if (s->d_pos) (void)hipFree(s->d_pos);
    if (s->d_inter) (void)hipFree(s->d_inter);
    *s = SbwtGenotypeState();
}

static void gt_scan(const i64 *in, i64 n, i64 *out, i64 *bsum, hipStream_t st) {
    const unsigned gb = (unsigned)((n + 1023) / 1024);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(gb), dim3(256), 0, st, in, n, bsum);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, st, bsum, (i64)gb);
    hipLaunchKernelGGL(k_scan_apply, dim3(gb), dim3(256), 0, st, in, n, (const i64 *)bsum, out);
}

static unsigned gt_grid(i64 items, i64 per_block, i64 cap) {
    const i64 g = (items + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

hipError_t sbwt_genotype_build(const SbwtGenotypeGraph &g, SbwtGenotypeState *out, int *bad, hipStream_t stream) {
    *out = SbwtGenotypeState();
    *bad = 0;
    SbwtGenotypeState S;
    S.n_bubbles = g.n_bubbles;
    S.n_nodes = g.n_nodes;
    const i64 n_slots = 2 * g.n_bubbles, n_words = (g.n_nodes + 63) / 64;
    const i64 n_scan = n_slots > n_words ? n_slots : n_words;
    // scratch: [err, 256 bytes][slot_of][nk][cnt][pre][bsum]
    const size_t o_slot = 256, o_nk = o_slot + (((size_t)g.n_unitigs * 4 + 255) & ~(size_t)255),
                 o_cnt = o_nk + (((size_t)n_slots * 8 + 255) & ~(size_t)255), o_pre = o_cnt + (((size_t)n_words * 8 + 255) & ~(size_t)255),
                 o_bsum = o_pre + (((size_t)(n_words + 1) * 8 + 255) & ~(size_t)255),
                 scratch_bytes = o_bsum + ((size_t)((n_scan + 1023) / 1024) + 2) * 8;
    char *scratch = nullptr;
    hipError_t e = hipMalloc((void **)&scratch, scratch_bytes);
    auto fail = [&](hipError_t err) {
        (void)hipStreamSynchronize(stream);
        if (scratch) (void)hipFree(scratch);
        sbwt_genotype_free(&S);
        return err;
    };
    if (e == hipSuccess) e = hipMalloc((void **)&S.d_branch_off, (size_t)(n_slots + 1) * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&S.d_bitmap, (size_t)n_words * 8 + 8);
    if (e == hipSuccess) e = hipMalloc((void **)&S.d_dir, (size_t)n_words * 4 + 4);
    if (e == hipSuccess && g.d_inter && g.words > 0 && n_slots > 0) {
        const size_t bytes = (size_t)n_slots * (size_t)g.words * 8;
        e = hipMalloc((void **)&S.d_inter, bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(S.d_inter, g.d_inter, bytes, hipMemcpyDeviceToDevice, stream);
    }
    if (e != hipSuccess) return fail(e);
    unsigned *err = reinterpret_cast<unsigned *>(scratch), *slot_of = reinterpret_cast<unsigned *>(scratch + o_slot);
    i64 *nk = reinterpret_cast<i64 *>(scratch + o_nk), *cnt = reinterpret_cast<i64 *>(scratch + o_cnt),
        *pre = reinterpret_cast<i64 *>(scratch + o_pre), *bsum = reinterpret_cast<i64 *>(scratch + o_bsum);
    if ((e = hipMemsetAsync(scratch, 0, 256, stream)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(slot_of, 0xFF, (size_t)g.n_unitigs * 4, stream)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(S.d_branch_off, 0, (size_t)(n_slots + 1) * 8, stream)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(pre, 0, (size_t)(n_words + 1) * 8, stream)) != hipSuccess) return fail(e);
    if (n_slots > 0) {
        hipLaunchKernelGGL(k_gt_slots, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, stream, g.d_rec, n_slots, (const i64 *)g.d_off,
                           (i64)g.n_unitigs, (i64)g.k, slot_of, nk, err);
        gt_scan(nk, n_slots, S.d_branch_off, bsum, stream);
    }
    if (n_words > 0) {
        hipLaunchKernelGGL(k_gt_bitmap, dim3(gt_grid(n_words, 4, 4096)), dim3(256), 0, stream, g.d_col_unitig, (i64)g.n_nodes,
                           (i64)g.n_unitigs, (const unsigned *)slot_of, S.d_bitmap, n_words, cnt);
        gt_scan(cnt, n_words, pre, bsum, stream);
    }
    if ((e = hipGetLastError()) != hipSuccess) return fail(e);
    // P, the branch columns of the map and the error word come back before what P sizes is allocated
    i64 P = 0, R = 0;
    unsigned herr = 0;
    if ((e = hipMemcpyAsync(&P, S.d_branch_off + n_slots, 8, hipMemcpyDeviceToHost, stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(&R, pre + n_words, 8, hipMemcpyDeviceToHost, stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(&herr, err, 4, hipMemcpyDeviceToHost, stream)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return fail(e);
    if (herr == 0 && R != P) herr = SBWT_GT_BAD_COLUMNS;
    if (herr) {
        *bad = (int)herr;
        return fail(hipSuccess);
    }
    S.n_positions = P;
    S.acc_bytes = 256 + (size_t)P * 8;
    if ((e = hipMalloc((void **)&S.d_acc, S.acc_bytes)) != hipSuccess) return fail(e);
    if ((e = hipMalloc((void **)&S.d_pos, (size_t)P * 4 + 4)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(S.d_acc, 0, S.acc_bytes, stream)) != hipSuccess) return fail(e);
    if (n_words > 0) {
        hipLaunchKernelGGL(k_gt_pos, dim3(gt_grid(n_words, 4, 4096)), dim3(256), 0, stream, g.d_col_unitig, g.d_col_offset,
                           (const unsigned *)slot_of, (const i64 *)S.d_branch_off, (const u64 *)S.d_bitmap, n_words, (const i64 *)pre, S.d_dir,
                           S.d_pos, P, err);
        if ((e = hipGetLastError()) != hipSuccess) return fail(e);
    }
    if ((e = hipMemcpyAsync(&herr, err, 4, hipMemcpyDeviceToHost, stream)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return fail(e);
    if (herr) {
        *bad = (int)herr;
        return fail(hipSuccess);
    }
    (void)hipFree(scratch);
    *out = S;
    return hipSuccess;
}

// ---------------------------------------------------------------------------------------------
// results -> accumulator
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_gt_add(const int *__restrict__ res, const int *__restrict__ res2,
                                                const i64 *__restrict__ out_off, i64 n_reads, i64 n_nodes,
                                                const u64 *__restrict__ bitmap, const unsigned *__restrict__ dir,
                                                const unsigned *__restrict__ pos, i64 n_positions, u64 *kmer_hits,
                                                SbwtGenotypeCounters *ctr) {
    const int lane = threadIdx.x & 63;
    const i64 W = out_off[n_reads];
    const i64 total = res2 ? 2 * W : W;                    // the mirrored batch's results follow the forward ones
    if (blockIdx.x == 0 && threadIdx.x == 0 && total > 0) atomicAdd(&ctr->n_windows, (u64)total);
    const i64 n_spans = (total + GT_SPAN - 1) / GT_SPAN;
    u64 hits = 0, site = 0;                                // of this lane's wave (the same in every lane)
    for (i64 g = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); g < n_spans; g += (i64)gridDim.x * 4) {
        const i64 base = g * GT_SPAN;
        for (int it = 0; it < GT_SPAN / 64 && base + it * 64 < total; it++) {
            const i64 i = base + it * 64 + lane;
            i64 v = -1;
            if (i < total) v = i < W ? res[i] : res2[i - W];
            const bool hit = v >= 0 && v < n_nodes;
            bool on = false;
            if (hit) {
                const u64 word = bitmap[v >> 6];
                if ((word >> (v & 63)) & 1ull) {
                    const i64 r = (i64)dir[v >> 6] + (i64)__popcll(word & low_mask((int)(v & 63)));
                    if (r < n_positions) {                 // (always: the directory counts the bits of this bitmap)
                        const unsigned p = pos[r];
                        if ((i64)p < n_positions) {        // (always: the build wrote positions below P)
                            atomicAdd(kmer_hits + p, 1ull);
                            on = true;
                        }
                    }
                }
            }
            hits += (u64)__popcll(__ballot(hit));
            site += (u64)__popcll(__ballot(on));
        }
    }
    if (lane == 0 && hits) atomicAdd(&ctr->n_hits, hits);
    if (lane == 0 && site) atomicAdd(&ctr->n_site_hits, site);
}

void sbwt_launch_genotype_add(const int *d_res, const int *d_res2, const long long *d_out_off, long long n_reads, long long max_results,
                              const SbwtGenotypeState &s, hipStream_t stream) {
    const i64 total = d_res2 ? 2 * max_results : max_results;
    hipLaunchKernelGGL(k_gt_add, dim3(gt_grid(total, 4 * GT_SPAN, 2048)), dim3(256), 0, stream, d_res, d_res2, (const i64 *)d_out_off,
                       (i64)n_reads, (i64)s.n_nodes, (const u64 *)s.d_bitmap, (const unsigned *)s.d_dir, (const unsigned *)s.d_pos,
                       (i64)s.n_positions, (u64 *)s.kmer_hits(), s.ctr());
}

// ---------------------------------------------------------------------------------------------
// accumulator -> per-branch vectors
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_gt_branches(const i64 *__restrict__ branch_off, i64 n_slots, const u64 *__restrict__ kmer_hits,
                                                     i64 *__restrict__ seen, i64 *__restrict__ hits, i64 *__restrict__ min_hits) {
    const int lane = threadIdx.x & 63;
    for (i64 s = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); s < n_slots; s += (i64)gridDim.x * 4) {
        const i64 lo = branch_off[s], hi = branch_off[s + 1];
        u64 sum = 0, n = 0, mn = ~0ull;
        for (i64 p = lo + lane; p < hi; p += 64) {
            const u64 h = kmer_hits[p];
            sum += h;
            n += h != 0;
            mn = h < mn ? h : mn;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            sum += __shfl_down(sum, off);
            n += __shfl_down(n, off);
            const u64 o = __shfl_down(mn, off);
            mn = o < mn ? o : mn;
        }
        if (lane == 0) {
            seen[s] = (i64)n;
            hits[s] = (i64)sum;
            min_hits[s] = hi > lo ? (i64)mn : 0;
        }
    }
}

void sbwt_launch_genotype_branches(const SbwtGenotypeState &s, long long *d_seen, long long *d_hits, long long *d_min, hipStream_t stream) {
    const i64 n_slots = 2 * s.n_bubbles;
    if (n_slots == 0) return;
    hipLaunchKernelGGL(k_gt_branches, dim3(gt_grid(n_slots, 4, 4096)), dim3(256), 0, stream, (const i64 *)s.d_branch_off, n_slots,
                       (const u64 *)s.kmer_hits(), (i64 *)d_seen, (i64 *)d_hits, (i64 *)d_min);
}

// ---------------------------------------------------------------------------------------------
// per-branch vectors -> calls and per-colour vectors
// ---------------------------------------------------------------------------------------------
// allele present: seen * 10^6 >= breadth_ppm * n and hits >= min_depth * n, the second as hits / n >= min_depth (the same
// for integers, and it cannot overflow)
__device__ __forceinline__ bool gt_present(i64 seen, i64 hits, i64 n, i64 ppm, i64 min_depth) {
    if (seen * 1000000 < ppm * n) return false;
    return n == 0 || hits / n >= min_depth;
}

// grid: x slices the bubbles, y = the word of colours (1 without colours)
__global__ void __launch_bounds__(256) k_gt_calls(const i64 *__restrict__ branch_off, const i64 *__restrict__ seen,
                                                  const i64 *__restrict__ hits, i64 n_bubbles, i64 ppm, i64 min_depth,
                                                  const u64 *__restrict__ inter, int words, int n_colors,
                                                  unsigned char *__restrict__ call_out, u64 *__restrict__ ref) {
    __shared__ u64 part[3][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w = blockIdx.y;
    u64 a0 = 0, a1 = 0, a2 = 0;                            // lane l: colour 64 w + l
    for (i64 i0 = ((i64)blockIdx.x * 4 + wave) * 64; i0 < n_bubbles; i0 += (i64)gridDim.x * 256) {
        const i64 i = i0 + lane;
        unsigned call = 0;
        u64 x = 0, ra = 0;
        if (i < n_bubbles) {
            const i64 o0 = branch_off[2 * i], o1 = branch_off[2 * i + 1], o2 = branch_off[2 * i + 2];
            if (gt_present(seen[2 * i], hits[2 * i], o1 - o0, ppm, min_depth)) call |= 1u;
            if (gt_present(seen[2 * i + 1], hits[2 * i + 1], o2 - o1, ppm, min_depth)) call |= 2u;
            if (w == 0 && call_out) call_out[i] = (unsigned char)call;
            if (ref && call) {
                ra = inter[(2 * i) * words + w];
                x = ra ^ inter[(2 * i + 1) * words + w];
            }
        }
        u64 left = __ballot(x != 0);
        while (left) {                                     // one trip per called bubble with an informative colour in this word
            const int src = __ffsll((i64)left) - 1;
            left &= left - 1;
            const u64 bits = gt_readlane64(x, src), in_a = gt_readlane64(ra, src);
            const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)call, src);
            if ((bits >> lane) & 1ull) {
                const unsigned mine = ((in_a >> lane) & 1ull) ? 1u : 2u;    // the allele this colour carries, as a call bit
                a0 += 1;
                a1 += (c & mine) != 0;
                a2 += c == mine;
            }
        }
    }
    if (!ref) return;
    part[0][wave][lane] = a0;
    part[1][wave][lane] = a1;
    part[2][wave][lane] = a2;
    __syncthreads();
    if (threadIdx.x < 192) {
        const int v = threadIdx.x >> 6;                    // wave v adds up vector v
        const u64 s = part[v][0][lane] + part[v][1][lane] + part[v][2][lane] + part[v][3][lane];
        const int c = w * 64 + lane;
        if (c < n_colors && s) atomicAdd(ref + (i64)v * n_colors + c, s);
    }
}

void sbwt_launch_genotype_calls(const SbwtGenotypeState &s, const long long *d_seen, const long long *d_hits, int breadth_ppm,
                                long long min_depth, int words, int n_colors, unsigned char *d_call, unsigned long long *d_ref,
                                hipStream_t stream) {
    if (d_ref) (void)hipMemsetAsync(d_ref, 0, (size_t)3 * (size_t)n_colors * 8, stream);
    if (s.n_bubbles == 0) return;
    const int gy = d_ref && words > 0 ? words : 1;
    const i64 cap = 1024 / gy < 1 ? 1 : 1024 / gy;
    const dim3 grid(gt_grid(s.n_bubbles, 256, cap), (unsigned)gy), block(256);
    hipLaunchKernelGGL(k_gt_calls, grid, block, 0, stream, (const i64 *)s.d_branch_off, (const i64 *)d_seen, (const i64 *)d_hits,
                       (i64)s.n_bubbles, (i64)breadth_ppm, (i64)min_depth, (const u64 *)s.d_inter, words, n_colors, d_call, (u64 *)d_ref);
}
