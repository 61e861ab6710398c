// sbwt_pileup.hip -- the pileup of aligned reads (include/sbwtgpu.h, "pileup of aligned reads").
//
// The accumulate pass gives every read one lane, as k_verify and k_align do: a lane loads its three records, applies the filter
// and walks its runs.  Every coordinate of [ref_begin, ref_end) is exactly one of = X D, so the = columns get no counter: a piled
// read adds +1 and -1 to a difference array at the two ends of its interval, and one 32-bit atomic per X or D column and per
// interior I run.  At read-out the depth is the prefix sum of the difference array and the matches are the depth minus the rest.
//
// The cells lie at the coordinates of the reference object's packed layout (sequence s starts at cell 64 * slot), so a cell
// index is slot * 64 + p with no second table, and the prefix sum runs over ALL cells: the -1 that a read ending at n of a
// sequence of 64 m bases leaves on the next sequence's cell 0 is part of that cell's true prefix.
#include "sbwt_pileup.h"
#include "sbwt_scan.h"
#include "sbwt_verify_text.h"

// ---- accumulate ----------------------------------------------------------------------------------------------------------------
// the code of the oriented read's base j (0 .. 3), VF_NONE for an invalid one or one that is not there
__device__ __forceinline__ unsigned pile_read_code(const char *__restrict__ bases, i64 total, i64 off, i64 L, int strand, i64 j) {
    if ((u64)j >= (u64)L) return VF_NONE;
    const i64 at = strand ? off + L - 1 - j : off + j;
    if ((u64)at >= (u64)total) return VF_NONE;
    const unsigned c = vf_code((unsigned char)bases[at]);
    return (strand && c != VF_NONE) ? 3u - c : c;
}

static __global__ void __launch_bounds__(256) k_pile_add(const char *__restrict__ bases, i64 total, const i64 *__restrict__ read_off, i64 n_reads,
                                                         const SbwtVerifyMap *__restrict__ map, const SbwtReadVerify *__restrict__ ver,
                                                         const SbwtReadAlign *__restrict__ al, const i64 *__restrict__ op_off,
                                                         const unsigned *__restrict__ ops, SbwtPileFilter f, const SbwtRefSeq *__restrict__ tab,
                                                         i64 n_seqs, SbwtPileCell *cells, i64 n_cells, SbwtPileCounters *ctr) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    u64 offered = 0, piled = 0, columns = 0, clipped = 0, overhang = 0;
    if (i < n_reads) {
        offered = 1;
        const SbwtReadAlign a = al[i];
        const SbwtVerifyMap m = map[i];
        bool pile = a.n_ops > 0 && m.seq >= 0 && m.seq < n_seqs && m.votes >= f.min_votes && (f.require_unique == 0 || m.votes > m.votes2);
        if (pile && f.max_edit >= 0) pile = ver[i].edit <= f.max_edit;
        SbwtRefSeq s = {0, 0};
        if (pile) {
            s = tab[m.seq];
            pile = s.slot >= 0 && s.len >= 0 && s.slot * 64 + s.len < n_cells;     // (the cells [g, g + n] are the object's: always, for the object it was made from)
        }
        if (pile) {
            piled = 1;
            const i64 n = s.len, g = s.slot * 64;
            const i64 off = read_off[i], L = read_off[i + 1] - off;
            const int strand = m.strand != 0;
            const unsigned *__restrict__ o = ops + op_off[i];
            i64 p = a.ref_begin, j = 0;
            for (int k = 0; k < a.n_ops; k++) {
                const unsigned op = o[k], code = op & 15u;
                const i64 len = op >> 4;
                if (code == 7u) {
                    p += len;
                    j += len;
                } else if (code == 8u) {
                    for (i64 t = 0; t < len; t++, p++, j++) {
                        if ((u64)p >= (u64)n) { overhang++; continue; }
                        const unsigned c = pile_read_code(bases, total, off, L, strand, j);
                        atomicAdd(c == VF_NONE ? &cells[g + p].other : &cells[g + p].x[c], 1u);
                    }
                } else if (code == 2u) {
                    for (i64 t = 0; t < len; t++, p++) {
                        if ((u64)p >= (u64)n) { overhang++; continue; }
                        atomicAdd(&cells[g + p].del, 1u);
                    }
                } else if (code == 1u) {
                    if (k == 0 || k == a.n_ops - 1) clipped += (u64)len;
                    else if ((u64)(p - 1) < (u64)n) atomicAdd(&cells[g + p - 1].ins, 1u);
                    else overhang++;
                    j += len;
                }
            }
            const i64 lo = a.ref_begin < 0 ? 0 : (a.ref_begin > n ? n : a.ref_begin), hi = p < 0 ? 0 : (p > n ? n : p);
            if (hi > lo) {
                atomicAdd(&cells[g + lo].diff, 1);
                atomicAdd(&cells[g + hi].diff, -1);
                columns = (u64)(hi - lo);
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        offered += __shfl_down(offered, d);
        piled += __shfl_down(piled, d);
        columns += __shfl_down(columns, d);
        clipped += __shfl_down(clipped, d);
        overhang += __shfl_down(overhang, d);
    }
    if ((threadIdx.x & 63) == 0) {
        if (offered) atomicAdd(&ctr->n_offered, offered);
        if (piled) atomicAdd(&ctr->n_piled, piled);
        if (columns) atomicAdd(&ctr->n_columns, columns);
        if (clipped) atomicAdd(&ctr->n_clipped, clipped);
        if (overhang) atomicAdd(&ctr->n_overhang, overhang);
    }
}

// ---- read-out: the depth ---------------------------------------------------------------------------------------------------------
// k_scan_block_sums over the cells' diff
static __global__ void __launch_bounds__(256) k_pile_block_sums(const SbwtPileCell *__restrict__ cells, i64 n_cells, i64 *__restrict__ bsum) {
    __shared__ i64 sh[4];
    const i64 base = (i64)blockIdx.x * SBWT_PILE_BLOCK;
    i64 s = 0;
    for (int t = threadIdx.x; t < SBWT_PILE_BLOCK; t += 256) s += (base + t < n_cells) ? cells[base + t].diff : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// in place: sh[t] becomes the sum of sh[0 .. t] (256 threads; every thread of the block calls it)
__device__ __forceinline__ void pile_scan256(i64 *sh) {
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const i64 add = ((int)threadIdx.x >= off) ? sh[threadIdx.x - off] : 0;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
}

// the depths of the thread's four cells base .. base + 3 of block blk (bsum: the scanned block sums)
__device__ __forceinline__ void pile_depths(const SbwtPileCell *__restrict__ cells, i64 n_cells, const i64 *__restrict__ bsum, i64 blk, i64 base,
                                            i64 *sh, unsigned depth[4]) {
    int d[4];
    i64 loc = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        d[t] = (base + t < n_cells) ? cells[base + t].diff : 0;
        loc += d[t];
    }
    sh[threadIdx.x] = loc;
    pile_scan256(sh);
    i64 run = bsum[blk] + sh[threadIdx.x] - loc;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        run += d[t];
        depth[t] = (unsigned)run;
    }
    __syncthreads();                    // (sh is free again)
}

// the reference's code at coordinate p of the sequence at `slot`, VF_NONE on an invalid base
__device__ __forceinline__ unsigned pile_ref_code(const u64 *__restrict__ bits, const u64 *__restrict__ valid, i64 slot, i64 p) {
    if (!((valid[slot + (p >> 6)] >> (p & 63)) & 1ull)) return VF_NONE;
    return (unsigned)(bits[2 * slot + (p >> 5)] >> (2 * (p & 31))) & 3u;
}

// the record of a cell of depth `depth` whose reference base has code rc: the = columns are what the others leave of the depth
__device__ __forceinline__ SbwtPileBase pile_record(const SbwtPileCell &c, unsigned depth, unsigned rc) {
    SbwtPileBase r;
    r.depth = depth;
    r.n[0] = c.x[0]; r.n[1] = c.x[1]; r.n[2] = c.x[2]; r.n[3] = c.x[3];
    r.n_del = c.del; r.n_ins = c.ins; r.n_other = c.other;
    const unsigned eq = rc != VF_NONE ? depth - (c.x[0] + c.x[1] + c.x[2] + c.x[3] + c.del + c.other) : 0u;
#pragma unroll
    for (unsigned b = 0; b < 4; b++) r.n[b] += b == rc ? eq : 0u;      // (no indexing by rc: the record stays in registers)
    return r;
}

static __global__ void __launch_bounds__(256) k_pile_counts(const SbwtPileCell *__restrict__ cells, i64 n_cells, const i64 *__restrict__ bsum,
                                                            const u64 *__restrict__ bits, const u64 *__restrict__ valid, i64 slot, i64 pos, i64 len,
                                                            i64 b0, SbwtPileBase *__restrict__ out) {
    __shared__ i64 sh[256];
    const i64 blk = b0 + blockIdx.x, base = blk * SBWT_PILE_BLOCK + threadIdx.x * 4, c0 = slot * 64 + pos;
    unsigned depth[4];
    pile_depths(cells, n_cells, bsum, blk, base, sh, depth);
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const i64 q = base + t - c0;
        if (q < 0 || q >= len || base + t >= n_cells) continue;
        out[q] = pile_record(cells[base + t], depth[t], pile_ref_code(bits, valid, slot, pos + q));
    }
}

// ---- read-out: the calls ---------------------------------------------------------------------------------------------------------
// The calls at one valid reference base, in ascending allele: counted, and stored at out when it is not NULL
__device__ __forceinline__ int pile_cell_calls(const SbwtPileBase &r, unsigned rc, int min_depth, int min_alt, int ppm, i64 pos, int seq,
                                               SbwtPileCall *out) {
    if (r.depth < (unsigned)min_depth) return 0;
    const unsigned ref_count = rc == 0 ? r.n[0] : rc == 1 ? r.n[1] : rc == 2 ? r.n[2] : r.n[3];
    int n = 0;
#pragma unroll
    for (int a = 0; a < 6; a++) {
        if ((unsigned)a == rc) continue;
        const unsigned c = a < 4 ? r.n[a] : (a == 4 ? r.n_del : r.n_ins);
        if (c < (unsigned)min_alt || (u64)c * 1000000ull < (u64)ppm * (u64)r.depth) continue;
        if (out) out[n] = SbwtPileCall{pos, seq, a, (int)rc, (int)r.depth, (int)c, (int)ref_count};
        n++;
    }
    return n;
}

template <bool FILL>
static __global__ void __launch_bounds__(256) k_pile_calls(const SbwtPileCell *__restrict__ cells, i64 n_cells, const i64 *__restrict__ bsum,
                                                           const u64 *__restrict__ bits, const u64 *__restrict__ valid,
                                                           const SbwtRefSeq *__restrict__ tab, i64 n_seqs, int min_depth, int min_alt, int ppm,
                                                           i64 *__restrict__ cnt, const i64 *__restrict__ off, SbwtPileCall *__restrict__ out) {
    __shared__ i64 sh[256];
    const i64 blk = blockIdx.x, base = blk * SBWT_PILE_BLOCK + threadIdx.x * 4;
    unsigned depth[4];
    pile_depths(cells, n_cells, bsum, blk, base, sh, depth);
    // the sequence of the thread's first cell: the last one that starts at or before it (sequences start at multiples of 64, so
    // the four cells share it)
    i64 lo = 0, hi = n_seqs;            // tab[lo - 1].slot * 64 <= base < tab[hi].slot * 64
    while (lo < hi) {
        const i64 mid = (lo + hi) >> 1;
        if (tab[mid].slot * 64 <= base) lo = mid + 1; else hi = mid;
    }
    const int seq = (int)lo - 1;
    SbwtRefSeq s = {0, 0};
    if (seq >= 0) s = tab[seq];
    int mine = 0;
    if (seq >= 0) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const i64 p = base + t - s.slot * 64;
            if (p >= s.len || base + t >= n_cells || depth[t] == 0) continue;
            const unsigned rc = pile_ref_code(bits, valid, s.slot, p);
            if (rc == VF_NONE) continue;
            mine += pile_cell_calls(pile_record(cells[base + t], depth[t], rc), rc, min_depth, min_alt, ppm, p, seq, nullptr);
        }
    }
    sh[threadIdx.x] = mine;
    pile_scan256(sh);
    if (!FILL) {
        if (threadIdx.x == 255) cnt[blk] = sh[255];
        return;
    }
    if (mine == 0) return;
    SbwtPileCall *w = out + off[blk] + sh[threadIdx.x] - mine;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const i64 p = base + t - s.slot * 64;
        if (p >= s.len || base + t >= n_cells || depth[t] == 0) continue;
        const unsigned rc = pile_ref_code(bits, valid, s.slot, p);
        if (rc == VF_NONE) continue;
        w += pile_cell_calls(pile_record(cells[base + t], depth[t], rc), rc, min_depth, min_alt, ppm, p, seq, w);
    }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
void sbwt_launch_pile_add(const char *d_bases, long long total_bases, const long long *d_read_off, long long n_reads,
                          const SbwtVerifyMap *d_map, const SbwtReadVerify *d_verify, const SbwtReadAlign *d_align,
                          const long long *d_op_off, const unsigned *d_ops, SbwtPileFilter f, const SbwtRefSeq *tab, long long n_seqs,
                          SbwtPileCell *cells, long long n_cells, SbwtPileCounters *ctr, hipStream_t stream) {
    if (n_reads <= 0) return;
    hipLaunchKernelGGL(k_pile_add, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, stream, d_bases, (i64)total_bases,
                       (const i64 *)d_read_off, (i64)n_reads, d_map, d_verify, d_align, (const i64 *)d_op_off, d_ops, f, tab, (i64)n_seqs, cells,
                       (i64)n_cells, ctr);
}

void sbwt_launch_pile_scan(const SbwtPileCell *cells, long long n_cells, long long *d_bsum, hipStream_t stream) {
    const i64 nb = sbwt_pile_blocks(n_cells);
    hipLaunchKernelGGL(k_pile_block_sums, dim3((unsigned)nb), dim3(256), 0, stream, cells, (i64)n_cells, (i64 *)d_bsum);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, stream, (i64 *)d_bsum, nb);
}

void sbwt_launch_pile_counts(const SbwtPileCell *cells, long long n_cells, const long long *d_bsum, const unsigned long long *d_bits,
                             const unsigned long long *d_valid, long long slot, long long pos, long long len, SbwtPileBase *d_out,
                             hipStream_t stream) {
    if (len <= 0) return;
    const i64 c0 = slot * 64 + pos, b0 = c0 / SBWT_PILE_BLOCK, b1 = (c0 + len - 1) / SBWT_PILE_BLOCK;
    hipLaunchKernelGGL(k_pile_counts, dim3((unsigned)(b1 - b0 + 1)), dim3(256), 0, stream, cells, (i64)n_cells, (const i64 *)d_bsum,
                       (const u64 *)d_bits, (const u64 *)d_valid, (i64)slot, (i64)pos, (i64)len, b0, d_out);
}

void sbwt_launch_pile_calls(const SbwtPileCell *cells, long long n_cells, const long long *d_bsum, const unsigned long long *d_bits,
                            const unsigned long long *d_valid, const SbwtRefSeq *tab, long long n_seqs, int min_depth, int min_alt,
                            int min_frac_ppm, long long *d_cnt, const long long *d_off, SbwtPileCall *d_out, hipStream_t stream) {
    const unsigned nb = (unsigned)sbwt_pile_blocks(n_cells);
    if (!d_out)
        hipLaunchKernelGGL(k_pile_calls<false>, dim3(nb), dim3(256), 0, stream, cells, (i64)n_cells, (const i64 *)d_bsum, (const u64 *)d_bits,
                           (const u64 *)d_valid, tab, (i64)n_seqs, min_depth, min_alt, min_frac_ppm, (i64 *)d_cnt, (const i64 *)nullptr,
                           (SbwtPileCall *)nullptr);
    else
        hipLaunchKernelGGL(k_pile_calls<true>, dim3(nb), dim3(256), 0, stream, cells, (i64)n_cells, (const i64 *)d_bsum, (const u64 *)d_bits,
                           (const u64 *)d_valid, tab, (i64)n_seqs, min_depth, min_alt, min_frac_ppm, (i64 *)nullptr, (const i64 *)d_off, d_out);
}

void sbwt_launch_pile_scan_i64(const long long *d_in, long long n, long long *d_bsum, long long *d_out, hipStream_t stream) {
    const unsigned nb = (unsigned)((n + 1023) / 1024);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(nb), dim3(256), 0, stream, (const i64 *)d_in, (i64)n, (i64 *)d_bsum);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, stream, (i64 *)d_bsum, (i64)nb);
    hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(256), 0, stream, (const i64 *)d_in, (i64)n, (const i64 *)d_bsum, (i64 *)d_out);
}
