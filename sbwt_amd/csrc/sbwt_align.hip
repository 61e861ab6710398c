// sbwt_align.hip -- the alignment of mapped reads: where the best alignment of a verified read begins and its runs of = X I D
// (include/sbwtgpu.h, "alignment of mapped reads").  The forward pass is sbwt_launch_verify, unchanged: it
// gives edit and ref_end, and with them the one cell (L, tE) the walk starts from.  Everything is exact integers.
//
//   k_align        ONE LANE PER READ, a fixed grid of waves over groups of 64 reads.  A lane with edit = 0 writes its one run at
//                  once.  The others run Sellers' table on the 2 E + 1 diagonals around tE - L (the band lemma; E >= edit is the
//                  wave's instantiation, chosen by its widest member from 1, 3, 7, 15, 31), the row in registers, the text of
//                  the row's columns as four bit masks that shift by one column per row.  Per row and band cell two bits: does
//                  the diagonal step apply (and is it = or X), does the insertion apply.  A row's two mask words go to the
//                  wave's scratch in the workspace, [row][lane], one contiguous store per wave and row; the walk back reads
//                  the lane's own words.  Reads with edit > fast_edit or more than SBWT_AL_FAST_ROWS bases go onto a list.
//   k_align_slow   ONE WAVE PER READ over that list: the whole window, 24 columns per lane in registers, the horizontal step
//                  as a min-plus scan over the lanes; two bits per cell, one 64-bit word per lane and row, in the wave's scratch.
//                  The walk runs on every lane alike and takes a cell's bits from the lane that owns them.
//
// Both kernels run twice: a pass that counts every read's runs and writes the records, a device scan of the counts, and a
// pass that stores the runs at their offsets (a walk yields its runs last first, so the place of each needs the count).
#include "sbwt_kernels_common.h"
#include "sbwt_align.h"
#include "sbwt_verify_text.h"
#include "sbwt_scan.h"

#define AL_INF (1 << 28)            // a cell outside the table
#define AL_I 1u
#define AL_D 2u
#define AL_EQ 7u
#define AL_X 8u

typedef unsigned al_u32x2 __attribute__((ext_vector_type(2)));
typedef u64 al_u64x2 __attribute__((ext_vector_type(2)));
template <typename M> struct AlPair;
template <> struct AlPair<unsigned> { typedef al_u32x2 type; };
template <> struct AlPair<u64> { typedef al_u64x2 type; };

// what the two passes read and write beside the reads
struct AlOut {
    const SbwtReadVerify *verify;
    SbwtReadAlign *out;
    i64 *cnt;               // the run count of every read, what the scan sums
    const i64 *op_off;      // (second pass)
    unsigned *ops;
    i64 ops_cap;
};

// The runs of one read as its walk yields them, last run first.  The second pass stores run j at op_off[r] + n_ops - 1 - j.
struct AlRuns {
    unsigned code, len;
    int n_ops, n_eq;
    i64 lo, last;           // second pass: the read's first and last place in ops
};
template <bool FILL>
__device__ __forceinline__ void al_flush(AlRuns &U, const AlOut &O, bool store) {
    if (U.len == 0) return;
    if (FILL) {
        const i64 at = U.last - U.n_ops;
        if (store && at >= U.lo && at < O.ops_cap) O.ops[at] = (U.len << 4) | U.code;
    }
    U.n_ops++;
}
template <bool FILL>
__device__ __forceinline__ void al_emit(AlRuns &U, unsigned op, const AlOut &O, bool store) {
    if (op == U.code) {
        U.len++;
    } else {
        al_flush<FILL>(U, O, store);
        U.code = op;
        U.len = 1;
    }
    U.n_eq += (int)(op == AL_EQ);
}
template <bool FILL>
__device__ __forceinline__ AlRuns al_runs(i64 r, const AlOut &O) {
    AlRuns U = {0u, 0u, 0, 0, 0, 0};
    if (FILL) {
        U.lo = O.op_off[r];
        U.last = U.lo + O.out[r].n_ops - 1;
    }
    return U;
}

// 1 for x = 0, 0 for x > 0, without a compare: sixty-three of them a row would keep their results in scalar registers
__device__ __forceinline__ unsigned al_is_zero(int x) { return (unsigned)(x - 1) >> 31; }

struct AlRead {
    i64 off, L, start, ref_end;
    int strand, edit;
    VfText T;
};
// Read r's verify record, map record and sequence.  false: its alignment needs no table and is written here (no alignment,
// no bases, or edit = 0: the single run L=).
template <bool FILL>
__device__ __forceinline__ bool al_open(i64 r, const i64 *__restrict__ read_off, const SbwtVerifyMap *__restrict__ map,
                                        const SbwtRefSeq *__restrict__ tab, const u64 *__restrict__ bits, const u64 *__restrict__ valid,
                                        int B, const AlOut &O, bool store, AlRead &R) {
    const SbwtReadVerify v = O.verify[r];
    R.edit = v.edit;
    R.ref_end = v.ref_end;
    R.off = read_off[r];
    R.L = read_off[r + 1] - R.off;
    R.start = map[r].start;
    R.strand = map[r].strand;
    if (v.edit < 0 || R.L <= 0) {
        if (!FILL && store) {
            O.out[r] = SbwtReadAlign{v.edit < 0 ? 0 : R.start - B, 0, 0};
            O.cnt[r] = 0;
        }
        return false;
    }
    if (v.edit == 0) {
        if (!FILL && store) {
            O.out[r] = SbwtReadAlign{v.ref_end - R.L, 1, (int)R.L};
            O.cnt[r] = 1;
        }
        if (FILL && store && O.op_off[r] < O.ops_cap) O.ops[O.op_off[r]] = ((unsigned)R.L << 4) | AL_EQ;
        return false;
    }
    const SbwtRefSeq s = tab[map[r].seq];      // (edit >= 0: the verify kernel has checked seq)
    R.T = VfText{bits + 2 * s.slot, valid + s.slot, s.len, 0, 0, false};
    return true;
}

// A read of at most SBWT_AL_FAST_ROWS bases and 1 <= edit <= E.  Band cell b of row i is column t = i + (tE - L) - E + b.
template <int E, typename M, bool FILL>
__device__ __forceinline__ i64 al_fast(const char *__restrict__ bases, i64 total, AlRead &R, int B, char *slab, int lane, AlRuns &U,
                                       const AlOut &O) {
    typedef typename AlPair<M>::type Pair;
    constexpr int W = 2 * E + 1;
    constexpr M TOP = (M)1 << (W - 1);
    Pair *rows = reinterpret_cast<Pair *>(slab) + lane;        // row i - 1 at rows[(i - 1) * 64]
    const int L = (int)R.L;
    const unsigned comp = R.strand ? 3u : 0u;
    const int d0 = (int)(R.ref_end - (R.start - B)) - L;        // tE - L
    int prev[W];
#pragma unroll
    for (int b = 0; b < W; b++) prev[b] = d0 - E + b >= 0 ? 0 : AL_INF;    // D[0][t] = 0 from column 0 on
    // bit b of tm[c]: the coordinate of the row's band cell b holds code c.  One column enters at the top per row.
    M tm0 = 0, tm1 = 0, tm2 = 0, tm3 = 0;
    i64 p = R.start - B + d0 - E;                               // the coordinate of row 1, cell 0
    for (int k = 0; k < W - 1; k++, p++) {
        const unsigned c = vf_text(R.T, p);
        tm0 = (tm0 >> 1) | (c == 0 ? TOP : 0);
        tm1 = (tm1 >> 1) | (c == 1 ? TOP : 0);
        tm2 = (tm2 >> 1) | (c == 2 ? TOP : 0);
        tm3 = (tm3 >> 1) | (c == 3 ? TOP : 0);
    }
    u64 x = 0;
    for (int i = 1; i <= L; i++, p++) {
        const unsigned c = vf_text(R.T, p);
        tm0 = (tm0 >> 1) | (c == 0 ? TOP : 0);
        tm1 = (tm1 >> 1) | (c == 1 ? TOP : 0);
        tm2 = (tm2 >> 1) | (c == 2 ? TOP : 0);
        tm3 = (tm3 >> 1) | (c == 3 ? TOP : 0);
        if (((i - 1) & 7) == 0) x = vf_read8(bases, total, R.off, L, R.strand, i - 1);
        const unsigned rc = vf_code((unsigned)x & 0xffu) ^ comp;            // (VF_NONE stays above 3)
        x >>= 8;
        const M eq = rc == 0 ? tm0 : rc == 1 ? tm1 : rc == 2 ? tm2 : rc == 3 ? tm3 : 0;
        const M ne = ~eq;
        const int neg = E - d0 - i;                             // cells b < neg lie left of column 0
        int left = AL_INF;
        M am = 0, bm = 0;
#pragma unroll
        for (int b = 0; b < W; b++) {
            const unsigned cost = (unsigned)(ne >> b) & 1u;
            const int dg = prev[b] + (int)cost;
            const int up = (b + 1 < W ? prev[b + 1] : AL_INF) + 1;
            int v = dg < up ? dg : up;
            v = left + 1 < v ? left + 1 : v;
            v = b < neg ? AL_INF : v;
            const unsigned a = al_is_zero(dg - v), u = al_is_zero(up - v);     // (v <= dg, up wherever the cell is in the table)
            am |= (M)a << b;
            bm |= (M)(u ^ (a & (u ^ cost))) << b;                               // a ? cost : u
            prev[b] = v;
            left = v;
        }
        Pair w;
        w.x = am;
        w.y = bm;
        rows[(i64)(i - 1) * 64] = w;
    }
    // the walk: from (L, tE), cell E, to row 0
    int i = L, b = E, row = 0;
    M am = 0, bm = 0;
    for (int guard = L + W + 1; i > 0 && guard > 0 && (unsigned)b < (unsigned)W; guard--) {
        if (row != i) {
            const Pair w = rows[(i64)(i - 1) * 64];
            am = w.x;
            bm = w.y;
            row = i;
        }
        const bool a = (am >> b) & 1, s = (bm >> b) & 1;
        if (a) {
            al_emit<FILL>(U, s ? AL_X : AL_EQ, O, true);
            i--;
        } else if (s) {
            al_emit<FILL>(U, AL_I, O, true);
            i--;
            b++;
        } else {
            al_emit<FILL>(U, AL_D, O, true);
            b--;
        }
    }
    al_flush<FILL>(U, O, true);
    return R.start - B + d0 - E + b;
}

template <bool FILL>
__global__ void __launch_bounds__(64) k_align(const char *__restrict__ bases, i64 total, const i64 *__restrict__ read_off, i64 n_reads,
                                              const SbwtVerifyMap *__restrict__ map, const SbwtRefSeq *__restrict__ tab,
                                              const u64 *__restrict__ bits, const u64 *__restrict__ valid, int B, int fast_edit, AlOut O,
                                              SbwtAlignHeader *hdr, unsigned *__restrict__ slow, char *slabs) {
    const int lane = threadIdx.x;
    char *slab = slabs + (i64)blockIdx.x * SBWT_AL_FAST_SLAB;
    const i64 groups = (n_reads + 63) >> 6;
    for (i64 g = blockIdx.x; g < groups; g += gridDim.x) {
        const i64 r = g * 64 + lane;
        AlRead R;
        bool mine = false;
        if (r < n_reads && al_open<FILL>(r, read_off, map, tab, bits, valid, B, O, true, R)) {
            if (R.edit > fast_edit || R.L > SBWT_AL_FAST_ROWS) {
                if (!FILL) slow[atomicAdd(&hdr->n_slow, 1u)] = (unsigned)r;   // the second kernel writes this read's record
            } else {
                mine = true;
            }
        }
        int e = mine ? R.edit : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int o = __shfl_xor(e, off);
            if (o > e) e = o;
        }
        e = (int)uniform32((unsigned)e);                       // the wave's widest band chooses the instantiation
        if (mine) {
            AlRuns U = al_runs<FILL>(r, O);
            i64 begin;
            if (e <= 1) begin = al_fast<1, unsigned, FILL>(bases, total, R, B, slab, lane, U, O);
            else if (e <= 3) begin = al_fast<3, unsigned, FILL>(bases, total, R, B, slab, lane, U, O);
            else if (e <= 7) begin = al_fast<7, unsigned, FILL>(bases, total, R, B, slab, lane, U, O);
            else if (e <= 15) begin = al_fast<15, unsigned, FILL>(bases, total, R, B, slab, lane, U, O);
            else begin = al_fast<31, u64, FILL>(bases, total, R, B, slab, lane, U, O);
            if (!FILL) {
                O.out[r] = SbwtReadAlign{begin, U.n_ops, U.n_eq};
                O.cnt[r] = U.n_ops;
            }
        }
    }
}

// The reads of the list, one wave each.  Lane l owns the columns t = 24 l + 1 + k, k < 24; column 0 (D[i][0] = i) enters lane 0
// from the left.
template <bool FILL>
__global__ void __launch_bounds__(64) k_align_slow(const char *__restrict__ bases, i64 total, const i64 *__restrict__ read_off, i64 n_reads,
                                                   const SbwtVerifyMap *__restrict__ map, const SbwtRefSeq *__restrict__ tab,
                                                   const u64 *__restrict__ bits, const u64 *__restrict__ valid, int B, AlOut O,
                                                   const SbwtAlignHeader *hdr, const unsigned *__restrict__ slow, char *slabs) {
    constexpr int C = SBWT_AL_SLOW_COLS;
    const int lane = threadIdx.x;
    u64 *rows = reinterpret_cast<u64 *>(slabs + (i64)blockIdx.x * SBWT_AL_SLOW_SLAB) + lane;
    i64 n_slow = hdr->n_slow;
    if (n_slow > n_reads) n_slow = n_reads;                    // (never: a read is listed once)
    for (i64 e = blockIdx.x; e < n_slow; e += gridDim.x) {
        const i64 r = slow[e];
        AlRead R;
        if (r >= n_reads || !al_open<FILL>(r, read_off, map, tab, bits, valid, B, O, lane == 0, R)) continue;     // (never)
        const int L = (int)R.L;
        if (L > SBWT_VF_MAX_READ) continue;                    // (never: such a read has edit = -1)
        const unsigned comp = R.strand ? 3u : 0u;
        const int tE = (int)(R.ref_end - (R.start - B));
        unsigned tm0 = 0, tm1 = 0, tm2 = 0, tm3 = 0;           // bit k: the coordinate of the lane's column k holds that code
        i64 p = R.start - B + (i64)lane * C;
        for (int k = 0; k < C; k++, p++) {
            const unsigned c = vf_text(R.T, p);
            tm0 |= c == 0 ? 1u << k : 0;
            tm1 |= c == 1 ? 1u << k : 0;
            tm2 |= c == 2 ? 1u << k : 0;
            tm3 |= c == 3 ? 1u << k : 0;
        }
        int prev[C], y[C];
#pragma unroll
        for (int k = 0; k < C; k++) prev[k] = 0;
        u64 x = 0;
        for (int i = 1; i <= L; i++) {
            if (((i - 1) & 7) == 0) x = vf_read8(bases, total, R.off, L, R.strand, i - 1);
            const unsigned rc = vf_code((unsigned)x & 0xffu) ^ comp;
            x >>= 8;
            const unsigned eq = rc == 0 ? tm0 : rc == 1 ? tm1 : rc == 2 ? tm2 : rc == 3 ? tm3 : 0;
            int pl = __shfl_up(prev[C - 1], 1);                // D[i - 1][the column left of the lane's first]
            if (lane == 0) pl = i - 1;
            // the diagonal and vertical minima, then the horizontal step inside the lane
            int pd = pl, run = lane == 0 ? i : AL_INF;
#pragma unroll
            for (int k = 0; k < C; k++) {
                const int dg = pd + (int)(~(eq >> k) & 1), up = prev[k] + 1;
                int v = dg < up ? dg : up;
                v = run + 1 < v ? run + 1 : v;
                y[k] = v;
                run = v;
                pd = prev[k];
            }
            // ... and across the lanes: D[i][last column of lane l] = min over l' <= l of y_l'[C - 1] + C (l - l')
            int s = run - C * lane;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_up(s, off);
                if (lane >= off && o < s) s = o;
            }
            int carry = __shfl_up(s + C * lane, 1);
            if (lane == 0) carry = AL_INF;
            u64 word = 0;
            pd = pl;
#pragma unroll
            for (int k = 0; k < C; k++) {
                const unsigned cost = (~eq >> k) & 1u;
                const int dg = pd + (int)cost, up = prev[k] + 1;
                const int v = carry + k + 1 < y[k] ? carry + k + 1 : y[k];
                const unsigned a = al_is_zero(dg - v), u = al_is_zero(up - v);
                word |= (u64)(a | ((u ^ (a & (u ^ cost))) << 1)) << (2 * k);
                pd = prev[k];
                prev[k] = v;
            }
            rows[(i64)(i - 1) * 64] = word;
        }
        // the walk, the same on every lane; lane 0 stores
        AlRuns U = al_runs<FILL>(r, O);
        int i = L, t = tE, row = 0;
        u64 w = 0;
        for (int guard = 2 * L + 2 * B + 2; i > 0 && guard > 0; guard--) {
            if (t <= 0) {                                      // column 0: D[i][0] = i, insertions only
                al_emit<FILL>(U, AL_I, O, lane == 0);
                i--;
                continue;
            }
            if (row != i) {
                w = rows[(i64)(i - 1) * 64];
                row = i;
            }
            const int owner = (t - 1) / C, k = (t - 1) - owner * C;
            const unsigned two = (unsigned)(__shfl(w, owner) >> (2 * k)) & 3u;
            if (two & 1u) {
                al_emit<FILL>(U, (two & 2u) ? AL_X : AL_EQ, O, lane == 0);
                i--;
                t--;
            } else if (two & 2u) {
                al_emit<FILL>(U, AL_I, O, lane == 0);
                i--;
            } else {
                al_emit<FILL>(U, AL_D, O, lane == 0);
                t--;
            }
        }
        al_flush<FILL>(U, O, lane == 0);
        if (!FILL && lane == 0) {
            O.out[r] = SbwtReadAlign{R.start - B + t, U.n_ops, U.n_eq};
            O.cnt[r] = U.n_ops;
        }
    }
}

void sbwt_launch_align(const char *d_bases, long long total_bases, const long long *d_read_off, long long n_reads,
                       const SbwtVerifyMap *d_map, const SbwtRefSeq *tab, const unsigned long long *d_bits,
                       const unsigned long long *d_valid, int band, int fast_edit, const SbwtReadVerify *d_verify, SbwtReadAlign *d_out,
                       long long *d_op_off, unsigned *d_ops, long long ops_cap, char *ws, hipStream_t stream) {
    if (n_reads <= 0) {
        (void)hipMemsetAsync(d_op_off, 0, 8, stream);
        return;
    }
    if (fast_edit < 1 || fast_edit > SBWT_AL_FAST_EDIT) fast_edit = SBWT_AL_FAST_EDIT;
    const SbwtAlignLayout a = sbwt_align_layout(n_reads);
    SbwtAlignHeader *hdr = reinterpret_cast<SbwtAlignHeader *>(ws + a.o_hdr);
    unsigned *slow = reinterpret_cast<unsigned *>(ws + a.o_slow);
    i64 *cnt = reinterpret_cast<i64 *>(ws + a.o_cnt), *bsum = reinterpret_cast<i64 *>(ws + a.o_bsum);
    const AlOut O = {d_verify, d_out, cnt, (const i64 *)d_op_off, d_ops, (i64)ops_cap};
    const unsigned nb = (unsigned)((n_reads + 1023) / 1024);
    (void)hipMemsetAsync(hdr, 0, sizeof(SbwtAlignHeader), stream);
    hipLaunchKernelGGL(k_align<false>, dim3((unsigned)a.fast_waves), dim3(64), 0, stream, d_bases, (i64)total_bases, (const i64 *)d_read_off,
                       (i64)n_reads, d_map, tab, (const u64 *)d_bits, (const u64 *)d_valid, band, fast_edit, O, hdr, slow, ws + a.o_fast);
    hipLaunchKernelGGL(k_align_slow<false>, dim3((unsigned)a.slow_waves), dim3(64), 0, stream, d_bases, (i64)total_bases,
                       (const i64 *)d_read_off, (i64)n_reads, d_map, tab, (const u64 *)d_bits, (const u64 *)d_valid, band, O, hdr, slow,
                       ws + a.o_slab);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(nb), dim3(256), 0, stream, (const i64 *)cnt, (i64)n_reads, bsum);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, stream, bsum, (i64)nb);
    hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(256), 0, stream, (const i64 *)cnt, (i64)n_reads, (const i64 *)bsum, (i64 *)d_op_off);
    if (ops_cap <= 0) return;                                  // (nothing can be stored)
    hipLaunchKernelGGL(k_align<true>, dim3((unsigned)a.fast_waves), dim3(64), 0, stream, d_bases, (i64)total_bases, (const i64 *)d_read_off,
                       (i64)n_reads, d_map, tab, (const u64 *)d_bits, (const u64 *)d_valid, band, fast_edit, O, hdr, slow, ws + a.o_fast);
    hipLaunchKernelGGL(k_align_slow<true>, dim3((unsigned)a.slow_waves), dim3(64), 0, stream, d_bases, (i64)total_bases,
                       (const i64 *)d_read_off, (i64)n_reads, d_map, tab, (const u64 *)d_bits, (const u64 *)d_valid, band, O, hdr, slow,
                       ws + a.o_slab);
}
