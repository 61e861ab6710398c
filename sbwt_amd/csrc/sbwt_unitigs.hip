// sbwt_unitigs.hip -- the unitigs of the node-centric de Bruijn graph of an index, spelled on the device.
//
// Definitions (include/sbwtgpu.h has the contract).  A column is REAL when its label holds no '$': k backward steps from it
// do not pass column 0; the others are the dummies, a tree under the root that the predecessor function spans.  The
// out-neighbours of a real column v are the targets C[c] + rank_c(g) of the set of g, the first column of v's suffix group;
// the in-neighbours of w are the real members of the group that starts at pred(w).  A dummy's group is the dummy alone and
// a group with a real column holds real columns only, so an edge v -> w is INTERNAL (outdeg(v) = 1 and indeg(w) = 1) exactly
// when v is real, is a whole group by itself and has one set bit; w is then a start unless pred(w) is such a column.
//
// Passes (sbwt_unitigs_run), every one a flat launch over the columns or over the unitigs:
//   1  pred[C[c] + rank_c(u)] = u, and the marks as one bit vector (from the blocks, or derived from pred when the image has none)
//   2  level of every dummy, k-1 rounds from the root; a column no round reaches is real
//   3  ranking state per column: a start is ranked { head = itself, rank 0 }, any other real column is open { pointer = pred,
//      window minimum = itself at offset 0 }
//   4  pointer jumping: round r doubles the window of every open column from 2^r to 2^(r+1) predecessors; a column whose
//      pointer is ranked takes head and rank + 2^r from it, any other keeps the smallest column of its window and the offset of
//      its first occurrence.  The rounds end when no column is open, or after ceil(log2 n): what is open then lies on a pure
//      cycle that its window has covered, so the minimum is the cycle's smallest column -- its head -- and the offset the rank.
//   5  start flags -> exclusive scan -> unitig ids in column order; the one tail of every unitig writes its length; exclusive
//      scan -> 64-bit offsets into the bases
//   6  every real column stores its last character at off[id(head)] + k - 1 + rank; every start walks k-1 predecessors for the
//      first k-1 characters of its label
// A coloured run (d_ids given) cuts where the colour set changes: passes 3 and 5 take an edge for
// internal only if both ends carry the same set, pass 5 gathers the set id of every unitig.  Passes 1, 2, 4 and 6 are the same.
// Asked for a graph, the run goes on after pass 6, on the state the six passes leave:
//   7  links: every tail counts the set bits of its group's first column into deg[unitig]; exclusive scan -> link_off; every
//      tail writes the unitig ids of its out-neighbours, which are first columns, in character order
//   8  column map: every real column stores uid[head] and its rank
// No lane loops over a unitig: the longest loop of a lane is k steps (or the words of a row across a candidate break).
// Columns are 32-bit unsigned as in the image.
//
// Pass 6 scatters single bytes instead of filling an order[] array first and streaming it out: a scattered store moves a whole
// sector whether it carries one byte or four, so the array would add a 4-byte write and a 4-byte read per column on top of the
// same number of scattered stores (and a search for the unitig of every output byte).
#include "sbwt_kernels_common.h"
#include "sbwt_colwalk.h"
#include "sbwt_scan.h"
#include "sbwt_unitigs.h"

#define UT_NONE 0xFFFFFFFFu
#define UT_OPEN 0u          // state .w: { pointer, offset of the window's minimum, the minimum, UT_OPEN }
#define UT_RANKED 1u        //           { head, rank, -, UT_RANKED }
#define UT_DUMMY 2u         //           not a real column

__device__ __forceinline__ bool ut_mark(const u64 *__restrict__ marks, i64 j) { return (marks[j >> 6] >> (j & 63)) & 1ull; }
// ---- pass 1 ----
// (k_ut_pred: sbwt_colwalk.h)
// the marks of the blocks: quads 0 and 1 hold the two halves of a block's word
__global__ void __launch_bounds__(256) k_ut_marks_copy(SbwtIndexView ix, u64 *__restrict__ marks, i64 n_words) {
    const i64 b = (i64)blockIdx.x * 256 + threadIdx.x;
    if (b >= n_words) return;
    marks[b] = (u64)ix.blocks[b * 4].w | ((u64)ix.blocks[b * 4 + 1].w << 32);
}
// column j starts a group unless the labels of j-1 and j share their last k-1 characters: both walk back through pred while
// their last characters agree ('$' agrees with nothing; only the smaller column can reach the root).  One word per wave.
__global__ void __launch_bounds__(256) k_ut_marks_derive(SbwtIndexView ix, const unsigned *__restrict__ pred, u64 *__restrict__ marks) {
    const i64 n = ix.n_nodes;
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    bool start = false;
    if (j < n) {
        start = true;
        if (j >= 1) {
            const int cap = ix.k - 1;
            i64 a = j - 1, b = j;
            int d = 0;
            while (d < cap && a != 0 && ut_last_char(ix, a) == ut_last_char(ix, b)) {
                a = (i64)pred[a];
                b = (i64)pred[b];
                d++;
            }
            start = d < cap;
        }
    }
    const u64 word = __ballot(start);
    if ((threadIdx.x & 63) == 0 && j < n + 64) marks[j >> 6] = word;
}

// ---- pass 2 ----
// (k_ut_level: sbwt_colwalk.h)

// ---- pass 3 ----
// is the one edge out of column p internal?  (p real, a group of its own, one set bit)
__device__ __forceinline__ bool ut_single_out(const SbwtIndexView &ix, const unsigned char *__restrict__ lev,
                                              const u64 *__restrict__ marks, i64 p) {
    if (lev[p] != 0 || !ut_mark(marks, p) || (p + 1 < ix.n_nodes && !ut_mark(marks, p + 1))) return false;
    const uint4 *blk = ix.blocks + ((p >> 6) << 2);
    int deg = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) deg += (int)((quad_bits(blk[c]) >> (p & 63)) & 1ull);
    return deg == 1;
}
// the colour view of a coloured run (section 18): the ids and the table of a colour-set object, read in place
struct UtColors {
    const unsigned *__restrict__ ids;      // n_nodes
    const u64 *__restrict__ table;         // n_sets x words
    int words;
};
// do columns a and b carry the same set?  Equal ids do; otherwise the two rows decide, word for word (an uploaded object may
// hold one row twice).  Called across single edges only, so the rows are read where a break is possible, not per column.
__device__ __forceinline__ bool ut_same_set(const UtColors &cs, i64 a, i64 b) {
    const unsigned ia = cs.ids[a], ib = cs.ids[b];
    if (ia == ib) return true;
    const u64 *ra = cs.table + (i64)ia * cs.words, *rb = cs.table + (i64)ib * cs.words;
    for (int w = 0; w < cs.words; w++)
        if (ra[w] != rb[w]) return false;
    return true;
}
// COLORED: an edge is internal only if both ends carry the same set; the others of the single edges are the colour breaks,
// counted per wave into *n_breaks
template <bool COLORED>
__global__ void __launch_bounds__(256) k_ut_link(SbwtIndexView ix, const unsigned *__restrict__ pred, const unsigned char *__restrict__ lev,
                                                 const u64 *__restrict__ marks, uint4 *__restrict__ st, int *__restrict__ open,
                                                 UtColors cs, unsigned long long *__restrict__ n_breaks) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v >= ix.n_nodes) return;                             // (whole waves, or the upper lanes of the last one)
    uint4 s;
    bool brk = false;
    if (lev[v] != 0) {
        s = make_uint4(UT_NONE, 0u, UT_NONE, UT_DUMMY);
    } else {
        const i64 p = (i64)pred[v];
        bool internal = ut_single_out(ix, lev, marks, p);
        if constexpr (COLORED) {
            brk = internal && !ut_same_set(cs, p, v);
            internal = internal && !brk;
        }
        if (internal) {
            s = make_uint4((unsigned)p, 0u, (unsigned)v, UT_OPEN);
            *open = 1;
        } else {
            s = make_uint4((unsigned)v, 0u, 0u, UT_RANKED);
        }
    }
    st[v] = s;
    if constexpr (COLORED) {
        const u64 b = __ballot(brk);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(n_breaks, (unsigned long long)__popcll(b));   // (lane 0 outlives the return above)
    }
}

// ---- pass 4 ----
__global__ void __launch_bounds__(256) k_ut_jump(i64 n, const uint4 *__restrict__ in, uint4 *__restrict__ out, unsigned window,
                                                 int *__restrict__ open) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    uint4 s = in[v];
    if (s.w == UT_OPEN) {
        const uint4 p = in[s.x];
        if (p.w == UT_RANKED) {
            s = make_uint4(p.x, p.y + window, 0u, UT_RANKED);
        } else {                                             // (an open column's pointer is real: open as well)
            if (p.z < s.z) { s.z = p.z; s.y = p.y + window; }
            s.x = p.x;
            *open = 1;
        }
    }
    out[v] = s;
}
// what is still open lies on a pure cycle: it starts at its smallest column
__global__ void __launch_bounds__(256) k_ut_close(i64 n, uint4 *__restrict__ st) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const uint4 s = st[v];
    if (s.w == UT_OPEN) st[v] = make_uint4(s.z, s.y, 0u, UT_RANKED);
}

// ---- pass 5 ----
__global__ void __launch_bounds__(256) k_ut_starts(i64 n, const uint4 *__restrict__ st, i64 *__restrict__ flag) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const uint4 s = st[v];
    flag[v] = (s.w == UT_RANKED && s.y == 0u) ? 1 : 0;
}
// the start of a unitig notes its column, the tail (no internal edge out, or one back to the head: a cut cycle) its length.
// COLORED: a single edge into another set is no internal edge either.
template <bool MEGA, bool COLORED>
__device__ __forceinline__ bool ut_is_tail(const SbwtIndexView &ix, const unsigned char *__restrict__ lev, const u64 *__restrict__ marks,
                                           const uint4 &s, i64 v, const UtColors &cs) {
    bool tail = true;
    if (ut_single_out(ix, lev, marks, v)) {
        const uint4 *blk = ix.blocks + ((v >> 6) << 2);
        i64 w = -1;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const uint4 q = blk[c];
            if ((quad_bits(q) >> (v & 63)) & 1ull) w = (i64)quad_rank<MEGA>(ix, q, v, c);
        }
        tail = w == (i64)s.x;
        if constexpr (COLORED) {
            if (!tail && w >= 0 && w < ix.n_nodes) tail = !ut_same_set(cs, v, w);
        }
    }
    return tail;
}
template <bool MEGA, bool COLORED>
__global__ void __launch_bounds__(256) k_ut_lengths(SbwtIndexView ix, const unsigned char *__restrict__ lev, const u64 *__restrict__ marks,
                                                    const uint4 *__restrict__ st, const i64 *__restrict__ uid,
                                                    i64 *__restrict__ first_col, i64 *__restrict__ len, UtColors cs) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v >= ix.n_nodes) return;
    const uint4 s = st[v];
    if (s.w != UT_RANKED) return;
    if (s.y == 0u) first_col[uid[v]] = v;
    if (ut_is_tail<MEGA, COLORED>(ix, lev, marks, s, v, cs)) len[uid[s.x]] = (i64)s.y + 1 + (ix.k - 1);
}

// the set id of a coloured unitig is the id of its first column
__global__ void __launch_bounds__(256) k_ut_setids(const unsigned *__restrict__ ids, i64 n_nodes, const i64 *__restrict__ first_col,
                                                   i64 n_unitigs, unsigned *__restrict__ set_id) {
    const i64 u = (i64)blockIdx.x * 256 + threadIdx.x;
    if (u >= n_unitigs) return;
    const i64 v = first_col[u];
    set_id[u] = (v >= 0 && v < n_nodes) ? ids[v] : 0u;
}

// ---- pass 6 ----
__global__ void __launch_bounds__(256) k_ut_chars(SbwtIndexView ix, const uint4 *__restrict__ st, const i64 *__restrict__ uid,
                                                  const i64 *__restrict__ off, char *__restrict__ bases) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v >= ix.n_nodes) return;
    const uint4 s = st[v];
    if (s.w != UT_RANKED) return;
    bases[off[uid[s.x]] + (ix.k - 1) + (i64)s.y] = "ACGT"[ut_last_char(ix, v)];
}
__global__ void __launch_bounds__(256) k_ut_labels(SbwtIndexView ix, const unsigned *__restrict__ pred, const i64 *__restrict__ first_col,
                                                   const i64 *__restrict__ off, i64 n_unitigs, char *__restrict__ bases) {
    const i64 u = (i64)blockIdx.x * 256 + threadIdx.x;
    if (u >= n_unitigs) return;
    i64 v = first_col[u];
    char *to = bases + off[u] + (ix.k - 1);
    for (int j = 1; j < ix.k; j++) {
        v = (i64)pred[v];
        to[-j] = "ACGT"[ut_last_char(ix, v)];
    }
}

// ---- pass 7: links (section 21) ----
// the first column of v's suffix group: a group holds at most 4 columns (one per character that can precede its suffix), so at
// most 3 steps back, possibly into the previous word of the marks; column 0 starts a group
__device__ __forceinline__ i64 ut_group_first(const u64 *__restrict__ marks, i64 v) {
    i64 g = v;
    for (int i = 0; i < 3 && g > 0 && !ut_mark(marks, g); i++) g--;
    return g;
}
// the tail of every unitig counts its out-neighbours: the set bits of its group's first column
template <bool MEGA, bool COLORED>
__global__ void __launch_bounds__(256) k_ut_link_count(SbwtIndexView ix, const unsigned char *__restrict__ lev, const u64 *__restrict__ marks,
                                                       const uint4 *__restrict__ st, const i64 *__restrict__ uid, i64 *__restrict__ deg,
                                                       UtColors cs) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v >= ix.n_nodes) return;
    const uint4 s = st[v];
    if (s.w != UT_RANKED || !ut_is_tail<MEGA, COLORED>(ix, lev, marks, s, v, cs)) return;
    const i64 g = ut_group_first(marks, v);
    const uint4 *blk = ix.blocks + ((g >> 6) << 2);
    int d = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) d += (int)((quad_bits(blk[c]) >> (g & 63)) & 1ull);
    deg[uid[s.x]] = d;
}
// ... and writes their unitigs in character order: an out-neighbour of a tail is a first column, so uid[] of it is its unitig
template <bool MEGA, bool COLORED>
__global__ void __launch_bounds__(256) k_ut_link_fill(SbwtIndexView ix, const unsigned char *__restrict__ lev, const u64 *__restrict__ marks,
                                                      const uint4 *__restrict__ st, const i64 *__restrict__ uid,
                                                      const i64 *__restrict__ link_off, unsigned *__restrict__ link_to, UtColors cs) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v >= ix.n_nodes) return;
    const uint4 s = st[v];
    if (s.w != UT_RANKED || !ut_is_tail<MEGA, COLORED>(ix, lev, marks, s, v, cs)) return;
    const i64 g = ut_group_first(marks, v);
    const uint4 *blk = ix.blocks + ((g >> 6) << 2);
    const i64 u = uid[s.x];
    i64 at = link_off[u];
    const i64 end = link_off[u + 1];                         // (what k_ut_link_count counted from the same bits)
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint4 q = blk[c];
        if (((quad_bits(q) >> (g & 63)) & 1ull) && at < end) {
            const u64 w = quad_rank<MEGA>(ix, q, g, c);
            link_to[at++] = w < (u64)ix.n_nodes ? (unsigned)uid[w] : UT_NONE;
        }
    }
}

// ---- pass 8: column map ----
__global__ void __launch_bounds__(256) k_ut_colmap(i64 n, const uint4 *__restrict__ st, const i64 *__restrict__ uid,
                                                   unsigned *__restrict__ col_unitig, unsigned *__restrict__ col_offset) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const uint4 s = st[v];
    const bool real = s.w == UT_RANKED;
    col_unitig[v] = real ? (unsigned)uid[s.x] : UT_NONE;
    col_offset[v] = real ? s.y : UT_NONE;
}
// locate: the map gathered at search results
__global__ void __launch_bounds__(256) k_ut_locate(const unsigned *__restrict__ col_unitig, const unsigned *__restrict__ col_offset,
                                                   i64 n_nodes, const i64 *__restrict__ cols, i64 n, unsigned *__restrict__ unitig,
                                                   unsigned *__restrict__ offset) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const i64 c = cols[i];
    const bool in = c >= 0 && c < n_nodes;
    unitig[i] = in ? col_unitig[c] : UT_NONE;
    offset[i] = in ? col_offset[c] : UT_NONE;
}

// ---------------------------------------------------------------------------------------------
static inline i64 ut_pad(i64 n) { return (n + 64 + 255) & ~(i64)255; }
struct UtLayout {
    i64 pred, lev, marks, st0, st1, bsum, ctl, bytes;
    explicit UtLayout(i64 n) {
        const i64 np = ut_pad(n);
        pred = 0;
        lev = pred + 4 * np;
        marks = lev + np;
        st0 = marks + ((8 * (np / 64 + 2) + 255) & ~(i64)255);
        st1 = st0 + 16 * np;
        bsum = st1 + 16 * np;
        ctl = bsum + ((8 * (np / 1024 + 4) + 255) & ~(i64)255);
        bytes = ctl + 256;
    }
};
long long sbwt_unitigs_scratch_bytes(long long n_nodes) { return UtLayout(n_nodes).bytes; }

static void ut_scan(const i64 *in, i64 n, i64 *bsum, i64 *out, hipStream_t stream) {
    if (n <= 0) {
        (void)hipMemsetAsync(out, 0, 8, stream);
        return;
    }
    const unsigned nb = (unsigned)((n + 1023) / 1024);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(nb), dim3(256), 0, stream, in, n, bsum);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, stream, bsum, (i64)nb);
    hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(256), 0, stream, in, n, bsum, out);
}

#define UT_TRY(expr)                      \
    do {                                  \
        e = (expr);                       \
        if (e != hipSuccess) goto done;   \
    } while (0)

hipError_t sbwt_unitigs_run(const SbwtIndexView &ix, int has_marks, void *d_scratch, SbwtUnitigRun *run, hipStream_t stream,
                            const unsigned *d_ids, const unsigned long long *d_table, int words, unsigned graph) {
    const bool mega = ix.n_mega > 1 || ix.force_mega;
    const i64 n = ix.n_nodes;
    const UtLayout L(n);
    char *base = static_cast<char *>(d_scratch);
    unsigned *pred = reinterpret_cast<unsigned *>(base + L.pred);
    unsigned char *lev = reinterpret_cast<unsigned char *>(base + L.lev);
    u64 *marks = reinterpret_cast<u64 *>(base + L.marks);
    uint4 *st[2] = {reinterpret_cast<uint4 *>(base + L.st0), reinterpret_cast<uint4 *>(base + L.st1)};
    i64 *bsum = reinterpret_cast<i64 *>(base + L.bsum);
    int *open = reinterpret_cast<int *>(base + L.ctl);
    unsigned long long *n_breaks = reinterpret_cast<unsigned long long *>(base + L.ctl + 8);   // (the memset of `open` zeroes it)
    const bool colored = d_ids != nullptr;
    const UtColors cs = {d_ids, reinterpret_cast<const u64 *>(d_table), words};
    unsigned long long h_breaks = 0;
    const unsigned g = grid_for(n);
    hipEvent_t ev[SBWT_UT_N_PASSES + 1] = {};
    hipError_t e = hipSuccess;
    int cur = 0, h_open = 0, max_rounds = 0;
    i64 n_unitigs = 0, total = 0;
    i64 *flag = nullptr, *uid = nullptr;
    hipEvent_t evg[2] = {};
    i64 n_links = 0;
    *run = SbwtUnitigRun();
    for (int i = 0; i <= SBWT_UT_N_PASSES; i++) UT_TRY(hipEventCreate(&ev[i]));

    UT_TRY(hipEventRecord(ev[SBWT_UT_PASS_PRED], stream));
    UT_TRY(hipMemsetAsync(lev, 0, (size_t)ut_pad(n), stream));
    UT_TRY(hipMemsetAsync(open, 0, 256, stream));
    if (mega) hipLaunchKernelGGL(k_ut_pred<true>, dim3(g), dim3(256), 0, stream, ix, pred);
    else hipLaunchKernelGGL(k_ut_pred<false>, dim3(g), dim3(256), 0, stream, ix, pred);
    if (has_marks) hipLaunchKernelGGL(k_ut_marks_copy, dim3(grid_for(n / 64 + 1)), dim3(256), 0, stream, ix, marks, n / 64 + 1);
    else hipLaunchKernelGGL(k_ut_marks_derive, dim3(g), dim3(256), 0, stream, ix, (const unsigned *)pred, marks);

    UT_TRY(hipEventRecord(ev[SBWT_UT_PASS_REAL], stream));
    for (int r = 0; r + 1 < ix.k; r++) {
        if (mega) hipLaunchKernelGGL(k_ut_level<true>, dim3(g), dim3(256), 0, stream, ix, lev, r);
        else hipLaunchKernelGGL(k_ut_level<false>, dim3(g), dim3(256), 0, stream, ix, lev, r);
    }

    UT_TRY(hipEventRecord(ev[SBWT_UT_PASS_LINK], stream));
    if (colored) hipLaunchKernelGGL(k_ut_link<true>, dim3(g), dim3(256), 0, stream, ix, (const unsigned *)pred, (const unsigned char *)lev,
                                    (const u64 *)marks, st[0], open, cs, n_breaks);
    else hipLaunchKernelGGL(k_ut_link<false>, dim3(g), dim3(256), 0, stream, ix, (const unsigned *)pred, (const unsigned char *)lev,
                            (const u64 *)marks, st[0], open, cs, n_breaks);

    UT_TRY(hipEventRecord(ev[SBWT_UT_PASS_RANK], stream));
    while (((i64)1 << max_rounds) < n) max_rounds++;
    UT_TRY(hipMemcpyAsync(&h_open, open, sizeof(int), hipMemcpyDeviceToHost, stream));
    if (colored) UT_TRY(hipMemcpyAsync(&h_breaks, n_breaks, 8, hipMemcpyDeviceToHost, stream));
    UT_TRY(hipStreamSynchronize(stream));
    for (int r = 0; h_open && r < max_rounds; r++) {
        UT_TRY(hipMemsetAsync(open, 0, sizeof(int), stream));
        hipLaunchKernelGGL(k_ut_jump, dim3(g), dim3(256), 0, stream, n, (const uint4 *)st[cur], st[cur ^ 1], 1u << r, open);
        cur ^= 1;
        run->jump_rounds++;
        UT_TRY(hipMemcpyAsync(&h_open, open, sizeof(int), hipMemcpyDeviceToHost, stream));
        UT_TRY(hipStreamSynchronize(stream));
    }
    if (h_open) hipLaunchKernelGGL(k_ut_close, dim3(g), dim3(256), 0, stream, n, st[cur]);

    // the scans work in the half of the ranking state that is free now: flag[n] (later the lengths), uid[n + 1]
    UT_TRY(hipEventRecord(ev[SBWT_UT_PASS_OFFSETS], stream));
    flag = reinterpret_cast<i64 *>(st[cur ^ 1]);
    uid = flag + n;
    hipLaunchKernelGGL(k_ut_starts, dim3(g), dim3(256), 0, stream, n, (const uint4 *)st[cur], flag);
    ut_scan(flag, n, bsum, uid, stream);
    UT_TRY(hipMemcpyAsync(&n_unitigs, uid + n, 8, hipMemcpyDeviceToHost, stream));
    UT_TRY(hipStreamSynchronize(stream));
    UT_TRY(hipMalloc((void **)&run->d_off, (size_t)(n_unitigs + 1) * 8));
    UT_TRY(hipMalloc((void **)&run->d_first_col, (size_t)(n_unitigs ? n_unitigs : 1) * 8));
    if (colored) UT_TRY(hipMalloc((void **)&run->d_set_id, (size_t)(n_unitigs ? n_unitigs : 1) * 4));
#define UT_LENGTHS(M, C)                                                                                                             \
    hipLaunchKernelGGL((k_ut_lengths<M, C>), dim3(g), dim3(256), 0, stream, ix, (const unsigned char *)lev, (const u64 *)marks,      \
                       (const uint4 *)st[cur], (const i64 *)uid, run->d_first_col, flag, cs)
    if (colored) {
        if (mega) UT_LENGTHS(true, true);
        else UT_LENGTHS(false, true);
        if (n_unitigs > 0)
            hipLaunchKernelGGL(k_ut_setids, dim3(grid_for(n_unitigs)), dim3(256), 0, stream, d_ids, n, (const i64 *)run->d_first_col,
                               n_unitigs, run->d_set_id);
    } else {
        if (mega) UT_LENGTHS(true, false);
        else UT_LENGTHS(false, false);
    }
#undef UT_LENGTHS
    ut_scan(flag, n_unitigs, bsum, run->d_off, stream);
    UT_TRY(hipMemcpyAsync(&total, run->d_off + n_unitigs, 8, hipMemcpyDeviceToHost, stream));
    UT_TRY(hipStreamSynchronize(stream));
    UT_TRY(hipMalloc((void **)&run->d_bases, (size_t)(total ? total : 1)));

    UT_TRY(hipEventRecord(ev[SBWT_UT_PASS_BASES], stream));
    if (n_unitigs > 0) {
        hipLaunchKernelGGL(k_ut_chars, dim3(g), dim3(256), 0, stream, ix, (const uint4 *)st[cur], (const i64 *)uid,
                           (const i64 *)run->d_off, run->d_bases);
        hipLaunchKernelGGL(k_ut_labels, dim3(grid_for(n_unitigs)), dim3(256), 0, stream, ix, (const unsigned *)pred,
                           (const i64 *)run->d_first_col, (const i64 *)run->d_off, n_unitigs, run->d_bases);
    }
    UT_TRY(hipEventRecord(ev[SBWT_UT_N_PASSES], stream));
    if (graph) {
        for (int i = 0; i < 2; i++) UT_TRY(hipEventCreate(&evg[i]));
        if (graph & SBWT_UT_GRAPH_LINKS) {
            // the degrees take the place of the lengths, which the offsets were scanned from
            UT_TRY(hipMalloc((void **)&run->d_link_off, (size_t)(n_unitigs + 1) * 8));
#define UT_LINK_COUNT(M, C)                                                                                                          \
    hipLaunchKernelGGL((k_ut_link_count<M, C>), dim3(g), dim3(256), 0, stream, ix, (const unsigned char *)lev, (const u64 *)marks,   \
                       (const uint4 *)st[cur], (const i64 *)uid, flag, cs)
            if (colored) {
                if (mega) UT_LINK_COUNT(true, true);
                else UT_LINK_COUNT(false, true);
            } else {
                if (mega) UT_LINK_COUNT(true, false);
                else UT_LINK_COUNT(false, false);
            }
#undef UT_LINK_COUNT
            ut_scan(flag, n_unitigs, bsum, run->d_link_off, stream);
            UT_TRY(hipMemcpyAsync(&n_links, run->d_link_off + n_unitigs, 8, hipMemcpyDeviceToHost, stream));
            UT_TRY(hipStreamSynchronize(stream));
            UT_TRY(hipMalloc((void **)&run->d_link_to, (size_t)(n_links ? n_links : 1) * 4));
#define UT_LINK_FILL(M, C)                                                                                                           \
    hipLaunchKernelGGL((k_ut_link_fill<M, C>), dim3(g), dim3(256), 0, stream, ix, (const unsigned char *)lev, (const u64 *)marks,    \
                       (const uint4 *)st[cur], (const i64 *)uid, (const i64 *)run->d_link_off, run->d_link_to, cs)
            if (n_links > 0) {
                if (colored) {
                    if (mega) UT_LINK_FILL(true, true);
                    else UT_LINK_FILL(false, true);
                } else {
                    if (mega) UT_LINK_FILL(true, false);
                    else UT_LINK_FILL(false, false);
                }
            }
#undef UT_LINK_FILL
        }
        UT_TRY(hipEventRecord(evg[0], stream));
        if (graph & SBWT_UT_GRAPH_COLUMN_MAP) {
            UT_TRY(hipMalloc((void **)&run->d_col_unitig, (size_t)n * 4));
            UT_TRY(hipMalloc((void **)&run->d_col_offset, (size_t)n * 4));
            hipLaunchKernelGGL(k_ut_colmap, dim3(g), dim3(256), 0, stream, n, (const uint4 *)st[cur], (const i64 *)uid, run->d_col_unitig,
                               run->d_col_offset);
        }
        UT_TRY(hipEventRecord(evg[1], stream));
    }
    UT_TRY(hipGetLastError());
    UT_TRY(hipStreamSynchronize(stream));
    for (int i = 0; i < SBWT_UT_N_PASSES; i++) UT_TRY(hipEventElapsedTime(&run->ms[i], ev[i], ev[i + 1]));
    if (graph) {
        UT_TRY(hipEventElapsedTime(&run->links_ms, ev[SBWT_UT_N_PASSES], evg[0]));
        UT_TRY(hipEventElapsedTime(&run->map_ms, evg[0], evg[1]));
    }
    run->n_links = n_links;
    run->n_unitigs = n_unitigs;
    run->total_bases = total;
    run->n_color_breaks = (long long)h_breaks;
done:
    for (int i = 0; i <= SBWT_UT_N_PASSES; i++)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    for (int i = 0; i < 2; i++)
        if (evg[i]) (void)hipEventDestroy(evg[i]);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(stream);
        (void)hipGetLastError();
        if (run->d_bases) (void)hipFree(run->d_bases);
        if (run->d_off) (void)hipFree(run->d_off);
        if (run->d_first_col) (void)hipFree(run->d_first_col);
        if (run->d_set_id) (void)hipFree(run->d_set_id);
        if (run->d_link_off) (void)hipFree(run->d_link_off);
        if (run->d_link_to) (void)hipFree(run->d_link_to);
        if (run->d_col_unitig) (void)hipFree(run->d_col_unitig);
        if (run->d_col_offset) (void)hipFree(run->d_col_offset);
        *run = SbwtUnitigRun();
    }
    return e;
}

hipError_t sbwt_unitigs_locate(const unsigned *d_col_unitig, const unsigned *d_col_offset, long long n_nodes, const long long *d_cols,
                               long long n, unsigned *d_unitig, unsigned *d_offset, hipStream_t stream) {
    const i64 chunk = (i64)1 << 30;                          // (one dispatch holds fewer than 2^32 work-items)
    for (i64 at = 0; at < n; at += chunk) {
        const i64 m = n - at < chunk ? n - at : chunk;
        hipLaunchKernelGGL(k_ut_locate, dim3(grid_for(m)), dim3(256), 0, stream, d_col_unitig, d_col_offset, (i64)n_nodes,
                           (const i64 *)d_cols + at, m, d_unitig + at, d_offset + at);
    }
    return hipGetLastError();
}
