// sbwt_posmap.h -- what the map kernels of sbwt_positions.hip and sbwt_occurrences.hip (section 27) share:
// the placement key, the per-lane (best, runner-up) fold, the butterfly that writes a record, the wave's table in LDS and the
// peel that fills it, the end of a read, the result frame of the adds (k_pos_add, k_occ_add), and the launchers' grid clamp
// and strands dispatch.
#pragma once
#include <type_traits>
#include "sbwt_kernels_common.h"
#include "sbwt_positions.h"

#define PM_NOKEY (~0ull)

__device__ __forceinline__ u64 pm_readlane64(u64 v, int src) {
    return (u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src) |
           ((u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src) << 32);
}

// The placement (seq, o, start) that a hit of window i (of m), search s, on a column with position f votes for, as one
// integer: seq < 2^30 in bits 33 .., o in bit 32, start + 2^31 in the low word (start lies in (-2^30, 2^31)).  Unsigned order
// of the keys is the lexicographic order of the triples with start signed.
__device__ __forceinline__ u64 pm_key(u64 f, i64 i, i64 m, unsigned s) {
    const u64 seq = f >> 32;
    const i64 pos = (i64)(((unsigned)f) >> 1);
    const unsigned o = s ^ ((unsigned)f & 1u);
    const i64 start = o ? pos - (m - 1 - i) : pos - i;
    return (seq << 33) | ((u64)o << 32) | (u64)(unsigned)(start + ((i64)1 << 31));
}

// a lane's candidates for the winner and for the best of the rest: (bc, bk) the most votes and among those the smallest key,
// sc the most votes of a key other than bk.  Keys may repeat (each time with the same count).
struct PmBest { u64 bk; int bc, sc; };
__device__ __forceinline__ void pm_offer(PmBest &b, u64 key, int c) {
    if (key == b.bk) return;
    if (c > b.bc || (c == b.bc && key < b.bk)) {
        if (b.bc > b.sc) b.sc = b.bc;
        b.bk = key;
        b.bc = c;
    } else if (c > b.sc) {
        b.sc = c;
    }
}

// the wave's lanes' candidates -> the record (every lane calls it; lane 0 writes)
__device__ __forceinline__ void pm_write(PmBest b, int found, int anchored, SbwtReadMap *out, int lane) {
    u64 wk = b.bk;
    int wc = b.bc;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 ok = __shfl_xor(wk, off);
        const int oc = __shfl_xor(wc, off);
        if (oc > wc || (oc == wc && ok < wk)) { wk = ok; wc = oc; }
    }
    // a lane whose best is not the winner holds no entry of the winner's key: its best is the best of its rest
    int v2 = b.bk == wk ? b.sc : b.bc;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o2 = __shfl_xor(v2, off);
        if (o2 > v2) v2 = o2;
    }
    if (lane == 0) {
        SbwtReadMap r;
        if (anchored == 0) {
            r.start = 0; r.seq = -1; r.strand = 0; r.votes = 0; r.votes2 = 0;
        } else {
            r.start = (i64)(unsigned)wk - ((i64)1 << 31);
            r.seq = (int)(wk >> 33);
            r.strand = (int)((wk >> 32) & 1ull);
            r.votes = wc;
            r.votes2 = v2;
        }
        r.n_found = found;
        r.n_anchored = anchored;
        *out = r;
    }
}

// The run (key, c) into the wave's table of n_ent entries (n_ent, key, c are the same in every lane).  false: the table
// holds `cap` other keys already.
__device__ __forceinline__ bool pm_put(u64 *keys, int *cnt, int &n_ent, int cap, u64 key, int c, int lane) {
    for (int b = 0; b < n_ent; b += 64) {
        const int j = b + lane;
        const bool eq = j < n_ent && keys[j] == key;
        if (__ballot(eq)) {
            if (eq) cnt[j] += c;
            __builtin_amdgcn_wave_barrier();
            return true;
        }
    }
    if (n_ent >= cap) return false;
    if (lane == 0) { keys[n_ent] = key; cnt[n_ent] = c; }
    n_ent++;
    __builtin_amdgcn_wave_barrier();
    return true;
}

// The iteration's distinct keys of one trip, peeled (readlane, ballot, popcount), against a pending run: a key that continues
// the run adds to it, another one sends the run to the table and starts the next.
__device__ __forceinline__ void pm_peel_pending(u64 mine, u64 &pend_key, int &pend_n, u64 *keys, int *cnt, int &n_ent, int cap, bool &fits,
                                                int lane) {
    u64 live = __ballot(mine != PM_NOKEY);
    while (live) {                                        // one trip per distinct key
        const int src = __ffsll((i64)live) - 1;
        const u64 k0 = pm_readlane64(mine, src);
        const u64 eq = __ballot(mine == k0);
        live &= ~eq;
        if (pend_n != 0 && k0 == pend_key) {
            pend_n += __popcll(eq);
        } else {
            if (pend_n != 0 && fits) fits = pm_put(keys, cnt, n_ent, cap, pend_key, pend_n, lane);
            pend_key = k0;
            pend_n = __popcll(eq);
        }
    }
}
// the same without a run: every distinct key goes to the table
__device__ __forceinline__ void pm_peel_put(u64 mine, u64 *keys, int *cnt, int &n_ent, int cap, bool &fits, int lane) {
    u64 live = __ballot(mine != PM_NOKEY);
    while (live && fits) {
        const int src = __ffsll((i64)live) - 1;
        const u64 k0 = pm_readlane64(mine, src);
        const u64 eq = __ballot(mine == k0);
        live &= ~eq;
        fits = pm_put(keys, cnt, n_ent, cap, k0, __popcll(eq), lane);
    }
}

// The end of read r in the first map kernels: a read whose table overflowed goes onto the list for the second kernel, any
// other one's table is folded and its record written.
__device__ __forceinline__ void pm_end_read(bool fits, u64 *keys, int *cnt, int n_ent, int found, int anchored, i64 r,
                                            SbwtReadMap *__restrict__ out, SbwtPosMapHeader *hdr, unsigned *__restrict__ slow, int lane) {
    if (fits) {
        PmBest b = {PM_NOKEY, 0, 0};
        for (int j = lane; j < n_ent; j += 64) pm_offer(b, keys[j], cnt[j]);
        __builtin_amdgcn_wave_barrier();                  // (the next read's first entry comes after these loads)
        pm_write(b, found, anchored, out + r, lane);
    } else if (lane == 0) {                               // the second kernel writes this read's record
        slow[atomicAdd(&hdr->n_slow, 1u)] = (unsigned)r;
    }
}

// Every result of a batch's searches, and of the mirrored batch's behind them, a lane per result: the frame of the adds.  A
// hit finds its sequence and offset by bisecting the window offsets and forms the key (seq << 32) | (pos << 1) | t; f(hit, v,
// key) runs in every lane of the wave (an append needs the ballot).  *n_windows grows by the results, *n_hits by the hits,
// *n_hit_windows by the windows with a hit on either strand.
template <typename F>
__device__ __forceinline__ void pm_for_each_result(const int *__restrict__ res, const int *__restrict__ res2, const i64 *__restrict__ out_off,
                                                   i64 n_reads, i64 first_seq, i64 n_nodes, u64 *n_windows, u64 *n_hits, u64 *n_hit_windows,
                                                   F f) {
    const int lane = threadIdx.x & 63;
    const i64 W = out_off[n_reads];
    const i64 total = res2 ? 2 * W : W;                    // the mirrored batch's results follow the forward ones
    if (blockIdx.x == 0 && threadIdx.x == 0 && total > 0) atomicAdd(n_windows, (u64)total);
    u64 hits = 0, hit_windows = 0;                         // of this lane's wave (the same in every lane)
    // (whole waves go round together: the bound is rounded up to the wave, and a lane past the end sits the ballots out)
    for (i64 i0 = (i64)blockIdx.x * 256 + (threadIdx.x & ~63u); i0 < total; i0 += (i64)gridDim.x * 256) {
        const i64 i = i0 + lane;
        i64 v = -1, p = 0;
        u64 t = 0;
        bool either = false;
        if (i < W) {
            v = res[i];
            p = i;
            either = v >= 0 || (res2 && res2[W - 1 - i] >= 0);
        } else if (i < total) {
            v = res2[i - W];
            p = W - 1 - (i - W);                           // the window of the batch as given that this result belongs to
            t = 1;
        }
        const bool hit = v >= 0 && v < n_nodes;
        u64 key = 0;
        if (hit) {
            i64 lo = 0, hi = n_reads;                      // out_off[lo] <= p < out_off[hi]
            while (hi - lo > 1) {
                const i64 mid = (lo + hi) >> 1;
                if (out_off[mid] <= p) lo = mid;
                else hi = mid;
            }
            key = ((u64)(first_seq + lo) << 32) | ((u64)(p - out_off[lo]) << 1) | t;
        }
        f(hit, v, key);
        hits += (u64)__popcll(__ballot(hit));
        hit_windows += (u64)__popcll(__ballot(either));
    }
    if (lane == 0 && hits) atomicAdd(n_hits, hits);
    if (lane == 0 && hit_windows) atomicAdd(n_hit_windows, hit_windows);
}

// ---- launch helpers ----
// blocks for n items at per_block a block: at least one, at most `most`
static inline unsigned pm_grid(i64 n, i64 per_block, i64 most) {
    const i64 g = (n + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : g > most ? most : g);
}
// f(std::true_type) for two strands, f(std::false_type) for one: a launcher names each kernel template once
template <typename F>
static inline void pm_strands(bool two, F f) {
    if (two) f(std::true_type());
    else f(std::false_type());
}
