// sbwt_posmap.h -- what the map kernels of sbwt_positions.hip and sbwt_occurrences.hip (section 27) share:
// the placement key, the per-lane (best, runner-up) fold, the butterfly that writes a record, and the wave's table in LDS.
#pragma once
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
