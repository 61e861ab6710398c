// sbwt_verify_text.h -- what the kernels over mapped reads share (sbwt_verify.hip, sbwt_align.hip): the code of a base, the
// packed reference sequence as a lane walks it upwards, and eight bases of the oriented read.  Device code only.
#pragma once
#include "sbwt_kernels_common.h"

typedef u64 u64_a1 __attribute__((aligned(1)));

#define VF_NONE 4u      // the code of a base that matches nothing: invalid, or outside its sequence

__device__ __forceinline__ unsigned vf_code(unsigned b) { return is_ACGT(b) ? dna_code(b) : VF_NONE; }

// The reference sequence of a read as its lane walks it, coordinate by coordinate upwards: one 64-bit load per 32 columns and
// one validity word per 64.
struct VfText {
    const u64 *bits, *valid;    // the sequence's own words
    i64 n;
    u64 tw, vw;
    bool loaded;
};
// the code of coordinate p (0 .. 3), VF_NONE outside [0, n) and on an invalid base.  p goes up by one from call to call.
__device__ __forceinline__ unsigned vf_text(VfText &T, i64 p) {
    if ((u64)p >= (u64)T.n) return VF_NONE;
    if (!T.loaded || (p & 31) == 0) {
        T.tw = T.bits[p >> 5];
        if (!T.loaded || (p & 63) == 0) T.vw = T.valid[p >> 6];
        T.loaded = true;
    }
    return ((T.vw >> (p & 63)) & 1ull) ? (unsigned)(T.tw >> (2 * (p & 31))) & 3u : VF_NONE;
}

// eight bytes of the batch at a, those past its end as zero
__device__ __forceinline__ u64 vf_load8(const char *__restrict__ bases, i64 total, i64 a) {
    if (a + 8 <= total) return *reinterpret_cast<const u64_a1 *>(bases + a);
    u64 x = 0;
    for (int k = 0; k < 8 && a + k < total; k++) x |= (u64)(unsigned char)bases[a + k] << (8 * k);
    return x;
}
// Byte q of the result is the base at position j0 + q of the oriented read, not yet complemented (the caller complements the
// code); bytes at positions >= L are junk.  The read is bases[off .. off + L), j0 < L.
__device__ __forceinline__ u64 vf_read8(const char *__restrict__ bases, i64 total, i64 off, i64 L, int strand, i64 j0) {
    if (!strand) return vf_load8(bases, total, off + j0);
    const i64 m0 = L - 8 - j0;                             // (> -8)
    if (m0 >= 0) return __builtin_bswap64(vf_load8(bases, total, off + m0));
    return __builtin_bswap64(vf_load8(bases, total, off)) >> (8 * (int)(-m0));
}
