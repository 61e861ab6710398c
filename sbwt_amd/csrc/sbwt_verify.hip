// sbwt_verify.hip -- the reference sequences packed on the device, and mapped reads verified against them: the mismatches on
// the voted diagonal and the best edit distance in a window around it (include/sbwtgpu.h, "reference sequences and
// verification").  Everything is exact integers.
//
//   k_ref_pack     ASCII -> 2 bits per base + one validity bit per base, one lane per 2-bit word (32 bases, two 16-byte loads);
//                  the even lane of a pair also writes the validity word of the pair's 64 bases.  A sequence starts at a
//                  multiple of 64 bases, so no two sequences share a word and nothing here needs an atomic but the count of
//                  invalid bases (one per wave).
//   k_ref_unpack   (sequence, pos, len) -> ASCII, N for an invalid base: what sbwtgpu_refseqs_get returns.
//   k_verify       ONE LANE PER READ.  Myers' bit-vector form of Sellers' table is sequential over the window's columns and
//                  parallel over 64 rows per machine word, so 64 reads per wave keep every lane busy.  A lane builds
//                  Peq[4][w] from its oriented read and walks the columns with the block form of the recurrence (Ph / Mh carry
//                  between the words, no carry enters at row 0: the start in the text is free); it tracks the score of row L,
//                  its minimum and the minimum's first column.  The match bit of column B + j, row j is the mismatch count's.
//                  State in registers for w <= 4; the wave takes the instantiation of its longest read.  Longer reads go
//                  onto a list.
//   k_verify_slow  grid-stride over that list, its length read on the device: the same recurrence with up to 16 words of state
//                  per lane in LDS, laid out [word][lane]; reads above SBWT_VF_MAX_READ get their mismatches from a linear pass.
#include "sbwt_kernels_common.h"
#include "sbwt_verify.h"
#include "sbwt_verify_text.h"

typedef unsigned u32x4_a1 __attribute__((ext_vector_type(4), aligned(1)));

// ---------------------------------------------------------------------------------------------
// the object: pack and unpack
// ---------------------------------------------------------------------------------------------
// four bases of a dword into word / v at base q of the lane's 32
__device__ __forceinline__ void vf_pack4(unsigned x, int q, u64 &word, unsigned &v) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned c = vf_code((x >> (8 * k)) & 0xffu);
        if (c != VF_NONE) {
            word |= (u64)c << (2 * (q + k));
            v |= 1u << (q + k);
        }
    }
}

__global__ void __launch_bounds__(256) k_ref_pack(const char *__restrict__ src, const i64 *__restrict__ src_off,
                                                  const SbwtRefSeq *__restrict__ tab, i64 first_seq, i64 n, i64 slot_lo, i64 slot_hi,
                                                  u64 *__restrict__ bits, u64 *__restrict__ valid, SbwtRefCounters *ctr) {
    const int lane = threadIdx.x & 63;
    const i64 n_words = 2 * (slot_hi - slot_lo);           // even: the two lanes of a pair are in range together
    u64 invalid = 0;
    for (i64 g0 = (i64)blockIdx.x * 256 + (threadIdx.x & ~63u); g0 < n_words; g0 += (i64)gridDim.x * 256) {
        const i64 g = g0 + lane;
        u64 word = 0;
        unsigned v = 0;
        if (g < n_words) {
            const i64 slot = slot_lo + (g >> 1);
            i64 lo = 0, hi = n;                            // tab[first_seq + lo].slot <= slot < tab[first_seq + hi].slot (hi = n: slot_hi)
            while (hi - lo > 1) {
                const i64 mid = (lo + hi) >> 1;
                if (tab[first_seq + mid].slot <= slot) lo = mid;
                else hi = mid;
            }
            const SbwtRefSeq s = tab[first_seq + lo];
            const i64 p0 = (g - 2 * (s.slot - slot_lo)) * 32;       // the word's first base in its sequence
            const i64 nb = s.len - p0 < 32 ? s.len - p0 : 32;       // (<= 0: the word is padding)
            const char *p = src + src_off[lo] + p0;
            if (nb == 32) {
                const u32x4_a1 a = *reinterpret_cast<const u32x4_a1 *>(p), b = *reinterpret_cast<const u32x4_a1 *>(p + 16);
                vf_pack4(a.x, 0, word, v); vf_pack4(a.y, 4, word, v); vf_pack4(a.z, 8, word, v); vf_pack4(a.w, 12, word, v);
                vf_pack4(b.x, 16, word, v); vf_pack4(b.y, 20, word, v); vf_pack4(b.z, 24, word, v); vf_pack4(b.w, 28, word, v);
            } else {
                for (i64 q = 0; q < nb; q++) {
                    const unsigned c = vf_code((unsigned char)p[q]);
                    if (c != VF_NONE) {
                        word |= (u64)c << (2 * q);
                        v |= 1u << q;
                    }
                }
            }
            if (nb > 0) invalid += (u64)(nb - __popc(v));
            bits[2 * slot_lo + g] = word;
        }
        const unsigned other = __shfl_xor(v, 1);
        if (g < n_words && (g & 1) == 0) valid[slot_lo + (g >> 1)] = (u64)v | ((u64)other << 32);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) invalid += __shfl_down(invalid, off);
    if (lane == 0 && invalid) atomicAdd(&ctr->n_invalid, invalid);
}

void sbwt_launch_ref_pack(const char *d_src, const long long *d_src_off, const SbwtRefSeq *tab, long long first_seq, long long n,
                          long long slot_lo, long long slot_hi, unsigned long long *d_bits, unsigned long long *d_valid,
                          SbwtRefCounters *ctr, hipStream_t stream) {
    if (n <= 0 || slot_hi <= slot_lo) return;
    const i64 blocks = (2 * (slot_hi - slot_lo) + 255) / 256;
    hipLaunchKernelGGL(k_ref_pack, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, stream, d_src, (const i64 *)d_src_off, tab,
                       (i64)first_seq, (i64)n, (i64)slot_lo, (i64)slot_hi, (u64 *)d_bits, (u64 *)d_valid, ctr);
}

__global__ void __launch_bounds__(256) k_ref_unpack(const u64 *__restrict__ bits, const u64 *__restrict__ valid, i64 pos, i64 len,
                                                    char *__restrict__ out) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < len; i += (i64)gridDim.x * 256) {
        const i64 p = pos + i;
        const bool ok = (valid[p >> 6] >> (p & 63)) & 1ull;
        out[i] = ok ? "ACGT"[(bits[p >> 5] >> (2 * (p & 31))) & 3ull] : 'N';
    }
}

void sbwt_launch_ref_unpack(const unsigned long long *d_bits, const unsigned long long *d_valid, long long slot, long long pos,
                            long long len, char *d_out, hipStream_t stream) {
    if (len <= 0) return;
    const i64 blocks = (len + 255) / 256;
    hipLaunchKernelGGL(k_ref_unpack, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, stream, (const u64 *)d_bits + 2 * slot,
                       (const u64 *)d_valid + slot, (i64)pos, (i64)len, d_out);
}

// ---------------------------------------------------------------------------------------------
// verification
// ---------------------------------------------------------------------------------------------
struct VfRead {
    i64 off, L, start;
    int strand;
    VfText T;
};
// Read r's record and sequence.  false: its record is final and written here (unverified, or a read of no bases).
__device__ __forceinline__ bool vf_open(i64 r, i64 total, const i64 *__restrict__ read_off, const SbwtVerifyMap *__restrict__ map,
                                        const SbwtRefSeq *__restrict__ tab, i64 n_seqs, const u64 *__restrict__ bits,
                                        const u64 *__restrict__ valid, int B, SbwtReadVerify *__restrict__ out, VfRead &R) {
    R.off = read_off[r];
    R.L = read_off[r + 1] - R.off;
    R.start = map[r].start;
    R.strand = map[r].strand;
    const i64 seq = map[r].seq;
    const i64 lim = (i64)1 << 40;
    if (seq < 0 || seq >= n_seqs || (R.strand != 0 && R.strand != 1) || R.start >= lim || R.start <= -lim ||
        R.L < 0 || R.L >= ((i64)1 << 31) || R.off < 0 || R.off + R.L > total) {     // (the last four: offsets that are not a batch's)
        out[r] = SbwtReadVerify{0, -1, -1};
        return false;
    }
    if (R.L == 0) {
        out[r] = SbwtReadVerify{R.start - B, 0, 0};
        return false;
    }
    const SbwtRefSeq s = tab[seq];
    R.T = VfText{bits + 2 * s.slot, valid + s.slot, s.len, 0, 0, false};
    return true;
}

// one word of rows, one column: Myers' block step.  hp / hm: the horizontal delta that enters at the word's row 0 (+1 / -1) and,
// afterwards, the one that leaves at its row 63; ph / mh come back unshifted, for the score of a row inside the word.
__device__ __forceinline__ void vf_block(u64 eq, u64 &pv, u64 &mv, u64 &hp, u64 &hm, u64 &ph, u64 &mh) {
    const u64 xv = eq | mv;
    eq |= hm;
    const u64 xh = (((eq & pv) + pv) ^ pv) | eq;
    ph = mv | ~(xh | pv);
    mh = pv & xh;
    const u64 ps = (ph << 1) | hp, ms = (mh << 1) | hm;
    hp = ph >> 63;
    hm = mh >> 63;
    pv = ms | ~(xv | ps);
    mv = ps & xv;
}

// A read of at most 64 W bases with its rows in registers
template <int W>
__device__ __forceinline__ void vf_fast(const char *__restrict__ bases, i64 total, VfRead &R, int B, SbwtReadVerify &res) {
    const int L = (int)R.L;
    const unsigned comp = R.strand ? 3u : 0u;
    u64 peq[4][W], pv[W], mv[W];
#pragma unroll
    for (int w = 0; w < W; w++) {
        peq[0][w] = peq[1][w] = peq[2][w] = peq[3][w] = 0;
        pv[w] = ~0ull;
        mv[w] = 0;
        for (int j0 = 64 * w; j0 < L && j0 < 64 * w + 64; j0 += 8) {
            u64 x = vf_read8(bases, total, R.off, L, R.strand, j0);
            const int nk = L - j0 < 8 ? L - j0 : 8;
            for (int q = 0; q < nk; q++, x >>= 8) {
                const unsigned c = vf_code((unsigned)x & 0xffu) ^ comp;     // (VF_NONE stays above 3)
                const u64 bit = 1ull << (j0 - 64 * w + q);
                peq[0][w] |= c == 0 ? bit : 0;
                peq[1][w] |= c == 1 ? bit : 0;
                peq[2][w] |= c == 2 ? bit : 0;
                peq[3][w] |= c == 3 ? bit : 0;
            }
        }
    }
    const int wl = (L - 1) >> 6;
    const u64 top = 1ull << ((L - 1) & 63);
    const int n_cols = L + 2 * B;
    int score = L, best = L, best_t = 0, mm = 0;
    i64 p = R.start - B;
    for (int t = 0; t < n_cols; t++, p++) {
        const unsigned c = vf_text(R.T, p);
        const int j = t - B;                               // the row of this column on the voted diagonal
        const bool on_diag = (unsigned)j < (unsigned)L;
        u64 hp = 0, hm = 0;
#pragma unroll
        for (int w = 0; w < W; w++) {
            const u64 eq = c == 0 ? peq[0][w] : c == 1 ? peq[1][w] : c == 2 ? peq[2][w] : c == 3 ? peq[3][w] : 0;
            if (on_diag && (j >> 6) == w) mm += (int)(~(eq >> (j & 63)) & 1ull);
            u64 ph, mh;
            vf_block(eq, pv[w], mv[w], hp, hm, ph, mh);
            if (w == wl) score += (int)((ph & top) != 0) - (int)((mh & top) != 0);
        }
        if (score < best) {
            best = score;
            best_t = t + 1;
        }
    }
    res = SbwtReadVerify{R.start - B + best_t, mm, best};
}

__global__ void __launch_bounds__(256) k_verify(const char *__restrict__ bases, i64 total, const i64 *__restrict__ read_off, i64 n_reads,
                                                const SbwtVerifyMap *__restrict__ map, const SbwtRefSeq *__restrict__ tab, i64 n_seqs,
                                                const u64 *__restrict__ bits, const u64 *__restrict__ valid, int B, int fast_bases,
                                                SbwtReadVerify *__restrict__ out, SbwtVerifyHeader *hdr, unsigned *__restrict__ slow) {
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    VfRead R;
    bool mine = false;
    if (r < n_reads && vf_open(r, total, read_off, map, tab, n_seqs, bits, valid, B, out, R)) {
        if (R.L > fast_bases) slow[atomicAdd(&hdr->n_slow, 1u)] = (unsigned)r;      // the second kernel writes this read's record
        else mine = true;
    }
    int words = mine ? (int)((R.L + 63) >> 6) : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(words, off);
        if (o > words) words = o;
    }
    words = (int)uniform32((unsigned)words);               // the wave's longest read chooses the instantiation
    if (!mine) return;
    SbwtReadVerify res;
    switch (words) {
        case 1: vf_fast<1>(bases, total, R, B, res); break;
        case 2: vf_fast<2>(bases, total, R, B, res); break;
        case 3: vf_fast<3>(bases, total, R, B, res); break;
        default: vf_fast<4>(bases, total, R, B, res); break;
    }
    out[r] = res;
}

// The reads of the list: up to 16 words of rows per lane in LDS, [array][word][lane] (a lane only ever touches its own
// column, 8 bytes wide: no two lanes of a wave share a bank in one access and nothing needs a barrier)
#define VF_SLOW_WORDS (SBWT_VF_MAX_READ / 64)
__global__ void __launch_bounds__(64) k_verify_slow(const char *__restrict__ bases, i64 total, const i64 *__restrict__ read_off, i64 n_reads,
                                                    const SbwtVerifyMap *__restrict__ map, const SbwtRefSeq *__restrict__ tab, i64 n_seqs,
                                                    const u64 *__restrict__ bits, const u64 *__restrict__ valid, int B,
                                                    SbwtReadVerify *__restrict__ out, const SbwtVerifyHeader *hdr,
                                                    const unsigned *__restrict__ slow) {
    __shared__ u64 st[6][VF_SLOW_WORDS][64];               // Peq[4], Pv, Mv
    const int lane = threadIdx.x;
    i64 n_slow = hdr->n_slow;
    if (n_slow > n_reads) n_slow = n_reads;                // (never: a read is listed once)
    for (i64 e = (i64)blockIdx.x * 64 + lane; e < n_slow; e += (i64)gridDim.x * 64) {
        const i64 r = slow[e];
        VfRead R;
        if (r >= n_reads || !vf_open(r, total, read_off, map, tab, n_seqs, bits, valid, B, out, R)) continue;    // (never)
        if (R.L > SBWT_VF_MAX_READ) continue;              // (the loop below)
        const unsigned comp = R.strand ? 3u : 0u;
        const int L = (int)R.L, nw = (L + 63) >> 6;
        for (int w = 0; w < nw; w++) {
            st[0][w][lane] = st[1][w][lane] = st[2][w][lane] = st[3][w][lane] = 0;
            st[4][w][lane] = ~0ull;
            st[5][w][lane] = 0;
        }
        for (int j0 = 0; j0 < L; j0 += 8) {
            u64 x = vf_read8(bases, total, R.off, L, R.strand, j0);
            const int nk = L - j0 < 8 ? L - j0 : 8;
            for (int q = 0; q < nk; q++, x >>= 8) {
                const unsigned c = vf_code((unsigned)x & 0xffu) ^ comp;
                if (c < 4) st[c][(j0 + q) >> 6][lane] |= 1ull << ((j0 + q) & 63);
            }
        }
        const int wl = nw - 1;
        const u64 top = 1ull << ((L - 1) & 63);
        const int n_cols = L + 2 * B;
        int score = L, best = L, best_t = 0, mm = 0;
        i64 p = R.start - B;
        for (int t = 0; t < n_cols; t++, p++) {
            const unsigned c = vf_text(R.T, p);
            const int j = t - B;
            if ((unsigned)j < (unsigned)L) mm += !(c < 4 && ((st[c][j >> 6][lane] >> (j & 63)) & 1ull));
            u64 hp = 0, hm = 0, ph = 0, mh = 0;
            for (int w = 0; w < nw; w++) {
                const u64 eq = c < 4 ? st[c][w][lane] : 0;
                u64 pv = st[4][w][lane], mv = st[5][w][lane];
                vf_block(eq, pv, mv, hp, hm, ph, mh);
                st[4][w][lane] = pv;
                st[5][w][lane] = mv;
            }
            score += (int)((ph & top) != 0) - (int)((mh & top) != 0);      // (ph, mh: the last word's)
            if (score < best) {
                best = score;
                best_t = t + 1;
            }
        }
        out[r] = SbwtReadVerify{R.start - B + best_t, mm, best};
    }
    // The reads too long for the table: their mismatches from a linear pass along the diagonal.  (A loop of its own over the
    // list: inside the loop above its nest costs the kernel its last scalar registers.)
    for (i64 e = (i64)blockIdx.x * 64 + lane; e < n_slow; e += (i64)gridDim.x * 64) {
        const i64 r = slow[e];
        VfRead R;
        if (r >= n_reads || !vf_open(r, total, read_off, map, tab, n_seqs, bits, valid, B, out, R) || R.L <= SBWT_VF_MAX_READ) continue;
        const unsigned comp = R.strand ? 3u : 0u;
        int mm = 0;
        i64 p = R.start;
        for (i64 j0 = 0; j0 < R.L; j0 += 8) {
            u64 x = vf_read8(bases, total, R.off, R.L, R.strand, j0);
            const int nk = R.L - j0 < 8 ? (int)(R.L - j0) : 8;
            for (int q = 0; q < nk; q++, x >>= 8, p++) {
                const unsigned c = vf_code((unsigned)x & 0xffu) ^ comp;
                const unsigned tc = vf_text(R.T, p);       // (at every p: it reloads its words as p passes their edges)
                mm += !(c < 4 && c == tc);
            }
        }
        out[r] = SbwtReadVerify{0, mm, -1};
    }
}

void sbwt_launch_verify(const char *d_bases, long long total_bases, const long long *d_read_off, long long n_reads,
                        const SbwtVerifyMap *d_map, const SbwtRefSeq *tab, long long n_seqs, const unsigned long long *d_bits,
                        const unsigned long long *d_valid, int band, int fast_bases, SbwtReadVerify *d_out, SbwtVerifyHeader *hdr,
                        unsigned *d_slow, hipStream_t stream) {
    if (fast_bases < 1 || fast_bases > SBWT_VF_FAST_BASES) fast_bases = SBWT_VF_FAST_BASES;
    (void)hipMemsetAsync(hdr, 0, sizeof(SbwtVerifyHeader), stream);
    const i64 blocks = (n_reads + 255) / 256, slow_blocks = (n_reads + 63) / 64;
    hipLaunchKernelGGL(k_verify, dim3((unsigned)(blocks < 1 ? 1 : blocks)), dim3(256), 0, stream, d_bases, (i64)total_bases,
                       (const i64 *)d_read_off, (i64)n_reads, d_map, tab, (i64)n_seqs, (const u64 *)d_bits, (const u64 *)d_valid, band,
                       fast_bases, d_out, hdr, d_slow);
    hipLaunchKernelGGL(k_verify_slow, dim3((unsigned)(slow_blocks < 1 ? 1 : slow_blocks > 1024 ? 1024 : slow_blocks)), dim3(64), 0, stream,
                       d_bases, (i64)total_bases, (const i64 *)d_read_off, (i64)n_reads, d_map, tab, (i64)n_seqs, (const u64 *)d_bits,
                       (const u64 *)d_valid, band, d_out, hdr, d_slow);
}
