// sbwt_readhits.h -- per-read hit profiles (sbwt_readhits.hip): what the C-ABI host code launches.
#pragma once
#include <hip/hip_runtime.h>
#include "sbwt_device.h"

// Reads of fewer windows than this are reduced by one lane each, longer ones by a whole wave ("read_hits_wave_min").
// 1024 windows are 16 words of the bit vector: a lane walks them in a few hundred cycles, and a wave's iteration over
// 64 words with its cross-lane combine only pays from there.
#define SBWT_RH_WAVE_MIN 1024

// the record of a read (sbwtgpu_read_hits of include/sbwtgpu.h)
struct SbwtReadHits { int n_kmers, n_found, covered_bases, longest_run; };
static_assert(sizeof(SbwtReadHits) == 16, "a read's record is four int32");

// Where the parts of a read-hits workspace lie, in bytes from its start (every part 256-byte aligned).  The search
// workspace comes first, so the search's status word is where sbwtgpu_workspace_status looks for it.
struct SbwtRhLayout {
    long long hdr;      // SbwtRhHeader
    long long res;      // search results: 8 bytes per base (int32 results use the first half)
    long long bits;     // one bit per window, 64 per word
    long long cnt;      // windows per read (n_reads entries)
    long long ooff;     // their exclusive scan (n_reads + 1)
    long long bsum;     // the scan's block sums
    long long rc;       // two strands: the reverse complement of the whole base buffer ...
    long long roff2;    // ... the mirrored read offsets ...
    long long ooff2;    // ... and the mirrored result offsets
    long long total;
};
struct SbwtRhHeader {
    int status;         // the first non-zero status word of this call's searches (SbwtWorkHeader::status)
    int pad[63];
};
static_assert(sizeof(SbwtRhHeader) == 256, "read-hits header is 256 bytes");

SbwtRhLayout sbwt_rh_layout(long long search_ws_bytes, long long total_bases, long long n_reads, int strands);

// out_off[r] = sum over q < r of max(0, len_q - k + 1), from the read offsets alone (n_reads >= 1)
void sbwt_launch_rh_offsets(const long long *d_read_off, long long n_reads, int k, long long *d_cnt, long long *d_bsum,
                            long long *d_out_off, hipStream_t stream);
// rc[T - 1 - b] = complement(bases[b]) for the T bases of the buffer, and the offsets of the mirrored batch:
// roff2[j] = T - read_off[n - j], ooff2[j] = W - out_off[n - j] (W = out_off[n])
void sbwt_launch_rh_mirror(const char *d_bases, long long total_bases, const long long *d_read_off, const long long *d_out_off,
                           long long n_reads, char *d_rc, long long *d_roff2, long long *d_ooff2, hipStream_t stream);
// bit p of d_bits = (result p >= 0) for the W = d_out_off[n_reads] results (max_results bounds W for the grid); mirrored:
// bit p |= (result W - 1 - p >= 0).  wide: the results are int64, else int32.  The search's status word is noted in hdr.
void sbwt_launch_rh_bits(const void *d_res, int wide, const long long *d_out_off, long long n_reads, long long max_results,
                         int mirrored, unsigned long long *d_bits, const SbwtWorkHeader *search_ws, SbwtRhHeader *hdr,
                         hipStream_t stream);
void sbwt_launch_rh_reduce(const unsigned long long *d_bits, const long long *d_out_off, long long n_reads, int k, int wave_min,
                           SbwtReadHits *d_out, hipStream_t stream);
