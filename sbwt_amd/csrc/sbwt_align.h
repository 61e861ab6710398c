// sbwt_align.h -- the alignment of mapped reads: from a verify record (edit, ref_end) to the begin of the best alignment and
// its runs of = X I D (sbwt_align.hip; include/sbwtgpu.h, "alignment of mapped reads").  What the C-ABI
// host code launches.
#pragma once
#include <hip/hip_runtime.h>

#include "sbwt_verify.h"

#define SBWT_AL_FAST_EDIT 31        // the largest edit the first kernel takes: a band of 2 * 31 + 1 = 63 diagonals, one mask word
#define SBWT_AL_FAST_ROWS 256       // the longest read the first kernel takes: the rows of one wave's scratch
#define SBWT_AL_FAST_GRID 1024      // waves of the first kernel (a fixed grid: the scratch does not grow with the batch)
#define SBWT_AL_SLOW_GRID 64        // waves of the second kernel
#define SBWT_AL_SLOW_COLS 24        // window columns per lane in the second kernel: 64 * 24 = 1536 = 1024 + 2 * 256

// the record the kernels write (sbwtgpu_read_align)
struct SbwtReadAlign { long long ref_begin; int n_ops, n_eq; };
static_assert(sizeof(SbwtReadAlign) == 16, "the record of the ABI");

// the head of the align calls' own workspace: the length of the list of reads left to the second kernel
struct SbwtAlignHeader { unsigned n_slow; unsigned pad[63]; };
static_assert(sizeof(SbwtAlignHeader) == 256, "the align header is 256 bytes");

// one wave's scratch in either kernel: [row][lane] mask words
#define SBWT_AL_FAST_SLAB ((long long)SBWT_AL_FAST_ROWS * 64 * 16)
#define SBWT_AL_SLOW_SLAB ((long long)SBWT_VF_MAX_READ * 64 * 8)

// What the align kernels need behind the verify workspace, laid out by sbwt_align_layout: the header, the list (4 bytes per
// read), the run counts and the scan's block sums (8 bytes each), then the waves' scratch.
struct SbwtAlignLayout { long long o_hdr, o_slow, o_cnt, o_bsum, o_fast, o_slab, bytes; int fast_waves, slow_waves; };
static inline SbwtAlignLayout sbwt_align_layout(long long n_reads) {
    if (n_reads < 0) n_reads = 0;
    auto up = [](long long x) { return (x + 255) & ~255ll; };
    SbwtAlignLayout a;
    const long long groups = (n_reads + 63) / 64;
    a.fast_waves = (int)(groups < SBWT_AL_FAST_GRID ? groups : SBWT_AL_FAST_GRID);
    a.slow_waves = (int)(n_reads < SBWT_AL_SLOW_GRID ? n_reads : SBWT_AL_SLOW_GRID);
    a.o_hdr = 0;
    a.o_slow = a.o_hdr + (long long)sizeof(SbwtAlignHeader);
    a.o_cnt = a.o_slow + up(n_reads * 4);
    a.o_bsum = a.o_cnt + up(n_reads * 8);
    a.o_fast = a.o_bsum + up((n_reads / 1024 + 2) * 8);
    a.o_slab = a.o_fast + a.fast_waves * SBWT_AL_FAST_SLAB;
    a.bytes = a.o_slab + a.slow_waves * SBWT_AL_SLOW_SLAB;
    return a;
}

// From the verify records d_verify (as sbwt_launch_verify wrote them for the same reads, map records and band): d_out, the run
// offsets d_op_off[0 .. n_reads] and the runs below ops_cap.  Two passes of the same two kernels around a device scan: the first
// counts every read's runs, the second stores them.  fast_edit: 1 .. SBWT_AL_FAST_EDIT.  ws: sbwt_align_layout(n_reads).bytes.
void sbwt_launch_align(const char *d_bases, long long total_bases, const long long *d_read_off, long long n_reads,
                       const SbwtVerifyMap *d_map, const SbwtRefSeq *tab, const unsigned long long *d_bits,
                       const unsigned long long *d_valid, int band, int fast_edit, const SbwtReadVerify *d_verify, SbwtReadAlign *d_out,
                       long long *d_op_off, unsigned *d_ops, long long ops_cap, char *ws, hipStream_t stream);
