// sbwt_pileup.h -- the pileup of aligned reads on the reference sequences: per-base counters that live on the device across
// batches, and their read-out as records and calls (sbwt_pileup.hip; include/sbwtgpu.h, "pileup of aligned
// reads").  What the C-ABI host code launches.
#pragma once
#include <hip/hip_runtime.h>

#include "sbwt_align.h"

// One cell per coordinate of the reference object's layout (sequence s starts at cell 64 * slot), and one cell beyond the last
// slot.  diff is the difference array of the depth: +1 where a piled read begins, -1 where it ends; the depth of a cell is the
// prefix sum of diff over ALL cells up to it.  x[c] counts the X columns whose read base has code c; the = columns have no
// counter.
struct SbwtPileCell { int diff; unsigned x[4]; unsigned del, ins, other; };
static_assert(sizeof(SbwtPileCell) == 32, "a cell is 32 bytes");

// the records of the ABI (sbwtgpu_pileup_base, sbwtgpu_pileup_call, sbwtgpu_pileup_filter)
struct SbwtPileBase { unsigned depth, n[4], n_del, n_ins, n_other; };
struct SbwtPileCall { long long pos; int seq, allele, ref, depth, count, ref_count; };
struct SbwtPileFilter { int min_votes, require_unique, max_edit, reserved; };
static_assert(sizeof(SbwtPileBase) == 32 && sizeof(SbwtPileCall) == 32 && sizeof(SbwtPileFilter) == 16, "the records of the ABI");

// the scalars of a pileup, on the device.  n_columns is the sum of the depth over all bases: every piled read adds the length
// of its clamped interval.
struct SbwtPileCounters { unsigned long long n_offered, n_piled, n_columns, n_clipped, n_overhang; unsigned long long pad[27]; };
static_assert(sizeof(SbwtPileCounters) == 256, "the pileup counters are 256 bytes");

#define SBWT_PILE_BLOCK 1024        // cells per block of the read-out kernels, and per entry of the depth's block sums

// the 8-byte entries of the read-outs' scratch for n_cells cells: the block sums of diff, scanned in place
static inline long long sbwt_pile_blocks(long long n_cells) { return (n_cells + SBWT_PILE_BLOCK - 1) / SBWT_PILE_BLOCK; }

// The accumulate pass: one lane per read.  A read is piled iff its align record has runs, its seq is below n_seqs and the filter
// passes; its runs d_ops[d_op_off[i] .. + n_ops) are walked from ref_begin.  Only atomic adds touch cells and ctr.
void sbwt_launch_pile_add(const char *d_bases, long long total_bases, const long long *d_read_off, long long n_reads,
                          const SbwtVerifyMap *d_map, const SbwtReadVerify *d_verify, const SbwtReadAlign *d_align,
                          const long long *d_op_off, const unsigned *d_ops, SbwtPileFilter f, const SbwtRefSeq *tab, long long n_seqs,
                          SbwtPileCell *cells, long long n_cells, SbwtPileCounters *ctr, hipStream_t stream);

// d_bsum[b] = the sum of diff over the cells before block b (d_bsum: sbwt_pile_blocks(n_cells) + 1 entries).  Reads the cells only.
void sbwt_launch_pile_scan(const SbwtPileCell *cells, long long n_cells, long long *d_bsum, hipStream_t stream);

// d_out[0 .. len) = the records of coordinates pos .. pos + len of the sequence at `slot` (after sbwt_launch_pile_scan)
void sbwt_launch_pile_counts(const SbwtPileCell *cells, long long n_cells, const long long *d_bsum, const unsigned long long *d_bits,
                             const unsigned long long *d_valid, long long slot, long long pos, long long len, SbwtPileBase *d_out,
                             hipStream_t stream);

// The calls of every block of cells (after sbwt_launch_pile_scan).  d_out == nullptr: d_cnt[b] = the calls of block b.  Otherwise
// d_off[b] is where block b's calls go in d_out, ascending in (seq, pos, allele) within the block as the blocks are among each
// other.
void sbwt_launch_pile_calls(const SbwtPileCell *cells, long long n_cells, const long long *d_bsum, const unsigned long long *d_bits,
                            const unsigned long long *d_valid, const SbwtRefSeq *tab, long long n_seqs, int min_depth, int min_alt,
                            int min_frac_ppm, long long *d_cnt, const long long *d_off, SbwtPileCall *d_out, hipStream_t stream);

// exclusive scan of n int64 values, d_out[n] = the total (sbwt_scan.h); d_bsum: n / 1024 + 2 entries
void sbwt_launch_pile_scan_i64(const long long *d_in, long long n, long long *d_bsum, long long *d_out, hipStream_t stream);
