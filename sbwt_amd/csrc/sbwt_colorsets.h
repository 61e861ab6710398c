// sbwt_colorsets.h -- deduplicated colour sets (sbwt_colorsets.hip): one uint32 id per column and a table of the distinct
// rows of `words` 64-bit words, in place of the wide matrix of sbwt_colors.h.  What the C-ABI host code calls.
#pragma once
#include <hip/hip_runtime.h>
#include "sbwt_colors.h"

// what k_cs_check_table found first (lowest table row, then this order); 0 = nothing
enum { SBWT_CS_OK = 0, SBWT_CS_ROW0_NOT_ZERO = 1, SBWT_CS_ZERO_ROW = 2, SBWT_CS_HIGH_BIT = 3 };

// The canonical colour-set object of a matrix of n x words words: the distinct non-zero rows are numbered 1, 2, ... in the
// order of the smallest column that carries them, row 0 of the table is the empty set.  *d_ids (n uint32) and *d_table
// (*n_sets x words) are allocated here and belong to the caller; on an error neither is left allocated.  Scratch, freed before
// it returns: 8 bytes per column for the hash table's slots (2 n + 1 uint32), 1 for the representatives' flags, 4 for their
// scan, and rocPRIM's temporary storage (a few KiB).  Synchronises `stream`.
hipError_t sbwt_colorsets_compress(const unsigned long long *d_rows, long long n, int words, unsigned **d_ids,
                                   unsigned long long **d_table, long long *n_sets, hipStream_t stream);

// d_rows[j * words + w] = d_table[d_ids[j] * words + w]
void sbwt_launch_cs_expand(const unsigned *d_ids, const unsigned long long *d_table, long long n, int words,
                           unsigned long long *d_rows, hipStream_t stream);

// d_count[0] += the number of ids that are not 0 (the caller zeroes it first)
void sbwt_launch_cs_count(const unsigned *d_ids, long long n, unsigned long long *d_count, hipStream_t stream);

// An uploaded object checked on the device.  The ids of dummy columns (sbwt_colwalk.h levels, as sbwt_colors_clean) are set to
// 0; then h_report[0] = the smallest column whose id is >= n_sets (or ~0), h_report[1] = (table row << 8 | SBWT_CS_ kind) of
// the first violation in the table (or ~0).  Scratch of one byte per column and 16 bytes, freed before it returns;
// synchronises `stream`.
hipError_t sbwt_colorsets_validate(const SbwtIndexView &ix, unsigned *d_ids, const unsigned long long *d_table, long long n_sets,
                                   int n_colors, unsigned long long h_report[2], hipStream_t stream);

// sbwt_launch_pa_reduce_wide over ids and table: the same inputs, outputs and dynamic LDS
void sbwt_launch_pa_reduce_sets(const int *d_res, const int *d_res2, const long long *d_out_off, long long n_reads,
                                const unsigned *d_ids, const unsigned long long *d_table, long long n_nodes, long long n_sets,
                                int words, int n_colors, int threshold_ppm, int denominator, SbwtReadFound *d_out,
                                unsigned long long *d_colors, int *d_counts, hipStream_t stream);
