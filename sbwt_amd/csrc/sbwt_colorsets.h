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

// ---- the builder: colour sets made one colour at a time ----
// What a builder holds on the device: ids (n uint32, all 0 at first), a table of `cap` rows of `words` words of which n_sets
// are in use (row 0 zero), cnt (cap uint32: the columns that carry each id; cnt[0] = n at first) and the mark bitmap (one bit
// per column in 64-bit words).  The capacity starts at SBWT_CSB_FIRST_CAPACITY rows and doubles.
#define SBWT_CSB_FIRST_CAPACITY 64
struct SbwtCsbState {
    long long n = 0;
    int words = 1;
    long long cap = 0, n_sets = 1, n_colored = 0;
    unsigned *d_ids = nullptr, *d_cnt = nullptr;
    unsigned long long *d_table = nullptr, *d_marks = nullptr;
};

// allocates and zeroes the state; on an error nothing is left allocated.  Synchronises `stream`.
hipError_t sbwt_csb_init(SbwtCsbState *b, long long n, int words, hipStream_t stream);
void sbwt_csb_free(SbwtCsbState *b);
// 4 n + 8 ceil(n / 64) + cap (8 words + 4); 0 once finish has taken the state apart
long long sbwt_csb_device_bytes(const SbwtCsbState *b);

// sbwt_launch_col_mark with a bit per column in the place of a row: a hit on column j sets bit j & 63 of d_marks[j >> 6]
void sbwt_launch_csb_mark(const int *d_res, const int *d_other, const long long *d_out_off, long long n_reads, long long max_results,
                          unsigned long long *d_marks, long long n_nodes, int count, SbwtPaHeader *hdr, hipStream_t stream);

// Closes `color` (in no row of the table yet): every marked column's set becomes its old set + the colour, the bitmap is
// cleared, n_sets and n_colored follow, *n_marked = the marked columns.  Scratch, freed before it returns: 4 bytes per set and
// 32 bytes.  The table grows when the sets that split need it; an error (hipErrorOutOfMemory from there, for one) leaves the
// state unusable for anything but sbwt_csb_free.  Synchronises `stream`.
hipError_t sbwt_csb_close(SbwtCsbState *b, int color, long long *n_marked, hipStream_t stream);

// The canonical colour-set object of the state (no colour open): *d_ids is the state's id array renumbered, *d_table a new
// table of *n_sets rows; both belong to the caller and the state is freed.  Scratch: 4 bytes per set, 1 + 4 bytes per column
// and rocPRIM's temporary storage.  On an error the state keeps what it had.  Synchronises `stream`.
hipError_t sbwt_csb_finish(SbwtCsbState *b, unsigned **d_ids, unsigned long long **d_table, long long *n_sets, hipStream_t stream);
