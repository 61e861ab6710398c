// sbwt_occurrences.h -- every reference occurrence of every column's k-mer, and reads mapped by voting over all of them
// (sbwt_occurrences.hip; include/sbwtgpu.h, "occurrences").  What the C-ABI host code launches.
#pragma once
#include <hip/hip_runtime.h>
#include "sbwt_positions.h"

#define SBWT_OM_TABLE 256       // distinct placements a wave keeps in LDS per read (the compiled T)
#define SBWT_OM_PENDING 8       // pending (key, count) runs in registers: lane j's, for occurrence rank j < 8 (at most 64)
#define SBWT_OM_MAX_SLICES 1024 // the second kernel doubles its slices up to here; beyond, the third counts key by key without a table

// The counters of a builder and of an object, on the device.
struct SbwtOccCounters {
    unsigned long long n_windows;       // windows offered, once per strand searched
    unsigned long long n_hits;          // results >= 0
    unsigned long long log_len;         // builder: entries in the log
    unsigned long long n_unique;        // finish: distinct (column, key) pairs
    unsigned long long n_positioned;    // columns with an occurrence
    unsigned long long max_count;       // the largest count of a column
    unsigned long long bad_column;      // upload: the first offending column (~0: none)
    unsigned long long bad_kind;        // upload: what is wrong with it (SBWT_OCC_BAD_*)
};
static_assert(sizeof(SbwtOccCounters) == 64, "the occurrence counters are eight words");
enum { SBWT_OCC_BAD_OFF0 = 1, SBWT_OCC_BAD_MONOTONE = 2, SBWT_OCC_BAD_TOTAL = 3, SBWT_OCC_BAD_ORDER = 4, SBWT_OCC_BAD_SEQ = 5 };

// One launch per add: d_res, d_res2, d_out_off, max_results and first_seq as for sbwt_launch_pos_add.  Every result v with
// 0 <= v < n_nodes appends (v, key) to the log: log_col[e], log_key[e] with e handed out by one atomic per wave on
// ctr->log_len (ballot, prefix popcount).  The caller guarantees room for log_len + W (2 W with d_res2) entries; log_cap is
// that room, and an entry beyond it (never) is dropped and sets ctr->bad_kind.
void sbwt_launch_occ_add(const int *d_res, const int *d_res2, const long long *d_out_off, long long n_reads, long long max_results,
                         long long first_seq, long long n_nodes, unsigned *d_log_col, unsigned long long *d_log_key,
                         unsigned long long log_cap, SbwtOccCounters *ctr, unsigned long long *d_n_hit_windows, hipStream_t stream);

// The log of n entries sorted by (column, key): two stable radix sorts through (d_alt_col, d_alt_key), the result back in
// (d_log_col, d_log_key).  key_bits / col_bits: the bits in use.  tmp: sbwt_occ_sort_tmp_bytes(n).
size_t sbwt_occ_sort_tmp_bytes(long long n);
hipError_t sbwt_occ_sort(unsigned *d_log_col, unsigned long long *d_log_key, unsigned *d_alt_col, unsigned long long *d_alt_key,
                         long long n, int key_bits, int col_bits, void *tmp, size_t tmp_bytes, hipStream_t stream);
// d_flag[i] = 1 where entry i of the sorted log differs from entry i - 1; d_off[v] += 1 per flagged entry of column v (d_off:
// n_nodes + 1 words, zeroed here first); ctr->n_unique = the flags set.
void sbwt_launch_occ_flag(const unsigned *d_col, const unsigned long long *d_key, long long n, unsigned char *d_flag,
                          unsigned long long *d_off, long long n_nodes, SbwtOccCounters *ctr, hipStream_t stream);
// d_off (counts per column, a zero behind them) -> the exclusive scan in place.  tmp: sbwt_occ_scan_tmp_bytes(n_nodes).
size_t sbwt_occ_scan_tmp_bytes(long long n_nodes);
hipError_t sbwt_occ_scan(unsigned long long *d_off, long long n_nodes, void *tmp, size_t tmp_bytes, hipStream_t stream);
// the flagged keys, in order, to d_occ (room for n_unique).  tmp: sbwt_occ_select_tmp_bytes(n); d_count: one word of scratch.
size_t sbwt_occ_select_tmp_bytes(long long n);
hipError_t sbwt_occ_select(const unsigned long long *d_key, const unsigned char *d_flag, long long n, unsigned long long *d_occ,
                           unsigned long long *d_count, void *tmp, size_t tmp_bytes, hipStream_t stream);
// ctr->n_positioned, ctr->max_count from d_off (both zeroed here first)
void sbwt_launch_occ_stats(const unsigned long long *d_off, long long n_nodes, SbwtOccCounters *ctr, hipStream_t stream);
// upload's checks.  _check_off: off[0] = 0, off non-decreasing, off[n] = n_occ; _check_keys (only after the first passed, it
// reads occ through off): keys strictly ascending within a column, seq < 2^30.  ctr->bad_column: the smallest offending column.
void sbwt_launch_occ_check_off(const unsigned long long *d_off, long long n_nodes, unsigned long long n_occ, SbwtOccCounters *ctr,
                               hipStream_t stream);
void sbwt_launch_occ_check_keys(const unsigned long long *d_off, const unsigned long long *d_occ, long long n_nodes, SbwtOccCounters *ctr,
                                hipStream_t stream);
// d_first[v] = occ[off[v]], SBWT_POS_NONE for an empty column
void sbwt_launch_occ_first(const unsigned long long *d_off, const unsigned long long *d_occ, long long n_nodes, unsigned long long *d_first,
                           hipStream_t stream);

// One record per read from the int32 results, (d_off, d_occ) and d_out_off; d_res2 (may be NULL) as above.  Three launches:
// one wave per read with a table of `cap` (1 .. SBWT_OM_TABLE) placements in LDS, which appends the reads that outgrow it to
// d_slow; a grid-stride kernel over that list which recomputes them exactly in slices of the key space and marks the entries
// that no slicing up to SBWT_OM_MAX_SLICES fits; and a grid-stride kernel over the marked entries that needs no table.  hdr is
// zeroed here first.
void sbwt_launch_occ_map(const int *d_res, const int *d_res2, const long long *d_out_off, long long n_reads,
                         const unsigned long long *d_off, const unsigned long long *d_occ, long long n_nodes, int max_occ, int cap,
                         SbwtReadMap *d_out, SbwtPosMapHeader *hdr, unsigned *d_slow, hipStream_t stream);
