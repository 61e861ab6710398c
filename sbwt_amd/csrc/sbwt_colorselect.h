// sbwt_colorselect.h -- k-mers selected by a predicate over their colour sets (sbwt_colorselect.hip, DESIGN.md section 20;
// include/sbwtgpu.h, "colour select").  What the C-ABI host code calls.
#pragma once
#include <hip/hip_runtime.h>

// d_verdict[t] = 1 when row t of the table matches, else 0, for t < n_sets:
//     (row & exclude) == 0  and  min_in <= popcount(row & include) <= max_in.
// d_masks holds 2 x words words: include, then exclude.  No scratch, nothing synchronises.
void sbwt_launch_csel_verdict(const unsigned long long *d_table, long long n_sets, int words, const unsigned long long *d_masks,
                              int min_in, int max_in, unsigned char *d_verdict, hipStream_t stream);

struct SbwtCselCounts {
    long long n_real = 0, n_selected = 0, n_sets_matched = 0;
};
// The keys of an index (sbwt_setops_keys with their columns: n_keys of key_bytes = 8 or 16, ascending) under the predicate:
// key i is selected when d_verdict-of-the-predicate[d_ids[d_cols[i]]] is 1.  counts: n_real = n_keys, n_selected, and
// n_sets_matched = the distinct rows (by content, not by number) that match and that a real column carries.  With d_out the
// selected keys in their order, a device allocation of the caller's (never null on success); d_out == nullptr: counts only.
// Scratch, freed before it returns: 6 bytes per set (verdict, size, keep flag), one byte per key with d_out, rocPRIM's
// temporary storage, and -- only when more than one non-empty row matched -- 4 + 8 words bytes per such row and what
// sbwt_colorsets_compress needs for that many rows.  Synchronises `stream`.  On failure nothing is left allocated;
// hipErrorUnknown says that the ids and the keys disagree about the number of selected columns (a broken object).
hipError_t sbwt_colorselect(const unsigned *d_ids, long long n_nodes, const unsigned long long *d_table, long long n_sets, int words,
                            const unsigned long long *d_masks, int min_in, int max_in, const void *d_keys, const unsigned *d_cols,
                            long long n_keys, int key_bytes, void **d_out, SbwtCselCounts *counts, hipStream_t stream);
