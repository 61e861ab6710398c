// sbwt_unitigs.h -- unitig extraction (sbwt_unitigs.hip): what the C-ABI host code launches.
#pragma once
#include <hip/hip_runtime.h>
#include "sbwt_device.h"

// the passes of one extraction, in the order they run (SbwtUnitigRun::ms)
enum { SBWT_UT_PASS_PRED = 0,   // predecessor array + suffix-group marks (copied from the blocks, or derived)
       SBWT_UT_PASS_REAL,       // real flags: k-1 rounds down the dummy tree
       SBWT_UT_PASS_LINK,       // internal edges: every column's initial ranking state
       SBWT_UT_PASS_RANK,       // pointer jumping
       SBWT_UT_PASS_OFFSETS,    // start flags -> unitig ids, lengths -> 64-bit base offsets
       SBWT_UT_PASS_BASES,      // every column's last character + every start's label
       SBWT_UT_N_PASSES };
// what a run adds to the unitigs when asked; the values are those of SBWTGPU_UNITIGS_* in the ABI
enum { SBWT_UT_GRAPH_LINKS = 1u,        // pass 7: the links between the unitigs, CSR
       SBWT_UT_GRAPH_COLUMN_MAP = 2u }; // pass 8: (unitig, offset) of every column

struct SbwtUnitigRun {
    // results: device allocations of their own, owned by the caller of sbwt_unitigs_run on success
    char *d_bases = nullptr;                // total_bases bytes
    long long *d_off = nullptr;             // n_unitigs + 1
    long long *d_first_col = nullptr;       // n_unitigs
    unsigned *d_set_id = nullptr;           // n_unitigs: ids[first column], a coloured run only
    long long n_color_breaks = 0;           // single edges between two sets (a coloured run only)
    long long n_unitigs = 0, total_bases = 0;
    int jump_rounds = 0;                    // launches of the pointer-jumping kernel
    float ms[SBWT_UT_N_PASSES] = {0, 0, 0, 0, 0, 0};
    // the graph (section 21), filled as far as the run was asked to; device allocations like the results above
    long long *d_link_off = nullptr;        // n_unitigs + 1
    unsigned *d_link_to = nullptr;          // n_links
    long long n_links = 0;
    unsigned *d_col_unitig = nullptr;       // n_nodes: 0xFFFFFFFF for a dummy column
    unsigned *d_col_offset = nullptr;       // n_nodes
    float links_ms = 0, map_ms = 0;
};

// scratch per column while sbwt_unitigs_run works (freed before it returns): 4 (pred) + 1 (dummy level) + 1/8 (marks) +
// 2 x 16 (ranking state, double-buffered; the scans reuse one half) bytes
long long sbwt_unitigs_scratch_bytes(long long n_nodes);
// has_marks: the blocks carry suffix-group marks (given or derived); otherwise they are derived into the scratch.
// Synchronises `stream` between passes (it reads two counts and a flag per jump round back).  hipSuccess, or the error of
// the call that failed (hipErrorOutOfMemory: a result could not be allocated); on failure nothing is left allocated.
// A colour view (d_ids: n_nodes ids, d_table: rows of `words` words, both read in place) selects the coloured run of DESIGN.md
// section 18: unitigs end where the colour set changes, run->d_set_id and run->n_color_breaks are filled.  d_ids == nullptr
// is the plain run.  `graph`: SBWT_UT_GRAPH_* bits; 0 runs passes 1 to 6 and nothing else.
hipError_t sbwt_unitigs_run(const SbwtIndexView &ix, int has_marks, void *d_scratch, SbwtUnitigRun *run, hipStream_t stream,
                            const unsigned *d_ids = nullptr, const unsigned long long *d_table = nullptr, int words = 0,
                            unsigned graph = 0);
// (unitig, offset) of the columns cols[0 .. n) from a column map: a gather on `stream`, which it never synchronises.  A value
// outside [0, n_nodes) gives 0xFFFFFFFF in both, as a dummy column does.
hipError_t sbwt_unitigs_locate(const unsigned *d_col_unitig, const unsigned *d_col_offset, long long n_nodes, const long long *d_cols,
                               long long n, unsigned *d_unitig, unsigned *d_offset, hipStream_t stream);
