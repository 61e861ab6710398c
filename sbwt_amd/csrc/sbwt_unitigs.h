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
};

// scratch per column while sbwt_unitigs_run works (freed before it returns): 4 (pred) + 1 (dummy level) + 1/8 (marks) +
// 2 x 16 (ranking state, double-buffered; the scans reuse one half) bytes
long long sbwt_unitigs_scratch_bytes(long long n_nodes);
// has_marks: the blocks carry suffix-group marks (given or derived); otherwise they are derived into the scratch.
// Synchronises `stream` between passes (it reads two counts and a flag per jump round back).  hipSuccess, or the error of
// the call that failed (hipErrorOutOfMemory: a result could not be allocated); on failure nothing is left allocated.
// A colour view (d_ids: n_nodes ids, d_table: rows of `words` words, both read in place) selects the coloured run of DESIGN.md
// section 18: unitigs end where the colour set changes, run->d_set_id and run->n_color_breaks are filled.  d_ids == nullptr
// is the plain run.
hipError_t sbwt_unitigs_run(const SbwtIndexView &ix, int has_marks, void *d_scratch, SbwtUnitigRun *run, hipStream_t stream,
                            const unsigned *d_ids = nullptr, const unsigned long long *d_table = nullptr, int words = 0);
