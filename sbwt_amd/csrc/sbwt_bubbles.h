// sbwt_bubbles.h -- bubbles of the plain unitig graph and the colours of their branches (sbwt_bubbles.hip, DESIGN.md
// section 24; include/sbwtgpu.h, "bubbles").  What the C-ABI host code launches.
#pragma once
#include <hip/hip_runtime.h>

// the record of the ABI (sbwtgpu_bubble)
struct SbwtBubble {
    unsigned source, branch[2], sink, n_kmers[2], kind, reserved;
};
static_assert(sizeof(SbwtBubble) == 32, "a bubble record is eight words");

// the passes of one run, in the order they run (SbwtBubbleRun::ms)
enum { SBWT_BB_PASS_INDEG = 0,   // in-degrees: atomics over link_to
       SBWT_BB_PASS_DETECT,      // one lane per source applies the definition
       SBWT_BB_PASS_COMPACT,     // scan of the flags, records and slot table
       SBWT_BB_PASS_COLORS,      // AND / OR of the colour rows of the branch columns (0 without an object)
       SBWT_BB_N_PASSES };

// what a run works on: the links and lengths of a plain graph handle and, for the colours, its column map and a colour view
struct SbwtBubbleGraph {
    const long long *d_link_off = nullptr;      // n_unitigs + 1
    const unsigned *d_link_to = nullptr;        // n_links
    const long long *d_off = nullptr;           // n_unitigs + 1: base offsets of the spellings
    long long n_unitigs = 0, n_links = 0, k = 0;
    const unsigned *d_col_unitig = nullptr;     // n_nodes, with colours only
    long long n_nodes = 0;
    const unsigned *d_ids = nullptr;            // n_nodes; nullptr: no colours
    const unsigned long long *d_table = nullptr;
    int words = 0, n_colors = 0;
};

struct SbwtBubbleRun {
    // results: device allocations of their own, owned by the caller of sbwt_bubbles_run on success (nullptr when empty)
    SbwtBubble *d_rec = nullptr;                // n_bubbles
    unsigned long long *d_inter = nullptr;      // 2 n_bubbles x words, with colours only
    unsigned long long *d_uni = nullptr;
    long long n_bubbles = 0, n_snps = 0;
    float ms[SBWT_BB_N_PASSES] = {0, 0, 0, 0};
};

// scratch while sbwt_bubbles_run works (allocated and freed by it): 4 (in-degree) + 4 (slot) bytes per unitig, and for the
// scan 16 per unitig (flag and prefix, int64) and 8 per 1024 unitigs
long long sbwt_bubbles_scratch_bytes(long long n_unitigs);
// Synchronises `stream` twice (it reads the number of bubbles back before it allocates the results, and the number of SNPs
// at the end).  hipSuccess, or the error of the call that failed (hipErrorOutOfMemory: scratch or a result could not be
// allocated); on failure nothing is left allocated.
hipError_t sbwt_bubbles_run(const SbwtBubbleGraph &g, SbwtBubbleRun *run, hipStream_t stream);
// pass 1 alone: d_indeg[j] = the entries of link_to equal to j (n_unitigs uint32, zeroed here first); asynchronous on `stream`
hipError_t sbwt_bubbles_in_degrees(const unsigned *d_link_to, long long n_links, long long n_unitigs, unsigned *d_indeg,
                                   hipStream_t stream);
