// sbwt_genotype.h -- genotyping a read set at the bubbles: per-allele k-mer depth and calls (sbwt_genotype.hip, DESIGN.md
// section 25; include/sbwtgpu.h, "genotype").  What the C-ABI host code launches.
#pragma once
#include <hip/hip_runtime.h>

#include "sbwt_bubbles.h"

// The counters of a genotype object, on the device: every add adds to them with atomics, nothing else writes them.
struct SbwtGenotypeCounters {
    unsigned long long n_windows;       // the sample's size, misses counted (two strands: twice the windows)
    unsigned long long n_hits;          // results >= 0
    unsigned long long n_site_hits;     // of them, on branch columns
    unsigned long long pad[5];
};
static_assert(sizeof(SbwtGenotypeCounters) == 64, "the genotype counters are eight words");

// what a build works on: the bubble records (and their inter rows) and the plain graph handle's lengths and column map
struct SbwtGenotypeGraph {
    const SbwtBubble *d_rec = nullptr;          // n_bubbles
    const unsigned long long *d_inter = nullptr;// 2 n_bubbles x words; nullptr: no colours
    long long n_bubbles = 0;
    int words = 0;
    const long long *d_off = nullptr;           // n_unitigs + 1: base offsets of the spellings
    long long n_unitigs = 0, k = 0;
    const unsigned *d_col_unitig = nullptr, *d_col_offset = nullptr;    // n_nodes each
    long long n_nodes = 0;
};

// Device state of one object.  d_acc is one allocation, [counters, 256 bytes][kmer_hits, P uint64]: what an add writes and
// a reset zeroes.  The rest is written by the build and only read afterwards.
struct SbwtGenotypeState {
    char *d_acc = nullptr;
    size_t acc_bytes = 0;
    long long *d_branch_off = nullptr;          // 2 B + 1: the exclusive prefix sum of n_kmers in slot order
    unsigned long long *d_bitmap = nullptr;     // ceil(n_nodes / 64) words: bit v = column v is a branch column
    unsigned *d_dir = nullptr;                  // per word of the bitmap: the branch columns before it
    unsigned *d_pos = nullptr;                  // per branch column, in column order: its position p
    unsigned long long *d_inter = nullptr;      // the object's copy of the inter rows (nullptr without colours)
    long long n_bubbles = 0, n_positions = 0, n_nodes = 0;
    SbwtGenotypeCounters *ctr() const { return reinterpret_cast<SbwtGenotypeCounters *>(d_acc); }
    unsigned long long *kmer_hits() const { return reinterpret_cast<unsigned long long *>(d_acc + 256); }
};

// why a build refused its records (SbwtGenotypeState stays empty)
enum { SBWT_GT_BAD_UNITIG = 1,      // a record names a unitig >= n_unitigs, or n_kmers is not that unitig's k-mer count
       SBWT_GT_BAD_SHARED = 2,      // a unitig is the branch of two slots
       SBWT_GT_BAD_COLUMNS = 4 };   // the branch columns of the map are not the positions of the records

// Builds the tables of an object: slot table with the consistency check, branch bitmap, rank directory, positions; copies
// the inter rows; zeroes the accumulator.  Synchronises `stream` (it reads P and the error word back before it allocates
// what P sizes).  Scratch, freed before it returns: 4 bytes per unitig, 16 per slot, 16 per 64 columns.  hipSuccess with
// *bad = 0: the state is the caller's to free (sbwt_genotype_free).  hipSuccess with *bad != 0 or an error: nothing is
// left allocated.
hipError_t sbwt_genotype_build(const SbwtGenotypeGraph &g, SbwtGenotypeState *out, int *bad, hipStream_t stream);
void sbwt_genotype_free(SbwtGenotypeState *s);

// One launch per add.  d_res: the W = d_out_off[n_reads] int32 results of the batch, d_res2 (may be NULL): the W results of
// the mirrored batch (max_results bounds W for the grid).  Every result v with 0 <= v < n_nodes is a hit; a hit on a branch
// column adds 1 to kmer_hits at that column's position.  The counters grow by the windows, the hits and the branch hits.
void sbwt_launch_genotype_add(const int *d_res, const int *d_res2, const long long *d_out_off, long long n_reads, long long max_results,
                              const SbwtGenotypeState &s, hipStream_t stream);

// seen, hits, min_hits: 2 B int64 each, one segmented reduce over kmer_hits
void sbwt_launch_genotype_branches(const SbwtGenotypeState &s, long long *d_seen, long long *d_hits, long long *d_min, hipStream_t stream);

// d_call (B bytes, may be NULL) from d_seen / d_hits and the two parameters; with d_ref (3 n_colors int64: sites, match,
// only; zeroed here first; needs the inter rows) the three per-colour vectors
void sbwt_launch_genotype_calls(const SbwtGenotypeState &s, const long long *d_seen, const long long *d_hits, int breadth_ppm,
                                long long min_depth, int words, int n_colors, unsigned char *d_call, unsigned long long *d_ref,
                                hipStream_t stream);
