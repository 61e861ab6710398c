// sbwt_colormatrix.h -- pairwise shared k-mer counts between colours: the weighted Gram matrix of a colour-set table
// (sbwt_colormatrix.hip; include/sbwtgpu.h, "shared k-mers").  What the C-ABI host code calls.
#pragma once
#include <hip/hip_runtime.h>

// The workspace begins with this header of eight 64-bit words.  status is the smallest set (other than 0) whose caller-supplied
// weight is negative or above 2^31 - 1, or ~0 when there is none; n_used the sets that count (weight > 0, set 0 left out);
// max_w the largest weight among them; n_limb[l] the sets whose weight is at least 128^l (the matrix-core route only).
struct SbwtGmHeader {
    unsigned long long status, n_used, max_w, n_limb[5];
};

#define SBWT_GM_MIN_SETS_DEFAULT 512        // fewer sets than this: the plain kernel ("gram_mfma_min_sets")
#define SBWT_GM_FLUSH_DEFAULT 65536         // sets a wave adds up in 32 bits before it adds the tile into the 64-bit matrix
#define SBWT_GM_FLUSH_MAX 16909320ll        // the largest interval: 127 * 16909320 = 2^31 - 8
static_assert(127ll * SBWT_GM_FLUSH_DEFAULT < (1ll << 31), "a wave's 32-bit sums of limbs of at most 127 must not overflow");
static_assert(127ll * SBWT_GM_FLUSH_MAX < (1ll << 31) && 127ll * (SBWT_GM_FLUSH_MAX + 1) >= (1ll << 31), "the refusal bound is exact");

// d_sizes[t] = the columns whose id is t, for t < n_sets (n_sets uint32, zeroed here first).  No scratch.
void sbwt_launch_gm_sizes(const unsigned *d_ids, long long n, long long n_sets, unsigned *d_sizes, hipStream_t stream);

// Scratch of one call, both routes (the plain kernel needs only the header and 4 bytes per set): with S = n_sets rounded up to
// 64 and P = n_colors rounded up to 64, 256 bytes + 16 S (weights, numbers, sorted weights, permutation: 4 bytes each) + 5 S
// (limbs) + S P / 8 (bit planes) + 8 P^2 (the padded 64-bit matrix) + rocPRIM's sort storage; -1 when that cannot be asked.
long long sbwt_gm_workspace_bytes(long long n_sets, int n_colors);
long long sbwt_gm_plain_workspace_bytes(long long n_sets);      // what a call on the plain route touches of it

// G[a][b] = the sum of w[t] over the sets t >= 1 whose table row holds colours a and b, into d_matrix (n_colors x n_colors
// int64, every entry written).  d_weights == nullptr: w = the sizes (sbwt_launch_gm_sizes).  Nothing here synchronises
// unless pass_ms is given (sizes, transpose and compaction, product, mirror: the host clock around a synchronisation each).
// use_mfma picks the route, flush_sets (1 .. SBWT_GM_FLUSH_MAX) the matrix-core route's flush interval; the result depends
// on neither.  The header at the start of d_ws says afterwards what the weights were like.
hipError_t sbwt_gm_enqueue(const unsigned *d_ids, long long n, const unsigned long long *d_table, long long n_sets, int n_colors,
                           const long long *d_weights, long long *d_matrix, void *d_ws, long long ws_bytes, bool use_mfma,
                           long long flush_sets, double *pass_ms, hipStream_t stream);
