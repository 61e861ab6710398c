// sbwtgpu_capi.cpp -- implementation of the C ABI declared in include/sbwtgpu.h.
// Host-side glue only: builds the device image of an index, owns device memory, and enqueues
// the kernels of sbwt_search.hip and its siblings.  There is deliberately no CPU query path in this library:
// every query entry point runs on the GPU or fails with an error code.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <cstdarg>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <cstddef>
#include <cstring>
#include <new>
#include <vector>
#include <thread>

#include "../../include/sbwtgpu.h"
#include "sbwt_device.h"
#include "sbwt_ms.h"
#include "sbwt_unitigs.h"
#include "sbwt_setops.h"
#include "sbwt_readhits.h"
#include "sbwt_walks.h"
#include "sbwt_colors.h"
#include "sbwt_colorsets.h"
#include "sbwt_colormerge.h"
#include "sbwt_colormatrix.h"
#include "sbwt_colorselect.h"
#include "sbwt_screen.h"
#include "sbwt_bubbles.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// a search's device status word (SbwtWorkHeader::status) as the call's result: a k-mer search that did not end on one column,
// or the sorted fused kernel's stall detector (a workgroup that made no progress for 2^20 waits)
static int fail_status(int status) {
    if (status == SBWTGPU_ERR_STALLED)
        return fail(SBWTGPU_ERR_STALLED, "Bug: the sorted fused search kernel stalled (no progress in a workgroup)");
    return fail(SBWTGPU_ERR_NOT_SINGLETON, "Bug: k-mer search did not give a singleton interval");
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(e_ == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP,         \
                        "%s failed: %s", #expr, hipGetErrorString(e_));                        \
    } while (0)

// Depth of the device-side prefix table: deep enough that most walks start with a nearly unique
// interval (ceil(log4(n_nodes)) + 2), capped at 14 (4 GiB of the 288 GB of HBM) unless
// SBWTGPU_DEVICE_PRECALC asks otherwise.  Measured on MI355X: 12.8 M columns (tools/ab_bench.py)
// 8: 33, 10: 45, 11: 47, 12: 49 G k-mers/s; 142 M columns (bench.py --config 3) 11: 30.2, 12: 32.2,
// 13: 34.1, 14: 36.1 G k-mers/s.
// Depth of the dense device prefix table.  Without the derived structures it is the only accelerator of the
// walks: two levels past log4(n), where most entries are empty and end a probe at once.  With the sparse table
// and the probe filter it only backs exact fall-back walks, and log4(n) does (measured: 12 and 14 give the
// same 7.08 ms on config 2, and 4 GB less image).
int default_device_precalc(int64_t n_nodes, bool derived) {
    const char *e = getenv("SBWTGPU_DEVICE_PRECALC");
    int v;
    if (e) {
        v = atoi(e);
    } else {
        v = 1;
        while (v < 14 && ((int64_t)1 << (2 * v)) < n_nodes) v++;
        if (!derived) v = v + 2 > 14 ? 14 : v + 2;
        // An image with the sparse table and the filter hardly ever walks from the dense table (0.00 dense lookups per read on
        // configs 2, 3 and 5: whole k-mers and probe windows have their own structures), so a table of 4^8 entries serves the
        // rare window that fits neither -- not one entry per column: 21 B per column on config 2, 30 on config 3 (round 5)
        else if (v > 8) v = 8;
    }
    if (v < 0) v = 0;
    if (v > 14) v = 14;
    return v;
}

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
};
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

template <typename T>
inline T align256(T x) { return (x + 255) & ~(T)255; }

// a knob's initial value: the environment variable when it is set, else the default
int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}
int64_t env_i64(const char *name, int64_t dflt) {
    const char *e = getenv(name);
    return e ? (int64_t)atoll(e) : dflt;
}

}  // namespace

// tuning knobs (A/B experiments; defaults are the shipped configuration)
// 0 = k_search (reference order), 1 = k_search_cert on the blocks, 4 = k_search_cert along the path order (two passes: encode +
// search; 2 and 3, kernels of earlier rounds, mean 4 now), 5 = the fused route (k_search_fused + the general kernel behind it)
static int tuning_variant() {
    static int v = env_int("SBWTGPU_SEARCH_VARIANT", -1);
    return v;
}
static int g_variant_override = -1, g_probe_override = -1, g_debug = 0, g_derive_ssup = 1, g_kernel_events = 0;
static int g_fused_table = 1;      // the fused route's ticket table for batches with many long reads ("fused_table")
// the fused kernel with its lanes sorted by state ("fused_sort": 0 off, 1 on; env SBWTGPU_FUSED_SORT; sbwt_search_fused.hip)
static int g_fused_sort = env_int("SBWTGPU_FUSED_SORT", SBWT_FUSED_SORT_DEFAULT);
// set around a search call by the *_i32 entry points: the kernels of this call write int32 results (SbwtIndexView::out32)
static thread_local int t_out32 = 0;
static int64_t g_ev_count = 0;
// debug aid for the parity tests: fill the result range with a poison pattern before every search and every
// matching-statistics call, so that a result the kernel never writes cannot inherit a correct value from an earlier launch
static int g_poison = env_int("SBWTGPU_POISON_RESULTS", 0);
static int g_probe_filter = env_int("SBWTGPU_PROBE_FILTER", 1);
static int g_image_level = env_int("SBWTGPU_IMAGE_LEVEL", 0);
static int64_t g_max_image_bytes = env_i64("SBWTGPU_MAX_IMAGE_BYTES", 0);
static int g_sort_reads = env_int("SBWTGPU_SORT_READS", -1);   // -1 auto, 0 off, 1 on
static int g_force_mega = 0;    // tests: store every image's block counts relative to mega[c][0] (the dense rank-only layout)
static int g_path_safe = env_int("SBWTGPU_PATH_SAFE", 2);   // 0 off, 1 narrow rule, 2 wide
static int g_path_lookahead = env_int("SBWTGPU_PATH_LOOKAHEAD", 8);   // 0: the blind rule
static int g_path_order = env_int("SBWTGPU_PATH_ORDER", 1);
// SBWTGPU_VERBOSE=1: index_create says on stderr which part of the image it is building and how long each took (a build of
// 10^9 columns takes 10-30 s; a stall names its phase)
static int g_verbose = env_int("SBWTGPU_VERBOSE", 0);
struct PhaseLog {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void operator()(const char *what) {
        if (!g_verbose) return;
        (void)hipDeviceSynchronize();
        const auto t1 = std::chrono::steady_clock::now();
        size_t fr = 0, tot = 0;
        (void)hipMemGetInfo(&fr, &tot);
        fprintf(stderr, "sbwtgpu: index_create: %-34s %8.2f s   (%.1f GB of device memory free)\n", what,
                std::chrono::duration<double>(t1 - t0).count(), (double)fr / 1e9);
        t0 = t1;
    }
};
// the full image (path order, sparse table, filter) for indexes of 2^31 .. 2^32 - 2^24 columns with k <= 31 (round 5): columns
// and positions as full 32-bit unsigned values, read by k_search_fused<false, false, BIG>.  0: such an index gets blocks +
// dense table only, as before round 5 (23 G k-mers/s on 2.25 x 10^9 columns)
static int g_big_path = env_int("SBWTGPU_BIG_PATH", 1);
// long reads are cut into pieces on the device (SbwtPieceTab); 0: one lane per read whatever its length (tests)
static int g_split_long = env_int("SBWTGPU_SPLIT_LONG", 1);
// batches of reads of different lengths through the fused kernel (it fetches their offsets); 0: only reads of one length
static int g_fused_ragged = env_int("SBWTGPU_FUSED_RAGGED", 1);
// reads of more than 160 bases through the fused kernel as up to this many pieces of 160 bases (1: such reads go to the general
// kernel).  -1 (default) = 3: for 31 < k <= 63 the fused kernel walks with F_CMP (250-base reads 115 -> 243 G k-mers/s, the
// general kernel has neither bridges nor anchors there); for k <= 31 pieces and the two-pass route came out the same until
// round 5 made the fused kernel's writer cheaper (250-base reads: 235 vs 228 G, lengths 80-250: 203 vs 200 G, NOTES.md)
static int g_fused_pieces = env_int("SBWTGPU_FUSED_PIECES", -1);
// stitched chains (sbwt_derived.hip): 0 = vertex-disjoint paths only; the shortest stretch worth copying
static int g_path_stitch = env_int("SBWTGPU_PATH_STITCH", 1);
static int g_path_stitch_min = env_int("SBWTGPU_PATH_STITCH_MIN", 1);
// buckets of the sparse tables per 100 columns (two 16-byte entries each): 125 = 40 % of the slots in use (~6 % of the keys
// overflow their bucket), 100 = 50 % (~10 %): 8 bytes per column against 0.1 more probes per read.  0 (default) = by the index:
// 100 for k <= 31 (round 5, one box: config 2 4.74 vs 4.90 ms, config 3 6.39 vs 6.54 ms -- the smaller table is no slower), 125 where
// whole k-mers take two levels (k = 63: 4.18 ms at 125, 4.26 at 110, 4.29 at 100)
static int g_sparse_buckets_pct = [] { const int v = env_int("SBWTGPU_SPARSE_BUCKETS_PCT", 0); return v <= 0 ? 0 : v < 60 ? 60 : v > 400 ? 400 : v; }();
// per-read hit profiles (sbwt_readhits.hip): reads of this many windows or more are reduced by a wave instead of a lane; the
// host entry point's chunk budget in bases (0: 64 Mi); 1: int64 results on indexes that would take int32 (tests)
static int g_rh_wave_min = SBWT_RH_WAVE_MIN;
static int64_t g_rh_chunk_bases = 0;
static int g_rh_wide = 0;
static int64_t g_wk_chunk_bases = 0;      // "walks_chunk_bases": 0 = the default of 64 Mi
static int64_t g_pa_chunk_bases = 0;      // "pseudoalign_chunk_bases": 0 = the default of 64 Mi
static int64_t g_screen_chunk_bases = 0;  // "screen_chunk_bases": 0 = the default of 64 Mi
// shared k-mers (sbwt_colormatrix.hip): objects of this many sets or more go to the matrix cores, smaller ones to the plain
// kernel; the sets a wave adds up in 32 bits before it adds into the 64-bit matrix.  Neither shows in a result.
static int64_t g_gram_mfma_min_sets = SBWT_GM_MIN_SETS_DEFAULT;
static int64_t g_gram_flush_sets = SBWT_GM_FLUSH_DEFAULT;
// depth of the sparse (hashed) prefix table built at index creation (capped at k and at 31 = one 62-bit key)
static int g_sparse_depth = env_int("SBWTGPU_SPARSE_PRECALC", 31);

struct sbwtgpu_index {
    SbwtBlobHeader h;
    int device = 0;
    char *blob = nullptr;       // device
    bool owns_blob = true;
    // the LCS array of matching statistics (sbwt_ms.hip): its own allocation, outside the blob and its byte cap, built on
    // the first call that needs it (sbwtgpu_index_build_lcs); replicas (adopt / bcast) build their own
    mutable std::mutex lcs_mu;
    mutable unsigned char *lcs = nullptr;
    // probe length of the certificate walks: long enough that a random string of that length is almost
    // surely absent (log4(#k-mers) + 4), at least one char longer than the device prefix table
    int probe_len(bool allow_override = true) const {
        if (allow_override && g_probe_override >= 0) return g_probe_override < h.k ? g_probe_override : 0;
        int64_t nk = h.n_kmers > 0 ? h.n_kmers : h.n_nodes;
        int L = 4;
        while (L < 40 && ((int64_t)1 << (2 * L)) < nk) L++;
        L += 4;
        if (L < h.p_dev + 2) L = (int)h.p_dev + 2;
        if (L > h.k - 1) return 0;
        return L;
    }
    SbwtIndexView view() const {
        SbwtIndexView v;
        v.blocks = reinterpret_cast<const uint4 *>(blob + h.off_blocks);
        v.ptab = h.p_dev > 0 ? reinterpret_cast<const longlong2 *>(blob + h.off_ptab) : nullptr;
        v.mega = reinterpret_cast<const unsigned long long *>(blob + h.off_mega);
        v.n_nodes = h.n_nodes;
        v.n_pos = h.n_pos > 0 ? h.n_pos : h.n_nodes;
        for (int i = 0; i < 4; i++) v.C[i] = h.C[i];
        v.k = (int)h.k;
        v.p_dev = (int)h.p_dev;
        v.n_mega = (int)h.n_mega;
        v.has_ssup = h.has_ssup;
        v.probe_len = probe_len();
        v.debug = g_debug;
        v.fused_sort = g_fused_sort;
        v.big = h.big_layout;
        v.out32 = t_out32;
        v.force_mega = h.force_mega;
        v.p_sparse = (int)h.p_sparse;
        v.n_sb = (unsigned)h.n_sb;
        v.stab = h.p_sparse > 0 ? reinterpret_cast<const uint4 *>(blob + h.off_stab) : nullptr;
        v.col = h.has_path ? reinterpret_cast<const unsigned *>(blob + h.off_col) : nullptr;
        v.pos = h.has_path ? reinterpret_cast<const unsigned *>(blob + h.off_pos) : nullptr;
        v.pq = h.has_path ? reinterpret_cast<const uint4 *>(blob + h.off_pq) : nullptr;
        v.trans = (h.has_path && h.n_tslots > 0) ? reinterpret_cast<const uint4 *>(blob + h.off_trans) : nullptr;
        v.stab_pos = h.stab_pos;
        v.n_tslots = (unsigned)h.n_tslots;
        v.has_safe = h.has_safe;
        v.stab2 = h.n_sb2 > 0 ? reinterpret_cast<const uint4 *>(blob + h.off_stab2) : nullptr;
        v.n_sb2 = (unsigned)h.n_sb2;
        v.pfil = h.p_filter > 0 ? reinterpret_cast<const uint4 *>(blob + h.off_pfil) : nullptr;
        v.p_filter = (int)h.p_filter;
        v.log2f = (int)h.log2f;
        return v;
    }
};

// Which path-order route by default: the fused one (equal-length batches in one kernel, everything else through the
// general kernel behind it).
static inline int auto_variant(const SbwtBlobHeader &) { return 5; }

extern "C" {

#define SBWT_STR2(x) #x
#define SBWT_STR(x) SBWT_STR2(x)
#if SBWT_MEGA_SHIFT == 31
const char *sbwtgpu_version(void) { return "sbwtgpu 0.1 (gfx950)"; }
#else       // a test build with small mega blocks says so: its tests check that they loaded it
const char *sbwtgpu_version(void) { return "sbwtgpu 0.1 (gfx950) mega_shift=" SBWT_STR(SBWT_MEGA_SHIFT); }
#endif
const char *sbwtgpu_last_error(void) { return g_err; }

int sbwtgpu_set_tuning(const char *key, int64_t value) {
    if (!key) return fail(SBWTGPU_ERR_INVALID_ARG, "key is NULL");
    if (!strcmp(key, "search_variant")) { g_variant_override = (int)value; return SBWTGPU_OK; }
    if (!strcmp(key, "probe_len")) { g_probe_override = (int)value; return SBWTGPU_OK; }
    if (!strcmp(key, "debug")) { g_debug = (int)value; return SBWTGPU_OK; }
    if (!strcmp(key, "kernel_events")) { g_kernel_events = (int)value; if (value) g_ev_count = 0; return SBWTGPU_OK; }
    if (!strcmp(key, "derive_ssup")) { g_derive_ssup = (int)value; return SBWTGPU_OK; }
    if (!strcmp(key, "poison_results")) { g_poison = (int)value; return SBWTGPU_OK; }
    if (!strcmp(key, "probe_filter")) { g_probe_filter = (int)value; return SBWTGPU_OK; }   // indexes created afterwards
    if (!strcmp(key, "big_path")) { g_big_path = (int)value; return SBWTGPU_OK; }           // indexes created afterwards
    if (!strcmp(key, "image_level")) { g_image_level = (int)value; return SBWTGPU_OK; }          // indexes created afterwards
    if (!strcmp(key, "max_image_bytes")) { g_max_image_bytes = value; return SBWTGPU_OK; }     // indexes created afterwards
    if (!strcmp(key, "sort_reads")) { g_sort_reads = (int)value; return SBWTGPU_OK; }
    if (!strcmp(key, "trans_wide")) return SBWTGPU_OK;     // (round 2: wide transition entries; the table is sparse now)
    if (!strcmp(key, "force_mega")) { g_force_mega = (int)value; return SBWTGPU_OK; }     // indexes created afterwards
    if (!strcmp(key, "trans_ext")) return SBWTGPU_OK;      // (round 2: transitions always run on along their quoted steps now)
    if (!strcmp(key, "path_safe")) { g_path_safe = (int)value; return SBWTGPU_OK; }   // indexes created afterwards
    if (!strcmp(key, "path_lookahead")) { g_path_lookahead = value < 0 ? 0 : value > 64 ? 64 : (int)value; return SBWTGPU_OK; }
    if (!strcmp(key, "path_order")) { g_path_order = (int)value; return SBWTGPU_OK; }   // indexes created afterwards
    if (!strcmp(key, "fused_table")) { g_fused_table = (int)value; return SBWTGPU_OK; }
    if (!strcmp(key, "fused_sort")) { g_fused_sort = (int)value; return SBWTGPU_OK; }
    if (!strcmp(key, "fused_ragged")) { g_fused_ragged = (int)value; return SBWTGPU_OK; }
    if (!strcmp(key, "fused_pieces")) { g_fused_pieces = value < 1 ? -1 : value > 3 ? 3 : (int)value; return SBWTGPU_OK; }
    if (!strcmp(key, "split_long")) { g_split_long = (int)value; return SBWTGPU_OK; }
    if (!strcmp(key, "path_stitch")) { g_path_stitch = (int)value; return SBWTGPU_OK; }   // indexes created afterwards
    if (!strcmp(key, "path_stitch_min")) { g_path_stitch_min = (int)value < 1 ? 1 : (int)value; return SBWTGPU_OK; }
    if (!strcmp(key, "read_hits_wave_min")) { g_rh_wave_min = value < 1 ? SBWT_RH_WAVE_MIN : value > 0x7fffffff ? 0x7fffffff : (int)value; return SBWTGPU_OK; }
    if (!strcmp(key, "read_hits_chunk_bases")) { g_rh_chunk_bases = value < 0 ? 0 : value; return SBWTGPU_OK; }
    if (!strcmp(key, "read_hits_wide")) { g_rh_wide = (int)value; return SBWTGPU_OK; }
    if (!strcmp(key, "walks_chunk_bases")) { g_wk_chunk_bases = value < 0 ? 0 : value; return SBWTGPU_OK; }
    if (!strcmp(key, "pseudoalign_chunk_bases")) { g_pa_chunk_bases = value < 0 ? 0 : value; return SBWTGPU_OK; }
    if (!strcmp(key, "screen_chunk_bases")) { g_screen_chunk_bases = value < 0 ? 0 : value; return SBWTGPU_OK; }
    if (!strcmp(key, "gram_mfma_min_sets")) { g_gram_mfma_min_sets = value < 0 ? 0 : value; return SBWTGPU_OK; }
    if (!strcmp(key, "gram_flush_sets")) {
        if (value < 1 || value > SBWT_GM_FLUSH_MAX)
            return fail(SBWTGPU_ERR_INVALID_ARG, "gram_flush_sets must be in 1 .. %lld, not %lld: a wave adds up products of at most 127 "
                        "per set in 32 bits, and 127 * gram_flush_sets must stay below 2^31", (long long)SBWT_GM_FLUSH_MAX, (long long)value);
        g_gram_flush_sets = value;
        return SBWTGPU_OK;
    }
    if (!strcmp(key, "sparse_depth")) {      // takes effect for indexes created afterwards
        if (value < 0 || value > 31) return fail(SBWTGPU_ERR_INVALID_ARG, "sparse_depth must be in [0,31]");
        g_sparse_depth = (int)value;
        return SBWTGPU_OK;
    }
    return fail(SBWTGPU_ERR_INVALID_ARG, "unknown tuning key '%s'", key);
}

int sbwtgpu_device_count(int *count) {
    if (!count) return fail(SBWTGPU_ERR_INVALID_ARG, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(SBWTGPU_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return SBWTGPU_OK;
}

// set while sbwtgpu_index_create retries without the derived structures after running out of device memory
// Image levels: 0 = everything (path order, transition table, sparse table, probe filter: 139-168 bytes per column),
// 1 = no path order (sparse table + filter + dense prefix table: ~66 bytes per column), 2 = blocks + dense prefix table
// only (1 byte per column + the table).  index_create starts at "image_level" (tuning / SBWTGPU_IMAGE_LEVEL), and moves
// to the next level when the image would exceed "max_image_bytes" (SBWTGPU_MAX_IMAGE_BYTES) or device memory runs out.
static thread_local int t_image_level = -1;

int sbwtgpu_index_create(const sbwtgpu_index_desc *d, int device, sbwtgpu_index **out) {
    if (!d || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "desc/out is NULL");
    *out = nullptr;
    if (d->n_nodes <= 0 || !d->A_bits || !d->C_bits || !d->G_bits || !d->T_bits)
        return fail(SBWTGPU_ERR_INVALID_ARG, "n_nodes must be > 0 and the four bit vectors non-NULL");
    if (d->k <= 0 || d->k > 255) return fail(SBWTGPU_ERR_INVALID_ARG, "k must be in [1,255]");
    if (d->precalc_k < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "precalc_k < 0");
    if (d->precalc_k > 20)
        return fail(SBWTGPU_ERR_PRECALC_TOO_LONG,
                    "Error: Can't precalc longer than 20-mers (would take over 4^20 = 2^40 bytes");
    if (d->precalc_k > d->k)
        return fail(SBWTGPU_ERR_PRECALC_GT_K, "Error: Precalc length is longer than k (%lld > %lld)",
                    (long long)d->precalc_k, (long long)d->k);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SBWTGPU_ERR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= ndev) return fail(SBWTGPU_ERR_NO_DEVICE, "device %d out of range", device);
    DeviceGuard guard(device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", device);

    const int64_t n = d->n_nodes;
    const int64_t nw = (n + 63) / 64;
    const int64_t n_blocks = n / 64 + 1;
    const int64_t n_mega = (n >> SBWT_MEGA_SHIFT) + 1;
    int64_t p_file = d->precalc_k;
    const int level = t_image_level >= 0 ? t_image_level : (g_image_level < 0 ? 0 : g_image_level > 2 ? 2 : g_image_level);
    const bool t_minimal_image = level >= 2;
    DevBuf d_bits, d_bscr;                             // the uploaded bit vectors and the block builder's scratch (below)
    auto retry_next_level = [&]() {
        // (this frame's device buffers first: the retry uploads its own, and holding both could push a level that fits down
        // another level)
        if (d_bits.p) { (void)hipFree(d_bits.p); d_bits.p = nullptr; }
        if (d_bscr.p) { (void)hipFree(d_bscr.p); d_bscr.p = nullptr; }
        // never silently: a stepped-down image answers the same and three to ten times slower
        fprintf(stderr, "sbwtgpu: the level-%d image of this index (%lld columns, k = %lld) does not fit the device%s: building level %d "
                        "(%s)\n", level, (long long)n, (long long)d->k, g_max_image_bytes > 0 ? " or \"max_image_bytes\"" : "", level + 1,
                level + 1 == 1 ? "no path order: the blocks-only search kernel" : "blocks and dense prefix table only");
        t_image_level = level + 1;
        const int rc2 = sbwtgpu_index_create(d, device, out);
        t_image_level = -1;
        return rc2;
    };
    // 2^31 - 64 <= n < 2^32 - 2^24 (round 5): the same derived structures with full 32-bit unsigned columns and positions,
    // when whole k-mers fit the sparse table (k <= 31: every found k-mer comes with its path position, so no segment source
    // needs bit 31 as a flag) and the marks are there; absolute 32-bit block counts (the mega table stays zero)
    // (round 6: 31 < k <= 63 as well -- the second-level table's entries hold position + 1 and no flags in that layout.
    // "big_path" 2 gives ANY index that layout: the BIG instantiations are tested on small indexes)
    const bool big_range = (n >= ((int64_t)1 << 31) - 64 || g_big_path == 2) && n < ((int64_t)1 << 32) - ((int64_t)1 << 24);
    const bool big_k = d->k <= SBWT_SP_MAX_DEPTH ? g_sparse_depth >= d->k
                                                 : (d->k - SBWT_SP_MAX_DEPTH <= 32 && g_sparse_depth >= SBWT_SP_MAX_DEPTH);
    const bool big_path = big_range && g_big_path && level == 0 && d->k > 16 && big_k &&
                          g_probe_filter && g_path_order && (d->suffix_group_starts || g_derive_ssup);
    const bool derived = !t_minimal_image && g_sparse_depth > 0 && g_probe_filter &&
                         ((n < ((int64_t)1 << 31) - 64 && n_mega == 1) || big_path) && d->k > 16;
    int64_t p_dev = default_device_precalc(n, derived);
    if (p_dev < p_file) p_dev = p_file;
    if (p_dev > d->k) p_dev = d->k;
    if (level >= 2 && g_max_image_bytes > 0) {
        // the smallest kind of image under a cap: the deepest dense table that still fits (each level is 4x the bytes)
        auto est = [&](int64_t pd) {
            return align256(n_blocks * 64) + (pd > 0 ? (int64_t)16 << (2 * pd) : 0) +
                   ((p_file > 0 && p_file != pd) ? (int64_t)16 << (2 * p_file) : 0) + 4 * n_mega * 8 + 1024;
        };
        while (p_dev > p_file && p_dev > 0 && est(p_dev) > g_max_image_bytes) p_dev--;
    }

    sbwtgpu_index *idx = new (std::nothrow) sbwtgpu_index();
    if (!idx) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    SbwtBlobHeader &h = idx->h;
    memset(&h, 0, sizeof(h));
    h.magic = SBWT_BLOB_MAGIC;
    h.n_nodes = n;
    h.n_kmers = d->n_kmers;
    h.k = d->k;
    h.p_file = p_file;
    h.p_dev = p_dev;
    h.n_blocks = n_blocks;
    h.n_mega = n_mega;
    h.has_ssup = d->suffix_group_starts ? 1 : 0;
    h.off_blocks = 0;
    h.off_ptab = align256(n_blocks * 64);
    int64_t ptab_bytes = p_dev > 0 ? (int64_t)16 << (2 * p_dev) : 0;   // revised below for rank-only images
    h.off_ftab = align256(h.off_ptab + ptab_bytes);
    int64_t ftab_bytes = (p_file > 0 && p_file != p_dev) ? (int64_t)16 << (2 * p_file) : 0;
    (void)ptab_bytes;
    if (ftab_bytes == 0) h.off_ftab = h.off_ptab;   // the same table serves both
    h.off_mega = align256(h.off_ftab + (ftab_bytes ? ftab_bytes : ptab_bytes));
    h.blob_bytes = align256(h.off_mega + 4 * n_mega * 8);
    // sparse table one level above the dense one: 32-bit intervals only, one bucket per column on average
    int64_t p_sparse = g_sparse_depth < d->k ? g_sparse_depth : d->k;
    if (t_minimal_image) p_sparse = 0;
    if (p_sparse > SBWT_SP_MAX_DEPTH) p_sparse = SBWT_SP_MAX_DEPTH;
    if (p_sparse <= p_dev || p_dev <= 0 || n >= ((int64_t)1 << 32) || (n_mega > 1 && !big_path)) p_sparse = 0;
    // (2^31 columns and more: whole k-mers with their positions -- in the table itself, or through the second level -- or nothing)
    if (big_path && p_sparse != d->k && !(p_sparse == SBWT_SP_MAX_DEPTH && d->k > p_sparse && d->k - p_sparse <= 32)) p_sparse = 0;
    if (p_sparse > 0) {
        h.p_sparse = (int32_t)p_sparse;
        // (2^31 columns and more with two levels: one bucket per column in both -- at 1.25 the two tables are 180 GB of a 2.25 x 10^9-
        // column image and leave their own builder 7 GB short of its 108 GB of scratch on a 288 GB device)
        const int64_t bpct = g_sparse_buckets_pct > 0 ? g_sparse_buckets_pct
                                                      : (d->k > SBWT_SP_MAX_DEPTH && !(big_path && n >= ((int64_t)1 << 31) - 64) ? 125 : 100);
        h.n_sb = n * bpct / 100 + 64;       // two-entry buckets per column
        h.off_stab = h.blob_bytes;
        h.blob_bytes = align256(h.off_stab + 32 * h.n_sb);
        // second level for 31 < k <= 63 (the remaining k-31 bases fit one 64-bit key): 1.25 two-entry buckets per column, like the
        // first level (round 3: 2 n single 32-byte entries with linear probing -- a miss walked 2.5 of them)
        // (its entries keep their flags in bit 31 of the column / origin words: columns below 2^31 only -- p_sparse > 0 already
        // implies one mega block; said again here because a wider first level must not widen this one by accident)
        if (p_sparse == SBWT_SP_MAX_DEPTH && d->k > p_sparse && d->k - p_sparse <= 32 && (n < ((int64_t)1 << 31) - 64 || big_path)) {
            h.n_sb2 = n * bpct / 100 + 64;
            h.off_stab2 = h.blob_bytes;
            h.blob_bytes = align256(h.off_stab2 + 32 * h.n_sb2);
        }
        // probe filter at the certificate probes' length: 128-bit blocks of 8 .. 16 windows (8 .. 16 bits per column; round 5:
        // half of what it was -- config 2 at 12 windows per block runs as at 6, 4.69 vs 4.66 ms; at 24 it is 2.5 % slower).
        // A filter of more than 128 MB goes up to 20 per block: config 3 (142 M columns) 6.23 ms at 4 per block / 512 MB,
        // 6.18 at 8 / 256 MB, 6.09 at 17 / 128 MB, 6.23 at 34 -- the smaller filter stays in the Infinity Cache, and that is
        // worth more than the false positives cost (profiles/r05_experiments.txt)
        const int L0 = idx->probe_len(false);
        if (g_probe_filter && L0 > p_dev && L0 <= p_sparse) {
            int lf = 4;
            while (((int64_t)16 << lf) < n) lf++;
            if (((int64_t)16 << lf) > ((int64_t)128 << 20) && n <= ((int64_t)10 << lf)) lf--;
            // (experiments: SBWTGPU_FILTER_LOG2_ADJ = -1 halves the filter once more, 1 doubles it)
            { const char *ea = getenv("SBWTGPU_FILTER_LOG2_ADJ"); if (ea) { lf += atoi(ea); if (lf < 4) lf = 4; } }
            h.p_filter = L0;
            h.log2f = lf;
            h.off_pfil = h.blob_bytes;
            h.blob_bytes = align256(h.off_pfil + ((int64_t)16 << lf));
        }
    }
    // path order: needs suffix-group marks (given or derived) and 32-bit columns
    const bool marks = d->suffix_group_starts || (g_derive_ssup && d->k >= 2);
    int64_t pos_cap = n;
    if (g_path_order && level == 0 && marks && ((n < ((int64_t)1 << 31) - 64 && n_mega == 1 && !big_path) || (big_path && p_sparse > 0))) {
        // room for the path order with stitched chains (copies of shared stretches: at most a fifth of the columns, and
        // positions stay below 2^31); the finished image keeps what was used.  (2^31 columns and more: disjoint paths only --
        // the copies' room and the stitching's temporaries are what such an image has no memory for)
        pos_cap = (g_path_stitch && !big_path) ? std::min<int64_t>(n + n / 5 + 64, ((int64_t)1 << 31) - 64) : n;
        if (pos_cap < n) pos_cap = n;
        h.has_path = 1;
        h.big_layout = big_path ? 1 : 0;
        h.off_col = h.blob_bytes;
        h.off_pos = align256(h.off_col + (pos_cap + 4) * 4);
        h.off_pq = align256(h.off_pos + (n + 4) * 4);
        h.off_trans = align256(h.off_pq + sbwt_path_quads(pos_cap) * 16);
        h.blob_bytes = h.off_trans;        // the transition table follows once the path order has said how many entries it needs
    }
    idx->device = device;

    // The bit vectors go to the device once; counting, the per-block prefix counts and the interleaving all happen
    // there (sbwt_build.hip) -- 142 M columns took seconds in host loops.
    const uint64_t *cols[4] = {d->A_bits, d->C_bits, d->G_bits, d->T_bits};
    {
        hipError_t eb = d_bits.alloc((size_t)(5 * nw) * 8);
        if (eb == hipSuccess) eb = d_bscr.alloc((size_t)sbwt_blocks_scratch_bytes(n));
        for (int c = 0; c < 4 && eb == hipSuccess; c++)
            eb = hipMemcpy(static_cast<char *>(d_bits.p) + (size_t)c * (size_t)nw * 8, cols[c], (size_t)nw * 8, hipMemcpyHostToDevice);
        if (eb == hipSuccess && d->suffix_group_starts)
            eb = hipMemcpy(static_cast<char *>(d_bits.p) + (size_t)4 * (size_t)nw * 8, d->suffix_group_starts, (size_t)nw * 8,
                           hipMemcpyHostToDevice);
        if (eb != hipSuccess) {
            delete idx;
            return fail(eb == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "uploading the bit vectors: %s",
                        hipGetErrorString(eb));
        }
    }
    // C array (SBWT.hh:344-349): C[0] = 1 (ghost dollar into the root), C[i+1] = C[i] + rank(n, sigma_i)
    long long tot[5] = {0, 0, 0, 0, 0};
    if (sbwt_blocks_count(static_cast<const unsigned long long *>(d_bits.p), n, d_bscr.p, tot, 0) != 0) {
        delete idx;
        return fail(SBWTGPU_ERR_HIP, "counting the set bits on the device failed");
    }
    h.C[0] = 1;
    for (int c = 1; c < 4; c++) h.C[c] = h.C[c - 1] + tot[c - 1];
    h.path_lookahead = h.has_path ? g_path_lookahead : 0;
    // In an SBWT every column except the root has exactly one incoming edge, so the matrix holds
    // n_nodes - 1 set bits and every LF step stays inside [0, n_nodes).  Arbitrary bit vectors (the
    // stand-alone SubsetMatrixRank use) are still served, but only by rank(): walking them would
    // leave the image.
    const bool consistent = (tot[0] + tot[1] + tot[2] + tot[3] == n - 1);
    h.rank_only = consistent ? 0 : 1;
    // Dense arbitrary bit vectors: C[c] + rank_c can pass 2^32 well before n reaches 2^31 columns.  Then the 32-bit
    // block counts are stored relative to mega[c][0] = C[c] (inside one mega block rank_c <= 2^31 always fits).
    for (int c = 0; c < 4; c++) h.row_ones[c] = tot[c];
    h.force_mega = (n_mega == 1 && ((uint64_t)(h.C[3] + tot[3]) >= (1ull << 32) || (g_force_mega && !consistent))) ? 1 : 0;
    if (!consistent) {
        if (p_file > 0) {
            delete idx;
            return fail(SBWTGPU_ERR_INVALID_ARG,
                        "the four columns hold %lld set bits, an SBWT with %lld columns holds %lld: cannot "
                        "compute a prefix table", (long long)(tot[0] + tot[1] + tot[2] + tot[3]), (long long)n,
                        (long long)(n - 1));
        }
        p_dev = 0;
        h.p_dev = 0;
        h.has_ssup = 0;
        h.p_sparse = 0;
        h.n_sb2 = 0;
        h.p_filter = 0;
        h.has_path = 0;
        h.big_layout = 0;
    }
    if (d->precalc && p_file > 0) {
        const int64_t np = (int64_t)1 << (2 * p_file);
        for (int64_t e = 0; e < np; e++) {
            int64_t l = d->precalc[2 * e], r = d->precalc[2 * e + 1];
            if (!((l == -1 && r == -1) || (l >= 0 && l <= r && r < n))) {
                delete idx;
                return fail(SBWTGPU_ERR_INVALID_ARG, "prefix table entry %lld = (%lld, %lld) is outside the index",
                            (long long)e, (long long)l, (long long)r);
            }
        }
    }

    if (h.rank_only) {   // no tables in a rank-only image
        ptab_bytes = 0;
        ftab_bytes = 0;
        h.off_ptab = h.off_ftab = align256(n_blocks * 64);
        h.off_mega = h.off_ptab;
        h.blob_bytes = align256(h.off_mega + 4 * n_mega * 8);
        h.off_stab = 0;
        h.n_sb = 0;
        h.off_col = h.off_pos = h.off_pq = h.off_trans = 0;
    }
    h.image_level = (h.has_path ? 0 : h.p_sparse > 0 ? 1 : 2);
    if (g_max_image_bytes > 0 && h.blob_bytes > g_max_image_bytes) {
        // the derived structures are optional, and at level 2 the dense table shrinks until the image fits: an index without
        // path order or sparse table (k <= 16, or both switched off) still has that last resort
        if (level < 2) {
            delete idx;
            return retry_next_level();
        }
        delete idx;
        return fail(SBWTGPU_ERR_OOM, "the smallest image of this index (%lld bytes: blocks + depth-%lld prefix table) exceeds "
                    "max_image_bytes = %lld", (long long)h.blob_bytes, (long long)h.p_dev, (long long)g_max_image_bytes);
    }
    // An image with a path order is built in TWO allocations (round 6): first the index proper and the path arrays (at temporary
    // offsets right behind the mega table), then -- the path order says how long col[] is and how many transition entries there
    // are -- the image at its final size, into which the sparse tables and the filter are built directly.  (Before, everything
    // was built in one allocation and moved at the end: twice the image at the peak, which a 164 GB image of 2.25 x 10^9
    // columns at k = 32 does not have.)
    const int64_t f_off_col = h.off_col, f_blob_bytes = h.blob_bytes;       // (the one-allocation layout, for the size checks)
    int64_t p1_bytes = h.blob_bytes;
    if (h.has_path) {
        h.off_col = align256(h.off_mega + 4 * n_mega * 8);
        h.off_pos = align256(h.off_col + (pos_cap + 4) * 4);
        h.off_pq = align256(h.off_pos + (n + 4) * 4);
        p1_bytes = align256(h.off_pq + sbwt_path_quads(pos_cap) * 16);
    }
    (void)f_blob_bytes;
    hipError_t e = hipMalloc((void **)&idx->blob, (size_t)p1_bytes);
    if (e != hipSuccess && level < 2 && (h.has_path || h.p_sparse > 0)) {
        // the derived structures are optional: without them the blocks-only kernel serves
        (void)hipGetLastError();
        delete idx;
        return retry_next_level();
    }
    if (e != hipSuccess) {
        delete idx;
        return fail(SBWTGPU_ERR_OOM, "hipMalloc(%lld bytes) for the index image: %s", (long long)h.blob_bytes,
                    hipGetErrorString(e));
    }
    int rc = SBWTGPU_OK;
    unsigned char *alt_safe = nullptr;                 // per-position verdicts of the safe-bit pass, for the transition table
    // One scratch allocation serves the path order, the sparse tables and the safe bits in turn (round 6): fresh device memory
    // costs 20-30 ms per GB on this driver once an allocation goes beyond what the process has had before (2.25 x 10^9 columns: 128 GB
    // for the path order and 108 GB for the sparse tables were 5.9 s of an 10.8 s image).  It is let go early only where the final
    // image does not fit beside it (2.25 x 10^9 columns at k = 32: 167 GB).  SBWTGPU_SCRATCH_ARENA=0: an allocation per phase, as before.
    static const int use_arena = env_int("SBWTGPU_SCRATCH_ARENA", 1);
    void *arena = nullptr;
    size_t arena_bytes = 0;
    auto arena_drop = [&] { if (arena) (void)hipFree(arena); arena = nullptr; arena_bytes = 0; };
    auto arena_get = [&](size_t need, size_t later) -> void * {        // (later: what the phases behind this one will ask for)
        if (arena && arena_bytes >= need) return arena;
        arena_drop();
        const size_t want = (use_arena && later > need) ? later : need;
        if (hipMalloc(&arena, want) == hipSuccess) { arena_bytes = want; return arena; }
        (void)hipGetLastError();
        arena = nullptr;
        if (want > need && hipMalloc(&arena, need) == hipSuccess) { arena_bytes = need; return arena; }
        (void)hipGetLastError();
        arena = nullptr;
        return nullptr;
    };
    PhaseLog plog;
    plog("upload, counts, allocation");
    do {
        if ((e = hipMemset(idx->blob, 0, (size_t)p1_bytes)) != hipSuccess) break;
        {
            const long long Cs[4] = {h.C[0], h.C[1], h.C[2], h.C[3]};
            sbwt_blocks_fill(static_cast<const unsigned long long *>(d_bits.p),
                             d->suffix_group_starts ? static_cast<const unsigned long long *>(d_bits.p) + 4 * nw : nullptr, n,
                             d_bscr.p, Cs, ((n_mega > 1 && !(big_path && consistent)) || h.force_mega) ? 1 : 0, (int)n_mega,
                             reinterpret_cast<uint4 *>(idx->blob + h.off_blocks),
                             reinterpret_cast<unsigned long long *>(idx->blob + h.off_mega), 0);
            if ((e = hipDeviceSynchronize()) != hipSuccess) break;
            (void)hipFree(d_bits.p); d_bits.p = nullptr;          // the derived structures need the room
            (void)hipFree(d_bscr.p); d_bscr.p = nullptr;
        }
        SbwtIndexView v = idx->view();
        if (!d->suffix_group_starts && !h.rank_only && g_derive_ssup && d->k >= 2) {
            // no streaming support in the file: derive the marks for internal use (has_ssup stays 0)
            void *scr = nullptr;
            if ((e = hipMalloc(&scr, (size_t)sbwt_derive_scratch_bytes(n))) != hipSuccess) break;
            sbwt_launch_derive_marks(v, reinterpret_cast<uint4 *>(idx->blob + h.off_blocks), scr, 0);
            e = hipDeviceSynchronize();
            (void)hipFree(scr);
            if (e != hipSuccess) break;
            h.ssup_derived = 1;
        }
        plog("blocks (+ derived marks)");
        if (p_dev > 0) sbwt_launch_precalc(v, (int)p_dev, reinterpret_cast<longlong2 *>(idx->blob + h.off_ptab), 0);
        if (ftab_bytes) {
            if (d->precalc) {
                if ((e = hipMemcpy(idx->blob + h.off_ftab, d->precalc, (size_t)ftab_bytes, hipMemcpyHostToDevice)) !=
                    hipSuccess)
                    break;
            } else {
                sbwt_launch_precalc(v, (int)p_file, reinterpret_cast<longlong2 *>(idx->blob + h.off_ftab), 0);
            }
        }
        plog("dense prefix table(s)");
        if (h.has_path) {
            void *scr = arena_get((size_t)sbwt_path_scratch_bytes(n), h.p_sparse > 0 ? (size_t)sbwt_sparse_scratch_bytes(n) : 0);
            if (!scr) { e = hipErrorOutOfMemory; break; }
            if (g_verbose >= 2) plog("  (path order: scratch allocated)");
            long long n_pos = n;
            int prc = sbwt_launch_build_path(v, reinterpret_cast<unsigned *>(idx->blob + h.off_col),
                                             reinterpret_cast<unsigned *>(idx->blob + h.off_pos),
                                             reinterpret_cast<uint4 *>(idx->blob + h.off_pq), pos_cap, &n_pos, g_path_stitch,
                                             g_path_stitch_min, scr, g_path_lookahead, 0);
            if (g_verbose >= 2) plog("  (path order: built)");
            if (!use_arena) arena_drop();
            if (prc != 0) { e = hipErrorUnknown; break; }
            h.n_pos = n_pos;
            // col[n_pos] = 0xFFFFFFFF: the "position" whose column is -1 (the fused kernel's writer loads every result, absent
            // ones included, through col[]; the array has four entries of padding behind the last position)
            if ((e = hipMemset(idx->blob + h.off_col + (size_t)n_pos * 4, 0xFF, 16)) != hipSuccess) break;
            // ---- the final layout: the transition table's size (three entries per branching column, one per successor of a
            //      path's last column: counted now, filled in at the end) and the path arrays at the length the path order
            //      turned out to have; the image moves into its final allocation (the index proper and the path arrays:
            //      a tenth of it), the sparse tables and the filter are built there ----
            long long nb = 0;
            const long long n_ent = sbwt_launch_path_oth(idx->view(), reinterpret_cast<uint4 *>(idx->blob + h.off_pq), &nb, 0, 1);
            if (n_ent < 0) { e = hipErrorUnknown; break; }
            h.n_branch = nb;
            h.n_trans = n_ent;
            const int64_t n_slots = 3 * n_ent + 64;                         // load factor 1/3: ~1.25 probes per lookup
            if (n_slots >= ((int64_t)1 << 32)) { e = hipErrorOutOfMemory; break; }
            h.n_tslots = n_slots;
            const int64_t col_bytes = align256((h.n_pos + 4) * 4), pos_bytes = align256((n + 4) * 4);
            const int64_t pq_bytes = align256(sbwt_path_quads(h.n_pos) * 16);
            const int64_t new_pos = f_off_col + col_bytes, new_pq = new_pos + pos_bytes, new_trans = new_pq + pq_bytes;
            const int64_t full = align256(new_trans + 32 * n_slots);
            if (g_max_image_bytes > 0 && full > g_max_image_bytes && level < 2) { e = hipErrorOutOfMemory; break; }
            char *nblob = nullptr;
            if (g_verbose >= 2) plog("  (transition entries counted)");
            e = hipMalloc((void **)&nblob, (size_t)full);
            if (e != hipSuccess && arena) {             // (no room beside the scratch: the scratch goes first)
                (void)hipGetLastError();
                arena_drop();
                e = hipMalloc((void **)&nblob, (size_t)full);
            }
            if (e != hipSuccess) break;
            if (arena) {                                // (what is still to come -- alt_safe, the builders' small buffers -- must not fail for it)
                size_t fr = 0, tot = 0;
                if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < (size_t)h.n_pos * 2 + ((size_t)4 << 30)) arena_drop();
            }
            if (g_verbose >= 2) plog("  (final allocation)");
            const int64_t head = h.off_col;                                 // blocks, tables, mega: the same offsets in both
            if ((e = hipMemcpy(nblob, idx->blob, (size_t)head, hipMemcpyDeviceToDevice)) != hipSuccess ||
                (e = hipMemset(nblob + head, 0, (size_t)(f_off_col - head))) != hipSuccess ||        // the sparse tables' and the filter's room
                (e = hipMemcpy(nblob + f_off_col, idx->blob + h.off_col, (size_t)col_bytes, hipMemcpyDeviceToDevice)) != hipSuccess ||
                (e = hipMemcpy(nblob + new_pos, idx->blob + h.off_pos, (size_t)pos_bytes, hipMemcpyDeviceToDevice)) != hipSuccess ||
                (e = hipMemcpy(nblob + new_pq, idx->blob + h.off_pq, (size_t)pq_bytes, hipMemcpyDeviceToDevice)) != hipSuccess) {
                (void)hipFree(nblob);
                break;
            }
            if (g_verbose >= 2) plog("  (moved)");
            (void)hipFree(idx->blob);
            idx->blob = nblob;
            h.off_col = f_off_col;
            h.off_pos = new_pos;
            h.off_pq = new_pq;
            h.off_trans = new_trans;
            h.blob_bytes = full;
            v = idx->view();
        }
        plog("path order, final layout");
        if (h.p_sparse > 0) {
            void *scr = arena_get((size_t)sbwt_sparse_scratch_bytes(n), 0);
            if (!scr) { e = hipErrorOutOfMemory; break; }
            if (g_verbose >= 2) plog("  (sparse tables: scratch allocated)");
            int src = sbwt_launch_build_sparse(v, (int)p_dev, (int)h.p_sparse, (long long)h.n_sb,
                                               reinterpret_cast<uint4 *>(idx->blob + h.off_stab), scr,
                                               h.has_path ? reinterpret_cast<const unsigned *>(idx->blob + h.off_pos) : nullptr,
                                               (int)h.p_filter, (int)h.log2f,
                                               h.p_filter > 0 ? reinterpret_cast<uint4 *>(idx->blob + h.off_pfil) : nullptr,
                                               (long long)h.n_sb2,
                                               h.n_sb2 > 0 ? reinterpret_cast<uint4 *>(idx->blob + h.off_stab2) : nullptr, 0);
            e = hipDeviceSynchronize();
            if (g_verbose >= 2) plog("  (sparse tables: built)");
            if (!use_arena) arena_drop();
            if (src == -3) { h.n_sb2 = 0; src = 0; }   // some k-mer spans several columns: no second level
            if (src < 0 && e == hipSuccess) e = hipErrorUnknown;
            if (e != hipSuccess) break;
            h.stab_pos = src > 0 ? 1 : 0;
            plog("sparse table, second level, filter");
            // (2^31 columns and more: the fused kernel's BIG instantiation needs every k-mer's position in its table entry;
            // without them -- the columns are not an SBWT's -- the image steps down like one that does not fit)
            if (big_path && h.has_path && !(h.stab_pos || (h.n_sb2 > 0 && d->k > h.p_sparse))) { e = hipErrorOutOfMemory; break; }
            // substitution-safe bits of the path: need the whole k-mers in the sparse table
            // (31 < k <= 63: whole k-mers live in the two-level table -- the wide kernels, rule 2 only)
            const bool whole_kmers = h.p_sparse == d->k || (h.n_sb2 > 0 && d->k > h.p_sparse);
            if (h.has_path && whole_kmers && g_path_safe) {
                SbwtIndexView v2 = idx->view();
                // (rule 2 keeps the path heads' labels and their list in scratch)
                void *hscr = nullptr;
                const bool wide_safe = d->k > h.p_sparse;
                const size_t safe_bytes = (size_t)sbwt_path_safe_scratch_bytes(h.n_pos, (int)d->k);
                const bool hscr_in_arena = arena && arena_bytes >= safe_bytes;
                if (!hscr_in_arena) arena_drop();       // (too small to serve: its room may be what the allocation below needs)
                if (g_path_safe >= 2 || wide_safe) {
                    if (hscr_in_arena) hscr = arena;
                    else if (hipMalloc(&hscr, safe_bytes) != hipSuccess) {
                        (void)hipGetLastError();
                        hscr = nullptr;                 // no room for rule 2: the narrow rule needs none
                    }
                }
                // ... and hands the per-substitute verdicts to the transition table's negative entries through alt_safe (a byte
                // per position; without it only the steps that are safe for all three substitutes bridge)
                if (hscr && hipMalloc((void **)&alt_safe, (size_t)h.n_pos) != hipSuccess) {
                    (void)hipGetLastError();
                    alt_safe = nullptr;
                }
                sbwt_launch_path_safe(v2, reinterpret_cast<uint4 *>(idx->blob + h.off_pq), hscr ? (wide_safe ? 2 : g_path_safe) : 1, hscr, alt_safe, 0);
                e = hipDeviceSynchronize();
                const bool had_scratch = hscr != nullptr;
                if (hscr && !hscr_in_arena) (void)hipFree(hscr);
                if (e != hipSuccess) break;
                h.has_safe = (wide_safe && !had_scratch) ? 0 : 1;    // (no room for the head labels of long k-mers: no safe bits)
            }
        }
        plog("substitution-safe bits");
        if (h.has_path) {
            // Last: the only-successor bits, the path groups' final encoding, and the transition table (its room was made when
            // the image moved into its final allocation, behind the path order).
            SbwtIndexView v3 = idx->view();
            long long nb = 0;
            const long long n_ent = sbwt_launch_path_oth(v3, reinterpret_cast<uint4 *>(idx->blob + h.off_pq), &nb, 0);
            if (n_ent != h.n_trans) { e = hipErrorUnknown; break; }         // (the count the layout was made for)
            const int64_t n_slots = h.n_tslots;
            plog("only-successor bits");
            sbwt_launch_trans_insert(idx->view(), reinterpret_cast<uint4 *>(idx->blob + h.off_trans), n_slots, alt_safe, 0);
            if ((e = hipDeviceSynchronize()) != hipSuccess) break;
            h.n_paths = sbwt_count_paths(idx->view(), 0);
            if (h.n_paths < 0) { e = hipErrorUnknown; break; }
            plog("transition table");
        }
        if ((e = hipGetLastError()) != hipSuccess) break;
        e = hipDeviceSynchronize();
    } while (0);
    arena_drop();
    if (alt_safe) (void)hipFree(alt_safe);
    if (e == hipErrorOutOfMemory && level < 2 && (h.has_path || h.p_sparse > 0)) {
        (void)hipGetLastError();                       // scratch of a derived structure did not fit: build without them
        (void)hipFree(idx->blob);
        delete idx;
        return retry_next_level();
    }
    if (e != hipSuccess) {
        rc = fail(SBWTGPU_ERR_HIP, "building the index image: %s", hipGetErrorString(e));
        (void)hipFree(idx->blob);
        delete idx;
        return rc;
    }
    *out = idx;
    return SBWTGPU_OK;
}

void sbwtgpu_index_destroy(sbwtgpu_index *idx) {
    if (!idx) return;
    if (idx->blob && idx->owns_blob) {
        DeviceGuard guard(idx->device);
        (void)hipFree(idx->blob);
    }
    if (idx->lcs) {
        DeviceGuard guard(idx->device);
        (void)hipFree(idx->lcs);
    }
    delete idx;
}

int sbwtgpu_index_get_info(const sbwtgpu_index *idx, sbwtgpu_index_info *info) {
    if (!idx || !info) return fail(SBWTGPU_ERR_INVALID_ARG, "idx/info is NULL");
    info->n_nodes = idx->h.n_nodes;
    info->n_kmers = idx->h.n_kmers;
    info->k = idx->h.k;
    info->precalc_k = idx->h.p_file;
    for (int i = 0; i < 4; i++) info->C[i] = idx->h.C[i];
    info->has_streaming_support = idx->h.has_ssup;
    info->device = idx->device;
    info->device_precalc_k = idx->h.p_dev;
    info->blob_bytes = idx->h.blob_bytes;
    info->image_level = idx->h.image_level;
    info->n_paths = idx->h.n_paths;
    info->n_branch = idx->h.n_branch;
    info->default_search_variant = !idx->h.has_path ? 1 : auto_variant(idx->h);
    return SBWTGPU_OK;
}

int sbwtgpu_index_get_precalc(const sbwtgpu_index *idx, int64_t *out_pairs) {
    if (!idx || !out_pairs) return fail(SBWTGPU_ERR_INVALID_ARG, "idx/out is NULL");
    if (idx->h.p_file == 0) return SBWTGPU_OK;
    DeviceGuard guard(idx->device);
    HIP_TRY(hipMemcpy(out_pairs, idx->blob + idx->h.off_ftab, (size_t)16 << (2 * idx->h.p_file),
                      hipMemcpyDeviceToHost));
    return SBWTGPU_OK;
}

// ---- replication ---------------------------------------------------------------------------
int sbwtgpu_index_export_header(const sbwtgpu_index *idx, void *header_out, int64_t cap, int64_t *bytes) {
    if (!idx || !bytes) return fail(SBWTGPU_ERR_INVALID_ARG, "idx/bytes is NULL");
    *bytes = (int64_t)sizeof(SbwtBlobHeader);
    if (!header_out) return SBWTGPU_OK;   // size query
    if (cap < (int64_t)sizeof(SbwtBlobHeader)) return fail(SBWTGPU_ERR_INVALID_ARG, "header buffer too small");
    memcpy(header_out, &idx->h, sizeof(SbwtBlobHeader));
    return SBWTGPU_OK;
}

int sbwtgpu_index_blob(const sbwtgpu_index *idx, void **dev_ptr, int64_t *bytes) {
    if (!idx || !dev_ptr || !bytes) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    *dev_ptr = idx->blob;
    *bytes = idx->h.blob_bytes;
    return SBWTGPU_OK;
}

int sbwtgpu_index_copy_blob(const sbwtgpu_index *idx, void *dst_dev, int64_t bytes, void *stream) {
    if (!idx || !dst_dev) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    if (bytes != idx->h.blob_bytes) return fail(SBWTGPU_ERR_INVALID_ARG, "bytes must equal blob_bytes");
    DeviceGuard guard(idx->device);
    HIP_TRY(hipMemcpyAsync(dst_dev, idx->blob, (size_t)bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return SBWTGPU_OK;
}

int sbwtgpu_index_adopt(const void *header, int64_t header_bytes, void *dev_blob, int64_t blob_bytes, int device,
                        sbwtgpu_index **out) {
    if (!header || !dev_blob || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    if (header_bytes != (int64_t)sizeof(SbwtBlobHeader)) return fail(SBWTGPU_ERR_INVALID_ARG, "bad header size");
    SbwtBlobHeader h;
    memcpy(&h, header, sizeof(h));
    if (h.magic != SBWT_BLOB_MAGIC) return fail(SBWTGPU_ERR_INVALID_ARG, "bad header magic");
    if (h.blob_bytes != blob_bytes) return fail(SBWTGPU_ERR_INVALID_ARG, "blob size does not match its header");
    if (((uintptr_t)dev_blob & 255) != 0) return fail(SBWTGPU_ERR_INVALID_ARG, "the device image must be 256-byte aligned");
    sbwtgpu_index *idx = new (std::nothrow) sbwtgpu_index();
    if (!idx) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    idx->h = h;
    idx->device = device;
    idx->blob = static_cast<char *>(dev_blob);
    idx->owns_blob = false;
    *out = idx;
    return SBWTGPU_OK;
}

// RCCL is loaded lazily so that single-GPU use never needs it.
// devs[] may name a device more than once (several host threads per GPU): the image travels once per DISTINCT
// device and the duplicates share that device's handle.
// The plan of a replication, without touching any device (so that a box without GPUs can test it): the DISTINCT devices of
// devs[] in order of first appearance (uniq_out, n_dev entries of room), slot_out[i] = the index of devs[i] among them, and
// the root device's index (= its rank in the RCCL group, whose ranks are the distinct devices in that order).
int sbwtgpu_debug_bcast_plan(int n_dev, const int *devs, int root_device, int n_visible, int *uniq_out, int *slot_out, int *n_uniq,
                             int *root_rank) {
    if (n_dev <= 0 || !devs || !uniq_out || !slot_out || !n_uniq || !root_rank) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL/empty argument");
    int nu = 0;
    for (int i = 0; i < n_dev; i++) {
        if (devs[i] < 0 || devs[i] >= n_visible) return fail(SBWTGPU_ERR_NO_DEVICE, "device %d out of range", devs[i]);
        int u = 0;
        while (u < nu && uniq_out[u] != devs[i]) u++;
        if (u == nu) uniq_out[nu++] = devs[i];
        slot_out[i] = u;
    }
    *n_uniq = nu;
    *root_rank = -1;
    for (int u = 0; u < nu; u++)
        if (uniq_out[u] == root_device) *root_rank = u;
    if (*root_rank < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "the root's device must be in devs[]");
    return SBWTGPU_OK;
}

int sbwtgpu_index_bcast(sbwtgpu_index *root, int n_dev, const int *devs, sbwtgpu_index **out) {
    if (!root || n_dev <= 0 || !devs || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL/empty argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) ndev = 0;
    std::vector<int> uniq((size_t)n_dev, 0);            // distinct devices, in order of first appearance
    std::vector<int> slot((size_t)n_dev, 0);            // devs[i] -> its index in uniq
    int n_uniq = 0, root_rank = -1;
    {
        const int prc = sbwtgpu_debug_bcast_plan(n_dev, devs, root->device, ndev, uniq.data(), slot.data(), &n_uniq, &root_rank);
        if (prc != SBWTGPU_OK) return prc;
    }
    // SBWTGPU_BCAST_NO_DEDUP=1 (tests): every entry of devs[] is a rank of its own, duplicates included -- the RCCL call
    // sequence below then runs on a one-GPU box (with a stand-in library behind SBWTGPU_RCCL_LIB: RCCL itself refuses two
    // ranks on one device); the root's rank is its device's first entry
    const char *nd_env = getenv("SBWTGPU_BCAST_NO_DEDUP");
    if (nd_env && *nd_env == '1' && n_dev > 1) {
        n_uniq = n_dev;
        root_rank = -1;
        for (int i = 0; i < n_dev; i++) {
            uniq[(size_t)i] = devs[i];
            slot[(size_t)i] = i;
            if (root_rank < 0 && devs[i] == root->device) root_rank = i;
        }
    }
    uniq.resize((size_t)n_uniq);
    if (uniq.size() == 1) {
        for (int i = 0; i < n_dev; i++) out[i] = root;
        return SBWTGPU_OK;
    }
    typedef void *comm_t;
    typedef int (*init_all_t)(comm_t *, int, const int *);
    typedef int (*bcast_t)(const void *, void *, size_t, int, int, comm_t, hipStream_t);
    typedef int (*grp_t)(void);
    typedef int (*destroy_t)(comm_t);
    // (SBWTGPU_RCCL_LIB names another library with RCCL's five entry points: a site's own build, or a stand-in for tests)
    const char *rccl_name = getenv("SBWTGPU_RCCL_LIB");
    void *lib = (rccl_name && *rccl_name) ? dlopen(rccl_name, RTLD_NOW | RTLD_GLOBAL) : dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib && !(rccl_name && *rccl_name)) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return fail(SBWTGPU_ERR_HIP, "cannot load librccl.so: %s", dlerror());
    init_all_t init_all = (init_all_t)dlsym(lib, "ncclCommInitAll");
    bcast_t bcast = (bcast_t)dlsym(lib, "ncclBroadcast");
    grp_t gstart = (grp_t)dlsym(lib, "ncclGroupStart"), gend = (grp_t)dlsym(lib, "ncclGroupEnd");
    destroy_t destroy = (destroy_t)dlsym(lib, "ncclCommDestroy");
    if (!init_all || !bcast || !gstart || !gend || !destroy) {
        dlclose(lib);
        return fail(SBWTGPU_ERR_HIP, "RCCL symbols missing");
    }
    const int nu = (int)uniq.size();
    std::vector<comm_t> comms((size_t)nu, nullptr);
    std::vector<hipStream_t> streams((size_t)nu, nullptr);
    std::vector<char> have_stream((size_t)nu, 0);
    std::vector<sbwtgpu_index *> made((size_t)nu, nullptr);
    bool have_comms = false;
    int rc = SBWTGPU_OK;
    for (int u = 0; u < nu && rc == SBWTGPU_OK; u++) {
        if (hipSetDevice(uniq[u]) != hipSuccess || hipStreamCreate(&streams[u]) != hipSuccess) {
            rc = fail(SBWTGPU_ERR_HIP, "cannot set up device %d", uniq[u]);
            break;
        }
        have_stream[u] = 1;
        if (u != root_rank) {
            sbwtgpu_index *c = new (std::nothrow) sbwtgpu_index();
            if (!c || hipMalloc((void **)&c->blob, (size_t)root->h.blob_bytes) != hipSuccess) {
                delete c;
                rc = fail(SBWTGPU_ERR_OOM, "hipMalloc on device %d", uniq[u]);
                break;
            }
            c->h = root->h;
            c->device = uniq[u];
            made[u] = c;
        }
    }
    if (rc == SBWTGPU_OK) {
        if (init_all(comms.data(), nu, uniq.data()) != 0) rc = fail(SBWTGPU_ERR_HIP, "ncclCommInitAll failed");
        else have_comms = true;
    }
    if (rc == SBWTGPU_OK) {
        gstart();
        for (int u = 0; u < nu; u++) {
            (void)hipSetDevice(uniq[u]);
            void *buf = (u == root_rank) ? (void *)root->blob : (void *)made[u]->blob;
            if (bcast(buf, buf, (size_t)root->h.blob_bytes, /*ncclChar*/ 0, root_rank, comms[u], streams[u]) != 0)
                rc = fail(SBWTGPU_ERR_HIP, "ncclBroadcast failed");
        }
        if (gend() != 0 && rc == SBWTGPU_OK) rc = fail(SBWTGPU_ERR_HIP, "ncclGroupEnd failed");
        for (int u = 0; u < nu; u++) {
            (void)hipSetDevice(uniq[u]);
            if (hipStreamSynchronize(streams[u]) != hipSuccess && rc == SBWTGPU_OK)
                rc = fail(SBWTGPU_ERR_HIP, "broadcast to device %d failed", uniq[u]);
        }
    }
    for (int u = 0; u < nu; u++) {                       // only what was actually created
        if (!have_stream[u] && !have_comms) continue;
        (void)hipSetDevice(uniq[u]);
        if (have_comms) destroy(comms[u]);
        if (have_stream[u]) (void)hipStreamDestroy(streams[u]);
    }
    (void)hipSetDevice(root->device);
    if (rc != SBWTGPU_OK) {
        for (auto *c : made) sbwtgpu_index_destroy(c);
        dlclose(lib);
        return rc;
    }
    // success: librccl stays loaded for the life of the process (it keeps per-process state)
    for (int i = 0; i < n_dev; i++) out[i] = (slot[(size_t)i] == root_rank) ? root : made[(size_t)slot[(size_t)i]];
    return SBWTGPU_OK;
}

// ---- device-pointer entry points -----------------------------------------------------------
// Workspace = header | packed bases (16 bytes per 32 bases) | with "sort_reads" = 1, room to sort the reads by their place
// in the path order (sbwt_sort.hip): four 32-bit arrays of one entry per read + the radix sort's own temporary, sized
// for reads of >= 32 bases on average (a batch of shorter reads is searched unsorted).
static inline int64_t ws_packed_bytes(int64_t total_bases) {
    // + 2 groups that the encoder zero-fills (windows that run past the last base) + 2 that are only ever loaded (the
    // search kernel fetches the packed groups of a read ahead of their use, three at a time)
    const int64_t groups = (total_bases + SBWT_GROUP_BASES - 1) / SBWT_GROUP_BASES + 4;
    return (int64_t)sizeof(SbwtWorkHeader) + groups * 16;
}
static inline int64_t ws_sort_capacity(int64_t total_bases) {      // only when sorting is switched on ("sort_reads" = 1)
    return g_sort_reads > 0 ? total_bases / 32 + 4096 : 0;
}
// the fused route's list of reads handed on to the general kernel: one 32-bit entry per read, reads of >= 32 bases
static inline int64_t ws_defer_bytes(int64_t total_bases) { return align256(total_bases / 8 + 256); }
// the pieces of long reads (SbwtPieceTab, sbwt_device.h): two 16-byte entries per zone.  Zones of 128 k-mers while that
// makes at most 2^18 of them (a few genomes as single reads then fill the chip), doubling up to SBWT_PIECE beyond.
static inline int ws_piece_len(int64_t total_bases) {
    int piece = 128;
    while (piece < SBWT_PIECE && total_bases / piece > ((int64_t)1 << 18)) piece *= 2;
    return piece;
}
// (entries: non-decreasing in total_bases -- a workspace sized for a large batch serves every smaller one)
static inline int64_t ws_piece_cap(int64_t total_bases) {
    return std::max<int64_t>(total_bases / SBWT_PIECE, std::min<int64_t>(total_bases / 128, (int64_t)1 << 18)) + 2;
}
static inline int64_t ws_piece_bytes(int64_t total_bases) { return align256(ws_piece_cap(total_bases) * 32); }
// the fused route's ticket table (SbwtTickTab, round 6): one ticket per 64 bases of the batch at most (a batch of long reads has
// one per 98 .. 144 bases; a batch that would need more goes the general route), 16 + 4 bytes each, and one bit per read of the
// list of reads handed on (one read per 32 bases, like that list)
static inline int64_t ws_tick_cap(int64_t total_bases) { return total_bases / 64 + 64; }
static inline int64_t ws_tick_bytes(int64_t total_bases) {
    return align256(ws_tick_cap(total_bases) * 16) + align256(ws_tick_cap(total_bases) * 4) + align256(total_bases / 256 + 64);
}
static inline int64_t ws_fixed_bytes(int64_t total_bases) {
    return align256(ws_packed_bytes(total_bases)) + ws_defer_bytes(total_bases) + ws_piece_bytes(total_bases) + ws_tick_bytes(total_bases);
}
int64_t sbwtgpu_search_workspace_bytes(int64_t total_bases) {
    if (total_bases < 0) total_bases = 0;
    const int64_t n_cap = ws_sort_capacity(total_bases);
    return ws_fixed_bytes(total_bases) + (n_cap ? 32 * n_cap + ((int64_t)16 << 20) : 0);
}
static SbwtPieceTab ws_piece_tab(void *d_ws, int64_t total_bases) {
    SbwtPieceTab pt;
    if (!g_split_long) return pt;
    char *base = static_cast<char *>(d_ws) + align256(ws_packed_bytes(total_bases)) + ws_defer_bytes(total_bases);
    pt.cap = ws_piece_cap(total_bases);
    pt.piece = ws_piece_len(total_bases);
    pt.pairs = reinterpret_cast<uint4 *>(base);
    pt.outs = pt.pairs + pt.cap;
    return pt;
}

static SbwtTickTab ws_tick_tab(void *d_ws, int64_t total_bases) {
    SbwtTickTab tt;
    char *base = static_cast<char *>(d_ws) + align256(ws_packed_bytes(total_bases)) + ws_defer_bytes(total_bases) + ws_piece_bytes(total_bases);
    tt.cap = ws_tick_cap(total_bases);
    tt.tick = reinterpret_cast<uint4 *>(base);
    tt.tick_read = reinterpret_cast<unsigned *>(base + align256(tt.cap * 16));
    tt.defer_bits = reinterpret_cast<unsigned *>(base + align256(tt.cap * 16) + align256(tt.cap * 4));
    return tt;
}

static const char *RANK_ONLY_MSG =
    "the index columns are not a valid SBWT (set bits != n_nodes - 1): only rank() is available";

// SBWT::search through streaming steps on the device (the marks given with the index, or derived): exact where a streaming step
// and a full search agree on every k-mer of valid bases (tests/test_large.hh:104-115).  Not for k = 1: there every column is in
// the root's suffix group while the edges sit on the first k-mer's column (NodeBOSSInMemoryConstructor.hh:98-154), so the
// reference's own streaming_search misses every second 1-mer that search() finds (round 5, tests/test_gpu_corners.py).
static bool internal_streaming_ok(const SbwtBlobHeader &h) {
    return (h.has_ssup || h.ssup_derived) && g_derive_ssup && h.k >= 2;
}

static int search_dev_check(const sbwtgpu_index *idx, int64_t total_bases, int64_t n_reads, const void *d_ws,
                            int64_t ws_bytes, int streaming) {
    if (!idx) return fail(SBWTGPU_ERR_INVALID_ARG, "idx is NULL");
    if (idx->h.rank_only) return fail(SBWTGPU_ERR_INVALID_ARG, "%s", RANK_ONLY_MSG);
    if (streaming && !idx->h.has_ssup)
        return fail(SBWTGPU_ERR_NO_STREAMING, "Error: streaming search support not built");
    if (n_reads < 0 || total_bases < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative size");
    if (total_bases >= ((int64_t)1 << 36))
        return fail(SBWTGPU_ERR_INVALID_ARG, "more than 2^36 bases in one call: split the batch");
    if (!d_ws) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL workspace");
    if (ws_bytes < sbwtgpu_search_workspace_bytes(total_bases))
        return fail(SBWTGPU_ERR_INVALID_ARG, "workspace too small (%lld < %lld)", (long long)ws_bytes,
                    (long long)sbwtgpu_search_workspace_bytes(total_bases));
    if (((uintptr_t)d_ws & 15) != 0) return fail(SBWTGPU_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
    return SBWTGPU_OK;
}

int sbwtgpu_encode_bases_dev(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases, void *d_ws,
                             int64_t ws_bytes, void *stream) {
    int rc = search_dev_check(idx, total_bases, 0, d_ws, ws_bytes, 0);
    if (rc != SBWTGPU_OK) return rc;
    if (total_bases > 0 && !d_bases) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL device pointer");
    DeviceGuard guard(idx->device);
    SbwtWorkHeader *ws = static_cast<SbwtWorkHeader *>(d_ws);
    uint4 *packed = reinterpret_cast<uint4 *>(static_cast<char *>(d_ws) + sizeof(SbwtWorkHeader));
    sbwt_launch_encode(d_bases, total_bases, packed, ws, static_cast<hipStream_t>(stream));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return SBWTGPU_OK;
}

int sbwtgpu_search_encoded_dev(const sbwtgpu_index *idx, int64_t total_bases, const int64_t *d_read_off,
                               int64_t n_reads, int64_t *d_out, const int64_t *d_out_off, void *d_ws,
                               int64_t ws_bytes, int streaming, void *stream) {
    int rc = search_dev_check(idx, total_bases, n_reads, d_ws, ws_bytes, streaming);
    if (rc != SBWTGPU_OK) return rc;
    if (n_reads == 0) return SBWTGPU_OK;
    if (!d_read_off || !d_out_off) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL device pointer");
    DeviceGuard guard(idx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    SbwtWorkHeader *ws = static_cast<SbwtWorkHeader *>(d_ws);
    // the ticket counter and the work counters restart with every search launch
    hipError_t e = hipMemsetAsync(ws, 0, sizeof(SbwtWorkHeader), st);
    if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    const uint4 *packed = reinterpret_cast<const uint4 *>(static_cast<char *>(d_ws) + sizeof(SbwtWorkHeader));
    if (g_poison && n_reads > 0) {
        int64_t ends[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(&ends[0], d_out_off, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&ends[1], d_out_off + n_reads, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (ends[1] > ends[0]) {
                    const size_t vb = t_out32 ? 4 : 8;
                    HIP_TRY(hipMemsetAsync(reinterpret_cast<char *>(d_out) + (size_t)ends[0] * vb, 0xA5, (size_t)(ends[1] - ends[0]) * vb, st));
                }
    }
    // kernel: an explicit choice ("search_variant" / SBWTGPU_SEARCH_VARIANT), else by the index: the segment-list writer
    // where reads follow their paths for long (fewer than one column in 64 offers a choice of successors: config 2 has one
    // in 107, config 5 one in 586), the staged writer on branchy indexes (the star pan-genome of config 3: one in 31 --
    // its reads leave their path every 3-4 k-mers, and short segments fill the lists: 146.4 vs 143.8 ms)
    int variant = g_variant_override >= 0 ? g_variant_override : tuning_variant();
    if (variant < 0) variant = idx->h.has_path ? auto_variant(idx->h) : 2;
    if (variant == 5 || variant == 2 || variant == 3) variant = 4;   // already-encoded bases: the general path kernel
    const int eff_streaming = (!streaming && internal_streaming_ok(idx->h)) ? 2 : streaming;
    // reads sorted by their place in the path order (sbwt_sort.hip): when the batch covers the index a few times
    void *sort_scratch = nullptr;
    long long sort_bytes = 0;
    int key_bits = 1;
    while (key_bits < 32 && ((int64_t)1 << key_bits) <= idx->h.n_nodes) key_bits++;
    const bool path_kernel = variant == 4 && idx->h.has_path && eff_streaming && idx->h.stab_pos &&
                             idx->h.n_nodes < ((int64_t)1 << 31) - 128 && n_reads < ((int64_t)1 << 31);
    // Off unless asked for ("sort_reads" = 1): the path order numbers its paths in column order, not along the genome, so
    // reads sorted by path position share lines only within one path (kernel 6.45 -> 6.16 ms on config 2) and the
    // pre-pass costs 0.7 ms; reads that arrive in genome order get the full effect (5.3 ms) without any pre-pass.
    const bool want_sort = path_kernel && g_sort_reads > 0;
    if (want_sort) {
        // the scratch lives in the caller's workspace, behind the packed bases (no allocation, nothing shared between calls)
        const int64_t off = ws_fixed_bytes(total_bases);
        sort_bytes = sbwt_sort_scratch_bytes(n_reads, key_bits);
        if (n_reads <= ws_sort_capacity(total_bases) && off + sort_bytes <= ws_bytes) sort_scratch = static_cast<char *>(d_ws) + off;
    }
    sbwt_launch_search(idx->view(), packed, reinterpret_cast<const long long *>(d_read_off),
                       reinterpret_cast<const long long *>(d_out_off), reinterpret_cast<long long *>(d_out), n_reads,
                       ws, eff_streaming, st, variant, total_bases / SBWT_GROUP_BASES + 2, sort_scratch, sort_bytes, key_bits,
                       ws_piece_tab(d_ws, total_bases));
    e = hipGetLastError();
    if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return SBWTGPU_OK;
}

// HIP events around the dominant kernel of the search calls ("kernel_events" = 1; bench.py's roofline leg): a ring of
// event pairs, so that a timed loop of launches needs no synchronisation in between
static const int EV_RING = 256;
static hipEvent_t g_ev[EV_RING][2];
static int g_ev_made = 0;

int sbwtgpu_kernel_times(double *ms, int64_t cap, int64_t *n) {
    if (!n || (cap > 0 && !ms)) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    const int64_t have = g_ev_count < EV_RING ? g_ev_count : EV_RING;
    const int64_t first = g_ev_count - have;
    int64_t w = 0;
    for (int64_t q = first; q < g_ev_count && w < cap; q++, w++) {
        hipEvent_t *e = g_ev[q % EV_RING];
        HIP_TRY(hipEventSynchronize(e[1]));
        float f = 0;
        HIP_TRY(hipEventElapsedTime(&f, e[0], e[1]));
        ms[w] = (double)f;
    }
    *n = w;
    return SBWTGPU_OK;
}

static int search_dev_common(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases,
                             const int64_t *d_read_off, int64_t n_reads, int64_t *d_out, const int64_t *d_out_off,
                             void *d_ws, int64_t ws_bytes, void *stream, int streaming) {
    int rc = search_dev_check(idx, total_bases, n_reads, d_ws, ws_bytes, streaming);
    if (rc != SBWTGPU_OK) return rc;
    if (n_reads == 0) return SBWTGPU_OK;
    {
        // The fused route (sbwt_search_fused.hip; "search_variant" 5, the default on a path-order index): no separate
        // encode pass.  It decides on the device whether the batch qualifies (reads of one length, 32 .. 160 bases) and
        // runs the general kernel behind the fused one for everything that does not.
        int variant = g_variant_override >= 0 ? g_variant_override : tuning_variant();
        if (variant < 0) variant = idx->h.has_path ? auto_variant(idx->h) : 2;
        const int eff_streaming = (!streaming && internal_streaming_ok(idx->h)) ? 2 : streaming;
        // (an image of 2^31 columns or more has a path order only in the form the fused kernel's BIG instantiation reads:
        // k <= 31, whole k-mers with their positions; int64 results -- the int32 calls refuse such an index)
        const bool big_image = idx->h.big_layout && idx->h.has_path && !t_out32 &&
                               ((idx->h.stab_pos && idx->h.p_sparse == idx->h.k) || (idx->h.n_sb2 > 0 && idx->h.k > idx->h.p_sparse));
        const bool path_kernel = idx->h.has_path && eff_streaming &&
                                 ((idx->h.n_nodes < ((int64_t)1 << 31) - 128 && !idx->h.big_layout) || big_image) && n_reads < ((int64_t)1 << 31) &&
                                 total_bases / SBWT_GROUP_BASES + 2 < ((int64_t)1 << 31) - 4;
        if (variant == 5 && path_kernel && g_sort_reads <= 0 && !(g_debug & 16)) {
            if (!d_read_off || !d_out_off) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL device pointer");
            if (total_bases > 0 && !d_bases) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL device pointer");
            DeviceGuard guard(idx->device);
            hipStream_t st = static_cast<hipStream_t>(stream);
            SbwtWorkHeader *ws = static_cast<SbwtWorkHeader *>(d_ws);
            // (all but the header's last word: the hint the call before left for this one, SbwtWorkHeader::hint -- the only
            // part of a workspace that is read before it is written)
            HIP_TRY(hipMemsetAsync(ws, 0, SBWT_WS_CLEAR_BYTES, st));
            if (g_poison) {
                int64_t ends[2] = {0, 0};
                HIP_TRY(hipMemcpyAsync(&ends[0], d_out_off, 8, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipMemcpyAsync(&ends[1], d_out_off + n_reads, 8, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                if (ends[1] > ends[0]) {
                    const size_t vb = t_out32 ? 4 : 8;
                    HIP_TRY(hipMemsetAsync(reinterpret_cast<char *>(d_out) + (size_t)ends[0] * vb, 0xA5, (size_t)(ends[1] - ends[0]) * vb, st));
                }
            }
            uint4 *packed = reinterpret_cast<uint4 *>(static_cast<char *>(d_ws) + sizeof(SbwtWorkHeader));
            unsigned *defer = reinterpret_cast<unsigned *>(static_cast<char *>(d_ws) + align256(ws_packed_bytes(total_bases)));
            const SbwtTickTab tt_of_call = ws_tick_tab(d_ws, total_bases);
            // (the bits of the reads handed on: cleared with the header)
            HIP_TRY(hipMemsetAsync(tt_of_call.defer_bits, 0, (size_t)(total_bases / 256 + 64), st));
            SbwtTickTab tt_for_launch = tt_of_call;
            if (!(g_fused_table && g_fused_ragged && n_reads <= total_bases / 32)) { tt_for_launch.tick = nullptr; tt_for_launch.tick_read = nullptr; }
            hipEvent_t e0 = nullptr, e1 = nullptr;
            if (g_kernel_events) {
                const int slot = (int)(g_ev_count % EV_RING);
                if (slot >= g_ev_made) {
                    HIP_TRY(hipEventCreate(&g_ev[slot][0]));
                    HIP_TRY(hipEventCreate(&g_ev[slot][1]));
                    g_ev_made = slot + 1;
                }
                e0 = g_ev[slot][0]; e1 = g_ev[slot][1];
                g_ev_count++;
            }
            sbwt_launch_search_fused(idx->view(), d_bases, total_bases, packed, reinterpret_cast<const long long *>(d_read_off),
                                     reinterpret_cast<const long long *>(d_out_off), reinterpret_cast<long long *>(d_out), n_reads,
                                     ws, eff_streaming, st, defer, e0, e1, ws_piece_tab(d_ws, total_bases),
                                     // (the list of reads handed on has one entry per 32 bases of the batch)
                                     ((g_fused_ragged && n_reads <= total_bases / 32) ? 1 : 0) |
                                         ((g_fused_pieces > 0 ? g_fused_pieces : 3) << 8),
                                     // (the ticket table of batches with many long reads; "fused_table" 0 switches it off)
                                     tt_for_launch);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
            return SBWTGPU_OK;
        }
    }
    rc = sbwtgpu_encode_bases_dev(idx, d_bases, total_bases, d_ws, ws_bytes, stream);
    if (rc != SBWTGPU_OK) return rc;
    return sbwtgpu_search_encoded_dev(idx, total_bases, d_read_off, n_reads, d_out, d_out_off, d_ws, ws_bytes,
                                      streaming, stream);
}

int sbwtgpu_streaming_search_dev(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases,
                                 const int64_t *d_read_off, int64_t n_reads, int64_t *d_out,
                                 const int64_t *d_out_off, void *d_ws, int64_t ws_bytes, void *stream) {
    return search_dev_common(idx, d_bases, total_bases, d_read_off, n_reads, d_out, d_out_off, d_ws, ws_bytes, stream,
                             1);
}

int sbwtgpu_search_dev(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                       int64_t n_reads, int64_t *d_out, const int64_t *d_out_off, void *d_ws, int64_t ws_bytes,
                       void *stream) {
    return search_dev_common(idx, d_bases, total_bases, d_read_off, n_reads, d_out, d_out_off, d_ws, ws_bytes, stream,
                             0);
}

// The same two calls with int32 results (result compaction): every kernel of the route writes 4 bytes per k-mer
// instead of 8 -- half the write requests of a launch, which are 40 % of its time.
static int search_dev_i32(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                          int64_t n_reads, int32_t *d_out, const int64_t *d_out_off, void *d_ws, int64_t ws_bytes, void *stream,
                          int streaming) {
    if (!idx) return fail(SBWTGPU_ERR_INVALID_ARG, "idx is NULL");
    if (idx->h.n_nodes >= ((int64_t)1 << 31))
        return fail(SBWTGPU_ERR_INVALID_ARG, "int32 results need an index of fewer than 2^31 columns (this one has %lld)",
                    (long long)idx->h.n_nodes);
    t_out32 = 1;
    const int rc = search_dev_common(idx, d_bases, total_bases, d_read_off, n_reads, reinterpret_cast<int64_t *>(d_out), d_out_off,
                                     d_ws, ws_bytes, stream, streaming);
    t_out32 = 0;
    return rc;
}
int sbwtgpu_streaming_search_dev_i32(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases,
                                     const int64_t *d_read_off, int64_t n_reads, int32_t *d_out, const int64_t *d_out_off,
                                     void *d_ws, int64_t ws_bytes, void *stream) {
    return search_dev_i32(idx, d_bases, total_bases, d_read_off, n_reads, d_out, d_out_off, d_ws, ws_bytes, stream, 1);
}
int sbwtgpu_search_dev_i32(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                           int64_t n_reads, int32_t *d_out, const int64_t *d_out_off, void *d_ws, int64_t ws_bytes,
                           void *stream) {
    return search_dev_i32(idx, d_bases, total_bases, d_read_off, n_reads, d_out, d_out_off, d_ws, ws_bytes, stream, 0);
}

int sbwtgpu_rank_dev(const sbwtgpu_index *idx, const int64_t *d_pos, const char *d_sym, int64_t n, int64_t *d_out,
                     void *stream) {
    if (!idx) return fail(SBWTGPU_ERR_INVALID_ARG, "idx is NULL");
    if (n < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative size");
    if (n == 0) return SBWTGPU_OK;
    if (!d_pos || !d_sym || !d_out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL device pointer");
    DeviceGuard guard(idx->device);
    sbwt_launch_rank(idx->view(), reinterpret_cast<const long long *>(d_pos), d_sym, n,
                     reinterpret_cast<long long *>(d_out), static_cast<hipStream_t>(stream));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return SBWTGPU_OK;
}

int sbwtgpu_workspace_status(const void *d_ws, void *stream, int *status) {
    if (!d_ws || !status) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    SbwtWorkHeader hdr;
    HIP_TRY(hipMemcpyAsync(&hdr, d_ws, sizeof(hdr), hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    *status = hdr.status;
    return SBWTGPU_OK;
}

int sbwtgpu_workspace_stats(const void *d_ws, void *stream, int64_t stats[8]) {
    if (!d_ws || !stats) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    SbwtWorkHeader hdr;
    HIP_TRY(hipMemcpyAsync(&hdr, d_ws, sizeof(hdr), hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    stats[0] = (int64_t)hdr.n_stream;
    stats[1] = (int64_t)hdr.n_search;
    stats[2] = (int64_t)hdr.n_lf;
    stats[3] = (int64_t)hdr.n_tab_hit;
    stats[4] = (int64_t)hdr.n_ext;
    stats[5] = (int64_t)hdr.n_bridge;
    stats[6] = stats[7] = 0;
    return SBWTGPU_OK;
}

// ---- host-buffer entry points --------------------------------------------------------------
}  // extern "C"
namespace {
struct Stream {
    hipStream_t s = nullptr;
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
};

// Small calls (the scalar API of the reference -- SBWT::search(kmer), rank(pos, c), one update_sbwt_interval -- arrives
// here as batches of one): no hipMalloc / hipStreamCreate per call.  Every host thread keeps, per device, one stream,
// one pinned host buffer and one device buffer of SLOT_CAP bytes; a call whose data fits stages its inputs in the pinned
// buffer, moves them with ONE H2D copy, runs its kernels, and brings the results back with ONE D2H copy + one sync.
constexpr size_t SLOT_CAP = (size_t)1 << 20;
bool g_exiting = false;                                  // set at process exit: HIP may be gone, leak instead of freeing
struct SmallSlot {
    int device = -1;
    hipStream_t stream = nullptr;
    char *host = nullptr, *dev = nullptr;
    void release() {
        if (device < 0 || g_exiting) return;
        DeviceGuard guard(device);
        if (stream) (void)hipStreamDestroy(stream);
        if (host) (void)hipHostFree(host);
        if (dev) (void)hipFree(dev);
        stream = nullptr; host = dev = nullptr; device = -1;
    }
};
struct SlotSet {
    std::vector<SmallSlot> v;
    ~SlotSet() { for (auto &s : v) s.release(); }
};
thread_local SlotSet t_slots;
// The calling thread's slot on `device` (the current device must already be `device`), or nullptr when `need` does not
// fit or the buffers cannot be allocated (the caller then takes the general path).
SmallSlot *small_slot(int device, size_t need) {
    if (need > SLOT_CAP) return nullptr;
    static const bool once = [] { atexit([] { g_exiting = true; }); return true; }();
    (void)once;
    for (auto &s : t_slots.v)
        if (s.device == device) return &s;
    SmallSlot s;
    if (hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (hipHostMalloc((void **)&s.host, SLOT_CAP, hipHostMallocDefault) != hipSuccess ||
        hipMalloc((void **)&s.dev, SLOT_CAP) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamDestroy(s.stream);
        if (s.host) (void)hipHostFree(s.host);
        return nullptr;
    }
    s.device = device;
    t_slots.v.push_back(s);
    return &t_slots.v.back();
}

// One host-buffer call that is not pipelined: the caller lays its inputs, results and workspace out in one range of
// `bytes` bytes (every part 256-byte aligned) and names the parts by their offsets.  A call that fits SLOT_CAP runs on the
// thread's SmallSlot: in() copies into the pinned buffer, upload() is the ONE H2D copy, finish() the ONE D2H copy, the
// ONE synchronise and the copies out to the caller.  A larger call gets a temporary stream and one device allocation,
// and in() / out() copy straight between the caller's memory and the device: no host-side bounce.
struct Staging {
    std::vector<std::vector<int64_t>> kept;     // large calls: computed inputs, alive until the synchronise
    Stream tmp_stream;
    DevBuf tmp_dev;
    SmallSlot *sl = nullptr;
    char *dev = nullptr;
    hipStream_t stream = nullptr;
    size_t in_lo = SIZE_MAX, in_hi = 0, out_lo = SIZE_MAX, out_hi = 0;    // slot: the byte ranges of the two copies
    struct Back { void *dst; size_t off, n; } back[4];
    int n_back = 0;

    int open(int device, size_t bytes) {       // (the current device must already be `device`)
        sl = small_slot(device, bytes);
        if (sl) { dev = sl->dev; stream = sl->stream; return SBWTGPU_OK; }
        HIP_TRY(hipStreamCreateWithFlags(&tmp_stream.s, hipStreamNonBlocking));
        HIP_TRY(tmp_dev.alloc(bytes));
        dev = static_cast<char *>(tmp_dev.p);
        stream = tmp_stream.s;
        return SBWTGPU_OK;
    }
    template <typename T>
    T *at(size_t off) const { return reinterpret_cast<T *>(dev + off); }
    // n bytes of the caller's at src are the input at `off`
    int in(size_t off, const void *src, size_t n) {
        if (n == 0) return SBWTGPU_OK;
        if (!sl) {
            HIP_TRY(hipMemcpyAsync(dev + off, src, n, hipMemcpyHostToDevice, stream));
            return SBWTGPU_OK;
        }
        if (src != sl->host + off) memcpy(sl->host + off, src, n);
        in_lo = std::min(in_lo, off);
        in_hi = std::max(in_hi, off + n);
        return SBWTGPU_OK;
    }
    // the input at `off` is the n offsets src[0 .. n) rebased to start at 0 (device buffers start at their first base)
    int in_rebased(size_t off, const int64_t *src, int64_t n) {
        int64_t *o = nullptr;
        if (sl) {
            o = reinterpret_cast<int64_t *>(sl->host + off);
        } else {
            try {
                kept.emplace_back((size_t)n);
            } catch (const std::bad_alloc &) {
                return fail(SBWTGPU_ERR_OOM, "out of host memory");
            }
            o = kept.back().data();
        }
        for (int64_t t = 0; t < n; t++) o[t] = src[t] - src[0];
        return in(off, o, (size_t)n * 8);
    }
    int upload() {
        if (sl && in_hi > in_lo) HIP_TRY(hipMemcpyAsync(dev + in_lo, sl->host + in_lo, in_hi - in_lo, hipMemcpyHostToDevice, stream));
        return SBWTGPU_OK;
    }
    // after the kernels: the n bytes at `off` are a result and go to dst (written by the time finish() returns)
    int out(size_t off, void *dst, size_t n) {
        if (n == 0) return SBWTGPU_OK;
        if (!sl) {
            HIP_TRY(hipMemcpyAsync(dst, dev + off, n, hipMemcpyDeviceToHost, stream));
            return SBWTGPU_OK;
        }
        if (n_back == (int)(sizeof(back) / sizeof(back[0]))) return fail(SBWTGPU_ERR_HIP, "internal: too many results in one staged call");
        back[n_back++] = Back{dst, off, n};
        out_lo = std::min(out_lo, off);
        out_hi = std::max(out_hi, off + n);
        return SBWTGPU_OK;
    }
    int finish() {
        if (sl && out_hi > out_lo) HIP_TRY(hipMemcpyAsync(sl->host + out_lo, dev + out_lo, out_hi - out_lo, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        for (int i = 0; i < n_back; i++) memcpy(back[i].dst, sl->host + back[i].off, back[i].n);
        return SBWTGPU_OK;
    }
};
#define STG_TRY(expr)                                                                          \
    do {                                                                                       \
        const int rc_ = (expr);                                                                \
        if (rc_ != SBWTGPU_OK) return rc_;                                                     \
    } while (0)
}  // namespace
extern "C" {

// The length of read r as every host entry point checks it while it walks the offsets: not negative, below 2^31
static inline int check_read_length(const int64_t *read_off, int64_t r) {
    const int64_t len = read_off[r + 1] - read_off[r];
    if (len < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "read_off is not non-decreasing at read %lld", (long long)r);
    if (len >= ((int64_t)1 << 31)) return fail(SBWTGPU_ERR_READ_TOO_LONG, "read %lld has >= 2^31 bases", (long long)r);
    return SBWTGPU_OK;
}

// (*any_long: some read has more than 2 * PIECE k-mers -- the host entry points cut those into pieces, below)
static int check_reads(const int64_t *read_off, const int64_t *out_off, int64_t n_reads, int64_t k, bool *any_long = nullptr) {
    int64_t longest = 0;
    for (int64_t r = 0; r < n_reads; r++) {
        const int rc = check_read_length(read_off, r);
        if (rc != SBWTGPU_OK) return rc;
        int64_t m = read_off[r + 1] - read_off[r] - k + 1;
        if (m < 0) m = 0;
        if (out_off[r + 1] - out_off[r] != m)
            return fail(SBWTGPU_ERR_INVALID_ARG, "out_off[%lld+1]-out_off[%lld] must be max(0,len-k+1) = %lld",
                        (long long)r, (long long)r, (long long)m);
        if (m > longest) longest = m;
    }
    if (any_long) *any_long = longest > 4096;          // = 2 * PIECE
    return SBWTGPU_OK;
}


// ---- long reads -----------------------------------------------------------------------------------
// One lane walks one read, so a single very long query (a genome as one FASTA record) would keep one
// lane busy for millions of steps.  The host entry points therefore cut reads longer than 2*PIECE
// k-mers into pieces of about PIECE k-mers that overlap by k-1 bases and hand the pieces to the kernel
// as reads of their own; their result ranges tile the read's range, so nothing else changes.  This is
// exact: a piece starts at a k-mer whose window holds no lower-case acgt, and for such a k-mer the
// reference's result does not depend on what came before (streaming step and full search agree,
// tests/test_large.hh:104-115; only lower-case input makes the two differ).
static const int64_t PIECE = 2048;
static_assert(2 * PIECE == 4096, "check_reads flags reads of more than 4096 k-mers");

static inline bool window_has_lower(const char *s, int64_t k) {
    for (int64_t t = 0; t < k; t++) {
        char ch = s[t];
        if (ch == 'a' || ch == 'c' || ch == 'g' || ch == 't') return true;
    }
    return false;
}
// Appends the pieces of read `s` (len bases) to (dst bases, roff, ooff); dst may be NULL to count only.
// Returns the number of bytes appended.
static int64_t append_pieces(const char *s, int64_t len, int64_t k, char *dst, std::vector<int64_t> &roff,
                             std::vector<int64_t> &ooff) {
    const int64_t m = len - k + 1;
    int64_t written = 0;
    if (m <= 2 * PIECE) {
        if (dst && len > 0) memcpy(dst, s, (size_t)len);
        roff.push_back(roff.back() + len);
        ooff.push_back(ooff.back() + (m > 0 ? m : 0));
        return len;
    }
    int64_t start = 0;
    while (start < m) {
        int64_t next = start + PIECE;
        if (m - next < PIECE) next = m;                              // no tiny tail piece
        while (next < m && window_has_lower(s + next, k)) next++;    // a history-independent split point
        const int64_t nb = (next - start) + k - 1;
        if (dst) memcpy(dst + written, s + start, (size_t)nb);
        written += nb;
        roff.push_back(roff.back() + nb);
        ooff.push_back(ooff.back() + (next - start));
        start = next;
    }
    return written;
}
static inline int64_t pieces_bases_bound(int64_t len, int64_t k) {   // bytes append_pieces can write for a read
    const int64_t m = len - k + 1;
    if (m <= 2 * PIECE) return len > 0 ? len : 0;
    return len + (m / PIECE + 2) * (k - 1);
}

// ---- large host batches: chunks pipelined over two streams ------------------------------------------------------
// A batch whose results exceed PIPE_MIN bytes is cut into chunks of reads; chunk c+1's bases go up and its kernels run
// while chunk c's results come down (H2D and D2H use different DMA engines, the kernels are ~30x faster than either).
// Buffers of the caller that are pinned (hipHostMalloc / hipHostRegister / torch pin_memory: hipPointerGetAttributes says
// so) are the DMA's source and target themselves; pageable ones go through pinned staging buffers, copied by a few host
// threads.  The rate is then PCIe's: 8 bytes of results per k-mer.
}  // extern "C"
namespace {
// One slot of a pipeline: a stream, pinned staging buffers for what goes down and what comes back, a pinned status word
// and one device allocation, which the entry point carves for its chunk.  Pinned and device buffers are expensive to
// create (page pinning), so finished calls park their slots and later calls on the same device take them again, whichever
// entry point parked them; ensure() grows only what is too small for the taker.
struct PipeSlot {
    hipStream_t st = nullptr;
    char *h_in = nullptr, *h_out = nullptr;     // pinned staging: inputs; results (search: only for pageable callers)
    int *h_status = nullptr;                    // pinned, 64 bytes: the chunk's device status (text: and its text length)
    char *d_mem = nullptr;
    int64_t cap_in = 0, cap_out = 0, cap_dev = 0;
    hipError_t ensure(int64_t need_in, int64_t need_out, int64_t need_dev) {
        hipError_t e = hipSuccess;
        if (!st) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        if (e == hipSuccess && !h_status) e = hipHostMalloc((void **)&h_status, 64, hipHostMallocDefault);
        auto grow = [&e](char *&p, int64_t &cap, int64_t need, bool device) {
            if (e != hipSuccess || cap >= need) return;
            if (p) (void)(device ? hipFree(p) : hipHostFree(p));
            p = nullptr; cap = 0;
            e = device ? hipMalloc((void **)&p, (size_t)need) : hipHostMalloc((void **)&p, (size_t)need, hipHostMallocDefault);
            if (e == hipSuccess) cap = need;
        };
        grow(h_in, cap_in, need_in, false);
        grow(h_out, cap_out, need_out, false);
        grow(d_mem, cap_dev, need_dev, true);
        return e;
    }
    void release() {
        if (st) (void)hipStreamDestroy(st);
        if (h_in) (void)hipHostFree(h_in);
        if (h_out) (void)hipHostFree(h_out);
        if (h_status) (void)hipHostFree(h_status);
        if (d_mem) (void)hipFree(d_mem);
        *this = PipeSlot();
    }
};
std::mutex g_park_mutex;
struct Parked { int device; PipeSlot slot; };
std::vector<Parked> g_parked;
const size_t PARK_CAP = 8;                      // parked slots per device; a call that finishes beyond it frees its slots

// n slots for a call on `device` (the current device), each grown to the call's needs: parked ones first, the most
// recently parked first.  On failure nothing is left allocated.
int take_slots(int device, PipeSlot *S, int n, int64_t need_in, int64_t need_out, int64_t need_dev, const char *what) {
    {
        std::lock_guard<std::mutex> lock(g_park_mutex);
        int got = 0;
        for (size_t i = g_parked.size(); i-- > 0 && got < n;)
            if (g_parked[i].device == device) {
                S[got++] = g_parked[i].slot;
                g_parked.erase(g_parked.begin() + (long)i);
            }
    }
    for (int q = 0; q < n; q++) {
        const hipError_t e = S[q].ensure(need_in, need_out, need_dev);
        if (e == hipSuccess) continue;
        (void)hipGetLastError();
        for (int r = 0; r < n; r++) S[r].release();
        return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    }
    return SBWTGPU_OK;
}
// The end of a call on its slots: parked for the next one, or, after an error, freed once the device is idle.
void park_slots(int device, PipeSlot *S, int n, int rc) {
    if (rc != SBWTGPU_OK) (void)hipDeviceSynchronize();
    std::lock_guard<std::mutex> lock(g_park_mutex);
    size_t there = 0;
    for (const Parked &p : g_parked) there += p.device == device;
    for (int q = 0; q < n; q++) {
        if (rc == SBWTGPU_OK && there < PARK_CAP) { g_parked.push_back(Parked{device, S[q]}); there++; S[q] = PipeSlot(); }
        else S[q].release();
    }
}
// Two chunks in flight: chunk c is submitted once chunk c - 2 has been collected from the slot it takes
template <typename Submit, typename Collect>
int two_in_flight(int64_t n_chunks, Submit submit, Collect collect) {
    int rc = SBWTGPU_OK;
    for (int64_t c = 0; c < n_chunks && rc == SBWTGPU_OK; c++) {
        if (c >= 2) rc = collect(c - 2);
        if (rc == SBWTGPU_OK) rc = submit(c);
    }
    for (int64_t c = std::max<int64_t>(0, n_chunks - 2); c < n_chunks && rc == SBWTGPU_OK; c++) rc = collect(c);
    return rc;
}
bool is_pinned(const void *p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}
void parallel_memcpy(char *dst, const char *src, size_t n) {
    const int T = n >= ((size_t)8 << 20) ? 4 : 1;
    if (T == 1) { memcpy(dst, src, n); return; }
    std::vector<std::thread> th;
    const size_t per = (n / T + 4095) & ~(size_t)4095;
    for (int t = 0; t < T; t++) {
        const size_t lo = std::min(n, per * (size_t)t), hi = std::min(n, lo + per);
        if (hi > lo) th.emplace_back([=] { memcpy(dst + lo, src + lo, hi - lo); });
    }
    for (auto &x : th) x.join();
}
const int64_t PIPE_MIN = (int64_t)64 << 20;
}  // namespace
extern "C" {

// ro / oo: nv + 1 offsets into src_bases / out (rebased to 0 or not: only ro[0], oo[0] and differences are used)
// out32 != nullptr (and out == nullptr): the kernels write int32 results (SbwtIndexView::out32): half the bytes over PCIe
static int search_host_pipelined(const sbwtgpu_index *idx, const char *src_bases, const int64_t *ro, const int64_t *oo,
                                 int64_t nv, int64_t *out, int streaming, int32_t *out32 = nullptr) {
    const int64_t vb = out32 ? 4 : 8;                   // bytes of a result on its way to the host
    const bool pin_in = is_pinned(src_bases), pin_out = is_pinned(out32 ? (const void *)out32 : (const void *)out);
    // chunks: results <= 512 MiB when they land in the caller's pinned memory, <= 128 MiB when they are staged
    static const int64_t chunk_mb = env_i64("SBWTGPU_PIPE_CHUNK_MB", 0);
    const int64_t CH_OUT = (chunk_mb > 0 ? chunk_mb : (pin_out ? (int64_t)512 : (int64_t)128)) << 20;
    std::vector<int64_t> cuts{0};
    int64_t max_bases = 0, max_reads = 0, max_vals = 0;
    for (int64_t lo = 0; lo < nv;) {
        int64_t hi = lo + 1;
        // (offsets are non-decreasing: bisect for the last read whose results still fit)
        int64_t a = lo + 1, b = nv;
        while (a < b) {
            const int64_t mid = a + (b - a + 1) / 2;
            if ((oo[mid] - oo[lo]) * vb <= CH_OUT && ro[mid] - ro[lo] <= ((int64_t)1 << 30)) a = mid; else b = mid - 1;
        }
        hi = a;
        cuts.push_back(hi);
        max_bases = std::max(max_bases, ro[hi] - ro[lo]);
        max_reads = std::max(max_reads, hi - lo);
        max_vals = std::max(max_vals, oo[hi] - oo[lo]);
        lo = hi;
    }
    const int64_t n_chunks = (int64_t)cuts.size() - 1;
    const int64_t ws_bytes = sbwtgpu_search_workspace_bytes(max_bases);
    const int64_t need_in = align256(max_bases + 16) + 2 * align256((max_reads + 1) * 8);
    const int64_t need_out = pin_out ? 0 : align256(max_vals * vb + 8);
    const int64_t need_dev = align256(max_bases + 16) + 2 * align256((max_reads + 1) * 8) + align256(max_vals * 8 + 8) + align256(ws_bytes);
    DeviceGuard guard(idx->device);
    PipeSlot S[2];
    int rc = take_slots(idx->device, S, 2, need_in, need_out, need_dev, "pipeline buffers");
    if (rc != SBWTGPU_OK) return rc;
    int bug = 0;                    // the first nonzero device status of a chunk
    struct Carve { char *bases; int64_t *roff, *ooff, *out; char *ws; };
    auto carve = [&](PipeSlot &P) {
        Carve c;
        char *p = P.d_mem;
        c.bases = p; p += align256(max_bases + 16);
        c.roff = (int64_t *)p; p += align256((max_reads + 1) * 8);
        c.ooff = (int64_t *)p; p += align256((max_reads + 1) * 8);
        c.out = (int64_t *)p; p += align256(max_vals * 8 + 8);
        c.ws = p;
        return c;
    };
    auto submit = [&](int64_t c) -> int {
        PipeSlot &P = S[c & 1];
        const Carve d = carve(P);
        const int64_t lo = cuts[(size_t)c], hi = cuts[(size_t)c + 1], nr = hi - lo, nb = ro[hi] - ro[lo], nvals = oo[hi] - oo[lo];
        int64_t *hro = (int64_t *)(P.h_in + align256(max_bases + 16)), *hoo = (int64_t *)((char *)hro + align256((max_reads + 1) * 8));
        for (int64_t r = 0; r <= nr; r++) { hro[r] = ro[lo + r] - ro[lo]; hoo[r] = oo[lo + r] - oo[lo]; }
        const char *hb = src_bases + ro[lo];
        if (!pin_in) { memcpy(P.h_in, hb, (size_t)nb); hb = P.h_in; }
        hipError_t e;
        if ((e = hipMemcpyAsync(d.bases, hb, (size_t)nb, hipMemcpyHostToDevice, P.st)) != hipSuccess ||
            (e = hipMemcpyAsync(d.roff, hro, (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, P.st)) != hipSuccess ||
            (e = hipMemcpyAsync(d.ooff, hoo, (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, P.st)) != hipSuccess)
            return fail(SBWTGPU_ERR_HIP, "H2D copy: %s", hipGetErrorString(e));
        t_out32 = out32 ? 1 : 0;                        // (int32 results: the kernels write them into the same device range)
        int r2 = search_dev_common(idx, d.bases, nb, d.roff, nr, d.out, d.ooff, d.ws, ws_bytes, P.st, streaming);
        t_out32 = 0;
        if (r2 != SBWTGPU_OK) return r2;
        char *target = pin_out ? (out32 ? (char *)(out32 + oo[lo]) : (char *)(out + oo[lo])) : P.h_out;
        const void *from = d.out;
        if ((e = hipMemcpyAsync(target, from, (size_t)(nvals * vb), hipMemcpyDeviceToHost, P.st)) != hipSuccess ||
            (e = hipMemcpyAsync(P.h_status, d.ws + offsetof(SbwtWorkHeader, status), 4, hipMemcpyDeviceToHost, P.st)) != hipSuccess)
            return fail(SBWTGPU_ERR_HIP, "D2H copy: %s", hipGetErrorString(e));
        return SBWTGPU_OK;
    };
    auto collect = [&](int64_t c) -> int {
        PipeSlot &P = S[c & 1];
        hipError_t e = hipStreamSynchronize(P.st);
        if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "stream synchronize: %s", hipGetErrorString(e));
        if (P.h_status[0] != 0 && bug == 0) bug = P.h_status[0];
        const int64_t lo = cuts[(size_t)c], hi = cuts[(size_t)c + 1];
        if (!pin_out) parallel_memcpy(out32 ? (char *)(out32 + oo[lo]) : (char *)(out + oo[lo]), P.h_out, (size_t)((oo[hi] - oo[lo]) * vb));
        return SBWTGPU_OK;
    };
    rc = two_in_flight(n_chunks, submit, collect);
    park_slots(idx->device, S, 2, rc);
    if (rc != SBWTGPU_OK) return rc;
    if (bug) return fail_status(bug);
    return SBWTGPU_OK;
}

static int search_host_common(const sbwtgpu_index *idx, const char *bases, const int64_t *read_off, int64_t n_reads,
                              int64_t *out, const int64_t *out_off, int streaming) {
    if (!idx) return fail(SBWTGPU_ERR_INVALID_ARG, "idx is NULL");
    if (streaming && !idx->h.has_ssup)
        return fail(SBWTGPU_ERR_NO_STREAMING, "Error: streaming search support not built");
    if (n_reads < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative n_reads");
    if (n_reads == 0) return SBWTGPU_OK;
    if (!read_off || !out_off) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL offsets");
    bool any_long = false;
    int rc = check_reads(read_off, out_off, n_reads, idx->h.k, &any_long);
    if (rc != SBWTGPU_OK) return rc;
    const int64_t base0 = read_off[0], total = read_off[n_reads] - base0;
    const int64_t out0 = out_off[0], n_out = out_off[n_reads] - out0;
    if (total > 0 && !bases) return fail(SBWTGPU_ERR_INVALID_ARG, "bases is NULL");
    if (n_out > 0 && !out) return fail(SBWTGPU_ERR_INVALID_ARG, "out is NULL");
    if (n_out == 0) return SBWTGPU_OK;
    // a large batch of ordinary reads: the pipeline works on the caller's arrays as they are (it only ever uses
    // differences of offsets; every chunk's offsets are rebased into its staging buffer anyway)
    if (!any_long && n_out * 8 >= PIPE_MIN)
        return search_host_pipelined(idx, bases, read_off, out_off, n_reads, out, streaming);

    // offsets are rebased so that device buffers start at 0; long reads are cut into pieces (see above)
    const int64_t kk = idx->h.k;
    std::vector<int64_t> ro, oo;
    std::vector<char> vbases;
    const char *src_bases = bases + base0;
    int64_t nv = n_reads, vtotal = total;
    try {
        if (!any_long) {
            ro.resize((size_t)n_reads + 1);
            oo.resize((size_t)n_reads + 1);
            for (int64_t r = 0; r <= n_reads; r++) {
                ro[(size_t)r] = read_off[r] - base0;
                oo[(size_t)r] = out_off[r] - out0;
            }
        } else {
            int64_t bound = 0;
            for (int64_t r = 0; r < n_reads; r++) bound += pieces_bases_bound(read_off[r + 1] - read_off[r], kk);
            vbases.resize((size_t)bound + 16);
            ro.assign(1, 0);
            oo.assign(1, 0);
            int64_t w = 0;
            for (int64_t r = 0; r < n_reads; r++)
                w += append_pieces(bases + read_off[r], read_off[r + 1] - read_off[r], kk, vbases.data() + w, ro, oo);
            src_bases = vbases.data();
            vtotal = w;
            nv = (int64_t)ro.size() - 1;
        }
    } catch (const std::bad_alloc &) {
        return fail(SBWTGPU_ERR_OOM, "out of host memory");
    }
    if (n_out * 8 >= PIPE_MIN)
        return search_host_pipelined(idx, src_bases, ro.data(), oo.data(), nv, out + out0, streaming);
    DeviceGuard guard(idx->device);
    const int64_t ws_bytes = sbwtgpu_search_workspace_bytes(vtotal);
    // layout [roff][ooff][bases] (in) | [out][workspace]: a small call's one D2H copy ends with the workspace header
    const size_t o_roff = 0, o_ooff = align256((size_t)(nv + 1) * 8), o_bases = o_ooff + align256((size_t)(nv + 1) * 8);
    const size_t o_out = o_bases + align256((size_t)vtotal + 16), o_ws = o_out + align256((size_t)n_out * 8);
    Staging sg;
    STG_TRY(sg.open(idx->device, o_ws + (size_t)ws_bytes));
    STG_TRY(sg.in(o_roff, ro.data(), (size_t)(nv + 1) * 8));
    STG_TRY(sg.in(o_ooff, oo.data(), (size_t)(nv + 1) * 8));
    STG_TRY(sg.in(o_bases, src_bases, (size_t)vtotal));
    STG_TRY(sg.upload());
    STG_TRY(search_dev_common(idx, sg.at<const char>(o_bases), vtotal, sg.at<const int64_t>(o_roff), nv, sg.at<int64_t>(o_out),
                              sg.at<const int64_t>(o_ooff), sg.at<char>(o_ws), ws_bytes, sg.stream, streaming));
    SbwtWorkHeader hdr;
    STG_TRY(sg.out(o_out, out + out0, (size_t)n_out * 8));
    STG_TRY(sg.out(o_ws, &hdr, sizeof(hdr)));
    STG_TRY(sg.finish());
    if (hdr.status != 0) return fail_status(hdr.status);
    return SBWTGPU_OK;
}

int sbwtgpu_streaming_search_batch(const sbwtgpu_index *idx, const char *bases, const int64_t *read_off,
                                   int64_t n_reads, int64_t *out, const int64_t *out_off) {
    return search_host_common(idx, bases, read_off, n_reads, out, out_off, 1);
}

int sbwtgpu_search_batch(const sbwtgpu_index *idx, const char *bases, const int64_t *read_off, int64_t n_reads,
                         int64_t *out, const int64_t *out_off) {
    return search_host_common(idx, bases, read_off, n_reads, out, out_off, 0);
}

// Results as int32 (result compaction): for indexes of fewer than 2^31 columns every rank fits, -1 stays -1.  The
// kernels write int32 themselves, so a result costs 4 bytes of HBM writes and of PCIe instead of 8.  Large batches go through
// the same two-stream pipeline as the int64 calls; small ones through the int64 call and a host loop.
static int search_host_i32(const sbwtgpu_index *idx, const char *bases, const int64_t *read_off, int64_t n_reads,
                           int32_t *out, const int64_t *out_off, int streaming) {
    if (!idx) return fail(SBWTGPU_ERR_INVALID_ARG, "idx is NULL");
    if (idx->h.n_nodes >= ((int64_t)1 << 31))
        return fail(SBWTGPU_ERR_INVALID_ARG, "int32 results need an index of fewer than 2^31 columns (this one has %lld)",
                    (long long)idx->h.n_nodes);
    if (streaming && !idx->h.has_ssup) return fail(SBWTGPU_ERR_NO_STREAMING, "Error: streaming search support not built");
    if (n_reads < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative n_reads");
    if (n_reads == 0) return SBWTGPU_OK;
    if (!read_off || !out_off) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL offsets");
    bool any_long = false;
    int rc = check_reads(read_off, out_off, n_reads, idx->h.k, &any_long);
    if (rc != SBWTGPU_OK) return rc;
    const int64_t n_out = out_off[n_reads] - out_off[0];
    if (n_out == 0) return SBWTGPU_OK;
    if (!out) return fail(SBWTGPU_ERR_INVALID_ARG, "out is NULL");
    if (!any_long && n_out * 4 >= PIPE_MIN)
        return search_host_pipelined(idx, bases, read_off, out_off, n_reads, nullptr, streaming, out);
    std::vector<int64_t> wide;
    try { wide.resize((size_t)n_out); } catch (const std::bad_alloc &) { return fail(SBWTGPU_ERR_OOM, "out of host memory"); }
    std::vector<int64_t> oo((size_t)n_reads + 1);
    for (int64_t r = 0; r <= n_reads; r++) oo[(size_t)r] = out_off[r] - out_off[0];
    rc = search_host_common(idx, bases, read_off, n_reads, wide.data(), oo.data(), streaming);
    if (rc != SBWTGPU_OK) return rc;
    int32_t *dst = out + out_off[0];
    for (int64_t t = 0; t < n_out; t++) dst[t] = (int32_t)wide[(size_t)t];
    return SBWTGPU_OK;
}
int sbwtgpu_streaming_search_batch_i32(const sbwtgpu_index *idx, const char *bases, const int64_t *read_off,
                                       int64_t n_reads, int32_t *out, const int64_t *out_off) {
    return search_host_i32(idx, bases, read_off, n_reads, out, out_off, 1);
}
int sbwtgpu_search_batch_i32(const sbwtgpu_index *idx, const char *bases, const int64_t *read_off, int64_t n_reads,
                             int32_t *out, const int64_t *out_off) {
    return search_host_i32(idx, bases, read_off, n_reads, out, out_off, 0);
}

int sbwtgpu_rank_batch(const sbwtgpu_index *idx, const int64_t *pos, const char *sym, int64_t n, int64_t *out) {
    if (!idx) return fail(SBWTGPU_ERR_INVALID_ARG, "idx is NULL");
    if (n < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative n");
    if (n == 0) return SBWTGPU_OK;
    if (!pos || !sym || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    for (int64_t t = 0; t < n; t++)
        if (pos[t] < 0 || pos[t] > idx->h.n_nodes)
            return fail(SBWTGPU_ERR_INVALID_ARG, "pos[%lld] = %lld outside [0, n_nodes]", (long long)t, (long long)pos[t]);
    DeviceGuard guard(idx->device);
    // [pos][sym] in, [out] back
    const size_t o_sym = align256((size_t)n * 8), o_out = o_sym + align256((size_t)n);
    Staging sg;
    STG_TRY(sg.open(idx->device, o_out + (size_t)n * 8));
    STG_TRY(sg.in(0, pos, (size_t)n * 8));
    STG_TRY(sg.in(o_sym, sym, (size_t)n));
    STG_TRY(sg.upload());
    STG_TRY(sbwtgpu_rank_dev(idx, sg.at<const int64_t>(0), sg.at<const char>(o_sym), n, sg.at<int64_t>(o_out), sg.stream));
    STG_TRY(sg.out(o_out, out, (size_t)n * 8));
    return sg.finish();
}

int sbwtgpu_update_interval_batch(const sbwtgpu_index *idx, const char *bases, const int64_t *off, int64_t n,
                                  int64_t *first, int64_t *second) {
    if (!idx) return fail(SBWTGPU_ERR_INVALID_ARG, "idx is NULL");
    if (idx->h.rank_only) return fail(SBWTGPU_ERR_INVALID_ARG, "%s", RANK_ONLY_MSG);
    if (n < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative n");
    if (n == 0) return SBWTGPU_OK;
    if (!off || !first || !second) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    const int64_t base0 = off[0], total = off[n] - base0;
    if (total < 0 || (total > 0 && !bases)) return fail(SBWTGPU_ERR_INVALID_ARG, "bad bases/offsets");
    for (int64_t t = 0; t < n; t++) {
        if (off[t + 1] < off[t]) return fail(SBWTGPU_ERR_INVALID_ARG, "off is not non-decreasing");
        if (first[t] != -1 && (first[t] < 0 || second[t] >= idx->h.n_nodes || second[t] < -1))
            return fail(SBWTGPU_ERR_INVALID_ARG, "interval %lld out of range", (long long)t);
    }
    DeviceGuard guard(idx->device);
    // [first][second] (in and back) [off][bases]
    const size_t o_s = align256((size_t)n * 8), o_off = 2 * o_s, o_bases = o_off + align256((size_t)(n + 1) * 8);
    Staging sg;
    STG_TRY(sg.open(idx->device, o_bases + (size_t)total + 16));
    STG_TRY(sg.in(0, first, (size_t)n * 8));
    STG_TRY(sg.in(o_s, second, (size_t)n * 8));
    STG_TRY(sg.in_rebased(o_off, off, n + 1));
    STG_TRY(sg.in(o_bases, bases + base0, (size_t)total));
    STG_TRY(sg.upload());
    sbwt_launch_update_interval(idx->view(), sg.at<const char>(o_bases), sg.at<const long long>(o_off), n, sg.at<long long>(0),
                                sg.at<long long>(o_s), sg.stream);
    HIP_TRY(hipGetLastError());
    STG_TRY(sg.out(0, first, (size_t)n * 8));
    STG_TRY(sg.out(o_s, second, (size_t)n * 8));
    return sg.finish();
}

int sbwtgpu_forward_batch(const sbwtgpu_index *idx, const int64_t *node, const char *sym, int64_t n, int64_t *out) {
    if (!idx) return fail(SBWTGPU_ERR_INVALID_ARG, "idx is NULL");
    if (idx->h.rank_only) return fail(SBWTGPU_ERR_INVALID_ARG, "%s", RANK_ONLY_MSG);
    if (!idx->h.has_ssup)
        return fail(SBWTGPU_ERR_NO_STREAMING, "Error: Streaming support required for SBWT::forward");
    if (n < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative n");
    if (n == 0) return SBWTGPU_OK;
    if (!node || !sym || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    for (int64_t t = 0; t < n; t++)
        if (node[t] < 0 || node[t] >= idx->h.n_nodes)
            return fail(SBWTGPU_ERR_INVALID_ARG, "node[%lld] out of range", (long long)t);
    DeviceGuard guard(idx->device);
    // [node][sym] in, [out] back
    const size_t o_sym = align256((size_t)n * 8), o_out = o_sym + align256((size_t)n);
    Staging sg;
    STG_TRY(sg.open(idx->device, o_out + (size_t)n * 8));
    STG_TRY(sg.in(0, node, (size_t)n * 8));
    STG_TRY(sg.in(o_sym, sym, (size_t)n));
    STG_TRY(sg.upload());
    sbwt_launch_forward(idx->view(), sg.at<const long long>(0), sg.at<const char>(o_sym), n, sg.at<long long>(o_out), sg.stream);
    HIP_TRY(hipGetLastError());
    STG_TRY(sg.out(o_out, out, (size_t)n * 8));
    return sg.finish();
}

int sbwtgpu_partial_search_batch(const sbwtgpu_index *idx, const char *bases, const int64_t *off, int64_t n,
                                 int64_t *first, int64_t *second, int64_t *matched) {
    if (!idx) return fail(SBWTGPU_ERR_INVALID_ARG, "idx is NULL");
    if (idx->h.rank_only) return fail(SBWTGPU_ERR_INVALID_ARG, "%s", RANK_ONLY_MSG);
    if (n < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative n");
    if (n == 0) return SBWTGPU_OK;
    if (!off || !first || !second || !matched) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    const int64_t base0 = off[0], total = off[n] - base0;
    if (total < 0 || (total > 0 && !bases)) return fail(SBWTGPU_ERR_INVALID_ARG, "bad bases/offsets");
    for (int64_t t = 0; t < n; t++)
        if (off[t + 1] < off[t]) return fail(SBWTGPU_ERR_INVALID_ARG, "off is not non-decreasing");
    DeviceGuard guard(idx->device);
    // [first][second][matched] (back) [off][bases] (in)
    const size_t o_s = align256((size_t)n * 8), o_m = 2 * o_s, o_off = 3 * o_s, o_bases = o_off + align256((size_t)(n + 1) * 8);
    Staging sg;
    STG_TRY(sg.open(idx->device, o_bases + (size_t)total + 16));
    STG_TRY(sg.in_rebased(o_off, off, n + 1));
    STG_TRY(sg.in(o_bases, bases + base0, (size_t)total));
    STG_TRY(sg.upload());
    sbwt_launch_partial_search(idx->view(), sg.at<const char>(o_bases), sg.at<const long long>(o_off), n, sg.at<long long>(0),
                               sg.at<long long>(o_s), sg.at<long long>(o_m), sg.stream);
    HIP_TRY(hipGetLastError());
    STG_TRY(sg.out(0, first, (size_t)n * 8));
    STG_TRY(sg.out(o_s, second, (size_t)n * 8));
    STG_TRY(sg.out(o_m, matched, (size_t)n * 8));
    return sg.finish();
}

int sbwtgpu_get_kmer_batch(const sbwtgpu_index *idx, const int64_t *colex_rank, int64_t n, char *out) {
    if (!idx) return fail(SBWTGPU_ERR_INVALID_ARG, "idx is NULL");
    if (idx->h.rank_only) return fail(SBWTGPU_ERR_INVALID_ARG, "%s", RANK_ONLY_MSG);
    if (n < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative n");
    if (n == 0) return SBWTGPU_OK;
    if (!colex_rank || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    for (int64_t t = 0; t < n; t++)
        if (colex_rank[t] < 0 || colex_rank[t] >= idx->h.n_nodes)
            return fail(SBWTGPU_ERR_INVALID_ARG, "colex_rank[%lld] out of range", (long long)t);
    DeviceGuard guard(idx->device);
    const int64_t k = idx->h.k;
    const size_t o_out = align256((size_t)n * 8);
    Staging sg;
    STG_TRY(sg.open(idx->device, o_out + (size_t)(n * k) + 16));
    STG_TRY(sg.in(0, colex_rank, (size_t)n * 8));
    STG_TRY(sg.upload());
    sbwt_launch_get_kmer(idx->view(), sg.at<const long long>(0), n, sg.at<char>(o_out), sg.stream);
    HIP_TRY(hipGetLastError());
    STG_TRY(sg.out(o_out, out, (size_t)(n * k)));
    return sg.finish();
}

int sbwtgpu_select_batch(const sbwtgpu_index *idx, const int64_t *j, const char *sym, int64_t n, int64_t *out) {
    if (!idx) return fail(SBWTGPU_ERR_INVALID_ARG, "idx is NULL");
    if (n < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative n");
    if (n == 0) return SBWTGPU_OK;
    if (!j || !sym || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    for (int64_t t = 0; t < n; t++) {
        const char ch = sym[t];
        const int c = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : -1;
        if (c >= 0 && (j[t] < 1 || j[t] > idx->h.row_ones[c]))
            return fail(SBWTGPU_ERR_INVALID_ARG, "j[%lld] = %lld outside [1, %lld] (ones in row %c)", (long long)t,
                        (long long)j[t], (long long)idx->h.row_ones[c], ch);
    }
    DeviceGuard guard(idx->device);
    const size_t o_sym = align256((size_t)n * 8), o_out = o_sym + align256((size_t)n);
    Staging sg;
    STG_TRY(sg.open(idx->device, o_out + (size_t)n * 8));
    STG_TRY(sg.in(0, j, (size_t)n * 8));
    STG_TRY(sg.in(o_sym, sym, (size_t)n));
    STG_TRY(sg.upload());
    long long ones[4] = {idx->h.row_ones[0], idx->h.row_ones[1], idx->h.row_ones[2], idx->h.row_ones[3]};
    sbwt_launch_select(idx->view(), sg.at<const long long>(0), sg.at<const char>(o_sym), n, ones, sg.at<long long>(o_out), sg.stream);
    HIP_TRY(hipGetLastError());
    STG_TRY(sg.out(o_out, out, (size_t)n * 8));
    return sg.finish();
}

// ---- construction on the device ---------------------------------------------------
}  // extern "C"
namespace {
// The host part between the builder's two device phases: the dummy prefixes of the predecessor-less k-mers
// (NodeBOSSInMemoryConstructor.hh:70-79) + the root, sorted like Kmer::operator< (label, then length), equal nodes merged.
// KT = the key type of the device builder: uint64_t for k <= 32, unsigned __int128 for 32 < k <= 64.
template <typename KT>
int build_columns_t(SbwtBuildState &S, int64_t k, int build_streaming_support, sbwtgpu_plain_matrix_bits *out) {
    std::vector<KT> nopred, ddata;
    std::vector<unsigned long long> rows;
    std::vector<unsigned> dedges;
    nopred.resize((size_t)S.n_nopred);
    if (sbwt_build_copy_nopred(&S, nopred.data()) != 0) { sbwt_build_release(&S); return fail(SBWTGPU_ERR_HIP, "device builder: copy"); }
    struct Dm { KT data; unsigned len, edges; };
    std::vector<Dm> dm;
    dm.reserve((size_t)S.n_nopred * (size_t)k + 1);
    dm.push_back(Dm{(KT)0, 0, 0});
    const int kbits = 2 * (int)k;
    for (KT zk : nopred)
        for (int j = 0; j < (int)k; j++) {
            KT label = (j == 0) ? (KT)0 : (KT)((zk & ((((KT)1) << (2 * j)) - (KT)1)) << (kbits - 2 * j));
            dm.push_back(Dm{label, (unsigned)j, 1u << (unsigned)((unsigned)(zk >> (2 * j)) & 3u)});
        }
    std::sort(dm.begin(), dm.end(), [](const Dm &a, const Dm &b) { return a.data != b.data ? a.data < b.data : a.len < b.len; });
    size_t wd = 0;
    for (size_t i = 0; i < dm.size(); i++) {
        if (wd > 0 && dm[wd - 1].data == dm[i].data && dm[wd - 1].len == dm[i].len) dm[wd - 1].edges |= dm[i].edges;
        else dm[wd++] = dm[i];
    }
    dm.resize(wd);
    ddata.resize(wd);
    dedges.resize(wd);
    for (size_t i = 0; i < wd; i++) { ddata[i] = dm[i].data; dedges[i] = dm[i].edges; }
    const int64_t n = S.nk + (int64_t)wd, nw = (n + 63) / 64;
    rows.resize((size_t)(5 * nw));
    int rb = sbwt_build_phase_b(&S, ddata.data(), dedges.data(), (long long)wd, build_streaming_support ? 1 : 0, rows.data(), 0);
    const int64_t nk = S.nk;
    sbwt_build_release(&S);
    if (rb != 0) return fail(rb == -8 ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "device builder, phase B");
    uint64_t *mem = static_cast<uint64_t *>(malloc((size_t)(5 * nw) * 8 + 8));
    if (!mem) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    memcpy(mem, rows.data(), (size_t)(5 * nw) * 8);
    out->n_nodes = n;
    out->n_kmers = nk;
    out->k = k;
    out->A_bits = mem;
    out->C_bits = mem + nw;
    out->G_bits = mem + 2 * nw;
    out->T_bits = mem + 3 * nw;
    out->suffix_group_starts = build_streaming_support ? mem + 4 * nw : nullptr;
    return SBWTGPU_OK;
}
}  // namespace
extern "C" {

int sbwtgpu_build_plain_matrix(const char *const *seqs, const int64_t *seq_len, int64_t n_seqs, int64_t k, int add_revcomp,
                               int build_streaming_support, int device, sbwtgpu_plain_matrix_bits *out) {
    if (!out) return fail(SBWTGPU_ERR_INVALID_ARG, "out is NULL");
    memset(out, 0, sizeof(*out));
    if (n_seqs < 0 || (n_seqs > 0 && (!seqs || !seq_len))) return fail(SBWTGPU_ERR_INVALID_ARG, "bad sequence list");
    if (k < 2 || k > 64)
        return fail(SBWTGPU_ERR_INVALID_ARG, "the device builder packs a k-mer into 64 or 128 bits: 2 <= k <= 64");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SBWTGPU_ERR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= ndev) return fail(SBWTGPU_ERR_NO_DEVICE, "device %d out of range", device);
    DeviceGuard guard(device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", device);
    // one text, sequences separated by a byte that is not ACGT: a k-mer window across a boundary is invalid like one with N
    int64_t n_text = 0;
    for (int64_t i = 0; i < n_seqs; i++) {
        if (seq_len[i] < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative sequence length");
        n_text += seq_len[i] + 1;
    }
    std::vector<char> text;
    SbwtBuildState S;
    int rc = SBWTGPU_OK;
    try {
        text.resize((size_t)n_text + 1);
        int64_t w = 0;
        for (int64_t i = 0; i < n_seqs; i++) {
            if (seq_len[i]) memcpy(text.data() + w, seqs[i], (size_t)seq_len[i]);
            w += seq_len[i];
            text[(size_t)w++] = '$';
        }
        int ra = sbwt_build_phase_a(text.data(), n_text, (int)k, add_revcomp ? 1 : 0, &S, 0);
        if (ra != 0) { sbwt_build_release(&S); return fail(ra == -8 ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "device builder, phase A"); }
        std::vector<char>().swap(text);
        // the dummy prefixes are expanded on the host, k per predecessor-less k-mer at 16-32 bytes each: about one k-mer per
        // input SEQUENCE, so a genome has a handful and a read set has millions.  Past 2^26 records the caller's host
        // builder (index_builder.hh) is the better tool: report it as "does not fit".
        if ((long long)S.n_nopred * (long long)k > (1ll << 26)) {
            sbwt_build_release(&S);
            return fail(SBWTGPU_ERR_OOM, "device builder: %lld predecessor-less k-mers x k = %lld dummy records (limit 2^26): "
                        "use the host builder for inputs with this many sequences", (long long)S.n_nopred,
                        (long long)S.n_nopred * (long long)k);
        }
        rc = (k <= 32) ? build_columns_t<unsigned long long>(S, k, build_streaming_support, out)
                       : build_columns_t<unsigned __int128>(S, k, build_streaming_support, out);
    } catch (const std::bad_alloc &) {
        sbwt_build_release(&S);
        rc = fail(SBWTGPU_ERR_OOM, "out of host memory");
    }
    return rc;
}

void sbwtgpu_free_plain_matrix(sbwtgpu_plain_matrix_bits *b) {
    if (!b) return;
    free(b->A_bits);                                   // one allocation holds all five rows
    memset(b, 0, sizeof(*b));
}

// ---- device-side formatting + pipelined host path ------------------------------------------------
int64_t sbwtgpu_format_text_bound(const sbwtgpu_index *idx, int64_t n_values, int64_t n_reads) {
    int digits = 1;
    for (int64_t x = idx ? idx->h.n_nodes : INT64_MAX; x >= 10; x /= 10) digits++;
    int tok = digits + 1 > 3 ? digits + 1 : 3;
    return n_values * tok + n_reads + 16;
}
int64_t sbwtgpu_format_scratch_bytes(int64_t n_reads) { return sbwt_format_scratch_bytes(n_reads < 0 ? 0 : n_reads); }

int sbwtgpu_format_results_dev(const sbwtgpu_index *idx, const int64_t *d_values, const int64_t *d_out_off,
                               int64_t n_reads, int64_t n_values, char *d_text, int64_t text_cap, int64_t *d_line_off,
                               void *d_scratch, int64_t scratch_bytes, void *stream) {
    if (!idx) return fail(SBWTGPU_ERR_INVALID_ARG, "idx is NULL");
    if (n_reads < 0 || n_values < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative size");
    if (n_reads == 0) return SBWTGPU_OK;
    if (!d_out_off || !d_text || !d_line_off || !d_scratch || (n_values > 0 && !d_values))
        return fail(SBWTGPU_ERR_INVALID_ARG, "NULL device pointer");
    if (text_cap < sbwtgpu_format_text_bound(idx, n_values, n_reads))
        return fail(SBWTGPU_ERR_INVALID_ARG, "text buffer smaller than sbwtgpu_format_text_bound()");
    if (scratch_bytes < sbwtgpu_format_scratch_bytes(n_reads)) return fail(SBWTGPU_ERR_INVALID_ARG, "scratch too small");
    DeviceGuard guard(idx->device);
    sbwt_launch_format(reinterpret_cast<const long long *>(d_values), reinterpret_cast<const long long *>(d_out_off),
                       n_reads, d_text, reinterpret_cast<long long *>(d_line_off), d_scratch,
                       static_cast<hipStream_t>(stream));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return SBWTGPU_OK;
}

void sbwtgpu_free_host(void *p) { free(p); }

void sbwtgpu_release_cached_buffers(void) {
    {
        std::lock_guard<std::mutex> lock(g_park_mutex);
        for (auto &p : g_parked) { DeviceGuard guard(p.device); p.slot.release(); }
        g_parked.clear();
    }
    for (auto &sl : t_slots.v) sl.release();            // the calling thread's small-call slots
    t_slots.v.clear();
}

int sbwtgpu_search_text_stream(const sbwtgpu_index *idx, const char *bases, const int64_t *read_off, int64_t n_reads,
                               int streaming, sbwtgpu_text_sink sink, void *sink_ctx, int64_t *n_queries) {
    if (!idx || !sink) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    if (n_queries) *n_queries = 0;
    if (streaming && !idx->h.has_ssup)
        return fail(SBWTGPU_ERR_NO_STREAMING, "Error: streaming search support not built");
    if (idx->h.rank_only) return fail(SBWTGPU_ERR_INVALID_ARG, "%s", RANK_ONLY_MSG);
    if (n_reads < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative n_reads");
    if (n_reads > 0 && (!read_off || (read_off[n_reads] > read_off[0] && !bases)))
        return fail(SBWTGPU_ERR_INVALID_ARG, "NULL input");
    const int64_t k = idx->h.k;
    // ---- chunking: <= 8 Mi bases and <= 1 Mi reads per chunk (small pinned buffers, deep overlap) ----
    const int64_t CH_BASES = (int64_t)8 << 20, CH_READS = (int64_t)1 << 20;
    std::vector<int64_t> cuts{0};
    int64_t max_bases = 0, max_reads = 0, max_vals = 0, max_vreads = 0;
    {
        // vb / vr: bases and reads of the chunk after long reads are cut into pieces
        int64_t lo = 0, vals = 0, vb = 0, vr = 0;
        for (int64_t r = 0; r < n_reads; r++) {
            const int rc = check_read_length(read_off, r);
            if (rc != SBWTGPU_OK) return rc;
            const int64_t len = read_off[r + 1] - read_off[r];
            if (r > lo && (read_off[r + 1] - read_off[lo] > CH_BASES || r - lo >= CH_READS)) {
                max_bases = std::max(max_bases, vb);
                max_reads = std::max(max_reads, r - lo);
                max_vreads = std::max(max_vreads, vr);
                max_vals = std::max(max_vals, vals);
                cuts.push_back(r);
                lo = r;
                vals = vb = vr = 0;
            }
            const int64_t mm = std::max<int64_t>(0, len - k + 1);
            vals += mm;
            vb += pieces_bases_bound(len, k);
            vr += (mm > 2 * PIECE) ? mm / PIECE + 2 : 1;
        }
        if (n_reads > lo) {
            max_bases = std::max(max_bases, vb);
            max_reads = std::max(max_reads, n_reads - lo);
            max_vreads = std::max(max_vreads, vr);
            max_vals = std::max(max_vals, vals);
            cuts.push_back(n_reads);
        }
    }
    const int64_t n_chunks = (int64_t)cuts.size() - 1;
    if (n_chunks == 0) return SBWTGPU_OK;
    DeviceGuard guard(idx->device);
    // a slot's pinned input: [bases][pieces' base offsets][pieces' result offsets][reads' result offsets]; its pinned output: the
    // text; its device range: the same four, the reads' line offsets, the results, the search workspace, the text, the
    // formatter's scratch.  (The workspace is sized by what sbwtgpu_search_workspace_bytes asks for NOW: tuning may have changed it.)
    const int64_t cap_text = sbwtgpu_format_text_bound(idx, max_vals, max_reads);
    const int64_t ws_bytes = sbwtgpu_search_workspace_bytes(max_bases), scr_bytes = sbwtgpu_format_scratch_bytes(max_reads);
    const int64_t b_bases = align256(max_bases + 16), b_voff = align256((max_vreads + 1) * 8), b_off = align256((max_reads + 1) * 8);
    const int n_slots = n_chunks > 2 ? 3 : (int)n_chunks;
    PipeSlot slots[3];
    int rc = take_slots(idx->device, slots, n_slots, b_bases + 2 * b_voff + b_off, cap_text,
                        b_bases + 2 * b_voff + 2 * b_off + align256(max_vals * 8 + 8) + align256(ws_bytes) + align256(cap_text) +
                            align256(scr_bytes), "text pipeline buffers");
    if (rc != SBWTGPU_OK) return rc;
    struct Carve { char *bases; int64_t *roff, *vooff, *ooff, *line, *out; char *ws, *text, *scr; };
    auto carve = [&](const PipeSlot &P) {
        Carve c;
        char *p = P.d_mem;
        c.bases = p; p += b_bases;
        c.roff = (int64_t *)p; p += b_voff;
        c.vooff = (int64_t *)p; p += b_voff;           // result offsets of the pieces (roff holds the pieces' base offsets)
        c.ooff = (int64_t *)p; p += b_off;
        c.line = (int64_t *)p; p += b_off;
        c.out = (int64_t *)p; p += align256(max_vals * 8 + 8);
        c.ws = p; p += align256(ws_bytes);
        c.text = p; p += align256(cap_text);
        c.scr = p;
        return c;
    };
    int64_t text_len[3] = {0, 0, 0};                   // of the chunk in flight on each slot
    int64_t total_queries = 0;
    int bug = 0;                    // the first nonzero device status of a chunk
    // enqueue everything of chunk c on its slot's stream up to the copy of the text length
    auto submit = [&](int64_t c) -> int {
        PipeSlot &S = slots[c % n_slots];
        const Carve d = carve(S);
        const int64_t lo = cuts[(size_t)c], hi = cuts[(size_t)c + 1], nr = hi - lo;
        char *hb = S.h_in;
        int64_t *hro = (int64_t *)(S.h_in + b_bases);                   // pieces: base offsets
        int64_t *hvo = (int64_t *)((char *)hro + b_voff);               // pieces: result offsets
        int64_t *hoo = (int64_t *)((char *)hvo + b_voff);               // reads: result offsets
        int64_t nb = 0, acc = 0, nv = 0;
        hoo[0] = 0;
        bool any_long = false;
        for (int64_t r = 0; r < nr && !any_long; r++) any_long = (read_off[lo + r + 1] - read_off[lo + r] - k + 1) > 2 * PIECE;
        if (!any_long) {
            // the usual chunk: no read long enough to be cut, pieces = reads -- one copy of the bases, offsets by a loop
            const int64_t b0 = read_off[lo];
            nb = read_off[hi] - b0;
            if (nb > max_bases || nr > max_vreads) return fail(SBWTGPU_ERR_HIP, "internal: piece bound exceeded");
            if (nb > 0) memcpy(hb, bases + b0, (size_t)nb);
            hro[0] = 0;
            hvo[0] = 0;
            for (int64_t r = 0; r < nr; r++) {
                const int64_t len = read_off[lo + r + 1] - read_off[lo + r];
                acc += std::max<int64_t>(0, len - k + 1);
                hro[r + 1] = read_off[lo + r + 1] - b0;
                hvo[r + 1] = acc;
                hoo[r + 1] = acc;
            }
            nv = nr;
        } else {
            std::vector<int64_t> vro{0}, voo{0};
            for (int64_t r = 0; r < nr; r++) {
                const int64_t len = read_off[lo + r + 1] - read_off[lo + r];
                nb += append_pieces(bases + read_off[lo + r], len, k, hb + nb, vro, voo);
                acc += std::max<int64_t>(0, len - k + 1);
                hoo[r + 1] = acc;
            }
            nv = (int64_t)vro.size() - 1;
            if (nv > max_vreads || nb > max_bases) return fail(SBWTGPU_ERR_HIP, "internal: piece bound exceeded");
            memcpy(hro, vro.data(), (size_t)(nv + 1) * 8);
            memcpy(hvo, voo.data(), (size_t)(nv + 1) * 8);
        }
        total_queries += acc;
        hipError_t e;
        if ((e = hipMemcpyAsync(d.bases, hb, (size_t)nb, hipMemcpyHostToDevice, S.st)) != hipSuccess ||
            (e = hipMemcpyAsync(d.roff, hro, (size_t)(nv + 1) * 8, hipMemcpyHostToDevice, S.st)) != hipSuccess ||
            (e = hipMemcpyAsync(d.vooff, hvo, (size_t)(nv + 1) * 8, hipMemcpyHostToDevice, S.st)) != hipSuccess ||
            (e = hipMemcpyAsync(d.ooff, hoo, (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, S.st)) != hipSuccess)
            return fail(SBWTGPU_ERR_HIP, "H2D copy: %s", hipGetErrorString(e));
        int r2 = search_dev_common(idx, d.bases, nb, d.roff, nv, d.out, d.vooff, d.ws, ws_bytes, S.st, streaming);
        if (r2 != SBWTGPU_OK) return r2;
        r2 = sbwtgpu_format_results_dev(idx, d.out, d.ooff, nr, acc, d.text, cap_text, d.line, d.scr, scr_bytes, S.st);
        if (r2 != SBWTGPU_OK) return r2;
        // the status word, and behind it (8-byte aligned) the length of the text
        if ((e = hipMemcpyAsync(S.h_status + 2, d.line + nr, 8, hipMemcpyDeviceToHost, S.st)) != hipSuccess ||
            (e = hipMemcpyAsync(S.h_status, d.ws + offsetof(SbwtWorkHeader, status), 4, hipMemcpyDeviceToHost, S.st)) != hipSuccess)
            return fail(SBWTGPU_ERR_HIP, "D2H copy: %s", hipGetErrorString(e));
        return SBWTGPU_OK;
    };
    // wait for chunk c's kernels, then start the copy of its text
    auto fetch = [&](int64_t c) -> int {
        PipeSlot &S = slots[c % n_slots];
        hipError_t e = hipStreamSynchronize(S.st);
        if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "stream synchronize: %s", hipGetErrorString(e));
        int64_t &len = text_len[c % n_slots];
        memcpy(&len, S.h_status + 2, 8);
        if (S.h_status[0] != 0 && bug == 0) bug = S.h_status[0];
        if (len < 0 || len > cap_text) return fail(SBWTGPU_ERR_HIP, "formatted text overflows its bound");
        e = hipMemcpyAsync(S.h_out, carve(S).text, (size_t)len, hipMemcpyDeviceToHost, S.st);
        if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "D2H copy: %s", hipGetErrorString(e));
        return SBWTGPU_OK;
    };
    // wait for chunk c's text and hand it to the sink (straight out of the pinned staging buffer)
    auto collect = [&](int64_t c) -> int {
        PipeSlot &S = slots[c % n_slots];
        hipError_t e = hipStreamSynchronize(S.st);
        if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "stream synchronize: %s", hipGetErrorString(e));
        const int64_t len = text_len[c % n_slots];
        if (len > 0 && sink(sink_ctx, S.h_out, len) != 0) return fail(SBWTGPU_ERR_INVALID_ARG, "the text sink reported an error");
        return SBWTGPU_OK;
    };
    // Three slots: while the sink has chunk c-2's text (a write to a file takes several times longer than the GPU needs
    // for a chunk), chunk c is on the GPU and chunk c-1's text is on its way down.
    for (int64_t c = 0; c < n_chunks && rc == SBWTGPU_OK; c++) {
        rc = submit(c);                                            // its slot was freed by collect(c - 3) in the last round
        if (rc == SBWTGPU_OK && c >= 1) rc = fetch(c - 1);
        if (rc == SBWTGPU_OK && c >= 2) rc = collect(c - 2);
    }
    if (rc == SBWTGPU_OK) rc = fetch(n_chunks - 1);
    for (int64_t c = std::max<int64_t>(0, n_chunks - 2); c < n_chunks && rc == SBWTGPU_OK; c++) rc = collect(c);
    park_slots(idx->device, slots, n_slots, rc);
    if (rc != SBWTGPU_OK) return rc;
    if (bug) return fail_status(bug);
    if (n_queries) *n_queries = total_queries;
    return SBWTGPU_OK;
}

// The same with the whole text in one malloc'ed buffer: sized by the bound of the batch (untouched pages cost nothing)
// and shrunk at the end, so every chunk's text is copied exactly once.
namespace {
struct TextAcc { char *buf; int64_t len, cap; };
int text_acc_sink(void *ctx, const char *text, int64_t bytes) {
    TextAcc *a = static_cast<TextAcc *>(ctx);
    if (a->len + bytes > a->cap) return 1;
    memcpy(a->buf + a->len, text, (size_t)bytes);
    a->len += bytes;
    return 0;
}
}  // namespace
int sbwtgpu_search_text_batch(const sbwtgpu_index *idx, const char *bases, const int64_t *read_off, int64_t n_reads,
                              int streaming, char **text, int64_t *text_bytes, int64_t *n_queries) {
    if (!idx || !text || !text_bytes) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    *text = nullptr;
    *text_bytes = 0;
    if (n_queries) *n_queries = 0;
    if (n_reads < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative n_reads");
    if (n_reads > 0 && !read_off) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL input");
    int64_t all_vals = 0;
    for (int64_t r = 0; r < n_reads; r++) all_vals += std::max<int64_t>(0, read_off[r + 1] - read_off[r] - idx->h.k + 1);
    TextAcc acc{nullptr, 0, sbwtgpu_format_text_bound(idx, all_vals, n_reads) + 1};
    acc.buf = (char *)malloc((size_t)acc.cap);
    if (!acc.buf) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    const int rc = sbwtgpu_search_text_stream(idx, bases, read_off, n_reads, streaming, text_acc_sink, &acc, n_queries);
    if (rc != SBWTGPU_OK) { free(acc.buf); return rc; }
    char *shrunk = (char *)realloc(acc.buf, (size_t)(acc.len ? acc.len : 1));
    *text = shrunk ? shrunk : acc.buf;
    *text_bytes = acc.len;
    return SBWTGPU_OK;
}

// ---- matching statistics (sbwt_ms.hip) ------------------------------------------------------------
namespace {
int lcs_build_locked(const sbwtgpu_index *idx) {
    if (idx->lcs) return SBWTGPU_OK;
    DeviceGuard guard(idx->device);
    const int64_t n = idx->h.n_nodes;
    DevBuf scratch;
    unsigned char *d_lcs = nullptr;
    // n + 1 entries (lcs[n] = 0), rounded up to whole 64-byte lines: the contraction reads aligned 8-byte words
    const size_t lcs_bytes = (size_t)((n + 1 + 63) & ~(int64_t)63) + 64;
    hipError_t e = hipMalloc((void **)&d_lcs, lcs_bytes);
    if (e == hipSuccess) e = scratch.alloc((size_t)sbwt_lcs_scratch_bytes(n));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (d_lcs) (void)hipFree(d_lcs);
        return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "LCS array: hipMalloc failed: %s",
                    hipGetErrorString(e));
    }
    Stream st;
    e = hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMemsetAsync(d_lcs, 0, lcs_bytes, st.s);
    if (e == hipSuccess) e = hipMemsetAsync(scratch.p, 0, (size_t)sbwt_lcs_scratch_bytes(n), st.s);
    if (e == hipSuccess) {
        sbwt_launch_build_lcs(idx->view(), scratch.p, d_lcs, st.s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st.s);
    if (e != hipSuccess) {
        (void)hipFree(d_lcs);
        return fail(SBWTGPU_ERR_HIP, "LCS build: %s", hipGetErrorString(e));
    }
    idx->lcs = d_lcs;
    return SBWTGPU_OK;
}
int lcs_ensure(const sbwtgpu_index *idx) {
    if (!idx) return fail(SBWTGPU_ERR_INVALID_ARG, "idx is NULL");
    if (idx->h.rank_only) return fail(SBWTGPU_ERR_INVALID_ARG, "%s", RANK_ONLY_MSG);
    std::lock_guard<std::mutex> lock(idx->lcs_mu);
    return lcs_build_locked(idx);
}
int ms_check_ptrs(const int64_t *first, const int64_t *second) {
    if ((first == nullptr) != (second == nullptr)) return fail(SBWTGPU_ERR_INVALID_ARG, "first and second must be both NULL or both non-NULL");
    return SBWTGPU_OK;
}
}  // namespace

int sbwtgpu_index_build_lcs(sbwtgpu_index *idx) { return lcs_ensure(idx); }

int sbwtgpu_index_get_lcs(const sbwtgpu_index *idx, uint8_t *out) {
    if (!out) return fail(SBWTGPU_ERR_INVALID_ARG, "out is NULL");
    int rc = lcs_ensure(idx);
    if (rc != SBWTGPU_OK) return rc;
    DeviceGuard guard(idx->device);
    HIP_TRY(hipMemcpy(out, idx->lcs, (size_t)idx->h.n_nodes, hipMemcpyDeviceToHost));
    return SBWTGPU_OK;
}

int64_t sbwtgpu_ms_workspace_bytes(int64_t total_bases) {
    (void)total_bases;
    return (int64_t)sizeof(SbwtMsWork);
}

int sbwtgpu_matching_statistics_dev(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases,
                                    const int64_t *d_read_off, int64_t n_reads, uint8_t *d_len, int64_t *d_first,
                                    int64_t *d_second, void *d_ws, int64_t ws_bytes, void *stream) {
    int rc = lcs_ensure(idx);
    if (rc != SBWTGPU_OK) return rc;
    if ((rc = ms_check_ptrs(d_first, d_second)) != SBWTGPU_OK) return rc;
    if (n_reads < 0 || total_bases < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative size");
    if (total_bases >= ((int64_t)1 << 36))
        return fail(SBWTGPU_ERR_INVALID_ARG, "more than 2^36 bases in one call: split the batch");
    if (!d_ws || ws_bytes < sbwtgpu_ms_workspace_bytes(total_bases))
        return fail(SBWTGPU_ERR_INVALID_ARG, "workspace missing or too small (%lld < %lld)", (long long)ws_bytes,
                    (long long)sbwtgpu_ms_workspace_bytes(total_bases));
    if (((uintptr_t)d_ws & 15) != 0) return fail(SBWTGPU_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
    if (n_reads > 0 && !d_read_off) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL device pointer");
    if (total_bases > 0 && (!d_bases || !d_len)) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL device pointer");
    DeviceGuard guard(idx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(d_ws, 0, sizeof(SbwtMsWork), st));
    if (g_poison && n_reads > 0 && total_bases > 0) {
        // len 0xFF is above every k, so a slot the kernel skips cannot pass for an answer
        int64_t b0 = 0;
        HIP_TRY(hipMemcpyAsync(&b0, d_read_off, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemsetAsync(d_len + b0, 0xFF, (size_t)total_bases, st));
        if (d_first) {
            HIP_TRY(hipMemsetAsync(d_first + b0, 0xA5, (size_t)total_bases * 8, st));
            HIP_TRY(hipMemsetAsync(d_second + b0, 0xA5, (size_t)total_bases * 8, st));
        }
    }
    sbwt_launch_ms(idx->view(), idx->lcs, d_bases, total_bases, reinterpret_cast<const long long *>(d_read_off), n_reads,
                   d_len, reinterpret_cast<long long *>(d_first), reinterpret_cast<long long *>(d_second),
                   static_cast<SbwtMsWork *>(d_ws), st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return SBWTGPU_OK;
}

int sbwtgpu_ms_workspace_stats(const void *d_ws, void *stream, int64_t stats[5]) {
    if (!d_ws || !stats) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    SbwtMsWork w;
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(&w, d_ws, sizeof(w), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    stats[0] = (int64_t)w.n_out;
    stats[1] = (int64_t)w.n_walk;
    stats[2] = (int64_t)w.n_full;
    stats[3] = (int64_t)w.n_contract;
    stats[4] = (int64_t)w.n_recompute;
    return SBWTGPU_OK;
}

int sbwtgpu_matching_statistics_batch(const sbwtgpu_index *idx, const char *bases, const int64_t *read_off,
                                      int64_t n_reads, uint8_t *len, int64_t *first, int64_t *second) {
    int rc = lcs_ensure(idx);
    if (rc != SBWTGPU_OK) return rc;
    if ((rc = ms_check_ptrs(first, second)) != SBWTGPU_OK) return rc;
    if (n_reads < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative n_reads");
    if (n_reads == 0) return SBWTGPU_OK;
    if (!read_off) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    for (int64_t r = 0; r < n_reads; r++)
        if ((rc = check_read_length(read_off, r)) != SBWTGPU_OK) return rc;
    const int64_t base0 = read_off[0], total = read_off[n_reads] - base0;
    if (total == 0) return SBWTGPU_OK;
    if (!bases || !len) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    DeviceGuard guard(idx->device);
    // [bases][read_off][len][first][second][workspace], every part 256-byte aligned
    const size_t o_off = align256((size_t)total + 8), o_len = o_off + align256((size_t)(n_reads + 1) * 8),
                 o_f = o_len + align256((size_t)total), o_s = o_f + (first ? align256((size_t)total * 8) : 0),
                 o_ws = o_s + (first ? align256((size_t)total * 8) : 0);
    const int64_t ws_bytes = sbwtgpu_ms_workspace_bytes(total);
    Staging sg;
    STG_TRY(sg.open(idx->device, o_ws + (size_t)ws_bytes));
    STG_TRY(sg.in(0, bases + base0, (size_t)total));
    STG_TRY(sg.in_rebased(o_off, read_off, n_reads + 1));
    STG_TRY(sg.upload());
    STG_TRY(sbwtgpu_matching_statistics_dev(idx, sg.at<const char>(0), total, sg.at<const int64_t>(o_off), n_reads, sg.at<uint8_t>(o_len),
                                            first ? sg.at<int64_t>(o_f) : nullptr, first ? sg.at<int64_t>(o_s) : nullptr,
                                            sg.at<char>(o_ws), ws_bytes, sg.stream));
    STG_TRY(sg.out(o_len, len + base0, (size_t)total));
    if (first) {
        STG_TRY(sg.out(o_f, first + base0, (size_t)total * 8));
        STG_TRY(sg.out(o_s, second + base0, (size_t)total * 8));
    }
    return sg.finish();
}

// ---- unitigs (sbwt_unitigs.hip) ---------------------------------------------------------------------
struct sbwtgpu_unitigs {
    int device = 0;
    int64_t k = 0;
    SbwtUnitigRun run;
    // a coloured handle (sbwtgpu_unitigs_create_colored): what its colour-set object said of itself
    bool colored = false;
    int64_t n_sets = 0;
    int n_colors = 0;
    // a graph handle (sbwtgpu_unitigs_create_graph): the SBWTGPU_UNITIGS_* flags it was made with, and what locate checks against
    unsigned graph = 0;
    int64_t n_nodes = 0;
    // the walks' start bitmap (sbwtgpu_unitigs_walks_prepare): one bit per column, made once from the
    // column map under the mutex and then only read
    mutable std::mutex walks_mutex;
    mutable std::atomic<unsigned long long *> d_walk_start{nullptr};
};

// the plain call, or with a colour view (ids, table, words) the coloured one; graph: SBWTGPU_UNITIGS_* flags
static int unitigs_create_common(const sbwtgpu_index *idx, const unsigned *d_ids, const unsigned long long *d_table, int words,
                                 int64_t n_sets, int n_colors, unsigned graph, sbwtgpu_unitigs **out) {
    if (idx->h.rank_only) return fail(SBWTGPU_ERR_INVALID_ARG, "%s", RANK_ONLY_MSG);
    if (idx->h.k < 2) return fail(SBWTGPU_ERR_INVALID_ARG, "unitigs need k >= 2");
    if (idx->h.n_nodes >= ((int64_t)1 << 32) - ((int64_t)1 << 24))
        return fail(SBWTGPU_ERR_INVALID_ARG, "unitigs: columns are 32-bit unsigned values (%lld columns)", (long long)idx->h.n_nodes);
    DeviceGuard guard(idx->device);
    sbwtgpu_unitigs *u = new (std::nothrow) sbwtgpu_unitigs();
    if (!u) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    u->device = idx->device;
    u->k = idx->h.k;
    u->colored = d_ids != nullptr;
    u->n_sets = n_sets;
    u->n_colors = n_colors;
    u->graph = graph;
    u->n_nodes = idx->h.n_nodes;
    DevBuf scratch;
    Stream st;
    hipError_t e = scratch.alloc((size_t)sbwt_unitigs_scratch_bytes(idx->h.n_nodes));
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking);
    if (e == hipSuccess)
        e = sbwt_unitigs_run(idx->view(), idx->h.has_ssup || idx->h.ssup_derived, scratch.p, &u->run, st.s, d_ids, d_table, words,
                             graph);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        delete u;
        return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "unitigs: %s", hipGetErrorString(e));
    }
    const int64_t nk = u->run.total_bases - u->run.n_unitigs * (u->k - 1);
    if (idx->h.n_kmers > 0 && nk != idx->h.n_kmers) {
        sbwtgpu_unitigs_destroy(u);
        return fail(SBWTGPU_ERR_INVALID_ARG, "unitigs: the index has %lld real columns, its n_kmers says %lld", (long long)nk,
                    (long long)idx->h.n_kmers);
    }
    *out = u;
    return SBWTGPU_OK;
}

int sbwtgpu_unitigs_create(const sbwtgpu_index *idx, sbwtgpu_unitigs **out) {
    if (!idx || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    return unitigs_create_common(idx, nullptr, nullptr, 0, 0, 0, 0u, out);
}

void sbwtgpu_unitigs_destroy(sbwtgpu_unitigs *u) {
    if (!u) return;
    DeviceGuard guard(u->device);
    if (u->run.d_bases) (void)hipFree(u->run.d_bases);
    if (u->run.d_off) (void)hipFree(u->run.d_off);
    if (u->run.d_first_col) (void)hipFree(u->run.d_first_col);
    if (u->run.d_set_id) (void)hipFree(u->run.d_set_id);
    if (u->run.d_link_off) (void)hipFree(u->run.d_link_off);
    if (u->run.d_link_to) (void)hipFree(u->run.d_link_to);
    if (u->run.d_col_unitig) (void)hipFree(u->run.d_col_unitig);
    if (u->run.d_col_offset) (void)hipFree(u->run.d_col_offset);
    if (u->d_walk_start.load()) (void)hipFree(u->d_walk_start.load());
    delete u;
}

int sbwtgpu_unitigs_info(const sbwtgpu_unitigs *u, int64_t *n_unitigs, int64_t *total_bases, int64_t *n_kmers) {
    if (!u) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    if (n_unitigs) *n_unitigs = u->run.n_unitigs;
    if (total_bases) *total_bases = u->run.total_bases;
    if (n_kmers) *n_kmers = u->run.total_bases - u->run.n_unitigs * (u->k - 1);
    return SBWTGPU_OK;
}

int sbwtgpu_unitigs_dev(const sbwtgpu_unitigs *u, const char **d_bases, const int64_t **d_off, const int64_t **d_first_col) {
    if (!u) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    if (d_bases) *d_bases = u->run.d_bases;
    if (d_off) *d_off = reinterpret_cast<const int64_t *>(u->run.d_off);
    if (d_first_col) *d_first_col = reinterpret_cast<const int64_t *>(u->run.d_first_col);
    return SBWTGPU_OK;
}

int sbwtgpu_unitigs_copy(const sbwtgpu_unitigs *u, char *bases, int64_t *off, int64_t *first_col) {
    if (!u || !off || (!bases && u->run.total_bases > 0)) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    DeviceGuard guard(u->device);
    if (u->run.total_bases > 0) HIP_TRY(hipMemcpy(bases, u->run.d_bases, (size_t)u->run.total_bases, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(off, u->run.d_off, (size_t)(u->run.n_unitigs + 1) * 8, hipMemcpyDeviceToHost));
    if (first_col && u->run.n_unitigs > 0)
        HIP_TRY(hipMemcpy(first_col, u->run.d_first_col, (size_t)u->run.n_unitigs * 8, hipMemcpyDeviceToHost));
    return SBWTGPU_OK;
}

int sbwtgpu_unitigs_stats(const sbwtgpu_unitigs *u, double pass_ms[6], int64_t *jump_rounds) {
    if (!u) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    if (pass_ms)
        for (int i = 0; i < SBWT_UT_N_PASSES; i++) pass_ms[i] = (double)u->run.ms[i];
    if (jump_rounds) *jump_rounds = u->run.jump_rounds;
    return SBWTGPU_OK;
}

static int unitigs_check_colored(const sbwtgpu_unitigs *u) {
    if (!u) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    if (!u->colored)
        return fail(SBWTGPU_ERR_INVALID_ARG, "unitigs: a handle of sbwtgpu_unitigs_create carries no colours (sbwtgpu_unitigs_create_colored does)");
    return SBWTGPU_OK;
}

int sbwtgpu_unitigs_set_ids_dev(const sbwtgpu_unitigs *u, const uint32_t **d_set_id) {
    const int rc = unitigs_check_colored(u);
    if (rc != SBWTGPU_OK) return rc;
    if (!d_set_id) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    *d_set_id = reinterpret_cast<const uint32_t *>(u->run.d_set_id);
    return SBWTGPU_OK;
}

int sbwtgpu_unitigs_set_ids_copy(const sbwtgpu_unitigs *u, uint32_t *set_id) {
    const int rc = unitigs_check_colored(u);
    if (rc != SBWTGPU_OK) return rc;
    if (!set_id && u->run.n_unitigs > 0) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    DeviceGuard guard(u->device);
    if (u->run.n_unitigs > 0) HIP_TRY(hipMemcpy(set_id, u->run.d_set_id, (size_t)u->run.n_unitigs * 4, hipMemcpyDeviceToHost));
    return SBWTGPU_OK;
}

int sbwtgpu_unitigs_color_info(const sbwtgpu_unitigs *u, int64_t *n_color_breaks, int64_t *n_sets, int32_t *n_colors) {
    const int rc = unitigs_check_colored(u);
    if (rc != SBWTGPU_OK) return rc;
    if (n_color_breaks) *n_color_breaks = u->run.n_color_breaks;
    if (n_sets) *n_sets = u->n_sets;
    if (n_colors) *n_colors = u->n_colors;
    return SBWTGPU_OK;
}

// ---- the unitig graph: links, column map, locate (sbwtgpu_unitigs_create_graph is with the colour sets) ----
static int unitigs_check_graph(const sbwtgpu_unitigs *u, unsigned need, const char *what) {
    if (!u) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    if (!(u->graph & need))
        return fail(SBWTGPU_ERR_INVALID_ARG, "unitigs: the handle was made without %s (sbwtgpu_unitigs_create_graph takes the flag)", what);
    return SBWTGPU_OK;
}

int sbwtgpu_unitigs_links_info(const sbwtgpu_unitigs *u, int64_t *n_links) {
    const int rc = unitigs_check_graph(u, SBWTGPU_UNITIGS_LINKS, "SBWTGPU_UNITIGS_LINKS");
    if (rc != SBWTGPU_OK) return rc;
    if (!n_links) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    *n_links = u->run.n_links;
    return SBWTGPU_OK;
}

int sbwtgpu_unitigs_links_dev(const sbwtgpu_unitigs *u, const int64_t **d_link_off, const uint32_t **d_link_to) {
    const int rc = unitigs_check_graph(u, SBWTGPU_UNITIGS_LINKS, "SBWTGPU_UNITIGS_LINKS");
    if (rc != SBWTGPU_OK) return rc;
    if (!d_link_off || !d_link_to) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    *d_link_off = reinterpret_cast<const int64_t *>(u->run.d_link_off);
    *d_link_to = reinterpret_cast<const uint32_t *>(u->run.d_link_to);
    return SBWTGPU_OK;
}

int sbwtgpu_unitigs_links_copy(const sbwtgpu_unitigs *u, int64_t *link_off, uint32_t *link_to) {
    const int rc = unitigs_check_graph(u, SBWTGPU_UNITIGS_LINKS, "SBWTGPU_UNITIGS_LINKS");
    if (rc != SBWTGPU_OK) return rc;
    if (!link_off || (!link_to && u->run.n_links > 0)) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    DeviceGuard guard(u->device);
    HIP_TRY(hipMemcpy(link_off, u->run.d_link_off, (size_t)(u->run.n_unitigs + 1) * 8, hipMemcpyDeviceToHost));
    if (u->run.n_links > 0) HIP_TRY(hipMemcpy(link_to, u->run.d_link_to, (size_t)u->run.n_links * 4, hipMemcpyDeviceToHost));
    return SBWTGPU_OK;
}

int sbwtgpu_unitigs_column_map_dev(const sbwtgpu_unitigs *u, const uint32_t **d_col_unitig, const uint32_t **d_col_offset) {
    const int rc = unitigs_check_graph(u, SBWTGPU_UNITIGS_COLUMN_MAP, "SBWTGPU_UNITIGS_COLUMN_MAP");
    if (rc != SBWTGPU_OK) return rc;
    if (!d_col_unitig || !d_col_offset) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    *d_col_unitig = reinterpret_cast<const uint32_t *>(u->run.d_col_unitig);
    *d_col_offset = reinterpret_cast<const uint32_t *>(u->run.d_col_offset);
    return SBWTGPU_OK;
}

int sbwtgpu_unitigs_column_map_copy(const sbwtgpu_unitigs *u, uint32_t *col_unitig, uint32_t *col_offset) {
    const int rc = unitigs_check_graph(u, SBWTGPU_UNITIGS_COLUMN_MAP, "SBWTGPU_UNITIGS_COLUMN_MAP");
    if (rc != SBWTGPU_OK) return rc;
    if (!col_unitig || !col_offset) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    DeviceGuard guard(u->device);
    HIP_TRY(hipMemcpy(col_unitig, u->run.d_col_unitig, (size_t)u->n_nodes * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(col_offset, u->run.d_col_offset, (size_t)u->n_nodes * 4, hipMemcpyDeviceToHost));
    return SBWTGPU_OK;
}

int sbwtgpu_unitigs_locate_dev(const sbwtgpu_unitigs *u, const int64_t *d_cols, int64_t n, uint32_t *d_unitig, uint32_t *d_offset,
                               void *stream) {
    const int rc = unitigs_check_graph(u, SBWTGPU_UNITIGS_COLUMN_MAP, "SBWTGPU_UNITIGS_COLUMN_MAP");
    if (rc != SBWTGPU_OK) return rc;
    if (n < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative n");
    if (n == 0) return SBWTGPU_OK;
    if (!d_cols || !d_unitig || !d_offset) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    DeviceGuard guard(u->device);
    HIP_TRY(sbwt_unitigs_locate(u->run.d_col_unitig, u->run.d_col_offset, u->n_nodes, reinterpret_cast<const long long *>(d_cols), n,
                                d_unitig, d_offset, static_cast<hipStream_t>(stream)));
    return SBWTGPU_OK;
}

int sbwtgpu_unitigs_locate_batch(const sbwtgpu_unitigs *u, const int64_t *cols, int64_t n, uint32_t *unitig, uint32_t *offset) {
    const int rc = unitigs_check_graph(u, SBWTGPU_UNITIGS_COLUMN_MAP, "SBWTGPU_UNITIGS_COLUMN_MAP");
    if (rc != SBWTGPU_OK) return rc;
    if (n < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative n");
    if (n == 0) return SBWTGPU_OK;
    if (!cols || !unitig || !offset) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    DeviceGuard guard(u->device);
    // [cols] in, [unitig][offset] back
    const size_t o_u = align256((size_t)n * 8), o_o = o_u + align256((size_t)n * 4);
    Staging sg;
    STG_TRY(sg.open(u->device, o_o + (size_t)n * 4));
    STG_TRY(sg.in(0, cols, (size_t)n * 8));
    STG_TRY(sg.upload());
    STG_TRY(sbwtgpu_unitigs_locate_dev(u, sg.at<const int64_t>(0), n, sg.at<uint32_t>(o_u), sg.at<uint32_t>(o_o), sg.stream));
    STG_TRY(sg.out(o_u, unitig, (size_t)n * 4));
    STG_TRY(sg.out(o_o, offset, (size_t)n * 4));
    return sg.finish();
}

int sbwtgpu_unitigs_graph_stats(const sbwtgpu_unitigs *u, double *links_ms, double *map_ms) {
    if (!u) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    if (links_ms) *links_ms = (double)u->run.links_ms;
    if (map_ms) *map_ms = (double)u->run.map_ms;
    return SBWTGPU_OK;
}

// ---- per-read hit profiles (sbwt_readhits.hip) --------------------------------------------------------
static_assert(sizeof(sbwtgpu_read_hits) == sizeof(SbwtReadHits), "the record of the ABI is the kernels' record");

int64_t sbwtgpu_read_hits_workspace_bytes(int64_t total_bases, int64_t n_reads, int strands) {
    if (total_bases < 0) total_bases = 0;
    if (n_reads < 0) n_reads = 0;
    return sbwt_rh_layout(sbwtgpu_search_workspace_bytes(total_bases), total_bases, n_reads, strands == 2 ? 2 : 1).total;
}

static int read_hits_check(const sbwtgpu_index *idx, int64_t n_reads, int strands) {
    if (!idx) return fail(SBWTGPU_ERR_INVALID_ARG, "idx is NULL");
    if (idx->h.rank_only) return fail(SBWTGPU_ERR_INVALID_ARG, "%s", RANK_ONLY_MSG);
    if (strands != 1 && strands != 2) return fail(SBWTGPU_ERR_INVALID_ARG, "strands must be 1 (forward) or 2 (either strand), not %d", strands);
    if (n_reads < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative n_reads");
    if (n_reads >= ((int64_t)1 << 31)) return fail(SBWTGPU_ERR_INVALID_ARG, "2^31 reads or more in one call: split the batch");
    return SBWTGPU_OK;
}

int sbwtgpu_read_hits_dev(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                          int64_t n_reads, int strands, sbwtgpu_read_hits *d_out, void *d_ws, int64_t ws_bytes, void *stream) {
    int rc = read_hits_check(idx, n_reads, strands);
    if (rc != SBWTGPU_OK) return rc;
    if (total_bases < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative size");
    if (total_bases >= ((int64_t)1 << 36))
        return fail(SBWTGPU_ERR_INVALID_ARG, "more than 2^36 bases in one call: split the batch");
    const int64_t need = sbwtgpu_read_hits_workspace_bytes(total_bases, n_reads, strands);
    if (!d_ws || ws_bytes < need)
        return fail(SBWTGPU_ERR_INVALID_ARG, "workspace missing or too small (%lld < %lld)", (long long)ws_bytes, (long long)need);
    if (((uintptr_t)d_ws & 15) != 0) return fail(SBWTGPU_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
    if (n_reads == 0) return SBWTGPU_OK;
    if (!d_read_off || !d_out || (total_bases > 0 && !d_bases)) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL device pointer");
    DeviceGuard guard(idx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t search_ws = sbwtgpu_search_workspace_bytes(total_bases);
    const SbwtRhLayout L = sbwt_rh_layout(search_ws, total_bases, n_reads, strands);
    char *w = static_cast<char *>(d_ws);
    SbwtRhHeader *hdr = reinterpret_cast<SbwtRhHeader *>(w + L.hdr);
    int64_t *res = reinterpret_cast<int64_t *>(w + L.res);
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(w + L.bits);
    long long *ooff = reinterpret_cast<long long *>(w + L.ooff);
    // int32 results where the index allows them: half the bytes written and read back ("read_hits_wide": tests of the other)
    const int wide = (idx->h.n_nodes >= ((int64_t)1 << 31) || g_rh_wide) ? 1 : 0;
    const int k = (int)idx->h.k;
    HIP_TRY(hipMemsetAsync(hdr, 0, sizeof(SbwtRhHeader), st));
    if (g_poison) HIP_TRY(hipMemsetAsync(d_out, 0xA5, (size_t)n_reads * sizeof(sbwtgpu_read_hits), st));
    sbwt_launch_rh_offsets(reinterpret_cast<const long long *>(d_read_off), n_reads, k, reinterpret_cast<long long *>(w + L.cnt),
                           reinterpret_cast<long long *>(w + L.bsum), ooff, st);
    // (a batch of fewer than k bases has no window: nothing to search and no bit to write -- the reducer reads no word of
    // the bit vector for a read without windows -- and the records are zeros)
    const bool any = total_bases >= k;
    const SbwtWorkHeader *sws = reinterpret_cast<const SbwtWorkHeader *>(w);
    if (any) {
        t_out32 = wide ? 0 : 1;
        rc = search_dev_common(idx, d_bases, total_bases, d_read_off, n_reads, res, reinterpret_cast<const int64_t *>(ooff), d_ws,
                               search_ws, stream, 0);
        t_out32 = 0;
        if (rc != SBWTGPU_OK) return rc;
        sbwt_launch_rh_bits(res, wide, ooff, n_reads, total_bases, 0, bits, sws, hdr, st);
    }
    if (strands == 2 && any) {
        char *rcb = w + L.rc;
        long long *roff2 = reinterpret_cast<long long *>(w + L.roff2), *ooff2 = reinterpret_cast<long long *>(w + L.ooff2);
        sbwt_launch_rh_mirror(d_bases, total_bases, reinterpret_cast<const long long *>(d_read_off), ooff, n_reads, rcb, roff2, ooff2, st);
        t_out32 = wide ? 0 : 1;
        rc = search_dev_common(idx, rcb, total_bases, reinterpret_cast<const int64_t *>(roff2), n_reads, res,
                               reinterpret_cast<const int64_t *>(ooff2), d_ws, search_ws, stream, 0);
        t_out32 = 0;
        if (rc != SBWTGPU_OK) return rc;
        sbwt_launch_rh_bits(res, wide, ooff, n_reads, total_bases, 1, bits, sws, hdr, st);
    }
    sbwt_launch_rh_reduce(bits, ooff, n_reads, k, g_rh_wave_min, reinterpret_cast<SbwtReadHits *>(d_out), st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return SBWTGPU_OK;
}

// Host buffers: the batch is cut into chunks of whole reads of at most "read_hits_chunk_bases" bases (a chunk always takes
// one read), two chunks in flight on the parked slots of the search pipeline.  Bases and offsets go down, records come back.
int sbwtgpu_read_hits_batch(const sbwtgpu_index *idx, const char *bases, const int64_t *read_off, int64_t n_reads, int strands,
                            sbwtgpu_read_hits *out) {
    int rc = read_hits_check(idx, n_reads, strands);
    if (rc != SBWTGPU_OK) return rc;
    if (n_reads == 0) return SBWTGPU_OK;
    if (!read_off || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    if (read_off[n_reads] > read_off[0] && !bases) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    const int64_t budget = g_rh_chunk_bases > 0 ? g_rh_chunk_bases : (int64_t)64 << 20, CH_READS = (int64_t)1 << 24;
    std::vector<int64_t> cuts{0};
    int64_t max_bases = 0, max_reads = 0;
    try {
        for (int64_t lo = 0, r = 0; r < n_reads; r++) {
            if ((rc = check_read_length(read_off, r)) != SBWTGPU_OK) return rc;
            if (r > lo && (read_off[r + 1] - read_off[lo] > budget || r - lo >= CH_READS)) {
                cuts.push_back(r);
                lo = r;
            }
            max_bases = std::max(max_bases, read_off[r + 1] - read_off[lo]);
            max_reads = std::max(max_reads, r + 1 - lo);
        }
        cuts.push_back(n_reads);
    } catch (const std::bad_alloc &) {
        return fail(SBWTGPU_ERR_OOM, "out of host memory");
    }
    const int64_t n_chunks = (int64_t)cuts.size() - 1;
    const bool pin_in = is_pinned(bases), pin_out = is_pinned(out);
    const int64_t ws_bytes = sbwtgpu_read_hits_workspace_bytes(max_bases, max_reads, strands);
    const int64_t need_in = align256(max_bases + 16) + align256((max_reads + 1) * 8);
    const int64_t need_out = pin_out ? 0 : align256(max_reads * 16);
    const int64_t need_dev = align256(max_bases + 16) + align256((max_reads + 1) * 8) + align256(max_reads * 16) + align256(ws_bytes);
    DeviceGuard guard(idx->device);
    const int n_slots = n_chunks > 1 ? 2 : 1;
    PipeSlot S[2];
    if ((rc = take_slots(idx->device, S, n_slots, need_in, need_out, need_dev, "read-hits buffers")) != SBWTGPU_OK) return rc;
    int bug = 0;                    // the first nonzero device status of a chunk
    const int64_t o_roff = align256(max_bases + 16), o_rec = o_roff + align256((max_reads + 1) * 8), o_ws = o_rec + align256(max_reads * 16);
    auto submit = [&](int64_t c) -> int {
        PipeSlot &P = S[c % n_slots];
        const int64_t lo = cuts[(size_t)c], hi = cuts[(size_t)c + 1], nr = hi - lo, nb = read_off[hi] - read_off[lo];
        int64_t *hro = (int64_t *)(P.h_in + align256(max_bases + 16));
        for (int64_t r = 0; r <= nr; r++) hro[r] = read_off[lo + r] - read_off[lo];
        const char *hb = bases + read_off[lo];
        if (!pin_in && nb > 0) { parallel_memcpy(P.h_in, hb, (size_t)nb); hb = P.h_in; }
        hipError_t e;
        if ((nb > 0 && (e = hipMemcpyAsync(P.d_mem, hb, (size_t)nb, hipMemcpyHostToDevice, P.st)) != hipSuccess) ||
            (e = hipMemcpyAsync(P.d_mem + o_roff, hro, (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, P.st)) != hipSuccess)
            return fail(SBWTGPU_ERR_HIP, "H2D copy: %s", hipGetErrorString(e));
        const int r2 = sbwtgpu_read_hits_dev(idx, P.d_mem, nb, (const int64_t *)(P.d_mem + o_roff), nr, strands,
                                             (sbwtgpu_read_hits *)(P.d_mem + o_rec), P.d_mem + o_ws, ws_bytes, P.st);
        if (r2 != SBWTGPU_OK) return r2;
        const SbwtRhLayout L = sbwt_rh_layout(sbwtgpu_search_workspace_bytes(nb), nb, nr, strands);
        char *target = pin_out ? (char *)(out + lo) : P.h_out;
        if ((e = hipMemcpyAsync(target, P.d_mem + o_rec, (size_t)nr * 16, hipMemcpyDeviceToHost, P.st)) != hipSuccess ||
            (e = hipMemcpyAsync(P.h_status, P.d_mem + o_ws + L.hdr, 4, hipMemcpyDeviceToHost, P.st)) != hipSuccess)
            return fail(SBWTGPU_ERR_HIP, "D2H copy: %s", hipGetErrorString(e));
        return SBWTGPU_OK;
    };
    auto collect = [&](int64_t c) -> int {
        PipeSlot &P = S[c % n_slots];
        hipError_t e = hipStreamSynchronize(P.st);
        if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "stream synchronize: %s", hipGetErrorString(e));
        if (P.h_status[0] != 0 && bug == 0) bug = P.h_status[0];
        const int64_t lo = cuts[(size_t)c], hi = cuts[(size_t)c + 1];
        if (!pin_out) memcpy(out + lo, P.h_out, (size_t)(hi - lo) * 16);
        return SBWTGPU_OK;
    };
    rc = two_in_flight(n_chunks, submit, collect);
    park_slots(idx->device, S, n_slots, rc);
    if (rc != SBWTGPU_OK) return rc;
    if (bug) return fail_status(bug);
    return SBWTGPU_OK;
}

// ---- reads threaded through the unitig graph (sbwt_walks.hip) -----------------------
static_assert(sizeof(sbwtgpu_walk_step) == sizeof(SbwtWalkStep), "the record of the ABI is the kernels' record");

int sbwtgpu_unitigs_walks_prepare(sbwtgpu_unitigs *u) {
    const int rc = unitigs_check_graph(u, SBWTGPU_UNITIGS_COLUMN_MAP, "SBWTGPU_UNITIGS_COLUMN_MAP");
    if (rc != SBWTGPU_OK) return rc;
    if (u->d_walk_start.load(std::memory_order_acquire)) return SBWTGPU_OK;
    std::lock_guard<std::mutex> lock(u->walks_mutex);
    if (u->d_walk_start.load(std::memory_order_acquire)) return SBWTGPU_OK;
    DeviceGuard guard(u->device);
    DevBuf bits;
    Stream st;
    hipError_t e = bits.alloc((size_t)((u->n_nodes + 63) / 64 + 1) * 8);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking);
    if (e == hipSuccess) {
        sbwt_launch_walk_startbits(u->run.d_col_offset, u->n_nodes, static_cast<unsigned long long *>(bits.p), st.s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st.s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "walks: start bitmap: %s", hipGetErrorString(e));
    }
    u->d_walk_start.store(static_cast<unsigned long long *>(bits.p), std::memory_order_release);
    bits.p = nullptr;
    return SBWTGPU_OK;
}

int64_t sbwtgpu_unitigs_walks_workspace_bytes(int64_t total_bases, int64_t n_reads) {
    if (total_bases < 0) total_bases = 0;
    if (n_reads < 0) n_reads = 0;
    return sbwt_walk_layout(sbwtgpu_search_workspace_bytes(total_bases), total_bases, n_reads).total;
}

static int walks_check(const sbwtgpu_index *idx, const sbwtgpu_unitigs *u, int64_t n_reads) {
    if (!idx) return fail(SBWTGPU_ERR_INVALID_ARG, "idx is NULL");
    if (!u) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    // (the size first, as the colour layer does: an index of that size is refused for it whatever else is wrong with the call)
    if (idx->h.n_nodes >= ((int64_t)1 << 31))
        return fail(SBWTGPU_ERR_INVALID_ARG, "walks: the index has %lld columns, the walks read int32 search results (fewer than 2^31 columns)",
                    (long long)idx->h.n_nodes);
    int rc = unitigs_check_graph(u, SBWTGPU_UNITIGS_COLUMN_MAP, "SBWTGPU_UNITIGS_COLUMN_MAP");
    if (rc != SBWTGPU_OK) return rc;
    if (idx->h.rank_only) return fail(SBWTGPU_ERR_INVALID_ARG, "%s", RANK_ONLY_MSG);
    if (u->n_nodes != idx->h.n_nodes || u->k != idx->h.k || u->device != idx->device)
        return fail(SBWTGPU_ERR_INVALID_ARG, "walks: the handle (%lld columns, k = %lld, device %d) was not made from this index (%lld columns, k = %lld, device %d)",
                    (long long)u->n_nodes, (long long)u->k, u->device, (long long)idx->h.n_nodes, (long long)idx->h.k, idx->device);
    if (n_reads < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative n_reads");
    if (n_reads >= ((int64_t)1 << 31)) return fail(SBWTGPU_ERR_INVALID_ARG, "2^31 reads or more in one call: split the batch");
    return SBWTGPU_OK;
}

int sbwtgpu_unitigs_walks_dev(const sbwtgpu_index *idx, const sbwtgpu_unitigs *u, const char *d_bases, int64_t total_bases,
                              const int64_t *d_read_off, int64_t n_reads, int64_t *d_step_off, sbwtgpu_walk_step *d_steps,
                              int64_t steps_cap, int64_t *d_unitig_kmers, void *d_ws, int64_t ws_bytes, void *stream) {
    int rc = walks_check(idx, u, n_reads);
    if (rc != SBWTGPU_OK) return rc;
    if (steps_cap < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative steps_cap");
    if (total_bases < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative size");
    if (total_bases >= ((int64_t)1 << 36))
        return fail(SBWTGPU_ERR_INVALID_ARG, "more than 2^36 bases in one call: split the batch");
    const unsigned long long *start = u->d_walk_start.load(std::memory_order_acquire);
    if (!start)
        return fail(SBWTGPU_ERR_INVALID_ARG, "walks: the handle is not prepared (sbwtgpu_unitigs_walks_prepare builds its start bitmap)");
    const int64_t need = sbwtgpu_unitigs_walks_workspace_bytes(total_bases, n_reads);
    if (!d_ws || ws_bytes < need)
        return fail(SBWTGPU_ERR_INVALID_ARG, "workspace missing or too small (%lld < %lld)", (long long)ws_bytes, (long long)need);
    if (((uintptr_t)d_ws & 15) != 0) return fail(SBWTGPU_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
    if (!d_step_off || (steps_cap > 0 && !d_steps)) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL device pointer");
    DeviceGuard guard(idx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_reads == 0) {
        HIP_TRY(hipMemsetAsync(d_step_off, 0, 8, st));
        return SBWTGPU_OK;
    }
    if (!d_read_off || (total_bases > 0 && !d_bases)) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL device pointer");
    const int64_t search_ws = sbwtgpu_search_workspace_bytes(total_bases);
    const SbwtWalkLayout L = sbwt_walk_layout(search_ws, total_bases, n_reads);
    char *w = static_cast<char *>(d_ws);
    int32_t *res = reinterpret_cast<int32_t *>(w + L.res);
    long long *ooff = reinterpret_cast<long long *>(w + L.ooff);
    const int k = (int)idx->h.k;
    sbwt_launch_rh_offsets(reinterpret_cast<const long long *>(d_read_off), n_reads, k, reinterpret_cast<long long *>(w + L.cnt),
                           reinterpret_cast<long long *>(w + L.bsum), ooff, st);
    // (a batch of fewer than k bases has no window: nothing to search, W = 0 and no pass below reads a result; the status
    // word that sbwtgpu_workspace_status looks at is then cleared here)
    if (total_bases >= k) {
        rc = search_dev_i32(idx, d_bases, total_bases, d_read_off, n_reads, res, reinterpret_cast<const int64_t *>(ooff), d_ws, search_ws,
                            stream, 0);
        if (rc != SBWTGPU_OK) return rc;
    } else {
        HIP_TRY(hipMemsetAsync(d_ws, 0, sizeof(SbwtWorkHeader), st));
    }
    const hipError_t e = sbwt_launch_walks(res, ooff, n_reads, total_bases, start, u->run.d_col_unitig, u->run.d_col_offset, u->n_nodes, w, L,
                                           reinterpret_cast<long long *>(d_step_off), reinterpret_cast<SbwtWalkStep *>(d_steps), steps_cap,
                                           reinterpret_cast<long long *>(d_unitig_kmers), st);
    if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "walks passes: %s", hipGetErrorString(e));
    return SBWTGPU_OK;
}

// Host buffers: the batch is cut into chunks of whole reads of at most "walks_chunk_bases" bases (a chunk always takes one
// read), one after the other on a parked slot of the search pipeline: a chunk's step count decides how many records come
// back, so its offsets are read before its records are fetched.  step_off is stitched: a chunk's offsets plus the steps of
// the chunks before it.
int sbwtgpu_unitigs_walks_batch(const sbwtgpu_index *idx, const sbwtgpu_unitigs *u, const char *bases, const int64_t *read_off,
                                int64_t n_reads, int64_t *step_off, sbwtgpu_walk_step **steps_out, int64_t *n_steps,
                                int64_t *unitig_kmers) {
    int rc = walks_check(idx, u, n_reads);
    if (rc != SBWTGPU_OK) return rc;
    if (!step_off || !steps_out || !n_steps) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    *steps_out = nullptr;
    *n_steps = 0;
    step_off[0] = 0;
    const int64_t n_unitigs = u->run.n_unitigs;
    if (unitig_kmers && n_unitigs > 0) memset(unitig_kmers, 0, (size_t)n_unitigs * 8);
    if (n_reads == 0) return SBWTGPU_OK;
    if (!read_off) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    if (read_off[n_reads] > read_off[0] && !bases) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    if ((rc = sbwtgpu_unitigs_walks_prepare(const_cast<sbwtgpu_unitigs *>(u))) != SBWTGPU_OK) return rc;
    const int64_t budget = g_wk_chunk_bases > 0 ? g_wk_chunk_bases : (int64_t)64 << 20, CH_READS = (int64_t)1 << 24, k = idx->h.k;
    std::vector<int64_t> cuts{0};
    int64_t max_bases = 0, max_reads = 0, max_windows = 0, windows = 0;
    try {
        for (int64_t lo = 0, r = 0; r < n_reads; r++) {
            if ((rc = check_read_length(read_off, r)) != SBWTGPU_OK) return rc;
            if (r > lo && (read_off[r + 1] - read_off[lo] > budget || r - lo >= CH_READS)) {
                cuts.push_back(r);
                lo = r;
                windows = 0;
            }
            windows += std::max<int64_t>(0, read_off[r + 1] - read_off[r] - k + 1);
            max_bases = std::max(max_bases, read_off[r + 1] - read_off[lo]);
            max_reads = std::max(max_reads, r + 1 - lo);
            max_windows = std::max(max_windows, windows);
        }
        cuts.push_back(n_reads);
    } catch (const std::bad_alloc &) {
        return fail(SBWTGPU_ERR_OOM, "out of host memory");
    }
    const int64_t n_chunks = (int64_t)cuts.size() - 1;
    const bool pin_in = is_pinned(bases);
    const int64_t ws_bytes = sbwtgpu_unitigs_walks_workspace_bytes(max_bases, max_reads);
    // device: [bases][read_off][step_off][coverage][steps][workspace]; pinned: bases and offsets down, step_off (and coverage) back
    const int64_t o_roff = align256(max_bases + 16), o_soff = o_roff + align256((max_reads + 1) * 8),
                  o_cov = o_soff + align256((max_reads + 1) * 8), o_steps = o_cov + (unitig_kmers ? align256(n_unitigs * 8 + 8) : 0),
                  o_ws = o_steps + align256(max_windows * 16 + 16), need_dev = o_ws + align256(ws_bytes);
    const int64_t need_in = o_soff, need_out = align256((max_reads + 1) * 8);
    DeviceGuard guard(idx->device);
    PipeSlot S[1];
    if ((rc = take_slots(idx->device, S, 1, need_in, need_out, need_dev, "walks buffers")) != SBWTGPU_OK) return rc;
    PipeSlot &P = S[0];
    int bug = 0;                    // the first nonzero device status of a chunk
    sbwtgpu_walk_step *steps = nullptr;
    int64_t total = 0, cap = 0;
    auto run = [&]() -> int {
        hipError_t e;
        if (unitig_kmers && n_unitigs > 0 && (e = hipMemsetAsync(P.d_mem + o_cov, 0, (size_t)n_unitigs * 8, P.st)) != hipSuccess)
            return fail(SBWTGPU_ERR_HIP, "memset: %s", hipGetErrorString(e));
        for (int64_t c = 0; c < n_chunks; c++) {
            const int64_t lo = cuts[(size_t)c], hi = cuts[(size_t)c + 1], nr = hi - lo, nb = read_off[hi] - read_off[lo];
            int64_t *hro = (int64_t *)(P.h_in + o_roff);
            for (int64_t r = 0; r <= nr; r++) hro[r] = read_off[lo + r] - read_off[lo];
            const char *hb = bases + read_off[lo];
            if (!pin_in && nb > 0) { parallel_memcpy(P.h_in, hb, (size_t)nb); hb = P.h_in; }
            if ((nb > 0 && (e = hipMemcpyAsync(P.d_mem, hb, (size_t)nb, hipMemcpyHostToDevice, P.st)) != hipSuccess) ||
                (e = hipMemcpyAsync(P.d_mem + o_roff, hro, (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, P.st)) != hipSuccess)
                return fail(SBWTGPU_ERR_HIP, "H2D copy: %s", hipGetErrorString(e));
            const int r2 = sbwtgpu_unitigs_walks_dev(idx, u, P.d_mem, nb, (const int64_t *)(P.d_mem + o_roff), nr, (int64_t *)(P.d_mem + o_soff),
                                                     (sbwtgpu_walk_step *)(P.d_mem + o_steps), max_windows,
                                                     unitig_kmers ? (int64_t *)(P.d_mem + o_cov) : nullptr, P.d_mem + o_ws, ws_bytes, P.st);
            if (r2 != SBWTGPU_OK) return r2;
            if ((e = hipMemcpyAsync(P.h_out, P.d_mem + o_soff, (size_t)(nr + 1) * 8, hipMemcpyDeviceToHost, P.st)) != hipSuccess ||
                (e = hipMemcpyAsync(P.h_status, P.d_mem + o_ws + offsetof(SbwtWorkHeader, status), 4, hipMemcpyDeviceToHost, P.st)) != hipSuccess ||
                (e = hipStreamSynchronize(P.st)) != hipSuccess)
                return fail(SBWTGPU_ERR_HIP, "D2H copy: %s", hipGetErrorString(e));
            if (P.h_status[0] != 0 && bug == 0) bug = P.h_status[0];
            const int64_t *so = (const int64_t *)P.h_out, ns = so[nr];
            for (int64_t r = 1; r <= nr; r++) step_off[lo + r] = total + so[r];
            if (ns > 0) {
                if (total + ns > cap) {
                    const int64_t want = std::max(total + ns, cap + cap / 2);
                    void *q = realloc(steps, (size_t)want * sizeof(sbwtgpu_walk_step));
                    if (!q) return fail(SBWTGPU_ERR_OOM, "out of host memory");
                    steps = static_cast<sbwtgpu_walk_step *>(q);
                    cap = want;
                }
                if ((e = hipMemcpyAsync(steps + total, P.d_mem + o_steps, (size_t)ns * sizeof(sbwtgpu_walk_step), hipMemcpyDeviceToHost, P.st)) != hipSuccess ||
                    (e = hipStreamSynchronize(P.st)) != hipSuccess)
                    return fail(SBWTGPU_ERR_HIP, "D2H copy: %s", hipGetErrorString(e));
                total += ns;
            }
        }
        if (unitig_kmers && n_unitigs > 0 &&
            ((e = hipMemcpyAsync(unitig_kmers, P.d_mem + o_cov, (size_t)n_unitigs * 8, hipMemcpyDeviceToHost, P.st)) != hipSuccess ||
             (e = hipStreamSynchronize(P.st)) != hipSuccess))
            return fail(SBWTGPU_ERR_HIP, "D2H copy: %s", hipGetErrorString(e));
        return SBWTGPU_OK;
    };
    rc = run();
    park_slots(idx->device, S, 1, rc);
    if (rc == SBWTGPU_OK && bug) rc = fail_status(bug);
    if (rc != SBWTGPU_OK) {
        free(steps);
        return rc;
    }
    *steps_out = steps;
    *n_steps = total;
    return SBWTGPU_OK;
}

// ---- colours and pseudoalignment (sbwt_colors.hip) ----------------------------------------------------
static_assert(sizeof(sbwtgpu_pseudoalignment) == sizeof(SbwtPseudoalignment), "the record of the ABI is the kernels' record");
static_assert(sizeof(sbwtgpu_read_found) == sizeof(SbwtReadFound), "the wide record of the ABI is the kernels' record");

struct sbwtgpu_colors {
    const sbwtgpu_index *idx = nullptr;
    int device = 0;
    int64_t n_nodes = 0, k = 0;
    int n_colors = 0;
    int words = 1;                      // 64-bit words per row: ceil(n_colors / 64)
    unsigned long long *d_rows = nullptr;
};
// deduplicated colour sets (sbwt_colorsets.hip): `base` binds the object to its index as a colours object is bound (no rows)
struct sbwtgpu_colorsets {
    sbwtgpu_colors base;
    int64_t n_sets = 0, n_colored = 0;
    unsigned *d_ids = nullptr;
    unsigned long long *d_table = nullptr;
};

// a colour-set builder (sbwt_colorsets.hip, "the builder"): `base` binds it to its index; a colour is new, open or closed
struct sbwtgpu_colorsets_builder {
    sbwtgpu_colors base;
    SbwtCsbState st;
    Stream stream;                      // of the closes and of finish, for the builder's life: a stream costs milliseconds to make
    std::vector<unsigned char> state;   // per colour: CSB_NEW, CSB_OPEN, CSB_CLOSED
    std::vector<int64_t> per_color;     // the columns marked when the colour was closed
    int open = -1;                      // the open colour, or -1
    bool finished = false, broken = false;
};
enum { CSB_NEW = 0, CSB_OPEN = 1, CSB_CLOSED = 2 };

static int colors_check_index(const sbwtgpu_index *idx) {
    if (idx->h.n_nodes >= ((int64_t)1 << 31))
        return fail(SBWTGPU_ERR_INVALID_ARG, "colours: the index has %lld columns, the colour layer reads int32 search results (fewer than 2^31 columns)",
                    (long long)idx->h.n_nodes);
    if (idx->h.rank_only) return fail(SBWTGPU_ERR_INVALID_ARG, "%s", RANK_ONLY_MSG);
    return SBWTGPU_OK;
}
// the object and the index it was made for still agree (a colours object is bound to its index at creation)
static int colors_check(const sbwtgpu_colors *c) {
    if (!c || !c->idx) return fail(SBWTGPU_ERR_INVALID_ARG, "colours object is NULL");
    if (c->idx->h.n_nodes != c->n_nodes || c->idx->h.k != c->k)
        return fail(SBWTGPU_ERR_INVALID_ARG, "colours of %lld columns at k = %lld used with an index of %lld columns at k = %lld",
                    (long long)c->n_nodes, (long long)c->k, (long long)c->idx->h.n_nodes, (long long)c->idx->h.k);
    return colors_check_index(c->idx);
}
static int colors_check_batch(int64_t n_reads, int strands) {
    if (strands != 1 && strands != 2) return fail(SBWTGPU_ERR_INVALID_ARG, "strands must be 1 (forward) or 2 (either strand), not %d", strands);
    if (n_reads < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative n_reads");
    if (n_reads >= ((int64_t)1 << 31)) return fail(SBWTGPU_ERR_INVALID_ARG, "2^31 reads or more in one call: split the batch");
    return SBWTGPU_OK;
}
static int colors_check_query(int threshold_ppm, int denominator) {
    if (threshold_ppm < 1 || threshold_ppm > 1000000)
        return fail(SBWTGPU_ERR_INVALID_ARG, "threshold_ppm must be in 1 .. 1000000, not %d", threshold_ppm);
    if (denominator != 0 && denominator != 1)
        return fail(SBWTGPU_ERR_INVALID_ARG, "denominator must be 0 (the found k-mers) or 1 (all k-mers), not %d", denominator);
    return SBWTGPU_OK;
}

// what both creates do once n_colors has passed their own bound
static int colors_create_checked(const sbwtgpu_index *idx, int n_colors, const uint64_t *rows_or_null, sbwtgpu_colors **out) {
    DeviceGuard guard(idx->device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", idx->device);
    sbwtgpu_colors *c = new (std::nothrow) sbwtgpu_colors();
    if (!c) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    c->idx = idx;
    c->device = idx->device;
    c->n_nodes = idx->h.n_nodes;
    c->k = idx->h.k;
    c->n_colors = n_colors;
    c->words = (n_colors + 63) / 64;
    const size_t bytes = (size_t)c->n_nodes * (size_t)c->words * 8;
    Stream st;
    hipError_t e = hipMalloc((void **)&c->d_rows, bytes ? bytes : 16);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking);
    if (e == hipSuccess && !rows_or_null) e = hipMemsetAsync(c->d_rows, 0, bytes, st.s);
    if (e == hipSuccess && rows_or_null) e = hipMemcpyAsync(c->d_rows, rows_or_null, bytes, hipMemcpyHostToDevice, st.s);
    if (e == hipSuccess) e = rows_or_null ? sbwt_colors_clean(idx->view(), c->d_rows, n_colors, st.s) : hipStreamSynchronize(st.s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        sbwtgpu_colors_destroy(c);
        return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "colours: %s", hipGetErrorString(e));
    }
    *out = c;
    return SBWTGPU_OK;
}

int sbwtgpu_colors_create(const sbwtgpu_index *idx, int n_colors, const uint64_t *rows_or_null, sbwtgpu_colors **out) {
    if (!idx || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    int rc = colors_check_index(idx);
    if (rc != SBWTGPU_OK) return rc;
    if (n_colors < 1 || n_colors > 64)
        return fail(SBWTGPU_ERR_INVALID_ARG,
                    "n_colors must be in 1 .. 64, not %d (more than 64 colours are out of scope here: sbwtgpu_colors_create_wide takes up to %d)",
                    n_colors, SBWTGPU_MAX_COLORS);
    return colors_create_checked(idx, n_colors, rows_or_null, out);
}

int sbwtgpu_colors_create_wide(const sbwtgpu_index *idx, int n_colors, const uint64_t *rows_or_null, sbwtgpu_colors **out) {
    if (!idx || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    int rc = colors_check_index(idx);
    if (rc != SBWTGPU_OK) return rc;
    if (n_colors < 1 || n_colors > SBWTGPU_MAX_COLORS)
        return fail(SBWTGPU_ERR_INVALID_ARG, "n_colors must be in 1 .. %d, not %d", SBWTGPU_MAX_COLORS, n_colors);
    return colors_create_checked(idx, n_colors, rows_or_null, out);
}

int sbwtgpu_colors_words(const sbwtgpu_colors *c) { return c ? c->words : 0; }

void sbwtgpu_colors_destroy(sbwtgpu_colors *c) {
    if (!c) return;
    DeviceGuard guard(c->device);
    if (c->d_rows) (void)hipFree(c->d_rows);
    delete c;
}

// h: 64 words + 1 entries -- the coloured columns per colour, then those of any colour
static int colors_stats(const sbwtgpu_colors *c, unsigned long long *h) {
    const size_t bytes = ((size_t)c->words * 64 + 1) * 8;
    DeviceGuard guard(c->device);
    DevBuf stats;
    Stream st;
    HIP_TRY(stats.alloc(bytes));
    HIP_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    HIP_TRY(hipMemsetAsync(stats.p, 0, bytes, st.s));
    sbwt_launch_col_stats(c->d_rows, c->n_nodes, c->words, static_cast<unsigned long long *>(stats.p), st.s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, stats.p, bytes, hipMemcpyDeviceToHost, st.s));
    HIP_TRY(hipStreamSynchronize(st.s));
    return SBWTGPU_OK;
}

int sbwtgpu_colors_info(const sbwtgpu_colors *c, sbwtgpu_colors_info_t *info) {
    if (!c || !info) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    memset(info, 0, sizeof(*info));
    if (c->n_colors > 64)
        return fail(SBWTGPU_ERR_INVALID_ARG, "the colours object has %d colours, sbwtgpu_colors_info_t holds 64: use sbwtgpu_colors_info_wide",
                    c->n_colors);
    info->n_columns = c->n_nodes;
    info->k = c->k;
    info->n_colors = c->n_colors;
    unsigned long long h[65];
    const int rc = colors_stats(c, h);
    if (rc != SBWTGPU_OK) return rc;
    for (int i = 0; i < 64; i++) info->per_color[i] = (int64_t)h[i];
    info->n_colored_columns = (int64_t)h[64];
    return SBWTGPU_OK;
}

int sbwtgpu_colors_info_wide(const sbwtgpu_colors *c, int64_t *n_columns, int64_t *k, int32_t *n_colors, int64_t *n_colored_columns,
                             int64_t *per_color) {
    if (!c) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    if (n_columns) *n_columns = c->n_nodes;
    if (k) *k = c->k;
    if (n_colors) *n_colors = c->n_colors;
    if (!n_colored_columns && !per_color) return SBWTGPU_OK;
    unsigned long long h[SBWTGPU_MAX_COLORS + 1];
    const int rc = colors_stats(c, h);
    if (rc != SBWTGPU_OK) return rc;
    if (per_color)
        for (int i = 0; i < c->n_colors; i++) per_color[i] = (int64_t)h[i];
    if (n_colored_columns) *n_colored_columns = (int64_t)h[(size_t)c->words * 64];
    return SBWTGPU_OK;
}

int sbwtgpu_colors_copy(const sbwtgpu_colors *c, uint64_t *rows_out) {
    if (!c || !rows_out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    DeviceGuard guard(c->device);
    HIP_TRY(hipMemcpy(rows_out, c->d_rows, (size_t)c->n_nodes * (size_t)c->words * 8, hipMemcpyDeviceToHost));
    return SBWTGPU_OK;
}

int sbwtgpu_colors_dev(const sbwtgpu_colors *c, const uint64_t **d_rows) {
    if (!c || !d_rows) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    *d_rows = reinterpret_cast<const uint64_t *>(c->d_rows);
    return SBWTGPU_OK;
}

int64_t sbwtgpu_pseudoalign_workspace_bytes(int64_t total_bases, int64_t n_reads, int strands) {
    if (total_bases < 0) total_bases = 0;
    if (n_reads < 0) n_reads = 0;
    return sbwt_pa_layout(sbwtgpu_search_workspace_bytes(total_bases), total_bases, n_reads, strands == 2 ? 2 : 1).total;
}

// What colouring and the query share: the result offsets, the int32 search of the batch and, for two strands, of the mirrored
// batch into the second result buffer; `tail` enqueues what turns the results into bits or records (res2: NULL with one strand,
// and for a batch without any window, whose result buffers nobody wrote).
}  // extern "C"
template <typename Tail>
static int colors_dev_common(const sbwtgpu_colors *c, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                             int64_t n_reads, int strands, void *d_ws, int64_t ws_bytes, void *stream, Tail tail) {
    if (total_bases < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative size");
    if (total_bases >= ((int64_t)1 << 36))
        return fail(SBWTGPU_ERR_INVALID_ARG, "more than 2^36 bases in one call: split the batch");
    const int64_t need = sbwtgpu_pseudoalign_workspace_bytes(total_bases, n_reads, strands);
    if (!d_ws || ws_bytes < need)
        return fail(SBWTGPU_ERR_INVALID_ARG, "workspace missing or too small (%lld < %lld)", (long long)ws_bytes, (long long)need);
    if (((uintptr_t)d_ws & 15) != 0) return fail(SBWTGPU_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
    if (n_reads == 0) return SBWTGPU_OK;
    if (!d_read_off || (total_bases > 0 && !d_bases)) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL device pointer");
    const sbwtgpu_index *idx = c->idx;
    DeviceGuard guard(idx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t search_ws = sbwtgpu_search_workspace_bytes(total_bases);
    const SbwtPaLayout L = sbwt_pa_layout(search_ws, total_bases, n_reads, strands);
    char *w = static_cast<char *>(d_ws);
    SbwtPaHeader *hdr = reinterpret_cast<SbwtPaHeader *>(w + L.hdr);
    int *res = reinterpret_cast<int *>(w + L.res);
    long long *ooff = reinterpret_cast<long long *>(w + L.ooff);
    const int k = (int)idx->h.k;
    HIP_TRY(hipMemsetAsync(hdr, 0, sizeof(SbwtPaHeader), st));
    sbwt_launch_rh_offsets(reinterpret_cast<const long long *>(d_read_off), n_reads, k, reinterpret_cast<long long *>(w + L.cnt),
                           reinterpret_cast<long long *>(w + L.bsum), ooff, st);
    // (a batch of fewer than k bases has no window: nothing to search, and `tail` reads no result)
    const bool any = total_bases >= k;
    const SbwtWorkHeader *sws = reinterpret_cast<const SbwtWorkHeader *>(w);
    int *res2 = nullptr;
    int rc;
    if (any) {
        t_out32 = 1;
        rc = search_dev_common(idx, d_bases, total_bases, d_read_off, n_reads, reinterpret_cast<int64_t *>(res),
                               reinterpret_cast<const int64_t *>(ooff), d_ws, search_ws, stream, 0);
        t_out32 = 0;
        if (rc != SBWTGPU_OK) return rc;
        sbwt_launch_pa_note_status(sws, hdr, st);
    }
    if (strands == 2 && any) {
        res2 = reinterpret_cast<int *>(w + L.res2);
        char *rcb = w + L.rc;
        long long *roff2 = reinterpret_cast<long long *>(w + L.roff2), *ooff2 = reinterpret_cast<long long *>(w + L.ooff2);
        sbwt_launch_rh_mirror(d_bases, total_bases, reinterpret_cast<const long long *>(d_read_off), ooff, n_reads, rcb, roff2, ooff2, st);
        t_out32 = 1;
        rc = search_dev_common(idx, rcb, total_bases, reinterpret_cast<const int64_t *>(roff2), n_reads, reinterpret_cast<int64_t *>(res2),
                               reinterpret_cast<const int64_t *>(ooff2), d_ws, search_ws, stream, 0);
        t_out32 = 0;
        if (rc != SBWTGPU_OK) return rc;
        sbwt_launch_pa_note_status(sws, hdr, st);
    }
    tail(res, res2, ooff, hdr, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return SBWTGPU_OK;
}
extern "C" {

int sbwtgpu_pseudoalign_dev(const sbwtgpu_colors *c, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                            int64_t n_reads, int strands, int threshold_ppm, int denominator, sbwtgpu_pseudoalignment *d_out,
                            int32_t *d_counts_or_null, void *d_ws, int64_t ws_bytes, void *stream) {
    int rc = colors_check(c);
    if (rc == SBWTGPU_OK) rc = colors_check_batch(n_reads, strands);
    if (rc == SBWTGPU_OK) rc = colors_check_query(threshold_ppm, denominator);
    if (rc != SBWTGPU_OK) return rc;
    if (c->n_colors > 64)
        return fail(SBWTGPU_ERR_INVALID_ARG, "the colours object has %d colours, a 16-byte record holds 64: use sbwtgpu_pseudoalign_wide_dev",
                    c->n_colors);
    if (n_reads > 0 && !d_out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL device pointer");
    return colors_dev_common(c, d_bases, total_bases, d_read_off, n_reads, strands, d_ws, ws_bytes, stream,
                             [&](const int *res, const int *res2, const long long *ooff, SbwtPaHeader *, hipStream_t st) {
                                 sbwt_launch_pa_reduce(res, res2, ooff, n_reads, c->d_rows, c->n_nodes, c->n_colors, threshold_ppm,
                                                       denominator, reinterpret_cast<SbwtPseudoalignment *>(d_out), d_counts_or_null, st);
                             });
}

int sbwtgpu_pseudoalign_wide_dev(const sbwtgpu_colors *c, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                                 int64_t n_reads, int strands, int threshold_ppm, int denominator, sbwtgpu_read_found *d_out,
                                 uint64_t *d_colors, int32_t *d_counts_or_null, void *d_ws, int64_t ws_bytes, void *stream) {
    int rc = colors_check(c);
    if (rc == SBWTGPU_OK) rc = colors_check_batch(n_reads, strands);
    if (rc == SBWTGPU_OK) rc = colors_check_query(threshold_ppm, denominator);
    if (rc != SBWTGPU_OK) return rc;
    if (n_reads > 0 && (!d_out || !d_colors)) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL device pointer");
    return colors_dev_common(c, d_bases, total_bases, d_read_off, n_reads, strands, d_ws, ws_bytes, stream,
                             [&](const int *res, const int *res2, const long long *ooff, SbwtPaHeader *, hipStream_t st) {
                                 sbwt_launch_pa_reduce_wide(res, res2, ooff, n_reads, c->d_rows, c->n_nodes, c->words, c->n_colors,
                                                            threshold_ppm, denominator, reinterpret_cast<SbwtReadFound *>(d_out),
                                                            reinterpret_cast<unsigned long long *>(d_colors), d_counts_or_null, st);
                             });
}

// Host buffers, for colouring (out == NULL: bit `color` is set, *n_hit the windows with a hit) and for the query alike: the batch
// is cut into chunks of whole reads of at most "pseudoalign_chunk_bases" bases (a chunk always takes one read), two chunks in
// flight on the parked slots of the search pipeline.  Bases and offsets go down; records, and counts if asked for, come back.
// wide_colors != NULL: the wide query -- `out` holds 8-byte records (sbwtgpu_read_found) and wide_colors the reads' colour
// words, 8 + 8 words bytes per read instead of 16; a chunk then also ends where its results would outgrow what 2^24 reads of
// 64 colours with counts bring back.  sets != NULL: the wide query over a colour-set object, whose `base` is c.  marks != NULL:
// colouring for a colour-set builder, whose `base` is c -- a hit sets its column's bit in the builder's mark bitmap.
static int colors_host_batch(const sbwtgpu_colors *c, const char *bases, const int64_t *read_off, int64_t n_reads, int strands,
                             int color, int threshold_ppm, int denominator, void *out, uint64_t *wide_colors, int32_t *counts,
                             int64_t *n_windows, int64_t *n_hit, const sbwtgpu_colorsets *sets = nullptr,
                             unsigned long long *marks = nullptr) {
    const sbwtgpu_index *idx = c->idx;
    if (n_windows) *n_windows = 0;
    if (n_hit) *n_hit = 0;
    if (n_reads == 0) return SBWTGPU_OK;
    if (!read_off) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    if (read_off[n_reads] > read_off[0] && !bases) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    const int64_t nc = c->n_colors, k = c->k, nw = c->words;
    const int64_t rec_bytes = wide_colors ? 8 : 16, per_read = rec_bytes + (wide_colors ? 8 * nw : 0) + (counts ? 4 * nc : 0);
    const int64_t budget = g_pa_chunk_bases > 0 ? g_pa_chunk_bases : (int64_t)64 << 20;
    const int64_t CH_READS = std::min((int64_t)1 << 24, std::max<int64_t>(1, (((int64_t)1 << 24) * 272) / per_read));
    std::vector<int64_t> cuts{0};
    int64_t max_bases = 0, max_reads = 0, windows = 0;
    int rc;
    try {
        for (int64_t lo = 0, r = 0; r < n_reads; r++) {
            if ((rc = check_read_length(read_off, r)) != SBWTGPU_OK) return rc;
            if (r > lo && (read_off[r + 1] - read_off[lo] > budget || r - lo >= CH_READS)) {
                cuts.push_back(r);
                lo = r;
            }
            max_bases = std::max(max_bases, read_off[r + 1] - read_off[lo]);
            max_reads = std::max(max_reads, r + 1 - lo);
            windows += std::max<int64_t>(0, read_off[r + 1] - read_off[r] - k + 1);
        }
        cuts.push_back(n_reads);
    } catch (const std::bad_alloc &) {
        return fail(SBWTGPU_ERR_OOM, "out of host memory");
    }
    const int64_t n_chunks = (int64_t)cuts.size() - 1;
    const bool pin_in = is_pinned(bases);
    const int64_t ws_bytes = sbwtgpu_pseudoalign_workspace_bytes(max_bases, max_reads, strands);
    const int64_t b_rec = out ? align256(max_reads * rec_bytes) : 0, b_col = wide_colors ? align256(max_reads * nw * 8) : 0,
                  b_cnt = counts ? align256(max_reads * nc * 4) : 0;
    const int64_t need_in = align256(max_bases + 16) + align256((max_reads + 1) * 8);
    const int64_t need_out = b_rec + b_col + b_cnt;
    const int64_t need_dev = align256(max_bases + 16) + align256((max_reads + 1) * 8) + b_rec + b_col + b_cnt + align256(ws_bytes);
    DeviceGuard guard(idx->device);
    const int n_slots = n_chunks > 1 ? 2 : 1;
    PipeSlot S[2];
    if ((rc = take_slots(idx->device, S, n_slots, need_in, need_out, need_dev, "pseudoalignment buffers")) != SBWTGPU_OK) return rc;
    int bug = 0;                    // the first nonzero device status of a chunk
    int64_t hits = 0;
    const int64_t o_roff = align256(max_bases + 16), o_rec = o_roff + align256((max_reads + 1) * 8), o_col = o_rec + b_rec,
                  o_cnt = o_col + b_col, o_ws = o_cnt + b_cnt;
    auto submit = [&](int64_t ch) -> int {
        PipeSlot &P = S[ch % n_slots];
        const int64_t lo = cuts[(size_t)ch], hi = cuts[(size_t)ch + 1], nr = hi - lo, nb = read_off[hi] - read_off[lo];
        int64_t *hro = (int64_t *)(P.h_in + align256(max_bases + 16));
        for (int64_t r = 0; r <= nr; r++) hro[r] = read_off[lo + r] - read_off[lo];
        const char *hb = bases + read_off[lo];
        if (!pin_in && nb > 0) { parallel_memcpy(P.h_in, hb, (size_t)nb); hb = P.h_in; }
        hipError_t e;
        if ((nb > 0 && (e = hipMemcpyAsync(P.d_mem, hb, (size_t)nb, hipMemcpyHostToDevice, P.st)) != hipSuccess) ||
            (e = hipMemcpyAsync(P.d_mem + o_roff, hro, (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, P.st)) != hipSuccess)
            return fail(SBWTGPU_ERR_HIP, "H2D copy: %s", hipGetErrorString(e));
        int r2;
        const int64_t *d_roff = (const int64_t *)(P.d_mem + o_roff);
        if (sets) {
            r2 = sbwtgpu_pseudoalign_sets_dev(sets, P.d_mem, nb, d_roff, nr, strands, threshold_ppm, denominator,
                                              (sbwtgpu_read_found *)(P.d_mem + o_rec), (uint64_t *)(P.d_mem + o_col),
                                              counts ? (int32_t *)(P.d_mem + o_cnt) : nullptr, P.d_mem + o_ws, ws_bytes, P.st);
        } else if (wide_colors) {
            r2 = sbwtgpu_pseudoalign_wide_dev(c, P.d_mem, nb, d_roff, nr, strands, threshold_ppm, denominator,
                                              (sbwtgpu_read_found *)(P.d_mem + o_rec), (uint64_t *)(P.d_mem + o_col),
                                              counts ? (int32_t *)(P.d_mem + o_cnt) : nullptr, P.d_mem + o_ws, ws_bytes, P.st);
        } else if (out) {
            r2 = sbwtgpu_pseudoalign_dev(c, P.d_mem, nb, d_roff, nr, strands, threshold_ppm, denominator,
                                         (sbwtgpu_pseudoalignment *)(P.d_mem + o_rec), counts ? (int32_t *)(P.d_mem + o_cnt) : nullptr,
                                         P.d_mem + o_ws, ws_bytes, P.st);
        } else if (marks) {
            r2 = colors_dev_common(c, P.d_mem, nb, d_roff, nr, strands, P.d_mem + o_ws, ws_bytes, P.st,
                                   [&](const int *res, const int *res2, const long long *ooff, SbwtPaHeader *hdr, hipStream_t st) {
                                       sbwt_launch_csb_mark(res, res2, ooff, nr, nb, marks, c->n_nodes, 1, hdr, st);
                                       if (res2) sbwt_launch_csb_mark(res2, nullptr, ooff, nr, nb, marks, c->n_nodes, 0, hdr, st);
                                   });
        } else {
            r2 = colors_dev_common(c, P.d_mem, nb, d_roff, nr, strands, P.d_mem + o_ws, ws_bytes, P.st,
                                   [&](const int *res, const int *res2, const long long *ooff, SbwtPaHeader *hdr, hipStream_t st) {
                                       sbwt_launch_col_mark(res, res2, ooff, nr, nb, c->d_rows, c->n_nodes, c->words, color, 1, hdr, st);
                                       if (res2)
                                           sbwt_launch_col_mark(res2, nullptr, ooff, nr, nb, c->d_rows, c->n_nodes, c->words, color, 0, hdr, st);
                                   });
        }
        if (r2 != SBWTGPU_OK) return r2;
        const SbwtPaLayout L = sbwt_pa_layout(sbwtgpu_search_workspace_bytes(nb), nb, nr, strands);
        if ((out && (e = hipMemcpyAsync(P.h_out, P.d_mem + o_rec, (size_t)(nr * rec_bytes), hipMemcpyDeviceToHost, P.st)) != hipSuccess) ||
            (wide_colors &&
             (e = hipMemcpyAsync(P.h_out + b_rec, P.d_mem + o_col, (size_t)(nr * nw) * 8, hipMemcpyDeviceToHost, P.st)) != hipSuccess) ||
            (counts && nr * nc > 0 &&
             (e = hipMemcpyAsync(P.h_out + b_rec + b_col, P.d_mem + o_cnt, (size_t)(nr * nc) * 4, hipMemcpyDeviceToHost, P.st)) != hipSuccess) ||
            (e = hipMemcpyAsync(P.h_status, P.d_mem + o_ws + L.hdr, 16, hipMemcpyDeviceToHost, P.st)) != hipSuccess)
            return fail(SBWTGPU_ERR_HIP, "D2H copy: %s", hipGetErrorString(e));
        return SBWTGPU_OK;
    };
    auto collect = [&](int64_t ch) -> int {
        PipeSlot &P = S[ch % n_slots];
        hipError_t e = hipStreamSynchronize(P.st);
        if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "stream synchronize: %s", hipGetErrorString(e));
        if (P.h_status[0] != 0 && bug == 0) bug = P.h_status[0];
        unsigned long long nh;
        memcpy(&nh, P.h_status + 2, 8);                  // (SbwtPaHeader::n_hit)
        hits += (int64_t)nh;
        const int64_t lo = cuts[(size_t)ch], hi = cuts[(size_t)ch + 1];
        if (out) memcpy((char *)out + lo * rec_bytes, P.h_out, (size_t)((hi - lo) * rec_bytes));
        if (wide_colors) memcpy(wide_colors + lo * nw, P.h_out + b_rec, (size_t)((hi - lo) * nw) * 8);
        if (counts && (hi - lo) * nc > 0) memcpy(counts + lo * nc, P.h_out + b_rec + b_col, (size_t)((hi - lo) * nc) * 4);
        return SBWTGPU_OK;
    };
    rc = two_in_flight(n_chunks, submit, collect);
    park_slots(idx->device, S, n_slots, rc);
    if (rc != SBWTGPU_OK) return rc;
    if (bug) return fail_status(bug);
    if (n_windows) *n_windows = windows;
    if (n_hit) *n_hit = hits;
    return SBWTGPU_OK;
}

int sbwtgpu_colors_add_batch(sbwtgpu_colors *c, int color, const char *bases, const int64_t *read_off, int64_t n_reads, int strands,
                             int64_t *n_windows, int64_t *n_hit_windows) {
    int rc = colors_check(c);
    if (rc == SBWTGPU_OK) rc = colors_check_batch(n_reads, strands);
    if (rc != SBWTGPU_OK) return rc;
    if (color < 0 || color >= c->n_colors)
        return fail(SBWTGPU_ERR_INVALID_ARG, "color %d is out of range: the colours object has %d colours", color, c->n_colors);
    return colors_host_batch(c, bases, read_off, n_reads, strands, color, 0, 0, nullptr, nullptr, nullptr, n_windows, n_hit_windows);
}

int sbwtgpu_pseudoalign_batch(const sbwtgpu_colors *c, const char *bases, const int64_t *read_off, int64_t n_reads, int strands,
                              int threshold_ppm, int denominator, sbwtgpu_pseudoalignment *out, int32_t *counts_or_null) {
    int rc = colors_check(c);
    if (rc == SBWTGPU_OK) rc = colors_check_batch(n_reads, strands);
    if (rc == SBWTGPU_OK) rc = colors_check_query(threshold_ppm, denominator);
    if (rc != SBWTGPU_OK) return rc;
    if (c->n_colors > 64)
        return fail(SBWTGPU_ERR_INVALID_ARG, "the colours object has %d colours, a 16-byte record holds 64: use sbwtgpu_pseudoalign_wide_batch",
                    c->n_colors);
    if (n_reads > 0 && !out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    return colors_host_batch(c, bases, read_off, n_reads, strands, 0, threshold_ppm, denominator, out, nullptr, counts_or_null, nullptr,
                             nullptr);
}

int sbwtgpu_pseudoalign_wide_batch(const sbwtgpu_colors *c, const char *bases, const int64_t *read_off, int64_t n_reads, int strands,
                                   int threshold_ppm, int denominator, sbwtgpu_read_found *out, uint64_t *colors_out,
                                   int32_t *counts_or_null) {
    int rc = colors_check(c);
    if (rc == SBWTGPU_OK) rc = colors_check_batch(n_reads, strands);
    if (rc == SBWTGPU_OK) rc = colors_check_query(threshold_ppm, denominator);
    if (rc != SBWTGPU_OK) return rc;
    if (n_reads > 0 && (!out || !colors_out)) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    return colors_host_batch(c, bases, read_off, n_reads, strands, 0, threshold_ppm, denominator, out, colors_out, counts_or_null,
                             nullptr, nullptr);
}

// ---- deduplicated colour sets (sbwt_colorsets.hip) -----------------------------------------------------
static int colorsets_check(const sbwtgpu_colorsets *s) {
    if (!s) return fail(SBWTGPU_ERR_INVALID_ARG, "colour-set object is NULL");
    return colors_check(&s->base);
}

static sbwtgpu_colorsets *colorsets_new(const sbwtgpu_index *idx, int n_colors) {
    sbwtgpu_colorsets *s = new (std::nothrow) sbwtgpu_colorsets();
    if (!s) return nullptr;
    s->base.idx = idx;
    s->base.device = idx->device;
    s->base.n_nodes = idx->h.n_nodes;
    s->base.k = idx->h.k;
    s->base.n_colors = n_colors;
    s->base.words = (n_colors + 63) / 64;
    return s;
}

// n_colored = the ids that are not 0
static hipError_t colorsets_count(sbwtgpu_colorsets *s, hipStream_t st) {
    DevBuf count;
    unsigned long long h = 0;
    hipError_t e = count.alloc(8);
    if (e == hipSuccess) e = hipMemsetAsync(count.p, 0, 8, st);
    if (e == hipSuccess) {
        sbwt_launch_cs_count(s->d_ids, s->base.n_nodes, static_cast<unsigned long long *>(count.p), st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h, count.p, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    s->n_colored = (int64_t)h;
    return e;
}

static int colorsets_hip_failed(sbwtgpu_colorsets *s, hipError_t e) {
    (void)hipGetLastError();
    sbwtgpu_colorsets_destroy(s);
    return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "colour sets: %s", hipGetErrorString(e));
}

int sbwtgpu_colorsets_compress(const sbwtgpu_colors *c, sbwtgpu_colorsets **out) {
    if (!c || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    const int rc = colors_check(c);
    if (rc != SBWTGPU_OK) return rc;
    DeviceGuard guard(c->device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", c->device);
    sbwtgpu_colorsets *s = colorsets_new(c->idx, c->n_colors);
    if (!s) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    Stream st;
    long long n_sets = 0;
    hipError_t e = hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking);
    if (e == hipSuccess) e = sbwt_colorsets_compress(c->d_rows, c->n_nodes, c->words, &s->d_ids, &s->d_table, &n_sets, st.s);
    s->n_sets = n_sets;
    if (e == hipSuccess) e = colorsets_count(s, st.s);
    if (e != hipSuccess) return colorsets_hip_failed(s, e);
    *out = s;
    return SBWTGPU_OK;
}

int sbwtgpu_colorsets_create(const sbwtgpu_index *idx, int n_colors, const uint32_t *ids, int64_t n_sets, const uint64_t *table,
                             sbwtgpu_colorsets **out) {
    if (!idx || !out || !ids || !table) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    const int rc = colors_check_index(idx);
    if (rc != SBWTGPU_OK) return rc;
    if (n_colors < 1 || n_colors > SBWTGPU_MAX_COLORS)
        return fail(SBWTGPU_ERR_INVALID_ARG, "n_colors must be in 1 .. %d, not %d", SBWTGPU_MAX_COLORS, n_colors);
    if (n_sets < 1 || n_sets > (int64_t)0xFFFFFFFFll)
        return fail(SBWTGPU_ERR_INVALID_ARG, "n_sets must be in 1 .. 2^32 - 1, not %lld (row 0, the empty set, is always there)", (long long)n_sets);
    DeviceGuard guard(idx->device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", idx->device);
    sbwtgpu_colorsets *s = colorsets_new(idx, n_colors);
    if (!s) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    s->n_sets = n_sets;
    const size_t id_bytes = (size_t)s->base.n_nodes * 4, table_bytes = (size_t)n_sets * (size_t)s->base.words * 8;
    Stream st;
    unsigned long long report[2] = {~0ull, ~0ull};
    hipError_t e = hipMalloc((void **)&s->d_ids, id_bytes + 16);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_table, table_bytes);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMemcpyAsync(s->d_ids, ids, id_bytes, hipMemcpyHostToDevice, st.s);
    if (e == hipSuccess) e = hipMemcpyAsync(s->d_table, table, table_bytes, hipMemcpyHostToDevice, st.s);
    if (e == hipSuccess) e = sbwt_colorsets_validate(idx->view(), s->d_ids, s->d_table, n_sets, n_colors, report, st.s);
    if (e == hipSuccess && report[0] == ~0ull && report[1] == ~0ull) e = colorsets_count(s, st.s);
    if (e != hipSuccess) return colorsets_hip_failed(s, e);
    if (report[1] != ~0ull || report[0] != ~0ull) {
        sbwtgpu_colorsets_destroy(s);
        const long long row = (long long)(report[1] >> 8);
        if (report[1] == ~0ull)
            return fail(SBWTGPU_ERR_INVALID_ARG, "colour sets: the id of column %lld is not below n_sets = %lld", (long long)report[0],
                        (long long)n_sets);
        switch ((int)(report[1] & 255)) {
        case SBWT_CS_ROW0_NOT_ZERO:
            return fail(SBWTGPU_ERR_INVALID_ARG, "colour sets: row 0 of the table is not all zero (id 0 is the empty set)");
        case SBWT_CS_ZERO_ROW:
            return fail(SBWTGPU_ERR_INVALID_ARG, "colour sets: row %lld of the table is all zero (only row 0 may be)", row);
        default:
            return fail(SBWTGPU_ERR_INVALID_ARG, "colour sets: row %lld of the table has a bit >= n_colors = %d", row, n_colors);
        }
    }
    *out = s;
    return SBWTGPU_OK;
}

int sbwtgpu_colorsets_expand(const sbwtgpu_colorsets *s, sbwtgpu_colors **out) {
    if (!s || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    int rc = colorsets_check(s);
    if (rc != SBWTGPU_OK) return rc;
    sbwtgpu_colors *c = nullptr;
    if ((rc = colors_create_checked(s->base.idx, s->base.n_colors, nullptr, &c)) != SBWTGPU_OK) return rc;
    DeviceGuard guard(s->base.device);
    Stream st;
    hipError_t e = hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking);
    if (e == hipSuccess) {
        sbwt_launch_cs_expand(s->d_ids, s->d_table, s->base.n_nodes, s->base.words, c->d_rows, st.s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st.s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        sbwtgpu_colors_destroy(c);
        return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "colour sets: %s", hipGetErrorString(e));
    }
    *out = c;
    return SBWTGPU_OK;
}

void sbwtgpu_colorsets_destroy(sbwtgpu_colorsets *s) {
    if (!s) return;
    DeviceGuard guard(s->base.device);
    if (s->d_ids) (void)hipFree(s->d_ids);
    if (s->d_table) (void)hipFree(s->d_table);
    delete s;
}

int sbwtgpu_colorsets_info(const sbwtgpu_colorsets *s, int64_t *n_columns, int64_t *k, int32_t *n_colors, int32_t *words, int64_t *n_sets,
                           int64_t *n_colored_columns, int64_t *device_bytes) {
    if (!s) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    if (n_columns) *n_columns = s->base.n_nodes;
    if (k) *k = s->base.k;
    if (n_colors) *n_colors = s->base.n_colors;
    if (words) *words = s->base.words;
    if (n_sets) *n_sets = s->n_sets;
    if (n_colored_columns) *n_colored_columns = s->n_colored;
    if (device_bytes) *device_bytes = s->base.n_nodes * 4 + s->n_sets * (int64_t)s->base.words * 8;
    return SBWTGPU_OK;
}

int sbwtgpu_colorsets_copy(const sbwtgpu_colorsets *s, uint32_t *ids_out, uint64_t *table_out) {
    if (!s) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    DeviceGuard guard(s->base.device);
    if (ids_out && s->base.n_nodes > 0) HIP_TRY(hipMemcpy(ids_out, s->d_ids, (size_t)s->base.n_nodes * 4, hipMemcpyDeviceToHost));
    if (table_out) HIP_TRY(hipMemcpy(table_out, s->d_table, (size_t)s->n_sets * (size_t)s->base.words * 8, hipMemcpyDeviceToHost));
    return SBWTGPU_OK;
}

int sbwtgpu_colorsets_dev(const sbwtgpu_colorsets *s, const uint32_t **d_ids, const uint64_t **d_table) {
    if (!s) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    if (d_ids) *d_ids = reinterpret_cast<const uint32_t *>(s->d_ids);
    if (d_table) *d_table = reinterpret_cast<const uint64_t *>(s->d_table);
    return SBWTGPU_OK;
}

// coloured unitigs (sbwt_unitigs.hip with a colour view): the object's ids and table are read in place during the call only
int sbwtgpu_unitigs_create_colored(const sbwtgpu_colorsets *s, sbwtgpu_unitigs **out) {
    if (!s || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    const int rc = colorsets_check(s);
    if (rc != SBWTGPU_OK) return rc;
    return unitigs_create_common(s->base.idx, s->d_ids, s->d_table, s->base.words, s->n_sets, s->base.n_colors, 0u, out);
}

// the unitigs as a graph (section 21): the plain run of idx or the coloured run of s, with the links and the column map asked for
int sbwtgpu_unitigs_create_graph(const sbwtgpu_index *idx, const sbwtgpu_colorsets *s, unsigned flags, sbwtgpu_unitigs **out) {
    if (!out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if ((idx != nullptr) == (s != nullptr))
        return fail(SBWTGPU_ERR_INVALID_ARG, "unitig graph: give exactly one of idx (a plain run) and s (a coloured run), %s were given",
                    idx ? "both" : "neither");
    if (flags & ~(unsigned)(SBWTGPU_UNITIGS_LINKS | SBWTGPU_UNITIGS_COLUMN_MAP))
        return fail(SBWTGPU_ERR_INVALID_ARG, "unitig graph: unknown flag bits 0x%x", flags & ~(unsigned)(SBWTGPU_UNITIGS_LINKS | SBWTGPU_UNITIGS_COLUMN_MAP));
    if (idx) return unitigs_create_common(idx, nullptr, nullptr, 0, 0, 0, flags, out);
    const int rc = colorsets_check(s);
    if (rc != SBWTGPU_OK) return rc;
    return unitigs_create_common(s->base.idx, s->d_ids, s->d_table, s->base.words, s->n_sets, s->base.n_colors, flags, out);
}

int sbwtgpu_pseudoalign_sets_dev(const sbwtgpu_colorsets *s, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                                 int64_t n_reads, int strands, int threshold_ppm, int denominator, sbwtgpu_read_found *d_out,
                                 uint64_t *d_colors, int32_t *d_counts_or_null, void *d_ws, int64_t ws_bytes, void *stream) {
    int rc = colorsets_check(s);
    if (rc == SBWTGPU_OK) rc = colors_check_batch(n_reads, strands);
    if (rc == SBWTGPU_OK) rc = colors_check_query(threshold_ppm, denominator);
    if (rc != SBWTGPU_OK) return rc;
    if (n_reads > 0 && (!d_out || !d_colors)) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL device pointer");
    const sbwtgpu_colors *c = &s->base;
    return colors_dev_common(c, d_bases, total_bases, d_read_off, n_reads, strands, d_ws, ws_bytes, stream,
                             [&](const int *res, const int *res2, const long long *ooff, SbwtPaHeader *, hipStream_t st) {
                                 sbwt_launch_pa_reduce_sets(res, res2, ooff, n_reads, s->d_ids, s->d_table, c->n_nodes, s->n_sets, c->words,
                                                            c->n_colors, threshold_ppm, denominator, reinterpret_cast<SbwtReadFound *>(d_out),
                                                            reinterpret_cast<unsigned long long *>(d_colors), d_counts_or_null, st);
                             });
}

int sbwtgpu_pseudoalign_sets_batch(const sbwtgpu_colorsets *s, const char *bases, const int64_t *read_off, int64_t n_reads, int strands,
                                   int threshold_ppm, int denominator, sbwtgpu_read_found *out, uint64_t *colors_out,
                                   int32_t *counts_or_null) {
    int rc = colorsets_check(s);
    if (rc == SBWTGPU_OK) rc = colors_check_batch(n_reads, strands);
    if (rc == SBWTGPU_OK) rc = colors_check_query(threshold_ppm, denominator);
    if (rc != SBWTGPU_OK) return rc;
    if (n_reads > 0 && (!out || !colors_out)) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    return colors_host_batch(&s->base, bases, read_off, n_reads, strands, 0, threshold_ppm, denominator, out, colors_out, counts_or_null,
                             nullptr, nullptr, s);
}

// ---- the colour-set builder (sbwt_colorsets.hip, "the builder") -----------------------------------------
static int builder_check(const sbwtgpu_colorsets_builder *b) {
    if (!b) return fail(SBWTGPU_ERR_INVALID_ARG, "colour-set builder is NULL");
    if (b->finished) return fail(SBWTGPU_ERR_INVALID_ARG, "colour-set builder: finish has consumed it, only destroy is left");
    if (b->broken) return fail(SBWTGPU_ERR_INVALID_ARG, "colour-set builder is broken by an earlier error, only destroy is left");
    return colors_check(&b->base);
}

static int builder_failed(sbwtgpu_colorsets_builder *b, hipError_t e) {
    (void)hipGetLastError();
    b->broken = true;
    return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "colour-set builder: %s", hipGetErrorString(e));
}

// merges the open colour's marks into (ids, table); nothing open: nothing to do
static int builder_close_open(sbwtgpu_colorsets_builder *b) {
    if (b->open < 0) return SBWTGPU_OK;
    long long marked = 0;
    const hipError_t e = sbwt_csb_close(&b->st, b->open, &marked, b->stream.s);
    if (e != hipSuccess) return builder_failed(b, e);
    b->per_color[(size_t)b->open] = marked;
    b->state[(size_t)b->open] = CSB_CLOSED;
    b->open = -1;
    return SBWTGPU_OK;
}

int sbwtgpu_colorsets_builder_create(const sbwtgpu_index *idx, int n_colors, sbwtgpu_colorsets_builder **out) {
    if (!idx || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    const int rc = colors_check_index(idx);
    if (rc != SBWTGPU_OK) return rc;
    if (n_colors < 1 || n_colors > SBWTGPU_MAX_COLORS)
        return fail(SBWTGPU_ERR_INVALID_ARG, "n_colors must be in 1 .. %d, not %d", SBWTGPU_MAX_COLORS, n_colors);
    DeviceGuard guard(idx->device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", idx->device);
    sbwtgpu_colorsets_builder *b = new (std::nothrow) sbwtgpu_colorsets_builder();
    if (!b) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    try {
        b->state.assign((size_t)n_colors, CSB_NEW);
        b->per_color.assign((size_t)n_colors, 0);
    } catch (const std::bad_alloc &) {
        delete b;
        return fail(SBWTGPU_ERR_OOM, "out of host memory");
    }
    b->base.idx = idx;
    b->base.device = idx->device;
    b->base.n_nodes = idx->h.n_nodes;
    b->base.k = idx->h.k;
    b->base.n_colors = n_colors;
    b->base.words = (n_colors + 63) / 64;
    hipError_t e = hipStreamCreateWithFlags(&b->stream.s, hipStreamNonBlocking);
    if (e == hipSuccess) e = sbwt_csb_init(&b->st, b->base.n_nodes, b->base.words, b->stream.s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        delete b;
        return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "colour-set builder: %s", hipGetErrorString(e));
    }
    *out = b;
    return SBWTGPU_OK;
}

void sbwtgpu_colorsets_builder_destroy(sbwtgpu_colorsets_builder *b) {
    if (!b) return;
    DeviceGuard guard(b->base.device);
    sbwt_csb_free(&b->st);
    delete b;
}

int sbwtgpu_colorsets_builder_add_batch(sbwtgpu_colorsets_builder *b, int color, const char *bases, const int64_t *read_off,
                                        int64_t n_reads, int strands, int64_t *n_windows, int64_t *n_hit_windows) {
    int rc = builder_check(b);
    if (rc == SBWTGPU_OK) rc = colors_check_batch(n_reads, strands);
    if (rc != SBWTGPU_OK) return rc;
    if (color < 0 || color >= b->base.n_colors)
        return fail(SBWTGPU_ERR_INVALID_ARG, "color %d is out of range: the colour-set builder has %d colours", color, b->base.n_colors);
    if (b->state[(size_t)color] == CSB_CLOSED)
        return fail(SBWTGPU_ERR_INVALID_ARG,
                    "colour %d is closed: the sequences of one colour must come in consecutive calls (another colour was added after it)", color);
    // (what colors_host_batch would refuse is refused here, before the call closes a colour)
    if (n_reads > 0 && (!read_off || (read_off[n_reads] > read_off[0] && !bases))) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    for (int64_t r = 0; r < n_reads; r++)
        if ((rc = check_read_length(read_off, r)) != SBWTGPU_OK) return rc;
    DeviceGuard guard(b->base.device);
    if (b->open != color) {
        if ((rc = builder_close_open(b)) != SBWTGPU_OK) return rc;
        b->open = color;
        b->state[(size_t)color] = CSB_OPEN;
    }
    rc = colors_host_batch(&b->base, bases, read_off, n_reads, strands, color, 0, 0, nullptr, nullptr, nullptr, n_windows, n_hit_windows,
                           nullptr, b->st.d_marks);
    if (rc == SBWTGPU_ERR_OOM || rc == SBWTGPU_ERR_HIP) b->broken = true;          // (some of the batch may be marked, some not)
    return rc;
}

int sbwtgpu_colorsets_builder_info(const sbwtgpu_colorsets_builder *b, int64_t *n_columns, int64_t *k, int32_t *n_colors, int32_t *words,
                                   int64_t *n_sets, int64_t *n_colored_columns, int64_t *per_color, int64_t *device_bytes) {
    const int rc = builder_check(b);
    if (rc != SBWTGPU_OK) return rc;
    if (n_columns) *n_columns = b->base.n_nodes;
    if (k) *k = b->base.k;
    if (n_colors) *n_colors = b->base.n_colors;
    if (words) *words = b->base.words;
    if (n_sets) *n_sets = b->st.n_sets;
    if (n_colored_columns) *n_colored_columns = b->st.n_colored;
    if (per_color) std::copy(b->per_color.begin(), b->per_color.end(), per_color);
    if (device_bytes) *device_bytes = sbwt_csb_device_bytes(&b->st);
    return SBWTGPU_OK;
}

int sbwtgpu_colorsets_builder_finish(sbwtgpu_colorsets_builder *b, sbwtgpu_colorsets **out) {
    if (!out) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    int rc = builder_check(b);
    if (rc != SBWTGPU_OK) return rc;
    DeviceGuard guard(b->base.device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", b->base.device);
    if ((rc = builder_close_open(b)) != SBWTGPU_OK) return rc;
    sbwtgpu_colorsets *s = colorsets_new(b->base.idx, b->base.n_colors);
    if (!s) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    long long n_sets = 0;
    s->n_colored = b->st.n_colored;
    const hipError_t e = sbwt_csb_finish(&b->st, &s->d_ids, &s->d_table, &n_sets, b->stream.s);
    s->n_sets = n_sets;
    if (e != hipSuccess) {
        sbwtgpu_colorsets_destroy(s);
        return builder_failed(b, e);
    }
    b->finished = true;
    *out = s;
    return SBWTGPU_OK;
}

// ---- set operations (sbwt_setops.hip) ---------------------------------------------------------------
}  // extern "C"
namespace {
double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
// what the label extraction needs of an index: the unitig pass's conditions, and a key of 64 or 128 bits
int setop_check_index(const sbwtgpu_index *idx, const char *who) {
    if (idx->h.rank_only) return fail(SBWTGPU_ERR_INVALID_ARG, "%s", RANK_ONLY_MSG);
    if (idx->h.k < 2 || idx->h.k > 64)
        return fail(SBWTGPU_ERR_INVALID_ARG, "%s: k = %lld, the keys of the device builder hold 2 <= k <= 64", who, (long long)idx->h.k);
    if (idx->h.n_nodes >= ((int64_t)1 << 32) - ((int64_t)1 << 24))
        return fail(SBWTGPU_ERR_INVALID_ARG, "%s: columns are 32-bit unsigned values (%lld columns)", who, (long long)idx->h.n_nodes);
    return SBWTGPU_OK;
}
int setop_check_pair(const sbwtgpu_index *a, const sbwtgpu_index *b, int op) {
    if (!a || !b) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    if (op < SBWTGPU_SETOP_UNION || op > SBWTGPU_SETOP_SYMMETRIC_DIFFERENCE)
        return fail(SBWTGPU_ERR_INVALID_ARG, "set operation %d: 0 union, 1 intersection, 2 difference, 3 symmetric difference", op);
    if (a->h.k != b->h.k)
        return fail(SBWTGPU_ERR_INVALID_ARG, "set operation: the indexes differ in k (%lld and %lld)", (long long)a->h.k, (long long)b->h.k);
    if (a->device != b->device)
        return fail(SBWTGPU_ERR_INVALID_ARG, "set operation: the indexes are on different devices (%d and %d)", a->device, b->device);
    int rc = setop_check_index(a, "set operation, a");
    if (rc == SBWTGPU_OK && b != a) rc = setop_check_index(b, "set operation, b");
    return rc;
}
int setop_hip_fail(hipError_t e, const char *what) {
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "set operation, %s: %s", what, hipGetErrorString(e));
}
// keys of a, keys of b, merge + select.  With d_res: the result's keys (a device allocation the caller owns).
int setop_merge(const sbwtgpu_index *a, const sbwtgpu_index *b, int op, hipStream_t st, void **d_res, sbwtgpu_setop_info *info) {
    DevBuf ka, kb;
    long long na = 0, nb = 0;
    const int key_bytes = a->h.k <= 32 ? 8 : 16;
    auto t0 = std::chrono::steady_clock::now();
    hipError_t e = sbwt_setops_keys(a->view(), &ka.p, &na, st);
    if (e != hipSuccess) return setop_hip_fail(e, "keys of a");
    info->pass_ms[0] = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    if (b != a) {
        e = sbwt_setops_keys(b->view(), &kb.p, &nb, st);
        if (e != hipSuccess) return setop_hip_fail(e, "keys of b");
    } else {
        nb = na;
    }
    info->pass_ms[1] = ms_since(t0);
    if (na + nb >= ((int64_t)1 << 32) - ((int64_t)1 << 24))
        return fail(SBWTGPU_ERR_INVALID_ARG, "set operation: %lld + %lld k-mers exceed the 2^32 work-items of one launch", na, nb);
    t0 = std::chrono::steady_clock::now();
    SbwtSetopCounts c;
    e = sbwt_setops_merge(ka.p, na, b != a ? kb.p : ka.p, nb, key_bytes, op, d_res, &c, st);
    if (e != hipSuccess) return setop_hip_fail(e, "merge");
    info->pass_ms[2] = ms_since(t0);
    info->n_a = c.n_a; info->n_b = c.n_b; info->n_both = c.n_both; info->n_either = c.n_either; info->n_result = c.n_result;
    return SBWTGPU_OK;
}
}  // namespace
extern "C" {

int sbwtgpu_index_setop(const sbwtgpu_index *a, const sbwtgpu_index *b, int op, int build_streaming_support,
                        sbwtgpu_plain_matrix_bits *out, sbwtgpu_setop_info *info) {
    sbwtgpu_setop_info local;
    if (!info) info = &local;
    memset(info, 0, sizeof(*info));
    if (!out) return fail(SBWTGPU_ERR_INVALID_ARG, "out is NULL");
    memset(out, 0, sizeof(*out));
    int rc = setop_check_pair(a, b, op);
    if (rc != SBWTGPU_OK) return rc;
    DeviceGuard guard(a->device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", a->device);
    Stream st;
    HIP_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    const int64_t k = a->h.k;
    void *d_res = nullptr;
    rc = setop_merge(a, b, op, st.s, &d_res, info);
    if (rc != SBWTGPU_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    SbwtBuildState S;
    try {
        const int ra = sbwt_build_from_keys(d_res, info->n_result, (int)k, &S, st.s);       // (S owns d_res now)
        if (ra != 0) { sbwt_build_release(&S); return fail(ra == -8 ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "set operation: builder tail"); }
        info->n_nopred = S.n_nopred;
        if ((long long)S.n_nopred * (long long)k > (1ll << 26)) {
            sbwt_build_release(&S);
            return fail(SBWTGPU_ERR_OOM, "set operation: the result has %lld predecessor-less k-mers x k = %lld dummy records (limit 2^26; "
                        "the dummies are expanded on the host).  Intersections and differences of fragmented sets reach this limit "
                        "sooner than genomes do: dump the unitigs of both indexes and use the host builder",
                        (long long)S.n_nopred, (long long)S.n_nopred * (long long)k);
        }
        rc = (k <= 32) ? build_columns_t<unsigned long long>(S, k, build_streaming_support, out)
                       : build_columns_t<unsigned __int128>(S, k, build_streaming_support, out);
    } catch (const std::bad_alloc &) {
        sbwt_build_release(&S);
        rc = fail(SBWTGPU_ERR_OOM, "out of host memory");
    }
    info->pass_ms[3] = ms_since(t0);
    return rc;
}

int sbwtgpu_index_setop_counts(const sbwtgpu_index *a, const sbwtgpu_index *b, sbwtgpu_setop_info *info) {
    if (!info) return fail(SBWTGPU_ERR_INVALID_ARG, "info is NULL");
    memset(info, 0, sizeof(*info));
    int rc = setop_check_pair(a, b, SBWTGPU_SETOP_UNION);
    if (rc != SBWTGPU_OK) return rc;
    DeviceGuard guard(a->device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", a->device);
    Stream st;
    HIP_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    return setop_merge(a, b, SBWTGPU_SETOP_UNION, st.s, nullptr, info);
}

int sbwtgpu_index_kmer_keys(const sbwtgpu_index *idx, void *out_keys, int64_t cap_bytes, int64_t *n_keys, int *key_bytes) {
    if (!idx) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    if (cap_bytes < 0 || (!out_keys && cap_bytes > 0)) return fail(SBWTGPU_ERR_INVALID_ARG, "out_keys is NULL");
    int rc = setop_check_index(idx, "k-mer keys");
    if (rc != SBWTGPU_OK) return rc;
    DeviceGuard guard(idx->device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", idx->device);
    Stream st;
    HIP_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    DevBuf keys;
    long long n = 0;
    const int kb = idx->h.k <= 32 ? 8 : 16;
    hipError_t e = sbwt_setops_keys(idx->view(), &keys.p, &n, st.s);
    if (e != hipSuccess) return setop_hip_fail(e, "keys");
    if (n_keys) *n_keys = n;
    if (key_bytes) *key_bytes = kb;
    if (!out_keys && cap_bytes == 0) return SBWTGPU_OK;
    if (cap_bytes < n * kb)
        return fail(SBWTGPU_ERR_INVALID_ARG, "k-mer keys: %lld keys of %d bytes need %lld bytes, cap_bytes is %lld", n, kb, n * kb,
                    (long long)cap_bytes);
    if (n > 0) HIP_TRY(hipMemcpy(out_keys, keys.p, (size_t)(n * kb), hipMemcpyDeviceToHost));
    return SBWTGPU_OK;
}

// ---- colour sets carried onto another index (sbwt_colormerge.hip) ---------------------------------------
int sbwtgpu_colorsets_merge(const sbwtgpu_index *u, const sbwtgpu_colorsets *sa, const sbwtgpu_colorsets *sb, int color_offset_b,
                            sbwtgpu_colorsets **out, sbwtgpu_colorsets_merge_info *info) {
    if (info) memset(info, 0, sizeof(*info));
    if (out) *out = nullptr;
    if (!u || !sa || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "colour-set merge: NULL argument (u, sa and out are needed)");
    int rc = colorsets_check(sa);
    if (rc == SBWTGPU_OK && sb) rc = colorsets_check(sb);
    if (rc != SBWTGPU_OK) return rc;
    const sbwtgpu_index *a = sa->base.idx, *b = sb ? sb->base.idx : nullptr;
    if (u->h.n_nodes >= ((int64_t)1 << 31))
        return fail(SBWTGPU_ERR_INVALID_ARG, "colour-set merge: u has %lld columns, a colour-set object needs fewer than 2^31 columns",
                    (long long)u->h.n_nodes);
    if (u->h.k != a->h.k || (b && b->h.k != a->h.k))
        return fail(SBWTGPU_ERR_INVALID_ARG, "colour-set merge: the indexes differ in k (u %lld, a %lld, b %lld)", (long long)u->h.k,
                    (long long)a->h.k, (long long)(b ? b->h.k : a->h.k));
    if ((rc = setop_check_index(u, "colour-set merge, u")) != SBWTGPU_OK) return rc;
    if (a != u && (rc = setop_check_index(a, "colour-set merge, a")) != SBWTGPU_OK) return rc;
    if (b && b != u && b != a && (rc = setop_check_index(b, "colour-set merge, b")) != SBWTGPU_OK) return rc;
    if (u->device != a->device || (b && b->device != a->device))
        return fail(SBWTGPU_ERR_INVALID_ARG, "colour-set merge: the indexes are on different devices (u %d, a %d, b %d)", u->device,
                    a->device, b ? b->device : a->device);
    if (color_offset_b < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "colour-set merge: color_offset_b must not be negative, not %d", color_offset_b);
    if (!sb && color_offset_b != 0)
        return fail(SBWTGPU_ERR_INVALID_ARG, "colour-set merge: color_offset_b = %d without sb (it must be 0 then)", color_offset_b);
    const int64_t n_colors_out = std::max<int64_t>(sa->base.n_colors, sb ? (int64_t)color_offset_b + sb->base.n_colors : 0);
    if (n_colors_out > SBWTGPU_MAX_COLORS)
        return fail(SBWTGPU_ERR_INVALID_ARG, "colour-set merge: color_offset_b %d + %d colours of b = %lld colours, more than %d",
                    color_offset_b, sb ? sb->base.n_colors : 0, (long long)n_colors_out, SBWTGPU_MAX_COLORS);
    DeviceGuard guard(u->device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", u->device);
    sbwtgpu_colorsets *s = colorsets_new(u, (int)n_colors_out);
    if (!s) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    SbwtCmSide A{a->view()}, B{a->view()};
    A.d_ids = sa->d_ids; A.d_table = sa->d_table; A.n_sets = sa->n_sets; A.words = sa->base.words;
    if (sb) { B.ix = b->view(); B.d_ids = sb->d_ids; B.d_table = sb->d_table; B.n_sets = sb->n_sets; B.words = sb->base.words; }
    SbwtCmInfo ci;
    Stream st;
    long long n_sets = 0;
    hipError_t e = hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking);
    if (e == hipSuccess)
        e = sbwt_colormerge(u->view(), A, sb ? &B : nullptr, u == a ? 1 : (b && u == b) ? 2 : 0, b == a, color_offset_b, s->base.words,
                            &s->d_ids, &s->d_table, &n_sets, &ci, st.s);
    s->n_sets = n_sets;
    if (e == hipSuccess) e = colorsets_count(s, st.s);
    if (e != hipSuccess) return colorsets_hip_failed(s, e);
    if (info) {
        info->n_real_u = ci.n_real_u; info->n_from_a = ci.n_from_a; info->n_from_b = ci.n_from_b; info->n_from_both = ci.n_from_both;
        info->n_pairs = ci.n_pairs; info->n_sets = ci.n_sets;
        for (int i = 0; i < 4; i++) info->pass_ms[i] = ci.pass_ms[i];
    }
    *out = s;
    return SBWTGPU_OK;
}

// ---- shared k-mers: the colours' weighted Gram matrix (sbwt_colormatrix.hip) -----------------------------
int sbwtgpu_colorsets_set_sizes(const sbwtgpu_colorsets *s, int64_t *sizes_out) {
    if (!s || !sizes_out) return fail(SBWTGPU_ERR_INVALID_ARG, "set sizes: NULL argument (s and sizes_out are needed)");
    const int rc = colorsets_check(s);
    if (rc != SBWTGPU_OK) return rc;
    DeviceGuard guard(s->base.device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", s->base.device);
    Stream st;
    DevBuf d;
    std::vector<uint32_t> h;
    try { h.resize((size_t)s->n_sets); } catch (const std::bad_alloc &) { return fail(SBWTGPU_ERR_OOM, "out of host memory"); }
    HIP_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    HIP_TRY(d.alloc((size_t)s->n_sets * 4));
    sbwt_launch_gm_sizes(s->d_ids, s->base.n_nodes, s->n_sets, static_cast<unsigned *>(d.p), st.s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h.data(), d.p, (size_t)s->n_sets * 4, hipMemcpyDeviceToHost, st.s));
    HIP_TRY(hipStreamSynchronize(st.s));
    for (int64_t t = 0; t < s->n_sets; t++) sizes_out[t] = (int64_t)h[(size_t)t];
    return SBWTGPU_OK;
}

int64_t sbwtgpu_colorsets_shared_workspace_bytes(const sbwtgpu_colorsets *s) {
    if (!s) return 0;
    DeviceGuard guard(s->base.device);
    return sbwt_gm_workspace_bytes(s->n_sets, s->base.n_colors);
}

int sbwtgpu_colorsets_shared_kmers_dev(const sbwtgpu_colorsets *s, const int64_t *d_weights_or_null, int64_t *d_matrix, void *d_workspace,
                                       int64_t workspace_bytes, void *stream) {
    if (!s || !d_matrix || !d_workspace)
        return fail(SBWTGPU_ERR_INVALID_ARG, "shared k-mers: NULL argument (s, d_matrix and d_workspace are needed)");
    const int rc = colorsets_check(s);
    if (rc != SBWTGPU_OK) return rc;
    DeviceGuard guard(s->base.device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", s->base.device);
    const int64_t need = sbwt_gm_workspace_bytes(s->n_sets, s->base.n_colors);
    if (need < 0) return fail(SBWTGPU_ERR_HIP, "shared k-mers: the sort's storage size could not be asked");
    if (workspace_bytes < need)
        return fail(SBWTGPU_ERR_INVALID_ARG, "shared k-mers: the workspace has %lld bytes, %lld sets of %d colours need %lld "
                    "(sbwtgpu_colorsets_shared_workspace_bytes)", (long long)workspace_bytes, (long long)s->n_sets, s->base.n_colors,
                    (long long)need);
    const hipError_t e = sbwt_gm_enqueue(s->d_ids, s->base.n_nodes, s->d_table, s->n_sets, s->base.n_colors,
                                         reinterpret_cast<const long long *>(d_weights_or_null), reinterpret_cast<long long *>(d_matrix),
                                         d_workspace, workspace_bytes, s->n_sets >= g_gram_mfma_min_sets, g_gram_flush_sets, nullptr,
                                         static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "shared k-mers: %s", hipGetErrorString(e));
    }
    return SBWTGPU_OK;
}

int sbwtgpu_colorsets_shared_kmers(const sbwtgpu_colorsets *s, const int64_t *weights_or_null, int64_t *matrix_out,
                                   sbwtgpu_shared_info *info) {
    if (info) memset(info, 0, sizeof(*info));
    if (!s || !matrix_out) return fail(SBWTGPU_ERR_INVALID_ARG, "shared k-mers: NULL argument (s and matrix_out are needed)");
    const int rc = colorsets_check(s);
    if (rc != SBWTGPU_OK) return rc;
    DeviceGuard guard(s->base.device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", s->base.device);
    const int C = s->base.n_colors;
    const bool use_mfma = s->n_sets >= g_gram_mfma_min_sets;
    const int64_t ws_bytes = sbwt_gm_workspace_bytes(s->n_sets, C);
    if (ws_bytes < 0) return fail(SBWTGPU_ERR_HIP, "shared k-mers: the sort's storage size could not be asked");
    const size_t m_bytes = (size_t)C * (size_t)C * 8;
    Stream st;
    DevBuf ws, w, m;
    SbwtGmHeader hdr;
    double ms[4] = {0, 0, 0, 0};
    // (the plain route touches the header and the weights only: its workspace need not hold the planes)
    const int64_t ws_alloc = use_mfma ? ws_bytes : sbwt_gm_plain_workspace_bytes(s->n_sets);
    hipError_t e = hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking);
    if (e == hipSuccess) e = ws.alloc((size_t)ws_alloc);
    if (e == hipSuccess) e = m.alloc(m_bytes);
    if (e == hipSuccess && weights_or_null) e = w.alloc((size_t)s->n_sets * 8);
    if (e == hipSuccess && weights_or_null) e = hipMemcpyAsync(w.p, weights_or_null, (size_t)s->n_sets * 8, hipMemcpyHostToDevice, st.s);
    if (e == hipSuccess)
        e = sbwt_gm_enqueue(s->d_ids, s->base.n_nodes, s->d_table, s->n_sets, C, static_cast<const long long *>(w.p),
                            static_cast<long long *>(m.p), ws.p, ws_alloc, use_mfma, g_gram_flush_sets, ms, st.s);
    const auto t0 = std::chrono::steady_clock::now();
    if (e == hipSuccess) e = hipMemcpyAsync(&hdr, ws.p, sizeof(hdr), hipMemcpyDeviceToHost, st.s);
    if (e == hipSuccess) e = hipStreamSynchronize(st.s);
    if (e == hipSuccess && hdr.status == ~0ull) e = hipMemcpy(matrix_out, m.p, m_bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "shared k-mers: %s", hipGetErrorString(e));
    }
    if (hdr.status != ~0ull)
        return fail(SBWTGPU_ERR_INVALID_ARG, "shared k-mers: the weight of set %llu is %lld, weights must be in 0 .. 2^31 - 1",
                    hdr.status, (long long)weights_or_null[hdr.status]);
    ms[3] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (info) {
        info->n_sets_used = (int64_t)hdr.n_used;
        info->n_colors = C;
        info->words = s->base.words;
        info->used_mfma = use_mfma ? 1 : 0;
        for (uint64_t x = hdr.max_w; x; x >>= 7) info->n_limbs++;
        for (int i = 0; i < 4; i++) info->pass_ms[i] = ms[i];
    }
    return SBWTGPU_OK;
}

// ---- screen: per-colour k-mer containment of a read set (sbwt_screen.hip) -----------
}  // extern "C"
// One device allocation: the counters (256 bytes), set_hits (n_sets int64) and the seen bitmap.  The adds only ever add to it
// with atomics; the queries take `mu`, run on `stream` and bring their scratch with them.
struct sbwtgpu_screen {
    const sbwtgpu_colorsets *s = nullptr;
    int device = 0;
    int64_t n_nodes = 0, n_sets = 0, n_words = 0;       // n_words = ceil(n_nodes / 64)
    DevBuf mem;
    size_t bytes = 0;
    SbwtScreenCounters *d_ctr = nullptr;
    unsigned long long *d_set_hits = nullptr, *d_seen = nullptr;
    Stream stream;
    mutable std::mutex mu;
};
static int screen_check(const sbwtgpu_screen *x) {
    if (!x) return fail(SBWTGPU_ERR_INVALID_ARG, "screen: the object is NULL");
    return colorsets_check(x->s);
}
extern "C" {

int sbwtgpu_screen_create(const sbwtgpu_colorsets *s, sbwtgpu_screen **out) {
    if (!s || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "screen: NULL argument (s and out are needed)");
    *out = nullptr;
    const int rc = colorsets_check(s);
    if (rc != SBWTGPU_OK) return rc;
    DeviceGuard guard(s->base.device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", s->base.device);
    sbwtgpu_screen *x = new (std::nothrow) sbwtgpu_screen();
    if (!x) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    x->s = s;
    x->device = s->base.device;
    x->n_nodes = s->base.n_nodes;
    x->n_sets = s->n_sets;
    x->n_words = (x->n_nodes + 63) / 64;
    const size_t o_hits = 256, o_seen = o_hits + align256((size_t)x->n_sets * 8);
    x->bytes = o_seen + align256((size_t)x->n_words * 8 + 8);
    hipError_t e = hipStreamCreateWithFlags(&x->stream.s, hipStreamNonBlocking);
    if (e == hipSuccess) e = x->mem.alloc(x->bytes);
    if (e == hipSuccess) e = hipMemsetAsync(x->mem.p, 0, x->bytes, x->stream.s);
    if (e == hipSuccess) e = hipStreamSynchronize(x->stream.s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        delete x;
        return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "screen: %s", hipGetErrorString(e));
    }
    char *m = static_cast<char *>(x->mem.p);
    x->d_ctr = reinterpret_cast<SbwtScreenCounters *>(m);
    x->d_set_hits = reinterpret_cast<unsigned long long *>(m + o_hits);
    x->d_seen = reinterpret_cast<unsigned long long *>(m + o_seen);
    *out = x;
    return SBWTGPU_OK;
}

int sbwtgpu_screen_reset(sbwtgpu_screen *x) {
    const int rc = screen_check(x);
    if (rc != SBWTGPU_OK) return rc;
    DeviceGuard guard(x->device);
    std::lock_guard<std::mutex> lock(x->mu);
    // (adds of the caller's on other streams have to be over, as for the queries: the device is waited for, then zeroed)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemsetAsync(x->mem.p, 0, x->bytes, x->stream.s));
    HIP_TRY(hipStreamSynchronize(x->stream.s));
    return SBWTGPU_OK;
}

void sbwtgpu_screen_destroy(sbwtgpu_screen *x) {
    if (!x) return;
    DeviceGuard guard(x->device);
    delete x;
}

int64_t sbwtgpu_screen_workspace_bytes(int64_t total_bases, int64_t n_reads, int strands) {
    return sbwtgpu_pseudoalign_workspace_bytes(total_bases, n_reads, strands);
}

int sbwtgpu_screen_add_dev(sbwtgpu_screen *x, const char *d_bases, int64_t total_bases, const int64_t *d_read_off, int64_t n_reads,
                           int strands, void *d_ws, int64_t ws_bytes, void *stream) {
    int rc = screen_check(x);
    if (rc == SBWTGPU_OK) rc = colors_check_batch(n_reads, strands);
    if (rc != SBWTGPU_OK) return rc;
    const sbwtgpu_colorsets *s = x->s;
    return colors_dev_common(&s->base, d_bases, total_bases, d_read_off, n_reads, strands, d_ws, ws_bytes, stream,
                             [&](const int *res, const int *res2, const long long *ooff, SbwtPaHeader *, hipStream_t st) {
                                 sbwt_launch_screen_add(res, res2, ooff, n_reads, total_bases, s->d_ids, x->n_nodes, x->n_sets, x->d_seen,
                                                        x->d_set_hits, x->d_ctr, st);
                             });
}

// Host buffers: read_hits_batch's chunks of whole reads under "screen_chunk_bases", two in flight on the parked slots of the
// search pipeline.  Bases and offsets go down; only each chunk's status word comes back.
int sbwtgpu_screen_add_batch(sbwtgpu_screen *x, const char *bases, const int64_t *read_off, int64_t n_reads, int strands) {
    int rc = screen_check(x);
    if (rc == SBWTGPU_OK) rc = colors_check_batch(n_reads, strands);
    if (rc != SBWTGPU_OK) return rc;
    if (n_reads == 0) return SBWTGPU_OK;
    if (!read_off) return fail(SBWTGPU_ERR_INVALID_ARG, "screen: NULL argument (read_off)");
    if (read_off[n_reads] > read_off[0] && !bases) return fail(SBWTGPU_ERR_INVALID_ARG, "screen: NULL argument (bases)");
    const int64_t budget = g_screen_chunk_bases > 0 ? g_screen_chunk_bases : (int64_t)64 << 20, CH_READS = (int64_t)1 << 24;
    std::vector<int64_t> cuts{0};
    int64_t max_bases = 0, max_reads = 0;
    try {
        for (int64_t lo = 0, r = 0; r < n_reads; r++) {
            if ((rc = check_read_length(read_off, r)) != SBWTGPU_OK) return rc;
            if (r > lo && (read_off[r + 1] - read_off[lo] > budget || r - lo >= CH_READS)) {
                cuts.push_back(r);
                lo = r;
            }
            max_bases = std::max(max_bases, read_off[r + 1] - read_off[lo]);
            max_reads = std::max(max_reads, r + 1 - lo);
        }
        cuts.push_back(n_reads);
    } catch (const std::bad_alloc &) {
        return fail(SBWTGPU_ERR_OOM, "out of host memory");
    }
    const int64_t n_chunks = (int64_t)cuts.size() - 1;
    const bool pin_in = is_pinned(bases);
    const int64_t ws_bytes = sbwtgpu_screen_workspace_bytes(max_bases, max_reads, strands);
    const int64_t need_in = align256(max_bases + 16) + align256((max_reads + 1) * 8);
    const int64_t need_dev = need_in + align256(ws_bytes);
    DeviceGuard guard(x->device);
    const int n_slots = n_chunks > 1 ? 2 : 1;
    PipeSlot S[2];
    if ((rc = take_slots(x->device, S, n_slots, need_in, 0, need_dev, "screen buffers")) != SBWTGPU_OK) return rc;
    int bug = 0;                    // the first nonzero device status of a chunk
    const int64_t o_roff = align256(max_bases + 16), o_ws = need_in;
    auto submit = [&](int64_t c) -> int {
        PipeSlot &P = S[c % n_slots];
        const int64_t lo = cuts[(size_t)c], hi = cuts[(size_t)c + 1], nr = hi - lo, nb = read_off[hi] - read_off[lo];
        int64_t *hro = (int64_t *)(P.h_in + o_roff);
        for (int64_t r = 0; r <= nr; r++) hro[r] = read_off[lo + r] - read_off[lo];
        const char *hb = bases + read_off[lo];
        if (!pin_in && nb > 0) { parallel_memcpy(P.h_in, hb, (size_t)nb); hb = P.h_in; }
        hipError_t e;
        if ((nb > 0 && (e = hipMemcpyAsync(P.d_mem, hb, (size_t)nb, hipMemcpyHostToDevice, P.st)) != hipSuccess) ||
            (e = hipMemcpyAsync(P.d_mem + o_roff, hro, (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, P.st)) != hipSuccess)
            return fail(SBWTGPU_ERR_HIP, "H2D copy: %s", hipGetErrorString(e));
        const int r2 = sbwtgpu_screen_add_dev(x, P.d_mem, nb, (const int64_t *)(P.d_mem + o_roff), nr, strands, P.d_mem + o_ws, ws_bytes, P.st);
        if (r2 != SBWTGPU_OK) return r2;
        const SbwtPaLayout L = sbwt_pa_layout(sbwtgpu_search_workspace_bytes(nb), nb, nr, strands);
        if ((e = hipMemcpyAsync(P.h_status, P.d_mem + o_ws + L.hdr, 4, hipMemcpyDeviceToHost, P.st)) != hipSuccess)
            return fail(SBWTGPU_ERR_HIP, "D2H copy: %s", hipGetErrorString(e));
        return SBWTGPU_OK;
    };
    auto collect = [&](int64_t c) -> int {
        PipeSlot &P = S[c % n_slots];
        hipError_t e = hipStreamSynchronize(P.st);
        if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "stream synchronize: %s", hipGetErrorString(e));
        if (P.h_status[0] != 0 && bug == 0) bug = P.h_status[0];
        return SBWTGPU_OK;
    };
    rc = two_in_flight(n_chunks, submit, collect);
    park_slots(x->device, S, n_slots, rc);
    if (rc != SBWTGPU_OK) return rc;
    if (bug) return fail_status(bug);
    return SBWTGPU_OK;
}

int sbwtgpu_screen_info(const sbwtgpu_screen *x, int64_t *n_windows, int64_t *n_hits, int64_t *n_seen, int64_t *n_sets,
                        int32_t *n_colors) {
    const int rc = screen_check(x);
    if (rc != SBWTGPU_OK) return rc;
    if (n_sets) *n_sets = x->n_sets;
    if (n_colors) *n_colors = x->s->base.n_colors;
    if (!n_windows && !n_hits && !n_seen) return SBWTGPU_OK;
    DeviceGuard guard(x->device);
    std::lock_guard<std::mutex> lock(x->mu);
    hipStream_t st = x->stream.s;
    SbwtScreenCounters h;
    unsigned long long seen = 0;
    DevBuf d;
    if (n_seen) {
        HIP_TRY(d.alloc(8));
        sbwt_launch_screen_popcount(x->d_seen, x->n_words, static_cast<unsigned long long *>(d.p), st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&seen, d.p, 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(&h, x->d_ctr, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n_windows) *n_windows = (int64_t)h.n_windows;
    if (n_hits) *n_hits = (int64_t)h.n_hits;
    if (n_seen) *n_seen = (int64_t)seen;
    return SBWTGPU_OK;
}

}  // extern "C"
// what _sets and _colors share: the per-set vectors on the device (d: [set_kmers][set_seen], n_sets int64 each; set_hits is the
// object's own), enqueued on the object's stream under its mutex
static int screen_set_vectors(const sbwtgpu_screen *x, DevBuf &d) {
    HIP_TRY(d.alloc((size_t)x->n_sets * 16));
    unsigned long long *kmers = static_cast<unsigned long long *>(d.p);
    sbwt_launch_screen_sets(x->s->d_ids, x->n_nodes, x->n_sets, x->d_seen, kmers, kmers + x->n_sets, x->stream.s);
    HIP_TRY(hipGetLastError());
    return SBWTGPU_OK;
}
extern "C" {

int sbwtgpu_screen_sets(const sbwtgpu_screen *x, int64_t *set_kmers, int64_t *set_seen, int64_t *set_hits) {
    int rc = screen_check(x);
    if (rc != SBWTGPU_OK) return rc;
    if (!set_kmers && !set_seen && !set_hits) return SBWTGPU_OK;
    DeviceGuard guard(x->device);
    std::lock_guard<std::mutex> lock(x->mu);
    hipStream_t st = x->stream.s;
    const size_t nb = (size_t)x->n_sets * 8;
    DevBuf d;
    if (set_kmers || set_seen) {
        if ((rc = screen_set_vectors(x, d)) != SBWTGPU_OK) return rc;
        if (set_kmers) HIP_TRY(hipMemcpyAsync(set_kmers, d.p, nb, hipMemcpyDeviceToHost, st));
        if (set_seen) HIP_TRY(hipMemcpyAsync(set_seen, static_cast<char *>(d.p) + nb, nb, hipMemcpyDeviceToHost, st));
    }
    if (set_hits) HIP_TRY(hipMemcpyAsync(set_hits, x->d_set_hits, nb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SBWTGPU_OK;
}

int sbwtgpu_screen_colors(const sbwtgpu_screen *x, int64_t *ref_kmers, int64_t *ref_seen, int64_t *ref_hits) {
    int rc = screen_check(x);
    if (rc != SBWTGPU_OK) return rc;
    if (!ref_kmers && !ref_seen && !ref_hits) return SBWTGPU_OK;
    DeviceGuard guard(x->device);
    std::lock_guard<std::mutex> lock(x->mu);
    hipStream_t st = x->stream.s;
    const sbwtgpu_colorsets *s = x->s;
    const int C = s->base.n_colors;
    const size_t cb = (size_t)C * 8;
    DevBuf d, ref;
    if ((rc = screen_set_vectors(x, d)) != SBWTGPU_OK) return rc;
    HIP_TRY(ref.alloc(3 * cb));
    unsigned long long *kmers = static_cast<unsigned long long *>(d.p);
    sbwt_launch_screen_expand(s->d_table, x->n_sets, s->base.words, C, kmers, kmers + x->n_sets, x->d_set_hits,
                              static_cast<unsigned long long *>(ref.p), st);
    HIP_TRY(hipGetLastError());
    if (ref_kmers) HIP_TRY(hipMemcpyAsync(ref_kmers, ref.p, cb, hipMemcpyDeviceToHost, st));
    if (ref_seen) HIP_TRY(hipMemcpyAsync(ref_seen, static_cast<char *>(ref.p) + cb, cb, hipMemcpyDeviceToHost, st));
    if (ref_hits) HIP_TRY(hipMemcpyAsync(ref_hits, static_cast<char *>(ref.p) + 2 * cb, cb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SBWTGPU_OK;
}

int sbwtgpu_screen_seen_dev(const sbwtgpu_screen *x, const uint64_t **d_seen) {
    if (!x || !d_seen) return fail(SBWTGPU_ERR_INVALID_ARG, "screen: NULL argument");
    *d_seen = reinterpret_cast<const uint64_t *>(x->d_seen);
    return SBWTGPU_OK;
}

int sbwtgpu_screen_seen_copy(const sbwtgpu_screen *x, uint64_t *seen) {
    const int rc = screen_check(x);
    if (rc != SBWTGPU_OK) return rc;
    if (!seen) return fail(SBWTGPU_ERR_INVALID_ARG, "screen: NULL argument (seen)");
    DeviceGuard guard(x->device);
    std::lock_guard<std::mutex> lock(x->mu);
    HIP_TRY(hipMemcpyAsync(seen, x->d_seen, (size_t)x->n_words * 8, hipMemcpyDeviceToHost, x->stream.s));
    HIP_TRY(hipStreamSynchronize(x->stream.s));
    return SBWTGPU_OK;
}

// ---- colour select: k-mers by a predicate over their colour sets (sbwt_colorselect.hip) ------------------
}  // extern "C"
namespace {
// the checks of all three calls; masks: include, then exclude (2 W words, what the kernels read)
int colorselect_check(const sbwtgpu_colorsets *s, const sbwtgpu_color_predicate *p, bool needs_keys, std::vector<uint64_t> &masks) {
    if (!s || !p || !p->include) return fail(SBWTGPU_ERR_INVALID_ARG, "colour select: NULL argument (s, the predicate and its include mask are needed)");
    int rc = colorsets_check(s);
    if (rc != SBWTGPU_OK) return rc;
    const int W = s->base.words, C = s->base.n_colors;
    try { masks.assign((size_t)2 * W, 0); } catch (const std::bad_alloc &) { return fail(SBWTGPU_ERR_OOM, "out of host memory"); }
    for (int w = 0; w < W; w++) {
        masks[(size_t)w] = p->include[w];
        masks[(size_t)W + w] = p->exclude_or_null ? p->exclude_or_null[w] : 0;
    }
    if (C & 63) {
        const uint64_t high = ~0ull << (C & 63);
        if (masks[(size_t)W - 1] & high)
            return fail(SBWTGPU_ERR_INVALID_ARG, "colour select: the include mask has a bit at or above n_colors = %d", C);
        if (masks[(size_t)2 * W - 1] & high)
            return fail(SBWTGPU_ERR_INVALID_ARG, "colour select: the exclude mask has a bit at or above n_colors = %d", C);
    }
    if (p->min_in < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "colour select: min_in must not be negative, not %d", p->min_in);
    if (p->max_in < p->min_in) return fail(SBWTGPU_ERR_INVALID_ARG, "colour select: max_in = %d is below min_in = %d", p->max_in, p->min_in);
    if (needs_keys) rc = setop_check_index(s->base.idx, "colour select");
    return rc;
}
int colorselect_hip_fail(hipError_t e, const char *what) {
    (void)hipGetLastError();
    if (e == hipErrorUnknown)
        return fail(SBWTGPU_ERR_HIP, "colour select, %s: the ids and the keys disagree about the selected columns (a broken object)", what);
    return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "colour select, %s: %s", what, hipGetErrorString(e));
}
// keys of the index, verdicts, counts and -- with d_res -- the selected keys (a device allocation the caller owns)
int colorselect_run(const sbwtgpu_colorsets *s, const sbwtgpu_color_predicate *p, const std::vector<uint64_t> &masks, hipStream_t st,
                    void **d_res, sbwtgpu_color_select_info *info) {
    const sbwtgpu_index *idx = s->base.idx;
    const int key_bytes = idx->h.k <= 32 ? 8 : 16;
    DevBuf keys, cols, dm;
    long long nk = 0;
    auto t0 = std::chrono::steady_clock::now();
    hipError_t e = sbwt_setops_keys(idx->view(), &keys.p, &nk, st, reinterpret_cast<unsigned **>(&cols.p));
    if (e != hipSuccess) return colorselect_hip_fail(e, "keys");
    info->pass_ms[0] = ms_since(t0);
    info->n_real = nk;
    t0 = std::chrono::steady_clock::now();
    e = dm.alloc(masks.size() * 8);
    if (e == hipSuccess) e = hipMemcpyAsync(dm.p, masks.data(), masks.size() * 8, hipMemcpyHostToDevice, st);
    SbwtCselCounts c;
    if (e == hipSuccess)
        e = sbwt_colorselect(s->d_ids, s->base.n_nodes, s->d_table, s->n_sets, s->base.words, static_cast<const unsigned long long *>(dm.p),
                             p->min_in, p->max_in, keys.p, static_cast<const unsigned *>(cols.p), nk, key_bytes, d_res, &c, st);
    if (e != hipSuccess) return colorselect_hip_fail(e, "verdicts and select");
    info->pass_ms[1] = ms_since(t0);
    info->n_selected = c.n_selected;
    info->n_sets_matched = c.n_sets_matched;
    return SBWTGPU_OK;
}
}  // namespace
extern "C" {

int sbwtgpu_colorsets_match_sets(const sbwtgpu_colorsets *s, const sbwtgpu_color_predicate *p, uint8_t *match_out) {
    if (!match_out) return fail(SBWTGPU_ERR_INVALID_ARG, "colour select: match_out is NULL");
    std::vector<uint64_t> masks;
    const int rc = colorselect_check(s, p, false, masks);
    if (rc != SBWTGPU_OK) return rc;
    DeviceGuard guard(s->base.device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", s->base.device);
    Stream st;
    DevBuf dm, dv;
    HIP_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    HIP_TRY(dm.alloc(masks.size() * 8));
    HIP_TRY(dv.alloc((size_t)s->n_sets));
    HIP_TRY(hipMemcpyAsync(dm.p, masks.data(), masks.size() * 8, hipMemcpyHostToDevice, st.s));
    sbwt_launch_csel_verdict(s->d_table, s->n_sets, s->base.words, static_cast<const unsigned long long *>(dm.p), p->min_in, p->max_in,
                             static_cast<unsigned char *>(dv.p), st.s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(match_out, dv.p, (size_t)s->n_sets, hipMemcpyDeviceToHost, st.s));
    HIP_TRY(hipStreamSynchronize(st.s));
    return SBWTGPU_OK;
}

int sbwtgpu_colorsets_select_counts(const sbwtgpu_colorsets *s, const sbwtgpu_color_predicate *p, sbwtgpu_color_select_info *info) {
    if (!info) return fail(SBWTGPU_ERR_INVALID_ARG, "colour select: info is NULL");
    memset(info, 0, sizeof(*info));
    std::vector<uint64_t> masks;
    const int rc = colorselect_check(s, p, true, masks);
    if (rc != SBWTGPU_OK) return rc;
    DeviceGuard guard(s->base.device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", s->base.device);
    Stream st;
    HIP_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    return colorselect_run(s, p, masks, st.s, nullptr, info);
}

int sbwtgpu_colorsets_select(const sbwtgpu_colorsets *s, const sbwtgpu_color_predicate *p, int build_streaming_support,
                             sbwtgpu_plain_matrix_bits *out, sbwtgpu_color_select_info *info) {
    sbwtgpu_color_select_info local;
    if (!info) info = &local;
    memset(info, 0, sizeof(*info));
    if (!out) return fail(SBWTGPU_ERR_INVALID_ARG, "colour select: out is NULL");
    memset(out, 0, sizeof(*out));
    std::vector<uint64_t> masks;
    int rc = colorselect_check(s, p, true, masks);
    if (rc != SBWTGPU_OK) return rc;
    DeviceGuard guard(s->base.device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", s->base.device);
    Stream st;
    HIP_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    const int64_t k = s->base.k;
    void *d_res = nullptr;
    rc = colorselect_run(s, p, masks, st.s, &d_res, info);
    if (rc != SBWTGPU_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    SbwtBuildState S;
    try {
        const int ra = sbwt_build_from_keys(d_res, info->n_selected, (int)k, &S, st.s);     // (S owns d_res now)
        if (ra != 0) { sbwt_build_release(&S); return fail(ra == -8 ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "colour select: builder tail"); }
        info->n_nopred = S.n_nopred;
        if ((long long)S.n_nopred * (long long)k > (1ll << 26)) {
            sbwt_build_release(&S);
            return fail(SBWTGPU_ERR_OOM, "colour select: the result has %lld predecessor-less k-mers x k = %lld dummy records (limit 2^26; "
                        "the dummies are expanded on the host).  Selections are fragmented sets and reach this limit sooner than "
                        "genomes do: dump the unitigs and use the host builder",
                        (long long)S.n_nopred, (long long)S.n_nopred * (long long)k);
        }
        rc = (k <= 32) ? build_columns_t<unsigned long long>(S, k, build_streaming_support, out)
                       : build_columns_t<unsigned __int128>(S, k, build_streaming_support, out);
    } catch (const std::bad_alloc &) {
        sbwt_build_release(&S);
        rc = fail(SBWTGPU_ERR_OOM, "out of host memory");
    }
    info->pass_ms[2] = ms_since(t0);
    return rc;
}


// ---- bubbles: variant sites of the plain unitig graph and the colours of each allele (sbwt_bubbles.hip) ----
}  // extern "C"
static_assert(sizeof(sbwtgpu_bubble) == sizeof(SbwtBubble), "the record of the ABI is the kernels' record");
struct sbwtgpu_bubbles {
    int device = 0;
    int n_colors = 0, words = 0;
    SbwtBubbleRun run;
};
// what both bubble calls ask of the handle
static int bubbles_check_handle(const sbwtgpu_unitigs *u) {
    if (!(u->graph & SBWTGPU_UNITIGS_LINKS))
        return fail(SBWTGPU_ERR_INVALID_ARG, "bubbles: the handle was made without SBWTGPU_UNITIGS_LINKS (sbwtgpu_unitigs_create_graph takes the flag)");
    if (u->colored)
        return fail(SBWTGPU_ERR_INVALID_ARG, "bubbles: a coloured handle cuts the branches at colour breaks: pass the plain handle "
                    "(sbwtgpu_unitigs_create_graph with idx) plus the colour-set object");
    return SBWTGPU_OK;
}
extern "C" {

int sbwtgpu_bubbles_create(const sbwtgpu_unitigs *u, const sbwtgpu_colorsets *s, sbwtgpu_bubbles **out) {
    if (!u || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "bubbles: NULL argument (u and out are needed)");
    *out = nullptr;
    int rc = bubbles_check_handle(u);
    if (rc != SBWTGPU_OK) return rc;
    if (s) {
        if (!(u->graph & SBWTGPU_UNITIGS_COLUMN_MAP))
            return fail(SBWTGPU_ERR_INVALID_ARG, "bubbles: branch colours need the column map, and the handle was made without "
                        "SBWTGPU_UNITIGS_COLUMN_MAP (sbwtgpu_unitigs_create_graph takes the flag)");
        if ((rc = colorsets_check(s)) != SBWTGPU_OK) return rc;
        if (s->base.n_nodes != u->n_nodes || s->base.k != u->k)
            return fail(SBWTGPU_ERR_INVALID_ARG, "bubbles: colour sets of %lld columns at k = %lld used with unitigs of an index of %lld columns at k = %lld",
                        (long long)s->base.n_nodes, (long long)s->base.k, (long long)u->n_nodes, (long long)u->k);
        if (s->base.device != u->device)
            return fail(SBWTGPU_ERR_INVALID_ARG, "bubbles: the colour sets are on device %d, the unitigs on device %d", s->base.device, u->device);
    }
    DeviceGuard guard(u->device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", u->device);
    sbwtgpu_bubbles *b = new (std::nothrow) sbwtgpu_bubbles();
    if (!b) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    b->device = u->device;
    SbwtBubbleGraph g;
    g.d_link_off = u->run.d_link_off;
    g.d_link_to = u->run.d_link_to;
    g.d_off = u->run.d_off;
    g.n_unitigs = u->run.n_unitigs;
    g.n_links = u->run.n_links;
    g.k = u->k;
    if (s) {
        b->n_colors = s->base.n_colors;
        b->words = s->base.words;
        g.d_col_unitig = u->run.d_col_unitig;
        g.n_nodes = u->n_nodes;
        g.d_ids = s->d_ids;
        g.d_table = s->d_table;
        g.words = s->base.words;
        g.n_colors = s->base.n_colors;
    }
    Stream st;
    hipError_t e = hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking);
    if (e == hipSuccess) e = sbwt_bubbles_run(g, &b->run, st.s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        delete b;
        return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "bubbles: %s", hipGetErrorString(e));
    }
    *out = b;
    return SBWTGPU_OK;
}

void sbwtgpu_bubbles_destroy(sbwtgpu_bubbles *b) {
    if (!b) return;
    DeviceGuard guard(b->device);
    if (b->run.d_rec) (void)hipFree(b->run.d_rec);
    if (b->run.d_inter) (void)hipFree(b->run.d_inter);
    if (b->run.d_uni) (void)hipFree(b->run.d_uni);
    delete b;
}

int sbwtgpu_bubbles_info(const sbwtgpu_bubbles *b, int64_t *n_bubbles, int64_t *n_snps, int32_t *n_colors, int32_t *words) {
    if (!b) return fail(SBWTGPU_ERR_INVALID_ARG, "bubbles: the object is NULL");
    if (!n_bubbles) return fail(SBWTGPU_ERR_INVALID_ARG, "bubbles: NULL argument (n_bubbles)");
    *n_bubbles = b->run.n_bubbles;
    if (n_snps) *n_snps = b->run.n_snps;
    if (n_colors) *n_colors = b->n_colors;
    if (words) *words = b->words;
    return SBWTGPU_OK;
}

int sbwtgpu_bubbles_dev(const sbwtgpu_bubbles *b, const sbwtgpu_bubble **d_rec, const uint64_t **d_inter, const uint64_t **d_union) {
    if (!b) return fail(SBWTGPU_ERR_INVALID_ARG, "bubbles: the object is NULL");
    if (!d_rec) return fail(SBWTGPU_ERR_INVALID_ARG, "bubbles: NULL argument (d_rec)");
    *d_rec = reinterpret_cast<const sbwtgpu_bubble *>(b->run.d_rec);
    if (d_inter) *d_inter = reinterpret_cast<const uint64_t *>(b->run.d_inter);
    if (d_union) *d_union = reinterpret_cast<const uint64_t *>(b->run.d_uni);
    return SBWTGPU_OK;
}

int sbwtgpu_bubbles_copy(const sbwtgpu_bubbles *b, sbwtgpu_bubble *rec, uint64_t *inter, uint64_t *uni) {
    if (!b) return fail(SBWTGPU_ERR_INVALID_ARG, "bubbles: the object is NULL");
    const int64_t n = b->run.n_bubbles;
    if (n == 0) return SBWTGPU_OK;
    if (!rec) return fail(SBWTGPU_ERR_INVALID_ARG, "bubbles: NULL argument (rec, for %lld bubbles)", (long long)n);
    if (b->words > 0 && (!inter || !uni))
        return fail(SBWTGPU_ERR_INVALID_ARG, "bubbles: NULL argument (inter and uni: the object carries branch colours)");
    DeviceGuard guard(b->device);
    HIP_TRY(hipMemcpy(rec, b->run.d_rec, (size_t)n * sizeof(sbwtgpu_bubble), hipMemcpyDeviceToHost));
    if (b->words > 0) {
        const size_t bytes = (size_t)n * 2 * (size_t)b->words * 8;
        HIP_TRY(hipMemcpy(inter, b->run.d_inter, bytes, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(uni, b->run.d_uni, bytes, hipMemcpyDeviceToHost));
    }
    return SBWTGPU_OK;
}

int sbwtgpu_bubbles_in_degrees_copy(const sbwtgpu_unitigs *u, uint32_t *indeg) {
    if (!u) return fail(SBWTGPU_ERR_INVALID_ARG, "bubbles: NULL argument (u)");
    const int rc = bubbles_check_handle(u);
    if (rc != SBWTGPU_OK) return rc;
    const int64_t n = u->run.n_unitigs;
    if (n == 0) return SBWTGPU_OK;
    if (!indeg) return fail(SBWTGPU_ERR_INVALID_ARG, "bubbles: NULL argument (indeg, for %lld unitigs)", (long long)n);
    DeviceGuard guard(u->device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", u->device);
    DevBuf d;
    Stream st;
    hipError_t e = d.alloc((size_t)n * 4);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking);
    if (e == hipSuccess) e = sbwt_bubbles_in_degrees(u->run.d_link_to, u->run.n_links, n, static_cast<unsigned *>(d.p), st.s);
    if (e == hipSuccess) e = hipMemcpyAsync(indeg, d.p, (size_t)n * 4, hipMemcpyDeviceToHost, st.s);
    if (e == hipSuccess) e = hipStreamSynchronize(st.s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "bubbles: %s", hipGetErrorString(e));
    }
    return SBWTGPU_OK;
}

int sbwtgpu_bubbles_stats(const sbwtgpu_bubbles *b, double pass_ms[4]) {
    if (!b) return fail(SBWTGPU_ERR_INVALID_ARG, "bubbles: the object is NULL");
    if (pass_ms)
        for (int i = 0; i < SBWT_BB_N_PASSES; i++) pass_ms[i] = (double)b->run.ms[i];
    return SBWTGPU_OK;
}

}  // extern "C"
