// sbwtgpu_capi_reads.cpp -- the C ABI's layers over an index and its reads that know nothing of colours: matching statistics
// with the LCS array, set operations and k-mer keys, per-read hit profiles, unitigs and their graph (links, column map,
// locate), reads threaded through the graph (walks), bubbles, genotype.  What it shares with the other files: sbwtgpu_internal.h.
#include <cstdlib>

#include "sbwtgpu_internal.h"
#include "sbwt_ms.h"
#include "sbwt_setops.h"
#include "sbwt_readhits.h"
#include "sbwt_walks.h"
#include "sbwt_bubbles.h"
#include "sbwt_colors.h"
#include "sbwt_genotype.h"

using namespace sbwt_capi;

// knobs of this file (sbwtgpu_set_tuning sets them).  Per-read hit profiles (sbwt_readhits.hip): reads of this many windows or
// more are reduced by a wave instead of a lane; the host entry point's chunk budget in bases (0: 64 Mi); 1: int64 results on
// indexes that would take int32 (tests)
int sbwt_capi::g_rh_wave_min = SBWT_RH_WAVE_MIN;
int64_t sbwt_capi::g_rh_chunk_bases = 0;
int sbwt_capi::g_rh_wide = 0;
int64_t sbwt_capi::g_wk_chunk_bases = 0;      // "walks_chunk_bases": 0 = the default of 64 Mi
int64_t sbwt_capi::g_gt_chunk_bases = 0;      // "genotype_chunk_bases": 0 = the default of 64 Mi

extern "C" {

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
    if ((rc = check_batch_dev(n_reads, total_bases, d_ws, ws_bytes, sbwtgpu_ms_workspace_bytes(total_bases))) != SBWTGPU_OK) return rc;
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
// the plain call, or with a colour view (ids, table, words) the coloured one; graph: SBWTGPU_UNITIGS_* flags
}  // extern "C"
int sbwt_capi::unitigs_create_common(const sbwtgpu_index *idx, const unsigned *d_ids, const unsigned long long *d_table, int words,
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
extern "C" {

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
    rc = check_batch_dev(n_reads, total_bases, d_ws, ws_bytes, sbwtgpu_read_hits_workspace_bytes(total_bases, n_reads, strands));
    if (rc != SBWTGPU_OK) return rc;
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
    // (the plain search where the results are int64: "wide")
    auto search = [&](const char *b, const long long *roff, const long long *oo) {
        const int64_t *ro = reinterpret_cast<const int64_t *>(roff), *o = reinterpret_cast<const int64_t *>(oo);
        return wide ? search_dev_common(idx, b, total_bases, ro, n_reads, res, o, d_ws, search_ws, stream, 0)
                    : search_dev_i32(idx, b, total_bases, ro, n_reads, reinterpret_cast<int32_t *>(res), o, d_ws, search_ws, stream, 0);
    };
    if (any) {
        if ((rc = search(d_bases, reinterpret_cast<const long long *>(d_read_off), ooff)) != SBWTGPU_OK) return rc;
        sbwt_launch_rh_bits(res, wide, ooff, n_reads, total_bases, 0, bits, sws, hdr, st);
    }
    if (strands == 2 && any) {
        char *rcb = w + L.rc;
        long long *roff2 = reinterpret_cast<long long *>(w + L.roff2), *ooff2 = reinterpret_cast<long long *>(w + L.ooff2);
        sbwt_launch_rh_mirror(d_bases, total_bases, reinterpret_cast<const long long *>(d_read_off), ooff, n_reads, rcb, roff2, ooff2, st);
        if ((rc = search(rcb, roff2, ooff2)) != SBWTGPU_OK) return rc;
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
    SbwtReadChunks ch;
    if ((rc = cut_reads(read_off, n_reads, g_rh_chunk_bases > 0 ? g_rh_chunk_bases : (int64_t)64 << 20, (int64_t)1 << 24, idx->h.k, ch)) != SBWTGPU_OK)
        return rc;
    DeviceGuard guard(idx->device);
    ReadPipe pipe(bases, read_off, ch);
    // (records into a pinned `out` land there straight from the device)
    const int rec = pipe.region(ch.max_reads * 16, true, out, 16, is_pinned(out));
    rc = pipe.open(idx->device, sbwtgpu_read_hits_workspace_bytes(ch.max_bases, ch.max_reads, strands), ch.n_chunks() > 1 ? 2 : 1, "read-hits buffers");
    if (rc != SBWTGPU_OK) return rc;
    return pipe.run([&](const ReadPipe::Chunk &c) -> int {
        STG_TRY(sbwtgpu_read_hits_dev(idx, c.bases, c.nb, c.roff, c.nr, strands, pipe.at<sbwtgpu_read_hits>(c, rec), c.ws, pipe.ws_bytes, c.P->st));
        const SbwtRhLayout L = sbwt_rh_layout(sbwtgpu_search_workspace_bytes(c.nb), c.nb, c.nr, strands);
        return pipe.fetch(c, c.ws + L.hdr, 4);
    });
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
    if ((rc = check_batch_sizes(n_reads, total_bases)) != SBWTGPU_OK) return rc;
    const unsigned long long *start = u->d_walk_start.load(std::memory_order_acquire);
    if (!start)
        return fail(SBWTGPU_ERR_INVALID_ARG, "walks: the handle is not prepared (sbwtgpu_unitigs_walks_prepare builds its start bitmap)");
    rc = check_batch_dev(n_reads, total_bases, d_ws, ws_bytes, sbwtgpu_unitigs_walks_workspace_bytes(total_bases, n_reads));
    if (rc != SBWTGPU_OK) return rc;
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
    SbwtReadChunks ch;
    if ((rc = cut_reads(read_off, n_reads, g_wk_chunk_bases > 0 ? g_wk_chunk_bases : (int64_t)64 << 20, (int64_t)1 << 24, idx->h.k, ch)) != SBWTGPU_OK)
        return rc;
    DeviceGuard guard(idx->device);
    ReadPipe pipe(bases, read_off, ch);
    // regions: [step_off][coverage][steps]; step_off comes back chunk by chunk, the coverage once, at the end
    const int r_soff = pipe.region((ch.max_reads + 1) * 8, true), r_cov = pipe.region(unitig_kmers ? n_unitigs * 8 + 8 : 0),
              r_steps = pipe.region(ch.max_windows * 16 + 16);
    if ((rc = pipe.open(idx->device, sbwtgpu_unitigs_walks_workspace_bytes(ch.max_bases, ch.max_reads), 1, "walks buffers")) != SBWTGPU_OK) return rc;
    PipeSlot &P = pipe.S[0];
    char *const d_cov = P.d_mem + pipe.reg[r_cov].off;
    sbwtgpu_walk_step *steps = nullptr;
    int64_t total = 0, cap = 0;
    auto run = [&]() -> int {
        hipError_t e;
        if (unitig_kmers && n_unitigs > 0 && (e = hipMemsetAsync(d_cov, 0, (size_t)n_unitigs * 8, P.st)) != hipSuccess)
            return fail(SBWTGPU_ERR_HIP, "memset: %s", hipGetErrorString(e));
        for (int64_t c = 0; c < ch.n_chunks(); c++) {
            ReadPipe::Chunk k;
            STG_TRY(pipe.stage(c, k));
            const int64_t lo = k.lo, nr = k.nr;
            sbwtgpu_walk_step *d_steps = pipe.at<sbwtgpu_walk_step>(k, r_steps);
            STG_TRY(sbwtgpu_unitigs_walks_dev(idx, u, k.bases, k.nb, k.roff, nr, pipe.at<int64_t>(k, r_soff), d_steps, ch.max_windows,
                                              unitig_kmers ? (int64_t *)d_cov : nullptr, k.ws, pipe.ws_bytes, P.st));
            const int64_t *so = (const int64_t *)pipe.fetch_region(k, r_soff, (nr + 1) * 8);
            if (!so) return SBWTGPU_ERR_HIP;
            STG_TRY(pipe.fetch(k, k.ws + offsetof(SbwtWorkHeader, status), 4));
            if ((e = hipStreamSynchronize(P.st)) != hipSuccess) return fail(SBWTGPU_ERR_HIP, "D2H copy: %s", hipGetErrorString(e));
            pipe.note_status(P);
            const int64_t ns = so[nr];
            for (int64_t r = 1; r <= nr; r++) step_off[lo + r] = total + so[r];
            if (ns > 0) {
                if (total + ns > cap) {
                    const int64_t want = std::max(total + ns, cap + cap / 2);
                    void *q = realloc(steps, (size_t)want * sizeof(sbwtgpu_walk_step));
                    if (!q) return fail(SBWTGPU_ERR_OOM, "out of host memory");
                    steps = static_cast<sbwtgpu_walk_step *>(q);
                    cap = want;
                }
                if ((e = hipMemcpyAsync(steps + total, d_steps, (size_t)ns * sizeof(sbwtgpu_walk_step), hipMemcpyDeviceToHost, P.st)) != hipSuccess ||
                    (e = hipStreamSynchronize(P.st)) != hipSuccess)
                    return fail(SBWTGPU_ERR_HIP, "D2H copy: %s", hipGetErrorString(e));
                total += ns;
            }
        }
        if (unitig_kmers && n_unitigs > 0 &&
            ((e = hipMemcpyAsync(unitig_kmers, d_cov, (size_t)n_unitigs * 8, hipMemcpyDeviceToHost, P.st)) != hipSuccess ||
             (e = hipStreamSynchronize(P.st)) != hipSuccess))
            return fail(SBWTGPU_ERR_HIP, "D2H copy: %s", hipGetErrorString(e));
        return SBWTGPU_OK;
    };
    if ((rc = pipe.finish(run())) != SBWTGPU_OK) {
        free(steps);
        return rc;
    }
    *steps_out = steps;
    *n_steps = total;
    return SBWTGPU_OK;
}

// ---- set operations (sbwt_setops.hip) ---------------------------------------------------------------
}  // extern "C"
// what the label extraction needs of an index: the unitig pass's conditions, and a key of 64 or 128 bits
int sbwt_capi::setop_check_index(const sbwtgpu_index *idx, const char *who) {
    if (idx->h.rank_only) return fail(SBWTGPU_ERR_INVALID_ARG, "%s", RANK_ONLY_MSG);
    if (idx->h.k < 2 || idx->h.k > 64)
        return fail(SBWTGPU_ERR_INVALID_ARG, "%s: k = %lld, the keys of the device builder hold 2 <= k <= 64", who, (long long)idx->h.k);
    if (idx->h.n_nodes >= ((int64_t)1 << 32) - ((int64_t)1 << 24))
        return fail(SBWTGPU_ERR_INVALID_ARG, "%s: columns are 32-bit unsigned values (%lld columns)", who, (long long)idx->h.n_nodes);
    return SBWTGPU_OK;
}
namespace {
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
        rc = build_columns(S, k, build_streaming_support, out);
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

// ---- genotype: per-allele k-mer depth of a read set at the bubbles, and calls (sbwt_genotype.hip) ----
}  // extern "C"
// The adds only ever add to the state with atomics; the queries take `mu`, run on `stream` and bring their scratch with them.
struct sbwtgpu_genotype {
    const sbwtgpu_index *idx = nullptr;
    const sbwtgpu_unitigs *u = nullptr;
    int device = 0;
    int n_colors = 0, words = 0;
    SbwtGenotypeState st;
    Stream stream;
    mutable std::mutex mu;
};
// the object, and that its index and handle still are what it was made from
static int genotype_check(const sbwtgpu_genotype *g) {
    if (!g) return fail(SBWTGPU_ERR_INVALID_ARG, "genotype: the object is NULL");
    if (g->idx->h.n_nodes != g->st.n_nodes || g->u->n_nodes != g->st.n_nodes)
        return fail(SBWTGPU_ERR_INVALID_ARG, "genotype: the object was made for %lld columns, its index has %lld and its handle %lld",
                    (long long)g->st.n_nodes, (long long)g->idx->h.n_nodes, (long long)g->u->n_nodes);
    return SBWTGPU_OK;
}
extern "C" {

int sbwtgpu_genotype_create(const sbwtgpu_index *idx, const sbwtgpu_unitigs *u, const sbwtgpu_bubbles *b, sbwtgpu_genotype **out) {
    if (!idx || !u || !b || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "genotype: NULL argument (idx, u, b and out are needed)");
    *out = nullptr;
    // (the size first, as the colour layer does: an index of that size is refused for it whatever else is wrong with the call)
    if (idx->h.n_nodes >= ((int64_t)1 << 31))
        return fail(SBWTGPU_ERR_INVALID_ARG, "genotype: the index has %lld columns, the adds read int32 search results (fewer than 2^31 columns)",
                    (long long)idx->h.n_nodes);
    if (idx->h.rank_only) return fail(SBWTGPU_ERR_INVALID_ARG, "%s", RANK_ONLY_MSG);
    if (u->colored)
        return fail(SBWTGPU_ERR_INVALID_ARG, "genotype: a coloured handle cuts the branches at colour breaks: pass the plain handle "
                    "(sbwtgpu_unitigs_create_graph with idx) the bubbles were made from");
    if (!(u->graph & SBWTGPU_UNITIGS_LINKS))
        return fail(SBWTGPU_ERR_INVALID_ARG, "genotype: the handle was made without SBWTGPU_UNITIGS_LINKS (sbwtgpu_unitigs_create_graph takes the flag)");
    if (!(u->graph & SBWTGPU_UNITIGS_COLUMN_MAP))
        return fail(SBWTGPU_ERR_INVALID_ARG, "genotype: the handle was made without SBWTGPU_UNITIGS_COLUMN_MAP (sbwtgpu_unitigs_create_graph takes the flag)");
    if (u->n_nodes != idx->h.n_nodes || u->k != idx->h.k || u->device != idx->device)
        return fail(SBWTGPU_ERR_INVALID_ARG, "genotype: the handle (%lld columns, k = %lld, device %d) was not made from this index (%lld columns, k = %lld, device %d)",
                    (long long)u->n_nodes, (long long)u->k, u->device, (long long)idx->h.n_nodes, (long long)idx->h.k, idx->device);
    if (b->device != u->device)
        return fail(SBWTGPU_ERR_INVALID_ARG, "genotype: the bubbles are on device %d, the unitigs on device %d", b->device, u->device);
    DeviceGuard guard(u->device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", u->device);
    sbwtgpu_genotype *g = new (std::nothrow) sbwtgpu_genotype();
    if (!g) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    g->idx = idx;
    g->u = u;
    g->device = u->device;
    g->n_colors = b->n_colors;
    g->words = b->words;
    SbwtGenotypeGraph gg;
    gg.d_rec = b->run.d_rec;
    gg.d_inter = b->words > 0 ? b->run.d_inter : nullptr;
    gg.n_bubbles = b->run.n_bubbles;
    gg.words = b->words;
    gg.d_off = u->run.d_off;
    gg.n_unitigs = u->run.n_unitigs;
    gg.k = u->k;
    gg.d_col_unitig = u->run.d_col_unitig;
    gg.d_col_offset = u->run.d_col_offset;
    gg.n_nodes = u->n_nodes;
    int bad = 0;
    hipError_t e = hipStreamCreateWithFlags(&g->stream.s, hipStreamNonBlocking);
    if (e == hipSuccess) e = sbwt_genotype_build(gg, &g->st, &bad, g->stream.s);
    if (e != hipSuccess || bad) {
        (void)hipGetLastError();
        delete g;
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "genotype: %s", hipGetErrorString(e));
        return fail(SBWTGPU_ERR_INVALID_ARG, "genotype: the bubbles do not fit the handle (%s): they were made from another handle",
                    (bad & SBWT_GT_BAD_UNITIG) ? "a record names a unitig the handle does not have, or its n_kmers is not that unitig's k-mer count"
                    : (bad & SBWT_GT_BAD_SHARED) ? "two branches name one unitig"
                                                 : "the branch columns of the column map are not the k-mers of the records");
    }
    *out = g;
    return SBWTGPU_OK;
}

int sbwtgpu_genotype_reset(sbwtgpu_genotype *g) {
    const int rc = genotype_check(g);
    if (rc != SBWTGPU_OK) return rc;
    DeviceGuard guard(g->device);
    std::lock_guard<std::mutex> lock(g->mu);
    // (adds of the caller's on other streams have to be over, as for the queries: the device is waited for, then zeroed)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemsetAsync(g->st.d_acc, 0, g->st.acc_bytes, g->stream.s));
    HIP_TRY(hipStreamSynchronize(g->stream.s));
    return SBWTGPU_OK;
}

void sbwtgpu_genotype_destroy(sbwtgpu_genotype *g) {
    if (!g) return;
    DeviceGuard guard(g->device);
    sbwt_genotype_free(&g->st);
    delete g;
}

int64_t sbwtgpu_genotype_workspace_bytes(int64_t total_bases, int64_t n_reads, int strands) {
    return sbwtgpu_pseudoalign_workspace_bytes(total_bases, n_reads, strands);
}

int sbwtgpu_genotype_add_dev(sbwtgpu_genotype *g, const char *d_bases, int64_t total_bases, const int64_t *d_read_off, int64_t n_reads,
                             int strands, void *d_ws, int64_t ws_bytes, void *stream) {
    int rc = genotype_check(g);
    if (rc == SBWTGPU_OK) rc = check_strands_batch("genotype: ", n_reads, strands);
    if (rc != SBWTGPU_OK) return rc;
    StrandSearch q;
    STG_TRY(search_strands_dev(g->idx, d_bases, total_bases, d_read_off, n_reads, strands, d_ws, ws_bytes, stream, q));
    if (!q.enqueued) return SBWTGPU_OK;
    DeviceGuard guard(g->device);
    sbwt_launch_genotype_add(q.res, q.res2, q.ooff, n_reads, total_bases, g->st, static_cast<hipStream_t>(stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return SBWTGPU_OK;
}

// Host buffers: read_hits_batch's chunks of whole reads under "genotype_chunk_bases", two in flight on the parked slots of the
// search pipeline.  Bases and offsets go down; only each chunk's status word comes back.
int sbwtgpu_genotype_add_batch(sbwtgpu_genotype *g, const char *bases, const int64_t *read_off, int64_t n_reads, int strands) {
    int rc = genotype_check(g);
    if (rc == SBWTGPU_OK) rc = check_strands_batch("genotype: ", n_reads, strands);
    if (rc != SBWTGPU_OK) return rc;
    if (n_reads == 0) return SBWTGPU_OK;
    if (!read_off) return fail(SBWTGPU_ERR_INVALID_ARG, "genotype: NULL argument (read_off)");
    if (read_off[n_reads] > read_off[0] && !bases) return fail(SBWTGPU_ERR_INVALID_ARG, "genotype: NULL argument (bases)");
    SbwtReadChunks ch;
    rc = cut_reads(read_off, n_reads, g_gt_chunk_bases > 0 ? g_gt_chunk_bases : (int64_t)64 << 20, (int64_t)1 << 24, g->idx->h.k, ch);
    if (rc != SBWTGPU_OK) return rc;
    DeviceGuard guard(g->device);
    ReadPipe pipe(bases, read_off, ch);
    rc = pipe.open(g->device, sbwtgpu_genotype_workspace_bytes(ch.max_bases, ch.max_reads, strands), ch.n_chunks() > 1 ? 2 : 1, "genotype buffers");
    if (rc != SBWTGPU_OK) return rc;
    return pipe.run([&](const ReadPipe::Chunk &c) -> int {
        STG_TRY(sbwtgpu_genotype_add_dev(g, c.bases, c.nb, c.roff, c.nr, strands, c.ws, pipe.ws_bytes, c.P->st));
        const SbwtPaLayout L = sbwt_pa_layout(sbwtgpu_search_workspace_bytes(c.nb), c.nb, c.nr, strands);
        return pipe.fetch(c, c.ws + L.hdr, 4);
    });
}

int sbwtgpu_genotype_info(const sbwtgpu_genotype *g, int64_t *n_bubbles, int64_t *n_branch_kmers, int64_t *n_windows, int64_t *n_hits,
                          int64_t *n_site_hits, int32_t *n_colors) {
    const int rc = genotype_check(g);
    if (rc != SBWTGPU_OK) return rc;
    if (n_bubbles) *n_bubbles = g->st.n_bubbles;
    if (n_branch_kmers) *n_branch_kmers = g->st.n_positions;
    if (n_colors) *n_colors = g->n_colors;
    if (!n_windows && !n_hits && !n_site_hits) return SBWTGPU_OK;
    DeviceGuard guard(g->device);
    std::lock_guard<std::mutex> lock(g->mu);
    SbwtGenotypeCounters h;
    HIP_TRY(hipMemcpyAsync(&h, g->st.ctr(), sizeof(h), hipMemcpyDeviceToHost, g->stream.s));
    HIP_TRY(hipStreamSynchronize(g->stream.s));
    if (n_windows) *n_windows = (int64_t)h.n_windows;
    if (n_hits) *n_hits = (int64_t)h.n_hits;
    if (n_site_hits) *n_site_hits = (int64_t)h.n_site_hits;
    return SBWTGPU_OK;
}

int sbwtgpu_genotype_branches(const sbwtgpu_genotype *g, int64_t *seen, int64_t *hits, int64_t *min_hits) {
    const int rc = genotype_check(g);
    if (rc != SBWTGPU_OK) return rc;
    const int64_t n_slots = 2 * g->st.n_bubbles;
    if (n_slots == 0 || (!seen && !hits && !min_hits)) return SBWTGPU_OK;
    DeviceGuard guard(g->device);
    std::lock_guard<std::mutex> lock(g->mu);
    hipStream_t st = g->stream.s;
    const size_t nb = (size_t)n_slots * 8;
    DevBuf d;
    HIP_TRY(d.alloc(3 * nb));
    long long *v = static_cast<long long *>(d.p);
    sbwt_launch_genotype_branches(g->st, v, v + n_slots, v + 2 * n_slots, st);
    HIP_TRY(hipGetLastError());
    if (seen) HIP_TRY(hipMemcpyAsync(seen, v, nb, hipMemcpyDeviceToHost, st));
    if (hits) HIP_TRY(hipMemcpyAsync(hits, v + n_slots, nb, hipMemcpyDeviceToHost, st));
    if (min_hits) HIP_TRY(hipMemcpyAsync(min_hits, v + 2 * n_slots, nb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SBWTGPU_OK;
}

int sbwtgpu_genotype_kmer_hits_copy(const sbwtgpu_genotype *g, int64_t *branch_off, uint64_t *kmer_hits) {
    const int rc = genotype_check(g);
    if (rc != SBWTGPU_OK) return rc;
    if (!branch_off && !kmer_hits) return SBWTGPU_OK;
    DeviceGuard guard(g->device);
    std::lock_guard<std::mutex> lock(g->mu);
    hipStream_t st = g->stream.s;
    if (branch_off) HIP_TRY(hipMemcpyAsync(branch_off, g->st.d_branch_off, (size_t)(2 * g->st.n_bubbles + 1) * 8, hipMemcpyDeviceToHost, st));
    if (kmer_hits && g->st.n_positions > 0)
        HIP_TRY(hipMemcpyAsync(kmer_hits, g->st.kmer_hits(), (size_t)g->st.n_positions * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SBWTGPU_OK;
}

int sbwtgpu_genotype_calls(const sbwtgpu_genotype *g, int32_t breadth_ppm, int64_t min_depth, uint8_t *call, int64_t *ref_sites,
                           int64_t *ref_match, int64_t *ref_only) {
    const int rc = genotype_check(g);
    if (rc != SBWTGPU_OK) return rc;
    if (breadth_ppm < 1 || breadth_ppm > 1000000)
        return fail(SBWTGPU_ERR_INVALID_ARG, "genotype: breadth_ppm must be in 1 .. 1000000, not %d", (int)breadth_ppm);
    if (min_depth < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "genotype: min_depth must not be negative (%lld)", (long long)min_depth);
    const bool colours = ref_sites || ref_match || ref_only;
    if (colours && g->words == 0)
        return fail(SBWTGPU_ERR_INVALID_ARG, "genotype: the object was made from bubbles without colours (sbwtgpu_bubbles_create with a "
                    "colour-set object carries them): ref_sites, ref_match and ref_only must be NULL");
    if (!call && !colours) return SBWTGPU_OK;
    DeviceGuard guard(g->device);
    std::lock_guard<std::mutex> lock(g->mu);
    hipStream_t st = g->stream.s;
    const int64_t B = g->st.n_bubbles, n_slots = 2 * B;
    const size_t nb = (size_t)n_slots * 8, cb = (size_t)g->n_colors * 8;
    // scratch: [seen][hits][min_hits][ref: sites, match, only][call]
    DevBuf d;
    HIP_TRY(d.alloc(3 * nb + 3 * cb + (size_t)B));
    long long *v = static_cast<long long *>(d.p);
    unsigned long long *ref = colours ? reinterpret_cast<unsigned long long *>(static_cast<char *>(d.p) + 3 * nb) : nullptr;
    unsigned char *d_call = reinterpret_cast<unsigned char *>(static_cast<char *>(d.p) + 3 * nb + 3 * cb);
    sbwt_launch_genotype_branches(g->st, v, v + n_slots, v + 2 * n_slots, st);
    sbwt_launch_genotype_calls(g->st, v, v + n_slots, breadth_ppm, min_depth, g->words, g->n_colors, call ? d_call : nullptr, ref, st);
    HIP_TRY(hipGetLastError());
    if (call && B > 0) HIP_TRY(hipMemcpyAsync(call, d_call, (size_t)B, hipMemcpyDeviceToHost, st));
    if (ref_sites) HIP_TRY(hipMemcpyAsync(ref_sites, ref, cb, hipMemcpyDeviceToHost, st));
    if (ref_match) HIP_TRY(hipMemcpyAsync(ref_match, reinterpret_cast<char *>(ref) + cb, cb, hipMemcpyDeviceToHost, st));
    if (ref_only) HIP_TRY(hipMemcpyAsync(ref_only, reinterpret_cast<char *>(ref) + 2 * cb, cb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SBWTGPU_OK;
}

}  // extern "C"