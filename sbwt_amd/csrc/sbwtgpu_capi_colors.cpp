// sbwtgpu_capi_colors.cpp -- the C ABI's colour layers: colours and pseudoalignment, deduplicated colour sets and their
// builder, coloured unitigs and the unitig graph's create call (they take a colour-set object), colour sets carried onto a
// merged index, shared k-mers, screen, colour select.  What it shares with the other files: sbwtgpu_internal.h.
#include "sbwtgpu_internal.h"
#include "sbwt_readhits.h"
#include "sbwt_setops.h"
#include "sbwt_colors.h"
#include "sbwt_colorsets.h"
#include "sbwt_colormerge.h"
#include "sbwt_colormatrix.h"
#include "sbwt_colorselect.h"
#include "sbwt_screen.h"

using namespace sbwt_capi;

// knobs of this file (sbwtgpu_set_tuning sets them)
int64_t sbwt_capi::g_pa_chunk_bases = 0;      // "pseudoalign_chunk_bases": 0 = the default of 64 Mi
int64_t sbwt_capi::g_screen_chunk_bases = 0;  // "screen_chunk_bases": 0 = the default of 64 Mi
// shared k-mers (sbwt_colormatrix.hip): objects of this many sets or more go to the matrix cores, smaller ones to the plain
// kernel; the sets a wave adds up in 32 bits before it adds into the 64-bit matrix.  Neither shows in a result.
int64_t sbwt_capi::g_gram_mfma_min_sets = SBWT_GM_MIN_SETS_DEFAULT;
int64_t sbwt_capi::g_gram_flush_sets = SBWT_GM_FLUSH_DEFAULT;

extern "C" {

// ---- colours and pseudoalignment (sbwt_colors.hip) ----------------------------------------------------
static_assert(sizeof(sbwtgpu_pseudoalignment) == sizeof(SbwtPseudoalignment), "the record of the ABI is the kernels' record");
static_assert(sizeof(sbwtgpu_read_found) == sizeof(SbwtReadFound), "the wide record of the ABI is the kernels' record");


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

// What colouring, the queries, screen and the genotype adds share: the result offsets, the int32 search of the batch and, for
// two strands, of the mirrored batch into the second result buffer (res2: NULL with one strand, and for a batch without any
// window, whose result buffers nobody wrote).  The workspace is that of sbwtgpu_pseudoalign_workspace_bytes.
}  // extern "C"
int sbwt_capi::search_strands_dev(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                                  int64_t n_reads, int strands, void *d_ws, int64_t ws_bytes, void *stream, StrandSearch &out) {
    out = StrandSearch();
    STG_TRY(check_batch_dev(n_reads, total_bases, d_ws, ws_bytes, sbwtgpu_pseudoalign_workspace_bytes(total_bases, n_reads, strands)));
    if (n_reads == 0) return SBWTGPU_OK;
    if (!d_read_off || (total_bases > 0 && !d_bases)) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL device pointer");
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
    // (a batch of fewer than k bases has no window: nothing to search, and the caller's tail reads no result)
    const bool any = total_bases >= k;
    const SbwtWorkHeader *sws = reinterpret_cast<const SbwtWorkHeader *>(w);
    int *res2 = nullptr;
    int rc;
    if (any) {
        rc = search_dev_i32(idx, d_bases, total_bases, d_read_off, n_reads, res, reinterpret_cast<const int64_t *>(ooff), d_ws, search_ws,
                            stream, 0);
        if (rc != SBWTGPU_OK) return rc;
        sbwt_launch_pa_note_status(sws, hdr, st);
    }
    if (strands == 2 && any) {
        res2 = reinterpret_cast<int *>(w + L.res2);
        char *rcb = w + L.rc;
        long long *roff2 = reinterpret_cast<long long *>(w + L.roff2), *ooff2 = reinterpret_cast<long long *>(w + L.ooff2);
        sbwt_launch_rh_mirror(d_bases, total_bases, reinterpret_cast<const long long *>(d_read_off), ooff, n_reads, rcb, roff2, ooff2, st);
        rc = search_dev_i32(idx, rcb, total_bases, reinterpret_cast<const int64_t *>(roff2), n_reads, res2,
                            reinterpret_cast<const int64_t *>(ooff2), d_ws, search_ws, stream, 0);
        if (rc != SBWTGPU_OK) return rc;
        sbwt_launch_pa_note_status(sws, hdr, st);
    }
    out.res = res;
    out.res2 = res2;
    out.ooff = ooff;
    out.hdr = hdr;
    out.hdr_off = L.hdr;
    out.enqueued = true;
    return SBWTGPU_OK;
}
// `tail` enqueues what turns the results into bits or records
template <typename Tail>
static int colors_dev_common(const sbwtgpu_colors *c, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                             int64_t n_reads, int strands, void *d_ws, int64_t ws_bytes, void *stream, Tail tail) {
    StrandSearch q;
    STG_TRY(search_strands_dev(c->idx, d_bases, total_bases, d_read_off, n_reads, strands, d_ws, ws_bytes, stream, q));
    if (!q.enqueued) return SBWTGPU_OK;
    DeviceGuard guard(c->idx->device);
    tail(q.res, q.res2, q.ooff, static_cast<SbwtPaHeader *>(q.hdr), static_cast<hipStream_t>(stream));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return SBWTGPU_OK;
}
extern "C" {

int sbwtgpu_pseudoalign_dev(const sbwtgpu_colors *c, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                            int64_t n_reads, int strands, int threshold_ppm, int denominator, sbwtgpu_pseudoalignment *d_out,
                            int32_t *d_counts_or_null, void *d_ws, int64_t ws_bytes, void *stream) {
    int rc = colors_check(c);
    if (rc == SBWTGPU_OK) rc = check_strands_batch("", n_reads, strands);
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
    if (rc == SBWTGPU_OK) rc = check_strands_batch("", n_reads, strands);
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
    const int64_t CH_READS = std::min((int64_t)1 << 24, std::max<int64_t>(1, (((int64_t)1 << 24) * 272) / per_read));
    SbwtReadChunks ch;
    int rc = cut_reads(read_off, n_reads, g_pa_chunk_bases > 0 ? g_pa_chunk_bases : (int64_t)64 << 20, CH_READS, k, ch);
    if (rc != SBWTGPU_OK) return rc;
    DeviceGuard guard(idx->device);
    ReadPipe pipe(bases, read_off, ch);
    // regions: [records][colour words][counts], each there only if the call has it
    const int r_rec = pipe.region(out ? ch.max_reads * rec_bytes : 0, true, out, rec_bytes),
              r_col = pipe.region(wide_colors ? ch.max_reads * nw * 8 : 0, true, wide_colors, nw * 8),
              r_cnt = pipe.region(counts ? ch.max_reads * nc * 4 : 0, true, counts, nc * 4);
    rc = pipe.open(idx->device, sbwtgpu_pseudoalign_workspace_bytes(ch.max_bases, ch.max_reads, strands), ch.n_chunks() > 1 ? 2 : 1,
                   "pseudoalignment buffers");
    if (rc != SBWTGPU_OK) return rc;
    int64_t hits = 0;
    rc = pipe.run(
        [&](const ReadPipe::Chunk &q) -> int {
            const int64_t nr = q.nr, nb = q.nb, ws_bytes = pipe.ws_bytes;
            int32_t *d_cnt = counts ? pipe.at<int32_t>(q, r_cnt) : nullptr;
            hipStream_t st_q = q.P->st;
            int r2;
            if (sets) {
                r2 = sbwtgpu_pseudoalign_sets_dev(sets, q.bases, nb, q.roff, nr, strands, threshold_ppm, denominator,
                                                  pipe.at<sbwtgpu_read_found>(q, r_rec), pipe.at<uint64_t>(q, r_col), d_cnt, q.ws, ws_bytes, st_q);
            } else if (wide_colors) {
                r2 = sbwtgpu_pseudoalign_wide_dev(c, q.bases, nb, q.roff, nr, strands, threshold_ppm, denominator,
                                                  pipe.at<sbwtgpu_read_found>(q, r_rec), pipe.at<uint64_t>(q, r_col), d_cnt, q.ws, ws_bytes, st_q);
            } else if (out) {
                r2 = sbwtgpu_pseudoalign_dev(c, q.bases, nb, q.roff, nr, strands, threshold_ppm, denominator,
                                             pipe.at<sbwtgpu_pseudoalignment>(q, r_rec), d_cnt, q.ws, ws_bytes, st_q);
            } else if (marks) {
                r2 = colors_dev_common(c, q.bases, nb, q.roff, nr, strands, q.ws, ws_bytes, st_q,
                                       [&](const int *res, const int *res2, const long long *ooff, SbwtPaHeader *hdr, hipStream_t st) {
                                           sbwt_launch_csb_mark(res, res2, ooff, nr, nb, marks, c->n_nodes, 1, hdr, st);
                                           if (res2) sbwt_launch_csb_mark(res2, nullptr, ooff, nr, nb, marks, c->n_nodes, 0, hdr, st);
                                       });
            } else {
                r2 = colors_dev_common(c, q.bases, nb, q.roff, nr, strands, q.ws, ws_bytes, st_q,
                                       [&](const int *res, const int *res2, const long long *ooff, SbwtPaHeader *hdr, hipStream_t st) {
                                           sbwt_launch_col_mark(res, res2, ooff, nr, nb, c->d_rows, c->n_nodes, c->words, color, 1, hdr, st);
                                           if (res2)
                                               sbwt_launch_col_mark(res2, nullptr, ooff, nr, nb, c->d_rows, c->n_nodes, c->words, color, 0, hdr, st);
                                       });
            }
            if (r2 != SBWTGPU_OK) return r2;
            const SbwtPaLayout L = sbwt_pa_layout(sbwtgpu_search_workspace_bytes(nb), nb, nr, strands);
            return pipe.fetch(q, q.ws + L.hdr, 16);         // (status, and SbwtPaHeader::n_hit behind it)
        },
        [&](const PipeSlot &P) {
            unsigned long long nh;
            memcpy(&nh, P.h_status + 2, 8);                  // (SbwtPaHeader::n_hit)
            hits += (int64_t)nh;
        });
    if (rc != SBWTGPU_OK) return rc;
    if (n_windows) *n_windows = ch.windows;
    if (n_hit) *n_hit = hits;
    return SBWTGPU_OK;
}

int sbwtgpu_colors_add_batch(sbwtgpu_colors *c, int color, const char *bases, const int64_t *read_off, int64_t n_reads, int strands,
                             int64_t *n_windows, int64_t *n_hit_windows) {
    int rc = colors_check(c);
    if (rc == SBWTGPU_OK) rc = check_strands_batch("", n_reads, strands);
    if (rc != SBWTGPU_OK) return rc;
    if (color < 0 || color >= c->n_colors)
        return fail(SBWTGPU_ERR_INVALID_ARG, "color %d is out of range: the colours object has %d colours", color, c->n_colors);
    return colors_host_batch(c, bases, read_off, n_reads, strands, color, 0, 0, nullptr, nullptr, nullptr, n_windows, n_hit_windows);
}

int sbwtgpu_pseudoalign_batch(const sbwtgpu_colors *c, const char *bases, const int64_t *read_off, int64_t n_reads, int strands,
                              int threshold_ppm, int denominator, sbwtgpu_pseudoalignment *out, int32_t *counts_or_null) {
    int rc = colors_check(c);
    if (rc == SBWTGPU_OK) rc = check_strands_batch("", n_reads, strands);
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
    if (rc == SBWTGPU_OK) rc = check_strands_batch("", n_reads, strands);
    if (rc == SBWTGPU_OK) rc = colors_check_query(threshold_ppm, denominator);
    if (rc != SBWTGPU_OK) return rc;
    if (n_reads > 0 && (!out || !colors_out)) return fail(SBWTGPU_ERR_INVALID_ARG, "NULL argument");
    return colors_host_batch(c, bases, read_off, n_reads, strands, 0, threshold_ppm, denominator, out, colors_out, counts_or_null,
                             nullptr, nullptr);
}

// ---- deduplicated colour sets (sbwt_colorsets.hip) -----------------------------------------------------
}  // extern "C"
int sbwt_capi::colorsets_check(const sbwtgpu_colorsets *s) {
    if (!s) return fail(SBWTGPU_ERR_INVALID_ARG, "colour-set object is NULL");
    return colors_check(&s->base);
}
extern "C" {

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
    if (rc == SBWTGPU_OK) rc = check_strands_batch("", n_reads, strands);
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
    if (rc == SBWTGPU_OK) rc = check_strands_batch("", n_reads, strands);
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
    if (rc == SBWTGPU_OK) rc = check_strands_batch("", n_reads, strands);
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
    if (rc == SBWTGPU_OK) rc = check_strands_batch("", n_reads, strands);
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
    if (rc == SBWTGPU_OK) rc = check_strands_batch("", n_reads, strands);
    if (rc != SBWTGPU_OK) return rc;
    if (n_reads == 0) return SBWTGPU_OK;
    if (!read_off) return fail(SBWTGPU_ERR_INVALID_ARG, "screen: NULL argument (read_off)");
    if (read_off[n_reads] > read_off[0] && !bases) return fail(SBWTGPU_ERR_INVALID_ARG, "screen: NULL argument (bases)");
    SbwtReadChunks ch;
    rc = cut_reads(read_off, n_reads, g_screen_chunk_bases > 0 ? g_screen_chunk_bases : (int64_t)64 << 20, (int64_t)1 << 24, x->s->base.k, ch);
    if (rc != SBWTGPU_OK) return rc;
    DeviceGuard guard(x->device);
    ReadPipe pipe(bases, read_off, ch);
    rc = pipe.open(x->device, sbwtgpu_screen_workspace_bytes(ch.max_bases, ch.max_reads, strands), ch.n_chunks() > 1 ? 2 : 1, "screen buffers");
    if (rc != SBWTGPU_OK) return rc;
    return pipe.run([&](const ReadPipe::Chunk &c) -> int {
        STG_TRY(sbwtgpu_screen_add_dev(x, c.bases, c.nb, c.roff, c.nr, strands, c.ws, pipe.ws_bytes, c.P->st));
        const SbwtPaLayout L = sbwt_pa_layout(sbwtgpu_search_workspace_bytes(c.nb), c.nb, c.nr, strands);
        return pipe.fetch(c, c.ws + L.hdr, 4);
    });
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
        rc = build_columns(S, k, build_streaming_support, out);
    } catch (const std::bad_alloc &) {
        sbwt_build_release(&S);
        rc = fail(SBWTGPU_ERR_OOM, "out of host memory");
    }
    info->pass_ms[2] = ms_since(t0);
    return rc;
}


}  // extern "C"
