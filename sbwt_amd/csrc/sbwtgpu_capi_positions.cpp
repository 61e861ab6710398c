// sbwtgpu_capi_positions.cpp -- the C ABI's position layer: the smallest reference coordinate of every column's k-mer, and
// reads placed on the references by diagonal voting (sbwt_positions.hip).  What it shares with the
// other files: sbwtgpu_internal.h.
#include "sbwtgpu_internal.h"
#include "sbwt_colors.h"
#include "sbwt_positions.h"

using namespace sbwt_capi;

// knobs of this file (sbwtgpu_set_tuning sets them)
int64_t sbwt_capi::g_pos_chunk_bases = 0;     // "positions_chunk_bases": 0 = the default of 64 Mi
int sbwt_capi::g_pos_map_table = 0;           // "positions_map_table": 0 = the compiled SBWT_PM_TABLE

static_assert(sizeof(sbwtgpu_read_map) == sizeof(SbwtReadMap), "the record of the ABI is the kernels' record");
static_assert(SBWTGPU_POSITIONS_MAP_TABLE == SBWT_PM_TABLE, "the header names the compiled table capacity");

// One device allocation: the counters (256 bytes) and first (n uint64).  The adds only ever lower it with atomics; the
// queries take `mu`, run on `stream` and bring their scratch with them.
struct sbwtgpu_positions {
    const sbwtgpu_index *idx = nullptr;
    int device = 0;
    int64_t n_nodes = 0, k = 0;
    DevBuf mem;
    size_t bytes = 0;
    SbwtPosCounters *d_ctr = nullptr;
    unsigned long long *d_first = nullptr;
    Stream stream;
    mutable std::mutex mu;
};

static int pos_check_index(const sbwtgpu_index *idx) {
    if (idx->h.n_nodes >= ((int64_t)1 << 31))
        return fail(SBWTGPU_ERR_INVALID_ARG, "positions: the index has %lld columns, the position layer reads int32 search results (fewer than 2^31 columns)",
                    (long long)idx->h.n_nodes);
    if (idx->h.rank_only) return fail(SBWTGPU_ERR_INVALID_ARG, "positions: %s", RANK_ONLY_MSG);
    return SBWTGPU_OK;
}
static int pos_check(const sbwtgpu_positions *p) {
    if (!p || !p->idx) return fail(SBWTGPU_ERR_INVALID_ARG, "positions: the object is NULL");
    if (p->idx->h.n_nodes != p->n_nodes || p->idx->h.k != p->k)
        return fail(SBWTGPU_ERR_INVALID_ARG, "positions of %lld columns at k = %lld used with an index of %lld columns at k = %lld",
                    (long long)p->n_nodes, (long long)p->k, (long long)p->idx->h.n_nodes, (long long)p->idx->h.k);
    return pos_check_index(p->idx);
}
static int pos_check_batch(int64_t n_reads, int strands) {
    if (strands != 1 && strands != 2)
        return fail(SBWTGPU_ERR_INVALID_ARG, "positions: strands must be 1 (forward) or 2 (either strand), not %d", strands);
    if (n_reads < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "positions: negative n_reads");
    if (n_reads >= ((int64_t)1 << 31)) return fail(SBWTGPU_ERR_INVALID_ARG, "positions: 2^31 reads or more in one call: split the batch");
    return SBWTGPU_OK;
}
static int64_t pos_chunk_bases() { return g_pos_chunk_bases > 0 ? g_pos_chunk_bases : (int64_t)64 << 20; }

// the object with its memory, `first` not yet written
static int pos_alloc(const sbwtgpu_index *idx, sbwtgpu_positions **out) {
    *out = nullptr;
    STG_TRY(pos_check_index(idx));
    DeviceGuard guard(idx->device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", idx->device);
    sbwtgpu_positions *p = new (std::nothrow) sbwtgpu_positions();
    if (!p) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    p->idx = idx;
    p->device = idx->device;
    p->n_nodes = idx->h.n_nodes;
    p->k = idx->h.k;
    p->bytes = 256 + align256((size_t)p->n_nodes * 8 + 8);
    hipError_t e = hipStreamCreateWithFlags(&p->stream.s, hipStreamNonBlocking);
    if (e == hipSuccess) e = p->mem.alloc(p->bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        delete p;
        return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "positions: %s", hipGetErrorString(e));
    }
    char *m = static_cast<char *>(p->mem.p);
    p->d_ctr = reinterpret_cast<SbwtPosCounters *>(m);
    p->d_first = reinterpret_cast<unsigned long long *>(m + 256);
    *out = p;
    return SBWTGPU_OK;
}
// counters 0, every entry of first "no position"; waits for it
static int pos_clear(sbwtgpu_positions *p) {
    HIP_TRY(hipMemsetAsync(p->mem.p, 0, 256, p->stream.s));
    HIP_TRY(hipMemsetAsync(p->d_first, 0xff, p->bytes - 256, p->stream.s));
    HIP_TRY(hipStreamSynchronize(p->stream.s));
    return SBWTGPU_OK;
}

// what sbwtgpu_occurrences_to_positions fills: an object with every entry "no position", and its table on the device
int sbwt_capi::positions_alloc_cleared(const sbwtgpu_index *idx, sbwtgpu_positions **out, unsigned long long **d_first) {
    STG_TRY(sbwtgpu_positions_create(idx, out));
    *d_first = (*out)->d_first;
    return SBWTGPU_OK;
}

extern "C" {

int sbwtgpu_positions_create(const sbwtgpu_index *idx, sbwtgpu_positions **out) {
    if (!idx || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "positions: NULL argument (idx and out are needed)");
    sbwtgpu_positions *p = nullptr;
    STG_TRY(pos_alloc(idx, &p));
    DeviceGuard guard(p->device);
    const int rc = pos_clear(p);
    if (rc != SBWTGPU_OK) {
        (void)hipGetLastError();
        delete p;
        *out = nullptr;
        return rc;
    }
    *out = p;
    return SBWTGPU_OK;
}

int sbwtgpu_positions_upload(const sbwtgpu_index *idx, const uint64_t *first, sbwtgpu_positions **out) {
    if (!idx || !first || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "positions: NULL argument (idx, first and out are needed)");
    sbwtgpu_positions *p = nullptr;
    STG_TRY(pos_alloc(idx, &p));
    DeviceGuard guard(p->device);
    SbwtPosCounters h;
    memset(&h, 0, sizeof(h));
    hipStream_t st = p->stream.s;
    hipError_t e = hipMemsetAsync(p->mem.p, 0, 256, st);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_first, 0xff, p->bytes - 256, st);
    if (e == hipSuccess && p->n_nodes > 0) e = hipMemcpyAsync(p->d_first, first, (size_t)p->n_nodes * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        sbwt_launch_pos_check(p->d_first, p->n_nodes, p->d_ctr, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h, p->d_ctr, sizeof(h), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess || h.bad) {
        (void)hipGetLastError();
        delete p;
        *out = nullptr;
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "positions: %s", hipGetErrorString(e));
        return fail(SBWTGPU_ERR_INVALID_ARG, "positions: an entry of first is neither UINT64_MAX nor a key with a sequence number below 2^30");
    }
    *out = p;
    return SBWTGPU_OK;
}

int sbwtgpu_positions_reset(sbwtgpu_positions *p) {
    STG_TRY(pos_check(p));
    DeviceGuard guard(p->device);
    std::lock_guard<std::mutex> lock(p->mu);
    // (adds of the caller's on other streams have to be over, as for the queries: the device is waited for first)
    HIP_TRY(hipDeviceSynchronize());
    return pos_clear(p);
}

void sbwtgpu_positions_destroy(sbwtgpu_positions *p) {
    if (!p) return;
    DeviceGuard guard(p->device);
    delete p;
}

// Host buffers: read_hits_batch's chunks of whole sequences under "positions_chunk_bases", two in flight on the parked slots
// of the search pipeline.  Bases and offsets go down; each chunk's status word and its hit windows come back.
int sbwtgpu_positions_add_batch(sbwtgpu_positions *p, int64_t first_seq, const char *bases, const int64_t *read_off, int64_t n_reads,
                                int strands, int64_t *n_windows, int64_t *n_hit_windows) {
    if (n_windows) *n_windows = 0;
    if (n_hit_windows) *n_hit_windows = 0;
    STG_TRY(pos_check(p));
    STG_TRY(pos_check_batch(n_reads, strands));
    if (first_seq < 0 || first_seq + n_reads > ((int64_t)1 << 30))
        return fail(SBWTGPU_ERR_INVALID_ARG, "positions: sequence numbers %lld .. %lld are out of range (0 .. 2^30 - 1)", (long long)first_seq,
                    (long long)(first_seq + n_reads - 1));
    if (n_reads == 0) return SBWTGPU_OK;
    if (!read_off) return fail(SBWTGPU_ERR_INVALID_ARG, "positions: NULL argument (read_off)");
    if (read_off[n_reads] > read_off[0] && !bases) return fail(SBWTGPU_ERR_INVALID_ARG, "positions: NULL argument (bases)");
    SbwtReadChunks ch;
    STG_TRY(cut_reads(read_off, n_reads, pos_chunk_bases(), (int64_t)1 << 24, p->k, ch));
    DeviceGuard guard(p->device);
    ReadPipe pipe(bases, read_off, ch);
    STG_TRY(pipe.open(p->device, sbwtgpu_pseudoalign_workspace_bytes(ch.max_bases, ch.max_reads, strands), ch.n_chunks() > 1 ? 2 : 1,
                      "position buffers"));
    int64_t hits = 0;
    const int rc = pipe.run(
        [&](const ReadPipe::Chunk &c) -> int {
            StrandSearch q;
            STG_TRY(search_strands_dev(p->idx, c.bases, c.nb, c.roff, c.nr, strands, c.ws, pipe.ws_bytes, c.P->st, q));
            SbwtPaHeader *hdr = static_cast<SbwtPaHeader *>(q.hdr);
            sbwt_launch_pos_add(q.res, q.res2, q.ooff, c.nr, c.nb, first_seq + c.lo, p->n_nodes, p->d_first, p->d_ctr, &hdr->n_hit, c.P->st);
            HIP_TRY(hipGetLastError());
            return pipe.fetch(c, c.ws + q.hdr_off, 16);    // (status, and SbwtPaHeader::n_hit behind it)
        },
        [&](const PipeSlot &P) {
            unsigned long long nh;
            memcpy(&nh, P.h_status + 2, 8);
            hits += (int64_t)nh;
        });
    if (rc != SBWTGPU_OK) return rc;
    if (n_windows) *n_windows = ch.windows;
    if (n_hit_windows) *n_hit_windows = hits;
    return SBWTGPU_OK;
}

int sbwtgpu_positions_info(const sbwtgpu_positions *p, int64_t *n_columns, int64_t *k, int64_t *n_windows, int64_t *n_hits,
                           int64_t *n_positioned, int64_t *device_bytes) {
    STG_TRY(pos_check(p));
    if (n_columns) *n_columns = p->n_nodes;
    if (k) *k = p->k;
    if (device_bytes) *device_bytes = (int64_t)p->bytes;
    if (!n_windows && !n_hits && !n_positioned) return SBWTGPU_OK;
    DeviceGuard guard(p->device);
    std::lock_guard<std::mutex> lock(p->mu);
    hipStream_t st = p->stream.s;
    SbwtPosCounters h;
    unsigned long long positioned = 0;
    DevBuf d;
    if (n_positioned) {
        HIP_TRY(d.alloc(8));
        sbwt_launch_pos_count(p->d_first, p->n_nodes, static_cast<unsigned long long *>(d.p), st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&positioned, d.p, 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(&h, p->d_ctr, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n_windows) *n_windows = (int64_t)h.n_windows;
    if (n_hits) *n_hits = (int64_t)h.n_hits;
    if (n_positioned) *n_positioned = (int64_t)positioned;
    return SBWTGPU_OK;
}

int sbwtgpu_positions_first_copy(const sbwtgpu_positions *p, uint64_t *first) {
    STG_TRY(pos_check(p));
    if (!first) return fail(SBWTGPU_ERR_INVALID_ARG, "positions: NULL argument (first)");
    DeviceGuard guard(p->device);
    std::lock_guard<std::mutex> lock(p->mu);
    HIP_TRY(hipMemcpyAsync(first, p->d_first, (size_t)p->n_nodes * 8, hipMemcpyDeviceToHost, p->stream.s));
    HIP_TRY(hipStreamSynchronize(p->stream.s));
    return SBWTGPU_OK;
}

int sbwtgpu_positions_first_dev(const sbwtgpu_positions *p, const uint64_t **d_first) {
    if (!p || !d_first) return fail(SBWTGPU_ERR_INVALID_ARG, "positions: NULL argument");
    *d_first = reinterpret_cast<const uint64_t *>(p->d_first);
    return SBWTGPU_OK;
}

// [the pseudoalignment layout, which begins with the search workspace][SbwtPosMapHeader][the list: 4 bytes per read]
int64_t sbwtgpu_positions_map_workspace_bytes(int64_t total_bases, int64_t n_reads, int strands) {
    if (n_reads < 0) n_reads = 0;
    return align256(sbwtgpu_pseudoalign_workspace_bytes(total_bases, n_reads, strands)) + (int64_t)sizeof(SbwtPosMapHeader) +
           align256(n_reads * 4);
}

int sbwtgpu_positions_map_dev(const sbwtgpu_positions *p, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                              int64_t n_reads, int strands, sbwtgpu_read_map *d_out, void *d_ws, int64_t ws_bytes, void *stream) {
    STG_TRY(pos_check(p));
    STG_TRY(pos_check_batch(n_reads, strands));
    // (the lengths live on the device: what can be told here is that no read of fewer than 2^30 bases makes this batch)
    if (n_reads == 1 && total_bases >= ((int64_t)1 << 30)) return fail(SBWTGPU_ERR_READ_TOO_LONG, "read 0 has >= 2^30 bases");
    STG_TRY(check_batch_dev(n_reads, total_bases, d_ws, ws_bytes, sbwtgpu_positions_map_workspace_bytes(total_bases, n_reads, strands)));
    if (n_reads == 0) return SBWTGPU_OK;
    if (!d_out) return fail(SBWTGPU_ERR_INVALID_ARG, "positions: NULL device pointer (d_out)");
    const int64_t pa_bytes = sbwtgpu_pseudoalign_workspace_bytes(total_bases, n_reads, strands);
    StrandSearch q;
    STG_TRY(search_strands_dev(p->idx, d_bases, total_bases, d_read_off, n_reads, strands, d_ws, pa_bytes, stream, q));
    if (!q.enqueued) return SBWTGPU_OK;
    DeviceGuard guard(p->device);
    char *w = static_cast<char *>(d_ws) + align256(pa_bytes);
    sbwt_launch_pos_map(q.res, q.res2, q.ooff, n_reads, p->d_first, p->n_nodes, g_pos_map_table, reinterpret_cast<SbwtReadMap *>(d_out),
                        reinterpret_cast<SbwtPosMapHeader *>(w), reinterpret_cast<unsigned *>(w + sizeof(SbwtPosMapHeader)),
                        static_cast<hipStream_t>(stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return SBWTGPU_OK;
}

// Host buffers: chunks of whole reads under "positions_chunk_bases", two in flight.  Bases and offsets go down; the records
// and each chunk's status word come back.
int sbwtgpu_positions_map_batch(const sbwtgpu_positions *p, const char *bases, const int64_t *read_off, int64_t n_reads, int strands,
                                sbwtgpu_read_map *out) {
    STG_TRY(pos_check(p));
    STG_TRY(pos_check_batch(n_reads, strands));
    if (n_reads == 0) return SBWTGPU_OK;
    if (!read_off || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "positions: NULL argument (read_off and out are needed)");
    if (read_off[n_reads] > read_off[0] && !bases) return fail(SBWTGPU_ERR_INVALID_ARG, "positions: NULL argument (bases)");
    for (int64_t r = 0; r < n_reads; r++) {
        STG_TRY(check_read_length(read_off, r));
        if (read_off[r + 1] - read_off[r] >= ((int64_t)1 << 30))
            return fail(SBWTGPU_ERR_READ_TOO_LONG, "read %lld has >= 2^30 bases: its votes over two strands would not fit an int32", (long long)r);
    }
    SbwtReadChunks ch;
    STG_TRY(cut_reads(read_off, n_reads, pos_chunk_bases(), (int64_t)1 << 24, p->k, ch));
    DeviceGuard guard(p->device);
    ReadPipe pipe(bases, read_off, ch);
    const int r_rec = pipe.region(ch.max_reads * (int64_t)sizeof(sbwtgpu_read_map), true, out, sizeof(sbwtgpu_read_map));
    STG_TRY(pipe.open(p->device, sbwtgpu_positions_map_workspace_bytes(ch.max_bases, ch.max_reads, strands), ch.n_chunks() > 1 ? 2 : 1,
                      "position buffers"));
    return pipe.run([&](const ReadPipe::Chunk &c) -> int {
        STG_TRY(sbwtgpu_positions_map_dev(p, c.bases, c.nb, c.roff, c.nr, strands, pipe.at<sbwtgpu_read_map>(c, r_rec), c.ws, pipe.ws_bytes,
                                          c.P->st));
        const SbwtPaLayout L = sbwt_pa_layout(sbwtgpu_search_workspace_bytes(c.nb), c.nb, c.nr, strands);
        return pipe.fetch(c, c.ws + L.hdr, 4);
    });
}

}  // extern "C"
