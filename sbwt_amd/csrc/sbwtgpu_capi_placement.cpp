// sbwtgpu_capi_placement.cpp -- the C ABI's two placement layers.  Positions: the smallest reference coordinate of every
// column's k-mer, and reads placed on the references by diagonal voting (sbwt_positions.hip).
// Occurrences: every reference coordinate of every column's k-mer as CSR arrays, built from a log of hits, and reads placed by
// voting over all of them (sbwt_occurrences.hip).  The checks, the chunked adds and the map calls are
// written once, with the layer's words and its launch as parameters.  What it shares with the other files: sbwtgpu_internal.h.
#include "sbwtgpu_internal.h"
#include "sbwt_colors.h"
#include "sbwt_occurrences.h"
#include "sbwt_positions.h"

using namespace sbwt_capi;

// knobs of this file (sbwtgpu_set_tuning sets them)
int64_t sbwt_capi::g_pos_chunk_bases = 0;     // "positions_chunk_bases": 0 = the default of 64 Mi
int sbwt_capi::g_pos_map_table = 0;           // "positions_map_table": 0 = the compiled SBWT_PM_TABLE
int64_t sbwt_capi::g_occ_chunk_bases = 0;     // "occurrences_chunk_bases": 0 = the default of 64 Mi
int sbwt_capi::g_occ_map_table = 0;           // "occurrences_map_table": 0 = the compiled SBWT_OM_TABLE

static_assert(sizeof(sbwtgpu_read_map) == sizeof(SbwtReadMap), "the record of the ABI is the kernels' record");
static_assert(SBWTGPU_POSITIONS_MAP_TABLE == SBWT_PM_TABLE, "the header names the compiled table capacity");
static_assert(SBWTGPU_OCCURRENCES_MAP_TABLE == SBWT_OM_TABLE, "the header names the compiled table capacity");
static_assert(SBWTGPU_OCCURRENCES_MAP_TABLE >= 256, "the table holds at least 256 placements");

// the words in which the two layers' error texts differ, and the layer's chunk knob
struct Layer {
    const char *name, *who, *one, *buffers, *votes;
    const int64_t *chunk_knob;
    int64_t chunk_bases() const { return *chunk_knob > 0 ? *chunk_knob : (int64_t)64 << 20; }
};
static const Layer POS = {"positions", "positions: ", "position", "position buffers", "votes", &g_pos_chunk_bases};
static const Layer OCC = {"occurrences", "occurrences: ", "occurrence", "occurrence buffers", "hits", &g_occ_chunk_bases};

// What the three handles share: the index the object is bound to and what it said of itself then, a stream for the object's
// own work and a mutex (positions and occurrences: their queries take it; the builder: an add holds it for its whole length).
struct Placed {
    const sbwtgpu_index *idx = nullptr;
    int device = 0;
    int64_t n_nodes = 0, k = 0;
    Stream stream;
    mutable std::mutex mu;
    hipError_t bind(const sbwtgpu_index *i) {
        idx = i;
        device = i->device;
        n_nodes = i->h.n_nodes;
        k = i->h.k;
        return hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking);
    }
};

// One device allocation: the counters (256 bytes) and first (n uint64).  The adds only ever lower it with atomics; the
// queries take `mu`, run on `stream` and bring their scratch with them.
struct sbwtgpu_positions : Placed {
    DevBuf mem;
    size_t bytes = 0;
    SbwtPosCounters *d_ctr = nullptr;
    unsigned long long *d_first = nullptr;
};

// The finished object never changes: two device allocations (counters + off, and occ) and its scalars on the host.
struct sbwtgpu_occurrences : Placed {
    DevBuf off_mem, occ_mem;
    SbwtOccCounters *d_ctr = nullptr;
    unsigned long long *d_off = nullptr, *d_occ = nullptr;
    int64_t n_occ = 0, n_windows = 0, n_hits = 0, n_positioned = 0, max_count = 0;
    size_t bytes = 0;
};

// The builder: counters and a log of (column, key) pairs that grows by doubling.
struct sbwtgpu_occurrences_builder : Placed {
    DevBuf ctr_mem;
    SbwtOccCounters *d_ctr = nullptr;
    unsigned *d_col = nullptr;
    unsigned long long *d_key = nullptr;
    int64_t cap = 0;            // entries the log has room for
    int64_t reserved = 0;       // an upper bound of the log's length once every launched add has run
    int64_t max_seq = 0;        // the largest sequence number added (the sort's key bits)
    ~sbwtgpu_occurrences_builder() {
        if (d_col) (void)hipFree(d_col);
        if (d_key) (void)hipFree(d_key);
    }
};

// ---- checks ------------------------------------------------------------------------------------------------------
static int check_index(const Layer &L, const sbwtgpu_index *idx) {
    if (idx->h.n_nodes >= ((int64_t)1 << 31))
        return fail(SBWTGPU_ERR_INVALID_ARG, "%sthe index has %lld columns, the %s layer reads int32 search results (fewer than 2^31 columns)",
                    L.who, (long long)idx->h.n_nodes, L.one);
    if (idx->h.rank_only) return fail(SBWTGPU_ERR_INVALID_ARG, "%s%s", L.who, RANK_ONLY_MSG);
    return SBWTGPU_OK;
}
// the object, and that the index it was made for still is what it was
static int check_obj(const Layer &L, const Placed *o) {
    if (!o || !o->idx) return fail(SBWTGPU_ERR_INVALID_ARG, "%sthe object is NULL", L.who);
    if (o->idx->h.n_nodes != o->n_nodes || o->idx->h.k != o->k)
        return fail(SBWTGPU_ERR_INVALID_ARG, "%s of %lld columns at k = %lld used with an index of %lld columns at k = %lld", L.name,
                    (long long)o->n_nodes, (long long)o->k, (long long)o->idx->h.n_nodes, (long long)o->idx->h.k);
    return check_index(L, o->idx);
}
static int check_max_occ(int max_occ) {
    if (max_occ < 1 || max_occ > SBWTGPU_OCCURRENCES_MAX_OCC)
        return fail(SBWTGPU_ERR_INVALID_ARG, "occurrences: max_occ must be in 1 .. %d, not %d", SBWTGPU_OCCURRENCES_MAX_OCC, max_occ);
    return SBWTGPU_OK;
}
// a failed HIP call as the layer's error ("layer: what: text", or "layer: text")
static int hip_fail(const Layer &L, hipError_t e, const char *what = nullptr) {
    (void)hipGetLastError();
    const int code = e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP;
    return what ? fail(code, "%s%s: %s", L.who, what, hipGetErrorString(e)) : fail(code, "%s%s", L.who, hipGetErrorString(e));
}
static int bits_of(uint64_t x) {            // the bits that hold every value below x
    int b = 1;
    while (b < 64 && (x - 1) >> b) b++;
    return b;
}

// ---- the calls both layers have ------------------------------------------------------------------------------------
// An add over host buffers: read_hits_batch's chunks of whole sequences under the layer's chunk knob, two in flight on the
// parked slots of the search pipeline.  Bases and offsets go down; each chunk's status word and its hit windows come back.
// lock (may be NULL) is taken once the batch has passed its checks and is left held.  Per chunk: reserve(c), the searches,
// launch(c, q, d_n_hit_windows).
template <typename Reserve, typename Launch>
static int add_batch(const Layer &L, const Placed *o, std::unique_lock<std::mutex> *lock, int64_t first_seq, const char *bases,
                     const int64_t *read_off, int64_t n_reads, int strands, int64_t *n_windows, int64_t *n_hit_windows, Reserve reserve,
                     Launch launch) {
    if (n_windows) *n_windows = 0;
    if (n_hit_windows) *n_hit_windows = 0;
    STG_TRY(check_obj(L, o));
    STG_TRY(check_strands_batch(L.who, n_reads, strands));
    if (first_seq < 0 || first_seq + n_reads > ((int64_t)1 << 30))
        return fail(SBWTGPU_ERR_INVALID_ARG, "%ssequence numbers %lld .. %lld are out of range (0 .. 2^30 - 1)", L.who, (long long)first_seq,
                    (long long)(first_seq + n_reads - 1));
    if (n_reads == 0) return SBWTGPU_OK;
    if (!read_off) return fail(SBWTGPU_ERR_INVALID_ARG, "%sNULL argument (read_off)", L.who);
    if (read_off[n_reads] > read_off[0] && !bases) return fail(SBWTGPU_ERR_INVALID_ARG, "%sNULL argument (bases)", L.who);
    SbwtReadChunks ch;
    STG_TRY(cut_reads(read_off, n_reads, L.chunk_bases(), (int64_t)1 << 24, o->k, ch));
    DeviceGuard guard(o->device);
    if (lock) lock->lock();
    ReadPipe pipe(bases, read_off, ch);
    STG_TRY(pipe.open(o->device, sbwtgpu_pseudoalign_workspace_bytes(ch.max_bases, ch.max_reads, strands), ch.n_chunks() > 1 ? 2 : 1, L.buffers));
    int64_t hits = 0;
    const int rc = pipe.run(
        [&](const ReadPipe::Chunk &c) -> int {
            STG_TRY(reserve(c));
            StrandSearch q;
            STG_TRY(search_strands_dev(o->idx, c.bases, c.nb, c.roff, c.nr, strands, c.ws, pipe.ws_bytes, c.P->st, q));
            launch(c, q, &static_cast<SbwtPaHeader *>(q.hdr)->n_hit);
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

// [the pseudoalignment layout, which begins with the search workspace][SbwtPosMapHeader][the list: 4 bytes per read]
static int64_t map_workspace_bytes(int64_t total_bases, int64_t n_reads, int strands) {
    if (n_reads < 0) n_reads = 0;
    return align256(sbwtgpu_pseudoalign_workspace_bytes(total_bases, n_reads, strands)) + (int64_t)sizeof(SbwtPosMapHeader) +
           align256(n_reads * 4);
}

// A map over device buffers: the searches, then launch(q, d_out, hdr, d_slow, stream) on the call's own part of the workspace
template <typename Launch>
static int map_dev(const Layer &L, const Placed *o, const char *d_bases, int64_t total_bases, const int64_t *d_read_off, int64_t n_reads,
                   int strands, sbwtgpu_read_map *d_out, void *d_ws, int64_t ws_bytes, void *stream, Launch launch) {
    STG_TRY(check_obj(L, o));
    STG_TRY(check_strands_batch(L.who, n_reads, strands));
    // (the lengths live on the device: what can be told here is that no read of fewer than 2^30 bases makes this batch)
    if (n_reads == 1 && total_bases >= ((int64_t)1 << 30)) return fail(SBWTGPU_ERR_READ_TOO_LONG, "read 0 has >= 2^30 bases");
    STG_TRY(check_batch_dev(n_reads, total_bases, d_ws, ws_bytes, map_workspace_bytes(total_bases, n_reads, strands)));
    if (n_reads == 0) return SBWTGPU_OK;
    if (!d_out) return fail(SBWTGPU_ERR_INVALID_ARG, "%sNULL device pointer (d_out)", L.who);
    const int64_t pa_bytes = sbwtgpu_pseudoalign_workspace_bytes(total_bases, n_reads, strands);
    StrandSearch q;
    STG_TRY(search_strands_dev(o->idx, d_bases, total_bases, d_read_off, n_reads, strands, d_ws, pa_bytes, stream, q));
    if (!q.enqueued) return SBWTGPU_OK;
    DeviceGuard guard(o->device);
    char *w = static_cast<char *>(d_ws) + align256(pa_bytes);
    launch(q, reinterpret_cast<SbwtReadMap *>(d_out), reinterpret_cast<SbwtPosMapHeader *>(w),
           reinterpret_cast<unsigned *>(w + sizeof(SbwtPosMapHeader)), static_cast<hipStream_t>(stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return SBWTGPU_OK;
}

// A map over host buffers: chunks of whole reads under the layer's chunk knob, two in flight.  Bases and offsets go down; the
// records and each chunk's status word come back.  dev: the layer's exported map_dev for one chunk.
template <typename Dev>
static int map_batch(const Layer &L, const Placed *o, const char *bases, const int64_t *read_off, int64_t n_reads, int strands,
                     sbwtgpu_read_map *out, Dev dev) {
    STG_TRY(check_obj(L, o));
    STG_TRY(check_strands_batch(L.who, n_reads, strands));
    if (n_reads == 0) return SBWTGPU_OK;
    if (!read_off || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "%sNULL argument (read_off and out are needed)", L.who);
    if (read_off[n_reads] > read_off[0] && !bases) return fail(SBWTGPU_ERR_INVALID_ARG, "%sNULL argument (bases)", L.who);
    for (int64_t r = 0; r < n_reads; r++) {
        STG_TRY(check_read_length(read_off, r));
        if (read_off[r + 1] - read_off[r] >= ((int64_t)1 << 30))
            return fail(SBWTGPU_ERR_READ_TOO_LONG, "read %lld has >= 2^30 bases: its %s over two strands would not fit an int32", (long long)r,
                        L.votes);
    }
    SbwtReadChunks ch;
    STG_TRY(cut_reads(read_off, n_reads, L.chunk_bases(), (int64_t)1 << 24, o->k, ch));
    DeviceGuard guard(o->device);
    ReadPipe pipe(bases, read_off, ch);
    const int r_rec = pipe.region(ch.max_reads * (int64_t)sizeof(sbwtgpu_read_map), true, out, sizeof(sbwtgpu_read_map));
    STG_TRY(pipe.open(o->device, map_workspace_bytes(ch.max_bases, ch.max_reads, strands), ch.n_chunks() > 1 ? 2 : 1, L.buffers));
    return pipe.run([&](const ReadPipe::Chunk &c) -> int {
        STG_TRY(dev(c.bases, c.nb, c.roff, c.nr, pipe.at<sbwtgpu_read_map>(c, r_rec), c.ws, pipe.ws_bytes, c.P->st));
        const SbwtPaLayout lay = sbwt_pa_layout(sbwtgpu_search_workspace_bytes(c.nb), c.nb, c.nr, strands);
        return pipe.fetch(c, c.ws + lay.hdr, 4);
    });
}

// ---- positions: the object ---------------------------------------------------------------------------------------------
// the object with its memory, `first` not yet written
static int pos_alloc(const sbwtgpu_index *idx, sbwtgpu_positions **out) {
    *out = nullptr;
    STG_TRY(check_index(POS, idx));
    DeviceGuard guard(idx->device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", idx->device);
    sbwtgpu_positions *p = new (std::nothrow) sbwtgpu_positions();
    if (!p) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    hipError_t e = p->bind(idx);
    p->bytes = 256 + align256((size_t)p->n_nodes * 8 + 8);
    if (e == hipSuccess) e = p->mem.alloc(p->bytes);
    if (e != hipSuccess) {
        delete p;
        return hip_fail(POS, e);
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

// ---- occurrences: the object and the builder's log ---------------------------------------------------------------------
// the object with its counters and off (n + 1 words), nothing written yet, no occ
static int occ_alloc(const sbwtgpu_index *idx, sbwtgpu_occurrences **out) {
    *out = nullptr;
    sbwtgpu_occurrences *o = new (std::nothrow) sbwtgpu_occurrences();
    if (!o) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    hipError_t e = o->bind(idx);
    const size_t off_bytes = 256 + align256((size_t)(o->n_nodes + 1) * 8);
    if (e == hipSuccess) e = o->off_mem.alloc(off_bytes);
    if (e != hipSuccess) {
        delete o;
        return hip_fail(OCC, e, "allocation");
    }
    o->bytes = off_bytes;
    o->d_ctr = reinterpret_cast<SbwtOccCounters *>(o->off_mem.p);
    o->d_off = reinterpret_cast<unsigned long long *>(static_cast<char *>(o->off_mem.p) + 256);
    *out = o;
    return SBWTGPU_OK;
}
static hipError_t occ_alloc_keys(sbwtgpu_occurrences *o, int64_t n_occ) {
    const size_t b = align256((size_t)n_occ * 8 + 8);
    const hipError_t e = o->occ_mem.alloc(b);
    if (e != hipSuccess) return e;
    o->d_occ = static_cast<unsigned long long *>(o->occ_mem.p);
    o->n_occ = n_occ;
    o->bytes += b;
    return hipSuccess;
}

// room in the log for `need` more entries (under b->mu).  Growing waits for the device, so that no add still appends.
static int occ_reserve(sbwtgpu_occurrences_builder *b, int64_t need) {
    if (b->reserved + need <= b->cap) {
        b->reserved += need;
        return SBWTGPU_OK;
    }
    HIP_TRY(hipDeviceSynchronize());
    SbwtOccCounters h;
    HIP_TRY(hipMemcpy(&h, b->d_ctr, sizeof(h), hipMemcpyDeviceToHost));
    const int64_t used = (int64_t)h.log_len;
    if (used > b->cap) return fail(SBWTGPU_ERR_HIP, "occurrences: internal: the log holds %lld entries of %lld", (long long)used, (long long)b->cap);
    b->reserved = used;
    if (used + need > b->cap) {
        int64_t cap = std::max<int64_t>(2 * b->cap, (int64_t)1 << 16);
        while (cap < used + need) cap *= 2;
        unsigned *col = nullptr;
        unsigned long long *key = nullptr;
        hipError_t e = hipMalloc((void **)&col, (size_t)cap * 4);
        if (e == hipSuccess) e = hipMalloc((void **)&key, (size_t)cap * 8);
        if (e == hipSuccess && used > 0) e = hipMemcpy(col, b->d_col, (size_t)used * 4, hipMemcpyDeviceToDevice);
        if (e == hipSuccess && used > 0) e = hipMemcpy(key, b->d_key, (size_t)used * 8, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) {
            if (col) (void)hipFree(col);
            if (key) (void)hipFree(key);
            return hip_fail(OCC, e, "growing the log");
        }
        if (b->d_col) (void)hipFree(b->d_col);
        if (b->d_key) (void)hipFree(b->d_key);
        b->d_col = col;
        b->d_key = key;
        b->cap = cap;
    }
    b->reserved += need;
    return SBWTGPU_OK;
}

extern "C" {

// ---- positions -------------------------------------------------------------------------------------------------------
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
        delete p;
        *out = nullptr;
        if (e != hipSuccess) return hip_fail(POS, e);
        return fail(SBWTGPU_ERR_INVALID_ARG, "positions: an entry of first is neither UINT64_MAX nor a key with a sequence number below 2^30");
    }
    *out = p;
    return SBWTGPU_OK;
}

int sbwtgpu_positions_reset(sbwtgpu_positions *p) {
    STG_TRY(check_obj(POS, p));
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

int sbwtgpu_positions_add_batch(sbwtgpu_positions *p, int64_t first_seq, const char *bases, const int64_t *read_off, int64_t n_reads,
                                int strands, int64_t *n_windows, int64_t *n_hit_windows) {
    return add_batch(
        POS, p, nullptr, first_seq, bases, read_off, n_reads, strands, n_windows, n_hit_windows,
        [](const ReadPipe::Chunk &) { return SBWTGPU_OK; },
        [&](const ReadPipe::Chunk &c, const StrandSearch &q, unsigned long long *d_n_hit) {
            sbwt_launch_pos_add(q.res, q.res2, q.ooff, c.nr, c.nb, first_seq + c.lo, p->n_nodes, p->d_first, p->d_ctr, d_n_hit, c.P->st);
        });
}

int sbwtgpu_positions_info(const sbwtgpu_positions *p, int64_t *n_columns, int64_t *k, int64_t *n_windows, int64_t *n_hits,
                           int64_t *n_positioned, int64_t *device_bytes) {
    STG_TRY(check_obj(POS, p));
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
    STG_TRY(check_obj(POS, p));
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

int64_t sbwtgpu_positions_map_workspace_bytes(int64_t total_bases, int64_t n_reads, int strands) {
    return map_workspace_bytes(total_bases, n_reads, strands);
}

int sbwtgpu_positions_map_dev(const sbwtgpu_positions *p, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                              int64_t n_reads, int strands, sbwtgpu_read_map *d_out, void *d_ws, int64_t ws_bytes, void *stream) {
    return map_dev(POS, p, d_bases, total_bases, d_read_off, n_reads, strands, d_out, d_ws, ws_bytes, stream,
                   [&](const StrandSearch &q, SbwtReadMap *out, SbwtPosMapHeader *hdr, unsigned *d_slow, hipStream_t st) {
                       sbwt_launch_pos_map(q.res, q.res2, q.ooff, n_reads, p->d_first, p->n_nodes, g_pos_map_table, out, hdr, d_slow, st);
                   });
}

int sbwtgpu_positions_map_batch(const sbwtgpu_positions *p, const char *bases, const int64_t *read_off, int64_t n_reads, int strands,
                                sbwtgpu_read_map *out) {
    return map_batch(POS, p, bases, read_off, n_reads, strands, out,
                     [&](const char *d_bases, int64_t nb, const int64_t *d_roff, int64_t nr, sbwtgpu_read_map *d_out, void *ws, int64_t ws_bytes,
                         void *st) { return sbwtgpu_positions_map_dev(p, d_bases, nb, d_roff, nr, strands, d_out, ws, ws_bytes, st); });
}

// ---- occurrences -------------------------------------------------------------------------------------------------------
int sbwtgpu_occurrences_builder_create(const sbwtgpu_index *idx, sbwtgpu_occurrences_builder **out) {
    if (!idx || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "occurrences: NULL argument (idx and out are needed)");
    *out = nullptr;
    STG_TRY(check_index(OCC, idx));
    DeviceGuard guard(idx->device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", idx->device);
    sbwtgpu_occurrences_builder *b = new (std::nothrow) sbwtgpu_occurrences_builder();
    if (!b) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    hipError_t e = b->bind(idx);
    if (e == hipSuccess) e = b->ctr_mem.alloc(256);
    if (e == hipSuccess) e = hipMemset(b->ctr_mem.p, 0, 256);
    if (e != hipSuccess) {
        delete b;
        return hip_fail(OCC, e, "allocation");
    }
    b->d_ctr = static_cast<SbwtOccCounters *>(b->ctr_mem.p);
    *out = b;
    return SBWTGPU_OK;
}

void sbwtgpu_occurrences_builder_destroy(sbwtgpu_occurrences_builder *b) {
    if (!b) return;
    DeviceGuard guard(b->device);
    delete b;
}

// The whole add holds the builder's mutex: the log may move when it grows.
int sbwtgpu_occurrences_builder_add_batch(sbwtgpu_occurrences_builder *b, int64_t first_seq, const char *bases, const int64_t *read_off,
                                          int64_t n_reads, int strands, int64_t *n_windows, int64_t *n_hit_windows) {
    std::unique_lock<std::mutex> lock;
    if (b) lock = std::unique_lock<std::mutex>(b->mu, std::defer_lock);
    const int rc = add_batch(
        OCC, b, &lock, first_seq, bases, read_off, n_reads, strands, n_windows, n_hit_windows,
        [&](const ReadPipe::Chunk &c) {
            int64_t w = 0;                                 // the chunk's windows: what its searches can append, per strand
            for (int64_t r = c.lo; r < c.lo + c.nr; r++) w += std::max<int64_t>(read_off[r + 1] - read_off[r] - b->k + 1, 0);
            return occ_reserve(b, w * strands);
        },
        [&](const ReadPipe::Chunk &c, const StrandSearch &q, unsigned long long *d_n_hit) {
            sbwt_launch_occ_add(q.res, q.res2, q.ooff, c.nr, c.nb, first_seq + c.lo, b->n_nodes, b->d_col, b->d_key,
                                (unsigned long long)b->cap, b->d_ctr, d_n_hit, c.P->st);
        });
    if (rc == SBWTGPU_OK && n_reads > 0) b->max_seq = std::max(b->max_seq, first_seq + n_reads - 1);    // (still under the mutex)
    return rc;
}

// sort, flag, scan, select.  The builder is deleted on success only.
int sbwtgpu_occurrences_builder_finish(sbwtgpu_occurrences_builder *b, sbwtgpu_occurrences **out) {
    if (!out) return fail(SBWTGPU_ERR_INVALID_ARG, "occurrences: NULL argument (out)");
    *out = nullptr;
    STG_TRY(check_obj(OCC, b));
    DeviceGuard guard(b->device);
    sbwtgpu_occurrences *o = nullptr;
    {
        std::lock_guard<std::mutex> lock(b->mu);
        hipStream_t st = b->stream.s;
        HIP_TRY(hipDeviceSynchronize());                   // (every add has returned; their streams are idle)
        SbwtOccCounters h;
        HIP_TRY(hipMemcpy(&h, b->d_ctr, sizeof(h), hipMemcpyDeviceToHost));
        const int64_t n_log = (int64_t)h.log_len;
        if (h.bad_kind || n_log > b->cap) return fail(SBWTGPU_ERR_HIP, "occurrences: internal: the log overflowed (%lld of %lld)", (long long)n_log, (long long)b->cap);
        STG_TRY(occ_alloc(b->idx, &o));
        hipError_t e = hipSuccess;
        DevBuf alt_col, alt_key, tmp, flag;
        if (n_log > 0) {
            const size_t tmp_bytes = std::max(sbwt_occ_sort_tmp_bytes(n_log), sbwt_occ_select_tmp_bytes(n_log));
            e = alt_col.alloc((size_t)n_log * 4);
            if (e == hipSuccess) e = alt_key.alloc((size_t)n_log * 8);
            if (e == hipSuccess) e = tmp.alloc(tmp_bytes);
            if (e == hipSuccess)
                e = sbwt_occ_sort(b->d_col, b->d_key, static_cast<unsigned *>(alt_col.p), static_cast<unsigned long long *>(alt_key.p), n_log,
                                  32 + bits_of((uint64_t)b->max_seq + 1), bits_of((uint64_t)std::max<int64_t>(b->n_nodes, 1)), tmp.p, tmp_bytes, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (alt_col.p) { (void)hipFree(alt_col.p); alt_col.p = nullptr; }
            if (alt_key.p) { (void)hipFree(alt_key.p); alt_key.p = nullptr; }
            if (e == hipSuccess) e = flag.alloc((size_t)n_log);
            if (e == hipSuccess) {
                sbwt_launch_occ_flag(b->d_col, b->d_key, n_log, static_cast<unsigned char *>(flag.p), o->d_off, o->n_nodes, b->d_ctr, st);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipMemcpyAsync(&h, b->d_ctr, sizeof(h), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e == hipSuccess) e = occ_alloc_keys(o, (int64_t)h.n_unique);
            if (e == hipSuccess)
                e = sbwt_occ_select(b->d_key, static_cast<unsigned char *>(flag.p), n_log, o->d_occ, &b->d_ctr->n_unique, tmp.p, tmp_bytes, st);
        } else {
            e = hipMemsetAsync(o->d_off, 0, (size_t)(o->n_nodes + 1) * 8, st);
            if (e == hipSuccess) e = occ_alloc_keys(o, 0);
        }
        DevBuf scan_tmp;
        const size_t scan_bytes = sbwt_occ_scan_tmp_bytes(o->n_nodes);
        if (e == hipSuccess) e = scan_tmp.alloc(scan_bytes);
        if (e == hipSuccess) e = sbwt_occ_scan(o->d_off, o->n_nodes, scan_tmp.p, scan_bytes, st);
        if (e == hipSuccess) e = hipMemsetAsync(o->d_ctr, 0, 256, st);
        if (e == hipSuccess) {
            sbwt_launch_occ_stats(o->d_off, o->n_nodes, o->d_ctr, st);
            e = hipGetLastError();
        }
        SbwtOccCounters s;
        if (e == hipSuccess) e = hipMemcpyAsync(&s, o->d_ctr, sizeof(s), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            delete o;
            return hip_fail(OCC, e, "finish");
        }
        o->n_windows = (int64_t)h.n_windows;
        o->n_hits = (int64_t)h.n_hits;
        o->n_positioned = (int64_t)s.n_positioned;
        o->max_count = (int64_t)s.max_count;
    }
    delete b;                                              // (the log goes with it)
    *out = o;
    return SBWTGPU_OK;
}

int sbwtgpu_occurrences_upload(const sbwtgpu_index *idx, const uint64_t *off, const uint64_t *occ, int64_t n_occ, sbwtgpu_occurrences **out) {
    if (!idx || !off || !out || (n_occ > 0 && !occ))
        return fail(SBWTGPU_ERR_INVALID_ARG, "occurrences: NULL argument (idx, off, occ and out are needed)");
    *out = nullptr;
    if (n_occ < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "occurrences: negative n_occ");
    STG_TRY(check_index(OCC, idx));
    DeviceGuard guard(idx->device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", idx->device);
    sbwtgpu_occurrences *o = nullptr;
    STG_TRY(occ_alloc(idx, &o));
    hipStream_t st = o->stream.s;
    SbwtOccCounters h;
    memset(&h, 0, sizeof(h));
    h.bad_column = ~0ull;
    hipError_t e = occ_alloc_keys(o, n_occ);
    if (e == hipSuccess) e = hipMemcpyAsync(o->d_ctr, &h, sizeof(h), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(o->d_off, off, (size_t)(o->n_nodes + 1) * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && n_occ > 0) e = hipMemcpyAsync(o->d_occ, occ, (size_t)n_occ * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        sbwt_launch_occ_check_off(o->d_off, o->n_nodes, (unsigned long long)n_occ, o->d_ctr, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h, o->d_ctr, sizeof(h), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && h.bad_column == ~0ull) {        // the offsets are sound: the keys can be read through them
        sbwt_launch_occ_check_keys(o->d_off, o->d_occ, o->n_nodes, o->d_ctr, st);
        e = hipGetLastError();
        if (e == hipSuccess) sbwt_launch_occ_stats(o->d_off, o->n_nodes, o->d_ctr, st);
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&h, o->d_ctr, sizeof(h), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess || h.bad_column != ~0ull) {
        delete o;
        if (e != hipSuccess) return hip_fail(OCC, e, "upload");
        static const char *const what[] = {"", "off[0] is not 0", "off decreases behind it", "off[n] is not n_occ",
                                           "its keys are not strictly ascending", "a key's sequence number is 2^30 or more"};
        return fail(SBWTGPU_ERR_INVALID_ARG, "occurrences: column %lld: %s", (long long)h.bad_column, what[h.bad_kind <= 5 ? h.bad_kind : 0]);
    }
    o->n_positioned = (int64_t)h.n_positioned;
    o->max_count = (int64_t)h.max_count;
    *out = o;
    return SBWTGPU_OK;
}

void sbwtgpu_occurrences_destroy(sbwtgpu_occurrences *o) {
    if (!o) return;
    DeviceGuard guard(o->device);
    delete o;
}

int sbwtgpu_occurrences_info(const sbwtgpu_occurrences *o, int64_t *n_columns, int64_t *k, int64_t *n_windows, int64_t *n_hits,
                             int64_t *n_occurrences, int64_t *n_positioned, int64_t *max_count, int64_t *device_bytes) {
    STG_TRY(check_obj(OCC, o));
    if (n_columns) *n_columns = o->n_nodes;
    if (k) *k = o->k;
    if (n_windows) *n_windows = o->n_windows;
    if (n_hits) *n_hits = o->n_hits;
    if (n_occurrences) *n_occurrences = o->n_occ;
    if (n_positioned) *n_positioned = o->n_positioned;
    if (max_count) *max_count = o->max_count;
    if (device_bytes) *device_bytes = (int64_t)o->bytes;
    return SBWTGPU_OK;
}

int sbwtgpu_occurrences_offsets_copy(const sbwtgpu_occurrences *o, uint64_t *off) {
    STG_TRY(check_obj(OCC, o));
    if (!off) return fail(SBWTGPU_ERR_INVALID_ARG, "occurrences: NULL argument (off)");
    DeviceGuard guard(o->device);
    std::lock_guard<std::mutex> lock(o->mu);
    HIP_TRY(hipMemcpyAsync(off, o->d_off, (size_t)(o->n_nodes + 1) * 8, hipMemcpyDeviceToHost, o->stream.s));
    HIP_TRY(hipStreamSynchronize(o->stream.s));
    return SBWTGPU_OK;
}

int sbwtgpu_occurrences_keys_copy(const sbwtgpu_occurrences *o, uint64_t *occ) {
    STG_TRY(check_obj(OCC, o));
    if (o->n_occ == 0) return SBWTGPU_OK;
    if (!occ) return fail(SBWTGPU_ERR_INVALID_ARG, "occurrences: NULL argument (occ)");
    DeviceGuard guard(o->device);
    std::lock_guard<std::mutex> lock(o->mu);
    HIP_TRY(hipMemcpyAsync(occ, o->d_occ, (size_t)o->n_occ * 8, hipMemcpyDeviceToHost, o->stream.s));
    HIP_TRY(hipStreamSynchronize(o->stream.s));
    return SBWTGPU_OK;
}

int sbwtgpu_occurrences_offsets_dev(const sbwtgpu_occurrences *o, const uint64_t **d_off) {
    if (!o || !d_off) return fail(SBWTGPU_ERR_INVALID_ARG, "occurrences: NULL argument");
    *d_off = reinterpret_cast<const uint64_t *>(o->d_off);
    return SBWTGPU_OK;
}

int sbwtgpu_occurrences_keys_dev(const sbwtgpu_occurrences *o, const uint64_t **d_occ) {
    if (!o || !d_occ) return fail(SBWTGPU_ERR_INVALID_ARG, "occurrences: NULL argument");
    *d_occ = reinterpret_cast<const uint64_t *>(o->d_occ);
    return SBWTGPU_OK;
}

// a positions object with every entry "no position", then first[v] = the column's smallest key
int sbwtgpu_occurrences_to_positions(const sbwtgpu_occurrences *o, sbwtgpu_positions **out) {
    if (!out) return fail(SBWTGPU_ERR_INVALID_ARG, "occurrences: NULL argument (out)");
    *out = nullptr;
    STG_TRY(check_obj(OCC, o));
    DeviceGuard guard(o->device);
    sbwtgpu_positions *p = nullptr;
    STG_TRY(sbwtgpu_positions_create(o->idx, &p));
    std::lock_guard<std::mutex> lock(o->mu);
    sbwt_launch_occ_first(o->d_off, o->d_occ, o->n_nodes, p->d_first, o->stream.s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(o->stream.s);
    if (e != hipSuccess) {
        sbwtgpu_positions_destroy(p);
        return hip_fail(OCC, e, "to_positions");
    }
    *out = p;
    return SBWTGPU_OK;
}

int64_t sbwtgpu_occurrences_map_workspace_bytes(int64_t total_bases, int64_t n_reads, int strands) {
    return map_workspace_bytes(total_bases, n_reads, strands);
}

int sbwtgpu_occurrences_map_dev(const sbwtgpu_occurrences *o, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                                int64_t n_reads, int strands, int max_occ, sbwtgpu_read_map *d_out, void *d_ws, int64_t ws_bytes,
                                void *stream) {
    STG_TRY(check_max_occ(max_occ));
    return map_dev(OCC, o, d_bases, total_bases, d_read_off, n_reads, strands, d_out, d_ws, ws_bytes, stream,
                   [&](const StrandSearch &q, SbwtReadMap *out, SbwtPosMapHeader *hdr, unsigned *d_slow, hipStream_t st) {
                       sbwt_launch_occ_map(q.res, q.res2, q.ooff, n_reads, o->d_off, o->d_occ, o->n_nodes, max_occ, g_occ_map_table, out, hdr,
                                           d_slow, st);
                   });
}

int sbwtgpu_occurrences_map_batch(const sbwtgpu_occurrences *o, const char *bases, const int64_t *read_off, int64_t n_reads, int strands,
                                  int max_occ, sbwtgpu_read_map *out) {
    STG_TRY(check_max_occ(max_occ));
    return map_batch(OCC, o, bases, read_off, n_reads, strands, out,
                     [&](const char *d_bases, int64_t nb, const int64_t *d_roff, int64_t nr, sbwtgpu_read_map *d_out, void *ws, int64_t ws_bytes,
                         void *st) { return sbwtgpu_occurrences_map_dev(o, d_bases, nb, d_roff, nr, strands, max_occ, d_out, ws, ws_bytes, st); });
}

}  // extern "C"
