// sbwtgpu_capi_pileup.cpp -- the C ABI's pileup layer: per-base counters of a read set's alignments that live on the device
// across batches, read out as records and as calls (sbwt_pileup.hip).  The verify and align calls run as
// they are.  What it shares with the other files: sbwtgpu_internal.h.
#include "sbwtgpu_internal.h"
#include "sbwt_pileup.h"

#include <cstdlib>

using namespace sbwt_capi;

static_assert(sizeof(sbwtgpu_pileup_base) == sizeof(SbwtPileBase) && sizeof(sbwtgpu_pileup_call) == sizeof(SbwtPileCall) &&
                  sizeof(sbwtgpu_pileup_filter) == sizeof(SbwtPileFilter),
              "the records of the ABI are the kernels' records");

// The adds only ever add to the cells and the counters with atomics; the read-outs take `mu` and share the block sums, so each
// waits on the device for the one before it (`readout`).  `offered` is the host's count of the reads offered since the last
// reset: what the overflow rule asks.
struct sbwtgpu_pileup {
    const sbwtgpu_refseqs *r = nullptr;
    int device = 0;
    std::vector<SbwtRefSeq> tab;                // the sequences covered: r's at create
    int64_t n_slots = 0, n_cells = 0, total_bases = 0;
    DevBuf cells_mem, ctr_mem, bsum_mem;
    Stream stream;
    hipEvent_t readout = nullptr;
    mutable std::mutex mu;
    std::atomic<int64_t> offered{0};
    SbwtPileCell *cells() const { return static_cast<SbwtPileCell *>(cells_mem.p); }
    SbwtPileCounters *ctr() const { return static_cast<SbwtPileCounters *>(ctr_mem.p); }
    long long *bsum() const { return static_cast<long long *>(bsum_mem.p); }
    int64_t n_seqs() const { return (int64_t)tab.size(); }
    int64_t device_bytes() const { return n_cells * 32 + 256 + (sbwt_pile_blocks(n_cells) + 1) * 8; }
    ~sbwtgpu_pileup() {
        if (readout) (void)hipEventDestroy(readout);
    }
};

static int64_t records_bytes(int64_t n_reads) { return 2 * align256(n_reads * 16) + align256((n_reads + 1) * 8); }

// [the align workspace][verify records][align records][run offsets][2 L runs per read]
static int64_t pileup_workspace_bytes(int64_t total_bases, int64_t n_reads) {
    if (total_bases < 0) total_bases = 0;
    if (n_reads < 0) n_reads = 0;
    return sbwtgpu_align_workspace_bytes(total_bases, n_reads) + records_bytes(n_reads) + align256(2 * total_bases * 4 + 16);
}

static int check_filter(const sbwtgpu_pileup *p, const sbwtgpu_pileup_filter *f) {
    if (!p) return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: the object is NULL");
    if (!f) return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: NULL argument (the filter)");
    if (f->reserved != 0) return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: the filter's reserved field must be 0, not %d", (int)f->reserved);
    return SBWTGPU_OK;
}

// the overflow rule: the reads offered since the last reset stay below 2^31, so that no 32-bit counter can wrap
static int take_offered(sbwtgpu_pileup *p, int64_t n_reads) {
    const int64_t before = p->offered.fetch_add(n_reads);
    if (before + n_reads > (int64_t)INT32_MAX) {
        p->offered.fetch_sub(n_reads);
        return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: %lld reads on top of %lld would take the reads offered since the last reset above 2^31 - 1",
                    (long long)n_reads, (long long)before);
    }
    return SBWTGPU_OK;
}

// The start of a read-out on `st` (under mu): after the read-out before it, then the scanned block sums of the depth
static int begin_readout(const sbwtgpu_pileup *p, hipStream_t st) {
    HIP_TRY(hipStreamWaitEvent(st, p->readout, 0));
    sbwt_launch_pile_scan(p->cells(), p->n_cells, p->bsum(), st);
    HIP_TRY(hipGetLastError());
    return SBWTGPU_OK;
}
static int end_readout(const sbwtgpu_pileup *p, hipStream_t st) {
    HIP_TRY(hipEventRecord(p->readout, st));
    return SBWTGPU_OK;
}

static int check_range(const sbwtgpu_pileup *p, int64_t seq, int64_t pos, int64_t len) {
    if (!p) return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: the object is NULL");
    if (seq < 0 || seq >= p->n_seqs()) return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: sequence %lld of %lld", (long long)seq, (long long)p->n_seqs());
    const int64_t n = p->tab[(size_t)seq].len;
    if (pos < 0 || len < 0 || pos > n || len > n - pos)
        return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: bases %lld .. %lld lie outside sequence %lld of %lld bases", (long long)pos,
                    (long long)pos + (long long)len, (long long)seq, (long long)n);
    return SBWTGPU_OK;
}

static int counts_on(const sbwtgpu_pileup *p, int64_t seq, int64_t pos, int64_t len, sbwtgpu_pileup_base *d_out, hipStream_t st) {
    const RefSeqsView v = refseqs_view(p->r);
    STG_TRY(begin_readout(p, st));
    sbwt_launch_pile_counts(p->cells(), p->n_cells, p->bsum(), v.d_bits, v.d_valid, p->tab[(size_t)seq].slot, pos, len,
                            reinterpret_cast<SbwtPileBase *>(d_out), st);
    HIP_TRY(hipGetLastError());
    return end_readout(p, st);
}

extern "C" {

int sbwtgpu_pileup_create(const sbwtgpu_refseqs *r, sbwtgpu_pileup **out) {
    if (!r || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: NULL argument (r and out are needed)");
    *out = nullptr;
    const RefSeqsView v = refseqs_view(r);
    DeviceGuard guard(v.device);
    if (!guard.ok) return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", v.device);
    sbwtgpu_pileup *p = new (std::nothrow) sbwtgpu_pileup();
    if (!p) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    p->r = r;
    p->device = v.device;
    try {
        p->tab.resize((size_t)v.n_seqs);
    } catch (const std::bad_alloc &) {
        delete p;
        return fail(SBWTGPU_ERR_OOM, "out of host memory");
    }
    hipError_t e = hipSuccess;
    if (v.n_seqs > 0) e = hipMemcpy(p->tab.data(), v.d_tab, (size_t)v.n_seqs * sizeof(SbwtRefSeq), hipMemcpyDeviceToHost);
    if (e == hipSuccess) {
        for (const SbwtRefSeq &s : p->tab) {
            p->n_slots = std::max<int64_t>(p->n_slots, s.slot + (s.len + 63) / 64);
            p->total_bases += s.len;
        }
        p->n_cells = 64 * p->n_slots + 1;       // (one beyond the last slot: the -1 of a read that ends at the last sequence's n)
        e = hipStreamCreateWithFlags(&p->stream.s, hipStreamNonBlocking);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->readout, hipEventDisableTiming);
    if (e == hipSuccess) e = p->cells_mem.alloc((size_t)p->n_cells * sizeof(SbwtPileCell));
    if (e == hipSuccess) e = p->ctr_mem.alloc(sizeof(SbwtPileCounters));
    if (e == hipSuccess) e = p->bsum_mem.alloc((size_t)(sbwt_pile_blocks(p->n_cells) + 1) * 8);
    if (e == hipSuccess) e = hipMemsetAsync(p->cells_mem.p, 0, (size_t)p->n_cells * sizeof(SbwtPileCell), p->stream.s);
    if (e == hipSuccess) e = hipMemsetAsync(p->ctr_mem.p, 0, sizeof(SbwtPileCounters), p->stream.s);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream.s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        delete p;
        return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "pileup: allocation: %s", hipGetErrorString(e));
    }
    *out = p;
    return SBWTGPU_OK;
}

void sbwtgpu_pileup_destroy(sbwtgpu_pileup *p) {
    if (!p) return;
    DeviceGuard guard(p->device);
    delete p;
}

int sbwtgpu_pileup_reset(sbwtgpu_pileup *p) {
    if (!p) return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: the object is NULL");
    DeviceGuard guard(p->device);
    std::lock_guard<std::mutex> lock(p->mu);
    // (adds of the caller's on other streams have to be over, as for the read-outs: the device is waited for, then zeroed)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemsetAsync(p->cells_mem.p, 0, (size_t)p->n_cells * sizeof(SbwtPileCell), p->stream.s));
    HIP_TRY(hipMemsetAsync(p->ctr_mem.p, 0, sizeof(SbwtPileCounters), p->stream.s));
    HIP_TRY(hipStreamSynchronize(p->stream.s));
    p->offered.store(0);
    return SBWTGPU_OK;
}

int sbwtgpu_pileup_add_aligned_dev(sbwtgpu_pileup *p, const char *d_bases, int64_t total_bases, const int64_t *d_read_off, int64_t n_reads,
                                   const sbwtgpu_read_map *d_map, const sbwtgpu_read_verify *d_verify, const sbwtgpu_read_align *d_align,
                                   const int64_t *d_op_off, const uint32_t *d_ops, const sbwtgpu_pileup_filter *f, void *stream) {
    STG_TRY(check_filter(p, f));
    STG_TRY(check_verify(p->r, n_reads, 0));
    STG_TRY(check_batch_sizes(n_reads, total_bases));
    if (n_reads == 0) return SBWTGPU_OK;
    if (!d_read_off || !d_map || !d_verify || !d_align || !d_op_off || (total_bases > 0 && !d_bases))
        return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: NULL device pointer (d_bases, d_read_off, d_map, d_verify, d_align and d_op_off are needed)");
    STG_TRY(take_offered(p, n_reads));
    const RefSeqsView v = refseqs_view(p->r);
    DeviceGuard guard(p->device);
    const SbwtPileFilter ff = {f->min_votes, f->require_unique, f->max_edit, 0};
    sbwt_launch_pile_add(d_bases, total_bases, reinterpret_cast<const long long *>(d_read_off), n_reads,
                         reinterpret_cast<const SbwtVerifyMap *>(d_map), reinterpret_cast<const SbwtReadVerify *>(d_verify),
                         reinterpret_cast<const SbwtReadAlign *>(d_align), reinterpret_cast<const long long *>(d_op_off), d_ops, ff,
                         static_cast<const SbwtRefSeq *>(v.d_tab), p->n_seqs(), p->cells(), p->n_cells, p->ctr(), static_cast<hipStream_t>(stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return SBWTGPU_OK;
}

int64_t sbwtgpu_pileup_workspace_bytes(int64_t total_bases, int64_t n_reads) { return pileup_workspace_bytes(total_bases, n_reads); }

int sbwtgpu_pileup_add_dev(sbwtgpu_pileup *p, const char *d_bases, int64_t total_bases, const int64_t *d_read_off, int64_t n_reads,
                           const sbwtgpu_read_map *d_map, int band, const sbwtgpu_pileup_filter *f, void *d_ws, int64_t ws_bytes, void *stream) {
    STG_TRY(check_filter(p, f));
    STG_TRY(check_verify(p->r, n_reads, band));
    STG_TRY(check_batch_dev(n_reads, total_bases, d_ws, ws_bytes, pileup_workspace_bytes(total_bases, n_reads)));
    if (n_reads == 0) return SBWTGPU_OK;
    if (!d_read_off || !d_map || (total_bases > 0 && !d_bases))
        return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: NULL device pointer (d_bases, d_read_off and d_map are needed)");
    if (p->offered.load() + n_reads > (int64_t)INT32_MAX) return take_offered(p, n_reads);      // (refused before anything runs)
    const int64_t aws = sbwtgpu_align_workspace_bytes(total_bases, n_reads), rec = align256(n_reads * 16);
    char *w = static_cast<char *>(d_ws) + aws;
    sbwtgpu_read_verify *d_ver = reinterpret_cast<sbwtgpu_read_verify *>(w);
    sbwtgpu_read_align *d_al = reinterpret_cast<sbwtgpu_read_align *>(w + rec);
    int64_t *d_ooff = reinterpret_cast<int64_t *>(w + 2 * rec);
    uint32_t *d_ops = reinterpret_cast<uint32_t *>(w + records_bytes(n_reads));
    STG_TRY(sbwtgpu_align_dev(p->r, d_bases, total_bases, d_read_off, n_reads, d_map, band, d_ver, d_al, d_ooff, d_ops, 2 * total_bases, d_ws,
                              aws, stream));
    return sbwtgpu_pileup_add_aligned_dev(p, d_bases, total_bases, d_read_off, n_reads, d_map, d_ver, d_al, d_ooff, d_ops, f, stream);
}

// One staged range, as sbwtgpu_align_batch: bases, offsets and map records go down, nothing comes back.
int sbwtgpu_pileup_add_batch(sbwtgpu_pileup *p, const char *bases, const int64_t *read_off, int64_t n_reads, const sbwtgpu_read_map *map,
                             int band, const sbwtgpu_pileup_filter *f) {
    STG_TRY(check_filter(p, f));
    STG_TRY(check_verify(p->r, n_reads, band));
    if (n_reads == 0) return SBWTGPU_OK;
    if (!read_off || !map) return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: NULL argument (read_off and map are needed)");
    const int64_t nb = read_off[n_reads] - read_off[0];
    if (nb > 0 && !bases) return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: NULL argument (bases)");
    for (int64_t i = 0; i < n_reads; i++) STG_TRY(check_read_length(read_off, i));
    STG_TRY(check_batch_sizes(n_reads, nb));
    const int64_t ws_bytes = pileup_workspace_bytes(nb, n_reads);
    const size_t o_off = (size_t)align256(nb + 16), o_map = o_off + (size_t)align256((n_reads + 1) * 8),
                 o_ws = o_map + (size_t)align256(n_reads * (int64_t)sizeof(sbwtgpu_read_map));
    DeviceGuard guard(p->device);
    Staging g;
    STG_TRY(g.open(p->device, o_ws + (size_t)ws_bytes));
    STG_TRY(g.in(0, bases + read_off[0], (size_t)nb));
    STG_TRY(g.in_rebased(o_off, read_off, n_reads + 1));
    STG_TRY(g.in(o_map, map, (size_t)n_reads * sizeof(sbwtgpu_read_map)));
    STG_TRY(g.upload());
    STG_TRY(sbwtgpu_pileup_add_dev(p, g.at<char>(0), nb, g.at<int64_t>(o_off), n_reads, g.at<sbwtgpu_read_map>(o_map), band, f, g.at<char>(o_ws),
                                   ws_bytes, g.stream));
    return g.finish();
}

int sbwtgpu_pileup_info(const sbwtgpu_pileup *p, int64_t *n_seqs, int64_t *total_bases, int64_t *n_offered, int64_t *n_piled,
                        int64_t *n_columns, int64_t *n_clipped, int64_t *n_overhang, int64_t *device_bytes) {
    if (!p) return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: the object is NULL");
    if (n_seqs) *n_seqs = p->n_seqs();
    if (total_bases) *total_bases = p->total_bases;
    if (device_bytes) *device_bytes = p->device_bytes();
    if (!n_offered && !n_piled && !n_columns && !n_clipped && !n_overhang) return SBWTGPU_OK;
    DeviceGuard guard(p->device);
    std::lock_guard<std::mutex> lock(p->mu);
    SbwtPileCounters h;
    HIP_TRY(hipDeviceSynchronize());            // (every add that has returned, on whichever stream)
    HIP_TRY(hipMemcpyAsync(&h, p->ctr(), sizeof(h), hipMemcpyDeviceToHost, p->stream.s));
    HIP_TRY(hipStreamSynchronize(p->stream.s));
    if (n_offered) *n_offered = (int64_t)h.n_offered;
    if (n_piled) *n_piled = (int64_t)h.n_piled;
    if (n_columns) *n_columns = (int64_t)h.n_columns;
    if (n_clipped) *n_clipped = (int64_t)h.n_clipped;
    if (n_overhang) *n_overhang = (int64_t)h.n_overhang;
    return SBWTGPU_OK;
}

int sbwtgpu_pileup_counts_dev(const sbwtgpu_pileup *p, int64_t seq, int64_t pos, int64_t len, sbwtgpu_pileup_base *d_out, void *stream) {
    STG_TRY(check_range(p, seq, pos, len));
    if (len == 0) return SBWTGPU_OK;
    if (!d_out) return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: NULL device pointer (d_out)");
    DeviceGuard guard(p->device);
    std::lock_guard<std::mutex> lock(p->mu);
    return counts_on(p, seq, pos, len, d_out, static_cast<hipStream_t>(stream));
}

int sbwtgpu_pileup_counts_copy(const sbwtgpu_pileup *p, int64_t seq, int64_t pos, int64_t len, sbwtgpu_pileup_base *out) {
    STG_TRY(check_range(p, seq, pos, len));
    if (len == 0) return SBWTGPU_OK;
    if (!out) return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: NULL argument (out)");
    DeviceGuard guard(p->device);
    std::lock_guard<std::mutex> lock(p->mu);
    DevBuf d;
    HIP_TRY(d.alloc((size_t)len * sizeof(sbwtgpu_pileup_base)));
    HIP_TRY(hipDeviceSynchronize());            // (every add that has returned, on whichever stream)
    STG_TRY(counts_on(p, seq, pos, len, static_cast<sbwtgpu_pileup_base *>(d.p), p->stream.s));
    HIP_TRY(hipMemcpyAsync(out, d.p, (size_t)len * sizeof(sbwtgpu_pileup_base), hipMemcpyDeviceToHost, p->stream.s));
    HIP_TRY(hipStreamSynchronize(p->stream.s));
    return SBWTGPU_OK;
}

// count, scan, fill: the calls of every block of 1024 cells are counted, the counts scanned, and every block stores its calls
// at its offset, in the pattern of the bubbles' fill.
int sbwtgpu_pileup_calls(const sbwtgpu_pileup *p, int32_t min_depth, int32_t min_alt, int32_t min_frac_ppm, sbwtgpu_pileup_call **out,
                         int64_t *n) {
    if (!p) return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: the object is NULL");
    if (!out || !n) return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: NULL argument (out and n are needed)");
    *out = nullptr;
    *n = 0;
    if (min_depth < 1) return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: min_depth must be at least 1, not %d", (int)min_depth);
    if (min_alt < 1) return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: min_alt must be at least 1, not %d", (int)min_alt);
    if (min_frac_ppm < 0 || min_frac_ppm > 1000000)
        return fail(SBWTGPU_ERR_INVALID_ARG, "pileup: min_frac_ppm must be in 0 .. 1000000, not %d", (int)min_frac_ppm);
    if (p->n_seqs() == 0) return SBWTGPU_OK;
    const RefSeqsView v = refseqs_view(p->r);
    DeviceGuard guard(p->device);
    std::lock_guard<std::mutex> lock(p->mu);
    hipStream_t st = p->stream.s;
    const int64_t nb = sbwt_pile_blocks(p->n_cells);
    DevBuf d_cnt, d_off, d_bs, d_calls;
    HIP_TRY(d_cnt.alloc((size_t)nb * 8));
    HIP_TRY(d_off.alloc((size_t)(nb + 1) * 8));
    HIP_TRY(d_bs.alloc((size_t)(nb / 1024 + 2) * 8));
    HIP_TRY(hipDeviceSynchronize());            // (every add that has returned, on whichever stream)
    STG_TRY(begin_readout(p, st));
    const SbwtRefSeq *tab = static_cast<const SbwtRefSeq *>(v.d_tab);
    sbwt_launch_pile_calls(p->cells(), p->n_cells, p->bsum(), v.d_bits, v.d_valid, tab, p->n_seqs(), min_depth, min_alt, min_frac_ppm,
                           static_cast<long long *>(d_cnt.p), nullptr, nullptr, st);
    sbwt_launch_pile_scan_i64(static_cast<const long long *>(d_cnt.p), nb, static_cast<long long *>(d_bs.p), static_cast<long long *>(d_off.p), st);
    HIP_TRY(hipGetLastError());
    int64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, static_cast<const long long *>(d_off.p) + nb, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (total < 0 || total > 5 * p->total_bases) return fail(SBWTGPU_ERR_HIP, "internal: %lld calls on %lld bases", (long long)total, (long long)p->total_bases);
    if (total == 0) return end_readout(p, st);
    sbwtgpu_pileup_call *h = static_cast<sbwtgpu_pileup_call *>(malloc((size_t)total * sizeof(sbwtgpu_pileup_call)));
    if (!h) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    hipError_t e = d_calls.alloc((size_t)total * sizeof(sbwtgpu_pileup_call));
    if (e == hipSuccess) {
        sbwt_launch_pile_calls(p->cells(), p->n_cells, p->bsum(), v.d_bits, v.d_valid, tab, p->n_seqs(), min_depth, min_alt, min_frac_ppm, nullptr,
                               static_cast<const long long *>(d_off.p), reinterpret_cast<SbwtPileCall *>(d_calls.p), st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(p->readout, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h, d_calls.p, (size_t)total * sizeof(sbwtgpu_pileup_call), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        free(h);
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "pileup: calls: %s", hipGetErrorString(e));
    }
    *out = h;
    *n = total;
    return SBWTGPU_OK;
}

}  // extern "C"
