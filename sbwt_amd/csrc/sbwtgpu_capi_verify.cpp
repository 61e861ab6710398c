// sbwtgpu_capi_verify.cpp -- the C ABI's verification layer: the reference sequences packed on the device (2 bits and one
// validity bit per base) and the call that checks mapped reads against them, mismatches on the voted diagonal and the best
// edit distance in a window around it (sbwt_verify.hip).  The calls need no index: they take reads, map
// records and the reference object.  What it shares with the other files: sbwtgpu_internal.h.
#include "sbwtgpu_internal.h"
#include "sbwt_verify.h"

using namespace sbwt_capi;

// knob of this file (sbwtgpu_set_tuning sets it)
int sbwt_capi::g_verify_fast_bases = 0;       // "verify_fast_bases": 0 = the compiled SBWT_VF_FAST_BASES

static_assert(sizeof(sbwtgpu_read_verify) == sizeof(SbwtReadVerify), "the record of the ABI is the kernels' record");
static_assert(sizeof(sbwtgpu_read_map) == sizeof(SbwtVerifyMap), "the map record of the ABI is the one the kernels read");
static_assert(SBWTGPU_VERIFY_MAX_BAND == SBWT_VF_MAX_BAND && SBWTGPU_VERIFY_MAX_READ == SBWT_VF_MAX_READ, "the header names the compiled limits");

// Three device arrays that grow by doubling (the 2-bit words, the validity words, the sequence table) and the counters; the
// sequences' lengths also on the host.  Adds hold `mu` for their whole length; the verify calls only read.
struct sbwtgpu_refseqs {
    int device = 0;
    Stream stream;
    mutable std::mutex mu;
    DevBuf ctr_mem;
    SbwtRefCounters *d_ctr = nullptr;
    unsigned long long *d_bits = nullptr, *d_valid = nullptr;
    SbwtRefSeq *d_tab = nullptr;
    int64_t cap_slots = 0, cap_seqs = 0;      // room: units of 64 bases; table entries
    int64_t n_slots = 0;                      // used
    int64_t total_bases = 0, n_invalid = 0;
    std::vector<int64_t> len;                 // per sequence
    ~sbwtgpu_refseqs() {
        if (d_bits) (void)hipFree(d_bits);
        if (d_valid) (void)hipFree(d_valid);
        if (d_tab) (void)hipFree(d_tab);
    }
    int64_t device_bytes() const { return 256 + cap_slots * 24 + cap_seqs * (int64_t)sizeof(SbwtRefSeq); }
};

static int ref_fail(hipError_t e, const char *what) {
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP, "refseqs: %s: %s", what, hipGetErrorString(e));
}

// room for `slots` units of 64 bases and `seqs` table entries (under r->mu).  Growing waits for the device, so that no call
// of the caller's still reads the arrays that are freed; what the object holds moves to the new arrays.  On failure the
// object is as it was.
static int ref_reserve(sbwtgpu_refseqs *r, int64_t slots, int64_t seqs) {
    if (slots > r->cap_slots) {
        int64_t cap = std::max<int64_t>(2 * r->cap_slots, 1024);
        while (cap < slots) cap *= 2;
        unsigned long long *b = nullptr, *v = nullptr;
        hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMalloc((void **)&b, (size_t)cap * 16);
        if (e == hipSuccess) e = hipMalloc((void **)&v, (size_t)cap * 8);
        if (e == hipSuccess && r->n_slots > 0) e = hipMemcpy(b, r->d_bits, (size_t)r->n_slots * 16, hipMemcpyDeviceToDevice);
        if (e == hipSuccess && r->n_slots > 0) e = hipMemcpy(v, r->d_valid, (size_t)r->n_slots * 8, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) {
            if (b) (void)hipFree(b);
            if (v) (void)hipFree(v);
            return ref_fail(e, "growing the packed arrays");
        }
        if (r->d_bits) (void)hipFree(r->d_bits);
        if (r->d_valid) (void)hipFree(r->d_valid);
        r->d_bits = b;
        r->d_valid = v;
        r->cap_slots = cap;
    }
    if (seqs > r->cap_seqs) {
        int64_t cap = std::max<int64_t>(2 * r->cap_seqs, 256);
        while (cap < seqs) cap *= 2;
        SbwtRefSeq *t = nullptr;
        hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMalloc((void **)&t, (size_t)cap * sizeof(SbwtRefSeq));
        if (e == hipSuccess && !r->len.empty()) e = hipMemcpy(t, r->d_tab, r->len.size() * sizeof(SbwtRefSeq), hipMemcpyDeviceToDevice);
        if (e != hipSuccess) {
            if (t) (void)hipFree(t);
            return ref_fail(e, "growing the sequence table");
        }
        if (r->d_tab) (void)hipFree(r->d_tab);
        r->d_tab = t;
        r->cap_seqs = cap;
    }
    return SBWTGPU_OK;
}

// [SbwtVerifyHeader][the list: 4 bytes per read]
int64_t sbwt_capi::verify_workspace_bytes(int64_t n_reads) {
    if (n_reads < 0) n_reads = 0;
    return (int64_t)sizeof(SbwtVerifyHeader) + align256(n_reads * 4);
}

int sbwt_capi::check_verify(const sbwtgpu_refseqs *r, int64_t n_reads, int band) {
    if (!r) return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: the object is NULL");
    if (band < 0 || band > SBWTGPU_VERIFY_MAX_BAND)
        return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: band must be in 0 .. %d, not %d", SBWTGPU_VERIFY_MAX_BAND, band);
    if (n_reads < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: negative n_reads");
    if (n_reads >= ((int64_t)1 << 31)) return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: 2^31 reads or more in one call: split the batch");
    return SBWTGPU_OK;
}

RefSeqsView sbwt_capi::refseqs_view(const sbwtgpu_refseqs *r) {
    return RefSeqsView{r->device, r->d_tab, (int64_t)r->len.size(), r->d_bits, r->d_valid};
}

extern "C" {

int sbwtgpu_refseqs_create(int device, sbwtgpu_refseqs **out) {
    if (!out) return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: NULL argument (out)");
    *out = nullptr;
    DeviceGuard guard(device);
    if (!guard.ok) {
        (void)hipGetLastError();
        return fail(SBWTGPU_ERR_NO_DEVICE, "hipSetDevice(%d) failed", device);
    }
    sbwtgpu_refseqs *r = new (std::nothrow) sbwtgpu_refseqs();
    if (!r) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    r->device = device;
    hipError_t e = hipStreamCreateWithFlags(&r->stream.s, hipStreamNonBlocking);
    if (e == hipSuccess) e = r->ctr_mem.alloc(256);
    if (e == hipSuccess) e = hipMemset(r->ctr_mem.p, 0, 256);
    if (e != hipSuccess) {
        delete r;
        return ref_fail(e, "allocation");
    }
    r->d_ctr = static_cast<SbwtRefCounters *>(r->ctr_mem.p);
    *out = r;
    return SBWTGPU_OK;
}

void sbwtgpu_refseqs_destroy(sbwtgpu_refseqs *r) {
    if (!r) return;
    DeviceGuard guard(r->device);
    delete r;
}

// The whole add holds the object's mutex: the arrays may move when they grow.  Every allocation comes before the first change.
int sbwtgpu_refseqs_add_batch(sbwtgpu_refseqs *r, int64_t first_seq, const char *bases, const int64_t *read_off, int64_t n) {
    if (!r) return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: the object is NULL");
    if (n < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: negative n_seqs");
    std::lock_guard<std::mutex> lock(r->mu);
    const int64_t have = (int64_t)r->len.size();
    if (first_seq != have)
        return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: first_seq is %lld, the object holds %lld sequences and the next number is %lld",
                    (long long)first_seq, (long long)have, (long long)have);
    if (have + n > ((int64_t)1 << 30))
        return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: %lld sequences are more than 2^30", (long long)(have + n));
    if (n == 0) return SBWTGPU_OK;
    if (!read_off) return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: NULL argument (read_off)");
    if (read_off[n] > read_off[0] && !bases) return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: NULL argument (bases)");
    std::vector<SbwtRefSeq> tab;
    std::vector<int64_t> src_off;
    try {
        tab.resize((size_t)n);
        src_off.resize((size_t)n + 1);
        r->len.reserve((size_t)(have + n));
    } catch (const std::bad_alloc &) {
        return fail(SBWTGPU_ERR_OOM, "out of host memory");
    }
    int64_t slot = r->n_slots;
    for (int64_t i = 0; i < n; i++) {
        STG_TRY(check_read_length(read_off, i));
        const int64_t len = read_off[i + 1] - read_off[i];
        tab[(size_t)i] = SbwtRefSeq{slot, len};
        src_off[(size_t)i] = read_off[i] - read_off[0];
        slot += (len + 63) / 64;
    }
    const int64_t batch_bases = read_off[n] - read_off[0];
    src_off[(size_t)n] = batch_bases;
    DeviceGuard guard(r->device);
    DevBuf d_src, d_off;
    hipError_t e = d_src.alloc((size_t)batch_bases);
    if (e == hipSuccess) e = d_off.alloc((size_t)(n + 1) * 8);
    if (e != hipSuccess) return ref_fail(e, "staging a batch");
    STG_TRY(ref_reserve(r, slot, have + n));
    hipStream_t st = r->stream.s;
    SbwtRefCounters h;
    if (batch_bases > 0) e = hipMemcpyAsync(d_src.p, bases + read_off[0], (size_t)batch_bases, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off.p, src_off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(r->d_tab + have, tab.data(), (size_t)n * sizeof(SbwtRefSeq), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        sbwt_launch_ref_pack(static_cast<const char *>(d_src.p), static_cast<const long long *>(d_off.p), r->d_tab, have, n, r->n_slots, slot,
                             r->d_bits, r->d_valid, r->d_ctr, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h, r->d_ctr, sizeof(h), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        // (the words behind n_slots and the entries behind `have` belong to nobody; the count of invalid bases is set back)
        (void)hipGetLastError();
        h.n_invalid = (unsigned long long)r->n_invalid;
        (void)hipMemcpy(&r->d_ctr->n_invalid, &h.n_invalid, 8, hipMemcpyHostToDevice);
        return ref_fail(e, "add");
    }
    for (int64_t i = 0; i < n; i++) r->len.push_back(tab[(size_t)i].len);
    r->n_slots = slot;
    r->total_bases += batch_bases;
    r->n_invalid = (int64_t)h.n_invalid;
    return SBWTGPU_OK;
}

int sbwtgpu_refseqs_info(const sbwtgpu_refseqs *r, int64_t *n_seqs, int64_t *total_bases, int64_t *n_invalid, int64_t *device_bytes) {
    if (!r) return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: the object is NULL");
    std::lock_guard<std::mutex> lock(r->mu);
    if (n_seqs) *n_seqs = (int64_t)r->len.size();
    if (total_bases) *total_bases = r->total_bases;
    if (n_invalid) *n_invalid = r->n_invalid;
    if (device_bytes) *device_bytes = r->device_bytes();
    return SBWTGPU_OK;
}

int sbwtgpu_refseqs_lengths_copy(const sbwtgpu_refseqs *r, int64_t *len) {
    if (!r) return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: the object is NULL");
    std::lock_guard<std::mutex> lock(r->mu);
    if (r->len.empty()) return SBWTGPU_OK;
    if (!len) return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: NULL argument (len)");
    memcpy(len, r->len.data(), r->len.size() * 8);
    return SBWTGPU_OK;
}

int sbwtgpu_refseqs_get(const sbwtgpu_refseqs *r, int64_t seq, int64_t pos, int64_t len, char *out) {
    if (!r) return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: the object is NULL");
    std::lock_guard<std::mutex> lock(r->mu);
    if (seq < 0 || seq >= (int64_t)r->len.size())
        return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: sequence %lld of %lld", (long long)seq, (long long)r->len.size());
    const int64_t n = r->len[(size_t)seq];
    if (pos < 0 || len < 0 || pos > n || len > n - pos)
        return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: bases %lld .. %lld lie outside sequence %lld of %lld bases", (long long)pos,
                    (long long)pos + (long long)len, (long long)seq, (long long)n);
    if (len == 0) return SBWTGPU_OK;
    if (!out) return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: NULL argument (out)");
    DeviceGuard guard(r->device);
    SbwtRefSeq s;
    HIP_TRY(hipMemcpy(&s, r->d_tab + seq, sizeof(s), hipMemcpyDeviceToHost));
    Staging g;
    STG_TRY(g.open(r->device, (size_t)align256(len)));
    sbwt_launch_ref_unpack(r->d_bits, r->d_valid, s.slot, pos, len, g.at<char>(0), g.stream);
    HIP_TRY(hipGetLastError());
    STG_TRY(g.out(0, out, (size_t)len));
    return g.finish();
}

int64_t sbwtgpu_refseqs_verify_workspace_bytes(int64_t total_bases, int64_t n_reads) {
    (void)total_bases;              // (the workspace holds the list of reads for the second kernel and nothing per base)
    return verify_workspace_bytes(n_reads);
}

int sbwtgpu_refseqs_verify_dev(const sbwtgpu_refseqs *r, const char *d_bases, int64_t total_bases, const int64_t *d_read_off,
                               int64_t n_reads, const sbwtgpu_read_map *d_map, int band, sbwtgpu_read_verify *d_out, void *d_ws,
                               int64_t ws_bytes, void *stream) {
    STG_TRY(check_verify(r, n_reads, band));
    STG_TRY(check_batch_dev(n_reads, total_bases, d_ws, ws_bytes, verify_workspace_bytes(n_reads)));
    if (n_reads == 0) return SBWTGPU_OK;
    if (!d_read_off || !d_map || !d_out || (total_bases > 0 && !d_bases))
        return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: NULL device pointer (d_bases, d_read_off, d_map and d_out are needed)");
    DeviceGuard guard(r->device);
    char *w = static_cast<char *>(d_ws);
    sbwt_launch_verify(d_bases, total_bases, reinterpret_cast<const long long *>(d_read_off), n_reads,
                       reinterpret_cast<const SbwtVerifyMap *>(d_map), r->d_tab, (int64_t)r->len.size(), r->d_bits, r->d_valid, band,
                       g_verify_fast_bases, reinterpret_cast<SbwtReadVerify *>(d_out), reinterpret_cast<SbwtVerifyHeader *>(w),
                       reinterpret_cast<unsigned *>(w + sizeof(SbwtVerifyHeader)), static_cast<hipStream_t>(stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return SBWTGPU_OK;
}

// One call of the staging layer that is not pipelined: bases, offsets and map records go down, the records come back.  (The
// chunked ReadPipe stages bases and offsets only; a per-read INPUT region would change its stage() for every user.)
int sbwtgpu_refseqs_verify_batch(const sbwtgpu_refseqs *r, const char *bases, const int64_t *read_off, int64_t n_reads,
                                 const sbwtgpu_read_map *map, int band, sbwtgpu_read_verify *out) {
    STG_TRY(check_verify(r, n_reads, band));
    if (n_reads == 0) return SBWTGPU_OK;
    if (!read_off || !map || !out) return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: NULL argument (read_off, map and out are needed)");
    const int64_t nb = read_off[n_reads] - read_off[0];
    if (nb > 0 && !bases) return fail(SBWTGPU_ERR_INVALID_ARG, "refseqs: NULL argument (bases)");
    for (int64_t i = 0; i < n_reads; i++) STG_TRY(check_read_length(read_off, i));
    STG_TRY(check_batch_sizes(n_reads, nb));
    const int64_t ws_bytes = verify_workspace_bytes(n_reads);
    const size_t o_off = (size_t)align256(nb + 16), o_map = o_off + (size_t)align256((n_reads + 1) * 8),
                 o_out = o_map + (size_t)align256(n_reads * (int64_t)sizeof(sbwtgpu_read_map)),
                 o_ws = o_out + (size_t)align256(n_reads * (int64_t)sizeof(sbwtgpu_read_verify));
    DeviceGuard guard(r->device);
    Staging g;
    STG_TRY(g.open(r->device, o_ws + (size_t)ws_bytes));
    STG_TRY(g.in(0, bases + read_off[0], (size_t)nb));
    STG_TRY(g.in_rebased(o_off, read_off, n_reads + 1));
    STG_TRY(g.in(o_map, map, (size_t)n_reads * sizeof(sbwtgpu_read_map)));
    STG_TRY(g.upload());
    STG_TRY(sbwtgpu_refseqs_verify_dev(r, g.at<char>(0), nb, g.at<int64_t>(o_off), n_reads, g.at<sbwtgpu_read_map>(o_map), band,
                                       g.at<sbwtgpu_read_verify>(o_out), g.at<char>(o_ws), ws_bytes, g.stream));
    STG_TRY(g.out(o_out, out, (size_t)n_reads * sizeof(sbwtgpu_read_verify)));
    return g.finish();
}

}  // extern "C"
