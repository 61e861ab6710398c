// sbwtgpu_internal.h -- what the translation units of the C ABI share: sbwtgpu_capi.cpp (index image, search, rank, text),
// sbwtgpu_capi_reads.cpp (matching statistics, set operations, read hits, unitigs and their graph, walks, bubbles) and
// sbwtgpu_capi_colors.cpp (colours, colour sets, pseudoalignment, screen) and sbwtgpu_capi_placement.cpp (reference positions and
// all occurrences per column, read mapping over either) and sbwtgpu_capi_verify.cpp (the packed reference sequences and the
// verification of mapped reads against them) and sbwtgpu_capi_align.cpp (the alignment of verified reads).  Nothing here is part of the library's interface:
// every name has hidden visibility, and whatever holds state (the error text, the parked slots, the int32 switch of a search
// call) is defined once, in sbwtgpu_capi.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cassert>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/sbwtgpu.h"
#include "sbwt_device.h"
#include "sbwt_unitigs.h"
#include "sbwt_read_chunks.h"

#pragma GCC visibility push(hidden)

namespace sbwt_capi {

// sets the calling thread's error text (sbwtgpu_last_error) and returns code
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// a search's device status word (SbwtWorkHeader::status) as the call's result: a k-mer search that did not end on one column,
// or the sorted fused kernel's stall detector (a workgroup that made no progress for 2^20 waits)
int fail_status(int status);

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(e_ == hipErrorOutOfMemory ? SBWTGPU_ERR_OOM : SBWTGPU_ERR_HIP,         \
                        "%s failed: %s", #expr, hipGetErrorString(e_));                        \
    } while (0)
#define STG_TRY(expr)                                                                          \
    do {                                                                                       \
        const int rc_ = (expr);                                                                \
        if (rc_ != SBWTGPU_OK) return rc_;                                                     \
    } while (0)

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
struct Stream {
    hipStream_t s = nullptr;
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
};

template <typename T>
inline T align256(T x) { return (x + 255) & ~(T)255; }

inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

inline constexpr const char *RANK_ONLY_MSG =
    "the index columns are not a valid SBWT (set bits != n_nodes - 1): only rank() is available";

// tuning knobs that sbwtgpu_set_tuning (sbwtgpu_capi.cpp) sets for another file, each defined in the file that reads it; none
// is read before main (a knob with an environment default is a dynamic initialiser of its own file)
extern int g_poison;                                        // sbwtgpu_capi.cpp; the derived layers poison their results too
extern int g_rh_wave_min, g_rh_wide;                        // sbwtgpu_capi_reads.cpp
extern int64_t g_rh_chunk_bases, g_wk_chunk_bases, g_gt_chunk_bases;
extern int64_t g_pa_chunk_bases, g_screen_chunk_bases;      // sbwtgpu_capi_colors.cpp
extern int64_t g_gram_mfma_min_sets, g_gram_flush_sets;
extern int64_t g_pos_chunk_bases, g_occ_chunk_bases;        // sbwtgpu_capi_placement.cpp
extern int g_pos_map_table, g_occ_map_table;
extern int g_verify_fast_bases;                             // sbwtgpu_capi_verify.cpp
extern int g_align_fast_edit;                               // sbwtgpu_capi_align.cpp

}  // namespace sbwt_capi

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
    int probe_len(bool allow_override = true) const;
    // what the kernels get of the index; it reads the search knobs and the calling thread's int32 switch (search_dev_i32), so
    // it is defined beside them in sbwtgpu_capi.cpp
    SbwtIndexView view() const;
};

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

namespace sbwt_capi {

// ---- what one file defines for the others ----------------------------------------------------------------------
// sbwtgpu_capi.cpp: the search of a batch on the device (int64 results; _i32: int32 results, for an index below 2^31 columns),
// and the host half of the device builder (S is released whatever the result)
int search_dev_common(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases, const int64_t *d_read_off, int64_t n_reads,
                      int64_t *d_out, const int64_t *d_out_off, void *d_ws, int64_t ws_bytes, void *stream, int streaming);
int search_dev_i32(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases, const int64_t *d_read_off, int64_t n_reads,
                   int32_t *d_out, const int64_t *d_out_off, void *d_ws, int64_t ws_bytes, void *stream, int streaming);
int build_columns(SbwtBuildState &S, int64_t k, int build_streaming_support, sbwtgpu_plain_matrix_bits *out);
// sbwtgpu_capi_reads.cpp
int unitigs_create_common(const sbwtgpu_index *idx, const unsigned *d_ids, const unsigned long long *d_table, int words, int64_t n_sets,
                          int n_colors, unsigned graph, sbwtgpu_unitigs **out);
int setop_check_index(const sbwtgpu_index *idx, const char *who);
// sbwtgpu_capi_colors.cpp
int colorsets_check(const sbwtgpu_colorsets *s);
// The searches of a batch and, for two strands, of its mirrored batch, int32 results, in a workspace of
// sbwtgpu_pseudoalign_workspace_bytes: what the calls over colours and the genotype adds put in front of their own kernel.
// enqueued: false for a batch of no reads, where nothing was launched.  hdr: the workspace's SbwtPaHeader, whose first word
// is the searches' status, at byte hdr_off.
struct StrandSearch {
    const int *res = nullptr, *res2 = nullptr;
    const long long *ooff = nullptr;
    void *hdr = nullptr;
    int64_t hdr_off = 0;
    bool enqueued = false;
};
int search_strands_dev(const sbwtgpu_index *idx, const char *d_bases, int64_t total_bases, const int64_t *d_read_off, int64_t n_reads,
                       int strands, void *d_ws, int64_t ws_bytes, void *stream, StrandSearch &out);

// sbwtgpu_capi_verify.cpp, for the align calls (sbwtgpu_capi_align.cpp): what a verify call asks of its arguments, the bytes of
// its workspace, and what the kernels get of a reference object (d_tab: its SbwtRefSeq entries)
struct RefSeqsView {
    int device;
    const void *d_tab;
    int64_t n_seqs;
    const unsigned long long *d_bits, *d_valid;
};
int check_verify(const sbwtgpu_refseqs *r, int64_t n_reads, int band);
int64_t verify_workspace_bytes(int64_t n_reads);
RefSeqsView refseqs_view(const sbwtgpu_refseqs *r);

// The length of read r as every host entry point checks it while it walks the offsets: not negative, below 2^31
inline int check_read_length(const int64_t *read_off, int64_t r) {
    const int64_t len = read_off[r + 1] - read_off[r];
    if (len < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "read_off is not non-decreasing at read %lld", (long long)r);
    if (len >= ((int64_t)1 << 31)) return fail(SBWTGPU_ERR_READ_TOO_LONG, "read %lld has >= 2^31 bases", (long long)r);
    return SBWTGPU_OK;
}

// What every call over reads on one or two strands asks of `strands` and `n_reads`.  who: what the layer's texts begin with
// ("positions: ", "genotype: "; "" for the colour layer, whose texts carry no name)
inline int check_strands_batch(const char *who, int64_t n_reads, int strands) {
    if (strands != 1 && strands != 2)
        return fail(SBWTGPU_ERR_INVALID_ARG, "%sstrands must be 1 (forward) or 2 (either strand), not %d", who, strands);
    if (n_reads < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "%snegative n_reads", who);
    if (n_reads >= ((int64_t)1 << 31)) return fail(SBWTGPU_ERR_INVALID_ARG, "%s2^31 reads or more in one call: split the batch", who);
    return SBWTGPU_OK;
}

// What a device-pointer entry point over a batch of reads asks of its sizes and its workspace (need: the bytes its
// *_workspace_bytes call names for the batch).  check_batch_sizes is the first half, for a caller with a check in between.
inline int check_batch_sizes(int64_t n_reads, int64_t total_bases) {
    if (n_reads < 0 || total_bases < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "negative size");
    if (total_bases >= ((int64_t)1 << 36))
        return fail(SBWTGPU_ERR_INVALID_ARG, "more than 2^36 bases in one call: split the batch");
    return SBWTGPU_OK;
}
inline int check_batch_dev(int64_t n_reads, int64_t total_bases, const void *d_ws, int64_t ws_bytes, int64_t need) {
    STG_TRY(check_batch_sizes(n_reads, total_bases));
    if (!d_ws || ws_bytes < need)
        return fail(SBWTGPU_ERR_INVALID_ARG, "workspace missing or too small (%lld < %lld)", (long long)ws_bytes, (long long)need);
    if (((uintptr_t)d_ws & 15) != 0) return fail(SBWTGPU_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
    return SBWTGPU_OK;
}

// ---- small host-buffer calls: one staged range ------------------------------------------------------------------
// Small calls (the scalar API of the reference -- SBWT::search(kmer), rank(pos, c), one update_sbwt_interval -- arrives
// here as batches of one): no hipMalloc / hipStreamCreate per call.  Every host thread keeps, per device, one stream,
// one pinned host buffer and one device buffer of SLOT_CAP bytes; a call whose data fits stages its inputs in the pinned
// buffer, moves them with ONE H2D copy, runs its kernels, and brings the results back with ONE D2H copy + one sync.
constexpr size_t SLOT_CAP = (size_t)1 << 20;
struct SmallSlot {
    int device = -1;
    hipStream_t stream = nullptr;
    char *host = nullptr, *dev = nullptr;
    void release();
};
// The calling thread's slot on `device` (the current device must already be `device`), or nullptr when `need` does not
// fit or the buffers cannot be allocated (the caller then takes the general path).
SmallSlot *small_slot(int device, size_t need);

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

// ---- large host batches: chunks pipelined over two streams -------------------------------------------------------
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
// n slots for a call on `device` (the current device), each grown to the call's needs: parked ones first, the most
// recently parked first.  On failure nothing is left allocated.
int take_slots(int device, PipeSlot *S, int n, int64_t need_in, int64_t need_out, int64_t need_dev, const char *what);
// The end of a call on its slots: parked for the next one, or, after an error, freed once the device is idle.
void park_slots(int device, PipeSlot *S, int n, int rc);
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
bool is_pinned(const void *p);
void parallel_memcpy(char *dst, const char *src, size_t n);

// The cut of a batch for a chunked call (sbwt_read_chunks.h), with the error of a refused read
inline int cut_reads(const int64_t *read_off, int64_t n_reads, int64_t budget, int64_t max_chunk_reads, int64_t k, SbwtReadChunks &ch) {
    ch = sbwt_cut_read_chunks(read_off, n_reads, budget, max_chunk_reads, k);
    if (ch.bad == SbwtReadChunks::NO_MEMORY) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    return ch.bad ? check_read_length(read_off, ch.bad_read) : SBWTGPU_OK;
}

// A host-buffer call over reads, chunk by chunk on parked slots.  A slot's device memory is [bases + 16][read_off rebased to
// 0][the caller's regions, in the order declared][workspace], every part 256-byte aligned; bases and offsets go down through
// h_in, the regions that come back through h_out.  The caller declares its regions, opens, and then either runs a body per
// chunk with two chunks in flight (run), or stages chunk after chunk itself (stage, fetch, finish: the walks).
struct ReadPipe {
    // bytes 0: the region is absent.  back: it has room in h_out, at h_off.  dst: chunk results go there, `stride` bytes per
    // read, copied by fetch() and collect(); direct: dst is pinned and is the DMA's target itself (no room in h_out, no
    // memcpy).  A region that comes back without a dst is the caller's to fetch: fetch_region() (the walks' step offsets).
    struct Region { int64_t bytes; bool back; char *dst; int64_t stride; bool direct; int64_t off, h_off; };
    struct Chunk {
        PipeSlot *P;
        int64_t lo, nr, nb;             // first read, reads, bases
        const char *bases;              // device
        const int64_t *roff;
        char *ws;
    };
    const char *bases;
    const int64_t *read_off;
    const SbwtReadChunks &ch;
    Region reg[4];
    int n_reg = 0, n_slots = 0, device = 0;
    bool pin_in = false;
    PipeSlot S[2];
    int64_t o_roff = 0, o_ws = 0, ws_bytes = 0;
    int bug = 0;                        // the first nonzero device status of a chunk

    ReadPipe(const char *bases_, const int64_t *read_off_, const SbwtReadChunks &ch_) : bases(bases_), read_off(read_off_), ch(ch_) {}
    int region(int64_t bytes, bool back = false, void *dst = nullptr, int64_t stride = 0, bool direct = false) {
        assert(n_reg < (int)(sizeof(reg) / sizeof(reg[0])) && (dst == nullptr || back));
        reg[n_reg] = Region{bytes, back, static_cast<char *>(dst), stride, direct, 0, 0};
        return n_reg++;
    }
    template <typename T>
    T *at(const Chunk &c, int r) const { return reinterpret_cast<T *>(c.P->d_mem + reg[r].off); }
    // lays the slots out for chunks of at most (ch.max_bases, ch.max_reads) with a workspace of ws_bytes_, and takes n of them
    int open(int device_, int64_t ws_bytes_, int n, const char *what) {
        device = device_; ws_bytes = ws_bytes_; n_slots = n;
        pin_in = is_pinned(bases);
        o_roff = align256(ch.max_bases + 16);
        int64_t off = o_roff + align256((ch.max_reads + 1) * 8), need_out = 0;
        const int64_t need_in = off;
        for (int r = 0; r < n_reg; r++) {
            reg[r].off = off; off += align256(reg[r].bytes);
            reg[r].h_off = need_out; if (reg[r].back && !reg[r].direct) need_out += align256(reg[r].bytes);
        }
        o_ws = off;
        return take_slots(device, S, n_slots, need_in, need_out, o_ws + align256(ws_bytes), what);
    }
    // chunk c's bases (as they are if pinned, else through h_in) and rebased offsets on their way to its slot
    int stage(int64_t c, Chunk &k) {
        PipeSlot &P = S[c % n_slots];
        const int64_t lo = ch.cuts[(size_t)c], nr = ch.cuts[(size_t)c + 1] - lo, nb = read_off[lo + nr] - read_off[lo];
        int64_t *hro = (int64_t *)(P.h_in + o_roff);
        for (int64_t r = 0; r <= nr; r++) hro[r] = read_off[lo + r] - read_off[lo];
        const char *hb = bases + read_off[lo];
        if (!pin_in && nb > 0) { parallel_memcpy(P.h_in, hb, (size_t)nb); hb = P.h_in; }
        hipError_t e;
        if ((nb > 0 && (e = hipMemcpyAsync(P.d_mem, hb, (size_t)nb, hipMemcpyHostToDevice, P.st)) != hipSuccess) ||
            (e = hipMemcpyAsync(P.d_mem + o_roff, hro, (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, P.st)) != hipSuccess)
            return fail(SBWTGPU_ERR_HIP, "H2D copy: %s", hipGetErrorString(e));
        k = Chunk{&P, lo, nr, nb, P.d_mem, (const int64_t *)(P.d_mem + o_roff), P.d_mem + o_ws};
        return SBWTGPU_OK;
    }
    // the first `bytes` bytes of region r on their way to its place in the slot's h_out; the pointer to read them at after the
    // caller's synchronise
    const char *fetch_region(const Chunk &k, int r, int64_t bytes) {
        assert(reg[r].back && !reg[r].direct && bytes <= reg[r].bytes);
        const hipError_t e = hipMemcpyAsync(k.P->h_out + reg[r].h_off, k.P->d_mem + reg[r].off, (size_t)bytes, hipMemcpyDeviceToHost, k.P->st);
        if (e != hipSuccess) { fail(SBWTGPU_ERR_HIP, "D2H copy: %s", hipGetErrorString(e)); return nullptr; }
        return k.P->h_out + reg[r].h_off;
    }
    // after the chunk's kernels: its results towards their dst, and status_bytes at d_status into the slot's h_status
    int fetch(const Chunk &k, const void *d_status, size_t status_bytes) {
        hipError_t e = hipSuccess;
        for (int r = 0; r < n_reg && e == hipSuccess; r++) {
            const Region &g = reg[r];
            if (g.dst && k.nr * g.stride > 0)
                e = hipMemcpyAsync(g.direct ? g.dst + k.lo * g.stride : k.P->h_out + g.h_off, k.P->d_mem + g.off, (size_t)(k.nr * g.stride),
                                   hipMemcpyDeviceToHost, k.P->st);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(k.P->h_status, d_status, status_bytes, hipMemcpyDeviceToHost, k.P->st);
        if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "D2H copy: %s", hipGetErrorString(e));
        return SBWTGPU_OK;
    }
    void note_status(const PipeSlot &P) {
        if (P.h_status[0] != 0 && bug == 0) bug = P.h_status[0];
    }
    // waits for chunk c and hands its results to the caller; its slot's h_status holds what fetch() asked for
    int collect(int64_t c) {
        PipeSlot &P = S[c % n_slots];
        const hipError_t e = hipStreamSynchronize(P.st);
        if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "stream synchronize: %s", hipGetErrorString(e));
        note_status(P);
        const int64_t lo = ch.cuts[(size_t)c], nr = ch.cuts[(size_t)c + 1] - lo;
        for (int r = 0; r < n_reg; r++)
            if (reg[r].dst && !reg[r].direct && nr * reg[r].stride > 0)
                memcpy(reg[r].dst + lo * reg[r].stride, P.h_out + reg[r].h_off, (size_t)(nr * reg[r].stride));
        return SBWTGPU_OK;
    }
    // the end of the call: the slots parked (freed after an error), a chunk's device status as the result
    int finish(int rc) {
        park_slots(device, S, n_slots, rc);
        if (rc != SBWTGPU_OK) return rc;
        return bug ? fail_status(bug) : SBWTGPU_OK;
    }
    // body(chunk): the chunk's device call and its fetch(); collected(slot): after a chunk's results have arrived
    template <typename Body, typename Collected>
    int run(Body body, Collected collected) {
        return finish(two_in_flight(
            ch.n_chunks(),
            [&](int64_t c) -> int { Chunk k; STG_TRY(stage(c, k)); return body(k); },
            [&](int64_t c) -> int { STG_TRY(collect(c)); collected(S[c % n_slots]); return SBWTGPU_OK; }));
    }
    template <typename Body>
    int run(Body body) { return run(body, [](const PipeSlot &) {}); }
};

}  // namespace sbwt_capi

#pragma GCC visibility pop
