// sbwtgpu_capi_align.cpp -- the C ABI's alignment layer: from reads, their map records and the packed reference sequences to
// the begin of each read's best alignment and its runs of = X I D (sbwt_align.hip).  The forward pass is
// the verify call's, unchanged.  What it shares with the other files: sbwtgpu_internal.h.
#include "sbwtgpu_internal.h"
#include "sbwt_align.h"

#include <cstdlib>

using namespace sbwt_capi;

// knob of this file (sbwtgpu_set_tuning sets it)
int sbwt_capi::g_align_fast_edit = 0;         // "align_fast_edit": 0 = the compiled SBWT_AL_FAST_EDIT

static_assert(sizeof(sbwtgpu_read_align) == sizeof(SbwtReadAlign), "the record of the ABI is the kernels' record");

// [the verify workspace][what sbwt_align_layout names]
static int64_t align_workspace_bytes(int64_t n_reads) { return verify_workspace_bytes(n_reads) + sbwt_align_layout(n_reads).bytes; }

extern "C" {

int64_t sbwtgpu_align_workspace_bytes(int64_t total_bases, int64_t n_reads) {
    (void)total_bases;              // (nothing per base: the waves' scratch is a fixed grid's)
    return align_workspace_bytes(n_reads);
}

int sbwtgpu_align_dev(const sbwtgpu_refseqs *r, const char *d_bases, int64_t total_bases, const int64_t *d_read_off, int64_t n_reads,
                      const sbwtgpu_read_map *d_map, int band, sbwtgpu_read_verify *d_verify_out, sbwtgpu_read_align *d_out,
                      int64_t *d_op_off, uint32_t *d_ops, int64_t ops_cap, void *d_ws, int64_t ws_bytes, void *stream) {
    STG_TRY(check_verify(r, n_reads, band));
    if (ops_cap < 0) return fail(SBWTGPU_ERR_INVALID_ARG, "align: negative ops_cap");
    STG_TRY(check_batch_dev(n_reads, total_bases, d_ws, ws_bytes, align_workspace_bytes(n_reads)));
    if (!d_op_off) return fail(SBWTGPU_ERR_INVALID_ARG, "align: NULL device pointer (d_op_off)");
    if (ops_cap > 0 && !d_ops) return fail(SBWTGPU_ERR_INVALID_ARG, "align: NULL device pointer (d_ops with ops_cap > 0)");
    if (n_reads > 0 && (!d_verify_out || !d_out))
        return fail(SBWTGPU_ERR_INVALID_ARG, "align: NULL device pointer (d_verify_out and d_out are needed)");
    const int64_t vws = verify_workspace_bytes(n_reads);
    STG_TRY(sbwtgpu_refseqs_verify_dev(r, d_bases, total_bases, d_read_off, n_reads, d_map, band, d_verify_out, d_ws, vws, stream));
    const RefSeqsView v = refseqs_view(r);
    DeviceGuard guard(v.device);
    sbwt_launch_align(d_bases, total_bases, reinterpret_cast<const long long *>(d_read_off), n_reads,
                      reinterpret_cast<const SbwtVerifyMap *>(d_map), static_cast<const SbwtRefSeq *>(v.d_tab), v.d_bits, v.d_valid, band,
                      g_align_fast_edit, reinterpret_cast<const SbwtReadVerify *>(d_verify_out), reinterpret_cast<SbwtReadAlign *>(d_out),
                      reinterpret_cast<long long *>(d_op_off), d_ops, ops_cap, static_cast<char *>(d_ws) + vws,
                      static_cast<hipStream_t>(stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SBWTGPU_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
    return SBWTGPU_OK;
}

// One staged range, as sbwtgpu_refseqs_verify_batch.  The runs' total is known only after the call, so the range has room for
// the most there can be: a read of L bases has at most 2 L runs (every run holds a column, and a D run stands between two
// others).  The runs come back in a copy of their own once the offsets have.
int sbwtgpu_align_batch(const sbwtgpu_refseqs *r, const char *bases, const int64_t *read_off, int64_t n_reads, const sbwtgpu_read_map *map,
                        int band, sbwtgpu_read_verify *verify_out, sbwtgpu_read_align *out, int64_t *op_off, uint32_t **ops_out,
                        int64_t *n_ops) {
    STG_TRY(check_verify(r, n_reads, band));
    if (!op_off || !ops_out || !n_ops) return fail(SBWTGPU_ERR_INVALID_ARG, "align: NULL argument (op_off, ops_out and n_ops are needed)");
    *ops_out = nullptr;
    *n_ops = 0;
    op_off[0] = 0;
    if (n_reads == 0) return SBWTGPU_OK;
    if (!read_off || !map || !verify_out || !out)
        return fail(SBWTGPU_ERR_INVALID_ARG, "align: NULL argument (read_off, map, verify_out and out are needed)");
    const int64_t nb = read_off[n_reads] - read_off[0];
    if (nb > 0 && !bases) return fail(SBWTGPU_ERR_INVALID_ARG, "align: NULL argument (bases)");
    for (int64_t i = 0; i < n_reads; i++) STG_TRY(check_read_length(read_off, i));
    STG_TRY(check_batch_sizes(n_reads, nb));
    const int64_t ws_bytes = align_workspace_bytes(n_reads), ops_cap = 2 * nb;
    const size_t o_off = (size_t)align256(nb + 16), o_map = o_off + (size_t)align256((n_reads + 1) * 8),
                 o_ver = o_map + (size_t)align256(n_reads * (int64_t)sizeof(sbwtgpu_read_map)),
                 o_out = o_ver + (size_t)align256(n_reads * (int64_t)sizeof(sbwtgpu_read_verify)),
                 o_ooff = o_out + (size_t)align256(n_reads * (int64_t)sizeof(sbwtgpu_read_align)),
                 o_ops = o_ooff + (size_t)align256((n_reads + 1) * 8), o_ws = o_ops + (size_t)align256(ops_cap * 4 + 16);
    const RefSeqsView v = refseqs_view(r);
    DeviceGuard guard(v.device);
    Staging g;
    STG_TRY(g.open(v.device, o_ws + (size_t)ws_bytes));
    STG_TRY(g.in(0, bases + read_off[0], (size_t)nb));
    STG_TRY(g.in_rebased(o_off, read_off, n_reads + 1));
    STG_TRY(g.in(o_map, map, (size_t)n_reads * sizeof(sbwtgpu_read_map)));
    STG_TRY(g.upload());
    STG_TRY(sbwtgpu_align_dev(r, g.at<char>(0), nb, g.at<int64_t>(o_off), n_reads, g.at<sbwtgpu_read_map>(o_map), band,
                              g.at<sbwtgpu_read_verify>(o_ver), g.at<sbwtgpu_read_align>(o_out), g.at<int64_t>(o_ooff), g.at<uint32_t>(o_ops),
                              ops_cap, g.at<char>(o_ws), ws_bytes, g.stream));
    STG_TRY(g.out(o_ver, verify_out, (size_t)n_reads * sizeof(sbwtgpu_read_verify)));
    STG_TRY(g.out(o_out, out, (size_t)n_reads * sizeof(sbwtgpu_read_align)));
    STG_TRY(g.out(o_ooff, op_off, (size_t)(n_reads + 1) * 8));
    STG_TRY(g.finish());
    const int64_t total = op_off[n_reads];
    if (total < 0 || total > ops_cap) return fail(SBWTGPU_ERR_HIP, "internal: %lld runs for %lld bases", (long long)total, (long long)nb);
    if (total == 0) return SBWTGPU_OK;
    uint32_t *ops = static_cast<uint32_t *>(malloc((size_t)total * 4));
    if (!ops) return fail(SBWTGPU_ERR_OOM, "out of host memory");
    hipError_t e = hipMemcpyAsync(ops, g.at<uint32_t>(o_ops), (size_t)total * 4, hipMemcpyDeviceToHost, g.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (e != hipSuccess) {
        free(ops);
        return fail(SBWTGPU_ERR_HIP, "D2H copy: %s", hipGetErrorString(e));
    }
    *ops_out = ops;
    *n_ops = total;
    return SBWTGPU_OK;
}

}  // extern "C"
