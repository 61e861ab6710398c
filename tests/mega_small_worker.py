"""Child process of tests/test_gpu_mega_small.py (not a test module: pytest does not collect it).

    SBWTGPU_LIB=sbwt_amd/lib/libsbwtgpu_mega12.so python tests/mega_small_worker.py in.npz out.npz

It loads the TEST build of the GPU library (mega blocks of 2^12 columns, sbwt_amd/build.py), proves from the version string
that it did, and then only calls that library on the inputs of in.npz and stores the raw outputs in out.npz.  It computes no
expectation and compares nothing: the parent has the oracle and does all of that.  A fresh process because capi.py binds one
library per process, and the parent's is the product build.

in.npz: "meta" (JSON) and arrays.  meta["mode"] is "sbwt" (one index, one image per entry of meta["configs"]) or "rank_only"
(arbitrary bit vectors, rank alone).  Output keys are "<config>/<what>".  Any error ends the process with a traceback and a
non-zero status; nothing further is started on the GPU then."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GUARD = 64          # slots behind a device result array that must keep their fill
FILL = 77


def search_entry_points(capi, torch, idx, bases, off, streaming):
    """One batch through the four entry points: host int64 / int32, device int64 / int32 (with guard slots)."""
    dev = torch.device("cuda", 0)
    res = {}
    res["h64"] = (idx.streaming_search if streaming else idx.search)(bases, off)[0]
    res["h32"] = idx.search_i32(bases, off, bool(streaming))[0]
    ooff = capi.out_offsets(off, idx.k)
    n_out = int(ooff[-1])
    d_b, d_ro, d_oo = torch.from_numpy(bases).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(ooff).to(dev)
    wsb = capi.search_workspace_bytes(d_b.numel())
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    d64 = torch.full((n_out + GUARD,), FILL, dtype=torch.int64, device=dev)
    idx.streaming_search_dev(d_b.data_ptr(), d_b.numel(), d_ro.data_ptr(), len(off) - 1, d64.data_ptr(), d_oo.data_ptr(),
                             d_ws.data_ptr(), wsb, st, bool(streaming))
    d32 = torch.full((n_out + GUARD,), FILL, dtype=torch.int32, device=dev)
    idx.streaming_search_dev_i32(d_b.data_ptr(), d_b.numel(), d_ro.data_ptr(), len(off) - 1, d32.data_ptr(), d_oo.data_ptr(),
                                 d_ws.data_ptr(), wsb, st, bool(streaming))
    torch.cuda.synchronize()
    res["d64"] = d64.cpu().numpy()
    res["d32"] = d32.cpu().numpy()
    return res


def run_config(capi, torch, z, meta, cfg, out):
    name = cfg["name"]
    do = set(cfg["do"])
    for key, val in cfg.get("tunings", []):
        capi.set_tuning(key, val)
    try:
        idx = capi.Index.create(z["A"], z["C"], z["G"], z["T"], z["ssup"] if "ssup" in z.files else None, meta["n_nodes"],
                                meta["k"], meta["n_kmers"], meta["precalc_k"], None)
    finally:
        for key, val in cfg.get("restore", []):
            capi.set_tuning(key, val)
    out[name + "/info"] = np.array(json.dumps(dict(
        n_nodes=idx.n_nodes, C=idx.C, image_level=idx.image_level, n_paths=idx.n_paths, blob_bytes=idx.blob_bytes,
        default_search_variant=idx.default_search_variant, has_streaming_support=idx.has_streaming_support,
        precalc_k=idx.precalc_k)))
    if "rank" in do:
        out[name + "/rank"] = idx.rank(z["rank_pos"], z["rank_sym"])
    if "select" in do:
        out[name + "/select"] = idx.select(z["sel_j"], z["sel_sym"])
        rcs = []
        for j, s in zip(z["sel_bad_j"], z["sel_bad_sym"]):
            try:
                idx.select(np.array([j]), np.array([s], dtype=np.uint8))
                rcs.append(0)
            except capi.SbwtGpuError as e:
                rcs.append(e.code)
        out[name + "/select_bad_rc"] = np.array(rcs, dtype=np.int64)
    if "kmers" in do:
        out[name + "/kmers"] = idx.get_kmers(np.arange(idx.n_nodes, dtype=np.int64))
    if "forward" in do:
        out[name + "/forward"] = idx.forward(z["fwd_node"], z["fwd_sym"])
    if "update_interval" in do:
        f, s = idx.update_interval(z["ui_bases"], z["ui_off"], z["ui_first"], z["ui_second"])
        out[name + "/ui_first"], out[name + "/ui_second"] = f, s
    if "partial" in do:
        f, s, m = idx.partial_search(z["ps_bases"], z["ps_off"])
        out[name + "/ps_first"], out[name + "/ps_second"], out[name + "/ps_matched"] = f, s, m
    if "precalc" in do:
        out[name + "/precalc"] = idx.get_precalc()
    if "search" in do:
        capi.set_tuning("poison_results", 1)
        for b in range(meta["n_batches"]):
            bases, off = z["sb%d_bases" % b], z["sb%d_off" % b]
            for variant in cfg["variants"]:
                capi.set_tuning("search_variant", variant)
                try:
                    for streaming in cfg["streaming"]:
                        for ep, arr in search_entry_points(capi, torch, idx, bases, off, streaming).items():
                            out["%s/search/b%d/v%d/s%d/%s" % (name, b, variant, streaming, ep)] = arr
                finally:
                    capi.set_tuning("search_variant", -1)
    if "ms" in do:
        out[name + "/lcs"] = idx.lcs()
        ln, f, s = idx.matching_statistics(z["ms_bases"], z["ms_off"])
        out[name + "/ms_len"], out[name + "/ms_first"], out[name + "/ms_second"] = ln, f, s
        out[name + "/ms_len_only"] = idx.matching_statistics(z["ms_bases"], z["ms_off"], intervals=False)
    if "adopt" in do:
        hdr = idx.export_header()
        nb = idx.blob_bytes
        t = torch.empty(nb, dtype=torch.uint8, device=torch.device("cuda", 0))
        idx.copy_blob(t.data_ptr(), nb, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        rep = capi.Index.adopt(hdr, t.data_ptr(), nb, 0, keepalive=t)
        out[name + "/header"] = np.frombuffer(hdr, dtype=np.uint8).copy()
        bases, off = z["sb0_bases"], z["sb0_off"]
        for streaming in cfg["streaming"]:
            out["%s/adopt/s%d" % (name, streaming)] = (rep.streaming_search if streaming else rep.search)(bases, off)[0]
        out[name + "/adopt/rank"] = rep.rank(z["rank_pos"], z["rank_sym"])
        rep.close()
    idx.close()


def run_rank_only(capi, z, meta, out):
    for i, n_bits in enumerate(meta["sizes"]):
        idx = capi.Index.create(z["r%d_A" % i], z["r%d_C" % i], z["r%d_G" % i], z["r%d_T" % i], None, n_bits, 1, 0, 0)
        for j in range(meta["n_batches"]):
            out["r%d_out%d" % (i, j)] = idx.rank(z["r%d_pos%d" % (i, j)], z["r%d_sym%d" % (i, j)])
        idx.close()


def main(inp, outp):
    from sbwt_amd import capi
    z = np.load(inp, allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    version = capi.lib().sbwtgpu_version().decode()
    if meta["marker"] not in version:
        sys.exit("mega_small_worker: loaded %s, whose version is %r: no %r in it -- not the test build (SBWTGPU_LIB=%s)"
                 % (capi.LIB_PATH, version, meta["marker"], os.environ.get("SBWTGPU_LIB")))
    if capi.device_count() <= 0:
        sys.exit("mega_small_worker: no HIP device visible")
    out = {"version": np.array(version)}
    if meta["mode"] == "rank_only":
        run_rank_only(capi, z, meta, out)
    else:
        import torch
        for cfg in meta["configs"]:
            run_config(capi, torch, z, meta, cfg, out)
    np.savez(outp, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
