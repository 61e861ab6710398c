"""Read-hits benchmark: per-read hit profiles (sbwtgpu_read_hits_dev / _batch) against the per-k-mer calls they replace, on
bench.py's config 2 index and reads (the same synth calls and seeds, bench.gpu_reads for the reads), in ONE process.  Prints
one JSON line:

  device   read_hits_dev with one and with two strands, and streaming_search_dev_i32 on the same batch: device events around
           each call, median of --steps
  host     read_hits_batch (one and two strands) and sbwtgpu_streaming_search_batch_i32 from pageable host buffers on the
           same batch of --host-reads reads: host clock around the (synchronous) call, median of --host-steps

  python tools/read_hits_bench.py [--reads N] [--host-reads N] [--steps 7] [--warmup 2]
Kernel names and times: run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/read_hits_bench.py ...`."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--host-reads", type=int, default=2_000_000)
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--host-steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import bench
    from sbwt_amd import capi, synth

    k = 30
    genomes = synth.coli3_like(args.genome_len)
    dev = torch.device("cuda", 0)
    bits = capi.build_bits_gpu([g.tobytes() for g in genomes], k, False, True, device=0)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)
    del bits
    stream = torch.cuda.current_stream(dev)
    n = args.reads
    L = bench.READ_LEN
    bases_t = bench.gpu_reads(genomes, n, 12345, dev)
    T = bases_t.numel()
    off_t = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    W = n * (L - k + 1)

    def timed(call):
        times = []
        for s in range(args.warmup + args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            if s >= args.warmup:
                times.append(e0.elapsed_time(e1))
        med = float(np.median(times))
        return {"median_ms": round(med, 3), "min_ms": round(min(times), 3), "calls": len(times),
                "G_kmers_per_s": round(W / med / 1e6, 2)}

    res = {"config": 2, "k": k, "n_nodes": idx.n_nodes, "image_level": idx.image_level, "reads": n, "read_len": L, "kmers": W}
    # ---- device buffers ----
    d_out = torch.empty(W, dtype=torch.int32, device=dev)
    d_ooff = torch.arange(n + 1, dtype=torch.int64, device=dev) * (L - k + 1)
    ws = torch.zeros(capi.search_workspace_bytes(T), dtype=torch.uint8, device=dev)
    dev_rows = {}
    dev_rows["streaming_search_dev_i32"] = timed(lambda: idx.streaming_search_dev_i32(
        bases_t.data_ptr(), T, off_t.data_ptr(), n, d_out.data_ptr(), d_ooff.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream))
    dev_rows["streaming_search_dev_i32"]["result_bytes"] = 4 * W
    found_search = int((d_out >= 0).sum().item())
    del ws, d_ooff
    rec = torch.empty((n, 4), dtype=torch.int32, device=dev)
    for both in (False, True):
        need = capi.read_hits_workspace_bytes(T, n, both)
        rws = torch.zeros(need, dtype=torch.uint8, device=dev)
        row = timed(lambda: idx.read_hits_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, rec.data_ptr(), rws.data_ptr(), need, both,
                                              stream.cuda_stream))
        row["result_bytes"] = 16 * n
        row["workspace_bytes"] = need
        row["n_found"] = int(rec[:, 1].sum(dtype=torch.int64).item())
        row["covered_bases"] = int(rec[:, 2].sum(dtype=torch.int64).item())
        row["mean_longest_run"] = round(float(rec[:, 3].double().mean().item()), 3)
        if not both and row["n_found"] != found_search:
            raise SystemExit("read_hits_dev found %d k-mers, the search %d" % (row["n_found"], found_search))
        dev_rows["read_hits_dev_strands%d" % (2 if both else 1)] = row
        del rws
    res["device"] = dev_rows
    res["device"]["read_hits_over_search"] = round(dev_rows["read_hits_dev_strands1"]["median_ms"] /
                                                   dev_rows["streaming_search_dev_i32"]["median_ms"], 3)
    res["device"]["found_matches_search"] = True
    del d_out, rec
    # ---- host buffers (pageable), the same batch for every call ----
    hn = min(args.host_reads, n)
    hb = bases_t[: hn * L].cpu().numpy()
    ho = np.arange(hn + 1, dtype=np.int64) * L
    hoo = np.arange(hn + 1, dtype=np.int64) * (L - k + 1)
    hW = hn * (L - k + 1)
    del bases_t
    torch.cuda.empty_cache()
    lib = capi.lib()
    out32 = np.empty(hW, dtype=np.int32)
    hrec = np.empty((hn, 4), dtype=np.int32)

    def host_timed(call):
        times = []
        for s in range(1 + args.host_steps):                   # (one warm-up call: the staging buffers are made then)
            t0 = time.perf_counter()
            capi._check(call())
            dt = (time.perf_counter() - t0) * 1e3
            if s >= 1:
                times.append(dt)
        med = float(np.median(times))
        return {"median_ms": round(med, 3), "min_ms": round(min(times), 3), "calls": len(times),
                "G_kmers_per_s": round(hW / med / 1e6, 2)}

    host_rows = {"reads": hn, "kmers": hW, "input_bytes": int(hb.nbytes)}
    host_rows["streaming_search_batch_i32"] = host_timed(lambda: lib.sbwtgpu_streaming_search_batch_i32(
        idx.handle, hb.ctypes.data, ho.ctypes.data, hn, out32.ctypes.data, hoo.ctypes.data))
    host_rows["streaming_search_batch_i32"]["result_bytes"] = 4 * hW
    hfound = int((out32 >= 0).sum())
    for both in (False, True):
        row = host_timed(lambda: lib.sbwtgpu_read_hits_batch(idx.handle, hb.ctypes.data, ho.ctypes.data, hn, 2 if both else 1,
                                                             hrec.ctypes.data))
        row["result_bytes"] = 16 * hn
        if not both and int(hrec[:, 1].sum(dtype=np.int64)) != hfound:
            raise SystemExit("read_hits_batch found %d k-mers, the search %d" % (int(hrec[:, 1].sum(dtype=np.int64)), hfound))
        host_rows["read_hits_batch_strands%d" % (2 if both else 1)] = row
    host_rows["read_hits_over_search"] = round(host_rows["read_hits_batch_strands1"]["median_ms"] /
                                               host_rows["streaming_search_batch_i32"]["median_ms"], 3)
    res["host"] = host_rows
    print(json.dumps(res))


if __name__ == "__main__":
    main()
