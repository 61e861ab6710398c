"""Pseudoalignment benchmark: the colour layer (sbwtgpu_pseudoalign_dev / _batch, sbwtgpu_colors_add_batch) beside the calls it
is built on, on bench.py's config 2 index with its strains as colours and bench.gpu_reads for the reads, in ONE process.
Prints one JSON line:

  device   pseudoalign_dev with one and with two strands, with and without counts; streaming_search_dev_i32 and read_hits_dev
           on the same batch as the comparison: device events around each call, median of --steps
  host     pseudoalign_batch from pageable host buffers on --host-reads reads, and colors_add_batch per strain: host clock
           around the (synchronous) call

  python tools/pseudoalign_bench.py [--reads N] [--host-reads N] [--steps 7] [--warmup 2]
Kernel names and times: run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/pseudoalign_bench.py ...`."""
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
    res = {"config": 2, "k": k, "n_nodes": idx.n_nodes, "image_level": idx.image_level, "n_colors": len(genomes)}

    # ---- colouring: one strain per colour, each genome one sequence ----
    col = capi.Colors.create(idx, len(genomes))
    add_rows = []
    for c, g in enumerate(genomes):
        off = np.array([0, len(g)], dtype=np.int64)
        t0 = time.perf_counter()
        nw, nh = col.add_sequences(c, g, off)
        dt = (time.perf_counter() - t0) * 1e3
        add_rows.append({"color": c, "ms": round(dt, 3), "n_windows": nw, "n_hit_windows": nh, "G_kmers_per_s": round(nw / dt / 1e6, 3)})
    info = col.info()
    res["colors_add_batch"] = add_rows
    res["colored_columns"] = info["n_colored_columns"]
    res["per_color"] = info["per_color"]
    res["rows_bytes"] = 8 * idx.n_nodes

    stream = torch.cuda.current_stream(dev)
    n = args.reads
    L = bench.READ_LEN
    bases_t = bench.gpu_reads(genomes, n, 12345, dev)
    T = bases_t.numel()
    off_t = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    W = n * (L - k + 1)
    res.update({"reads": n, "read_len": L, "kmers": W})

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

    # ---- device buffers: the comparison calls first ----
    dev_rows = {}
    d_out = torch.empty(W, dtype=torch.int32, device=dev)
    d_ooff = torch.arange(n + 1, dtype=torch.int64, device=dev) * (L - k + 1)
    ws = torch.zeros(capi.search_workspace_bytes(T), dtype=torch.uint8, device=dev)
    dev_rows["streaming_search_dev_i32"] = timed(lambda: idx.streaming_search_dev_i32(
        bases_t.data_ptr(), T, off_t.data_ptr(), n, d_out.data_ptr(), d_ooff.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream))
    found_search = int((d_out >= 0).sum().item())
    del ws, d_ooff, d_out
    rec4 = torch.empty((n, 4), dtype=torch.int32, device=dev)
    need = capi.read_hits_workspace_bytes(T, n, False)
    rws = torch.zeros(need, dtype=torch.uint8, device=dev)
    dev_rows["read_hits_dev"] = timed(lambda: idx.read_hits_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, rec4.data_ptr(), rws.data_ptr(),
                                                                need, False, stream.cuda_stream))
    del rws, rec4
    rec = torch.empty((n, 2), dtype=torch.int64, device=dev)
    cnt = torch.empty((n, len(genomes)), dtype=torch.int32, device=dev)
    for both in (False, True):
        need = capi.pseudoalign_workspace_bytes(T, n, both)
        pws = torch.zeros(need, dtype=torch.uint8, device=dev)
        for counts in (False, True):
            row = timed(lambda: col.pseudoalign_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, rec.data_ptr(), cnt.data_ptr() if counts else 0,
                                                    pws.data_ptr(), need, both, 1_000_000, 0, stream.cuda_stream))
            row["result_bytes"] = 16 * n + (4 * len(genomes) * n if counts else 0)
            row["workspace_bytes"] = need
            h = rec.cpu().numpy().view(capi.PSEUDOALIGNMENT_DTYPE).reshape(n)
            row["n_found"] = int(h["n_found"].sum(dtype=np.int64))
            row["reads_by_colors"] = {str(v): int(c) for v, c in zip(*np.unique(h["colors"], return_counts=True))}
            if not both and row["n_found"] != found_search:
                raise SystemExit("pseudoalign_dev found %d k-mers, the search %d" % (row["n_found"], found_search))
            dev_rows["pseudoalign_dev_strands%d%s" % (2 if both else 1, "_counts" if counts else "")] = row
        del pws
    s_ms, r_ms = dev_rows["streaming_search_dev_i32"]["median_ms"], dev_rows["read_hits_dev"]["median_ms"]
    p_ms = dev_rows["pseudoalign_dev_strands1"]["median_ms"]
    dev_rows["pseudoalign_over_search"] = round(p_ms / s_ms, 3)
    dev_rows["pseudoalign_over_read_hits"] = round(p_ms / r_ms, 3)
    dev_rows["reduce_ms_estimate"] = round(p_ms - s_ms, 3)
    dev_rows["found_matches_search"] = True
    res["device"] = dev_rows
    del rec, cnt
    # ---- host buffers (pageable) ----
    hn = min(args.host_reads, n)
    hb = bases_t[: hn * L].cpu().numpy()
    ho = np.arange(hn + 1, dtype=np.int64) * L
    hW = hn * (L - k + 1)
    del bases_t
    torch.cuda.empty_cache()
    times = []
    for s in range(1 + args.host_steps):                   # (one warm-up call: the staging buffers are made then)
        t0 = time.perf_counter()
        hrec = col.pseudoalign(hb, ho)
        dt = (time.perf_counter() - t0) * 1e3
        if s >= 1:
            times.append(dt)
    med = float(np.median(times))
    res["host"] = {"reads": hn, "kmers": hW, "input_bytes": int(hb.nbytes),
                   "pseudoalign_batch": {"median_ms": round(med, 3), "min_ms": round(min(times), 3), "calls": len(times),
                                         "G_kmers_per_s": round(hW / med / 1e6, 2), "result_bytes": 16 * hn,
                                         "n_found": int(hrec["n_found"].sum(dtype=np.int64))}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
