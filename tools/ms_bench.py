"""Matching-statistics benchmark (sbwtgpu_matching_statistics_dev): builds bench.py's config 2, 3 or 5 index (the same synth
calls and seeds, bench.gpu_reads for the reads) and prints one JSON line: LCS build time, median kernel time of device-event
timed calls, G positions/s with and without intervals, the fraction of positions with len == k, contractions per base, a
bytes-per-position model, and rows for all-random reads and for 10 x 1 Mbp reads.

  python tools/ms_bench.py --config 2 [--reads N] [--steps 7] [--warmup 2]
Kernel names and times: run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/ms_bench.py ...`."""
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
    ap.add_argument("--config", type=int, default=2, choices=[2, 3, 5])
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--derived", type=int, default=64)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import bench
    from sbwt_amd import capi, synth

    k, streaming = 30, True
    if args.config == 3:
        k = 31
    elif args.config == 5:
        k, streaming = 63, False
    genomes = synth.pan_like(args.derived, args.genome_len) if args.config == 3 else synth.coli3_like(args.genome_len)
    dev = torch.device("cuda", 0)
    bits = capi.build_bits_gpu([g.tobytes() for g in genomes], k, False, streaming, device=0)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)
    del bits
    torch.cuda.synchronize(dev)
    t0 = time.time()
    idx.build_lcs()
    t_lcs = time.time() - t0
    lcs = idx.lcs()
    stream = torch.cuda.current_stream(dev)

    def run(bases_t, off_t, intervals, steps, warmup):
        n = bases_t.numel()
        dl = torch.empty(n, dtype=torch.uint8, device=dev)
        df = torch.empty(n if intervals else 0, dtype=torch.int64, device=dev)
        ds = torch.empty(n if intervals else 0, dtype=torch.int64, device=dev)
        ws = torch.zeros(capi.ms_workspace_bytes(n), dtype=torch.uint8, device=dev)
        times = []
        for s in range(warmup + steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            idx.matching_statistics_dev(bases_t.data_ptr(), n, off_t.data_ptr(), off_t.numel() - 1, dl.data_ptr(),
                                        df.data_ptr() if intervals else 0, ds.data_ptr() if intervals else 0, ws.data_ptr(),
                                        ws.numel(), stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            if s >= warmup:
                times.append(e0.elapsed_time(e1))
        st = idx.ms_workspace_stats(ws.data_ptr(), stream.cuda_stream)
        med = float(np.median(times))
        row = {"positions": n, "median_ms": round(med, 3), "min_ms": round(min(times), 3), "calls": len(times),
               "G_positions_per_s": round(n / med / 1e6, 2), "frac_len_k": round(st["full"] / max(1, n), 4),
               "contractions_per_base": round(st["contractions"] / max(1, st["walked"]), 4),
               "recomputes_per_base": round(st["recomputes"] / max(1, st["walked"]), 5),
               "walked_per_position": round(st["walked"] / max(1, n), 4)}
        # bytes per position: the base (1) and its len (1), 16 with intervals; the index lines a base touches are not
        # counted (two 16-byte quads per extension, mostly in one 64-byte line, cached or not)
        row["stream_bytes_per_position"] = 2 + (16 if intervals else 0)
        row["stream_GB_per_s"] = round(n * row["stream_bytes_per_position"] / med / 1e6, 1)
        return row

    bases_t = bench.gpu_reads(genomes, args.reads, 12345, dev)
    off_t = torch.arange(args.reads + 1, dtype=torch.int64, device=dev) * bench.READ_LEN
    res = {"config": args.config, "k": k, "streaming_support": streaming, "n_nodes": idx.n_nodes,
           "image_level": idx.image_level, "lcs_build_s": round(t_lcs, 4), "lcs_mean": round(float(lcs.mean()), 3),
           "lengths_only": run(bases_t, off_t, False, args.steps, args.warmup)}
    res["intervals"] = run(bases_t, off_t, True, args.steps, args.warmup)
    del bases_t
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    n_rand = min(args.reads, 2_000_000)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    rand_t = acgt[torch.randint(0, 4, (n_rand * bench.READ_LEN,), device=dev, generator=g)]
    off_r = torch.arange(n_rand + 1, dtype=torch.int64, device=dev) * bench.READ_LEN
    res["random_reads"] = run(rand_t, off_r, False, args.steps, args.warmup)
    del rand_t
    cat = np.concatenate(genomes)
    rng = np.random.default_rng(3)
    starts = rng.integers(0, len(cat) - 1_000_000, size=10)
    long_np = np.concatenate([synth.mutate(cat[s:s + 1_000_000].copy(), 0.01, int(s)) for s in starts])
    long_t = torch.from_numpy(long_np).to(dev)
    off_l = torch.arange(11, dtype=torch.int64, device=dev) * 1_000_000
    res["long_reads_10x1Mbp"] = run(long_t, off_l, False, args.steps, args.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
