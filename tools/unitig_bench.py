"""Unitig-export benchmark (sbwtgpu_unitigs_create): builds bench.py's config 2, 3 or 5 index (the same synth calls and seeds),
or the index of ONE random sequence (--single BASES: a genome that is a single unitig), and prints one JSON line: n_unitigs,
total bases, the time of the whole call, ms per pass from device events, the number of pointer-jumping rounds and its bound
ceil(log2 n_nodes) + 2 -- and, measured in the same run as scale references, the LCS build of the same index and a plain
device-to-device copy of total_bases bytes.

  python tools/unitig_bench.py --config 2 [--steps 5] [--warmup 1]
  python tools/unitig_bench.py --single 10000000
Kernel names and times: run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/unitig_bench.py ...`."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2, choices=[2, 3, 5])
    ap.add_argument("--single", type=int, default=0, help="index one random sequence of this many bases instead (k = 31)")
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--derived", type=int, default=64)
    ap.add_argument("--revcomp", type=int, default=0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import torch
    from sbwt_amd import capi, synth

    k, streaming = 30, True
    if args.single:
        k = 31
        genomes = [synth.random_genome(args.single, 1)]
    else:
        if args.config == 3:
            k = 31
        elif args.config == 5:
            k, streaming = 63, False
        genomes = synth.pan_like(args.derived, args.genome_len) if args.config == 3 else synth.coli3_like(args.genome_len)
    dev = torch.device("cuda", 0)
    bits = capi.build_bits_gpu([g.tobytes() for g in genomes], k, bool(args.revcomp), streaming, device=0)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)
    n_kmers = bits.n_kmers
    del bits
    torch.cuda.synchronize(dev)
    t0 = time.time()
    idx.build_lcs()
    t_lcs = time.time() - t0

    wall, passes, rounds = [], [], 0
    for s in range(args.warmup + args.steps):
        t0 = time.time()
        u = idx.unitigs_dev()
        t = time.time() - t0
        st = u.stats()
        n_unitigs, total, nk = u.n_unitigs, u.total_bases, u.n_kmers
        u.close()
        if s >= args.warmup:
            wall.append(t * 1e3)
            passes.append(st["pass_ms"])
            rounds = st["jump_rounds"]
    assert nk == n_kmers
    names = list(passes[0].keys())
    pass_ms = {p: round(float(np.median([x[p] for x in passes])), 3) for p in names}

    src = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    copies = []
    for s in range(args.warmup + args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        if s >= args.warmup:
            copies.append(e0.elapsed_time(e1))

    res = {"config": "single" if args.single else args.config, "k": k, "add_revcomp": bool(args.revcomp),
           "n_nodes": idx.n_nodes, "n_kmers": n_kmers, "image_level": idx.image_level,
           "n_unitigs": n_unitigs, "total_bases": total, "bytes_per_kmer": round(total / max(1, n_kmers), 4),
           "mean_unitig_kmers": round(n_kmers / max(1, n_unitigs), 2),
           "create_wall_ms_median": round(float(np.median(wall)), 3), "create_wall_ms_min": round(min(wall), 3),
           "pass_ms": pass_ms, "passes_sum_ms": round(sum(pass_ms.values()), 3),
           "jump_rounds": rounds, "jump_rounds_bound": int(math.ceil(math.log2(max(2, idx.n_nodes)))) + 2,
           "scratch_bytes_per_column": 38,
           "ref_lcs_build_ms": round(t_lcs * 1e3, 3), "ref_copy_total_bases_ms": round(float(np.median(copies)), 4),
           "calls": len(wall)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
