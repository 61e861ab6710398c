"""Coloured-unitig benchmark (sbwtgpu_unitigs_create_colored): bench.py's config 2 index (three strains,
k = 30) with its three strains as colours from the colour-set builder, built once outside the timing.  In ONE process,
alternating:

  plain     sbwtgpu_unitigs_create(index)            -- the call the project had before, unchanged code
  colored   sbwtgpu_unitigs_create_colored(sets)     -- the same passes, cut where the colour set changes

Host clock around each whole call (both are synchronous), --warmup rounds, then median and min-max of --steps, with the
per-pass device times of both (medians), n_unitigs both ways, the colour breaks and the jump rounds.  No ratio is fixed in
advance: the coloured call is measured against the plain call of the same run.  Writes one JSON line to --out and prints it.

--first colored swaps the order inside every round (what follows what matters to the allocator: see section 18).

  python tools/colored_unitig_bench.py [--steps 7] [--warmup 2] [--first plain|colored] [--out profiles/colored_unitigs_bench.json]"""
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
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--first", default="plain", choices=["plain", "colored"], help="which call of every round runs first")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colored_unitigs_bench.json"))
    args = ap.parse_args()
    from sbwt_amd import capi, synth

    if capi.device_count() <= 0:
        raise SystemExit("colored_unitig_bench needs a GPU")
    k = 30
    genomes = synth.coli3_like(args.genome_len)
    bits = capi.build_bits_gpu([g.tobytes() for g in genomes], k, False, True, device=0)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)
    n_kmers = bits.n_kmers
    del bits
    with capi.ColorSetsBuilder.create(idx, len(genomes)) as bld:
        for c, g in enumerate(genomes):
            bld.add_sequences(c, g, np.array([0, len(g)], dtype=np.int64))
        sets = bld.finish()

    def plain():
        return idx.unitigs_dev()

    def colored():
        return sets.unitigs_dev()

    names = ("plain", "colored") if args.first == "plain" else ("colored", "plain")
    wall = {n: [] for n in names}
    passes = {n: [] for n in names}
    counts = {}
    for s in range(args.warmup + args.steps):
        for name in names:
            call = plain if name == "plain" else colored
            t0 = time.perf_counter()
            u = call()
            dt = (time.perf_counter() - t0) * 1e3
            st = u.stats()
            counts[name] = {"n_unitigs": u.n_unitigs, "total_bases": u.total_bases, "jump_rounds": st["jump_rounds"]}
            assert u.n_kmers == n_kmers
            if name == "colored":
                counts[name].update(u.color_info())
            u.close()
            if s >= args.warmup:
                wall[name].append(dt)
                passes[name].append(st["pass_ms"])
    info = sets.info()
    res = {"bench": "colored_unitigs", "config": 2, "k": k, "genome_len": args.genome_len, "steps": args.steps, "warmup": args.warmup,
           "first": args.first, "n_nodes": idx.n_nodes, "n_kmers": n_kmers, "n_colors": info["n_colors"], "n_sets": info["n_sets"], "words": info["words"],
           "jump_rounds_bound": int(math.ceil(math.log2(max(2, idx.n_nodes)))) + 2}
    for name in names:
        t = wall[name]
        res[name] = dict(counts[name], median_ms=round(float(np.median(t)), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3),
                         calls=len(t), pass_ms={p: round(float(np.median([x[p] for x in passes[name]])), 3) for p in passes[name][0]})
        res[name]["passes_sum_ms"] = round(sum(res[name]["pass_ms"].values()), 3)
    res["colored_over_plain"] = round(res["colored"]["median_ms"] / res["plain"]["median_ms"], 3)
    res["colored_minus_plain_ms"] = round(res["colored"]["median_ms"] - res["plain"]["median_ms"], 3)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)
    sets.close()
    idx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
