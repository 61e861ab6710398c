"""Coloured-merge benchmark (sbwtgpu_colorsets_merge): bench.py's config 2 genomes as
tools/setop_bench.py splits them -- a = strains 1 + 2, b = strains 2 + 3, k = 30 -- each side coloured by the colour-set
builder (two colours a side), u = their union, built once outside the timing.  In ONE process, alternating:

  merge    sbwtgpu_colorsets_merge(u, sa, sb): three key extractions, locate and gather, pairs, rows, numbering
  readd    the route the project had before: a builder on u with four colours, every strain's sequence added again (strain 2
           twice: it is a colour of both sides), then finish

Host clock around each whole route (every call is synchronous), --warmup rounds, then median and min-max of --steps; the two
results must be equal byte for byte.  No speed gate: the re-add route grows with the reference bases, the merge with the
columns; both medians, their ratio, the merge's pass times and the number of 5 Mbp references at which the two lines would
cross by these numbers are reported.  Writes one JSON line to --out and prints it.

  python tools/colorsets_merge_bench.py [--steps 7] [--warmup 2] [--out profiles/colorsets_merge_bench.json]"""
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
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colorsets_merge_bench.json"))
    args = ap.parse_args()
    from sbwt_amd import capi, synth

    if capi.device_count() <= 0:
        raise SystemExit("colorsets_merge_bench needs a GPU")
    k = 30
    genomes = synth.coli3_like(args.genome_len)
    offs = [np.array([0, len(g)], dtype=np.int64) for g in genomes]

    def index_of(bits):
        return capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)
    sides = [(0, 1), (1, 2)]
    a, b = (index_of(capi.build_bits_gpu([genomes[i].tobytes() for i in side], k, False, True, device=0)) for side in sides)
    u = index_of(a.setop(b, "union")[0])
    colored = []
    for idx, side in ((a, sides[0]), (b, sides[1])):
        with capi.ColorSetsBuilder.create(idx, 2) as bld:
            for c, i in enumerate(side):
                bld.add_sequences(c, genomes[i], offs[i])
            colored.append(bld.finish())
    sa, sb = colored
    readds = [(c, i) for c, i in enumerate(sides[0] + sides[1])]          # colours 0 .. 3 of u

    def merge_route(keep):
        m = capi.ColorSets.merge(u, sa, sb)
        return m if keep else (m.merge_info, m.close())[0]

    def readd_route(keep):
        with capi.ColorSetsBuilder.create(u, 4) as bld:
            for c, i in readds:
                bld.add_sequences(c, genomes[i], offs[i])
            sets = bld.finish()
        return sets if keep else sets.close()

    got, want = merge_route(True), readd_route(True)                      # (the first warm-up round: the results are compared)
    cg, cw = got.copy(), want.copy()
    equal = got.info() == want.info() and cg[0].tobytes() == cw[0].tobytes() and cg[1].tobytes() == cw[1].tobytes()
    info = got.info()
    counts = {f: v for f, v in got.merge_info.items() if f != "pass_ms"}
    got.close(), want.close()
    del cg, cw
    times, passes = {"merge": [], "readd": []}, []
    for s in range(max(args.warmup - 1, 0) + args.steps):
        for name, route in (("merge", merge_route), ("readd", readd_route)):
            t0 = time.perf_counter()
            out = route(False)
            dt = (time.perf_counter() - t0) * 1e3
            if s >= max(args.warmup - 1, 0):
                times[name].append(dt)
                if name == "merge":
                    passes.append(out["pass_ms"])
    res = {"bench": "colorsets_merge", "config": 2, "k": k, "genome_len": args.genome_len, "steps": args.steps, "warmup": args.warmup,
           "n_nodes": {"a": a.n_nodes, "b": b.n_nodes, "u": u.n_nodes}, "n_colors_out": info["n_colors"], "n_sets": info["n_sets"],
           "counts": counts, "results_equal": bool(equal), "reference_bases_readded": int(sum(len(genomes[i]) for _, i in readds))}
    for name, t in times.items():
        res[name] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "calls": len(t)}
    res["merge"]["pass_ms"] = {p: round(float(np.median([x[p] for x in passes])), 3) for p in passes[0]}
    res["merge_over_readd"] = round(res["merge"]["median_ms"] / res["readd"]["median_ms"], 3)
    # the re-add route per reference of genome_len bases, by this run; the merge does not depend on the number of references
    per_ref = res["readd"]["median_ms"] / len(readds)
    res["readd_ms_per_reference"] = round(per_ref, 3)
    res["crossover_references"] = round(res["merge"]["median_ms"] / per_ref, 2)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)
    for x in (sa, sb, u, a, b):
        x.close()
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
