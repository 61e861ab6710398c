"""Colour-set build benchmark: the two ways to a colour-set object of bench.py's config 2 index with its three strains as
colours, as tools/pseudoalign_bench.py --sets places them -- at 64 colours (0, 1, 2), at 192 (0, 70, 130) and at 4096
(0, 2000, 4095) -- in ONE process, alternating:

  wide     sbwtgpu_colors_create_wide + three sbwtgpu_colors_add_batch + sbwtgpu_colorsets_compress (the n x W x 8-byte matrix
           is allocated, zeroed, coloured, hashed and freed)
  stream   sbwtgpu_colorsets_builder_create + three _add_batch + _finish (only the object is held)

Host clock around each whole route (every call is synchronous), --warmup rounds, then median and min-max of --steps; the
device bytes held at the peak of each route from the objects' own accounting; the two results must be equal byte for byte.
The gate of section 16 at 4096 colours: median(stream) <= median(wide) + (max - min of the wide route's timings); at 64 and
192 colours the ratio is reported only.  Also: the time of each close (an add call without sequences for the next colour) and
of finish alone on the same index.  Writes one JSON line to --out and prints it.

  python tools/colorsets_build_bench.py [--steps 7] [--warmup 2] [--out profiles/colorsets_stream_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STRAIN_COLORS = {64: (0, 1, 2), 192: (0, 70, 130), 4096: (0, 2000, 4095)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colorsets_stream_bench.json"))
    args = ap.parse_args()
    from sbwt_amd import capi, synth

    if capi.device_count() <= 0:
        raise SystemExit("colorsets_build_bench needs a GPU")
    k = 30
    genomes = synth.coli3_like(args.genome_len)
    offs = [np.array([0, len(g)], dtype=np.int64) for g in genomes]
    bits = capi.build_bits_gpu([g.tobytes() for g in genomes], k, False, True, device=0)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)
    del bits
    n = idx.n_nodes
    res = {"config": 2, "k": k, "n_nodes": n, "steps": args.steps, "warmup": args.warmup, "routes": {}, "gate": {}}

    def wide_route(nc, keep):
        with capi.WideColors.create(idx, nc) as wide:
            for c, g, off in zip(STRAIN_COLORS[nc], genomes, offs):
                wide.add_sequences(c, g, off)
            sets = capi.ColorSets.from_colors(wide)
        return sets if keep else sets.close()

    def stream_route(nc, keep, held=None):
        with capi.ColorSetsBuilder.create(idx, nc) as b:
            for c, g, off in zip(STRAIN_COLORS[nc], genomes, offs):
                b.add_sequences(c, g, off)
                if held is not None:
                    held.append(b.info()["device_bytes"])
            sets = b.finish()
        return sets if keep else sets.close()

    for nc in STRAIN_COLORS:
        words = (nc + 63) // 64
        a, b = wide_route(nc, True), stream_route(nc, True)          # (the first warm-up round: the results are compared)
        ia, ib = a.info(), b.info()
        ca, cb = a.copy(), b.copy()
        if ia != ib or ca[0].tobytes() != cb[0].tobytes() or ca[1].tobytes() != cb[1].tobytes():
            raise SystemExit("the two routes differ at %d colours" % nc)
        a.close(), b.close()
        del ca, cb
        held = []
        stream_route(nc, False, held)
        times = {"wide": [], "stream": []}
        for s in range(max(args.warmup - 1, 0) + args.steps):
            for name, route in (("wide", wide_route), ("stream", stream_route)):
                t0 = time.perf_counter()
                route(nc, False)
                dt = (time.perf_counter() - t0) * 1e3
                if s >= max(args.warmup - 1, 0):
                    times[name].append(dt)
        row = {"n_colors": nc, "words": words, "strain_colors": list(STRAIN_COLORS[nc]), "results_equal": True, "n_sets": ia["n_sets"],
               "n_colored_columns": ia["n_colored_columns"], "object_bytes": ia["device_bytes"],
               # n x W x 8 for the matrix; compress adds 13 bytes per column of scratch, the ids and the table
               "wide_peak_bytes": n * words * 8 + 13 * n + 4 * n + ia["n_sets"] * words * 8,
               "stream_held_bytes": max(held),
               # finish adds 1 + 4 bytes per column, 4 per set and the result's table
               "stream_peak_bytes": max(held) + 5 * n + 4 * ia["n_sets"] + ia["n_sets"] * words * 8}
        for name, t in times.items():
            row[name] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "calls": len(t)}
        row["stream_over_wide"] = round(row["stream"]["median_ms"] / row["wide"]["median_ms"], 3)
        # the closes and finish alone: an add call without sequences for a new colour closes the open one
        spare = [c for c in range(nc) if c not in STRAIN_COLORS[nc]][:1]
        with capi.ColorSetsBuilder.create(idx, nc) as bld:
            closes, adds = [], []
            order = list(STRAIN_COLORS[nc])
            for i, (c, g, off) in enumerate(zip(order, genomes, offs)):
                t0 = time.perf_counter()
                bld.add_sequences(c, g, off)
                adds.append(round((time.perf_counter() - t0) * 1e3, 3))
                nxt = order[i + 1] if i + 1 < len(order) else spare[0]
                t0 = time.perf_counter()
                bld.add_sequences(nxt, np.zeros(0, np.uint8), np.zeros(1, np.int64))
                closes.append(round((time.perf_counter() - t0) * 1e3, 3))
            t0 = time.perf_counter()
            fin = bld.finish()
            row["finish_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            fin.close()
        row["add_ms"], row["close_ms"] = adds, closes
        res["routes"][str(nc)] = row
        if nc == 4096:
            w = row["wide"]
            bound = w["median_ms"] + (w["max_ms"] - w["min_ms"])
            res["gate"] = {"stream_median_ms": row["stream"]["median_ms"], "wide_median_ms": w["median_ms"],
                           "wide_spread_ms": round(w["max_ms"] - w["min_ms"], 3), "bound_ms": round(bound, 3),
                           "passed": bool(row["stream"]["median_ms"] <= bound)}
    res["gate_passed"] = bool(res["gate"].get("passed", False))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)
    idx.close()


if __name__ == "__main__":
    main()
