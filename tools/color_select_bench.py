"""Colour-select benchmark (sbwtgpu_colorsets_select): bench.py's config 2 index (three strains, k = 30)
with its three strains as colours from the colour-set builder, built once outside the timing.  Three predicates -- the core of
all three strains, the k-mers unique to strain 0, the accessory k-mers -- and for each, in ONE process, alternating:

  select    sbwtgpu_colorsets_select(sets, predicate)   -- keys of the index, verdicts, flags, select, builder tail
  old       the route the project had before: ColorSets.unitigs() (coloured unitigs copied to the host), a host filter
            on set_id with numpy, capi.build_bits_gpu of the surviving strings

Host clock around each whole route (both end synchronised), --warmup rounds, then median and min-max of --steps, with the
select call's pass_ms (medians) beside it.  Both routes must give the same bits (asserted on every round).  No ratio is fixed
in advance: the old route is the yardstick.  Writes one JSON line to --out and prints it.

  python tools/color_select_bench.py [--steps 7] [--warmup 2] [--out profiles/color_select_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def same_bits(a, b):
    return (a.n_nodes, a.n_kmers) == (b.n_nodes, b.n_kmers) and all(np.array_equal(x, y) for x, y in zip(a.cols + [a.ssup], b.cols + [b.ssup]))


def popcounts(a):
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1), axis=1).sum(axis=1, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_select_bench.json"))
    args = ap.parse_args()
    from sbwt_amd import capi, synth

    if capi.device_count() <= 0:
        raise SystemExit("color_select_bench needs a GPU")
    k = 30
    genomes = synth.coli3_like(args.genome_len)
    bits = capi.build_bits_gpu([g.tobytes() for g in genomes], k, False, True, device=0)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)
    n_kmers = bits.n_kmers
    del bits
    C = len(genomes)
    with capi.ColorSetsBuilder.create(idx, C) as bld:
        for c, g in enumerate(genomes):
            bld.add_sequences(c, g, np.array([0, len(g)], dtype=np.int64))
        sets = bld.finish()
    everyone = list(range(C))
    predicates = {"core": (everyone, None, C, C), "unique_0": ([0], everyone[1:], 1, 1), "accessory": (everyone, None, 1, C - 1)}

    def select(pred):
        return sets.select(*pred)

    def old(pred):
        include, exclude, min_in, max_in = pred
        bases, off, first_col, set_id = sets.unitigs()
        _, table = sets.copy()
        inc = sets.color_mask(include)
        pop = popcounts(table & inc[None, :])
        ok = (pop >= min_in) & (pop <= max_in)
        if exclude is not None:
            ok &= ~(table & sets.color_mask(exclude)[None, :]).any(axis=1)
        raw = bases.tobytes()
        keep = np.nonzero(ok[set_id])[0]
        return capi.build_bits_gpu([raw[off[i]:off[i + 1]] for i in keep], k, False, True, device=0), {"n_unitigs_kept": int(len(keep)),
                                                                                                       "n_unitigs": int(len(set_id))}

    res = {"bench": "color_select", "config": 2, "k": k, "genome_len": args.genome_len, "steps": args.steps, "warmup": args.warmup,
           "n_nodes": idx.n_nodes, "n_kmers": n_kmers, "n_colors": C, "n_sets": sets.n_sets, "words": sets.words, "same_bits": True,
           "predicates": {}}
    for name, pred in predicates.items():
        wall = {"select": [], "old": []}
        passes, info, old_info = [], None, None
        for s in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            got, info = select(pred)
            t1 = time.perf_counter()
            want, old_info = old(pred)
            t2 = time.perf_counter()
            assert same_bits(got, want), name
            if s >= args.warmup:
                wall["select"].append((t1 - t0) * 1e3)
                wall["old"].append((t2 - t1) * 1e3)
                passes.append(info["pass_ms"])
        entry = {f: info[f] for f in ("n_real", "n_selected", "n_sets_matched", "n_nopred")}
        entry.update(old_info)
        for route, t in wall.items():
            entry[route] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "calls": len(t)}
        entry["select"]["pass_ms"] = {p: round(float(np.median([x[p] for x in passes])), 3) for p in passes[0]}
        entry["old_over_select"] = round(entry["old"]["median_ms"] / entry["select"]["median_ms"], 3)
        res["predicates"][name] = entry
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
