"""Set-operation benchmark (sbwtgpu_index_setop): bench.py's config 2 genome set (the same synth call: three coli-like
genomes, k = 30) split into two overlapping halves, a = genomes 0-1, b = genomes 1-2, each built into an index.  Prints one
JSON line: the counts, per operation the time of the whole call and its four passes (keys of a, keys of b, merge + select,
builder tail + columns; host clocks around synchronised passes), the counts-only call, and -- measured in the same run as
the yardstick for union -- the route the project had before: unitigs(a) + unitigs(b) -> sbwtgpu_build_plain_matrix.  The
union of both routes is compared bit for bit.

  python tools/setop_bench.py [--steps 5] [--warmup 1] [--genome-len 5000000] [--revcomp 0]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS = ("union", "intersection", "difference", "symmetric-difference")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--revcomp", type=int, default=0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    from sbwt_amd import capi, synth

    k = 30
    genomes = synth.coli3_like(args.genome_len)
    halves = [[g.tobytes() for g in genomes[:2]], [g.tobytes() for g in genomes[1:]]]
    idx = []
    for seqs in halves:
        bits = capi.build_bits_gpu(seqs, k, bool(args.revcomp), True, device=0)
        idx.append(capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0))
    a, b = idx

    def med(v):
        return round(float(np.median(v)), 3)
    ops, union_bits, info = {}, None, None
    for op in OPS:
        wall, passes = [], []
        for s in range(args.warmup + args.steps):
            t0 = time.time()
            bits, info = a.setop(b, op)
            t = time.time() - t0
            if s >= args.warmup:
                wall.append(t * 1e3)
                passes.append(info["pass_ms"])
        if op == "union":
            union_bits = bits
        ops[op] = {"call_ms": med(wall), "pass_ms": {p: med([x[p] for x in passes]) for p in passes[0]},
                   "n_result": info["n_result"], "n_nopred": info["n_nopred"], "n_nodes": bits.n_nodes}
    wall = []
    for s in range(args.warmup + args.steps):
        t0 = time.time()
        counts = a.setop_counts(b)
        if s >= args.warmup:
            wall.append((time.time() - t0) * 1e3)
    counts_ms = med(wall)

    # the yardstick: both indexes back to sequence, the text builder on the concatenation
    wall, parts = [], []
    for s in range(args.warmup + args.steps):
        t0 = time.time()
        ua, ub = a.unitigs(), b.unitigs()
        t1 = time.time()
        seqs = []
        for bases, off, _ in (ua, ub):
            raw = bases.tobytes()
            seqs += [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]
        t2 = time.time()
        rebuilt = capi.build_bits_gpu(seqs, k, False, True, device=0)
        t3 = time.time()
        if s >= args.warmup:
            wall.append((t3 - t0) * 1e3)
            parts.append({"unitigs": (t1 - t0) * 1e3, "host_split": (t2 - t1) * 1e3, "build": (t3 - t2) * 1e3})
    same = (rebuilt.n_nodes, rebuilt.n_kmers) == (union_bits.n_nodes, union_bits.n_kmers) and \
        all(np.array_equal(x, y) for x, y in zip(rebuilt.cols + [rebuilt.ssup], union_bits.cols + [union_bits.ssup]))
    yard = {"call_ms": med(wall), "parts_ms": {p: med([x[p] for x in parts]) for p in parts[0]}, "n_unitigs": len(seqs)}
    print(json.dumps({
        "bench": "setop", "k": k, "genome_len": args.genome_len, "revcomp": args.revcomp, "steps": args.steps,
        "n_nodes": [a.n_nodes, b.n_nodes],
        "counts": {f: counts[f] for f in ("n_a", "n_b", "n_both", "n_either")}, "jaccard": round(counts["jaccard"], 6),
        "ops": ops, "counts_only_ms": counts_ms, "unitig_rebuild_union": yard, "union_routes_bit_identical": bool(same),
        "union_speedup_over_rebuild": round(yard["call_ms"] / ops["union"]["call_ms"], 2),
    }))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
