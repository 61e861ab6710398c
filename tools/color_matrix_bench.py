"""Shared k-mer matrix benchmark (sbwtgpu_colorsets_shared_kmers) on bench.py's config 2 index: three
strains of --genome-len bases at k = 30.  It measures the real object (three colours, 8 sets) and, because 8 sets do not
load the product, synthetic objects uploaded onto the same index with ColorSets.from_arrays: n_sets 65 536 and 1 048 576,
n_colors 64, 192 and 4096, skewed sizes (sixteen large sets, a long tail of sets of one column).  For each shape, in ONE
process, alternating:

  device   ColorSets.shared_kmers(): sizes, sort, bit planes, the product on the matrix cores, mirror, copy to the host
  host     the route a user had before: copy() of ids and table, np.bincount, unpack, and B^T diag(w) B as an int64 matrix.
           The product runs over blocks of 65 536 sets through float64 BLAS (at most 16 threads) and is summed in int64: a
           block's entries are integers below 2^53, so every block is exact -- the fastest exact host route there is, many times
           quicker than numpy's own int64 matmul.

The two results are compared exactly.  A host route of more than --host-repeat-work multiply-adds (n_sets x C^2; half a
minute at the largest shape) runs once instead of every round.  Beyond --host-max-work (no default shape is) it runs on the
first sets only, the device call gets the same sets through weights that are 0 elsewhere for the comparison, and the host's
time is scaled up to all sets (reported as "host_scaled"); the device's time is always that of the whole object with its
sizes as weights.
Reports per shape the medians, the device's pass times, and the product's i8 multiply-add rate: the multiply-adds the
v_mfma_i32_16x16x64_i8 instructions issued (64 x 64 x sets-of-the-limb per tile pair and limb) over the product pass, against
the chip's i8 ceiling of 2.5 x 10^15 multiply-adds a second (twice the BF16 rate).  Writes one JSON line to --out and prints it;
exit status 1 when a comparison fails or the device is slower than the host at the largest shape.

  python tools/color_matrix_bench.py [--steps 3] [--warmup 1] [--out profiles/color_matrix_bench.json]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
os.environ.setdefault("OPENBLAS_NUM_THREADS", os.environ["OMP_NUM_THREADS"])
os.environ.setdefault("MKL_NUM_THREADS", os.environ["OMP_NUM_THREADS"])

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
I8_CEILING_MACS = 2.5e15
BLOCK = 65536


def host_route(sets, n_colors, limit=None):
    """(G int64, seconds) of the host route over the first `limit` sets (all when None)"""
    t0 = time.perf_counter()
    ids, table = sets.copy()
    w = np.bincount(ids, minlength=len(table)).astype(np.int64)
    w[0] = 0
    n = len(table) if limit is None else min(limit, len(table))
    G = np.zeros((n_colors, n_colors), dtype=np.int64)
    for lo in range(0, n, BLOCK):
        hi = min(lo + BLOCK, n)
        B = np.unpackbits(table[lo:hi].view(np.uint8), axis=1, bitorder="little")[:, :n_colors].astype(np.float64)
        G += ((B * w[lo:hi, None].astype(np.float64)).T @ B).astype(np.int64)
    return G, time.perf_counter() - t0, w


def synthetic(capi, idx, n_sets, n_colors, seed):
    rng = np.random.default_rng(seed)
    words = (n_colors + 63) // 64
    table = rng.integers(0, 2**64, size=(n_sets, words), dtype=np.uint64)
    table[:, 0] |= np.uint64(1)
    table[0] = 0
    n = idx.n_nodes
    ids = rng.integers(1, 17, size=n).astype(np.uint32)                  # sixteen large sets ...
    tail = rng.permutation(n)[:n_sets - 17]
    ids[tail] = np.arange(17, n_sets, dtype=np.uint32)                    # ... and a long tail of sets of one column
    return capi.ColorSets.from_arrays(idx, n_colors, ids, table)


def measure(sets, n_colors, steps, warmup, max_work, repeat_work):
    n_sets = sets.n_sets
    work = n_sets * n_colors * n_colors
    limit = None if work <= max_work else max(BLOCK, int(n_sets * max_work / work) // BLOCK * BLOCK)
    scale = 1.0 if limit is None else n_sets / limit
    dev_ms, host_ms, passes = [], [], []
    equal = True
    for s in range(warmup + steps):
        t0 = time.perf_counter()
        G = sets.shared_kmers()
        dt = (time.perf_counter() - t0) * 1e3
        info = sets.shared_info
        if s >= warmup:
            dev_ms.append(dt)
            passes.append(info["pass_ms"])
        if work > repeat_work and s > 0:                                  # a long host route runs once
            continue
        H, sec, w = host_route(sets, n_colors, limit)
        if s >= warmup or work > repeat_work:
            host_ms.append(sec * 1e3 * scale)
        if limit is not None:                                             # the same sets on the device: weights 0 elsewhere
            w[limit:] = 0
            G = sets.shared_kmers(w)
        equal = equal and G.tobytes() == H.tobytes()
    sizes = sets.set_sizes()[1:]
    tiles = (n_colors + 63) // 64
    macs = sum(int((sizes >= 128**l).sum() + 63) // 64 * 64 for l in range(5)) * 4096 * (tiles * (tiles + 1) // 2)
    product_ms = float(np.median([p["product"] for p in passes]))
    res = {"n_sets": n_sets, "n_colors": n_colors, "used_mfma": info["used_mfma"], "n_sets_used": info["n_sets_used"],
           "n_limbs": info["n_limbs"], "results_equal": bool(equal),
           "device_ms": {"median": round(float(np.median(dev_ms)), 3), "min": round(min(dev_ms), 3), "max": round(max(dev_ms), 3)},
           "device_pass_ms": {p: round(float(np.median([x[p] for x in passes])), 3) for p in passes[0]},
           "host_ms": {"median": round(float(np.median(host_ms)), 3), "min": round(min(host_ms), 3), "max": round(max(host_ms), 3),
                       "calls": len(host_ms)},
           "host_scaled": limit is not None, "host_sets_measured": n_sets if limit is None else limit}
    res["host_over_device"] = round(res["host_ms"]["median"] / res["device_ms"]["median"], 2)
    if info["used_mfma"] and product_ms > 0:
        res["i8_macs_issued"] = macs
        res["i8_tmacs_per_s"] = round(macs / product_ms / 1e9, 2)
        res["fraction_of_i8_ceiling"] = round(macs / (product_ms * 1e-3) / I8_CEILING_MACS, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n-sets", type=int, nargs="*", default=[65536, 1048576])
    ap.add_argument("--n-colors", type=int, nargs="*", default=[64, 192, 4096])
    ap.add_argument("--host-repeat-work", type=float, default=1.2e12)
    ap.add_argument("--host-max-work", type=float, default=2e13)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_matrix_bench.json"))
    args = ap.parse_args()
    from sbwt_amd import capi, synth

    if capi.device_count() <= 0:
        raise SystemExit("color_matrix_bench needs a GPU")
    k = 30
    genomes = synth.coli3_like(args.genome_len)
    bits = capi.build_bits_gpu([g.tobytes() for g in genomes], k, False, True, device=0)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)
    with capi.ColorSetsBuilder.create(idx, len(genomes)) as bld:
        for c, g in enumerate(genomes):
            bld.add_sequences(c, g, np.array([0, len(g)], dtype=np.int64))
        real = bld.finish()
    res = {"bench": "color_matrix", "config": 2, "k": k, "genome_len": args.genome_len, "steps": args.steps, "warmup": args.warmup,
           "n_nodes": idx.n_nodes, "threads": int(os.environ["OMP_NUM_THREADS"]), "shapes": []}
    with real:
        r = measure(real, real.n_colors, args.steps, args.warmup, args.host_max_work, args.host_repeat_work)
        r["object"] = "real"
        r["matrix"] = real.shared_kmers().tolist()
        res["shapes"].append(r)
    for n_sets in args.n_sets:
        for n_colors in args.n_colors:
            with synthetic(capi, idx, n_sets, n_colors, n_sets + n_colors) as s:
                r = measure(s, n_colors, args.steps, args.warmup, args.host_max_work, args.host_repeat_work)
                r["object"] = "synthetic"
                res["shapes"].append(r)
    last = res["shapes"][-1]
    res["results_equal"] = all(x["results_equal"] for x in res["shapes"])
    res["device_not_slower_at_largest"] = last["device_ms"]["median"] <= last["host_ms"]["median"]
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)
    idx.close()
    return 0 if res["results_equal"] and res["device_not_slower_at_largest"] else 1


if __name__ == "__main__":
    sys.exit(main())
