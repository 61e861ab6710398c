"""Bubble benchmark (sbwtgpu_bubbles_create): bench.py's config 2 index (three strains, k = 30) with its
three strains as colours from the colour-set builder, and one plain graph handle with links and column map, all built once
outside the timing.  In ONE process, alternating:

  (a) graph           sbwtgpu_unitigs_create_graph, LINKS | COLUMN_MAP, alone   -- the call the project had before
  (b) bubbles         sbwtgpu_bubbles_create on the handle, without colours
  (c) bubbles_colors  sbwtgpu_bubbles_create on the handle, with the colour-set object
  (d) host_route      what a user did before, from the same handle: links() + column_map() + copy() + ColorSets.copy() to the
                      host, numpy in-degrees, a vectorised diamond test, and a per-branch AND / OR reduce of the rows

Host clock around each whole leg (all are synchronous), --warmup rounds, then median and min-max of --steps; the order of the
legs rotates from round to round.  With them the device-event times the call reports itself (sbwtgpu_bubbles_stats; medians)
and the parts of the host route.  Before any timing the records and rows of (c) and of (d) are compared: they must be equal.
No time is fixed in advance.  Writes one JSON line to --out and prints it.

  python tools/bubbles_bench.py [--steps 7] [--warmup 2] [--out profiles/bubbles_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NONE = np.uint32(0xFFFFFFFF)


def host_route(u, sets, k, capi):
    """(records, inter, uni, ms of the parts): the bubbles recomputed on the host from what the handle and the object copy out."""
    t0 = time.perf_counter()
    lo, lt = u.links()
    cu, _ = u.column_map()
    _, off, _ = u.copy()
    ids, table = sets.copy()
    t1 = time.perf_counter()
    n = len(lo) - 1
    indeg = np.bincount(lt, minlength=n)
    outdeg = np.diff(lo)
    s = np.flatnonzero(outdeg == 2)
    a, b = lt[lo[s]].astype(np.int64), lt[lo[s] + 1].astype(np.int64)
    ok = (indeg[a] == 1) & (indeg[b] == 1) & (outdeg[a] == 1) & (outdeg[b] == 1) & (a != s) & (b != s) & (a != b)
    s, a, b = s[ok], a[ok], b[ok]
    t = lt[lo[a]].astype(np.int64)
    ok = (lt[lo[b]] == t) & (indeg[t] == 2) & (t != a) & (t != b)
    s, a, b, t = s[ok], a[ok], b[ok], t[ok]
    rec = np.zeros(len(s), dtype=capi.BUBBLE)
    rec["source"], rec["sink"] = s, t
    rec["branch"] = np.stack([a, b], axis=1)
    rec["n_kmers"] = np.stack([off[a + 1] - off[a], off[b + 1] - off[b]], axis=1) - (k - 1)
    rec["kind"] = np.all(rec["n_kmers"] == k, axis=1)
    t2 = time.perf_counter()
    W = table.shape[1]
    slot = np.full(n, NONE, dtype=np.uint32)
    slot[a] = 2 * np.arange(len(s), dtype=np.uint32)
    slot[b] = 2 * np.arange(len(s), dtype=np.uint32) + 1
    cols = np.flatnonzero(cu != NONE)
    sl = slot[cu[cols]]
    on = sl != NONE
    cols, sl = cols[on], sl[on]
    order = np.argsort(sl, kind="stable")
    rows = table[ids[cols[order]]]
    starts = np.searchsorted(sl[order], np.arange(2 * len(s)))
    inter = np.bitwise_and.reduceat(rows, starts, axis=0).reshape(len(s), 2, W) if len(s) else np.zeros((0, 2, W), dtype=np.uint64)
    uni = np.bitwise_or.reduceat(rows, starts, axis=0).reshape(len(s), 2, W) if len(s) else np.zeros((0, 2, W), dtype=np.uint64)
    t3 = time.perf_counter()
    return rec, inter, uni, {"copies_ms": (t1 - t0) * 1e3, "detect_ms": (t2 - t1) * 1e3, "reduce_ms": (t3 - t2) * 1e3}


def summary(t):
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "calls": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bubbles_bench.json"))
    args = ap.parse_args()
    from sbwt_amd import capi, synth

    if capi.device_count() <= 0:
        raise SystemExit("bubbles_bench needs a GPU")
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
    u = idx.unitig_graph_dev(links=True, column_map=True)

    # (c) and (d) give the same records and rows; (b) the same records
    with u.bubbles(sets) as b:
        rec, (inter, uni), info = b.records(), b.branch_colors(), b.info()
    h_rec, h_inter, h_uni, _ = host_route(u, sets, k, capi)
    assert rec.tobytes() == h_rec.tobytes(), "the records of the call and of the host route differ"
    assert np.array_equal(inter, h_inter) and np.array_equal(uni, h_uni), "the rows of the call and of the host route differ"
    with u.bubbles() as b:
        assert b.records().tobytes() == rec.tobytes() and b.info()["n_snps"] == info["n_snps"]
    kinds = {"n_bubbles": info["n_bubbles"], "n_snps": info["n_snps"],
             "branches_whole_in_one_strain": int((np.bitwise_count(inter[:, :, 0]) == 1).sum()) if hasattr(np, "bitwise_count") else None,
             "branches_inter_ne_union": int((inter != uni).any(axis=2).sum())}

    legs = ("graph", "bubbles", "bubbles_colors", "host_route")
    wall = {leg: [] for leg in legs}
    dev = {leg: [] for leg in legs}
    for s in range(args.warmup + args.steps):
        for leg in legs[s % 4:] + legs[:s % 4]:
            t0 = time.perf_counter()
            if leg == "graph":
                x = idx.unitig_graph_dev(links=True, column_map=True)
            elif leg == "host_route":
                d = host_route(u, sets, k, capi)[3]
            else:
                x = u.bubbles(sets if leg == "bubbles_colors" else None)
            dt = (time.perf_counter() - t0) * 1e3
            if leg == "graph":
                assert x.n_kmers == n_kmers
                d = {"passes_sum_ms": sum(x.stats()["pass_ms"].values()), **x.graph_stats()}
                x.close()
            elif leg != "host_route":
                assert x.n_bubbles == info["n_bubbles"]
                d = x.stats()["pass_ms"]
                x.close()
            if s >= args.warmup:
                wall[leg].append(dt)
                dev[leg].append(d)
    res = {"bench": "bubbles", "config": 2, "k": k, "genome_len": args.genome_len, "steps": args.steps, "warmup": args.warmup,
           "n_nodes": idx.n_nodes, "n_kmers": n_kmers, "n_unitigs": u.n_unitigs, "n_links": u.n_links(), "n_colors": len(genomes), **kinds}
    for leg in legs:
        res[leg] = summary(wall[leg])
        res[leg]["parts_ms"] = {key: round(float(np.median([x[key] for x in dev[leg]])), 3) for key in dev[leg][0]}
    res["host_route_over_bubbles_colors"] = round(res["host_route"]["median_ms"] / res["bubbles_colors"]["median_ms"], 2)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)
    u.close()
    sets.close()
    idx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
