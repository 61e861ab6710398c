"""Genotype benchmark (sbwtgpu_genotype_*): Genotype.add_dev beside the route a user had before it and
beside the calls it is built on, on bench.py's config 2 index (three strains, k = 30) with its three strains as colours, one
plain graph handle and its bubbles made outside the timing, and bench.gpu_reads for the reads, in ONE process.

  legs     (a)  Genotype.add_dev with one strand and with two
           (b)  the same counters entirely on the device without it: search_dev_i32, then torch -- a gather through a
                per-column position tensor made beforehand (-1 for a column that is no branch column), bincount into kmer_hits;
                once with two boolean-mask compactions (each synchronises with the host inside the leg), once lean: clamp the
                index, gather, send misses and other columns to one extra bin, no compaction and no synchronisation
           (c)  Screen.add_dev, for scale
           (d)  the search alone, for scale: the one the add runs (sbwtgpu_search_dev_i32)
           The legs alternate and rotate their order from round to round; --warmup rounds, then median and min-max of --steps.
           Device events around each call.  Before any timing (a) and (b) are checked to give equal kmer_hits.
  queries  branches() + calls() with colours on the accumulator, host clock (they synchronise); create, host clock
  strains  per strain, reads drawn from that strain alone: ref_only / ref_sites of every colour

No time is fixed in advance.  Writes one JSON line to --out and prints it.

  python tools/genotype_bench.py [--reads N] [--steps 7] [--warmup 2] [--out profiles/genotype_bench.json]"""
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
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
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
    with capi.ColorSetsBuilder.create(idx, len(genomes)) as b:
        for c, g in enumerate(genomes):
            b.add_sequences(c, g, np.array([0, len(g)], dtype=np.int64))
        sets = b.finish()
    u = idx.unitig_graph_dev(links=True, column_map=True)
    bub = u.bubbles(sets)
    res = {"config": 2, "k": k, "n_nodes": idx.n_nodes, "image_level": idx.image_level, "n_colors": len(genomes),
           "n_unitigs": u.n_unitigs, "n_bubbles": bub.n_bubbles, "n_snps": bub.n_snps}

    def host_clock(call, reps=5):
        call()
        t = []
        for _ in range(reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            call()
            t.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "calls": len(t)}

    res["create"] = host_clock(lambda: u.genotype(idx, bub).close())
    gt = {1: u.genotype(idx, bub), 2: u.genotype(idx, bub)}
    P = gt[1].n_branch_kmers
    res["n_branch_kmers"] = P
    res["object_bytes"] = {"kmer_hits": 8 * P, "bitmap": (idx.n_nodes + 63) // 64 * 8, "directory": (idx.n_nodes + 63) // 64 * 4,
                           "positions": 4 * P, "branch_off": 8 * (2 * bub.n_bubbles + 1), "inter": 16 * bub.words * bub.n_bubbles}

    stream = torch.cuda.current_stream(dev)
    n, L = args.reads, bench.READ_LEN
    bases_t = bench.gpu_reads(genomes, n, 12345, dev)
    T = bases_t.numel()
    off_t = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    W = n * (L - k + 1)
    res.update({"reads": n, "read_len": L, "windows": W})

    scr = sets.screen()
    need = {s: capi.genotype_workspace_bytes(T, n, s) for s in (1, 2)}
    ws = torch.zeros(max(need[2], capi.screen_workspace_bytes(T, n, 1), capi.search_workspace_bytes(T)), dtype=torch.uint8, device=dev)
    d_out = torch.empty(W, dtype=torch.int32, device=dev)
    d_ooff = torch.arange(n + 1, dtype=torch.int64, device=dev) * (L - k + 1)
    # the per-column position tensor of the torch route, from the handle's map and the records
    cu, co = u.column_map()
    rec = bub.records()
    slot = np.full(u.n_unitigs, -1, dtype=np.int64)
    slot[rec["branch"].reshape(-1)] = np.arange(2 * len(rec))
    branch_off = np.concatenate([[0], np.cumsum(rec["n_kmers"].reshape(-1).astype(np.int64))])
    real = cu != np.uint32(0xFFFFFFFF)
    col_slot = np.full(idx.n_nodes, -1, dtype=np.int64)
    col_slot[real] = slot[cu[real]]
    col_pos = np.where(col_slot >= 0, branch_off[np.maximum(col_slot, 0)] + co.astype(np.int64), -1)
    res["n_branch_columns"] = int((col_pos >= 0).sum())
    pos_t = torch.from_numpy(col_pos).to(dev)
    t_hits = torch.zeros(P, dtype=torch.int64, device=dev)
    t_lean = torch.zeros(P, dtype=torch.int64, device=dev)
    del cu, co, col_slot, col_pos

    def search():
        idx.streaming_search_dev_i32(bases_t.data_ptr(), T, off_t.data_ptr(), n, d_out.data_ptr(), d_ooff.data_ptr(), ws.data_ptr(),
                                     ws.numel(), stream.cuda_stream, False)

    def torch_route():
        search()
        p = pos_t[d_out[d_out >= 0].long()]
        t_hits.add_(torch.bincount(p[p >= 0], minlength=P))

    def torch_route_lean():
        search()
        p = torch.where(d_out >= 0, pos_t[d_out.clamp(min=0).long()], -1)
        t_lean.add_(torch.bincount(p + 1, minlength=P + 1)[1:])

    def add(strands):
        gt[strands].add_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, ws.data_ptr(), need[strands], strands, stream.cuda_stream)

    def screen_add():
        scr.add_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, ws.data_ptr(), ws.numel(), 1, stream.cuda_stream)

    # ---- (a) and (b) give equal counters: one add each on empty accumulators ----
    add(1)
    torch_route()
    torch_route_lean()
    torch.cuda.synchronize(dev)
    info = gt[1].info()
    off, hits = gt[1].kmer_hits()
    h_hits = t_hits.cpu().numpy()
    if not (torch.equal(t_hits, t_lean) and np.array_equal(off, branch_off) and np.array_equal(hits.astype(np.int64), h_hits)
            and info["n_site_hits"] == int(h_hits.sum()) and info["n_hits"] == int((d_out >= 0).sum().item()) and info["n_windows"] == W):
        raise SystemExit("Genotype.add_dev and the torch route disagree")
    res["agree_with_torch_route"] = True
    res["one_batch"] = {x: info[x] for x in ("n_windows", "n_hits", "n_site_hits")}
    call, sites, match, only = gt[1].calls()
    res["one_batch"]["calls"] = {name: int((call == v).sum()) for v, name in enumerate((".", "a", "b", "ab"))}

    # ---- the legs, alternating, their order rotated from round to round ----
    legs = [("genotype_add_dev_strands1", lambda: add(1)), ("genotype_add_dev_strands2", lambda: add(2)), ("torch_route", torch_route),
            ("torch_route_lean", torch_route_lean), ("screen_add_dev", screen_add), ("search_alone", search)]
    times = {name: [] for name, _ in legs}
    for r in range(args.warmup + args.steps):
        order = legs[r % len(legs):] + legs[:r % len(legs)]
        for name, fn in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if r >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    rows = {}
    for name, t in times.items():
        med = float(np.median(t))
        windows = 2 * W if name.endswith("strands2") else W
        rows[name] = {"median_ms": round(med, 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "calls": len(t),
                      "G_windows_per_s": round(windows / med / 1e6, 2)}
    a, tr, d, sc = (rows[x]["median_ms"] for x in ("genotype_add_dev_strands1", "torch_route", "search_alone", "screen_add_dev"))
    rows["torch_route_over_genotype_add"] = round(tr / a, 3)
    rows["torch_route_lean_over_genotype_add"] = round(rows["torch_route_lean"]["median_ms"] / a, 3)
    rows["genotype_add_over_search"] = round(a / d, 3)
    rows["accumulate_ms_estimate"] = round(a - d, 3)
    rows["screen_accumulate_ms_estimate"] = round(sc - d, 3)
    res["legs"] = rows
    res["workspace_bytes"] = {"strands1": need[1], "strands2": need[2]}

    # ---- the queries ----
    res["queries"] = {"branches": host_clock(gt[1].branches), "calls_with_colours": host_clock(gt[1].calls), "info": host_clock(gt[1].info),
                      "branches_then_calls": host_clock(lambda: (gt[1].branches(), gt[1].calls()))}
    del bases_t, t_hits, t_lean, pos_t

    # ---- which reference does a sample follow: reads of one strain at a time ----
    m = max(1, n // 10)
    off_m = torch.arange(m + 1, dtype=torch.int64, device=dev) * L
    res["strains"] = []
    for c, g in enumerate(genomes):
        reads_c = bench.gpu_reads([g], m, 777 + c, dev)
        gt[1].reset()
        gt[1].add_dev(reads_c.data_ptr(), reads_c.numel(), off_m.data_ptr(), m, ws.data_ptr(), need[1], 1, stream.cuda_stream)
        torch.cuda.synchronize(dev)
        call, sites, match, only = gt[1].calls()
        res["strains"].append({"reads_from": c, "reads": m, "calls": {name: int((call == v).sum()) for v, name in enumerate((".", "a", "b", "ab"))},
                               "ref_sites": sites.tolist(), "ref_match": match.tolist(), "ref_only": only.tolist(),
                               "only_over_sites": [round(int(o) / max(1, int(s)), 4) for o, s in zip(only, sites)]})
        del reads_c
    for x in gt.values():
        x.close()
    scr.close()
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
