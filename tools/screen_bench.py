"""Screen benchmark: Screen.add_dev beside the route a user had before it and beside the calls it is built
on, on bench.py's config 2 index with its three strains as colours and bench.gpu_reads for the reads, in ONE process.  Prints
one JSON line.

  legs     (a)  Screen.add_dev with one strand and with two
           (b)  the same accumulator entirely on the device without it: search_dev_i32, then torch -- a gather of
                ids[col], bincount into the per-set hits, a boolean scatter for the seen bitmap
           (c)  pseudoalign_sets_dev, for scale
           (d)  the search alone, for scale: the one the add runs (sbwtgpu_search_dev_i32), and the streaming one
           The legs alternate and rotate their order from round to round; --warmup rounds, then median and min-max of --steps.
           Device events around each call.  Before any timing (a) and (b) are checked to give equal vectors.
  queries  sets() + colors() on the accumulator, host clock (they synchronise)
  expand   a synthetic object of --synth-sets sets and 4096 colours on the same index: colors() and sets(), host clock; their
           difference is the per-colour expansion and its copies

  python tools/screen_bench.py [--reads N] [--steps 7] [--warmup 2] [--synth-sets 1000000]"""
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
    ap.add_argument("--synth-sets", type=int, default=1_000_000)
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
    n_sets = sets.n_sets
    res = {"config": 2, "k": k, "n_nodes": idx.n_nodes, "image_level": idx.image_level, "n_colors": len(genomes), "n_sets": n_sets}

    stream = torch.cuda.current_stream(dev)
    n, L = args.reads, bench.READ_LEN
    bases_t = bench.gpu_reads(genomes, n, 12345, dev)
    T = bases_t.numel()
    off_t = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    W = n * (L - k + 1)
    res.update({"reads": n, "read_len": L, "windows": W})

    scr = {1: sets.screen(), 2: sets.screen()}
    need = {s: capi.screen_workspace_bytes(T, n, s) for s in (1, 2)}
    ws = torch.zeros(max(need[2], capi.pseudoalign_workspace_bytes(T, n, False), capi.search_workspace_bytes(T)), dtype=torch.uint8, device=dev)
    d_out = torch.empty(W, dtype=torch.int32, device=dev)
    d_ooff = torch.arange(n + 1, dtype=torch.int64, device=dev) * (L - k + 1)
    ids_t = torch.from_numpy(sets.copy()[0].astype(np.int64)).to(dev)
    t_hits = torch.zeros(n_sets, dtype=torch.int64, device=dev)
    t_seen = torch.zeros(idx.n_nodes, dtype=torch.bool, device=dev)
    rec8 = torch.empty(n, dtype=torch.int64, device=dev)
    colw = torch.empty((n, sets.words), dtype=torch.int64, device=dev)

    def search(streaming=False):                                 # (the add runs the non-streaming search)
        idx.streaming_search_dev_i32(bases_t.data_ptr(), T, off_t.data_ptr(), n, d_out.data_ptr(), d_ooff.data_ptr(), ws.data_ptr(),
                                     ws.numel(), stream.cuda_stream, streaming)

    def torch_route():
        search()
        cols = d_out[d_out >= 0].long()
        t_hits.add_(torch.bincount(ids_t[cols], minlength=n_sets))
        t_seen[cols] = True

    def add(strands):
        scr[strands].add_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, ws.data_ptr(), need[strands], strands, stream.cuda_stream)

    def pseudoalign():
        sets.pseudoalign_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, rec8.data_ptr(), colw.data_ptr(), 0, ws.data_ptr(), ws.numel(),
                             False, 1_000_000, 0, stream.cuda_stream)

    # ---- (a) and (b) give equal vectors: one add each on empty accumulators ----
    add(1)
    torch_route()
    torch.cuda.synchronize(dev)
    info = scr[1].info()
    set_kmers, set_seen, set_hits = scr[1].sets()
    seen_bits = np.unpackbits(scr[1].seen().view(np.uint8), bitorder="little")[:idx.n_nodes].astype(bool)
    h_seen = t_seen.cpu().numpy()
    if not (np.array_equal(set_hits, t_hits.cpu().numpy()) and np.array_equal(seen_bits, h_seen) and info["n_hits"] == int(t_hits.sum().item())
            and info["n_seen"] == int(h_seen.sum()) and info["n_windows"] == W
            and np.array_equal(set_seen, np.bincount(ids_t.cpu().numpy()[h_seen], minlength=n_sets))):
        raise SystemExit("Screen.add_dev and the torch route disagree")
    res["agree_with_torch_route"] = True
    res["one_batch"] = {"n_windows": info["n_windows"], "n_hits": info["n_hits"], "n_seen": info["n_seen"]}
    ref = scr[1].colors()
    res["per_color"] = {"ref_kmers": ref[0].tolist(), "ref_seen": ref[1].tolist(), "ref_hits": ref[2].tolist()}

    # ---- the legs, alternating, their order rotated from round to round ----
    legs = [("screen_add_dev_strands1", lambda: add(1)), ("screen_add_dev_strands2", lambda: add(2)), ("torch_route", torch_route),
            ("pseudoalign_sets_dev", pseudoalign), ("search_alone", search), ("streaming_search_alone", lambda: search(True))]
    times = {name: [] for name, _ in legs}
    for r in range(args.warmup + args.steps):
        order = legs[r % len(legs):] + legs[:r % len(legs)]
        for name, call in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
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
    a, bb, d = rows["screen_add_dev_strands1"]["median_ms"], rows["torch_route"]["median_ms"], rows["search_alone"]["median_ms"]
    rows["torch_route_over_screen_add"] = round(bb / a, 3)
    rows["screen_add_over_search"] = round(a / d, 3)
    rows["accumulate_ms_estimate"] = round(a - d, 3)
    rows["screen_add_is_faster_than_torch_route"] = bool(a < bb)
    res["legs"] = rows
    res["workspace_bytes"] = {"strands1": need[1], "strands2": need[2]}

    # ---- the queries ----
    def host_clock(call, reps=5):
        call()
        t = []
        for _ in range(reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            call()
            t.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "calls": len(t)}

    res["queries"] = {"sets": host_clock(scr[1].sets), "colors": host_clock(scr[1].colors), "info": host_clock(scr[1].info),
                      "sets_then_colors": host_clock(lambda: (scr[1].sets(), scr[1].colors()))}
    del bases_t, d_out, ws, rec8, colw, t_seen, ids_t
    torch.cuda.empty_cache()

    # ---- the expansion at scale: a synthetic object of many sets and 4096 colours ----
    S, C = args.synth_sets, 4096
    rng = np.random.default_rng(23)
    table = rng.integers(0, 2**64, size=(S, C // 64), dtype=np.uint64)
    table &= rng.integers(0, 2**64, size=(S, C // 64), dtype=np.uint64)
    table[0] = 0
    ids = rng.integers(0, S, size=idx.n_nodes).astype(np.uint32)
    with capi.ColorSets.from_arrays(idx, C, ids, table) as big, big.screen() as bs:
        res["expand"] = {"n_sets": S, "n_colors": C, "table_bytes": int(table.nbytes), "sets": host_clock(bs.sets, 3),
                         "colors": host_clock(bs.colors, 3)}
        res["expand"]["colors_minus_sets_ms"] = round(res["expand"]["colors"]["median_ms"] - res["expand"]["sets"]["median_ms"], 3)
        ref_kmers = bs.colors()[0]
        sizes = np.bincount(big.copy()[0], minlength=S).astype(np.int64)
        sizes[0] = 0
        probe = [0, 63, 64, 2000, 4095]
        want = [int(sizes[((table[:, c >> 6] >> np.uint64(c & 63)) & np.uint64(1)).astype(bool)].sum()) for c in probe]
        if [int(ref_kmers[c]) for c in probe] != want:
            raise SystemExit("the expansion of the synthetic object is wrong")
        res["expand"]["checked_colors"] = probe
    for s in scr.values():
        s.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
