"""Positions benchmark (sbwtgpu_positions_*): Positions.map_dev beside the route a user had before it and
beside the calls it is built on, on bench.py's config 2 index (three strains, k = 30) with its three strains as sequences
0 .. 2, and bench.gpu_reads for the reads, in ONE process.

  legs     (a)  Positions.add of the three strains (host buffers: the host clock, the call synchronises)
           (b)  Positions.map_dev with one strand and with two
           (c)  the same records entirely on the device without it: search_dev_i32, then torch -- a gather of the copied
                table, the placement keys, a sort of (read, key), unique_consecutive with counts and a per-read arg-max (in
                slices of --slice reads, which bounds the sort's memory)
           (d)  ColorSets.pseudoalign_dev, Index.read_hits_dev and the search alone (sbwtgpu_search_dev_i32), for scale
           The legs alternate and rotate their order from round to round; --warmup rounds, then median and min-max of --steps.
           Device events around each call.  Before any timing the records of (b) with one strand and of (c) are compared
           field for field and must be equal.

No time is fixed in advance.  Writes one JSON line to --out and prints it.

  python tools/positions_bench.py [--reads N] [--steps 7] [--warmup 2] [--out profiles/positions_bench.json]"""
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
    ap.add_argument("--slice", type=int, default=1_000_000)
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
    res = {"config": 2, "k": k, "n_nodes": idx.n_nodes, "image_level": idx.image_level, "n_seqs": len(genomes),
           "map_table": capi.POSITIONS_MAP_TABLE}

    # ---- (a) the table: the three strains in one add, host buffers ----
    ref_bases = np.concatenate(genomes)
    ref_off = np.concatenate([[0], np.cumsum([len(g) for g in genomes])]).astype(np.int64)
    pos = idx.positions()
    add_ms = []
    for r in range(args.warmup + args.steps):
        pos.reset()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        pos.add_sequences(ref_bases, ref_off, 0, 1)
        if r >= args.warmup:
            add_ms.append((time.perf_counter() - t0) * 1e3)
    info = pos.info()
    res["table"] = {x: info[x] for x in ("n_windows", "n_hits", "n_positioned", "device_bytes")}
    res["add_three_strains"] = {"median_ms": round(float(np.median(add_ms)), 3), "min_ms": round(min(add_ms), 3),
                                "max_ms": round(max(add_ms), 3), "calls": len(add_ms), "clock": "host",
                                "M_windows_per_s": round(info["n_windows"] / float(np.median(add_ms)) / 1e3, 2)}

    stream = torch.cuda.current_stream(dev)
    n, L = args.reads, bench.READ_LEN
    Wr = L - k + 1
    bases_t = bench.gpu_reads(genomes, n, 12345, dev)
    T = bases_t.numel()
    off_t = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    W = n * Wr
    res.update({"reads": n, "read_len": L, "windows": W})
    need = {s: capi.Positions.workspace_bytes(T, n, s) for s in (1, 2)}
    ws = torch.zeros(max(need[2], capi.pseudoalign_workspace_bytes(T, n, False), capi.read_hits_workspace_bytes(T, n, False),
                         capi.search_workspace_bytes(T)), dtype=torch.uint8, device=dev)
    d_rec = torch.zeros(n * 4, dtype=torch.int64, device=dev)
    d_res = torch.empty(W, dtype=torch.int32, device=dev)
    d_ooff = torch.arange(n + 1, dtype=torch.int64, device=dev) * Wr
    d_found = torch.zeros(n * 2, dtype=torch.int32, device=dev)
    d_colors = torch.zeros(n * sets.words, dtype=torch.int64, device=dev)
    d_hits = torch.zeros(n * 4, dtype=torch.int32, device=dev)
    first_t = torch.from_numpy(pos.first().view(np.int64)).to(dev)      # "no position" reads as -1
    t_rec = torch.zeros((n, 7), dtype=torch.int64, device=dev)           # start seq strand votes votes2 n_found n_anchored
    lane = torch.arange(Wr, dtype=torch.int64, device=dev)

    def search():
        idx.streaming_search_dev_i32(bases_t.data_ptr(), T, off_t.data_ptr(), n, d_res.data_ptr(), d_ooff.data_ptr(), ws.data_ptr(),
                                     ws.numel(), stream.cuda_stream, False)

    def torch_route():
        search()
        for lo in range(0, n, args.slice):
            hi = min(n, lo + args.slice)
            m = hi - lo
            v = d_res[lo * Wr:hi * Wr].view(m, Wr)
            hit = v >= 0
            f = first_t[v.clamp(min=0).long()]
            anch = hit & (f >= 0)
            seq, p, t = f >> 32, (f & 0xFFFFFFFF) >> 1, f & 1
            start = torch.where(t == 0, p - lane, p - (Wr - 1 - lane))
            parity = (torch.arange(lo, hi, dtype=torch.int64, device=dev) & 1).unsqueeze(1) << 62       # rows never merge
            key = torch.where(anch, (seq << 33) | (t << 32) | (start + (1 << 31)), torch.full_like(f, 1 << 61)) | parity
            key, _ = torch.sort(key, dim=1)
            uniq, cnt = torch.unique_consecutive(key.reshape(-1), return_counts=True)
            row = (torch.cumsum(cnt, 0) - cnt) // Wr
            real = (uniq & ((1 << 62) - 1)) != (1 << 61)
            cnt = torch.where(real, cnt, torch.zeros_like(cnt))
            best = torch.zeros(m, dtype=torch.int64, device=dev).scatter_reduce(0, row, cnt, "amax")
            run = torch.arange(len(cnt), dtype=torch.int64, device=dev)
            cand = torch.where(real & (cnt == best[row]), run, torch.full_like(run, len(cnt)))
            win = torch.full((m,), len(cnt), dtype=torch.int64, device=dev).scatter_reduce(0, row, cand, "amin")      # keys ascend in a row
            has = win < len(cnt)
            wk = uniq[win.clamp(max=len(cnt) - 1)] & ((1 << 62) - 1)
            rest = cnt.clone()
            rest[win[has]] = 0
            second = torch.zeros(m, dtype=torch.int64, device=dev).scatter_reduce(0, row, rest, "amax")
            zero = torch.zeros_like(best)
            out = t_rec[lo:hi]
            out[:, 0] = torch.where(has, (wk & 0xFFFFFFFF) - (1 << 31), zero)
            out[:, 1] = torch.where(has, wk >> 33, zero - 1)
            out[:, 2] = torch.where(has, (wk >> 32) & 1, zero)
            out[:, 3] = torch.where(has, best, zero)
            out[:, 4] = torch.where(has, second, zero)
            out[:, 5] = hit.sum(1)
            out[:, 6] = anch.sum(1)

    def map_dev(strands):
        pos.map_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, d_rec.data_ptr(), ws.data_ptr(), need[strands], strands, stream.cuda_stream)

    def pseudoalign():
        sets.pseudoalign_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, d_found.data_ptr(), d_colors.data_ptr(), 0, ws.data_ptr(), ws.numel(),
                             False, 1_000_000, 0, stream.cuda_stream)

    def read_hits():
        idx.read_hits_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, d_hits.data_ptr(), ws.data_ptr(), ws.numel(), False, stream.cuda_stream)

    # ---- (b) and (c) give equal records ----
    map_dev(1)
    torch_route()
    torch.cuda.synchronize(dev)
    rec32 = d_rec.view(torch.int32).view(n, 8)
    got = torch.stack([d_rec.view(n, 4)[:, 0]] + [rec32[:, c].long() for c in range(2, 8)], dim=1)
    if not torch.equal(got, t_rec):
        bad = (got != t_rec).any(1).nonzero().flatten()
        raise SystemExit("Positions.map_dev and the torch route disagree on %d reads, the first %d: %s against %s" %
                         (len(bad), int(bad[0]), got[bad[0]].tolist(), t_rec[bad[0]].tolist()))
    res["agree_with_torch_route"] = True
    res["one_batch"] = {"placed": int((got[:, 1] >= 0).sum()), "unique_best": int((got[:, 3] > got[:, 4]).sum()),
                        "votes_mean": round(float(got[:, 3].float().mean()), 2), "n_found": int(got[:, 5].sum()), "n_anchored": int(got[:, 6].sum()),
                        "per_seq": [int((got[:, 1] == c).sum()) for c in range(len(genomes))], "reverse": int((got[:, 2] == 1).sum())}
    res["slow_list_reads"] = int(ws[capi.pseudoalign_workspace_bytes(T, n, False) + 255 & ~255:][:4].view(torch.int32)[0])

    # ---- the legs, alternating, their order rotated from round to round ----
    legs = [("map_dev_strands1", lambda: map_dev(1)), ("map_dev_strands2", lambda: map_dev(2)), ("torch_route", torch_route),
            ("pseudoalign_sets_dev", pseudoalign), ("read_hits_dev", read_hits), ("search_alone", search)]
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
    a, tr, d = (rows[x]["median_ms"] for x in ("map_dev_strands1", "torch_route", "search_alone"))
    rows["torch_route_over_map_dev"] = round(tr / a, 3)
    rows["map_dev_over_search"] = round(a / d, 3)
    rows["map_pass_ms_estimate"] = round(a - d, 3)
    rows["pseudoalign_reduce_ms_estimate"] = round(rows["pseudoalign_sets_dev"]["median_ms"] - d, 3)
    res["legs"] = rows
    res["workspace_bytes"] = {"strands1": need[1], "strands2": need[2]}
    pos.close()
    sets.close()
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
