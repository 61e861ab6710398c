"""Pseudoalignment benchmark: the colour layer (sbwtgpu_pseudoalign_dev / _batch, sbwtgpu_colors_add_batch) beside the calls it
is built on, on bench.py's config 2 index with its strains as colours and bench.gpu_reads for the reads, in ONE process.
Prints one JSON line:

  device   pseudoalign_dev with one and with two strands, with and without counts; streaming_search_dev_i32 and read_hits_dev
           on the same batch as the comparison: device events around each call, median of --steps
  host     pseudoalign_batch from pageable host buffers on --host-reads reads, and colors_add_batch per strain: host clock
           around the (synchronous) call

  wide     (--wide, instead of the above) the wide call beside the 64-colour call on the same batch: the three strains as
           colours 0, 70 and 130 of 192 (3 words a row), as colours 0, 1 and 2 of 64 through the wide call, and through the
           64-colour call; the three calls alternate, device events around each, medians of --steps

  sets     (--sets, instead of the above) colour-set objects beside the wide objects they were compressed from: the 64-colour
           call, wide and sets at 64 colours, at 192 (the strains on colours 0, 70, 130) and at 4096 (colours 0, 2000, 4095: the
           6.5 GB matrix is built, compressed, then timed); the seven calls alternate, device events around each, median and
           min-max of --steps; compress time, n_sets and device bytes per object; the gate of DESIGN.md section 15 at 192 and
           4096 colours: median(sets) <= median(wide) + (max - min of that wide call's timings)

  python tools/pseudoalign_bench.py [--reads N] [--host-reads N] [--steps 7] [--warmup 2] [--wide | --sets]
Kernel names and times: run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/pseudoalign_bench.py ...`."""
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
    ap.add_argument("--host-reads", type=int, default=2_000_000)
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--host-steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--sets", action="store_true")
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
    res = {"config": 2, "k": k, "n_nodes": idx.n_nodes, "image_level": idx.image_level, "n_colors": len(genomes)}
    if args.wide:
        print(json.dumps(wide_leg(args, torch, bench, capi, genomes, idx, k, dev, res)))
        return
    if args.sets:
        print(json.dumps(sets_leg(args, torch, bench, capi, genomes, idx, k, dev, res)))
        return

    # ---- colouring: one strain per colour, each genome one sequence ----
    col = capi.Colors.create(idx, len(genomes))
    add_rows = []
    for c, g in enumerate(genomes):
        off = np.array([0, len(g)], dtype=np.int64)
        t0 = time.perf_counter()
        nw, nh = col.add_sequences(c, g, off)
        dt = (time.perf_counter() - t0) * 1e3
        add_rows.append({"color": c, "ms": round(dt, 3), "n_windows": nw, "n_hit_windows": nh, "G_kmers_per_s": round(nw / dt / 1e6, 3)})
    info = col.info()
    res["colors_add_batch"] = add_rows
    res["colored_columns"] = info["n_colored_columns"]
    res["per_color"] = info["per_color"]
    res["rows_bytes"] = 8 * idx.n_nodes

    stream = torch.cuda.current_stream(dev)
    n = args.reads
    L = bench.READ_LEN
    bases_t = bench.gpu_reads(genomes, n, 12345, dev)
    T = bases_t.numel()
    off_t = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    W = n * (L - k + 1)
    res.update({"reads": n, "read_len": L, "kmers": W})

    def timed(call):
        times = []
        for s in range(args.warmup + args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            if s >= args.warmup:
                times.append(e0.elapsed_time(e1))
        med = float(np.median(times))
        return {"median_ms": round(med, 3), "min_ms": round(min(times), 3), "calls": len(times),
                "G_kmers_per_s": round(W / med / 1e6, 2)}

    # ---- device buffers: the comparison calls first ----
    dev_rows = {}
    d_out = torch.empty(W, dtype=torch.int32, device=dev)
    d_ooff = torch.arange(n + 1, dtype=torch.int64, device=dev) * (L - k + 1)
    ws = torch.zeros(capi.search_workspace_bytes(T), dtype=torch.uint8, device=dev)
    dev_rows["streaming_search_dev_i32"] = timed(lambda: idx.streaming_search_dev_i32(
        bases_t.data_ptr(), T, off_t.data_ptr(), n, d_out.data_ptr(), d_ooff.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream))
    found_search = int((d_out >= 0).sum().item())
    del ws, d_ooff, d_out
    rec4 = torch.empty((n, 4), dtype=torch.int32, device=dev)
    need = capi.read_hits_workspace_bytes(T, n, False)
    rws = torch.zeros(need, dtype=torch.uint8, device=dev)
    dev_rows["read_hits_dev"] = timed(lambda: idx.read_hits_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, rec4.data_ptr(), rws.data_ptr(),
                                                                need, False, stream.cuda_stream))
    del rws, rec4
    rec = torch.empty((n, 2), dtype=torch.int64, device=dev)
    cnt = torch.empty((n, len(genomes)), dtype=torch.int32, device=dev)
    for both in (False, True):
        need = capi.pseudoalign_workspace_bytes(T, n, both)
        pws = torch.zeros(need, dtype=torch.uint8, device=dev)
        for counts in (False, True):
            row = timed(lambda: col.pseudoalign_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, rec.data_ptr(), cnt.data_ptr() if counts else 0,
                                                    pws.data_ptr(), need, both, 1_000_000, 0, stream.cuda_stream))
            row["result_bytes"] = 16 * n + (4 * len(genomes) * n if counts else 0)
            row["workspace_bytes"] = need
            h = rec.cpu().numpy().view(capi.PSEUDOALIGNMENT_DTYPE).reshape(n)
            row["n_found"] = int(h["n_found"].sum(dtype=np.int64))
            row["reads_by_colors"] = {str(v): int(c) for v, c in zip(*np.unique(h["colors"], return_counts=True))}
            if not both and row["n_found"] != found_search:
                raise SystemExit("pseudoalign_dev found %d k-mers, the search %d" % (row["n_found"], found_search))
            dev_rows["pseudoalign_dev_strands%d%s" % (2 if both else 1, "_counts" if counts else "")] = row
        del pws
    s_ms, r_ms = dev_rows["streaming_search_dev_i32"]["median_ms"], dev_rows["read_hits_dev"]["median_ms"]
    p_ms = dev_rows["pseudoalign_dev_strands1"]["median_ms"]
    dev_rows["pseudoalign_over_search"] = round(p_ms / s_ms, 3)
    dev_rows["pseudoalign_over_read_hits"] = round(p_ms / r_ms, 3)
    dev_rows["reduce_ms_estimate"] = round(p_ms - s_ms, 3)
    dev_rows["found_matches_search"] = True
    res["device"] = dev_rows
    del rec, cnt
    # ---- host buffers (pageable) ----
    hn = min(args.host_reads, n)
    hb = bases_t[: hn * L].cpu().numpy()
    ho = np.arange(hn + 1, dtype=np.int64) * L
    hW = hn * (L - k + 1)
    del bases_t
    torch.cuda.empty_cache()
    times = []
    for s in range(1 + args.host_steps):                   # (one warm-up call: the staging buffers are made then)
        t0 = time.perf_counter()
        hrec = col.pseudoalign(hb, ho)
        dt = (time.perf_counter() - t0) * 1e3
        if s >= 1:
            times.append(dt)
    med = float(np.median(times))
    res["host"] = {"reads": hn, "kmers": hW, "input_bytes": int(hb.nbytes),
                   "pseudoalign_batch": {"median_ms": round(med, 3), "min_ms": round(min(times), 3), "calls": len(times),
                                         "G_kmers_per_s": round(hW / med / 1e6, 2), "result_bytes": 16 * hn,
                                         "n_found": int(hrec["n_found"].sum(dtype=np.int64))}}
    print(json.dumps(res))


def wide_leg(args, torch, bench, capi, genomes, idx, k, dev, res):
    """The same reads through sbwtgpu_pseudoalign_dev (64 colours), sbwtgpu_pseudoalign_wide_dev at 64 colours (1 word a row) and
    at 192 colours (3 words a row, the strains on colours 0, 70 and 130: one per word)."""
    wide_ids = (0, 70, 130)
    objs = {"narrow64": (capi.Colors.create(idx, 64), (0, 1, 2)), "wide64": (capi.WideColors.create(idx, 64), (0, 1, 2)),
            "wide192": (capi.WideColors.create(idx, 192), wide_ids)}
    for name, (col, ids) in objs.items():
        for c, g in zip(ids, genomes):
            col.add_sequences(c, g, np.array([0, len(g)], dtype=np.int64))
    res["wide_colors"] = {name: {"n_colors": col.n_colors, "words": getattr(col, "words", 1), "strain_colors": list(ids),
                                 "rows_bytes": 8 * idx.n_nodes * getattr(col, "words", 1)} for name, (col, ids) in objs.items()}
    stream = torch.cuda.current_stream(dev)
    n, L = args.reads, bench.READ_LEN
    bases_t = bench.gpu_reads(genomes, n, 12345, dev)
    T = bases_t.numel()
    off_t = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    W = n * (L - k + 1)
    res.update({"reads": n, "read_len": L, "kmers": W})
    rows = {}
    for both in (False, True):
        need = capi.pseudoalign_workspace_bytes(T, n, both)
        pws = torch.zeros(need, dtype=torch.uint8, device=dev)
        rec16 = torch.empty((n, 2), dtype=torch.int64, device=dev)
        rec8 = torch.empty(n, dtype=torch.int64, device=dev)
        colw = {name: torch.empty((n, getattr(col, "words", 1)), dtype=torch.int64, device=dev) for name, (col, _) in objs.items()}
        calls = {
            "narrow64": lambda: objs["narrow64"][0].pseudoalign_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, rec16.data_ptr(), 0,
                                                                    pws.data_ptr(), need, both, 1_000_000, 0, stream.cuda_stream)}
        for name in ("wide64", "wide192"):
            calls[name] = (lambda name=name: objs[name][0].pseudoalign_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, rec8.data_ptr(),
                                                                          colw[name].data_ptr(), 0, pws.data_ptr(), need, both,
                                                                          1_000_000, 0, stream.cuda_stream))
        times = {name: [] for name in calls}
        found, sets = {}, {}
        for s in range(args.warmup + args.steps):               # the three calls alternate
            for name, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                if s >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
                if s == 0:                                      # what each call found: the three must agree
                    if name == "narrow64":
                        h = rec16.cpu().numpy().view(capi.PSEUDOALIGNMENT_DTYPE).reshape(n)
                        found[name], words = h["n_found"].copy(), h["colors"].reshape(n, 1)
                    else:
                        found[name] = rec8.cpu().numpy().view(capi.READ_FOUND_DTYPE).reshape(n)["n_found"].copy()
                        words = colw[name].cpu().numpy().view(np.uint64)
                    ids = objs[name][1]
                    sets[name] = np.stack([(words[:, c >> 6] >> np.uint64(c & 63)) & np.uint64(1) for c in ids], axis=1)
        for name in ("wide64", "wide192"):
            if not (np.array_equal(found[name], found["narrow64"]) and np.array_equal(sets[name], sets["narrow64"])):
                raise SystemExit("%s and the 64-colour call disagree" % name)
        for name, t in times.items():
            med = float(np.median(t))
            rows["%s_strands%d" % (name, 2 if both else 1)] = {
                "median_ms": round(med, 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "calls": len(t),
                "G_kmers_per_s": round(W / med / 1e6, 2), "n_found": int(found[name].sum(dtype=np.int64)),
                "result_bytes": n * (16 if name == "narrow64" else 8 + 8 * objs[name][0].words)}
        for name in ("wide64", "wide192"):
            rows["%s_over_narrow64_strands%d" % (name, 2 if both else 1)] = round(
                rows["%s_strands%d" % (name, 2 if both else 1)]["median_ms"] / rows["narrow64_strands%d" % (2 if both else 1)]["median_ms"], 3)
        del pws, rec16, rec8, colw
    rows["results_agree"] = True
    res["wide"] = rows
    return res


def sets_leg(args, torch, bench, capi, genomes, idx, k, dev, res):
    """The same reads through sbwtgpu_pseudoalign_dev (64 colours), and through sbwtgpu_pseudoalign_wide_dev and
    sbwtgpu_pseudoalign_sets_dev at 64, 192 and 4096 colours, each colour-set object compressed from the wide object beside it."""
    strain_colors = {64: (0, 1, 2), 192: (0, 70, 130), 4096: (0, 2000, 4095)}
    objs = {"narrow64": (capi.Colors.create(idx, 64), strain_colors[64])}
    res["objects"] = {}
    for nc, ids in strain_colors.items():
        wide = capi.WideColors.create(idx, nc)
        for c, g in zip(ids, genomes):
            wide.add_sequences(c, g, np.array([0, len(g)], dtype=np.int64))
        if nc == 64:
            for c, g in zip(ids, genomes):
                objs["narrow64"][0].add_sequences(c, g, np.array([0, len(g)], dtype=np.int64))
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        sets = capi.ColorSets.from_colors(wide)                   # (synchronous: the host clock covers the whole call)
        compress_ms = (time.perf_counter() - t0) * 1e3
        info = sets.info()
        objs["wide%d" % nc], objs["sets%d" % nc] = (wide, ids), (sets, ids)
        res["objects"][str(nc)] = {"n_colors": nc, "words": wide.words, "strain_colors": list(ids), "wide_bytes": 8 * idx.n_nodes * wide.words,
                                   "sets_bytes": info["device_bytes"], "n_sets": info["n_sets"], "n_colored_columns": info["n_colored_columns"],
                                   "compress_ms": round(compress_ms, 3)}
    stream = torch.cuda.current_stream(dev)
    n, L = args.reads, bench.READ_LEN
    bases_t = bench.gpu_reads(genomes, n, 12345, dev)
    T = bases_t.numel()
    off_t = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    W = n * (L - k + 1)
    res.update({"reads": n, "read_len": L, "kmers": W})
    rows, gate = {}, {}
    rec16 = torch.empty((n, 2), dtype=torch.int64, device=dev)
    rec8 = torch.empty(n, dtype=torch.int64, device=dev)
    colw = {words: torch.empty((n, words), dtype=torch.int64, device=dev) for words in (1, 3, 64)}     # (shared by the calls of a width)
    for both in (False, True):
        st = 2 if both else 1
        need = capi.pseudoalign_workspace_bytes(T, n, both)
        pws = torch.zeros(need, dtype=torch.uint8, device=dev)
        calls = {"narrow64": lambda: objs["narrow64"][0].pseudoalign_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, rec16.data_ptr(), 0,
                                                                        pws.data_ptr(), need, both, 1_000_000, 0, stream.cuda_stream)}
        for name in objs:
            if name != "narrow64":
                calls[name] = (lambda name=name: objs[name][0].pseudoalign_dev(
                    bases_t.data_ptr(), T, off_t.data_ptr(), n, rec8.data_ptr(), colw[objs[name][0].words].data_ptr(), 0, pws.data_ptr(), need,
                    both, 1_000_000, 0, stream.cuda_stream))
        times = {name: [] for name in calls}
        found, strain_sets = {}, {}
        for s in range(args.warmup + args.steps):               # the seven calls alternate
            for name, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                if s >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
                if s == 0:                                      # what each call found: all must agree
                    if name == "narrow64":
                        h = rec16.cpu().numpy().view(capi.PSEUDOALIGNMENT_DTYPE).reshape(n)
                        found[name], words = h["n_found"].copy(), h["colors"].reshape(n, 1)
                    else:
                        found[name] = rec8.cpu().numpy().view(capi.READ_FOUND_DTYPE).reshape(n)["n_found"].copy()
                        words = colw[objs[name][0].words].cpu().numpy().view(np.uint64)
                    strain_sets[name] = np.stack([(words[:, c >> 6] >> np.uint64(c & 63)) & np.uint64(1) for c in objs[name][1]], axis=1)
                    del words
        for name in calls:
            if not (np.array_equal(found[name], found["narrow64"]) and np.array_equal(strain_sets[name], strain_sets["narrow64"])):
                raise SystemExit("%s and the 64-colour call disagree" % name)
        for name, t in times.items():
            med = float(np.median(t))
            rows["%s_strands%d" % (name, st)] = {
                "median_ms": round(med, 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "calls": len(t),
                "G_kmers_per_s": round(W / med / 1e6, 2), "n_found": int(found[name].sum(dtype=np.int64))}
        for nc in strain_colors:
            wide, sets = rows["wide%d_strands%d" % (nc, st)], rows["sets%d_strands%d" % (nc, st)]
            rows["sets%d_over_wide%d_strands%d" % (nc, nc, st)] = round(sets["median_ms"] / wide["median_ms"], 3)
            if nc != 64:                                        # (at 64 colours only reported)
                bound = wide["median_ms"] + (wide["max_ms"] - wide["min_ms"])
                gate["%d_strands%d" % (nc, st)] = {"sets_median_ms": sets["median_ms"], "wide_median_ms": wide["median_ms"],
                                                   "wide_spread_ms": round(wide["max_ms"] - wide["min_ms"], 3), "bound_ms": round(bound, 3),
                                                   "passed": bool(sets["median_ms"] <= bound)}
        del pws
    rows["results_agree"] = True
    res["sets"] = rows
    res["gate"] = gate
    res["gate_passed"] = all(g["passed"] for g in gate.values())
    return res


if __name__ == "__main__":
    main()
