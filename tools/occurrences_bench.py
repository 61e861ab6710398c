"""Occurrences benchmark (sbwtgpu_occurrences_*): Occurrences.map_dev beside Positions.map_dev, beside the
route a user had without it and beside the calls it is built on, on bench.py's config 2 index (three strains, k = 30) with its
three strains as sequences 0 .. 2, in ONE process.  The tool draws the reads itself (bench.gpu_reads' recipe), so that every
read's strain of origin is known.

  legs     (a)  Occurrences.map_dev at --max-occ (16), with one strand and with two
           (b)  Positions.map_dev (the projection onto the first reference, section 26)
           (c)  the records of (a) entirely on the device without it: search_dev_i32, then torch -- a gather of the counts,
                repeat_interleave of the occurrences, the placement keys, a sort of (read, key), unique_consecutive with
                counts and a per-read arg-max (in slices of --slice reads, which bounds the sort's memory)
           (d)  ColorSets.pseudoalign_dev and (e) the search alone (sbwtgpu_search_dev_i32), for scale
           (f)  the builder: the add of the three strains + finish (host buffers: the host clock, the calls synchronise)
           The legs alternate and rotate their order from round to round; --warmup rounds, then median and min-max of --steps.
           Device events around each call.  Before any timing the records of (a) with one strand and of (c) are compared
           field for field and must be equal.
  reported without a gate: per call the share of reads whose winner is their strain of origin, or tied with it
           (votes2 == votes), for (a) and for (b); the reads per sequence; the reads that reach the second kernel; the bytes.

Exit status 1 when (a) and (c) disagree or when (a) with one strand is slower than (c).  Writes one JSON line to --out and
prints it.

  python tools/occurrences_bench.py [--reads N] [--steps 7] [--warmup 2] [--out profiles/occurrences_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def draw_reads(genomes, n_reads, seed, dev, read_len, sub_rate):
    """bench.gpu_reads' reads, and the genome each was drawn from"""
    import torch
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    lens = torch.tensor([len(g) for g in genomes], device=dev)
    starts = torch.tensor(np.concatenate([[0], np.cumsum([len(g) for g in genomes])[:-1]]), device=dev)
    cat = torch.from_numpy(np.concatenate(genomes)).to(dev)
    code = torch.zeros(256, dtype=torch.uint8, device=dev)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    code[acgt.long()] = torch.arange(4, dtype=torch.uint8, device=dev)
    out = torch.empty(n_reads * read_len, dtype=torch.uint8, device=dev)
    origin = torch.empty(n_reads, dtype=torch.int64, device=dev)
    ar = torch.arange(read_len, device=dev)
    chunk = 1 << 20
    for lo in range(0, n_reads, chunk):
        n = min(chunk, n_reads - lo)
        which = torch.randint(0, len(genomes), (n,), device=dev, generator=gen)
        u = torch.rand(n, device=dev, generator=gen, dtype=torch.float64)
        off = (u * (lens[which] - read_len + 1)).long() + starts[which]
        r = cat[(off[:, None] + ar[None, :]).reshape(-1)]
        hit = torch.rand(n * read_len, device=dev, generator=gen) < sub_rate
        shift = torch.randint(1, 4, (n * read_len,), device=dev, generator=gen, dtype=torch.uint8)
        sub = acgt[((code[r.long()] + shift) & 3).long()]
        out[lo * read_len:(lo + n) * read_len] = torch.where(hit, sub, r)
        origin[lo:lo + n] = which
    return out, origin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--slice", type=int, default=500_000)
    ap.add_argument("--max-occ", type=int, default=16)
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
           "map_table": capi.OCCURRENCES_MAP_TABLE, "max_occ": args.max_occ}

    # ---- (f) the builder: the three strains in one add, then finish; host buffers, the host clock ----
    ref_bases = np.concatenate(genomes)
    ref_off = np.concatenate([[0], np.cumsum([len(g) for g in genomes])]).astype(np.int64)
    build_ms, occ = [], None
    for r in range(args.warmup + args.steps):
        if occ is not None:
            occ.close()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        with idx.occurrences_builder() as ob:
            ob.add_sequences(ref_bases, ref_off, 0, 1)
            occ = ob.finish()
        if r >= args.warmup:
            build_ms.append((time.perf_counter() - t0) * 1e3)
    info = occ.info()
    res["table"] = {x: info[x] for x in ("n_windows", "n_hits", "n_occurrences", "n_positioned", "max_count", "device_bytes")}
    res["build_three_strains"] = {"median_ms": round(float(np.median(build_ms)), 3), "min_ms": round(min(build_ms), 3),
                                  "max_ms": round(max(build_ms), 3), "calls": len(build_ms), "clock": "host",
                                  "M_windows_per_s": round(info["n_windows"] / float(np.median(build_ms)) / 1e3, 2)}
    pos = occ.positions()
    res["positions_device_bytes"] = pos.info()["device_bytes"]

    stream = torch.cuda.current_stream(dev)
    n, L = args.reads, bench.READ_LEN
    Wr = L - k + 1
    bases_t, origin = draw_reads(genomes, n, 12345, dev, L, bench.SUB_RATE)
    T = bases_t.numel()
    off_t = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    W = n * Wr
    res.update({"reads": n, "read_len": L, "windows": W, "reads_drawn_per_seq": torch.bincount(origin, minlength=len(genomes)).tolist()})
    need = {s: capi.Occurrences.workspace_bytes(T, n, s) for s in (1, 2)}
    ws = torch.zeros(max(need[2], capi.Positions.workspace_bytes(T, n, 1), capi.pseudoalign_workspace_bytes(T, n, False),
                         capi.search_workspace_bytes(T)), dtype=torch.uint8, device=dev)
    d_rec = torch.zeros(n * 4, dtype=torch.int64, device=dev)
    d_res = torch.empty(W, dtype=torch.int32, device=dev)
    d_ooff = torch.arange(n + 1, dtype=torch.int64, device=dev) * Wr
    d_found = torch.zeros(n * 2, dtype=torch.int32, device=dev)
    d_colors = torch.zeros(n * sets.words, dtype=torch.int64, device=dev)
    offs_t = torch.from_numpy(occ.offsets().view(np.int64)).to(dev)
    keys_t = torch.from_numpy(occ.keys().view(np.int64)).to(dev)
    t_rec = torch.zeros((n, 7), dtype=torch.int64, device=dev)           # start seq strand votes votes2 n_found n_anchored
    ROW = 36                                                             # a placement key of sequences 0 .. 3 has 36 bits
    assert len(genomes) <= 4 and args.slice <= 1 << 26

    def search():
        idx.streaming_search_dev_i32(bases_t.data_ptr(), T, off_t.data_ptr(), n, d_res.data_ptr(), d_ooff.data_ptr(), ws.data_ptr(),
                                     ws.numel(), stream.cuda_stream, False)

    def torch_route():
        search()
        for lo in range(0, n, args.slice):
            hi = min(n, lo + args.slice)
            m = hi - lo
            v = d_res[lo * Wr:hi * Wr]
            hit = v >= 0
            vv = v.clamp(min=0).long()
            base = offs_t[vv]
            c = offs_t[vv + 1] - base
            c = torch.where(hit & (c <= args.max_occ), c, torch.zeros_like(c))
            src = torch.repeat_interleave(torch.arange(m * Wr, dtype=torch.int64, device=dev), c)      # the window of every vote
            j = torch.arange(len(src), dtype=torch.int64, device=dev) - (torch.cumsum(c, 0) - c)[src]
            f = keys_t[base[src] + j]
            row, i = src // Wr, src % Wr
            seq, p, t = f >> 32, (f & 0xFFFFFFFF) >> 1, f & 1
            start = torch.where(t == 0, p - i, p - (Wr - 1 - i))
            key = (row << ROW) | (seq << 33) | (t << 32) | (start + (1 << 31))
            key, _ = torch.sort(key)
            uniq, cnt = torch.unique_consecutive(key, return_counts=True)
            row = uniq >> ROW
            best = torch.zeros(m, dtype=torch.int64, device=dev).scatter_reduce(0, row, cnt, "amax")
            run = torch.arange(len(cnt), dtype=torch.int64, device=dev)
            cand = torch.where(cnt == best[row], run, torch.full_like(run, len(cnt)))
            win = torch.full((m,), len(cnt), dtype=torch.int64, device=dev).scatter_reduce(0, row, cand, "amin")      # keys ascend in a row
            has = win < len(cnt)
            wk = uniq[win.clamp(max=max(len(cnt) - 1, 0))] & ((1 << ROW) - 1)
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
            out[:, 5] = hit.view(m, Wr).sum(1)
            out[:, 6] = (c > 0).view(m, Wr).sum(1)

    def occ_map(strands):
        occ.map_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, d_rec.data_ptr(), ws.data_ptr(), need[strands], strands, args.max_occ,
                    stream.cuda_stream)

    def pos_map():
        pos.map_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, d_rec.data_ptr(), ws.data_ptr(), ws.numel(), 1, stream.cuda_stream)

    def pseudoalign():
        sets.pseudoalign_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, d_found.data_ptr(), d_colors.data_ptr(), 0, ws.data_ptr(), ws.numel(),
                             False, 1_000_000, 0, stream.cuda_stream)

    def records():
        rec32 = d_rec.view(torch.int32).view(n, 8)
        return torch.stack([d_rec.view(n, 4)[:, 0]] + [rec32[:, c].long() for c in range(2, 8)], dim=1)

    def origin_stats(got):
        placed = got[:, 1] >= 0
        right = got[:, 1] == origin
        tied = placed & ~right & (got[:, 3] == got[:, 4])
        return {"placed": int(placed.sum()), "winner_is_origin": int(right.sum()), "tied_with_another": int(tied.sum()),
                "share_origin_or_tied": round(float((right | tied).sum()) / n, 5), "share_winner_is_origin": round(float(right.sum()) / n, 5),
                "unique_best": int((got[:, 3] > got[:, 4]).sum()), "per_seq": [int((got[:, 1] == c).sum()) for c in range(len(genomes))],
                "votes_mean": round(float(got[:, 3].float().mean()), 2), "n_found": int(got[:, 5].sum()), "n_anchored": int(got[:, 6].sum())}

    # ---- (a) and (c) give equal records; what (a) and (b) say of the reads' origin ----
    occ_map(1)
    torch_route()
    torch.cuda.synchronize(dev)
    got = records()
    agree = torch.equal(got, t_rec)
    res["agree_with_torch_route"] = agree
    if not agree:
        bad = (got != t_rec).any(1).nonzero().flatten()
        res["disagree"] = {"reads": len(bad), "first": int(bad[0]), "map_dev": got[bad[0]].tolist(), "torch": t_rec[bad[0]].tolist()}
    res["occurrences_map"] = origin_stats(got)
    res["slow_list_reads"] = int(ws[capi.pseudoalign_workspace_bytes(T, n, False) + 255 & ~255:][:4].view(torch.int32)[0])
    res["slow_list_share"] = round(res["slow_list_reads"] / n, 7)
    pos_map()
    torch.cuda.synchronize(dev)
    res["positions_map"] = origin_stats(records())

    # ---- the legs, alternating, their order rotated from round to round ----
    legs = [("occ_map_dev_strands1", lambda: occ_map(1)), ("occ_map_dev_strands2", lambda: occ_map(2)), ("pos_map_dev", pos_map),
            ("torch_route", torch_route), ("pseudoalign_sets_dev", pseudoalign), ("search_alone", search)]
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
    a, pm, tr, d = (rows[x]["median_ms"] for x in ("occ_map_dev_strands1", "pos_map_dev", "torch_route", "search_alone"))
    rows["torch_route_over_occ_map_dev"] = round(tr / a, 3)
    rows["occ_map_pass_ms_estimate"] = round(a - d, 3)
    rows["pos_map_pass_ms_estimate"] = round(pm - d, 3)
    rows["occ_pass_over_pos_pass"] = round((a - d) / (pm - d), 3)
    res["legs"] = rows
    res["condition_map_dev_not_slower_than_torch_route"] = bool(a <= tr)
    res["workspace_bytes"] = {"strands1": need[1], "strands2": need[2]}
    pos.close()
    occ.close()
    sets.close()
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    sys.exit(0 if agree and a <= tr else 1)


if __name__ == "__main__":
    main()
