"""Pileup benchmark (sbwtgpu_pileup_*) in the setting of tools/align_bench.py: bench.py's config 2 index
(three strains, k = 30) with its strains as sequences 0 .. 2, reads of known origin at 1 % substitutions drawn by
verify_bench.draw_reads, placed by Occurrences.map_dev, band 8, ONE process.

  legs     add_aligned_dev (the accumulate pass alone, on align_dev's output), add_dev (verify + align + accumulate), align_dev
           alone, torch_route (the same table on the device with torch: the runs expanded with repeat_interleave, one index_add_
           per counter, in chunks of --torch-chunk reads), counts_dev of one whole strain, calls.  The legs rotate their order
           from round to round; --warmup rounds, then median and min-max of --steps.  Device events around each leg (calls: the
           host clock, it returns host memory).
  before any timing: the pileup's table equals the torch route's on every base of all three strains, and its scalars too.

Exit status 1 when the comparison fails.  Writes one JSON line to --out and prints it.  No gate on any time.

  python tools/pileup_bench.py [--reads N] [--steps 7] [--warmup 2] [--out profiles/pileup_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--max-occ", type=int, default=16)
    ap.add_argument("--band", type=int, default=8)
    ap.add_argument("--torch-chunk", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bench
    from sbwt_amd import capi, synth
    from verify_bench import draw_reads

    k = 30
    genomes = synth.coli3_like(args.genome_len)
    dev = torch.device("cuda", 0)
    bits = capi.build_bits_gpu([g.tobytes() for g in genomes], k, False, True, device=0)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)
    del bits
    ref_bases = np.concatenate(genomes)
    lens = [len(g) for g in genomes]
    ref_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    with idx.occurrences_builder() as ob:
        ob.add_sequences(ref_bases, ref_off, 0, 1)
        occ = ob.finish()
    refs = capi.RefSeqs.create()
    refs.add_sequences(ref_bases, ref_off, 0)
    pl = refs.pileup()
    res = {"config": 2, "k": k, "n_nodes": idx.n_nodes, "n_seqs": len(genomes), "band": args.band, "max_occ": args.max_occ}

    stream = torch.cuda.current_stream(dev)
    n, L = args.reads, bench.READ_LEN
    T = n * L
    total_ref = int(ref_off[-1])
    off_t = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    need_map = capi.Occurrences.workspace_bytes(T, n, 1)
    need_al = capi.RefSeqs.align_workspace_bytes(T, n)
    need_pl = capi.Pileup.workspace_bytes(T, n)
    ws = torch.zeros(max(need_map, need_al, need_pl), dtype=torch.uint8, device=dev)
    ops_cap = 16 * n
    d_ver = torch.zeros(n * 2, dtype=torch.int64, device=dev)
    d_out = torch.zeros(n * 2, dtype=torch.int64, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_ops = torch.zeros(ops_cap, dtype=torch.int32, device=dev)
    d_rec = torch.zeros(n * 4, dtype=torch.int64, device=dev)
    d_cnt = torch.zeros(max(lens) * 8, dtype=torch.int32, device=dev)
    bases_t = draw_reads(genomes, n, 12345, dev, L, bench.SUB_RATE, 0.0, planted=True)[0]
    occ.map_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, d_rec.data_ptr(), ws.data_ptr(), need_map, 1, args.max_occ, stream.cuda_stream)

    def align():
        refs.align_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, d_rec.data_ptr(), d_ver.data_ptr(), d_out.data_ptr(), d_off.data_ptr(),
                       d_ops.data_ptr(), ops_cap, ws.data_ptr(), need_al, args.band, stream.cuda_stream)

    def add_aligned():
        pl.add_aligned_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, d_rec.data_ptr(), d_ver.data_ptr(), d_out.data_ptr(), d_off.data_ptr(),
                           d_ops.data_ptr(), stream=stream.cuda_stream)

    def add_dev():
        pl.add_dev(bases_t.data_ptr(), T, off_t.data_ptr(), n, d_rec.data_ptr(), ws.data_ptr(), need_pl, args.band, stream=stream.cuda_stream)

    def counts_strain(s=0):
        pl.counts_dev(s, 0, lens[s], d_cnt.data_ptr(), stream.cuda_stream)
        return d_cnt[:lens[s] * 8].view(lens[s], 8)

    # ---- the torch route: the same table from align_dev's output ----
    lut = torch.full((256,), 4, dtype=torch.int64, device=dev)
    for ch, c in ((65, 0), (67, 1), (71, 2), (84, 3)):
        lut[ch] = c
    ref_code = lut[torch.from_numpy(ref_bases).to(dev).long()]
    seq_off = torch.from_numpy(ref_off).to(dev)
    seq_len = torch.tensor(lens, dtype=torch.int64, device=dev)
    rec32 = d_rec.view(torch.int32).view(n, 8)

    def torch_route():
        """(table int64[total_ref, 8] in the record's order, scalars) with repeat_interleave and index_add_"""
        tab = torch.zeros(total_ref * 8, dtype=torch.int64, device=dev)
        one = lambda m: torch.ones(m.numel(), dtype=torch.int64, device=dev)     # noqa: E731
        sc = {"n_piled": 0, "n_columns": 0, "n_clipped": 0, "n_overhang": 0}
        begin = d_out.view(n, 2)[:, 0]
        n_ops = d_out.view(torch.int32).view(n, 4)[:, 2].long()
        seq, strand = rec32[:, 2].long(), rec32[:, 3].long()
        for a in range(0, n, args.torch_chunk):
            b = min(n, a + args.torch_chunk)
            lo, hi = int(d_off[a]), int(d_off[b])
            sc["n_piled"] += int((n_ops[a:b] > 0).sum())
            if hi == lo:
                continue
            owner = torch.repeat_interleave(torch.arange(a, b, device=dev), d_off[a + 1:b + 1] - d_off[a:b])
            o = d_ops[lo:hi].long() & 0xffffffff
            ln, code = o >> 4, o & 15
            at = torch.arange(lo, hi, device=dev)
            edge = (at == d_off[owner]) | (at == d_off[owner + 1] - 1)
            radv, qadv = torch.where(code == 1, 0, ln), torch.where(code == 2, 0, ln)
            cr, cq = torch.cumsum(radv, 0) - radv, torch.cumsum(qadv, 0) - qadv
            first = d_off[owner] - lo
            p0, j0 = begin[owner] + cr - cr[first], cq - cq[first]
            g, nl = seq_off[seq[owner]], seq_len[seq[owner]]
            ins = code == 1
            sc["n_clipped"] += int(ln[ins & edge].sum())
            anchor = p0[ins & ~edge] - 1
            ok = (anchor >= 0) & (anchor < nl[ins & ~edge])
            sc["n_overhang"] += int((~ok).sum())
            cell = (g[ins & ~edge] + anchor)[ok]
            tab.index_add_(0, cell * 8 + 6, one(cell))
            r = torch.nonzero(~ins).squeeze(1)
            lr = ln[r]
            kk = torch.repeat_interleave(r, lr)
            t = torch.arange(kk.numel(), device=dev) - torch.repeat_interleave(torch.cumsum(lr, 0) - lr, lr)
            p, j, ck = p0[kk] + t, j0[kk] + t, code[kk]
            inside = (p >= 0) & (p < nl[kk])
            sc["n_overhang"] += int((~inside).sum())
            sc["n_columns"] += int(inside.sum())
            cell = g[kk] + p
            tab.index_add_(0, cell[inside] * 8, one(cell[inside]))
            m = inside & (ck == 7)
            tab.index_add_(0, cell[m] * 8 + 1 + ref_code[cell[m]], one(cell[m]))
            m = inside & (ck == 2)
            tab.index_add_(0, cell[m] * 8 + 5, one(cell[m]))
            m = inside & (ck == 8)
            rd, st = owner[kk[m]], strand[owner[kk[m]]]
            c = lut[bases_t[rd * L + torch.where(st != 0, L - 1 - j[m], j[m])].long()]
            c = torch.where((st != 0) & (c < 4), 3 - c, c)
            tab.index_add_(0, cell[m] * 8 + torch.where(c < 4, 1 + c, torch.full_like(c, 7)), one(c))
        return tab.view(total_ref, 8), sc

    # ---- before any timing: the table on every base of all three strains ----
    align()
    torch.cuda.synchronize(dev)
    total_runs = int(d_off[n])
    assert total_runs <= ops_cap, (total_runs, ops_cap)
    pl.reset()
    add_aligned()
    torch.cuda.synchronize(dev)
    want, sc = torch_route()
    info = pl.info()
    same = all(info[key] == v for key, v in sc.items()) and info["n_offered"] == n
    for s in range(len(genomes)):
        got = counts_strain(s).long() & 0xffffffff
        same = same and bool(torch.equal(got, want[int(ref_off[s]):int(ref_off[s + 1])]))
    res["table_equals_torch_route"] = same
    res["info"] = {key: int(v) for key, v in info.items()}
    res["reads"], res["read_len"], res["total_runs"] = n, L, total_runs
    del want

    timed_calls = {"n": 0}

    def calls():
        timed_calls["n"] = len(pl.calls(10, 3, 200000))

    legs = [("add_aligned_dev", add_aligned), ("add_dev", add_dev), ("align_dev", align), ("torch_route", torch_route),
            ("counts_dev_one_strain", counts_strain), ("calls", calls)]
    times = {name: [] for name, _ in legs}
    for r in range(args.warmup + args.steps):
        order = legs[r % len(legs):] + legs[:r % len(legs)]
        for name, fn in order:
            if name in ("add_aligned_dev", "add_dev"):
                pl.reset()                      # (the same table every time: no counter grows over the run)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 if name == "calls" else e0.elapsed_time(e1)
            if r >= args.warmup:
                times[name].append(ms)
    rows = {}
    for name, t in times.items():
        med = float(np.median(t))
        rows[name] = {"median_ms": round(med, 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "calls": len(t)}
    rows["add_aligned_dev_over_align_dev"] = round(rows["add_aligned_dev"]["median_ms"] / rows["align_dev"]["median_ms"], 4)
    rows["torch_route_over_add_aligned_dev"] = round(rows["torch_route"]["median_ms"] / rows["add_aligned_dev"]["median_ms"], 2)
    res["legs"] = rows
    res["n_calls_at_10_3_0.2"] = timed_calls["n"]
    res["workspace_bytes"] = {"pileup": need_pl, "align": need_al}
    pl.close()
    refs.close()
    occ.close()
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
