"""Walks benchmark (sbwtgpu_unitigs_walks_dev): bench.py's config 2 index (three strains, k = 30) with
its three strains as colours, --reads reads of 150 bases (bench.gpu_reads), threaded through the coloured unitig graph.  In
ONE process, alternating, device events around every leg:

  (a) walks           sbwtgpu_unitigs_walks_dev
  (b) walks_cov       the same with unitig coverage
  (c) today           the route a user had before: sbwtgpu_search_dev (int64 results, what locate takes),
                      sbwtgpu_unitigs_locate_dev, then the step boundaries by torch ops on the two located arrays on the
                      device; "today_host" is the same route with the located arrays copied to the host and the boundaries in
                      numpy (host clock, --host-steps rounds)
  (d) read_hits       sbwtgpu_read_hits_dev on the same batch: the cheapest existing call of the same shape
  (e) search_i32      sbwtgpu_search_dev_i32 alone: what (a) spends before its own passes start, so (a) - (e) is their time
  (f) search_i64, locate   the two calls of (c) on their own, so that (c) splits into search, locate and the torch ops

--warmup rounds, then median and min-max of --steps; the order of the legs rotates from round to round.  Before any timing
the steps of (a) are compared with those of (c): they must be equal.  Prints one JSON line and writes it to --out.

  python tools/walks_bench.py [--reads 10000000] [--steps 7] [--warmup 2] [--host-steps 1] [--out profiles/walks_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(t):
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "calls": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-steps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walks_bench.json"))
    args = ap.parse_args()
    import torch
    import bench
    from sbwt_amd import capi, synth

    if capi.device_count() <= 0:
        raise SystemExit("walks_bench needs a GPU")
    lib = capi.lib()
    k = 30
    dev = torch.device("cuda", 0)
    genomes = synth.coli3_like(args.genome_len)
    bits = capi.build_bits_gpu([g.tobytes() for g in genomes], k, False, True, device=0)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)
    del bits
    with capi.ColorSetsBuilder.create(idx, len(genomes)) as bld:
        for c, g in enumerate(genomes):
            bld.add_sequences(c, g, np.array([0, len(g)], dtype=np.int64))
        sets = bld.finish()
    u = sets.unitig_graph_dev(links=False, column_map=True)
    t0 = time.perf_counter()
    u.walks_prepare()
    prepare_ms = (time.perf_counter() - t0) * 1e3
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream
    n, L = args.reads, bench.READ_LEN
    m = L - k + 1
    W = n * m
    bases_t = bench.gpu_reads(genomes, n, 12345, dev)
    T = bases_t.numel()
    off_t = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    ooff_t = torch.arange(n + 1, dtype=torch.int64, device=dev) * m

    cap = 8 * n
    wws = torch.zeros(capi.walks_workspace_bytes(T, n), dtype=torch.uint8, device=dev)
    step_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    steps = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    cov = torch.zeros(u.n_unitigs, dtype=torch.int64, device=dev)
    sws = torch.zeros(capi.search_workspace_bytes(T), dtype=torch.uint8, device=dev)
    res64 = torch.empty(W, dtype=torch.int64, device=dev)
    res32 = torch.empty(W, dtype=torch.int32, device=dev)
    loc_u = torch.empty(W, dtype=torch.int32, device=dev)
    loc_o = torch.empty(W, dtype=torch.int32, device=dev)
    rws = torch.zeros(capi.read_hits_workspace_bytes(T, n), dtype=torch.uint8, device=dev)
    rec = torch.empty((n, 4), dtype=torch.int32, device=dev)

    def walks(with_cov):
        u.walks_dev(idx, bases_t.data_ptr(), T, off_t.data_ptr(), n, step_off.data_ptr(), steps.data_ptr(), cap,
                    cov.data_ptr() if with_cov else 0, wws.data_ptr(), wws.numel(), sp)

    def search64():
        capi._check(lib.sbwtgpu_search_dev(idx.handle, bases_t.data_ptr(), T, off_t.data_ptr(), n, res64.data_ptr(), ooff_t.data_ptr(),
                                           sws.data_ptr(), sws.numel(), sp))

    def locate_only():                                            # (res64 holds the results of the search64 before)
        u.locate_dev(res64.data_ptr(), W, loc_u.data_ptr(), loc_o.data_ptr(), sp)

    def locate():
        search64()
        locate_only()

    def today():
        """(step_off, steps) from search + locate + torch ops on the located arrays"""
        locate()
        hit = loc_u != -1
        cont = hit[1:] & hit[:-1] & (loc_u[1:] == loc_u[:-1]) & (loc_o[1:] == loc_o[:-1] + 1)
        cont[ooff_t[1:-1] - 1] = False                            # a read's first window continues nothing
        start, end = hit.clone(), hit.clone()
        start[1:] &= ~cont
        end[:-1] &= ~cont
        pos, last = start.nonzero().squeeze(1), end.nonzero().squeeze(1)
        read = pos // m
        out = torch.stack([loc_u[pos], loc_o[pos], (pos - read * m).to(torch.int32), (last - pos + 1).to(torch.int32)], dim=1)
        return torch.searchsorted(pos, ooff_t), out

    def today_host():
        locate()
        hu, ho = loc_u.cpu().numpy(), loc_o.cpu().numpy()
        hit = hu != -1
        cont = hit[1:] & hit[:-1] & (hu[1:] == hu[:-1]) & (ho[1:] == ho[:-1] + 1)
        cont[np.arange(1, n, dtype=np.int64) * m - 1] = False
        start, end = hit.copy(), hit.copy()
        start[1:] &= ~cont
        end[:-1] &= ~cont
        pos, last = np.flatnonzero(start), np.flatnonzero(end)
        return np.searchsorted(pos, np.arange(n + 1, dtype=np.int64) * m), np.stack([hu[pos], ho[pos], (pos % m).astype(np.int32),
                                                                                       (last - pos + 1).astype(np.int32)], axis=1)

    # (a) and (c) give the same steps
    walks(True)
    want_off, want = today()
    n_steps = int(step_off[-1].item())
    if n_steps > cap:
        raise SystemExit("%d steps, room for %d" % (n_steps, cap))
    if not (torch.equal(step_off, want_off) and torch.equal(steps[:n_steps], want)):
        raise SystemExit("the steps of walks_dev and of search + locate + torch differ")
    if int(cov.sum().item()) != int(want[:, 3].sum(dtype=torch.int64).item()):
        raise SystemExit("coverage does not sum to the steps' k-mers")
    continued = int((want[1:, 2] == want[:-1, 2] + want[:-1, 3]).sum().item())
    del want_off, want

    legs = {"walks": lambda: walks(False), "walks_cov": lambda: walks(True), "today": today, "read_hits": lambda: idx.read_hits_dev(
                bases_t.data_ptr(), T, off_t.data_ptr(), n, rec.data_ptr(), rws.data_ptr(), rws.numel(), False, sp),
            "search_i32": lambda: idx.streaming_search_dev_i32(bases_t.data_ptr(), T, off_t.data_ptr(), n, res32.data_ptr(),
                                                                ooff_t.data_ptr(), sws.data_ptr(), sws.numel(), sp, streaming=False),
            "search_i64": search64, "locate": locate_only}
    names = list(legs)
    times = {name: [] for name in names}
    for s in range(args.warmup + args.steps):
        for name in names[s % len(names):] + names[:s % len(names)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            legs[name]()
            e1.record(stream)
            e1.synchronize()
            if s >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    host = []
    for s in range(args.host_steps):
        t0 = time.perf_counter()
        today_host()
        host.append((time.perf_counter() - t0) * 1e3)
    res = {"bench": "walks", "config": 2, "k": k, "n_nodes": idx.n_nodes, "n_unitigs": u.n_unitigs, "reads": n, "read_len": L, "windows": W,
           "found": round(float(cov.sum().item()) / (args.warmup + args.steps + 1) / W, 4), "n_steps": n_steps,
           "steps_per_read": round(n_steps / n, 3), "steps_continuing": continued, "prepare_ms": round(prepare_ms, 3),
           "workspace_bytes": wws.numel(), "steps": args.steps, "warmup": args.warmup}
    for name in names:
        res[name] = summary(times[name])
    if host:
        res["today_host"] = summary(host)
    med = {name: res[name]["median_ms"] for name in names}
    res["new_passes_ms"] = round(med["walks"] - med["search_i32"], 3)
    res["coverage_ms"] = round(med["walks_cov"] - med["walks"], 3)
    res["today_torch_ops_ms"] = round(med["today"] - med["search_i64"] - med["locate"], 3)
    res["today_over_walks"] = round(med["today"] / med["walks"], 3)
    res["walks_over_read_hits"] = round(med["walks"] / med["read_hits"], 3)
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
