"""Unitig-graph benchmark (sbwtgpu_unitigs_create_graph): bench.py's config 2 index (three strains,
k = 30) with its three strains as colours from the colour-set builder, built once outside the timing.  In ONE process,
alternating, for the plain run and for the coloured run:

  (a) create          sbwtgpu_unitigs_create / _create_colored        -- the calls the project had before, unchanged code
  (b) links           sbwtgpu_unitigs_create_graph, LINKS
  (c) links_map       sbwtgpu_unitigs_create_graph, LINKS | COLUMN_MAP
  (d) host_route      what a user did before: (a), copy the unitigs, the four extensions of every unitig's last k-mer
                      through sbwtgpu_search_batch, numpy.searchsorted of the hits on first_col
  (e) locate          sbwtgpu_unitigs_locate_dev over the streaming-search results of --reads reads of 150 bases (device
                      events), against a numpy gather of the copied map on the host (plain run only)

Host clock around each whole leg (all are synchronous), --warmup rounds, then median and min-max of --steps; the order of
(a), (b), (c) rotates from round to round, (d) ends the round, so no leg always follows the same one (what follows what
matters to the allocator: section 18).  With them the device event times the calls report themselves
(sbwtgpu_unitigs_stats, _graph_stats; medians).  Before any timing the links of (b) and of (d) are compared: they must be
equal.  No time is fixed in advance: (a) is compared with the figure of sections 10 and 18, (b) with (d) of the same run.
Writes one JSON line to --out and prints it.

  python tools/unitig_links_bench.py [--steps 7] [--warmup 2] [--reads 10000000] [--out profiles/unitig_links_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NONE = np.uint32(0xFFFFFFFF)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def host_route(idx, owner, k):
    """(link_off, link_to, ms of the search call alone): the links recomputed on the host from the unitigs."""
    with owner.unitigs_dev() as u:
        bases, off, first_col = u.copy()
    n = len(first_col)
    ext = np.empty((n, 4, k), dtype=np.uint8)
    ext[:, :, :k - 1] = bases[(off[1:] - (k - 1))[:, None] + np.arange(k - 1)][:, None, :]
    ext[:, :, k - 1] = ACGT[None, :]
    t0 = time.perf_counter()
    res, _ = idx.search(ext.reshape(-1), np.arange(4 * n + 1, dtype=np.int64) * k)
    search_ms = (time.perf_counter() - t0) * 1e3
    hit = res >= 0
    link_off = np.concatenate([[0], np.cumsum(hit.reshape(n, 4).sum(axis=1))]).astype(np.int64)
    link_to = np.searchsorted(first_col, res[hit]).astype(np.uint32)
    assert np.array_equal(first_col[link_to], res[hit]), "an out-neighbour of a tail is no first column"
    return link_off, link_to, search_ms


def summary(t):
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "calls": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reads", type=int, default=10_000_000, help="reads of 150 bases whose search results leg (e) locates")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unitig_links_bench.json"))
    args = ap.parse_args()
    import torch
    from sbwt_amd import capi, synth

    if capi.device_count() <= 0:
        raise SystemExit("unitig_links_bench needs a GPU")
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
    owners = {"plain": idx, "colored": sets}

    # (b) and (d) give the same links
    counts = {}
    for name, owner in owners.items():
        with owner.unitig_graph_dev(links=True, column_map=False) as u:
            lo, lt = u.links()
            counts[name] = {"n_unitigs": u.n_unitigs, "n_links": int(len(lt))}
        ho, ht, _ = host_route(idx, owner, k)
        assert np.array_equal(lo, ho) and np.array_equal(lt, ht), "%s: the links of the call and of the host route differ" % name

    legs = ("create", "links", "links_map", "host_route")
    wall = {(n, leg): [] for n in owners for leg in legs}
    dev = {(n, leg): [] for n in owners for leg in legs}
    for s in range(args.warmup + args.steps):
        for name, owner in owners.items():
            for leg in legs[s % 3:3] + legs[:s % 3] + legs[3:]:
                t0 = time.perf_counter()
                if leg == "host_route":
                    d = {"search_ms": host_route(idx, owner, k)[2]}
                else:
                    u = owner.unitigs_dev() if leg == "create" else owner.unitig_graph_dev(links=True, column_map=leg == "links_map")
                dt = (time.perf_counter() - t0) * 1e3
                if leg != "host_route":
                    assert u.n_kmers == n_kmers
                    d = {"passes_sum_ms": sum(u.stats()["pass_ms"].values())}
                    if leg != "create":
                        d.update(u.graph_stats())
                    u.close()
                if s >= args.warmup:
                    wall[(name, leg)].append(dt)
                    dev[(name, leg)].append(d)
    res = {"bench": "unitig_links", "config": 2, "k": k, "genome_len": args.genome_len, "steps": args.steps, "warmup": args.warmup,
           "n_nodes": idx.n_nodes, "n_kmers": n_kmers}
    for name in owners:
        res[name] = dict(counts[name])
        for leg in legs:
            res[name][leg] = summary(wall[(name, leg)])
            res[name][leg]["device_ms"] = {key: round(float(np.median([x[key] for x in dev[(name, leg)]])), 3) for key in dev[(name, leg)][0]}
        res[name]["links_minus_create_ms"] = round(res[name]["links"]["median_ms"] - res[name]["create"]["median_ms"], 3)
        res[name]["host_route_over_links"] = round(res[name]["host_route"]["median_ms"] / res[name]["links"]["median_ms"], 3)

    # (e) locate of search results on the device, against a numpy gather of the copied map
    read_len = 150
    bases, off = synth.sample_reads(genomes, args.reads, read_len, 0.01, 42)
    cols, _ = idx.streaming_search(bases, off)
    del bases, off
    with idx.unitig_graph_dev(links=False, column_map=True) as u:
        cu, co = u.column_map()
        d_cols = torch.from_numpy(cols).cuda()
        d_u = torch.empty(len(cols), dtype=torch.int32, device="cuda")
        d_r = torch.empty(len(cols), dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream()
        t_dev, t_host = [], []
        for s in range(args.warmup + args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            u.locate_dev(d_cols.data_ptr(), len(cols), d_u.data_ptr(), d_r.data_ptr(), stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            t0 = time.perf_counter()
            safe = np.where(cols >= 0, cols, 0)
            hu = np.where(cols >= 0, cu[safe], NONE)
            hr = np.where(cols >= 0, co[safe], NONE)
            dt = (time.perf_counter() - t0) * 1e3
            if s >= args.warmup:
                t_dev.append(e0.elapsed_time(e1))
                t_host.append(dt)
        assert np.array_equal(d_u.cpu().numpy().view(np.uint32), hu) and np.array_equal(d_r.cpu().numpy().view(np.uint32), hr)
    res["locate"] = {"reads": args.reads, "read_len": read_len, "n_results": int(len(cols)), "found": round(float((cols >= 0).mean()), 4),
                     "device": summary(t_dev), "numpy_gather": summary(t_host),
                     "gcols_per_s": round(len(cols) / (float(np.median(t_dev)) * 1e-3) / 1e9, 2)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)
    sets.close()
    idx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
