"""Verification benchmark (sbwtgpu_refseqs_*): RefSeqs.verify_dev on the records of Occurrences.map_dev,
beside the map call itself and beside the route a user had for the mismatches alone, on bench.py's config 2 index (three
strains, k = 30) with its three strains as sequences 0 .. 2, in ONE process.  The tool draws the reads itself, so that every
read's strain of origin is known: one set with substitutions only, a second one with one indel of 1 .. 3 bases in every tenth
read.

  legs     (a)  RefSeqs.verify_dev at --band (8) on the records of Occurrences.map_dev: mismatches AND edit distance
           (a2) the same on the second read set
           (b)  Occurrences.map_dev alone
           (c)  a torch route for the MISMATCHES ONLY: index arithmetic, a gather from the ASCII references on the device and
                a compare, in slices of --slice reads
           (d)  RefSeqs.add of the three strains (host buffers: the host clock, the call synchronises)
           The legs alternate and rotate their order from round to round; --warmup rounds, then median and min-max of --steps.
           Device events around each call.  Before any timing (a)'s mismatches are compared with (c)'s on every read, and (a)'s
           whole records with the brute force (tests/verify_brute.py) on a seeded sample of --sample reads of either set.
  reported without a gate: the share of reads with edit < mismatches, and the distribution of edit for the reads placed on and
           off their strain of origin, for either read set.

Exit status 1 when a comparison fails or when (a) is slower than (c).  Writes one JSON line to --out and prints it.

  python tools/verify_bench.py [--reads N] [--steps 7] [--warmup 2] [--out profiles/verify_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def draw_reads(genomes, n_reads, seed, dev, read_len, sub_rate, indel_share, planted=False):
    """reads of known origin: substitutions at sub_rate, and in indel_share of them one indel of 1 .. 3 bases (inserted into
    the read or deleted from it, at a random place); (bases, the genome of each, its offset there, whether it has an indel);
    planted: also the indel's length per read, positive for an insertion into the read, negative for a deletion, 0 for none"""
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
    at = torch.empty(n_reads, dtype=torch.int64, device=dev)
    has = torch.zeros(n_reads, dtype=torch.bool, device=dev)
    length = torch.zeros(n_reads, dtype=torch.int64, device=dev)
    ar = torch.arange(read_len, device=dev)
    chunk = 1 << 20
    for lo in range(0, n_reads, chunk):
        n = min(chunk, n_reads - lo)
        which = torch.randint(0, len(genomes), (n,), device=dev, generator=gen)
        u = torch.rand(n, device=dev, generator=gen, dtype=torch.float64)
        pos = (u * (lens[which] - read_len - 3 + 1)).long()                      # (room for a deletion of three bases)
        d = torch.randint(1, 4, (n,), device=dev, generator=gen)
        q = torch.randint(1, read_len - 4, (n,), device=dev, generator=gen)
        indel = torch.rand(n, device=dev, generator=gen) < indel_share
        ins = indel & (torch.rand(n, device=dev, generator=gen) < 0.5)
        dele = indel & ~ins
        j = ar[None, :].expand(n, read_len)
        behind_del = dele[:, None] & (j >= q[:, None])
        behind_ins = ins[:, None] & (j >= (q + d)[:, None])
        inside_ins = ins[:, None] & (j >= q[:, None]) & ~behind_ins
        src = j + torch.where(behind_del, d[:, None], torch.zeros_like(j)) - torch.where(behind_ins, d[:, None], torch.zeros_like(j))
        r = cat[((pos + starts[which])[:, None] + src).reshape(-1)]
        rnd = acgt[torch.randint(0, 4, (n * read_len,), device=dev, generator=gen)]
        r = torch.where(inside_ins.reshape(-1), rnd, r)
        hit = torch.rand(n * read_len, device=dev, generator=gen) < sub_rate
        shift = torch.randint(1, 4, (n * read_len,), device=dev, generator=gen, dtype=torch.uint8)
        sub = acgt[((code[r.long()] + shift) & 3).long()]
        out[lo * read_len:(lo + n) * read_len] = torch.where(hit, sub, r)
        origin[lo:lo + n] = which
        at[lo:lo + n] = pos
        has[lo:lo + n] = indel
        length[lo:lo + n] = torch.where(ins, d, torch.where(dele, -d, torch.zeros_like(d)))
    return (out, origin, at, has, length) if planted else (out, origin, at, has)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--slice", type=int, default=1_000_000)
    ap.add_argument("--max-occ", type=int, default=16)
    ap.add_argument("--band", type=int, default=8)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bench
    import verify_brute as vb
    from sbwt_amd import capi, synth

    k = 30
    genomes = synth.coli3_like(args.genome_len)
    dev = torch.device("cuda", 0)
    bits = capi.build_bits_gpu([g.tobytes() for g in genomes], k, False, True, device=0)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)
    del bits
    ref_bases = np.concatenate(genomes)
    ref_off = np.concatenate([[0], np.cumsum([len(g) for g in genomes])]).astype(np.int64)
    with idx.occurrences_builder() as ob:
        ob.add_sequences(ref_bases, ref_off, 0, 1)
        occ = ob.finish()
    res = {"config": 2, "k": k, "n_nodes": idx.n_nodes, "n_seqs": len(genomes), "band": args.band, "max_occ": args.max_occ}

    # ---- (d) the three strains into a new object; host buffers, the host clock ----
    add_ms, refs = [], None
    for r in range(args.warmup + args.steps):
        if refs is not None:
            refs.close()
        refs = capi.RefSeqs.create()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        refs.add_sequences(ref_bases, ref_off, 0)
        if r >= args.warmup:
            add_ms.append((time.perf_counter() - t0) * 1e3)
    info = refs.info()
    res["refseqs"] = info
    res["add_three_strains"] = {"median_ms": round(float(np.median(add_ms)), 3), "min_ms": round(min(add_ms), 3), "max_ms": round(max(add_ms), 3),
                                "calls": len(add_ms), "clock": "host", "G_bases_per_s": round(info["total_bases"] / float(np.median(add_ms)) / 1e6, 3)}

    stream = torch.cuda.current_stream(dev)
    n, L = args.reads, bench.READ_LEN
    T = n * L
    off_t = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    cat = torch.from_numpy(ref_bases).to(dev)
    g_start = torch.from_numpy(ref_off[:-1].copy()).to(dev)
    g_len = torch.tensor([len(g) for g in genomes], device=dev)
    comp = torch.zeros(256, dtype=torch.uint8, device=dev)                       # 0: an invalid base, which matches nothing
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    ident = torch.zeros(256, dtype=torch.uint8, device=dev)
    for a in b"ACGT":
        ident[a] = a
    need_map = capi.Occurrences.workspace_bytes(T, n, 1)
    need_ver = capi.RefSeqs.workspace_bytes(T, n)
    ws = torch.zeros(max(need_map, need_ver), dtype=torch.uint8, device=dev)
    d_out = torch.zeros(n * 2, dtype=torch.int64, device=dev)
    t_mm = torch.zeros(n, dtype=torch.int64, device=dev)
    ar = torch.arange(L, device=dev)
    sets = {}
    for name, share, seed in (("substitutions", 0.0, 12345), ("with_indels", 0.1, 54321)):
        bases_t, origin, at, has = draw_reads(genomes, n, seed, dev, L, bench.SUB_RATE, share)
        d_rec = torch.zeros(n * 4, dtype=torch.int64, device=dev)
        sets[name] = {"bases": bases_t, "origin": origin, "at": at, "indel": has, "rec": d_rec}

    def occ_map(s):
        occ.map_dev(s["bases"].data_ptr(), T, off_t.data_ptr(), n, s["rec"].data_ptr(), ws.data_ptr(), need_map, 1, args.max_occ,
                    stream.cuda_stream)

    def verify(s):
        refs.verify_dev(s["bases"].data_ptr(), T, off_t.data_ptr(), n, s["rec"].data_ptr(), d_out.data_ptr(), ws.data_ptr(), need_ver,
                        args.band, stream.cuda_stream)

    def torch_route(s):
        rec = s["rec"].view(n, 4)
        rec32 = s["rec"].view(torch.int32).view(n, 8)
        reads = s["bases"].view(n, L)
        for lo in range(0, n, args.slice):
            hi = min(n, lo + args.slice)
            start, seq, strand = rec[lo:hi, 0], rec32[lo:hi, 2].long(), rec32[lo:hi, 3].long()
            placed = seq >= 0
            sq = seq.clamp(min=0)
            p = start[:, None] + ar[None, :]
            inside = (p >= 0) & (p < g_len[sq][:, None])
            t = ident[cat[(g_start[sq][:, None] + p.clamp(min=0)).clamp(max=len(cat) - 1).reshape(-1)].long()].view(hi - lo, L)
            t = torch.where(inside, t, torch.zeros_like(t))
            fwd = ident[reads[lo:hi].reshape(-1).long()].view(hi - lo, L)
            rev = comp[reads[lo:hi].flip(1).reshape(-1).long()].view(hi - lo, L)
            r = torch.where((strand == 1)[:, None], rev, fwd)
            mm = ((t != r) | (t == 0)).sum(1)
            t_mm[lo:hi] = torch.where(placed, mm, torch.full_like(mm, -1))

    def out_records():
        o32 = d_out.view(torch.int32).view(n, 4)
        return d_out.view(n, 2)[:, 0].clone(), o32[:, 2].long(), o32[:, 3].long()      # ref_end, mismatches, edit

    # ---- before any timing: (a) against (c) on every read, (a) against the brute force on a sample ----
    refs_bytes = [g.tobytes() for g in genomes]
    ok = True
    rng = np.random.default_rng(2828)
    for name, s in sets.items():
        occ_map(s)
        verify(s)
        torch_route(s)
        torch.cuda.synchronize(dev)
        end, mm, edit = out_records()
        same = torch.equal(mm, t_mm)
        pick = np.sort(rng.choice(n, size=min(args.sample, n), replace=False))
        pk = torch.from_numpy(pick).to(dev)
        rec = s["rec"].view(n, 4)[pk].cpu().numpy()
        rec32 = rec.view(np.int32).reshape(len(pick), 8)
        rd = s["bases"].view(n, L)[pk].cpu().numpy()
        got = list(zip(end[pk].tolist(), mm[pk].tolist(), edit[pk].tolist()))
        want = [vb.record(refs_bytes, rd[i].tobytes(), (int(rec32[i, 2]), int(rec32[i, 3]), int(rec[i, 0])), args.band) for i in range(len(pick))]
        brute_ok = got == want
        ok = ok and same and brute_ok
        seq = s["rec"].view(torch.int32).view(n, 8)[:, 2].long()
        placed = seq >= 0
        on = placed & (seq == s["origin"])
        off_strain = placed & ~on

        def hist(mask):
            e = edit[mask]
            return {"reads": int(mask.sum()), "edit_mean": round(float(e.float().mean()), 3) if len(e) else None,
                    "edit_hist_0_to_15": torch.bincount(e.clamp(0, 15), minlength=16).tolist() if len(e) else None}
        sets[name]["report"] = {
            "mismatches_equal_torch_route": same, "sample_equals_brute_force": brute_ok, "sample": len(pick),
            "placed": int(placed.sum()), "at_origin": int((on & (s["rec"].view(n, 4)[:, 0] == s["at"])).sum()), "reads_with_indel": int(s["indel"].sum()),
            "share_edit_below_mismatches": round(float((placed & (edit < mm)).sum()) / n, 5),
            "share_edit_below_mismatches_among_indel_reads": round(float((placed & s["indel"] & (edit < mm)).sum()) / max(int(s["indel"].sum()), 1), 5),
            "mismatches_mean": round(float(mm[placed].float().mean()), 3), "edit_mean": round(float(edit[placed].float().mean()), 3),
            "on_strain_of_origin": hist(on), "off_strain_of_origin": hist(off_strain)}
        res[name] = sets[name]["report"]
    res["reads"], res["read_len"] = n, L

    # ---- the legs, alternating, their order rotated from round to round; the records of the sets stay what map_dev wrote ----
    s1, s2 = sets["substitutions"], sets["with_indels"]
    legs = [("verify_dev", lambda: verify(s1)), ("verify_dev_with_indels", lambda: verify(s2)), ("occ_map_dev", lambda: occ_map(s1)),
            ("torch_mismatches", lambda: torch_route(s1))]
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
        rows[name] = {"median_ms": round(med, 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "calls": len(t),
                      "M_reads_per_s": round(n / med / 1e3, 2)}
    a, c, b = (rows[x]["median_ms"] for x in ("verify_dev", "torch_mismatches", "occ_map_dev"))
    rows["torch_mismatches_over_verify_dev"] = round(c / a, 3)
    rows["verify_dev_over_occ_map_dev"] = round(a / b, 3)
    res["legs"] = rows
    verify(s1)
    torch.cuda.synchronize(dev)
    res["slow_list_reads"] = int(ws[:4].view(torch.int32)[0])
    res["condition_verify_dev_not_slower_than_torch_mismatches"] = bool(a <= c)
    res["workspace_bytes"] = {"verify": need_ver, "map": need_map}
    refs.close()
    occ.close()
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    sys.exit(0 if ok and a <= c else 1)


if __name__ == "__main__":
    main()
