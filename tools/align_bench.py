"""Alignment benchmark (sbwtgpu_align_*): RefSeqs.align_dev on the records of Occurrences.map_dev, beside
RefSeqs.verify_dev alone (the forward pass that align_dev contains, and the yardstick: the project has no other route that
produces alignments) and beside the map call, in the setting of tools/verify_bench.py: bench.py's config 2 index (three
strains, k = 30) with its strains as sequences 0 .. 2, reads of known origin drawn by verify_bench.draw_reads, one set with
substitutions only and one with an indel of 1 .. 3 bases in every tenth read, ONE process.

  legs     align_dev and align_dev_with_indels (the two read sets), verify_dev, occ_map_dev.  The legs alternate and rotate
           their order from round to round; --warmup rounds, then median and min-max of --steps.  Device events around each call.
  before any timing: align_dev's verify records equal verify_dev's on every read of either set, and align_dev's whole output
           equals the brute force (tests/align_brute.py) on a seeded sample of --sample reads of either set.
  reported without a gate: the share of reads by edit class (the first kernel's band widths), the reads that reach the second
           kernel, the total number of runs, and the share of indel-carrying reads whose CIGAR holds an I or D run of the
           planted length.

Exit status 1 when a comparison fails.  Writes one JSON line to --out and prints it.

  python tools/align_bench.py [--reads N] [--steps 7] [--warmup 2] [--out profiles/align_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

EDIT_CLASSES = (("unaligned", -1, -1), ("0", 0, 0), ("1", 1, 1), ("2_3", 2, 3), ("4_7", 4, 7), ("8_15", 8, 15), ("16_31", 16, 31), ("32_up", 32, 1 << 30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--max-occ", type=int, default=16)
    ap.add_argument("--band", type=int, default=8)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import align_brute as ab
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
    ref_off = np.concatenate([[0], np.cumsum([len(g) for g in genomes])]).astype(np.int64)
    with idx.occurrences_builder() as ob:
        ob.add_sequences(ref_bases, ref_off, 0, 1)
        occ = ob.finish()
    refs = capi.RefSeqs.create()
    refs.add_sequences(ref_bases, ref_off, 0)
    res = {"config": 2, "k": k, "n_nodes": idx.n_nodes, "n_seqs": len(genomes), "band": args.band, "max_occ": args.max_occ}

    stream = torch.cuda.current_stream(dev)
    n, L = args.reads, bench.READ_LEN
    T = n * L
    off_t = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    need_map = capi.Occurrences.workspace_bytes(T, n, 1)
    need_ver = capi.RefSeqs.workspace_bytes(T, n)
    need_al = capi.RefSeqs.align_workspace_bytes(T, n)
    ws = torch.zeros(max(need_map, need_ver, need_al), dtype=torch.uint8, device=dev)
    ops_cap = 16 * n
    d_ver = torch.zeros(n * 2, dtype=torch.int64, device=dev)
    d_ver_only = torch.zeros(n * 2, dtype=torch.int64, device=dev)
    d_out = torch.zeros(n * 2, dtype=torch.int64, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_ops = torch.zeros(ops_cap, dtype=torch.int32, device=dev)
    sets = {}
    for name, share, seed in (("substitutions", 0.0, 12345), ("with_indels", 0.1, 54321)):
        bases_t, origin, at, has, planted = draw_reads(genomes, n, seed, dev, L, bench.SUB_RATE, share, planted=True)
        sets[name] = {"bases": bases_t, "indel": has, "planted": planted, "rec": torch.zeros(n * 4, dtype=torch.int64, device=dev)}

    def occ_map(s):
        occ.map_dev(s["bases"].data_ptr(), T, off_t.data_ptr(), n, s["rec"].data_ptr(), ws.data_ptr(), need_map, 1, args.max_occ,
                    stream.cuda_stream)

    def verify(s):
        refs.verify_dev(s["bases"].data_ptr(), T, off_t.data_ptr(), n, s["rec"].data_ptr(), d_ver_only.data_ptr(), ws.data_ptr(), need_ver,
                        args.band, stream.cuda_stream)

    def align(s):
        refs.align_dev(s["bases"].data_ptr(), T, off_t.data_ptr(), n, s["rec"].data_ptr(), d_ver.data_ptr(), d_out.data_ptr(), d_off.data_ptr(),
                       d_ops.data_ptr(), ops_cap, ws.data_ptr(), need_al, args.band, stream.cuda_stream)

    # ---- before any timing: the verify records on every read, the whole output against the brute force on a sample ----
    refs_bytes = [g.tobytes() for g in genomes]
    ok = True
    rng = np.random.default_rng(2929)
    for name, s in sets.items():
        occ_map(s)
        verify(s)
        torch.cuda.synchronize(dev)
        align(s)
        torch.cuda.synchronize(dev)
        same = torch.equal(d_ver, d_ver_only)
        total = int(d_off[n])
        pick = np.sort(rng.choice(n, size=min(args.sample, n), replace=False))
        pk = torch.from_numpy(pick).to(dev)
        rec = s["rec"].view(n, 4)[pk].cpu().numpy()
        rec32 = rec.view(np.int32).reshape(len(pick), 8)
        rd = s["bases"].view(n, L)[pk].cpu().numpy()
        ver = d_ver.view(n, 2)[pk].cpu().numpy().view(capi.READ_VERIFY_DTYPE).reshape(-1)
        out = d_out.view(n, 2)[pk].cpu().numpy().view(capi.READ_ALIGN_DTYPE).reshape(-1)
        lo, hi = d_off[pk].cpu().numpy(), d_off[pk + 1].cpu().numpy()
        brute_ok = total <= ops_cap
        for i in range(len(pick)):
            runs = ab.decode(d_ops[int(lo[i]):int(hi[i])].cpu().numpy().view(np.uint32))
            got = ((int(ver[i]["ref_end"]), int(ver[i]["mismatches"]), int(ver[i]["edit"])),
                   (int(out[i]["ref_begin"]), int(out[i]["n_ops"]), int(out[i]["n_eq"])), runs)
            want = ab.alignment(refs_bytes, rd[i].tobytes(), (int(rec32[i, 2]), int(rec32[i, 3]), int(rec[i, 0])), args.band)
            brute_ok = brute_ok and got == want
        ok = ok and same and brute_ok
        edit = d_ver.view(torch.int32).view(n, 4)[:, 3].long()
        n_slow = int((edit > 31).sum()) if L <= 256 else int((edit > 0).sum())    # the first kernel's limits: 31 edits, 256 bases
        classes = {nm: round(float(((edit >= a) & (edit <= b)).sum()) / n, 5) for nm, a, b in EDIT_CLASSES}
        # the indel-carrying reads whose runs hold an I (insertion into the read) or D run of the planted length
        counts = d_off[1:] - d_off[:-1]
        owner = torch.repeat_interleave(torch.arange(n, device=dev), counts)
        o = d_ops[:total].long() & 0xffffffff
        want_code = torch.where(s["planted"] > 0, torch.ones_like(s["planted"]), torch.full_like(s["planted"], 2))
        hit = ((o >> 4) == s["planted"].abs()[owner]) & ((o & 15) == want_code[owner]) & s["indel"][owner]
        found = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, owner, hit.long()) > 0
        n_indel = int(s["indel"].sum())
        res[name] = {"verify_records_equal_verify_dev": same, "sample_equals_brute_force": brute_ok, "sample": len(pick),
                     "share_by_edit": classes, "second_kernel_reads": n_slow, "share_second_kernel": round(n_slow / n, 7),
                     "total_runs": total, "runs_per_read": round(total / n, 3), "reads_with_indel": n_indel,
                     "share_indel_reads_with_the_planted_run": round(float(found.sum()) / max(n_indel, 1), 5)}
        del owner, o, hit, found
    res["reads"], res["read_len"] = n, L

    s1, s2 = sets["substitutions"], sets["with_indels"]
    legs = [("align_dev", lambda: align(s1)), ("align_dev_with_indels", lambda: align(s2)), ("verify_dev", lambda: verify(s1)),
            ("occ_map_dev", lambda: occ_map(s1))]
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
    rows["align_dev_over_verify_dev"] = round(rows["align_dev"]["median_ms"] / rows["verify_dev"]["median_ms"], 3)
    rows["align_dev_over_occ_map_dev"] = round(rows["align_dev"]["median_ms"] / rows["occ_map_dev"]["median_ms"], 3)
    res["legs"] = rows
    res["workspace_bytes"] = {"align": need_al, "verify": need_ver, "map": need_map}
    refs.close()
    occ.close()
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
