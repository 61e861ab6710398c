"""GPU: k-bounded matching statistics and the LCS array (sbwt_ms.hip) against the definition-level brute force
(tests/ms_brute.py) on small indexes, against GPU streaming_search and the oracle's update_interval at scale, and through the
C++ CLI."""
import gzip
import json
import os
import random
import subprocess
import threading

import numpy as np
import pytest

from bruteforce import BruteSBWT, int_to_words
from ms_brute import BruteMS, format_ms, lcs_array, probe_reads
from oracle import OracleIndex
from sbwt_amd import capi, hostlib, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_kats.json")))


def make_index(seqs, k, rc=False, ssup=True):
    if k == 1:                        # (the host builder starts at k = 2: the columns straight from the definition)
        B = BruteSBWT([s.decode() if isinstance(s, bytes) else s for s in seqs], k, rc)
        cols, sg = B.columns()
        n = len(B.nodes)
        w = [int_to_words(c, n) for c in cols]
        return None, capi.Index.create(w[0], w[1], w[2], w[3], int_to_words(sg, n) if ssup else None, n, k, len(B.kmers), 0)
    bits = hostlib.build_bits([s.encode() if isinstance(s, str) else s for s in seqs], k, rc, ssup)
    return bits, capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k,
                                   bits.n_kmers, 0)


def check_against_brute(idx, B, reads, label):
    M = BruteMS(B)
    assert idx.n_nodes == len(B.nodes), label
    assert np.array_equal(idx.lcs(), np.array(lcs_array(B), dtype=np.uint8)), label
    bases, off = capi.concat_reads(reads)
    ln, f, s = idx.matching_statistics(bases, off)
    ln2 = idx.matching_statistics(bases, off, intervals=False)
    assert np.array_equal(ln, ln2), label
    for r, read in enumerate(reads):
        L, F, S = M.read(read)
        a, b = off[r], off[r + 1]
        assert list(ln[a:b]) == L, (label, read)
        assert list(f[a:b]) == F and list(s[a:b]) == S, (label, read)


def test_fixture_indexes(gpu):
    c = KATS["cli_end_to_end"]
    rng = random.Random(1)
    _, idx = make_index(c["seqs"], c["k"], c["add_reverse_complements"])
    B = BruteSBWT(c["seqs"], c["k"], c["add_reverse_complements"])
    check_against_brute(idx, B, [q.encode() for q in c["queries"]] + probe_reads(c["seqs"], c["k"], rng), "cli_end_to_end")
    c = KATS["redundant_dummies"]
    _, idx = make_index(c["seqs"], c["k"])
    assert idx.n_nodes == c["n_subsets"] == 9
    check_against_brute(idx, BruteSBWT(c["seqs"], c["k"]), probe_reads(c["seqs"], c["k"], rng), "redundant_dummies")
    for case in KATS["small_cases"]["cases"]:
        _, idx = make_index(case["seqs"], case["k"])
        check_against_brute(idx, BruteSBWT(case["seqs"], case["k"]), probe_reads(case["seqs"], case["k"], rng), case["name"])


@pytest.mark.parametrize("k", [1, 2, 3, 4, 7, 15, 31, 32, 63, 64])
@pytest.mark.parametrize("ssup", [True, False])
def test_random_small_indexes(gpu, k, ssup):
    rng = random.Random(31 * k + ssup)
    for trial in range(3):
        seqs = ["".join(rng.choice("ACGT") for _ in range(rng.randint(k, 2 * k + 60))) for _ in range(rng.randint(1, 3))]
        rc = trial == 1
        _, idx = make_index(seqs, k, rc, ssup)
        check_against_brute(idx, BruteSBWT(seqs, k, rc), probe_reads(seqs, k, rng), (k, ssup, trial))


@pytest.mark.parametrize("knob", [("force_mega", 1, 0), ("big_path", 2, 1), ("image_level", 1, 0), ("image_level", 2, 0)])
def test_layouts_and_image_levels(gpu, knob):
    key, val, back = knob
    rng = random.Random(5)
    for k in (7, 15, 31):
        seqs = ["".join(rng.choice("ACGT") for _ in range(300)) for _ in range(2)]
        capi.set_tuning(key, val)
        try:
            _, idx = make_index(seqs, k, True)
        finally:
            capi.set_tuning(key, back)
        if key == "image_level":
            assert idx.image_level >= val       # (a tiny index may go one level further)
        check_against_brute(idx, BruteSBWT(seqs, k, True), probe_reads(seqs, k, rng), (knob, k))
    # a byte cap that forces level 2 leaves the LCS outside the image
    seqs = ["".join(rng.choice("ACGT") for _ in range(2000))]
    _, idx0 = make_index(seqs, 15)
    capi.set_tuning("image_level", 2)
    try:
        _, idx2 = make_index(seqs, 15)
    finally:
        capi.set_tuning("image_level", 0)
    capi.set_tuning("max_image_bytes", idx2.blob_bytes)
    try:
        _, idx = make_index(seqs, 15)
    finally:
        capi.set_tuning("max_image_bytes", 0)
    assert idx.image_level == 2
    idx.build_lcs()
    assert np.array_equal(idx.lcs(), idx0.lcs())


def scale_check(idx, orc, bases, off, k, streaming, n_sample, seed):
    ln, f, s = idx.matching_statistics(bases, off)
    if streaming:
        ss, oo = idx.streaming_search(bases, off)
    else:
        ss, oo = idx.search(bases, off)
    # the k-mer of position i is result oo[r] + (i - off[r] - k + 1)
    lens = np.diff(off)
    read_of = np.repeat(np.arange(len(lens)), lens)
    pos_in = np.arange(len(bases)) - off[read_of]
    has = pos_in >= k - 1
    slot = oo[read_of[has]] + pos_in[has] - (k - 1)
    want = np.full(len(bases), -1, dtype=np.int64)
    want[np.nonzero(has)[0]] = ss[slot]
    full = ln == k
    assert np.array_equal(full, want >= 0)
    assert np.array_equal(f[full], want[full]) and np.array_equal(s[full], want[full])
    assert 0.2 < full.mean() < 0.99, full.mean()
    # sampled positions: the oracle's update_interval of the matched suffix, and no match one base further left
    rng = np.random.default_rng(seed)
    n = idx.n_nodes
    for i in rng.integers(0, len(bases), size=n_sample):
        d = int(ln[i])
        r = read_of[i]
        if d == 0:
            assert (f[i], s[i]) == (0, n - 1)
            continue
        w = bases[i - d + 1:i + 1].tobytes()
        assert orc.update_interval(w, 0, n - 1) == (f[i], s[i]), i
        if d < k and i - d >= off[r] and bases[i - d] in b"ACGT":
            assert orc.update_interval(bases[i - d:i + 1].tobytes(), 0, n - 1)[0] == -1, i


@pytest.fixture(scope="module")
def config2():
    genomes = synth.coli3_like(5_000_000)
    bits = capi.build_bits_gpu([g.tobytes() for g in genomes], 30, False, True)
    orc = OracleIndex.from_bits(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, 30,
                                bits.n_kmers, 0)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, 30, bits.n_kmers, 0)
    return genomes, orc, idx


def test_config2_scale(gpu, config2):
    genomes, orc, idx = config2
    bases, off = synth.sample_reads(genomes, 1_000_000, 150, 0.01, 3)
    bases = synth.inject(bases, 200_000, ord("N"), 4)
    scale_check(idx, orc, bases, off, 30, True, 20_000, 5)


def test_k63_without_streaming_support(gpu):
    genomes = synth.coli3_like(1_000_000)
    bits = capi.build_bits_gpu([g.tobytes() for g in genomes], 63, False, False)
    orc = OracleIndex.from_bits(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], None, bits.n_nodes, 63, bits.n_kmers, 0)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], None, bits.n_nodes, 63, bits.n_kmers, 0)
    assert not idx.has_streaming_support
    bases, off = synth.sample_reads(genomes, 200_000, 150, 0.005, 6)
    bases = synth.inject(bases, 20_000, ord("N"), 7)
    scale_check(idx, orc, bases, off, 63, False, 20_000, 8)


def test_long_reads_match_single_reads(gpu, config2):
    genomes, _, idx = config2
    g = genomes[0]
    rng = np.random.default_rng(9)
    reads = []
    for ln in (100_000, 1_000_000, 250_001):
        a = int(rng.integers(0, len(g) - ln))
        r = synth.mutate(g[a:a + ln].copy(), 0.01, int(ln))
        reads.append(synth.inject(r, 50, ord("N"), 3).tobytes())
        sb, _ = synth.sample_reads(genomes, 7, 150, 0.02, int(ln) + 1)
        reads += [sb[j * 150:(j + 1) * 150].tobytes() for j in range(7)]
    got = idx.matching_statistics_reads(reads)
    for r, read in enumerate(reads):
        one = idx.matching_statistics_reads([read])[0]
        for a, b in zip(got[r], one):
            assert np.array_equal(a, b), r


def test_dev_threads_and_rank_only(gpu, config2):
    import torch
    genomes, _, idx = config2
    bases, off = synth.sample_reads(genomes, 50_000, 150, 0.02, 11)
    bases = synth.inject(bases, 5000, ord("N"), 12)
    ln, f, s = idx.matching_statistics(bases, off)
    dev = torch.device("cuda", 0)
    tb, to = torch.from_numpy(bases).to(dev), torch.from_numpy(off).to(dev)
    dl = torch.zeros(len(bases), dtype=torch.uint8, device=dev)
    df = torch.zeros(len(bases), dtype=torch.int64, device=dev)
    dsec = torch.zeros(len(bases), dtype=torch.int64, device=dev)
    ws = torch.zeros(capi.ms_workspace_bytes(len(bases)), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    idx.matching_statistics_dev(tb.data_ptr(), len(bases), to.data_ptr(), len(off) - 1, dl.data_ptr(), df.data_ptr(),
                                dsec.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(dl.cpu().numpy(), ln) and np.array_equal(df.cpu().numpy(), f) and np.array_equal(dsec.cpu().numpy(), s)
    st = idx.ms_workspace_stats(ws.data_ptr(), stream)
    assert st["positions"] == len(bases) and st["full"] == int((ln == 30).sum())
    dl.zero_()
    idx.matching_statistics_dev(tb.data_ptr(), len(bases), to.data_ptr(), len(off) - 1, dl.data_ptr(), 0, 0, ws.data_ptr(),
                                ws.numel(), stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(dl.cpu().numpy(), ln)
    with pytest.raises(capi.SbwtGpuError):
        idx.matching_statistics_dev(tb.data_ptr(), len(bases), to.data_ptr(), len(off) - 1, dl.data_ptr(), df.data_ptr(), 0,
                                    ws.data_ptr(), ws.numel(), stream)
    # two threads on a fresh handle whose LCS is not built yet
    bits = capi.build_bits_gpu([g.tobytes() for g in genomes[:1]], 30, False, True)
    fresh = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, 30, bits.n_kmers, 0)
    mine = genomes[0][:200_000].tobytes()
    ref = None
    out, errs = [None, None], []

    def work(t):
        try:
            out[t] = fresh.matching_statistics(*capi.concat_reads([mine] * 4))
        except Exception as e:        # noqa: BLE001 -- reported below
            errs.append(e)
    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    ref = idx.matching_statistics(*capi.concat_reads([mine] * 4))
    for o in out:
        # the fresh index holds one genome: its lengths are those of this genome's own k-mers, all k
        assert np.array_equal(o[0], ref[0]) and (o[0][29:200_000] == 30).all()
    # rank-only image
    w = np.random.default_rng(1).integers(0, 2**64, size=4, dtype=np.uint64)
    ro = capi.Index.create(w, w, w, w, None, 256, 3)
    with pytest.raises(capi.SbwtGpuError) as ei:
        ro.matching_statistics(*capi.concat_reads([b"ACGT"]))
    assert ei.value.code == capi.ERR_INVALID_ARG and "only rank()" in ei.value.msg
    with pytest.raises(capi.SbwtGpuError):
        ro.build_lcs()


def test_cli_matching_statistics(gpu, tmp_path):
    d = str(tmp_path)
    rng = np.random.default_rng(21)
    g = synth.random_genome(20_000, 21)
    with open(d + "/g.fna", "w") as fh:
        fh.write(">g\n" + g.tobytes().decode() + "\n")
    k = 21
    p = subprocess.run([SBWT, "build", "-i", d + "/g.fna", "-o", d + "/i.sbwt", "-k", str(k)], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    bits, idx = make_index([g.tobytes()], k)
    bases, off = synth.sample_reads([g], 300, 90, 0.03, 22)
    bases = synth.inject(bases, 100, ord("N"), 23)
    reads = [bases[off[r]:off[r + 1]].tobytes() for r in range(300)] + [g[:5].tobytes(), g[100:400].tobytes()]
    res = idx.matching_statistics_reads(reads)
    want_l = b"".join(format_ms(x[0]) for x in res)
    want_i = b"".join(format_ms(*x) for x in res)
    with open(d + "/r.fq", "w") as fh:
        for j, r in enumerate(reads):
            fh.write("@r%d\n%s\n+\n%s\n" % (j, r.decode(), "I" * len(r)))
    with open(d + "/r.fna", "w") as fh:
        for j, r in enumerate(reads):
            fh.write(">r%d\n%s\n" % (j, r.decode()))
    with open(d + "/r.fq", "rb") as src, gzip.open(d + "/r.fq.gz", "wb") as dst:
        dst.write(src.read())
    with open(d + "/in.txt", "w") as fh:
        fh.write(d + "/r.fna\n" + d + "/r.fq.gz\n")
    with open(d + "/out.txt", "w") as fh:
        fh.write(d + "/l1.out\n" + d + "/l2.out\n")
    for q in ("r.fq", "r.fna", "r.fq.gz"):
        for z in (False, True):
            for iv in (False, True):
                out = "%s/%s.%d%d.out" % (d, q, z, iv)
                cmd = [SBWT, "matching-statistics", "-i", d + "/i.sbwt", "-q", d + "/" + q, "-o", out]
                cmd += (["-z"] if z else []) + (["--intervals"] if iv else [])
                p = subprocess.run(cmd, capture_output=True, timeout=300)
                assert p.returncode == 0, p.stderr.decode()
                text = gzip.open(out).read() if z else open(out, "rb").read()
                assert text == (want_i if iv else want_l), (q, z, iv)
    p = subprocess.run([SBWT, "matching-statistics", "-i", d + "/i.sbwt", "-q", d + "/in.txt", "-o", d + "/out.txt",
                        "--batch-bases", "1000"], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    assert open(d + "/l1.out", "rb").read() == want_l and open(d + "/l2.out", "rb").read() == want_l
    p = subprocess.run([SBWT], capture_output=True, timeout=60)
    assert b"matching-statistics" in p.stderr
