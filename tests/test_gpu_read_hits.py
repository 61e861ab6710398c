"""GPU: per-read hit profiles (sbwt_readhits.hip) against the definition-level brute force (tests/read_hits_brute.py) on small
indexes, against a numpy reduction of the GPU's own search at scale, at the word and threshold edges of the reducer, through
the device entry point and through the C++ CLI."""
import gzip
import json
import os
import random
import subprocess
import threading

import numpy as np
import pytest

from bruteforce import BruteSBWT
from read_hits_brute import format_table, profile_of_hits, profiles, reduce_hits, revcomp
from sbwt_amd import capi, hostlib, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_kats.json")))


def make_index(seqs, k, rc=False, ssup=True):
    bits = hostlib.build_bits([s.encode() if isinstance(s, str) else s for s in seqs], k, rc, ssup)
    return capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)


class tuning:
    """set_tuning for the length of a with-block"""

    def __init__(self, key, value, back):
        self.key, self.value, self.back = key, value, back

    def __enter__(self):
        capi.set_tuning(self.key, self.value)

    def __exit__(self, *exc):
        capi.set_tuning(self.key, self.back)


def probe_reads(seqs, k, rng):
    """Reads that exercise a small index: its sequences and pieces of them, their reverse complements, substitutions, N and
    lower case, reads shorter than k, of exactly k bases and empty."""
    reads = [b"", b"A", b"ACGT"[:k - 1], b"N" * (k + 2)]
    for s in seqs:
        s = s if isinstance(s, str) else s.decode()
        reads += [s.encode(), revcomp(s).encode(), s[:k].encode(), s[-k:].encode()]
        for _ in range(6):
            a = rng.randrange(0, len(s))
            piece = list(s[a:a + rng.randint(0, k + 40)])
            for _ in range(rng.randint(0, 3)):
                if piece:
                    piece[rng.randrange(len(piece))] = rng.choice("ACGTNacgt")
            piece = "".join(piece)
            reads += [piece.encode(), revcomp(piece).encode()]
    reads.append("".join(rng.choice("ACGT") for _ in range(3 * k + 70)).encode())
    return reads


def check_against_brute(idx, B, reads, label):
    for both in (False, True):
        got = idx.read_hits_reads(reads, both)
        want = np.array(profiles(B.kmers, B.k, reads, 2 if both else 1), dtype=np.int32).reshape(len(reads), 4)
        assert got.dtype == np.int32 and got.shape == (len(reads), 4), label
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (label, both, reads[bad[0]], got[bad[0]], want[bad[0]])


def test_fixture_indexes(gpu):
    rng = random.Random(1)
    c = KATS["cli_end_to_end"]
    for rc in (True, False):
        idx = make_index(c["seqs"], c["k"], rc)
        check_against_brute(idx, BruteSBWT(c["seqs"], c["k"], rc), [q.encode() for q in c["queries"]] + probe_reads(c["seqs"], c["k"], rng),
                            ("cli_end_to_end", rc))
    for case in KATS["small_cases"]["cases"] + [KATS["redundant_dummies"], KATS["api_example"]]:
        for ssup in (True, False):
            idx = make_index(case["seqs"], case["k"], False, ssup)
            check_against_brute(idx, BruteSBWT(case["seqs"], case["k"]), probe_reads(case["seqs"], case["k"], rng),
                                (case.get("name"), ssup))


@pytest.mark.parametrize("k", [2, 3, 7, 31, 32, 63, 64])
@pytest.mark.parametrize("ssup", [True, False])
def test_random_small_indexes(gpu, k, ssup):
    rng = random.Random(37 * k + ssup)
    for trial in range(2):
        seqs = ["".join(rng.choice("ACGT") for _ in range(rng.randint(k, 2 * k + 60))) for _ in range(rng.randint(1, 3))]
        rc = trial == 1
        idx = make_index(seqs, k, rc, ssup)
        check_against_brute(idx, BruteSBWT(seqs, k, rc), probe_reads(seqs, k, rng), (k, ssup, trial))


def mirrored_hits(idx, bases, off):
    """hit flags of the reverse complements of all windows, in forward window order, from a search of the mirrored batch"""
    comp = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    rcb = comp[bases[::-1]]
    T = len(bases)
    roff = (T - off[::-1]).astype(np.int64)
    res, _ = idx.search_i32(np.ascontiguousarray(rcb), roff, streaming=False)
    return (res >= 0)[::-1]


def want_from_search(idx, bases, off, both):
    res, oo = idx.search_i32(bases, off, streaming=False)
    hit = res >= 0
    if both:
        hit = hit | mirrored_hits(idx, bases, off)
    return reduce_hits(hit, oo, idx.k), hit, oo


def test_reduce_hits_helper_matches_the_definition():
    rng = np.random.default_rng(2)
    for k in (1, 4, 30):
        m = rng.integers(0, 70, size=200)
        oo = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
        hit = rng.random(int(oo[-1])) < rng.choice([0.1, 0.5, 0.9], size=int(oo[-1]))
        got = reduce_hits(hit, oo, k)
        for r in range(200):
            assert tuple(got[r]) == profile_of_hits([int(x) for x in hit[oo[r]:oo[r + 1]]], k), (k, r)


K_SCALE = 21


@pytest.fixture(scope="module")
def genome_set():
    g0 = synth.random_genome(50_000, 1)
    genomes = [g0, synth.mutate(g0, 0.05, 2)]
    fwd = make_index([g.tobytes() for g in genomes], K_SCALE, False)
    closed = make_index([g.tobytes() for g in genomes], K_SCALE, True)
    return genomes, fwd, closed


def ragged_batch(genomes, n, seed):
    bases, off = synth.ragged_reads(genomes, n, 0, 400, 0.02, seed)
    bases = synth.inject(bases, n // 4, ord("N"), seed + 1)
    bases = synth.inject(bases, n // 8, ord("a"), seed + 2)
    # every other read from the reverse strand
    comp = np.arange(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    for r in range(0, n, 2):
        a, b = off[r], off[r + 1]
        bases[a:b] = comp[bases[a:b][::-1]]
    return bases, off


def test_ragged_reads_against_own_search(gpu, genome_set):
    genomes, fwd, _ = genome_set
    bases, off = ragged_batch(genomes, 20_000, 5)
    for both in (False, True):
        want, hit, oo = want_from_search(fwd, bases, off, both)
        got = fwd.read_hits(bases, off, both)
        assert np.array_equal(got, want), both
        assert 0.05 < hit.mean() < 0.95
        # the reduction itself against the definition, on a sample of the reads
        for r in np.random.default_rng(6).integers(0, len(off) - 1, size=200):
            assert tuple(got[r]) == profile_of_hits([int(x) for x in hit[oo[r]:oo[r + 1]]], K_SCALE)
    assert (fwd.read_hits(bases, off, True)[:, 1] > fwd.read_hits(bases, off, False)[:, 1]).any()


def pattern_read(kind, m, rng):
    """A read of m windows at k = 2 over the k-mer set {AC, GG} whose hits follow `kind`."""
    L = m + 1 if m > 0 else rng.randint(0, 1)
    if kind == "all":
        s = "G" * L
    elif kind == "none":
        s = "T" * L
    elif kind == "alternating":
        s = ("AC" * (L // 2 + 1))[:L]
    elif kind == "run":                  # one run in the middle (it crosses a word boundary wherever the read lies)
        a = rng.randint(0, L // 3)
        b = rng.randint(2 * L // 3, L)
        s = "T" * a + "G" * (b - a) + "T" * (L - b)
    else:                                # one hit at each end
        s = "AC" + "T" * (L - 4) + "AC" if L >= 4 else "T" * L
    assert len(s) == L
    return s.encode()


def test_word_and_threshold_edges(gpu):
    k = 2
    seqs = ["AC", "GG"]
    B = BruteSBWT(seqs, k)
    assert B.kmers == {"AC", "GG"}
    idx = make_index(seqs, k)
    rng = random.Random(8)
    reads, cur = [], 0
    for kind in ("all", "none", "alternating", "run", "ends"):
        for m in (0, 1, 63, 64, 65, 127, 128, 129):          # (127 / 128 / 129: the threshold set below -1 / +0 / +1)
            for bit in range(64):
                fill = (bit - cur) % 64                       # a filler read puts the next read's first result at bit `bit`
                if fill:
                    reads.append(b"T" * (fill + 1))
                    cur += fill
                assert cur % 64 == bit
                reads.append(pattern_read(kind, m, rng))
                cur += m
    want = np.array(profiles(B.kmers, k, reads), dtype=np.int32)
    assert want[:, 3].max() == 129 and (want[:, 2] == 130).any()
    bases, off = capi.concat_reads(reads)
    for wave_min, back in ((1024, 1024), (128, 1024), (1, 1024)):        # all by lanes; both sides of 128; all by waves
        with tuning("read_hits_wave_min", wave_min, back):
            got = idx.read_hits(bases, off)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (wave_min, reads[bad[0]], got[bad[0]], want[bad[0]])
    with tuning("read_hits_wave_min", 128, 1024):
        assert np.array_equal(idx.read_hits(bases, off, True), np.array(profiles(B.kmers, k, reads, 2), dtype=np.int32))


def long_read_batch(genomes):
    g0 = genomes[0]
    long_read = np.concatenate([g0[:50_000], synth.mutate(g0, 0.01, 11), synth.mutate(g0, 0.002, 12), g0[10_000:50_000],
                                synth.mutate(g0, 0.05, 13), synth.mutate(g0, 0.01, 14), g0[:10_000]])
    assert len(long_read) == 300_000
    sb, so = synth.sample_reads(genomes, 40, 150, 0.02, 15)
    short = [sb[so[r]:so[r + 1]].tobytes() for r in range(40)]
    mid = synth.mutate(g0[20_000:25_019], 0.003, 16).tobytes()           # 5000 windows less one: a lane's read below
    reads = short[:20] + [long_read.tobytes()] + short[20:30] + [mid] + short[30:]
    return capi.concat_reads(reads)


def test_one_long_read_among_short_ones(gpu, genome_set):
    genomes, fwd, _ = genome_set
    bases, off = long_read_batch(genomes)
    want, hit, oo = want_from_search(fwd, bases, off, False)
    r_long = 20
    assert want[r_long, 0] == 300_000 - K_SCALE + 1 and want[r_long, 3] >= 50_000 - K_SCALE + 1 > 4096 * 2
    got = fwd.read_hits(bases, off)
    assert np.array_equal(got, want)
    assert tuple(got[r_long]) == profile_of_hits([int(x) for x in hit[oo[r_long]:oo[r_long + 1]]], K_SCALE)
    with tuning("read_hits_wave_min", 1 << 30, 1024):                      # lanes take the 4999-window and the long read
        assert np.array_equal(fwd.read_hits(bases, off), want)
    with tuning("read_hits_wave_min", 64, 1024):
        assert np.array_equal(fwd.read_hits(bases, off), want)
    want2, _, _ = want_from_search(fwd, bases, off, True)
    assert np.array_equal(fwd.read_hits(bases, off, True), want2)


def test_both_strands(gpu, genome_set):
    genomes, fwd, closed = genome_set
    bases, off = ragged_batch(genomes, 3000, 21)
    # an index built with reverse complements: the second strand adds nothing
    one, two = closed.read_hits(bases, off), closed.read_hits(bases, off, True)
    assert np.array_equal(one, two) and one[:, 1].sum() > 0
    # a forward-only index: the profile of rc(read) is that of the read, and the second strand only adds hits
    reads = [bases[off[r]:off[r + 1]].tobytes() for r in range(len(off) - 1)]
    rc_reads = [revcomp(r.decode()).encode() for r in reads]
    f1, f2 = fwd.read_hits(bases, off), fwd.read_hits(bases, off, True)
    assert np.array_equal(fwd.read_hits_reads(rc_reads, True), f2)
    assert (f2[:, 1] >= f1[:, 1]).all() and (f2[:, 1] > f1[:, 1]).any()
    assert np.array_equal(f2, one)                       # = one strand on the closed index
    # a window holding N is no hit in either mode: one N in a read of the genome takes exactly k windows away
    g = genomes[0]
    clean = g[1000:1200].copy()
    with_n = clean.copy()
    with_n[100] = ord("N")
    for idx in (fwd, closed):
        for both in (False, True):
            a = idx.read_hits_reads([clean.tobytes(), with_n.tobytes()], both)
            m = 200 - K_SCALE + 1
            assert tuple(a[0]) == (m, m, 200, m)
            assert tuple(a[1]) == (m, m - K_SCALE, 199, 100 - K_SCALE + 1)
    got = fwd.read_hits_reads([synth.revcomp(with_n).tobytes()], True)
    assert tuple(got[0]) == (180, 180 - K_SCALE, 199, 100 - K_SCALE + 1)
    assert fwd.read_hits_reads([synth.revcomp(clean).tobytes()], False)[0, 1] < 180


def test_chunking(gpu, genome_set):
    genomes, fwd, _ = genome_set
    bases, off = ragged_batch(genomes, 400, 31)
    reads = [bases[off[r]:off[r + 1]].tobytes() for r in range(400)]
    # a read longer than the budget, empty reads between full ones, a run of reads shorter than k
    reads[7] = genomes[1][3000:8000].tobytes()
    for r in (0, 8, 9, 10, 399):
        reads[r] = b""
    for r in range(50, 60):
        reads[r] = reads[r][:K_SCALE - 1]
    bases, off = capi.concat_reads(reads)
    for both in (False, True):
        want = fwd.read_hits(bases, off, both)
        assert np.array_equal(want, want_from_search(fwd, bases, off, both)[0])
        with tuning("read_hits_chunk_bases", 1000, 0):
            assert np.array_equal(fwd.read_hits(bases, off, both), want)
        with tuning("read_hits_chunk_bases", 1, 0):                   # one read per chunk
            assert np.array_equal(fwd.read_hits(bases[:off[40]], off[:41], both), want[:40])
    with tuning("read_hits_chunk_bases", 1000, 0):
        assert fwd.read_hits(np.zeros(0, np.uint8), np.zeros(1, np.int64)).shape == (0, 4)          # n_reads = 0
        short = [b"ACGT" * 5] * 300 + [b""] * 5                                                     # all shorter than k
        assert not fwd.read_hits_reads(short, True).any()
        assert not fwd.read_hits_reads([b"", b"", b""]).any()
    assert fwd.read_hits(np.zeros(0, np.uint8), np.zeros(1, np.int64), True).shape == (0, 4)
    # offsets that do not start at 0
    assert np.array_equal(fwd.read_hits(bases, off[5:]), want_from_search(fwd, bases, off, False)[0][5:])


def test_wide_results_give_identical_records(gpu, genome_set):
    genomes, fwd, _ = genome_set
    bases, off = ragged_batch(genomes, 2000, 41)
    lb, lo = long_read_batch(genomes)
    for both in (False, True):
        want, want_long = fwd.read_hits(bases, off, both), fwd.read_hits(lb, lo, both)
        with tuning("read_hits_wide", 1, 0):
            assert np.array_equal(fwd.read_hits(bases, off, both), want)
            assert np.array_equal(fwd.read_hits(lb, lo, both), want_long)


@pytest.mark.parametrize("knob", [("image_level", 0, 0), ("image_level", 1, 0), ("image_level", 2, 0), ("force_mega", 1, 0),
                                  ("big_path", 2, 1), ("path_order", 0, 1)])
def test_layouts_and_image_levels(gpu, knob, genome_set):
    key, val, back = knob
    genomes, fwd, _ = genome_set
    bases, off = ragged_batch(genomes, 1500, 51)
    with tuning(key, val, back):
        idx = make_index([g.tobytes() for g in genomes], K_SCALE, False)
        nomarks = make_index([g.tobytes() for g in genomes], K_SCALE, False, False)
    if key == "image_level":
        assert idx.image_level >= val
    for both in (False, True):
        want = fwd.read_hits(bases, off, both)
        assert np.array_equal(idx.read_hits(bases, off, both), want)
        assert np.array_equal(nomarks.read_hits(bases, off, both), want)


def test_device_entry_point(gpu, genome_set):
    import torch
    genomes, fwd, _ = genome_set
    dev = torch.device("cuda", 0)
    bases, off = ragged_batch(genomes, 4000, 61)
    n = len(off) - 1
    lead = 37                                                        # d_read_off[0] != 0: bases nobody asks about in front
    shifted = np.concatenate([np.frombuffer(b"ACGTN" * 8, dtype=np.uint8)[:lead], bases])
    tb, to = torch.from_numpy(shifted).to(dev), torch.from_numpy(off + lead).to(dev)
    T = len(shifted)
    GUARD = 9                                                        # (records at a 4-byte aligned address, as the ABI allows)
    for both in (False, True):
        want = fwd.read_hits(bases, off, both)
        need = capi.read_hits_workspace_bytes(T, n, both)
        assert need >= capi.search_workspace_bytes(T)
        outs = []
        streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
        wss = [torch.zeros(need, dtype=torch.uint8, device=dev) for _ in streams]
        bufs = [torch.full((4 * n + 2 * GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=dev) for _ in streams]
        torch.cuda.synchronize(dev)
        # two calls on two streams with two workspaces on one handle, nothing synchronised in between
        for st, ws, buf in zip(streams, wss, bufs):
            fwd.read_hits_dev(tb.data_ptr(), T, to.data_ptr(), n, buf.data_ptr() + 4 * GUARD, ws.data_ptr(), need, both, st.cuda_stream)
        torch.cuda.synchronize(dev)
        for st, ws, buf in zip(streams, wss, bufs):
            h = buf.cpu().numpy()
            assert (h[:GUARD] == 0x5A5A5A5A).all() and (h[-GUARD:] == 0x5A5A5A5A).all()          # guards intact
            outs.append(h[GUARD:-GUARD].reshape(n, 4))
            assert fwd.workspace_status(ws.data_ptr(), st.cuda_stream) == 0
        assert np.array_equal(outs[0], want) and outs[0].tobytes() == outs[1].tobytes()
        # the same call again on a used workspace: byte-identical
        fwd.read_hits_dev(tb.data_ptr(), T, to.data_ptr(), n, bufs[0].data_ptr() + 4 * GUARD, wss[1].data_ptr(), need, both,
                          streams[0].cuda_stream)
        torch.cuda.synchronize(dev)
        assert bufs[0].cpu().numpy()[GUARD:-GUARD].tobytes() == outs[0].tobytes()
        # a workspace one byte short is an error, and nothing is written
        bufs[1].fill_(0x5A5A5A5A)
        with pytest.raises(capi.SbwtGpuError) as ei:
            fwd.read_hits_dev(tb.data_ptr(), T, to.data_ptr(), n, bufs[1].data_ptr() + 4 * GUARD, wss[1].data_ptr(), need - 1, both,
                              streams[1].cuda_stream)
        assert ei.value.code == capi.ERR_INVALID_ARG and "workspace" in ei.value.msg
        torch.cuda.synchronize(dev)
        assert (bufs[1].cpu().numpy() == 0x5A5A5A5A).all()
    # a workspace sized for a larger batch serves a smaller one
    big = torch.zeros(capi.read_hits_workspace_bytes(2 * T, 2 * n, True), dtype=torch.uint8, device=dev)
    buf = torch.zeros(4 * n, dtype=torch.int32, device=dev)
    fwd.read_hits_dev(tb.data_ptr(), T, to.data_ptr(), n, buf.data_ptr(), big.data_ptr(), big.numel(), True)
    torch.cuda.synchronize(dev)
    assert np.array_equal(buf.cpu().numpy().reshape(n, 4), fwd.read_hits(bases, off, True))
    with pytest.raises(capi.SbwtGpuError):
        capi._check(capi.lib().sbwtgpu_read_hits_dev(fwd.handle, tb.data_ptr(), T, to.data_ptr(), n, 3, buf.data_ptr(), big.data_ptr(),
                                                     big.numel(), None))


def test_two_host_threads_and_rank_only(gpu, genome_set):
    genomes, fwd, _ = genome_set
    batches = [ragged_batch(genomes, 3000, 71), ragged_batch(genomes, 2500, 72)]
    want = [fwd.read_hits(b, o, True) for b, o in batches]
    out, errs = [None, None], []

    def work(t):
        try:
            with_chunks = []
            for _ in range(3):
                with_chunks.append(fwd.read_hits(batches[t][0], batches[t][1], True))
            out[t] = with_chunks
        except Exception as e:        # noqa: BLE001 -- reported below
            errs.append(e)
    with tuning("read_hits_chunk_bases", 100_000, 0):
        th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    assert not errs, errs
    for t in range(2):
        for got in out[t]:
            assert np.array_equal(got, want[t])
    # rank-only image
    w = np.random.default_rng(1).integers(0, 2**64, size=4, dtype=np.uint64)
    ro = capi.Index.create(w, w, w, w, None, 256, 3)
    with pytest.raises(capi.SbwtGpuError) as ei:
        ro.read_hits_reads([b"ACGT"])
    assert ei.value.code == capi.ERR_INVALID_ARG and "only rank()" in ei.value.msg


def test_cli_read_hits(gpu, tmp_path):
    kat = KATS["cli_end_to_end"]
    d = str(tmp_path)
    k = kat["k"]
    with open(d + "/s.fna", "w") as fh:
        for i, s in enumerate(kat["seqs"]):
            fh.write(">s%d\n%s\n" % (i, s))
    p = subprocess.run([SBWT, "build", "-i", d + "/s.fna", "-o", d + "/fwd.sbwt", "-k", str(k), "--temp-dir", d], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    rng = random.Random(81)
    # (the sequence reader upper-cases what it reads: the table is that of the upper-cased reads)
    reads = [q.encode() for q in kat["queries"]] + [r.upper() for r in probe_reads(kat["seqs"], k, rng) if r]
    B = BruteSBWT(kat["seqs"], k)
    want = {both: format_table(profiles(B.kmers, k, reads, 2 if both else 1)) for both in (False, True)}
    assert want[True] != want[False]
    with open(d + "/r.fq", "w") as fh:
        for j, r in enumerate(reads):
            fh.write("@r%d\n%s\n+\n%s\n" % (j, r.decode(), "I" * len(r)))
    with open(d + "/r.fna", "w") as fh:
        for j, r in enumerate(reads):
            fh.write(">r%d\n%s\n" % (j, r.decode()))
    with open(d + "/r.fq", "rb") as src, gzip.open(d + "/r.fq.gz", "wb") as dst:
        dst.write(src.read())
    for q in ("r.fq", "r.fna", "r.fq.gz"):
        for z in (False, True):
            for both in (False, True):
                out = "%s/%s.%d%d.out" % (d, q, z, both)
                cmd = [SBWT, "read-hits", "-i", d + "/fwd.sbwt", "-q", d + "/" + q, "-o", out]
                cmd += (["-z"] if z else []) + (["--both-strands"] if both else [])
                p = subprocess.run(cmd, capture_output=True, timeout=300)
                assert p.returncode == 0, p.stderr.decode()
                text = gzip.open(out).read() if z else open(out, "rb").read()
                assert text == want[both], (q, z, both)
    # list files and small batches
    with open(d + "/in.txt", "w") as fh:
        fh.write(d + "/r.fna\n" + d + "/r.fq.gz\n")
    with open(d + "/out.txt", "w") as fh:
        fh.write(d + "/l1.out\n" + d + "/l2.out\n")
    p = subprocess.run([SBWT, "read-hits", "-i", d + "/fwd.sbwt", "-q", d + "/in.txt", "-o", d + "/out.txt", "--batch-bases", "100"],
                       capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    assert open(d + "/l1.out", "rb").read() == want[False] and open(d + "/l2.out", "rb").read() == want[False]
    # an unknown option fails, and the command is listed
    p = subprocess.run([SBWT, "read-hits", "-i", d + "/fwd.sbwt", "-q", d + "/r.fq", "-o", d + "/x.out", "--no-such-option"],
                       capture_output=True, timeout=60)
    assert p.returncode != 0
    p = subprocess.run([SBWT], capture_output=True, timeout=60)
    assert b"read-hits" in p.stderr
