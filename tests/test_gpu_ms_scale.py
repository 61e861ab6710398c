"""GPU: matching statistics (sbwt_ms.hip) at scale against the oracle's definition-level MS and LCS, on EVERY position and
every column: config 2 with 1024-base chunks, a repetitive index that drives the recompute path, a k sweep with the full
LCS array, the image layouts, 1 Mbp reads, and the edges of the device entry point (offsets, unaligned len, guard bytes).

The oracle (orc_matching_statistics, orc_lcs) applies the definitions with update_interval from [0, n-1] and get_kmer's
backward step; it shares nothing with the kernel's algorithm (no LCS array, no contraction)."""
import numpy as np
import pytest

import bench
from oracle import OracleIndex
from sbwt_amd import capi, synth

pytestmark = pytest.mark.gpu

NT = max(1, min(16, bench.effective_cores()))


def oracle_of(bits, k, precalc_k=8):
    return OracleIndex.from_bits(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k,
                                 bits.n_kmers, precalc_k)


def index_of(bits, k):
    return capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k,
                             bits.n_kmers, 0)


def assert_same(got, want, label):
    """Equal arrays, or the first differing slot in the message."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (label, "%d slots differ, first at %d: got %d want %d" % (len(bad), bad[0], got[bad[0]], want[bad[0]]))


def check_ms(idx, bases, off, want, label):
    """Batch MS with intervals and lengths only, against the oracle's (len, first, second) on every position."""
    ln, f, s = idx.matching_statistics(bases, off)
    assert_same(ln, want[0], (label, "len"))
    assert_same(f, want[1], (label, "first"))
    assert_same(s, want[2], (label, "second"))
    assert_same(idx.matching_statistics(bases, off, intervals=False), want[0], (label, "len only"))
    return ln


def dirty(bases, seed, n):
    """N, lower case, NUL and 0xFF bytes at n random places each."""
    for j, ch in enumerate((ord("N"), ord("a"), ord("g"), 0, 0xFF)):
        bases = synth.inject(bases, n, ch, seed + j)
    return bases


# ---- config 2 ----
@pytest.fixture(scope="module")
def config2():
    genomes = synth.coli3_like(5_000_000)
    bits = capi.build_bits_gpu([g.tobytes() for g in genomes], 30, False, True)
    return genomes, oracle_of(bits, 30), index_of(bits, 30)


def test_config2_every_position(gpu, config2):
    """~470 k reads of 150 bp (> 2^26 bases: 1024-base chunks) with substitutions and dirty bytes, plus 200 k random reads
    (short matches, dense contractions); then a batch below 2^26 bases (256-base chunks) that is a prefix of the same reads."""
    genomes, orc, idx = config2
    k = 30
    b1, o1 = synth.sample_reads(genomes, 470_000, 150, 0.01, 31)
    b1 = dirty(b1, 32, 40_000)
    b2, o2 = synth.random_reads(200_000, 150, 33)
    bases = np.concatenate([b1, b2])
    off = np.concatenate([o1, o2[1:] + o1[-1]])
    assert len(bases) >= (1 << 26) and capi_chunk(len(bases), k) == 1024
    want = orc.matching_statistics(bases, off, n_threads=NT)
    ln = check_ms(idx, bases, off, want, "config 2")
    full = ln == k
    assert 0.3 < full[:len(b1)].mean() < 0.95 and full[len(b1):].mean() < 0.01, (full[:len(b1)].mean(), full[len(b1):].mean())
    # the first 400 k reads alone: below 2^26 bases, 256-base chunks; the same answers as in the large batch
    n_small = 400_000
    assert off[n_small] < (1 << 26) and capi_chunk(int(off[n_small]), k) == 256
    small = idx.matching_statistics(bases[:off[n_small]], off[:n_small + 1])
    for a, b, name in zip(small, want[:3], ("len", "first", "second")):
        assert_same(a, b[:off[n_small]], ("prefix batch", name))


def capi_chunk(total_bases, k):
    """The kernel's chunk rule (sbwt_ms_chunk): 256 output positions, 1024 from 2^26 bases on, at least 4k."""
    c = 1024 if total_bases >= (1 << 26) else 256
    while c < 4 * k:
        c *= 2
    return c


def test_long_reads_every_position(gpu, config2):
    """Three 1 Mbp reads with N and substitutions, each answered by about a thousand lanes."""
    genomes, orc, idx = config2
    rng = np.random.default_rng(51)
    reads = []
    for j in range(3):
        g = genomes[j]
        a = int(rng.integers(0, len(g) - 1_000_000))
        r = synth.mutate(g[a:a + 1_000_000].copy(), 0.005, 52 + j)
        reads.append(synth.inject(r, 300, ord("N"), 55 + j).tobytes())
    bases, off = capi.concat_reads(reads)
    check_ms(idx, bases, off, orc.matching_statistics(bases, off, n_threads=NT), "long reads")


# ---- the device entry point's edges ----
def dev_ms(idx, host, off, len_shift, intervals, guard=64):
    """sbwtgpu_matching_statistics_dev on torch buffers: bases `host` (slot b answers host[b]), d_len starting `len_shift`
    bytes past an aligned base, and `guard` guard slots after the last one; returns (len, first, second) of slots
    [0, off[-1]) and the workspace's counters.  Slots before off[0] and the guards must keep their fill."""
    import torch
    dev = torch.device("cuda", 0)
    n = int(off[-1])
    tb = torch.from_numpy(np.array(host, dtype=np.uint8)).to(dev)
    to = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to(dev)
    lbuf = torch.full((len_shift + n + guard,), 0x5A, dtype=torch.uint8, device=dev)
    fbuf = torch.full((n + guard,), -77, dtype=torch.int64, device=dev)
    sbuf = torch.full((n + guard,), -78, dtype=torch.int64, device=dev)
    ws = torch.zeros(capi.ms_workspace_bytes(n - int(off[0])), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    idx.matching_statistics_dev(tb.data_ptr(), n - int(off[0]), to.data_ptr(), len(off) - 1, lbuf.data_ptr() + len_shift,
                                fbuf.data_ptr() if intervals else 0, sbuf.data_ptr() if intervals else 0, ws.data_ptr(),
                                ws.numel(), stream)
    torch.cuda.synchronize(dev)
    st = idx.ms_workspace_stats(ws.data_ptr(), stream)
    L, F, S = lbuf.cpu().numpy(), fbuf.cpu().numpy(), sbuf.cpu().numpy()
    b0 = int(off[0])
    assert (L[:len_shift + b0] == 0x5A).all() and (L[len_shift + n:] == 0x5A).all(), "len guard bytes overwritten"
    if intervals:
        assert (F[:b0] == -77).all() and (F[n:] == -77).all() and (S[:b0] == -78).all() and (S[n:] == -78).all(), \
            "interval guard slots overwritten"
    else:
        assert (F == -77).all() and (S == -78).all()
    return (L[len_shift:len_shift + n], F[:n], S[:n]), st


def test_dev_offsets_alignment_and_guards(gpu, config2):
    genomes, orc, idx = config2
    k = 30
    g = genomes[1]
    rb, ro = synth.sample_reads(genomes, 3000, 150, 0.02, 61)
    rb = dirty(rb, 62, 300)
    reads = [b"", g[500:503].tobytes()] + [rb[ro[r]:ro[r + 1]].tobytes() for r in range(1500)] + [b"", b""]
    reads += [g[10_000:10_029].tobytes(), b"A", b"", g[20_000:25_000].tobytes()]          # shorter than k; > 3 chunks
    reads += [rb[ro[r]:ro[r + 1]].tobytes() for r in range(1500, 3000)] + [b""]
    cat, coff = capi.concat_reads(reads)
    junk = g[3_000_000:3_000_100]               # valid bases in front of the first read: no read may see them
    for b0 in (13, 64, 65):
        host = np.concatenate([junk[:b0], cat])
        off = coff + b0
        want = orc.matching_statistics(host, off, n_threads=NT)
        for shift in (0, 1, 2, 3):
            for intervals in (True, False):
                got, st = dev_ms(idx, host, off, shift, intervals)
                assert_same(got[0][b0:], want[0][b0:], (b0, shift, intervals, "len"))
                if intervals:
                    assert_same(got[1][b0:], want[1][b0:], (b0, shift, "first"))
                    assert_same(got[2][b0:], want[2][b0:], (b0, shift, "second"))
                assert st["positions"] == len(cat) and st["full"] == int((want[0][b0:] == k).sum()), (b0, shift, st)
    # a single base; a batch of one long read (many chunks) at an odd offset
    for host, off in ((np.frombuffer(b"TTC", np.uint8), np.array([2, 3])),
                      (np.concatenate([junk[:7], g[40_000:41_000]]), np.array([7, 1007]))):
        want = orc.matching_statistics(host, off)
        for shift in (0, 3):
            got, _ = dev_ms(idx, host, off, shift, True)
            b0 = int(off[0])
            for a, b in zip(got, want[:3]):
                assert_same(a[b0:], b[b0:], (len(host), shift))


# ---- a repetitive index: wide intervals on both sides of the scan bound, so the recompute path runs ----
UNITS = [b"AC", b"AGG", b"ATTC", b"TTAGG", b"A", b"CAG"]


def repeat_index_genome(seed):
    """A random 3 Mbp genome with 8 families of 1.2-2 kbp, each pasted 100-160 times as 1 %-diverged copies, and 4000 tandem
    tracts of 40-150 bases from six units in random contexts: the labels that end inside a tract of one unit form intervals
    of thousands of columns, so a contraction into a tract widens past the scan bound."""
    rng = np.random.default_rng(seed)
    g = synth.random_genome(3_000_000, seed)
    fams = [synth.random_genome(int(rng.integers(1200, 2001)), seed + 1 + f) for f in range(8)]
    for f, fam in enumerate(fams):
        for c in range(int(rng.integers(100, 161))):
            at = int(rng.integers(0, len(g) - len(fam)))
            g[at:at + len(fam)] = synth.mutate(fam.copy(), 0.01, seed * 1000 + f * 200 + c)
    tracts = []
    for t in range(4000):
        unit = np.frombuffer(UNITS[t % len(UNITS)], dtype=np.uint8)
        tract = np.tile(unit, 150 // len(unit) + 1)[:int(rng.integers(40, 151))]
        at = int(rng.integers(0, len(g) - len(tract)))
        g[at:at + len(tract)] = tract
        tracts.append((at, len(tract)))
    return g, fams, tracts


def test_repetitive_index_recompute_path(gpu):
    k = 31
    g, fams, tracts = repeat_index_genome(71)
    bits = capi.build_bits_gpu([g.tobytes()], k, True, True)
    orc, idx = oracle_of(bits, k), index_of(bits, k)
    rng = np.random.default_rng(72)
    # reads from fresh 1 %-diverged copies of the families (both strands), across the tandem tracts and their flanks, novel
    # sequence running into a tract, and reads from the genome
    reads = []
    for j in range(20_000):
        fam = fams[j % len(fams)]
        a = int(rng.integers(0, len(fam) - 150))
        r = synth.mutate(fam[a:a + 150].copy(), 0.01, 73 + j)
        reads.append((synth.revcomp(r) if j & 1 else r).tobytes())
    for j in range(20_000):
        at, ln = tracts[j % len(tracts)]
        a = max(0, at - int(rng.integers(0, 100)))
        reads.append(synth.mutate(g[a:a + 150].copy(), 0.01, 90_000 + j).tobytes())
    for j in range(20_000):
        unit = UNITS[j % len(UNITS)]
        novel = synth.random_genome(int(rng.integers(20, 90)), 200_000 + j).tobytes()
        reads.append((novel + unit * (150 // len(unit)))[:150])
    gb, go = synth.sample_reads([g], 40_000, 150, 0.01, 74)
    reads += [gb[go[r]:go[r + 1]].tobytes() for r in range(40_000)]
    bases, off = capi.concat_reads(reads)
    bases = dirty(bases, 75, 2000)
    want = orc.matching_statistics(bases, off, n_threads=NT)
    check_ms(idx, bases, off, want, "repeats")
    got, st = dev_ms(idx, bases, off, 0, True)
    for a, b in zip(got, want[:3]):
        assert_same(a, b, "repeats dev")
    print("repetitive index: %d columns, counters %s" % (idx.n_nodes, st))
    assert st["positions"] == len(bases) and st["full"] == int((want[0] == k).sum())
    # an MI355X counted 11 490 recomputes and 10.6 M contractions on these 15 M positions (config 2's reads: ~1e-5 per base)
    assert st["recomputes"] >= 5000, st
    assert st["contractions"] > len(bases) // 2, st


# ---- a k sweep with the full LCS array ----
@pytest.mark.parametrize("k", [15, 31, 32, 63, 64])
def test_k_sweep_lcs_and_every_position(gpu, k):
    g = synth.repeat_genome(800_000, 80 + k, 0.1)
    bits = capi.build_bits_gpu([g.tobytes()], k, True, True)
    assert 1_000_000 < bits.n_nodes < 4_000_000, bits.n_nodes
    orc = oracle_of(bits, k)
    want_lcs = orc.lcs(n_threads=NT)
    b1, o1 = synth.both_strand_reads([g], 20_000, 150, 0.01, 81)
    b1 = dirty(b1, 82, 1000)
    b2, o2 = synth.random_reads(2000, 150, 83)
    bases = np.concatenate([b1, b2])
    off = np.concatenate([o1, o2[1:] + o1[-1]])
    want = orc.matching_statistics(bases, off, n_threads=NT)
    assert (want[0] == k).mean() > 0.2
    for ssup in (True, False):
        idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup if ssup else None,
                                bits.n_nodes, k, bits.n_kmers, 0)
        assert idx.has_streaming_support == ssup
        assert_same(idx.lcs(), want_lcs, (k, ssup, "lcs"))
        check_ms(idx, bases, off, want, (k, ssup))
        idx.close()


# ---- the image layouts ----
@pytest.fixture(scope="module")
def layout_case():
    k = 31
    g = synth.repeat_genome(1_000_000, 90, 0.1)
    bits = capi.build_bits_gpu([g.tobytes()], k, True, True)
    orc = oracle_of(bits, k)
    b1, o1 = synth.both_strand_reads([g], 30_000, 150, 0.01, 91)
    b1 = dirty(b1, 92, 1000)
    b2, o2 = synth.random_reads(5000, 150, 93)
    bases = np.concatenate([b1, b2])
    off = np.concatenate([o1, o2[1:] + o1[-1]])
    return bits, k, orc.lcs(n_threads=NT), bases, off, orc.matching_statistics(bases, off, n_threads=NT)


@pytest.mark.parametrize("knob", [("force_mega", 1, 0), ("big_path", 2, 1), ("image_level", 1, 0), ("image_level", 2, 0)])
def test_layouts_every_position(gpu, layout_case, knob):
    bits, k, want_lcs, bases, off, want = layout_case
    assert 1_500_000 < bits.n_nodes < 3_000_000, bits.n_nodes
    key, val, back = knob
    capi.set_tuning(key, val)
    try:
        idx = index_of(bits, k)
    finally:
        capi.set_tuning(key, back)
    if key == "image_level":
        assert idx.image_level >= val
    assert_same(idx.lcs(), want_lcs, (knob, "lcs"))
    check_ms(idx, bases, off, want, knob)
    idx.close()
