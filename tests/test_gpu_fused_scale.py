"""GPU: the fused search route at scale, bit for bit against the oracle on EVERY k-mer.

The headline number comes from `k_search_fused<..., SORT>` (sbwt_search_fused.hip): lanes sorted by state, searcher waves and
path-follower waves that pass reads to each other through LDS slots and two rings of FZ_RING = 512 entries.  Here it runs at
full size (config 2: 10 M x 150 bp reads, 1.21e9 k-mers), with so few workgroups that its rings wrap hundreds of times, in
every sorted sub-mode, through the ticket table of long reads, on batches whose later reads contradict the 4096-read sample
the route is chosen from, and behind the pipelined host-buffer entry points.

Every device-pointer call also checks the workspace's status word (0; SBWTGPU_ERR_STALLED names the sorted kernel's stall
detector) and, on an image with a path order, which route ran: the fused kernel draws its reads from the header's ticket
counter (SbwtWorkHeader::ticket, the header's first word) and nothing else does -- the general kernel behind it counts in
`ticket2` --, so a nonzero counter means the fused route took the batch, and with "fused_sort" bit 12 (4096) and k <= 31 the
fused route is the sorted instantiation (the unsorted ones return at once).  `n_ext` (workspace_stats()[4]) > 0 says that
k-mers were answered along path runs; the general path kernel counts those too, so it shows work, not the route.  Results
are compared in chunks of at most about 1 M reads of 150 bases, so host memory stays near 2 GB."""
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest

from oracle import OracleIndex
from sbwt_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_KMERS = 121_000_000           # oracle chunks: 1 M reads of 150 bases (968 MB of int64 results)
HDR_WORDS = 40                      # SbwtWorkHeader: 320 bytes
SORTED = 7728                       # "fused_sort": the sorted kernel whatever the hint says (4096 | the default's sub-mode)
UNSORTED = 0                        # ... the unsorted kernel only
SORT_MODES = (4097, 4656, 6192, 6448, 7728)      # the sorted sub-modes tools/fuzz_gpu.py draws from


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


@contextmanager
def knobs(**kv):
    """Sets tuning knobs for a block; restores every knob these tests touch to its default afterwards."""
    try:
        for key, v in kv.items():
            capi.set_tuning(key, v)
        yield
    finally:
        capi.set_tuning("fused_sort", 3632)
        capi.set_tuning("fused_table", 1)
        capi.set_tuning("debug", 0)
        capi.set_tuning("search_variant", -1)


def routes_checked(idx) -> bool:
    """Route assertions hold on an image with a path order only (SBWTGPU_IMAGE_LEVEL > 0: no fused route)."""
    return int(os.environ.get("SBWTGPU_IMAGE_LEVEL", "0")) == 0 and idx.image_level == 0


def oracle_chunks(orc, bases, read_off, n_threads):
    """The oracle's results of a batch, chunk by chunk: (first k-mer, int64 results), <= CHUNK_KMERS k-mers a chunk
    (or one read).  `bases` may be a device tensor: each chunk's bases are copied to the host as they are needed."""
    read_off = np.ascontiguousarray(read_off, dtype=np.int64)
    oo = capi.out_offsets(read_off, orc.k)
    n = len(read_off) - 1
    lo = 0
    while lo < n:
        hi = int(np.searchsorted(oo, oo[lo] + CHUNK_KMERS, side="right")) - 1
        hi = min(n, max(hi, lo + 1))
        ro = read_off[lo:hi + 1]
        h = bases[int(ro[0]):int(ro[-1])]
        h = h.cpu().numpy() if hasattr(h, "cpu") else h
        part, _ = orc.batch_search(h, ro - ro[0], oo[lo:hi + 1] - oo[lo], n_threads)
        yield int(oo[lo]), part
        lo = hi


def oracle_of(orc, bases, read_off, n_threads):
    """The oracle's results of a whole batch as int32 (every column of these indexes is < 2^31)."""
    want = np.empty(int(capi.out_offsets(read_off, orc.k)[-1]), dtype=np.int32)
    for a, part in oracle_chunks(orc, bases, read_off, n_threads):
        assert part.min(initial=0) >= -1 and part.max(initial=0) < (1 << 31)
        want[a:a + len(part)] = part
    return want


def assert_oracle_streamed(orc, bases, read_off, got, n_threads, what):
    """got (device tensor) == the oracle on every k-mer, without holding the oracle's results of the whole batch."""
    n = 0
    for a, part in oracle_chunks(orc, bases, read_off, n_threads):
        assert_equal_chunked(got[a:a + len(part)], part.astype(np.int32), "%s, k-mers from %d" % (what, a))
        n += len(part)
    assert n == got.numel(), (what, n, got.numel())


def assert_equal_chunked(got, want, what):
    """got (device tensor, int64 or int32) == want (host int32 array), every element, in chunks."""
    import torch
    assert got.numel() == len(want), (what, got.numel(), len(want))
    for a in range(0, len(want), CHUNK_KMERS):
        b = min(len(want), a + CHUNK_KMERS)
        w = torch.from_numpy(want[a:b]).to(got.device)
        g = got[a:b]
        if not torch.equal(g.to(torch.int32) if g.dtype == torch.int64 else g, w):
            # (int64 results outside the int32 range would wrap: compare in int64 before naming the first difference)
            d = (g.to(torch.int64) != w.to(torch.int64)).nonzero()
            first = int(d[0].item()) if d.numel() else -1
            if first >= 0:
                raise AssertionError("%s: %d of %d results differ from the oracle, the first at %d: %d, want %d"
                                     % (what, d.numel(), b - a, a + first, int(g[first].item()), int(want[a + first])))
        if g.dtype == torch.int64:
            assert int(g.max().item()) < (1 << 31) and int(g.min().item()) >= -1, what


class DevBatch:
    """One batch resident on the device, and the device-pointer calls on it."""

    def __init__(self, bases, read_off, k):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.off = np.ascontiguousarray(read_off, dtype=np.int64)
        self.oo = capi.out_offsets(self.off, k)
        self.d_b = bases if isinstance(bases, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(bases)).to(self.dev)
        self.d_ro = torch.from_numpy(self.off).to(self.dev)
        self.d_oo = torch.from_numpy(self.oo).to(self.dev)
        self.n = len(self.off) - 1
        self.total = int(self.oo[-1])
        self.wsb = capi.search_workspace_bytes(self.d_b.numel())
        self.st = torch.cuda.current_stream().cuda_stream

    def zeroed_ws(self):
        return self.torch.zeros(self.wsb, dtype=self.torch.uint8, device=self.dev)

    def run(self, idx, what, i32=False, streaming=True, d_ws=None, fused=True, ext=True):
        """One call into a result buffer that holds -9 / 0xA5.. (the poison) wherever the call writes nothing.  fused:
        True = the fused route must take the batch, False = it must decline it, None = not checked.  Returns the results
        and the workspace's header."""
        torch = self.torch
        d_ws = self.zeroed_ws() if d_ws is None else d_ws
        out = torch.full((self.total,), -9, dtype=torch.int32 if i32 else torch.int64, device=self.dev)
        f = idx.streaming_search_dev_i32 if i32 else idx.streaming_search_dev
        f(self.d_b.data_ptr(), self.d_b.numel(), self.d_ro.data_ptr(), self.n, out.data_ptr(), self.d_oo.data_ptr(),
          d_ws.data_ptr(), self.wsb, self.st, streaming)
        torch.cuda.synchronize()
        status = idx.workspace_status(d_ws.data_ptr(), self.st)
        assert status == 0, "%s: workspace status %d (ERR_STALLED = %d, ERR_NOT_SINGLETON = %d)" % (
            what, status, capi.ERR_STALLED, capi.ERR_NOT_SINGLETON)
        hdr = d_ws[:8 * HDR_WORDS].cpu().numpy().view(np.int64)
        if fused is not None and routes_checked(idx):
            n_ext = idx.workspace_stats(d_ws.data_ptr(), self.st)[4]
            if fused:
                assert int(hdr[0]) > 0, "%s: the fused route did not take the batch (ticket counter 0)" % what
                if ext:
                    assert n_ext > 0, "%s: no k-mer answered along a path run" % what
            else:
                assert int(hdr[0]) == 0, "%s: the fused route took a batch it should decline (%d tickets)" % (what, int(hdr[0]))
        return out, hdr


def check_all(idx, batch, want, runs, what):
    """runs: (label, knob dict, run() keyword arguments); every run against the oracle, every k-mer."""
    for label, kn, kw in runs:
        with knobs(**kn):
            out, _ = batch.run(idx, "%s %s" % (what, label), **kw)
        assert_equal_chunked(out, want, "%s %s" % (what, label))
        del out


# ---------------------------------------------------------------------------------------------------------------------
# config 2: coli3-like genomes, k = 30, streaming support, precalc 8
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def config2():
    genomes = synth.coli3_like(5_000_000)
    bits = capi.build_bits_gpu([g.tobytes() for g in genomes], 30, False, True)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, 30,
                            bits.n_kmers, 8)
    orc = OracleIndex.from_bits(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, 30,
                                bits.n_kmers, 8)
    return genomes, idx, orc


def sampled(genomes, n_reads, read_len, sub_rate, seed, parts=4):
    """synth.sample_reads in `parts` pieces (the substitutions' random numbers of 3e8 bases at once would take 2.4 GB)."""
    bs = [synth.sample_reads(genomes, n_reads // parts, read_len, sub_rate, seed + 7 * q)[0] for q in range(parts)]
    return np.concatenate(bs), np.arange(n_reads // parts * parts + 1, dtype=np.int64) * read_len


def test_config2_full_size_sorted_every_kmer(gpu, config2):
    """The headline workload, 10 M x 150 bp reads (bench.gpu_reads, seed 4242), on zeroed workspaces: the unsorted kernel
    ("fused_sort" 0) and the sorted one (forced, 7728) give the same int64 results, and those equal the oracle on all
    1.21e9 k-mers; the sorted kernel's int32 results and SBWT::search (streaming=False) give the same.  Then the hint as
    the product uses it -- three default calls on one zeroed workspace: unsorted, unsorted, then sorted because the two
    calls before followed their paths -- and two more forced-sorted batches of 2 M reads where the followers are mostly
    idle (5 % substitutions) and have nothing to do at all (random reads), with status 0: the stall detector stays quiet."""
    import torch
    bench = _bench()
    genomes, idx, orc = config2
    n_reads, L = 10_000_000, 150
    d_bases = bench.gpu_reads(genomes, n_reads, 4242, torch.device("cuda:0"))
    B = DevBatch(d_bases, np.arange(n_reads + 1, dtype=np.int64) * L, 30)
    with knobs(fused_sort=UNSORTED):
        a, _ = B.run(idx, "config 2 unsorted")
    with knobs(fused_sort=SORTED):
        s, _ = B.run(idx, "config 2 sorted")
        assert torch.equal(a, s), "config 2: the sorted kernel differs from the unsorted one"
        del s
        s32, _ = B.run(idx, "config 2 sorted int32", i32=True)
        assert torch.equal(s32.to(torch.int64), a), "config 2: sorted int32 results differ from int64"
        del s32
        sq, _ = B.run(idx, "config 2 sorted search", streaming=False)
        assert torch.equal(sq, a), "config 2: sorted SBWT::search differs from streaming_search"
        del sq
    assert_oracle_streamed(orc, d_bases, B.off, a, bench.effective_cores(), "config 2 (all 1.21e9 k-mers)")
    hit = float((a >= 0).double().mean().item())
    assert 0.70 < hit < 0.78, hit
    # the hint at scale: three default calls on one zeroed workspace
    d_ws = B.zeroed_ws()
    for q, hint_want in enumerate((0x5B377A01, 0x5B377A02, 0x5B377A02)):
        out, hdr = B.run(idx, "config 2 default call %d" % q, d_ws=d_ws)
        assert torch.equal(out, a), "config 2 default call %d differs from the oracle's results" % q
        if routes_checked(idx):
            hint = int(hdr[39]) & 0xFFFFFFFF               # SbwtWorkHeader::hint (the header's last word)
            assert hint == hint_want, (q, hex(hint))
        del out
    del a
    # forced sorted, followers mostly idle and idle throughout
    for what, (bases, off), ext in (("5 % substitutions", sampled(genomes, 2_000_000, L, 0.05, 61), True),
                                    ("random reads", synth.random_reads(2_000_000, L, 62), False)):
        Bx = DevBatch(bases, off, 30)
        want = oracle_of(orc, bases, off, bench.effective_cores())
        check_all(idx, Bx, want, [("sorted", {"fused_sort": SORTED}, {"ext": ext})], "config 2, 2 M reads, " + what)
        del Bx, want


def test_rings_wrap_with_few_workgroups(gpu, config2):
    """The sorted kernel on 1, 2 and 7 workgroups ("debug" = n << 8), every sorted sub-mode the fuzzer draws, on 200 K reads
    each: reads that follow their paths (0.2 % substitutions), 1 % substitutions with N, 8 % substitutions, and ragged
    10-160 bp reads (the general, non-UNI sorted instantiation).

    Why this wraps the rings: a workgroup's 128 searcher lanes start with slots 0-127, the other 192 of FZ_SLOTS = 320 wait
    as free slots in the searchers' ring.  A read that starts to follow its path (F_EXT) is handed over -- its slot goes into
    the followers' ring -- and when a follower has finished it the slot goes back into the searchers' ring as a free one
    (written by the follower, or as kind 3 for a searcher wave to write).  So every read that reaches a path run pushes its
    slot through both rings once at least, and a ring's place is its running count modulo FZ_RING = 512.  With one
    workgroup all 200 K reads pass through the same two rings: about 390 wraps of each (from the loop's logic; the kernel
    has no counter that would show it in a default build)."""
    bench = _bench()
    genomes, idx, orc = config2
    batches = [("0.2 %", synth.sample_reads(genomes, 200_000, 150, 0.002, 71))]
    nb, no = synth.sample_reads(genomes, 200_000, 150, 0.01, 72)
    batches.append(("1 % + N", (synth.inject(nb, 3000, ord("N"), 73), no)))
    batches.append(("8 %", synth.sample_reads(genomes, 200_000, 150, 0.08, 74)))
    batches.append(("ragged 10-160", synth.ragged_reads(genomes, 200_000, 10, 160, 0.01, 75)))
    for what, (bases, off) in batches:
        B = DevBatch(bases, off, 30)
        want = oracle_of(orc, bases, off, bench.effective_cores())
        runs = [("%d workgroups, fused_sort %d" % (n, fs), {"fused_sort": fs, "debug": n << 8}, {})
                for n in (1, 2, 7) for fs in SORT_MODES]
        check_all(idx, B, want, runs, "rings, " + what)
        del B, want


# ---------------------------------------------------------------------------------------------------------------------
# the ticket table of long reads, sorted
# ---------------------------------------------------------------------------------------------------------------------
def long_read_batch(genomes, n_long, lo, hi, sub, seed, n_n=25, n_lower=10, whole=True):
    """Reads of lo .. hi bases, short reads in between, optionally a genome as one read; substitutions, N, lower case."""
    bases, off = synth.ragged_reads(genomes, n_long, lo, hi, sub, seed)
    short_b, short_o = synth.ragged_reads(genomes, 60, 5, 200, 0.01, seed + 1)
    parts, offs = [bases, short_b], [off, short_o[1:] + off[-1]]
    if whole:
        w = synth.mutate(genomes[1], 0.005, seed + 2)
        parts.append(w)
        offs.append(np.array([offs[-1][-1] + len(w)], dtype=np.int64))
    bases = np.concatenate(parts)
    off = np.concatenate(offs).astype(np.int64)
    bases = synth.inject(bases, n_n, ord("N"), seed + 3)
    bases = synth.inject(bases, n_lower, ord("g"), seed + 4)
    return bases, off


@pytest.mark.parametrize("k", [24, 31])
def test_sorted_ticket_table_small(gpu, k):
    """`k_search_fused<false, O32, false, false, true, true>` -- sorted lanes on the ticket table -- deterministically, for
    int64 and int32 results: the ticket-table batch of test_long_reads_through_the_fused_kernels_ticket_table (reads of
    300-6000 bases, a genome as one read, short reads, N, lower case) under "fused_sort" 7728 and 0, through the
    device-pointer calls (the route checked) and the host-buffer calls."""
    genomes = [synth.random_genome(150_000, 41)]
    genomes.append(synth.mutate(genomes[0], 0.03, 42))
    orc = OracleIndex.build([g.tobytes() for g in genomes], k, True, False, 4)
    cols = orc.columns()
    idx = capi.Index.create(cols[0], cols[1], cols[2], cols[3], orc.ssup_words(), orc.n_nodes, orc.k, orc.n_kmers, orc.precalc_k)
    bases, off = long_read_batch(genomes, 700, 300, 6000, 0.01, 13)
    want = oracle_of(orc, bases, off, _bench().effective_cores())
    B = DevBatch(bases, off, k)
    for fs in (SORTED, UNSORTED):
        with knobs(fused_sort=fs):
            for i32 in (False, True):
                out, hdr = B.run(idx, "k %d fused_sort %d int32 %s" % (k, fs, i32), i32=i32)
                if routes_checked(idx):
                    assert int(hdr[32]) > 0 and int(hdr[33]) == 0, "not in table mode (n_ftick %d, over %d)" % (hdr[32], hdr[33])
                assert_equal_chunked(out, want, "k %d fused_sort %d int32 %s" % (k, fs, i32))
            got = idx.streaming_search(bases, off)[0]
            assert np.array_equal(got, want), (k, fs)
            got = idx.search_i32(bases, off)[0]
            assert np.array_equal(got, want), (k, fs)


def test_sorted_ticket_table_at_scale(gpu, config2):
    """The ticket table on the config-2 index: 20 000 reads of 1-10 kbp (1.1e8 bases) with 1 % substitutions, N and lower
    case, and 100 000 reads of exactly 1 kbp (uniform reads longer than three pieces take the table too) -- sorted,
    unsorted, and with the table off (the fused route declines the batch) -- against the oracle on every k-mer."""
    bench = _bench()
    genomes, idx, orc = config2
    lb, lo = long_read_batch(genomes, 20_000, 1000, 10_000, 0.01, 81, n_n=400, n_lower=200, whole=False)
    ub, uo = synth.sample_reads(genomes, 100_000, 1000, 0.01, 82)
    for what, (bases, off) in (("1-10 kbp", (lb, lo)), ("1 kbp", (ub, uo))):
        B = DevBatch(bases, off, 30)
        want = oracle_of(orc, bases, off, bench.effective_cores())
        check_all(idx, B, want, [("sorted", {"fused_sort": SORTED}, {}),
                                 ("sorted int32", {"fused_sort": SORTED}, {"i32": True}),
                                 ("unsorted", {"fused_sort": UNSORTED}, {}),
                                 ("table off", {"fused_table": 0}, {"fused": False})], "ticket table, " + what)
        del B, want


def test_wide_ticket_table_k63(gpu):
    """k = 63 (the WIDE instantiation; no streaming support, SBWT::search) on the ticket table: 3 000 reads of 300-6000
    bases with a genome as one read, against the oracle on every k-mer, table on and off."""
    bench = _bench()
    genomes = synth.coli3_like(1_000_000)
    bits = capi.build_bits_gpu([g.tobytes() for g in genomes], 63, False, False)
    orc = OracleIndex.from_bits(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], None, bits.n_nodes, 63, bits.n_kmers, 8)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], None, bits.n_nodes, 63, bits.n_kmers, 8)
    bases, off = long_read_batch(genomes, 3000, 300, 6000, 0.01, 91)
    B = DevBatch(bases, off, 63)
    want = oracle_of(orc, bases, off, bench.effective_cores())
    check_all(idx, B, want, [("table", {}, {"streaming": False}),
                             ("table int32", {}, {"streaming": False, "i32": True}),
                             ("table off", {"fused_table": 0}, {"streaming": False, "fused": False})], "k 63 ticket table")


# ---------------------------------------------------------------------------------------------------------------------
# batches whose later reads contradict the 4096-read sample (SBWT_RG_SAMPLE) the fused route's mode is chosen from
# ---------------------------------------------------------------------------------------------------------------------
def two_part(genomes, first, rest, seed):
    """first / rest: (reads, min length, max length); one batch, the first part exactly the sample."""
    (n1, a1, b1), (n2, a2, b2) = first, rest
    x, xo = synth.ragged_reads(genomes, n1, a1, b1, 0.01, seed)
    y, yo = synth.ragged_reads(genomes, n2, a2, b2, 0.01, seed + 1)
    return np.concatenate([x, y]), np.concatenate([xo, yo[1:] + xo[-1]]).astype(np.int64)


def test_batches_that_contradict_the_sample(gpu, config2):
    """Pieces vs table is decided from the first 4096 reads (fused_sample_of_wave).  Later reads that the sample did not
    foresee go down the "too long, hand on" path of the refill (toolong, pc == 0): short reads then reads of 300-480
    bases; reads of 161-320 then 321-2000; long reads (table mode) then 50 000 short, empty or shorter-than-k reads; reads
    of exactly 160, 161, 480 and 481 bases on both sides of read 4096.  Sorted and unsorted, int64 and int32."""
    bench = _bench()
    genomes, idx, orc = config2
    batches = [("<= 160 then 300-480", two_part(genomes, (4096, 10, 160), (20_000, 300, 480), 101)),
               ("161-320 then 321-2000", two_part(genomes, (4096, 161, 320), (20_000, 321, 2000), 103)),
               ("2-5 kbp then short", two_part(genomes, (4096, 2000, 5000), (50_000, 0, 60), 105))]
    lens = np.full(8192, 150, dtype=np.int64)
    lens[4088:4104] = [160, 161, 480, 481] * 4
    cat = np.concatenate(genomes)
    rng = np.random.default_rng(107)
    st = rng.integers(0, len(cat) - 500, size=len(lens))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    bases = synth.mutate(np.concatenate([cat[a:a + n] for a, n in zip(st, lens)]), 0.01, 108)
    batches.append(("160/161/480/481 around read 4096", (bases, off)))
    for what, (bases, off) in batches:
        B = DevBatch(bases, off, 30)
        want = oracle_of(orc, bases, off, bench.effective_cores())
        check_all(idx, B, want, [("%s int32 %s" % (name, i32), {"fused_sort": fs}, {"i32": i32})
                                 for name, fs in (("sorted", SORTED), ("unsorted", UNSORTED)) for i32 in (False, True)],
                  "sample contradicted, " + what)


# ---------------------------------------------------------------------------------------------------------------------
# the host-buffer entry points at scale
# ---------------------------------------------------------------------------------------------------------------------
def test_host_buffer_pipeline_at_scale(gpu, config2):
    """idx.streaming_search and idx.search_i32 on 2 M config-2 reads in pageable buffers: chunks of <= 128 MiB of results
    (search_host_pipelined), about 15 of them on two pipeline slots, whose workspaces the hint can switch to the sorted
    kernel partway through.  At the default "fused_sort", forced sorted and unsorted; every k-mer against the oracle."""
    import torch
    bench = _bench()
    genomes, idx, orc = config2
    bases = bench.gpu_reads(genomes, 2_000_000, 4343, torch.device("cuda:0")).cpu().numpy()
    off = np.arange(2_000_001, dtype=np.int64) * 150
    want = oracle_of(orc, bases, off, bench.effective_cores())
    for fs in (3632, SORTED, UNSORTED):
        with knobs(fused_sort=fs):
            got = idx.streaming_search(bases, off)[0]
            for a in range(0, len(want), CHUNK_KMERS):
                assert np.array_equal(got[a:a + CHUNK_KMERS], want[a:a + CHUNK_KMERS]), (fs, a)
            del got
            got = idx.search_i32(bases, off)[0]
            assert got.dtype == np.int32 and np.array_equal(got, want), fs
            del got
