"""GPU: every route the library takes from k = 64 on, on branching indexes of many image blocks (tests/long_k_cases.py),
bit for bit against the oracle.

From k = 64 the image has a path order, the depth-31 sparse table and the probe filter but no second-level table (no whole k-mer
lives in a table), batches go to the general path kernel instead of the wide fused one, and the paths carry no safe bits.
The first test pins that down from the image's header; the others run search and streaming search (kernels 0, 1, 4, 5, dense
tables of depth 0, 2, 8, a shallower file table, marks given / derived / absent), the image levels and layouts, every entry
point (host and device buffers, int64 and int32, result ranges with gaps, two streams), long reads, matching statistics and
the LCS array, read hits, the column API, the documented refusals of the device builder's neighbours, the CLI and a bounded
fuzz on the same k.  tests/test_long_k_cpu.py checks the references themselves and that the cases are not vacuous."""
import os
import subprocess
import sys

import numpy as np
import pytest

import long_k_cases
from long_k_cases import KS, N_THREADS, oracle_of, oracle_results
from ms_brute import format_ms
from oracle import print_vector
from read_hits_brute import format_table, profile_of_hits
from sbwt_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")
DEFAULT_IMAGE = int(os.environ.get("SBWTGPU_IMAGE_LEVEL", "0")) == 0      # (a knob sweep may force levels 1 and 2 from outside)


class tuning:
    """set_tuning for the length of a with-block"""

    def __init__(self, key, value, back):
        self.key, self.value, self.back = key, value, back

    def __enter__(self):
        capi.set_tuning(self.key, self.value)

    def __exit__(self, *exc):
        capi.set_tuning(self.key, self.back)


def create(bits, marks=True, precalc_k=0, precalc=None) -> capi.Index:
    return capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup if marks else None, bits.n_nodes,
                             bits.k, bits.n_kmers, precalc_k, precalc)


@pytest.fixture(scope="module")
def indexes(gpu):
    """k -> (case, the index with marks, the index without): built once per module, on first use"""
    made = {}

    def get(k):
        if k not in made:
            case = long_k_cases.build_case(k)
            made[k] = (case, create(case.bits), create(case.bits_nomarks, marks=False))
        return made[k]
    return get


def check_both(idx, case, what):
    assert np.array_equal(idx.streaming_search(case.bases, case.off)[0], case.want_streaming), ("streaming_search", case.k, what)
    assert np.array_equal(idx.search(case.bases, case.off)[0], case.want_search), ("search", case.k, what)


def dev_call(idx, bases, off, k, streaming, i32=False, ooff=None, total=None, fill=-7):
    """One device-pointer call; the whole result array (gaps included) as int64."""
    import torch
    dev = torch.device("cuda:0")
    ooff = capi.out_offsets(off, k) if ooff is None else ooff
    total = int(ooff[-1]) if total is None else total
    d_b = torch.from_numpy(np.ascontiguousarray(bases)).to(dev)
    d_ro, d_oo = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to(dev), torch.from_numpy(np.ascontiguousarray(ooff)).to(dev)
    d_out = torch.full((total,), fill, dtype=torch.int32 if i32 else torch.int64, device=dev)
    wsb = capi.search_workspace_bytes(d_b.numel())
    d_ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    fn = idx.streaming_search_dev_i32 if i32 else idx.streaming_search_dev
    fn(d_b.data_ptr(), d_b.numel(), d_ro.data_ptr(), len(off) - 1, d_out.data_ptr(), d_oo.data_ptr(), d_ws.data_ptr(), wsb,
       torch.cuda.current_stream().cuda_stream, streaming)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().astype(np.int64)


def members_of_branching_groups(bits) -> int:
    n = bits.n_nodes
    deg = sum(np.unpackbits(c.view(np.uint8), bitorder="little")[:n].astype(np.int8) for c in bits.cols)
    marks = np.unpackbits(bits.ssup.view(np.uint8), bitorder="little")[:n]
    start = np.maximum.accumulate(np.where(marks == 1, np.arange(n), 0))          # the first column of every column's group
    return int((deg[start] >= 2).sum())


# ---- the image is the one meant ----
@pytest.mark.parametrize("k", KS)
def test_the_image_has_a_path_order_a_depth_31_table_and_no_second_level(indexes, k):
    case, idx, plain = indexes(k)
    h = idx.image_header()
    assert (h.k, h.n_nodes, h.has_ssup, h.rank_only, h.big_layout) == (k, case.bits.n_nodes, 1, 0, 0)
    # n_branch counts the path POSITIONS whose column's suffix group has two or more successors: every member of such a group,
    # and the copies that stitched chains hold of them; without stitching it is the members exactly
    members = members_of_branching_groups(case.bits)
    assert members >= case.conditions["branching"] >= 100 and idx.n_branch >= members
    if DEFAULT_IMAGE:
        with tuning("path_stitch", 0, 1):
            assert create(case.bits).n_branch == members
    assert h.n_blocks == case.bits.n_nodes // 64 + 1 and h.n_blocks > 300
    if DEFAULT_IMAGE:
        assert h.image_level == 0 and h.has_path == 1 and h.n_paths > 0 and idx.default_search_variant == 5
        assert h.p_sparse == 31 and h.n_sb > 0
        assert h.n_sb2 == 0 and h.off_stab2 == 0
        assert h.p_filter > 0 and h.p_file == 0 and (h.p_dev == 8 or "SBWTGPU_DEVICE_PRECALC" in os.environ)
        g = plain.image_header()                              # marks derived on the device: the same structures
        assert (g.has_ssup, g.ssup_derived, g.has_path, g.p_sparse, g.n_sb2) == (0, 1, 1, 31, 0)
    if k == 64 and DEFAULT_IMAGE:                             # ... and one k below the boundary the second level is there
        b63 = long_k_cases.hostlib.build_bits(case.seqs[:4], 63, False, True, n_threads=4)
        assert create(b63).image_header().n_sb2 > 0


# ---- search and streaming search ----
@pytest.mark.parametrize("k", KS)
def test_every_search_kernel(indexes, k):
    case, idx, _ = indexes(k)
    check_both(idx, case, "default")
    for variant in (0, 1, 4, 5):
        with tuning("search_variant", variant, -1):
            check_both(idx, case, variant)


@pytest.mark.parametrize("k", KS)
def test_dense_tables_of_depth_0_2_8_and_a_shallower_file_table(indexes, k):
    case, _, _ = indexes(k)
    before = os.environ.get("SBWTGPU_DEVICE_PRECALC")
    try:
        for p_dev in (0, 2, 8):
            os.environ["SBWTGPU_DEVICE_PRECALC"] = str(p_dev)
            idx = create(case.bits)
            h = idx.image_header()
            assert h.p_dev == p_dev and idx.device_precalc_k == p_dev and h.n_sb2 == 0
            if DEFAULT_IMAGE:                                     # (the sparse table stands on the dense one)
                assert h.p_sparse == (0 if p_dev == 0 else 31)
            check_both(idx, case, ("p_dev", p_dev))
        os.environ["SBWTGPU_DEVICE_PRECALC"] = "8"
        file_orc = oracle_of(case.bits, True, 2)
        idx = create(case.bits, precalc_k=2, precalc=file_orc.precalc())
        h = idx.image_header()
        assert (h.p_file, h.p_dev) == (2, 8) and h.off_ftab != h.off_ptab
        assert np.array_equal(idx.get_precalc(), file_orc.precalc())
        check_both(idx, case, "file table 2, device table 8")
    finally:
        if before is None:
            del os.environ["SBWTGPU_DEVICE_PRECALC"]
        else:
            os.environ["SBWTGPU_DEVICE_PRECALC"] = before


@pytest.mark.parametrize("derive", [1, 0])
@pytest.mark.parametrize("k", KS)
def test_index_without_marks(indexes, k, derive):
    case, _, _ = indexes(k)
    with tuning("derive_ssup", derive, 1):
        idx = create(case.bits_nomarks, marks=False)
        assert not idx.has_streaming_support
        assert idx.image_header().ssup_derived == derive
        with pytest.raises(capi.SbwtGpuError) as ei:
            idx.streaming_search(case.bases, case.off)            # "not built", like the reference
        assert ei.value.code == capi.ERR_NO_STREAMING
        for variant in (-1, 0, 1, 4, 5):
            with tuning("search_variant", variant, -1):
                assert np.array_equal(idx.search(case.bases, case.off)[0], case.want_search), (k, derive, variant)
        assert np.array_equal(idx.search_i32(case.bases, case.off, streaming=False)[0], case.want_search)


# ---- image levels and layouts ----
@pytest.mark.parametrize("k", KS)
def test_image_levels_and_layouts(indexes, k):
    case, default, _ = indexes(k)
    plain_bytes = default.blob_bytes
    for level in (0, 1, 2):
        with tuning("image_level", level, 0):
            idx = create(case.bits)
        h = idx.image_header()
        assert idx.image_level == level and h.has_path == (1 if level == 0 else 0) and h.n_sb2 == 0
        assert (h.p_sparse > 0) == (level < 2)
        check_both(idx, case, ("image_level", level))
        assert np.array_equal(dev_call(idx, case.bases, case.off, k, True), case.want_streaming), level
    # "force_mega" changes rank-only images only (include/sbwtgpu.h): the image of an SBWT must come out as without it, byte
    # count and answers (the relative-count layout on SBWTs is tested by the build with small mega blocks, test_gpu_mega_small.py)
    with tuning("force_mega", 1, 0):
        idx = create(case.bits)
    assert idx.blob_bytes == plain_bytes and idx.image_header().n_mega == 1
    check_both(idx, case, "force_mega")
    # the layout of 2^31 columns takes whole k-mers in its tables: not from k = 64 on, and the ordinary image is built
    with tuning("big_path", 2, 1):
        idx = create(case.bits)
        nomarks = create(case.bits_nomarks, marks=False)
    h = idx.image_header()
    assert h.big_layout == 0 and h.image_level == 0 and h.n_sb2 == 0 and h.has_path == 1 and h.p_sparse == 31
    check_both(idx, case, "big_path 2")
    assert np.array_equal(dev_call(idx, case.bases, case.off, k, True), case.want_streaming)
    assert np.array_equal(nomarks.search(case.bases, case.off)[0], case.want_search)


# ---- entry points ----
@pytest.mark.parametrize("k", KS)
def test_host_and_device_entry_points_int64_and_int32(indexes, k):
    case, idx, _ = indexes(k)
    for streaming, want in ((True, case.want_streaming), (False, case.want_search)):
        got32, oo = idx.search_i32(case.bases, case.off, streaming=streaming)
        assert got32.dtype == np.int32 and np.array_equal(oo, case.out_off) and np.array_equal(got32, want), (k, streaming)
        assert np.array_equal(dev_call(idx, case.bases, case.off, k, streaming), want), (k, streaming)
        assert np.array_equal(dev_call(idx, case.bases, case.off, k, streaming, i32=True), want), (k, streaming)
        for variant in (1, 4):
            with tuning("search_variant", variant, -1):
                assert np.array_equal(dev_call(idx, case.bases, case.off, k, streaming, i32=True), want), (k, streaming, variant)


@pytest.mark.parametrize("i32", [False, True])
@pytest.mark.parametrize("k", KS)
def test_result_ranges_with_gaps(indexes, k, i32):
    case, idx, _ = indexes(k)
    m = np.diff(case.out_off)
    rng = np.random.default_rng(k)
    # (the poison fills out[out_off[0] .. out_off[n]), gaps included; back to 1 afterwards: what conftest's `gpu` fixture sets for
    # the whole session, not the library's default)
    with tuning("poison_results", 0, 1):
        for gap in (rng.integers(0, 9, size=len(m)), (-m) % 16):
            starts = np.concatenate([[3], 3 + np.cumsum(m + gap)])[:-1]
            ooff = np.concatenate([starts, [starts[-1] + m[-1]]]).astype(np.int64)
            total = int(starts[-1] + m[-1] + gap[-1]) + 5
            inside = np.zeros(total, dtype=bool)
            for r in np.flatnonzero(m):
                inside[starts[r]:starts[r] + m[r]] = True
            for streaming, want in ((True, case.want_streaming), (False, case.want_search)):
                got = dev_call(idx, case.bases, case.off, k, streaming, i32=i32, ooff=ooff, total=total)
                assert np.array_equal(got[inside], want), (k, i32, streaming)
                assert (got[~inside] == -7).all(), (k, i32, streaming)


@pytest.mark.parametrize("k", KS)
def test_two_batches_in_flight_on_two_streams(indexes, k):
    import torch
    case, idx, _ = indexes(k)
    dev = torch.device("cuda:0")
    half = (len(case.off) - 1) // 2
    a0, a1 = int(case.off[half]), int(case.off[-1])
    parts = [(case.bases[:a0], case.off[:half + 1]), (case.bases[a0:a1], case.off[half:] - a0)]
    split = int(case.out_off[half])
    wants = [(case.want_streaming[:split], case.want_search[:split]), (case.want_streaming[split:], case.want_search[split:])]
    sets = []
    for q, (bases, off) in enumerate(parts):                    # every buffer of every launch first: a workspace and results per batch
        ooff = capi.out_offsets(off, k)
        d = {"bases": torch.from_numpy(np.ascontiguousarray(bases)).to(dev), "off": torch.from_numpy(np.ascontiguousarray(off)).to(dev),
             "ooff": torch.from_numpy(ooff).to(dev), "n": len(off) - 1, "stream": torch.cuda.Stream(device=dev),
             "out": {(s, w): torch.full((int(ooff[-1]),), -7, dtype=torch.int32 if w else torch.int64, device=dev)
                     for s in (True, False) for w in (False, True)}}
        d["wsb"] = capi.search_workspace_bytes(d["bases"].numel())
        d["ws"] = torch.zeros(d["wsb"], dtype=torch.uint8, device=dev)
        sets.append(d)
    torch.cuda.synchronize()
    for rep in range(8):                                        # launches of the two batches alternate; nothing waits in between
        d, streaming, i32 = sets[rep & 1], not (rep & 2), bool(rep & 4)
        fn = idx.streaming_search_dev_i32 if i32 else idx.streaming_search_dev
        fn(d["bases"].data_ptr(), d["bases"].numel(), d["off"].data_ptr(), d["n"], d["out"][(streaming, i32)].data_ptr(),
           d["ooff"].data_ptr(), d["ws"].data_ptr(), d["wsb"], d["stream"].cuda_stream, streaming)
    torch.cuda.synchronize()
    for q, d in enumerate(sets):
        for (streaming, i32), out in d["out"].items():
            assert np.array_equal(out.cpu().numpy().astype(np.int64), wants[q][0 if streaming else 1]), (k, q, streaming, i32)


# ---- long reads ----
@pytest.mark.parametrize("k", [64, 255])
def test_long_reads_among_short_ones(indexes, k):
    case, idx, _ = indexes(k)
    tiles = [synth.mutate(case.strains[i % 4], 0.005, 100 * k + i) for i in range(28)]
    long200 = np.concatenate(tiles)[:200_000].copy()
    long20 = np.concatenate(tiles[5:8])[1000:21_000].copy()
    long200[70_000:70_400] = np.frombuffer(long200[70_000:70_400].tobytes().lower(), dtype=np.uint8)     # across cut points
    long200[123_456] = ord("N")
    long20[9_999] = ord("n")
    short = case.reads[:40]
    reads = short[:25] + [long20.tobytes()] + short[25:33] + [long200.tobytes()] + short[33:]
    bases, off = capi.concat_reads(reads)
    want_s = oracle_results(case.orc, bases, off)
    want_n = oracle_results(case.orc_nomarks, bases, off)
    oo = capi.out_offsets(off, k)
    assert (want_s >= 0).mean() > 0.15 and (want_s[oo[34]:oo[35]] >= 0).sum() > 10_000
    for table in (1, 0):
        with tuning("fused_table", table, 1):
            assert np.array_equal(idx.streaming_search(bases, off)[0], want_s), (k, table)
            assert np.array_equal(idx.search(bases, off)[0], want_n), (k, table)
            assert np.array_equal(dev_call(idx, bases, off, k, True), want_s), (k, table)          # cut on the device
            assert np.array_equal(dev_call(idx, bases, off, k, False, i32=True), want_n), (k, table)
    with tuning("split_long", 0, 1):
        assert np.array_equal(dev_call(idx, bases, off, k, True), want_s), k
    for r in (25, 34):                                          # the same read searched alone
        one = np.frombuffer(reads[r], dtype=np.uint8)
        o1 = np.array([0, len(one)], dtype=np.int64)
        assert np.array_equal(idx.streaming_search(one, o1)[0], want_s[oo[r]:oo[r + 1]]), (k, r)
        assert np.array_equal(dev_call(idx, one, o1, k, True), want_s[oo[r]:oo[r + 1]]), (k, r)
        assert np.array_equal(dev_call(idx, one, o1, k, False), want_n[oo[r]:oo[r + 1]]), (k, r)


# ---- matching statistics and LCS ----
@pytest.mark.parametrize("k", KS)
def test_matching_statistics_on_every_position_and_lcs_on_every_column(indexes, k):
    """Every position of the whole batch against the exhaustive oracle, which tries every length from min(run, k) down at every
    position: next to a substitution that is k^2 / 2 steps, so the reference itself takes a second at k = 128 and several at
    k = 255 (by threads); the device calls take milliseconds."""
    case, idx, plain = indexes(k)
    lcs = case.orc.lcs(None, N_THREADS)
    assert lcs.max() == k - 1 and lcs[0] == 0
    bases, off = case.bases, case.off
    ln, first, second, _ = case.orc.matching_statistics(bases, off, N_THREADS, True)
    assert (ln == k).any() and (ln == 0).any() and ((ln > 0) & (ln < k)).any()
    oo = case.out_off
    hit_at = np.concatenate([off[r] + k - 1 + np.arange(oo[r + 1] - oo[r]) for r in range(len(off) - 1)]).astype(np.int64)
    assert np.array_equal(ln[hit_at] == k, case.want_search >= 0)                    # len == k exactly where the k-mer is found
    for which in (idx, plain):                                  # with and without marks
        assert np.array_equal(which.lcs(), lcs), k
        g_ln, g_first, g_second = which.matching_statistics(bases, off)
        assert np.array_equal(g_ln, ln) and np.array_equal(g_first, first) and np.array_equal(g_second, second), k
        assert np.array_equal(which.matching_statistics(bases, off, intervals=False), ln), k


# ---- read hits ----
def mirrored(bases, off):
    comp = np.arange(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    return np.ascontiguousarray(comp[bases[::-1]]), (len(bases) - off[::-1]).astype(np.int64)


@pytest.mark.parametrize("k", KS)
def test_read_hits_one_strand_and_both(indexes, k):
    case, idx, plain = indexes(k)
    oo, m = case.out_off, np.diff(case.out_off)
    assert set((oo[:-1][m > 0] % 64).tolist()) == set(range(64))              # reads start at every bit of a word of hit flags
    assert m.max() >= 1024                                                     # ... and some are reduced by a whole wave
    fwd = case.want_search >= 0
    rb, ro = mirrored(case.bases, case.off)
    either = fwd | (oracle_results(case.orc_nomarks, rb, ro) >= 0)[::-1]
    want1 = np.array([profile_of_hits(fwd[oo[r]:oo[r + 1]].tolist(), k) for r in range(len(m))], dtype=np.int32).reshape(len(m), 4)
    want2 = want1.copy()
    for r in range(len(m)):
        if not np.array_equal(fwd[oo[r]:oo[r + 1]], either[oo[r]:oo[r + 1]]):
            want2[r] = profile_of_hits(either[oo[r]:oo[r + 1]].tolist(), k)
    # (an index that holds the reverse complements finds on one strand what it finds on both)
    assert (want2[:, 1] > want1[:, 1]).any() == (not case.revcomp) and (want1[:, 3] >= 128).any()
    for wave_min in (1024, 128):
        with tuning("read_hits_wave_min", wave_min, 1024):
            for which in (idx, plain):
                assert np.array_equal(which.read_hits(case.bases, case.off, False), want1), (k, wave_min)
                assert np.array_equal(which.read_hits(case.bases, case.off, True), want2), (k, wave_min)
    with tuning("read_hits_wide", 1, 0):
        assert np.array_equal(idx.read_hits(case.bases, case.off, True), want2), k


# ---- the column API ----
def labels_of_every_column(case):
    """The k characters of every column from the rows alone: the last character of column v is the row whose range of C holds v,
    and the column it is entered from holds the (v - C[c] + 1)-th one of that row; '$' at the root."""
    n, k = case.bits.n_nodes, case.k
    last = np.full(n, ord("$"), dtype=np.uint8)
    pred = np.zeros(n, dtype=np.int64)
    at = 1
    for ci, ch in enumerate(b"ACGT"):
        ones = np.flatnonzero(np.unpackbits(case.bits.cols[ci].view(np.uint8), bitorder="little")[:n])
        last[at:at + len(ones)] = ch
        pred[at:at + len(ones)] = ones
        at += len(ones)
    assert at == n
    out = np.empty((n, k), dtype=np.uint8)
    cur = np.arange(n)
    for i in range(k):
        out[:, k - 1 - i] = last[cur]
        cur = pred[cur]
    return out


@pytest.mark.parametrize("k", KS)
def test_column_api_get_kmers_select_forward_rank(indexes, k):
    case, idx, _ = indexes(k)
    orc, n = case.orc, case.bits.n_nodes
    rng = np.random.default_rng(k)
    labels = labels_of_every_column(case)
    for v in np.concatenate([[0, 1, n - 1], rng.integers(0, n, size=150)]):
        assert labels[v].tobytes() == orc.get_kmer(int(v)), int(v)
    got = idx.get_kmers(np.arange(n))
    assert got.shape == (n, k) and got.strides == (k, 1) and np.array_equal(got, labels)      # k bytes per column, stride k
    back = idx.get_kmers(np.arange(n)[::-1])
    assert np.array_equal(back, labels[::-1])
    for ci, ch in enumerate(b"ACGT"):                                                     # every one of every row
        ones = np.flatnonzero(np.unpackbits(case.bits.cols[ci].view(np.uint8), bitorder="little")[:n])
        for j in (1, len(ones) // 2, len(ones)):
            assert orc.select(j, bytes([ch])) == ones[j - 1]
        assert np.array_equal(idx.select(np.arange(1, len(ones) + 1), np.full(len(ones), ch, dtype=np.uint8)), ones)
        with pytest.raises(capi.SbwtGpuError):
            idx.select(np.array([len(ones) + 1]), np.array([ch], dtype=np.uint8))
    node = np.repeat(np.arange(n), 4)
    sym = np.tile(np.frombuffer(b"ACGT", dtype=np.uint8), n)
    want = np.array([orc.forward(int(v), bytes([int(c)])) for v, c in zip(node, sym)], dtype=np.int64)
    assert (want >= 0).sum() >= n - 1 and (want == -1).any()
    assert np.array_equal(idx.forward(node, sym), want)
    edges = np.arange(0, n + 64, 64)
    pos = np.unique(np.clip(np.concatenate([edges - 1, edges, edges + 1, [0, n - 1, n]]), 0, n))
    pos, sym = np.repeat(pos, 6), np.tile(np.frombuffer(b"ACGTNa", dtype=np.uint8), len(pos))
    assert np.array_equal(idx.rank(pos, sym), orc.batch_rank(pos, sym, 1)[0])


@pytest.mark.parametrize("k", KS)
def test_column_api_update_interval_and_partial_search(indexes, k):
    case, idx, _ = indexes(k)
    orc, n = case.orc, case.bits.n_nodes
    rng = np.random.default_rng(100 + k)
    queries = []
    for L in (1, 30, 31, 32, 33, 63, 64, 65, k - 1, k, k + 1):
        for t in range(24):
            s = case.strains[t % 4]
            a = int(rng.integers(0, len(s) - L))
            q = bytearray(s[a:a + L].tobytes())
            if t % 6 == 1:
                q[int(rng.integers(0, L))] = ord("ACGT"[int(rng.integers(0, 4))])
            elif t % 6 == 2:
                q[int(rng.integers(0, L))] = ord("N")
            elif t % 6 == 3:
                q = bytearray(bytes(q).lower())
            elif t % 6 == 4:
                q = bytearray(synth.random_genome(L, 7 * L + t).tobytes())
            queries.append(bytes(q))
        queries.append(case.seqs[5][:L] if L <= len(case.seqs[5]) else case.seqs[5])          # the head of a lone sequence: dummies
    bases, off = capi.concat_reads(queries)
    first, second, matched = idx.partial_search(bases, off)
    want = [orc.partial_search(q) for q in queries]
    assert [(int(a), int(b), int(c)) for a, b, c in zip(first, second, matched)] == [(w[0][0], w[0][1], w[1]) for w in want]
    assert max(w[1] for w in want) == k + 1 and min(w[1] for w in want) < 30
    # update_interval: from the whole range, and from the interval of a character
    for f0, s0 in ((0, n - 1), orc.update_interval(b"G", 0, n - 1)):
        a, b = idx.update_interval(bases, off, np.full(len(queries), f0), np.full(len(queries), s0))
        want = [orc.update_interval(q, f0, s0) for q in queries]
        assert list(zip(a.tolist(), b.tolist())) == want
        assert any(w[0] >= 0 for w in want) and any(w == (-1, -1) for w in want)


# ---- refusals ----
def test_device_builder_set_operations_and_key_export_refuse_k_65(indexes):
    case, idx, _ = indexes(65)
    with pytest.raises(capi.SbwtGpuError) as ei:
        capi.build_bits_gpu(case.seqs[:4], 65)
    assert ei.value.code == capi.ERR_INVALID_ARG and ei.value.msg == "the device builder packs a k-mer into 64 or 128 bits: 2 <= k <= 64"
    check_both(idx, case, "after the builder's refusal")
    for call, who in ((lambda: idx.setop(idx, "union"), "sbwtgpu_index_setop"),
                      (lambda: idx.setop(idx, "difference", False), "sbwtgpu_index_setop"),
                      (lambda: idx.setop_counts(idx), "sbwtgpu_index_setop_counts"),
                      (lambda: idx.kmer_keys(), "sbwtgpu_index_kmer_keys")):
        with pytest.raises(capi.SbwtGpuError) as ei:
            call()
        assert ei.value.code == capi.ERR_INVALID_ARG, who
        assert ei.value.msg.endswith("k = 65, the keys of the device builder hold 2 <= k <= 64"), ei.value.msg
    check_both(idx, case, "after the refusals")
    _, idx64, _ = indexes(64)                                   # ... and one k below they all work
    assert idx64.setop_counts(idx64)["n_both"] == idx64.n_kmers and idx64.kmer_keys().shape == (idx64.n_kmers, 2)


# ---- the CLI ----
def test_cli_build_search_matching_statistics_read_hits_at_k_96(indexes, tmp_path):
    k = 96
    case, _, _ = indexes(k)
    d = str(tmp_path)
    with open(d + "/s.fna", "wb") as fh:
        fh.write(b"".join(b">s%d\n%s\n" % (i, s) for i, s in enumerate(case.seqs)))

    def run(*args):
        p = subprocess.run([SBWT] + list(args), capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode()
        return p
    run("build", "-i", d + "/s.fna", "-o", d + "/i.sbwt", "-k", str(k), "--add-reverse-complements", "--temp-dir", d)
    f = long_k_cases.hostlib.read_index_file(d + "/i.sbwt")
    assert (f.n_nodes, f.n_kmers, f.k) == (case.bits.n_nodes, case.bits.n_kmers, k)
    assert all(np.array_equal(a, b) for a, b in zip(f.cols, case.bits.cols)) and np.array_equal(f.ssup, case.bits.ssup)
    # (the sequence reader upper-cases what it reads and takes text: reads of A, C, G, T, N here)
    pick = [r for r in range(len(case.reads)) if case.reads[r] and not case.reads[r].strip(b"ACGTN")]
    assert len(pick) > 900
    reads = [case.reads[r] for r in pick]
    with open(d + "/r.fq", "wb") as fh:
        fh.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (j, r, b"I" * len(r)) for j, r in enumerate(reads)))
    oo = case.out_off
    run("search", "-i", d + "/i.sbwt", "-q", d + "/r.fq", "-o", d + "/search.out")
    assert open(d + "/search.out", "rb").read() == b"".join(print_vector(case.want_streaming[oo[r]:oo[r + 1]]) for r in pick)
    hits = [(case.want_search[oo[r]:oo[r + 1]] >= 0).tolist() for r in pick]
    run("read-hits", "-i", d + "/i.sbwt", "-q", d + "/r.fq", "-o", d + "/hits.out")
    assert open(d + "/hits.out", "rb").read() == format_table(profile_of_hits(h, k) for h in hits)
    few = reads[:120]
    with open(d + "/few.fna", "wb") as fh:
        fh.write(b"".join(b">r%d\n%s\n" % (j, r) for j, r in enumerate(few)))
    b, o = capi.concat_reads(few)
    ln, first, second, _ = case.orc.matching_statistics(b, o, N_THREADS, True)
    run("matching-statistics", "-i", d + "/i.sbwt", "-q", d + "/few.fna", "-o", d + "/ms.out")
    assert open(d + "/ms.out", "rb").read() == b"".join(format_ms(ln[o[j]:o[j + 1]]) for j in range(len(few)))
    run("matching-statistics", "-i", d + "/i.sbwt", "-q", d + "/few.fna", "-o", d + "/msi.out", "--intervals")
    assert open(d + "/msi.out", "rb").read() == b"".join(format_ms(ln[o[j]:o[j + 1]], first[o[j]:o[j + 1]], second[o[j]:o[j + 1]])
                                                         for j in range(len(few)))


# ---- fuzz ----
@pytest.mark.parametrize("seed", [64, 255])
def test_fuzz_all_routes_agree_from_k_64_on(gpu, seed):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_gpu
    stats = {}
    assert fuzz_gpu.fuzz(120.0, seed, max_cases=4, k_choices=list(KS), stats=stats, oracle_every=1) == 4
    assert stats["compared"] >= 3 and stats["oracle"] >= 1, stats             # (a case whose genomes are all shorter than its reads compares nothing)
