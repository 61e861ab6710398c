"""GPU: reads threaded through the unitig graph (sbwtgpu_unitigs_walks_*) -- steps, step offsets and
unitig coverage exactly against the brute-force restatement of the definition (tests/walks_brute.py), against read_hits and
locate of search on the same batch, and through the C++ CLI.  The helpers and shapes are those of tests/test_gpu_unitig_links.py."""
import ctypes as C
import gzip
import itertools
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

from bruteforce import BruteSBWT
from colored_unitig_brute import sets_of_references
from test_gpu_colored_unitigs import KATS, build_sets, index_of, pieces_as_references, random_refs, refused
from test_gpu_unitig_links import from_device, hip_runtime, spread_refs, text
from test_gpu_unitigs import make_index, random_seqs
from unitig_links_brute import brute_colored_links, brute_links
from walks_brute import brute_walks, check_consequences, random_reads
from sbwt_amd import capi, hostlib, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")
STEP = capi.WALK_STEP


def raw(reads):
    return [r.encode("latin-1") if isinstance(r, str) else r for r in reads]


def as_steps(steps):
    return np.array([tuple(s) for s in steps], dtype=STEP) if len(steps) else np.zeros(0, dtype=STEP)


def graph_of(owner):
    return owner.unitig_graph_dev(links=False, column_map=True)


def run_walks(idx, owner, reads):
    """(step_off, steps, coverage) of the batch entry; the call without coverage gives the same first two."""
    with graph_of(owner) as u:
        so, st, cov = u.walks_reads(idx, raw(reads), coverage=True)
        so2, st2 = u.walks_reads(idx, raw(reads))
    assert so.dtype == np.int64 and st.dtype == STEP and cov.dtype == np.int64
    assert np.array_equal(so, so2) and st.tobytes() == st2.tobytes()
    return so, st, cov


def brute_graph(seqs, k, rc, refs=None, both=False):
    B = BruteSBWT(text(seqs), k, rc)
    if refs is None:
        return brute_links(B.kmers, k)
    return brute_colored_links(B.kmers, k, sets_of_references(B.kmers, k, [text(r) for r in refs], 2 if both else 1))


def cross_check(idx, owner, reads, so, st):
    """Against the existing calls on the same batch: read_hits' n_found, and locate of search, window by window."""
    bases, off = capi.concat_reads(raw(reads))
    hits = idx.read_hits(bases, off)
    assert [int(st["n_kmers"][a:b].sum()) for a, b in zip(so[:-1], so[1:])] == hits[:, 1].tolist()
    res, out_off = idx.search(bases, off)
    with graph_of(owner) as u:
        lu, lo = u.locate(res)
    eu = np.full(len(res), 0xFFFFFFFF, dtype=np.uint32)
    eo = np.full(len(res), 0xFFFFFFFF, dtype=np.uint32)
    read_of = np.repeat(np.arange(len(so) - 1), np.diff(so))
    for s, r in zip(st, read_of):
        a = out_off[r] + s["read_pos"]
        assert np.all(eu[a:a + s["n_kmers"]] == 0xFFFFFFFF)                  # steps do not overlap
        eu[a:a + s["n_kmers"]] = s["unitig"]
        eo[a:a + s["n_kmers"]] = s["offset"] + np.arange(s["n_kmers"], dtype=np.uint32)
    assert np.array_equal(eu, lu) and np.array_equal(eo, lo)


def check_brute(idx, owner, reads, k, G, label, cross=True):
    """The walks of `reads` over the graph handle of `owner` == the brute force on G = (U, link_off, link_to, where)."""
    U, lo, lt, where = G
    want_off, want_steps, want_cov = brute_walks(reads, k, where, len(U))
    so, st, cov = run_walks(idx, owner, reads)
    assert so.tolist() == want_off, label
    assert st.tobytes() == as_steps(want_steps).tobytes(), label
    assert cov.tolist() == want_cov, label
    check_consequences(reads, k, where, U, lo, lt, so.tolist(), [tuple(int(x) for x in s) for s in st])
    if cross:
        cross_check(idx, owner, reads, so, st)
    return so, st, cov


# ---- 1. hand cases, reference inputs, random sets -------------------------------------------------------------------------------
HAND = [
    (["AACG", "AACT"], None, ["AACGAACT"], [(0, 0, 0, 1), (1, 0, 1, 1), (0, 0, 4, 1), (2, 0, 5, 1)]),
    (["ACGTACG"], None, ["ACGTACGTACGT"], [(0, 2, 0, 2), (0, 0, 2, 4), (0, 0, 6, 4)]),
    (["AACCG", "CCGGTT"], None, ["AACCGGTT"], [(0, 0, 0, 6)]),
    (["AACCG", "CCGGTT"], [["AACCG"], ["CCGGTT"]], ["AACCGGTT"], [(0, 0, 0, 2), (1, 0, 2, 1), (2, 0, 3, 3)]),
    (["AACCGGTT"], None, ["AACCgGTT", "AACNGGTT", "AA", "", "TTTTT"], [(0, 0, 0, 2), (0, 5, 5, 1), (0, 0, 0, 1), (0, 4, 4, 2)]),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_cases(gpu, case):
    seqs, refs, reads, steps = HAND[case]
    _, idx = make_index(seqs, 3)
    G = brute_graph(seqs, 3, False, refs)
    if refs is None:
        so, st, cov = check_brute(idx, idx, reads, 3, G, case)
    else:
        with build_sets(idx, refs) as s:
            so, st, cov = check_brute(idx, s, reads, 3, G, case)
    assert st.tobytes() == as_steps(steps).tobytes()


def test_reference_inputs(gpu):
    rng = random.Random(2)
    cases = [("cli_end_to_end", KATS["cli_end_to_end"]["seqs"], KATS["cli_end_to_end"]["k"], KATS["cli_end_to_end"]["add_reverse_complements"]),
             ("redundant_dummies", KATS["redundant_dummies"]["seqs"], KATS["redundant_dummies"]["k"], False)]
    cases += [(c["name"], c["seqs"], c["k"], False) for c in KATS["small_cases"]["cases"] if c["k"] >= 2]
    for n_refs, (name, seqs, k, rc) in zip([2, 3, 4, 5] * len(cases), cases):
        _, idx = make_index(seqs, k, rc)
        reads = random_reads(rng, seqs, k) + list(seqs)
        check_brute(idx, idx, reads, k, brute_graph(seqs, k, rc), name)
        refs = pieces_as_references(seqs, n_refs, rng)
        with build_sets(idx, refs, rc) as s:
            check_brute(idx, s, reads, k, brute_graph(seqs, k, rc, refs, rc), (name, n_refs))


@pytest.mark.parametrize("k,rc", [(k, rc) for k in (2, 3, 4, 5, 8, 16, 31, 32, 33, 63, 64) for rc in (False, True)] + [(65, False)])
def test_random_sets(gpu, k, rc):
    rng = random.Random(200 * k + rc)
    seqs = random_seqs(rng, k)
    refs = random_refs(rng, seqs, k) + random_refs(rng, seqs, k)
    n_colors = [3, 70, 5, 65, 64, 66][(k + rc) % 6]
    _, idx = make_index(seqs, k, rc)
    reads = random_reads(rng, seqs, k, 30)
    so, st, cov = check_brute(idx, idx, reads, k, brute_graph(seqs, k, rc), (k, rc))
    assert len(st) > 0
    refs = spread_refs(rng, refs, n_colors)
    with build_sets(idx, refs, rc, n_colors) as s:
        check_brute(idx, s, reads, k, brute_graph(seqs, k, rc, refs, rc), (k, rc, n_colors))


def test_all_64_3mers_every_window_is_a_step(gpu):
    """The densest output: n_steps = W, which is also the capacity the batch entry gives the device call."""
    seqs = ["".join(p) for p in itertools.product("ACGT", repeat=3)]
    _, idx = make_index(seqs, 3)
    rng = random.Random(64)
    reads = ["".join(rng.choice("ACGT") for _ in range(n)) for n in (3, 10, 64, 66, 200, 2, 4500)]
    so, st, cov = check_brute(idx, idx, reads, 3, brute_graph(seqs, 3, False), "64")
    W = sum(max(0, len(r) - 2) for r in reads)
    assert len(st) == W == int(cov.sum()) and np.all(st["n_kmers"] == 1) and np.all(st["offset"] == 0)


# ---- 2. word and wave edges: one random 5.2 kbp sequence at k = 31, a single unitig ----------------------------------------------
K31 = 31


@pytest.fixture(scope="module")
def line(gpu):
    rng = random.Random(31)
    g = "".join(rng.choice("ACGT") for _ in range(5200))
    _, idx = make_index([g], K31)
    G = brute_graph([g], K31, False)
    assert len(G[0]) == 1                     # no repeated 30-mer: the sequence is one unitig
    return g, idx, G


@pytest.mark.parametrize("W", [63, 64, 65, 4095, 4096, 4097])
def test_batches_of_W_windows(line, W):
    g, idx, G = line
    rng = random.Random(W)
    reads, left = [], W
    while left > 0:
        m = min(left, rng.choice([1, 2, 30, 64, 100, 700]))
        a = rng.randrange(len(g) - m - K31)
        r = list(g[a:a + m + K31 - 1])
        if rng.random() < 0.4:
            r[rng.randrange(len(r))] = "N"
        reads.append("".join(r))
        left -= m
        if rng.random() < 0.2:
            reads.append(g[:rng.randrange(K31)])          # no window
    assert sum(max(0, len(r) - K31 + 1) for r in reads) == W
    check_brute(idx, idx, reads, K31, G, W)


def test_step_from_bit_63_to_bit_0(line):
    g, idx, G = line
    reads = [g[0:63 + 30], g[100:100 + 2 + 30], g[300:300 + 62 + 30], g[7:7 + 1 + 30], g[9:9 + 1 + 30]]
    so, st, cov = check_brute(idx, idx, reads, K31, G, "bit 63")
    # windows 63 and 64 of the batch are one step; window 127 (bit 63) and window 128 (bit 0) are steps of one window each
    assert [tuple(int(x) for x in s) for s in st] == [(0, 0, 0, 63), (0, 100, 0, 2), (0, 300, 0, 62), (0, 7, 0, 1), (0, 9, 0, 1)]


def test_one_step_longer_than_a_wave(line):
    g, idx, G = line
    so, st, cov = check_brute(idx, idx, [g], K31, G, "long")
    assert [tuple(int(x) for x in s) for s in st] == [(0, 0, 0, 5200 - 30)] and cov.tolist() == [5170]
    r = list(g)
    for p, c in ((1000, None), (2047, None), (4097, None), (3000, "N")):
        r[p] = c or "ACGT"[("ACGT".index(r[p]) + 1) % 4]
    so, st, cov = check_brute(idx, idx, ["".join(r), g[5:]], K31, G, "long with substitutions")
    assert len(st) == 6 and st["n_kmers"][0] == 1000 - 30 and st["n_kmers"][-1] == 5200 - 5 - 30


def test_read_boundaries_cut_steps(line):
    """The last window of the first read and the first of the second are consecutive k-mers of one unitig: two steps."""
    g, idx, G = line
    reads = [g[0:100], g[70:200], g[170:170 + 31], g[171:171 + 31]]
    so, st, cov = check_brute(idx, idx, reads, K31, G, "boundaries")
    assert so.tolist() == [0, 1, 2, 3, 4]
    assert [tuple(int(x) for x in s) for s in st] == [(0, 0, 0, 70), (0, 70, 0, 100), (0, 170, 0, 1), (0, 171, 0, 1)]


# ---- 3. degenerate inputs ----------------------------------------------------------------------------------------------------------
def test_degenerate_batches(line):
    g, idx, G = line
    # an empty batch, empty reads, reads shorter than k, a batch with no hit at all (other bases, N, lower case)
    for reads in ([], [""], ["", "", ""], [g[:30], "", g[:5]], ["T" * 40, "N" * 50, g[:60].lower()]):
        so, st, cov = check_brute(idx, idx, reads, K31, G, reads, cross=bool(reads))
        assert len(st) == 0 and int(cov.sum()) == 0 and np.all(so == 0) and len(so) == len(reads) + 1
    reads = [g[:40], g[100:140].lower(), g[200:231] + "N" + g[232:270], "", g[50:80]]
    so, st, cov = check_brute(idx, idx, reads, K31, G, "lower case and N")
    assert [tuple(int(x) for x in s) for s in st] == [(0, 0, 0, 10), (0, 200, 0, 1), (0, 232, 32, 8)]


# ---- 4. the device entry -------------------------------------------------------------------------------------------------------------
def test_device_entry(line):
    g, idx, G = line
    rng = random.Random(4)
    reads = random_reads(rng, [g], K31, 40) + [g[:2000]]
    want_off, want_steps, want_cov = brute_walks(reads, K31, G[3], len(G[0]))
    n_steps = len(want_steps)
    assert n_steps > 20
    bases, off = capi.concat_reads(raw(reads))
    lead = 13
    bases = np.concatenate([np.frombuffer(b"ACGTACGTACGTA", dtype=np.uint8), bases])          # d_read_off[0] != 0
    off = off + lead
    n, T = len(reads), len(bases)
    ws_bytes = capi.walks_workspace_bytes(T, n)
    assert ws_bytes >= capi.search_workspace_bytes(T) and capi.walks_workspace_bytes(T + 1, n) >= ws_bytes
    assert capi.walks_workspace_bytes(T, n + 1) >= ws_bytes
    hip = hip_runtime()
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    d = {name: C.c_void_p() for name in ("bases", "off", "so", "st", "cov", "ws")}
    stream = C.c_void_p()
    GUARD = 8
    sizes = {"bases": T, "off": (n + 1) * 8, "so": (n + 1 + GUARD) * 8, "st": (n_steps + GUARD) * 16, "cov": (1 + GUARD) * 8, "ws": ws_bytes}
    for name, p in d.items():
        assert hip.hipMalloc(C.byref(p), sizes[name]) == 0
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    assert hip.hipMemcpy(d["bases"], bases.ctypes.data, T, 1) == 0 and hip.hipMemcpy(d["off"], off.ctypes.data, (n + 1) * 8, 1) == 0
    with graph_of(idx) as u:
        refused(lambda: u.walks_dev(idx, d["bases"].value, T, d["off"].value, n, d["so"].value, d["st"].value, n_steps, 0, d["ws"].value,
                                    ws_bytes, stream.value), "not prepared")
        u.walks_prepare()
        u.walks_prepare()                                                            # twice: nothing changes
        for cap in (n_steps, n_steps - 7, 1, 0):
            for name in ("so", "st"):
                assert hip.hipMemset(d[name], 0x5A, sizes[name]) == 0
            assert hip.hipMemset(d["cov"], 0, sizes["cov"]) == 0
            for calls in (1, 2):
                u.walks_dev(idx, d["bases"].value, T, d["off"].value, n, d["so"].value, d["st"].value, cap, d["cov"].value, d["ws"].value,
                            ws_bytes, stream.value)
                assert hip.hipStreamSynchronize(stream) == 0
                assert idx.workspace_status(d["ws"].value, stream.value) == 0
                so = from_device(hip, d["so"], n + 1 + GUARD, np.int64)
                st = from_device(hip, d["st"], n_steps + GUARD, STEP)
                cov = from_device(hip, d["cov"], 1 + GUARD, np.int64)
                assert so[:n + 1].tolist() == want_off                                  # the true count, whatever the capacity
                assert st[:cap].tobytes() == as_steps(want_steps)[:cap].tobytes()
                assert st[cap:].tobytes() == b"\x5a" * (16 * (n_steps + GUARD - cap))    # nothing at or beyond steps_cap
                assert np.all(so[n + 1:] == 0x5A5A5A5A5A5A5A5A)
                assert cov.tolist() == [calls * want_cov[0]] + [0] * GUARD              # added onto what the array holds
        # no coverage asked for, the default stream
        assert hip.hipMemset(d["st"], 0x5A, sizes["st"]) == 0
        u.walks_dev(idx, d["bases"].value, T, d["off"].value, n, d["so"].value, d["st"].value, n_steps, 0, d["ws"].value, ws_bytes, 0)
        assert hip.hipStreamSynchronize(None) == 0
        assert from_device(hip, d["st"], n_steps, STEP).tobytes() == as_steps(want_steps).tobytes()
        # an empty batch: step_off[0] = 0
        assert hip.hipMemset(d["so"], 0x5A, 16) == 0
        u.walks_dev(idx, 0, 0, 0, 0, d["so"].value, 0, 0, 0, d["ws"].value, ws_bytes, stream.value)
        assert hip.hipStreamSynchronize(stream) == 0
        assert from_device(hip, d["so"], 2, np.int64).tolist() == [0, 0x5A5A5A5A5A5A5A5A]
    for p in d.values():
        assert hip.hipFree(p) == 0
    assert hip.hipStreamDestroy(stream) == 0


# ---- 5. the batch entry ----------------------------------------------------------------------------------------------------------------
def mixed_case(seed, k=21):
    rng = random.Random(seed)
    seqs = random_seqs(rng, k)
    seqs += [s[:60] + rng.choice("ACGT") + s[61:120] for s in seqs if len(s) > 130][:6]          # branches
    refs = random_refs(rng, seqs, k)
    reads = random_reads(rng, seqs, k, 60)
    return k, seqs, refs, reads


def test_chunks_threads_and_determinism(gpu):
    k, seqs, refs, reads = mixed_case(5)
    _, idx = make_index(seqs, k, True)
    with build_sets(idx, refs, True) as s:
        for owner, G in ((idx, brute_graph(seqs, k, True)), (s, brute_graph(seqs, k, True, refs, True))):
            one = check_brute(idx, owner, reads, k, G, "one chunk")
            again = run_walks(idx, owner, reads)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(one, again))
            capi.set_tuning("walks_chunk_bases", 1)                     # every read is a chunk of its own
            try:
                each = run_walks(idx, owner, reads)
            finally:
                capi.set_tuning("walks_chunk_bases", 0)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(one, each))
            with graph_of(owner) as u:                                  # two host threads on one handle, not prepared before
                errors = []

                def work():
                    try:
                        for _ in range(3):
                            got = u.walks_reads(idx, raw(reads), coverage=True)
                            assert all(a.tobytes() == b.tobytes() for a, b in zip(one, got))
                    except Exception as e:                # noqa: BLE001
                        errors.append(e)
                threads = [threading.Thread(target=work) for _ in range(2)]
                for t in threads:
                    t.start()
                for t in threads:
                    t.join()
                assert not errors, errors


# ---- 6. images and layouts ---------------------------------------------------------------------------------------------------------------
def test_image_layouts_and_marks(gpu):
    k, seqs, refs, reads = mixed_case(77, 15)
    bits, idx = make_index(seqs, k, True)
    want_plain = check_brute(idx, idx, reads, k, brute_graph(seqs, k, True), "layouts")
    with build_sets(idx, refs, True) as s:
        want = check_brute(idx, s, reads, k, brute_graph(seqs, k, True, refs, True), "layouts coloured")
        ids, table = s.copy()
        n_colors = s.n_colors
    variants = []
    for key, val, back in (("image_level", 1, 0), ("image_level", 2, 0), ("force_mega", 1, 0), ("big_path", 2, 1)):
        capi.set_tuning(key, val)
        try:
            variants.append(((key, val), make_index(seqs, k, True)[1]))
        finally:
            capi.set_tuning(key, back)
    for derive in (1, 0):               # no marks given: derived into the image, or into the call's scratch
        capi.set_tuning("derive_ssup", derive)
        try:
            for level in (0, 2):
                capi.set_tuning("image_level", level)
                variants.append((("no marks", derive, level), make_index(seqs, k, True, ssup=False)[1]))
        finally:
            capi.set_tuning("derive_ssup", 1)
            capi.set_tuning("image_level", 0)
    for name, other in variants:
        got = run_walks(other, other, reads)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(want_plain, got)), name
        with capi.ColorSets.from_arrays(other, n_colors, ids, table) as s:
            got = run_walks(other, s, reads)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(want, got)), name


def test_mega_block_layout(gpu, tmp_path):
    """Through the test build with mega blocks of 2^12 columns (a fresh child loads it; tests/walks_mega_worker.py): the bytes
    the product build gives."""
    lib = os.path.join(ROOT, "sbwt_amd", "lib", "libsbwtgpu_mega12.so")
    assert os.path.exists(lib), "%s is missing: build it with `python -m sbwt_amd.build`" % lib
    k = 31
    g0 = synth.random_genome(40_000, 5)
    seqs = [g0.tobytes(), synth.mutate(g0, 0.03, 6).tobytes()]
    bits = hostlib.build_bits(seqs, k, True, True)
    assert (bits.n_nodes >> 12) >= 30
    idx = index_of(bits, k)
    rng = random.Random(12)
    reads = [seqs[rng.randrange(2)][a:a + 150] for a in (rng.randrange(40_000 - 150) for _ in range(300))]
    bases, off = capi.concat_reads(reads)
    want_plain = run_walks(idx, idx, reads)
    with build_sets(idx, [[seqs[0]], [seqs[1]], [seqs[0][a:a + 400] for a in range(0, 40_000, 1000)]], True) as s:
        ids, table = s.copy()
        want = run_walks(idx, s, reads)
    assert len(want[1]) > len(want_plain[1]) > 300
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, A=bits.cols[0], C=bits.cols[1], G=bits.cols[2], T=bits.cols[3], ssup=bits.ssup, ids=ids, table=table, bases=bases, off=off,
             meta=np.array([bits.n_nodes, k, bits.n_kmers, 3], dtype=np.int64))
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tests", "walks_mega_worker.py"), fin, fout],
                       env=dict(os.environ, SBWTGPU_LIB=lib), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-4000:]
    out = np.load(fout, allow_pickle=False)
    assert "mega_shift=12" in str(out["version"])
    for image in ("rel1", "rel0", "big1", "big0"):
        for key, a, b in zip(("step_off", "steps", "coverage"), want_plain, want):
            assert a.tobytes() == out["%s/plain/%s" % (image, key)].tobytes(), (image, key)
            assert b.tobytes() == out["%s/colored/%s" % (image, key)].tobytes(), (image, key)


# ---- 7. refusals and handle behaviour ------------------------------------------------------------------------------------------------------
def test_refusals_and_handles(gpu):
    L = capi.lib()
    seqs = ["ACGTTGCATGCCGTAAGCTTAGGCATCGA", "TTTTGGGGCCCCAAAA"]
    bits, idx = make_index(seqs, 6)
    _, idx7 = make_index(seqs, 7)
    _, other = make_index(seqs + ["GGATCCGATTACA"], 6)
    reads = raw(seqs)
    bases, off = capi.concat_reads(reads)
    n = len(reads)
    buf = np.zeros(256, dtype=np.int64)
    ptr = buf.ctypes.data
    p, ns = C.c_void_p(), C.c_int64(0)

    def batch(i, u, b=bases.ctypes.data, o=off.ctypes.data, nr=n, so=ptr, po=C.byref(p), pn=C.byref(ns)):
        capi._check(L.sbwtgpu_unitigs_walks_batch(i, u, b, o, nr, so, po, pn, None))

    with idx.unitig_graph_dev(links=True, column_map=False) as u:                  # flags = LINKS only
        refused(lambda: u.walks_reads(idx, reads), "SBWTGPU_UNITIGS_COLUMN_MAP")
        refused(u.walks_prepare, "SBWTGPU_UNITIGS_COLUMN_MAP")
        refused(lambda: u.walks_dev(idx, ptr, 8, ptr, 1, ptr, ptr, 1, 0, ptr, 1 << 30), "SBWTGPU_UNITIGS_COLUMN_MAP")
    with idx.unitigs_dev() as u:
        refused(lambda: u.walks_reads(idx, reads), "SBWTGPU_UNITIGS_COLUMN_MAP")
    with graph_of(idx) as u:
        ws = capi.walks_workspace_bytes(64, 1)
        refused(lambda: u.walks_dev(idx, ptr, 64, ptr, 1, ptr, ptr, 1, 0, ptr, ws), "not prepared")
        want = u.walks_reads(idx, reads, coverage=True)                                    # (prepares)
        u.walks_prepare()
        u.walks_prepare()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(want, u.walks_reads(idx, reads, coverage=True)))
        refused(lambda: u.walks_reads(idx7, reads), "k = 7")                               # another k
        refused(lambda: u.walks_reads(other, reads), "not made from this index")           # another n_nodes
        refused(lambda: batch(None, u._h), "NULL")
        refused(lambda: batch(idx._h, None), "NULL")
        refused(lambda: batch(idx._h, u._h, so=None), "NULL")
        refused(lambda: batch(idx._h, u._h, po=None), "NULL")
        refused(lambda: batch(idx._h, u._h, pn=None), "NULL")
        refused(lambda: batch(idx._h, u._h, o=None), "NULL")
        refused(lambda: batch(idx._h, u._h, b=None), "NULL")
        refused(lambda: batch(idx._h, u._h, nr=-1), "negative n_reads")
        refused(lambda: u.walks_dev(idx, ptr, 64, ptr, -1, ptr, ptr, 1, 0, ptr, ws), "negative n_reads")
        refused(lambda: u.walks_dev(idx, ptr, 64, ptr, 1, ptr, ptr, -1, 0, ptr, ws), "negative steps_cap")
        refused(lambda: u.walks_dev(idx, ptr, 64, ptr, 1, ptr, ptr, 1, 0, ptr, ws - 1), "too small")
        refused(lambda: u.walks_dev(idx, ptr, 64, ptr, 1, ptr, ptr, 1, 0, None, ws), "workspace")
        refused(lambda: u.walks_dev(idx, ptr, 64, ptr, 1, None, ptr, 1, 0, ptr, ws), "NULL")
        refused(lambda: u.walks_dev(idx, ptr, 64, ptr, 1, ptr, None, 1, 0, ptr, ws), "NULL")
        refused(lambda: u.walks_dev(idx, ptr, 64, None, 1, ptr, ptr, 1, 0, ptr, ws), "NULL")
        refused(lambda: u.walks_dev(idx, None, 64, ptr, 1, ptr, ptr, 1, 0, ptr, ws), "NULL")
        too_long = np.array([0, 1 << 31], dtype=np.int64)
        with pytest.raises(capi.SbwtGpuError) as e:
            batch(idx._h, u._h, o=too_long.ctypes.data, nr=1)
        assert e.value.code == capi.ERR_READ_TOO_LONG
        w = np.random.default_rng(1).integers(0, 2**64, size=4, dtype=np.uint64)
        ro = capi.Index.create(w, w, w, w, None, 256, 3)
        refused(lambda: u.walks_reads(ro, reads), "only rank()")
        refused(lambda: capi._check(L.sbwtgpu_unitigs_walks_prepare(None)), "NULL")
        assert capi.walks_workspace_bytes(-5, -5) == capi.walks_workspace_bytes(0, 0) > 0
        # flag bit 4 stays an unknown flag
        h = C.c_void_p()
        refused(lambda: capi._check(L.sbwtgpu_unitigs_create_graph(idx._h, None, 4, C.byref(h))), "unknown flag")
        # the handle serves its other calls unchanged after a walks call, and so does a handle made beside it
        assert all(a.tobytes() == b.tobytes() for a, b in zip(want, u.walks_reads(idx, reads, coverage=True)))


def test_index_of_2_pow_31_columns_is_refused(gpu):
    """Refused for its size before anything else, by both entries: any bits make an index that answers rank(), and any
    graph handle will do, because the handle is looked at only afterwards."""
    n = 1 << 31
    w = np.zeros(n // 64, dtype=np.uint64)
    big = capi.Index.create(w, w, w, w, None, n, 31, 0, 0)
    _, small = make_index(["ACGTTGCATGCCGTAAGCTTAGGCATCGA"], 6)
    reads = [b"ACGTTGCATGCC"]
    buf = np.zeros(64, dtype=np.int64)
    ptr = buf.ctypes.data
    with graph_of(small) as u:
        u.walks_prepare()
        refused(lambda: u.walks_reads(big, reads), "2^31", "columns")
        refused(lambda: u.walks_reads(big, reads, coverage=True), "2^31", "columns")
        refused(lambda: u.walks_dev(big, ptr, 64, ptr, 1, ptr, ptr, 1, 0, ptr, capi.walks_workspace_bytes(64, 1)), "2^31", "columns")
        assert len(u.walks_reads(small, reads)[1]) == 1                            # the handle is usable afterwards
    with small.unitigs_dev() as u:                                                 # even a handle without the map: the size comes first
        refused(lambda: u.walks_reads(big, reads), "2^31", "columns")
    big.close()


def test_existing_create_calls_unaffected(gpu):
    k, seqs, refs, reads = mixed_case(9)
    _, idx = make_index(seqs, k, True)

    def everything(owner):
        with owner.unitig_graph_dev(links=True, column_map=True) as u:
            return [a.tobytes() for a in u.copy() + u.links() + u.column_map()]
    with build_sets(idx, refs, True) as s:
        before = everything(idx), everything(s), [a.tobytes() for a in idx.unitigs()]
        with graph_of(s) as u, graph_of(idx) as v:
            u.walks_reads(idx, raw(reads), coverage=True)
            v.walks_reads(idx, raw(reads))
            assert [a.tobytes() for a in v.copy() + v.column_map()] == before[0][:3] + before[0][5:]
            after = everything(idx), everything(s), [a.tobytes() for a in idx.unitigs()]
    assert before == after


# ---- 8. the CLI ------------------------------------------------------------------------------------------------------------------------------
def run(cmd, timeout=300):
    return subprocess.run(cmd, capture_output=True, timeout=timeout)


def parse_walks(data, n_reads):
    lines = data.decode().split("\n")
    assert lines[-1] == "" and len(lines) == n_reads + 1
    step_off, steps = [0], []
    for r, ln in enumerate(lines[:-1]):
        f = ln.split(" ")
        assert f[0] == str(r)
        for t in f[1:]:
            p, u, o, nk = (int(x) for x in t.split(":"))
            steps.append((u, o, p, nk))
        step_off.append(len(steps))
    return step_off, steps


def test_cli_thread(gpu, tmp_path):
    d = str(tmp_path)
    c = KATS["cli_end_to_end"]
    k, seqs, rc = c["k"], c["seqs"], c["add_reverse_complements"]
    with open(d + "/in.fna", "w") as fh:
        for i, s in enumerate(seqs):
            fh.write(">%d\n%s\n" % (i, s))
    p = run([SBWT, "build", "-i", d + "/in.fna", "-o", d + "/i.sbwt", "-k", str(k)] + (["--add-reverse-complements"] if rc else []))
    assert p.returncode == 0, p.stderr.decode()
    rng = random.Random(15)
    refs = pieces_as_references(seqs, 3, rng)
    with open(d + "/refs.txt", "w") as fh:
        for ci, mine in enumerate(refs):
            name = "%s/ref%d.fna" % (d, ci)
            with open(name, "w") as out:
                out.write("".join(">r%d_%d\n%s\n" % (ci, j, s) for j, s in enumerate(mine)))
            fh.write(name + "\n")
    p = run([SBWT, "build-colors", "-i", d + "/i.sbwt", "-r", d + "/refs.txt", "-o", d + "/c.colors", "--compress"] + (["--both-strands"] if rc else []))
    assert p.returncode == 0, p.stderr.decode()
    # (a FASTQ record needs a base; the CLI's reader upper-cases what it reads)
    reads = [r.upper() for r in random_reads(rng, seqs, k, 40) if r] + ["AC"]
    fastq = "".join("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)) for i, r in enumerate(reads)).encode()
    open(d + "/reads.fastq", "wb").write(fastq)
    with gzip.open(d + "/reads.fastq.gz", "wb") as fh:
        fh.write(fastq)
    bits, idx = make_index(seqs, k, rc)
    with build_sets(idx, refs, rc) as s:
        want_colored = run_walks(idx, s, reads)
        with graph_of(s) as u:
            n_kmers_colored = np.diff(u.copy()[1]) - (k - 1)
    want_plain = run_walks(idx, idx, reads)
    with graph_of(idx) as u:
        n_kmers_plain = np.diff(u.copy()[1]) - (k - 1)
    assert len(want_colored[1]) > len(want_plain[1]) > 0
    for colored, want, nk in ((False, want_plain, n_kmers_plain), (True, want_colored, n_kmers_colored)):
        extra = ["--colors", d + "/c.colors"] if colored else []
        p = run([SBWT, "dump-unitigs", "-i", d + "/i.sbwt", "-o", d + "/u.gfa", "--gfa"] + extra)
        assert p.returncode == 0, p.stderr.decode()
        gfa = open(d + "/u.gfa", "rb").read()
        for z in (False, True):
            q = d + "/reads.fastq" + (".gz" if z else "")
            out = d + "/walks.txt" + (".gz" if z else "")
            p = run([SBWT, "thread", "-i", d + "/i.sbwt", "-q", q, "-o", out, "--coverage", d + "/cov.tsv", "--gfa", d + "/kc.gfa"] + extra +
                    (["-z"] if z else []))
            assert p.returncode == 0, p.stderr.decode()
            so, steps = parse_walks(gzip.open(out).read() if z else open(out, "rb").read(), len(reads))
            assert so == want[0].tolist() and as_steps(steps).tobytes() == want[1].tobytes()
            cov = [ln.split("\t") for ln in open(d + "/cov.tsv").read().split("\n")[:-1]]
            assert cov == [[str(i), str(a), str(b)] for i, (a, b) in enumerate(zip(nk.tolist(), want[2].tolist()))]
            kc = open(d + "/kc.gfa", "rb").read().split(b"\n")
            seg = 0
            for i, ln in enumerate(kc):
                if ln.startswith(b"S\t"):
                    tag = b"\tKC:i:%d" % want[2][seg]
                    assert ln.endswith(tag)
                    kc[i] = ln[:-len(tag)]
                    seg += 1
            assert seg == len(nk) and b"\n".join(kc) == gfa                     # stripped of its KC tags: dump-unitigs --gfa
