"""GPU: the unitig graph (sbwtgpu_unitigs_create_graph) -- the links between the unitigs, the column
map and locate -- exactly against the brute-force restatement of the definition (tests/unitig_links_brute.py), by construction
against streaming_search, at a moderate shape against numpy on the rows of the matrix, and through the C++ CLI as GFA.  The
helpers and shapes are those of tests/test_gpu_unitigs.py and tests/test_gpu_colored_unitigs.py."""
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
from test_gpu_colored_unitigs import KATS, build_sets, circular, index_of, pieces_as_references, random_refs, refused
from test_gpu_unitigs import make_index, random_seqs, split
from unitig_brute import flatten
from unitig_links_brute import brute_colored_links, brute_links, column_map, n_edges
from sbwt_amd import capi, hostlib, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")
NONE = 0xFFFFFFFF
KEYS = ("bases", "off", "first", "link_off", "link_to", "col_unitig", "col_offset")


def text(seqs):
    return [s.decode() if isinstance(s, bytes) else s for s in seqs]


def run_graph(owner, links=True, column_map=True):
    """Everything a graph handle of an Index or a ColorSets holds, as a dict of arrays."""
    with owner.unitig_graph_dev(links=links, column_map=column_map) as u:
        b, o, f = u.copy()
        g = {"bases": b, "off": o, "first": f}
        if links:
            g["link_off"], g["link_to"] = u.links()
            assert u.n_links() == len(g["link_to"]) == g["link_off"][-1]
        if column_map:
            g["col_unitig"], g["col_offset"] = u.column_map()
        if isinstance(owner, capi.ColorSets):
            g["set_id"] = u.set_ids()
        return g


def hip_runtime():
    """The HIP runtime the library loaded, for device buffers of the test's own."""
    hip = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    return hip


def from_device(hip, ptr, count, dtype):
    back = np.zeros(count, dtype=dtype)
    assert hip.hipMemcpy(back.ctypes.data, ptr, back.nbytes, 2) == 0          # (2: device to host)
    return back


def check_located(idx, g, owner):
    """By construction: streaming_search over the unitigs gives column c at window r of unitig i, so the map at c is (i, r),
    every other column is a dummy, and locate of the search results (on a map-only handle of `owner`) says the same."""
    res, out_off = idx.streaming_search(g["bases"], g["off"])
    n_win = np.diff(out_off)
    want_u = np.repeat(np.arange(len(n_win), dtype=np.uint32), n_win)
    want_r = (np.arange(len(res), dtype=np.int64) - np.repeat(out_off[:-1], n_win)).astype(np.uint32)
    assert len(res) == 0 or res.min() >= 0
    cu = np.full(idx.n_nodes, NONE, dtype=np.uint32)
    co = np.full(idx.n_nodes, NONE, dtype=np.uint32)
    cu[res], co[res] = want_u, want_r
    assert np.array_equal(g["col_unitig"], cu) and np.array_equal(g["col_offset"], co)
    with owner.unitig_graph_dev(links=False, column_map=True) as u:
        lu, lr = u.locate(res)
    assert np.array_equal(lu, want_u) and np.array_equal(lr, want_r)
    return res, out_off


def check_brute(idx, seqs, k, rc, label, refs=None, both=False, n_colors=None):
    """The graph of the plain run (refs is None) or of the coloured run == the brute force, exactly; returns the API result."""
    B = BruteSBWT(text(seqs), k, rc)
    assert idx.n_nodes == len(B.nodes), label
    if refs is None:
        U, lo, lt, where = brute_links(B.kmers, k)
        g = run_graph(idx)
        check_located(idx, g, idx)
    else:
        sets = sets_of_references(B.kmers, k, [text(r) for r in refs], 2 if both else 1)
        U, lo, lt, where = brute_colored_links(B.kmers, k, sets)
        with build_sets(idx, refs, both, n_colors) as s:
            g = run_graph(s)
            check_located(idx, g, s)
    want_bases, want_off = flatten(U)
    assert g["off"].tolist() == want_off and g["bases"].tobytes() == want_bases, label
    assert g["link_off"].dtype == np.int64 and g["link_to"].dtype == np.uint32
    assert g["link_off"].tolist() == lo, label
    assert g["link_to"].tolist() == lt, label
    assert len(lt) == n_edges(B.kmers) - (len(B.kmers) - len(U)), label
    cu, co = column_map(B, where)
    assert g["col_unitig"].tolist() == cu and g["col_offset"].tolist() == co, label
    return g


# ---- 1. the hand cases and the reference inputs ---------------------------------------------------------------------------------
HAND = [
    (["AACG", "AACT"], None, [b"AAC", b"ACG", b"ACT"], [0, 2, 2, 2], [1, 2]),
    (["AAAAA"], None, [b"AAA"], [0, 1], [0]),
    (["ACGTACG"], None, [b"GTACGT"], [0, 1], [0]),
    (["AACCG", "CCGGTT"], None, [b"AACCGGTT"], [0, 0], []),
    (["AACCG", "CCGGTT"], [["AACCG"], ["CCGGTT"]], [b"AACC", b"CCG", b"CGGTT"], [0, 1, 2, 2], [1, 2]),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_cases(gpu, case):
    seqs, refs, unitigs, link_off, link_to = HAND[case]
    _, idx = make_index(seqs, 3)
    g = check_brute(idx, seqs, 3, False, case, refs)
    assert split(g["bases"], g["off"]) == unitigs
    assert g["link_off"].tolist() == link_off and g["link_to"].tolist() == link_to


def test_all_64_3mers(gpu):
    """Out-degree 4 on every tail, suffix groups of four columns."""
    seqs = ["".join(p) for p in itertools.product("ACGT", repeat=3)]
    bits, idx = make_index(seqs, 3)
    marks = np.unpackbits(bits.ssup.view(np.uint8), bitorder="little")[:bits.n_nodes]
    assert bits.n_kmers == 64 and int(marks.sum()) <= 1 + 16 + 4 + 16          # (16 groups of four real columns)
    g = check_brute(idx, seqs, 3, False, "64")
    assert len(g["first"]) == 64 and g["link_off"].tolist() == list(range(0, 257, 4))
    U = split(g["bases"], g["off"])
    for i, u in enumerate(U):
        assert [U[j] for j in g["link_to"][4 * i:4 * i + 4]] == [u[1:] + c for c in (b"A", b"C", b"G", b"T")]
    refs = [[s for s in seqs if s[0] in "AC"], [s for s in seqs if s[1] in "CG"], seqs[::3]]
    check_brute(idx, seqs, 3, False, "64 coloured", refs)


def test_reference_inputs(gpu):
    rng = random.Random(1)
    cases = [("cli_end_to_end", KATS["cli_end_to_end"]["seqs"], KATS["cli_end_to_end"]["k"], KATS["cli_end_to_end"]["add_reverse_complements"]),
             ("redundant_dummies", KATS["redundant_dummies"]["seqs"], KATS["redundant_dummies"]["k"], False)]
    cases += [(c["name"], c["seqs"], c["k"], False) for c in KATS["small_cases"]["cases"] if c["k"] >= 2]
    for n_refs, (name, seqs, k, rc) in zip([2, 3, 4, 5] * len(cases), cases):
        _, idx = make_index(seqs, k, rc)
        check_brute(idx, seqs, k, rc, name)
        check_brute(idx, seqs, k, rc, (name, n_refs), pieces_as_references(seqs, n_refs, rng), rc)


# ---- 2. random sets -----------------------------------------------------------------------------------------------------------------
def spread_refs(rng, refs, n_colors):
    """The references dealt onto n_colors colours, the last colour always used (beyond 64 colours: the second word of a row)."""
    out = [[] for _ in range(n_colors)]
    slots = rng.sample(range(n_colors - 1), min(len(refs), n_colors) - 1) + [n_colors - 1]
    for c, mine in zip(slots, refs):
        out[c] = mine
    return out


@pytest.mark.parametrize("k", [2, 3, 4, 5, 8, 16, 31, 32, 33, 63, 64])
@pytest.mark.parametrize("rc", [False, True])
def test_random_sets(gpu, k, rc):
    rng = random.Random(100 * k + rc)
    seqs = random_seqs(rng, k)
    refs = random_refs(rng, seqs, k) + random_refs(rng, seqs, k)
    n_colors = [3, 70, 5, 65, 64, 66][(k + rc) % 6]
    _, idx = make_index(seqs, k, rc)
    check_brute(idx, seqs, k, rc, (k, rc))
    g = check_brute(idx, seqs, k, rc, (k, rc, n_colors), spread_refs(rng, refs, n_colors), rc, n_colors)
    assert len(g["first"]) > 0


# ---- 3. cycles ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 8, 31])
def test_pure_cycles_and_cycles_with_breaks(gpu, k):
    rng = random.Random(k)

    def rnd(n):
        return "".join(rng.choice("ACGT") for _ in range(n))
    one, two = rnd(k + 20), rnd(k + 33)
    cases = {"one cycle": [circular(one, k)], "two cycles": [circular(one, k), circular(two, k)], "self-loop": ["A" * (k + 3)],
             "self-loop and cycle": ["C" * k, circular(one, k)], "cycle and tail": [rnd(k + 4) + circular(one, k)]}
    if k == 3:
        one = "ACGT"
        cases = {"one cycle": [circular("ACGT", 3)], "two cycles": [circular("ACGT", 3), circular("AAG", 3)],
                 "self-loop": ["AAAAA"], "cycle and tail": ["CACGTACG"]}
    for name, seqs in cases.items():
        for rc in (False, True):
            _, idx = make_index(seqs, k, rc)
            check_brute(idx, seqs, k, rc, (name, rc))
    for name in ("one cycle", "self-loop"):                   # a cut pure cycle links to itself
        _, idx = make_index(cases[name], k)
        g = run_graph(idx)
        assert g["link_off"].tolist() == [0, 1] and g["link_to"].tolist() == [0], name
    # the cycle in arcs of different sets: every break is a link to the next piece, round the cycle
    seq = cases["one cycle"][0]
    _, idx = make_index([seq], k)
    L = len(one)
    trip = one * 3
    for cuts in ([0, L // 2], [1, 1 + L // 3, 1 + 2 * (L // 3)]):
        refs = [[seq]] + [[trip[a:a + ((z - a) % L or L) + k - 1]] for a, z in zip(cuts[1:], cuts[2:] + cuts[:1])]
        g = check_brute(idx, [seq], k, False, ("arcs", len(cuts)), refs)
        n = len(g["first"])
        assert n == len(cuts) and g["link_off"].tolist() == list(range(n + 1))
        assert sorted(g["link_to"].tolist()) == list(range(n)) and all(g["link_to"][i] != i for i in range(n))


# ---- 4. suffix groups across the 64-column words ------------------------------------------------------------------------------------
def test_groups_straddle_word_boundaries(gpu):
    """A dense k-mer set has groups of two to four columns everywhere, so some begin in one 64-column word of the marks and
    end in the next: the tails there find their group's first column in the previous word.  (Half of all 6-mers: some 2000
    real columns; over the alphabet AC alone k <= 5 gives 32 k-mers at most, which test_random_sets covers.)"""
    rng = random.Random(64)
    k = 6
    seqs = ["".join(p) for p in itertools.product("ACGT", repeat=k) if rng.random() < 0.5]
    bits, idx = make_index(seqs, k)
    assert 2000 <= bits.n_nodes <= 6000
    marks = np.unpackbits(bits.ssup.view(np.uint8), bitorder="little")[:bits.n_nodes]
    at = np.arange(64, bits.n_nodes, 64)
    assert int((marks[at] == 0).sum()) >= 5                   # a word's column 0 continues the group of the word before
    g = check_brute(idx, seqs, k, False, "dense")
    assert int((marks[at] == 0).sum()) <= int(((g["col_unitig"][at] != NONE) & (marks[at] == 0)).sum())   # real columns, all of them
    refs = [[s for s in seqs if rng.random() < 0.6] for _ in range(3)]
    check_brute(idx, seqs, k, False, "dense coloured", refs)


# ---- 5. layouts ---------------------------------------------------------------------------------------------------------------------------
def test_image_layouts_and_marks(gpu):
    rng = random.Random(77)
    k = 15
    seqs = ["".join(rng.choice("ACGT") for _ in range(rng.randint(20, 300))) for _ in range(12)]
    seqs += [s[:80] + rng.choice("ACGT") + s[81:160] for s in seqs[:6]]               # branches
    seqs.append(circular("".join(rng.choice("ACGT") for _ in range(k + 9)), k))
    refs = random_refs(rng, seqs, k)
    bits, idx = make_index(seqs, k, True)
    want_plain = check_brute(idx, seqs, k, True, "layouts")
    want = check_brute(idx, seqs, k, True, "layouts coloured", refs, True)
    assert len(want["link_to"]) > len(want_plain["link_to"]) > 0
    with build_sets(idx, refs, True) as s:
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
        got = run_graph(other)
        for key in KEYS:
            assert np.array_equal(want_plain[key], got[key]), (name, key)
        with capi.ColorSets.from_arrays(other, n_colors, ids, table) as s:
            got = run_graph(s)
        for key in KEYS + ("set_id",):
            assert np.array_equal(want[key], got[key]), (name, key)


def test_mega_block_layout(gpu, tmp_path):
    """The MEGA instantiations of the link kernels, through the test build with mega blocks of 2^12 columns (a fresh child
    loads it; tests/unitig_links_mega_worker.py): the bytes the product build gives."""
    lib = os.path.join(ROOT, "sbwt_amd", "lib", "libsbwtgpu_mega12.so")
    assert os.path.exists(lib), "%s is missing: build it with `python -m sbwt_amd.build`" % lib
    k = 31
    g0 = synth.random_genome(40_000, 5)
    seqs = [g0.tobytes(), synth.mutate(g0, 0.03, 6).tobytes()]
    bits = hostlib.build_bits(seqs, k, True, True)
    assert (bits.n_nodes >> 12) >= 30
    idx = index_of(bits, k)
    want_plain = run_graph(idx)
    with build_sets(idx, [[seqs[0]], [seqs[1]], [seqs[0][a:a + 400] for a in range(0, 40_000, 1000)]], True) as s:
        ids, table = s.copy()
        want = run_graph(s)
    assert len(want["link_to"]) > len(want_plain["link_to"]) + 50 > 100
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, A=bits.cols[0], C=bits.cols[1], G=bits.cols[2], T=bits.cols[3], ssup=bits.ssup, ids=ids, table=table,
             meta=np.array([bits.n_nodes, k, bits.n_kmers, 3], dtype=np.int64))
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tests", "unitig_links_mega_worker.py"), fin, fout],
                       env=dict(os.environ, SBWTGPU_LIB=lib), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-4000:]
    out = np.load(fout, allow_pickle=False)
    assert "mega_shift=12" in str(out["version"])
    for image in ("rel1", "rel0", "big1", "big0"):
        for key in KEYS:
            assert np.array_equal(want_plain[key], out["%s/plain/%s" % (image, key)]), (image, key)
            assert np.array_equal(want[key], out["%s/colored/%s" % (image, key)]), (image, key)


# ---- 6. locate ------------------------------------------------------------------------------------------------------------------------------
def test_locate_sentinels_and_device_entry(gpu):
    rng = random.Random(6)
    k = 12
    seqs = random_seqs(rng, k)
    bits, idx = make_index(seqs, k, True)
    with idx.unitig_graph_dev(links=False, column_map=True) as u:
        cu, co = u.column_map()
        dummies = np.flatnonzero(cu == NONE)
        assert len(dummies) > 1 and dummies[0] == 0 and np.array_equal(cu == NONE, co == NONE)
        real = np.flatnonzero(cu != NONE)
        assert len(real) == bits.n_kmers
        cols = np.array([-1, 0, int(dummies[-1]), idx.n_nodes, idx.n_nodes + 5, 1 << 40, -(1 << 62), int(real[0]), int(real[-1]),
                         idx.n_nodes - 1], dtype=np.int64)
        lu, lr = u.locate(cols)
        assert np.all(lu[:7] == NONE) and np.all(lr[:7] == NONE)
        assert np.array_equal(lu[7:], cu[cols[7:]]) and np.array_equal(lr[7:], co[cols[7:]])
        assert lu[7] != NONE and lu[8] != NONE
        assert all(len(a) == 0 for a in u.locate(np.zeros(0, dtype=np.int64)))
        # the device entry point on the caller's stream, and the device pointers of the map
        every = np.arange(-3, idx.n_nodes + 3, dtype=np.int64)
        hip = hip_runtime()
        m = len(every)
        fill = np.full(m + 8, 0x5A5A5A5A, dtype=np.uint32)
        d_cols, d_u, d_r, stream = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(d_cols), m * 8) == 0 and hip.hipMalloc(C.byref(d_u), fill.nbytes) == 0
        assert hip.hipMalloc(C.byref(d_r), fill.nbytes) == 0 and hip.hipStreamCreate(C.byref(stream)) == 0
        assert hip.hipMemcpy(d_cols, every.ctypes.data, m * 8, 1) == 0          # (1: host to device)
        assert hip.hipMemcpy(d_u, fill.ctypes.data, fill.nbytes, 1) == 0 and hip.hipMemcpy(d_r, fill.ctypes.data, fill.nbytes, 1) == 0
        u.locate_dev(d_cols.value, m, d_u.value, d_r.value, stream.value)
        assert hip.hipStreamSynchronize(stream) == 0
        hu, hr = from_device(hip, d_u, m + 8, np.uint32), from_device(hip, d_r, m + 8, np.uint32)
        for p in (d_cols, d_u, d_r):
            assert hip.hipFree(p) == 0
        assert hip.hipStreamDestroy(stream) == 0
        assert np.all(hu[m:] == 0x5A5A5A5A) and np.all(hr[m:] == 0x5A5A5A5A)      # nothing past n
        pad = np.full(3, NONE, dtype=np.uint32)
        assert np.array_equal(hu[:m], np.concatenate([pad, cu, pad]))
        assert np.array_equal(hr[:m], np.concatenate([pad, co, pad]))
        d_cu, d_co = u.column_map_dev()
        assert np.array_equal(from_device(hip, d_cu, idx.n_nodes, np.uint32), cu)
        assert np.array_equal(from_device(hip, d_co, idx.n_nodes, np.uint32), co)


# ---- 7. flags = 0, determinism, bounds ----------------------------------------------------------------------------------------------------
def test_flags_zero_is_the_existing_call(gpu):
    rng = random.Random(7)
    k = 21
    seqs = random_seqs(rng, k) + [circular("".join(rng.choice("ACGT") for _ in range(k + 30)), k)]
    bits, idx = make_index(seqs, k, True)
    want = idx.unitigs()
    with idx.unitig_graph_dev(links=False, column_map=False) as u:
        for a, b in zip(want, u.copy()):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        assert u.graph_stats() == {"links_ms": 0.0, "map_ms": 0.0}
        refused(u.links, "SBWTGPU_UNITIGS_LINKS")
        refused(u.column_map, "SBWTGPU_UNITIGS_COLUMN_MAP")
    with build_sets(idx, random_refs(rng, seqs, k), True) as s:
        want = s.unitigs()
        with s.unitig_graph_dev(links=False, column_map=False) as u:
            for a, b in zip(want, u.copy() + (u.set_ids(),)):
                assert a.dtype == b.dtype and np.array_equal(a, b)
            ci = u.color_info()
        with s.unitigs_dev() as u:
            assert u.color_info() == ci
        # and the flags change nothing of what the existing calls give
        g = run_graph(s)
        for a, key in zip(want, ("bases", "off", "first", "set_id")):
            assert np.array_equal(a, g[key])
    g = run_graph(idx)
    for a, key in zip(idx.unitigs(), ("bases", "off", "first")):
        assert np.array_equal(a, g[key])


def test_determinism_and_bounds(gpu):
    rng = random.Random(5)
    k = 21
    seqs = random_seqs(rng, k)
    seqs += [s[:60] + rng.choice("ACGT") + s[61:120] for s in seqs if len(s) > 130][:6]          # branches: links of the plain run
    refs = random_refs(rng, seqs, k)
    bits, idx = make_index(seqs, k, True)
    with build_sets(idx, refs, True) as s:
        for owner in (idx, s):
            r1, r2 = run_graph(owner), run_graph(owner)
            for key in KEYS:
                assert r1[key].tobytes() == r2[key].tobytes(), key
            with owner.unitig_graph_dev(links=True, column_map=True) as u:
                n, m, nn = u.n_unitigs, u.n_links(), idx.n_nodes
                assert m > 0
                G = 64
                ho = np.full(n + 1 + 2 * G, -7, dtype=np.int64)
                ht = np.full(m + 2 * G, 0xA5A5A5A5, dtype=np.uint32)
                hu = np.full(nn + 2 * G, 0xA5A5A5A5, dtype=np.uint32)
                hr = np.full(nn + 2 * G, 0xA5A5A5A5, dtype=np.uint32)
                capi._check(capi.lib().sbwtgpu_unitigs_links_copy(u._h, ho[G:].ctypes.data, ht[G:].ctypes.data))
                capi._check(capi.lib().sbwtgpu_unitigs_column_map_copy(u._h, hu[G:].ctypes.data, hr[G:].ctypes.data))
                for arr, cnt, fill in ((ho, n + 1, -7), (ht, m, 0xA5A5A5A5), (hu, nn, 0xA5A5A5A5), (hr, nn, 0xA5A5A5A5)):
                    assert np.all(arr[:G] == fill) and np.all(arr[G + cnt:] == fill)
                assert np.array_equal(ho[G:G + n + 1], r1["link_off"]) and np.array_equal(ht[G:G + m], r1["link_to"])
                assert np.array_equal(hu[G:G + nn], r1["col_unitig"]) and np.array_equal(hr[G:G + nn], r1["col_offset"])
                assert int(ht[G:G + m].max()) < n
                # the device pointers hold the same bytes
                d_lo, d_lt = u.links_dev()
                hip = hip_runtime()
                assert np.array_equal(from_device(hip, d_lo, n + 1, np.int64), r1["link_off"])
                assert np.array_equal(from_device(hip, d_lt, m, np.uint32), r1["link_to"])
                st = u.graph_stats()
                assert st["links_ms"] > 0 and st["map_ms"] > 0
                assert set(u.stats()["pass_ms"]) and u.stats()["jump_rounds"] >= 0          # _stats serves the handle unchanged


def test_two_host_threads(gpu):
    rng = random.Random(12)
    k = 17
    seqs = random_seqs(rng, k)
    bits, idx = make_index(seqs, k, True)
    want = run_graph(idx)
    cols = np.arange(-2, idx.n_nodes + 2, dtype=np.int64)
    with idx.unitig_graph_dev(links=True, column_map=True) as u:
        want_loc = u.locate(cols)
        errors = []

        def work():
            try:
                for _ in range(3):
                    lo, lt = u.links()
                    a, b = u.locate(cols)
                    assert np.array_equal(lo, want["link_off"]) and np.array_equal(lt, want["link_to"])
                    assert np.array_equal(a, want_loc[0]) and np.array_equal(b, want_loc[1])
                    g = run_graph(idx)
                    assert all(np.array_equal(g[key], want[key]) for key in KEYS)
            except Exception as e:                # noqa: BLE001
                errors.append(e)
        threads = [threading.Thread(target=work) for _ in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors


# ---- 8. refusals and empties --------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    L = capi.lib()
    seqs = ["ACGTTGCATGCCGTAAGCTTAGGCATCGA", "TTTTGGGGCCCCAAAA"]
    bits, idx = make_index(seqs, 6)
    h = C.c_void_p()
    n, p, q = C.c_int64(), C.c_void_p(), C.c_void_p()
    buf = np.zeros(idx.n_nodes + 64, dtype=np.int64)
    ptr = buf.ctypes.data
    with build_sets(idx, [[seqs[0]]]) as s:
        refused(lambda: capi._check(L.sbwtgpu_unitigs_create_graph(idx._h, s.handle, 1, C.byref(h))), "exactly one", "both")
        refused(lambda: capi._check(L.sbwtgpu_unitigs_create_graph(None, None, 1, C.byref(h))), "exactly one", "neither")
        refused(lambda: capi._check(L.sbwtgpu_unitigs_create_graph(idx._h, None, 4, C.byref(h))), "unknown flag")
        refused(lambda: capi._check(L.sbwtgpu_unitigs_create_graph(None, s.handle, 0x80000001, C.byref(h))), "unknown flag")
        refused(lambda: capi._check(L.sbwtgpu_unitigs_create_graph(idx._h, None, 3, None)), "NULL")
        with s.unitig_graph_dev(links=True, column_map=False) as u:              # links only
            assert u.n_links() >= 0 and len(u.links()) == 2
            refused(u.column_map, "SBWTGPU_UNITIGS_COLUMN_MAP")
            refused(u.column_map_dev, "SBWTGPU_UNITIGS_COLUMN_MAP")
            refused(lambda: u.locate(np.zeros(3, dtype=np.int64)), "SBWTGPU_UNITIGS_COLUMN_MAP")
            refused(lambda: u.locate_dev(0, 0, 0, 0), "SBWTGPU_UNITIGS_COLUMN_MAP")
            refused(lambda: capi._check(L.sbwtgpu_unitigs_links_info(u._h, None)), "NULL")
            refused(lambda: capi._check(L.sbwtgpu_unitigs_links_dev(u._h, None, C.byref(q))), "NULL")
            refused(lambda: capi._check(L.sbwtgpu_unitigs_links_dev(u._h, C.byref(p), None)), "NULL")
            refused(lambda: capi._check(L.sbwtgpu_unitigs_links_copy(u._h, None, ptr)), "NULL")
            if u.n_links():
                refused(lambda: capi._check(L.sbwtgpu_unitigs_links_copy(u._h, ptr, None)), "NULL")
            assert len(u.set_ids()) == u.n_unitigs and u.color_info()["n_colors"] == 1          # the coloured calls serve it
        with idx.unitig_graph_dev(links=False, column_map=True) as u:            # map only
            refused(u.n_links, "SBWTGPU_UNITIGS_LINKS")
            refused(u.links_dev, "SBWTGPU_UNITIGS_LINKS")
            refused(u.links, "SBWTGPU_UNITIGS_LINKS")
            refused(u.set_ids, "sbwtgpu_unitigs_create_colored")                 # a plain run carries no colours
            refused(lambda: capi._check(L.sbwtgpu_unitigs_column_map_dev(u._h, None, C.byref(q))), "NULL")
            refused(lambda: capi._check(L.sbwtgpu_unitigs_column_map_dev(u._h, C.byref(p), None)), "NULL")
            refused(lambda: capi._check(L.sbwtgpu_unitigs_column_map_copy(u._h, None, ptr)), "NULL")
            refused(lambda: capi._check(L.sbwtgpu_unitigs_column_map_copy(u._h, ptr, None)), "NULL")
            refused(lambda: capi._check(L.sbwtgpu_unitigs_locate_batch(u._h, ptr, -1, ptr, ptr)), "negative")
            refused(lambda: capi._check(L.sbwtgpu_unitigs_locate_batch(u._h, None, 2, ptr, ptr)), "NULL")
            refused(lambda: capi._check(L.sbwtgpu_unitigs_locate_batch(u._h, ptr, 2, None, ptr)), "NULL")
            refused(lambda: capi._check(L.sbwtgpu_unitigs_locate_batch(u._h, ptr, 2, ptr, None)), "NULL")
            refused(lambda: capi._check(L.sbwtgpu_unitigs_locate_dev(u._h, ptr, -1, ptr, ptr, None)), "negative")
            refused(lambda: capi._check(L.sbwtgpu_unitigs_locate_dev(u._h, None, 2, ptr, ptr, None)), "NULL")
            capi._check(L.sbwtgpu_unitigs_graph_stats(u._h, None, None))
        with idx.unitigs_dev() as u:                                             # the existing call's handle has neither
            refused(lambda: capi._check(L.sbwtgpu_unitigs_links_info(u._h, C.byref(n))), "SBWTGPU_UNITIGS_LINKS")
            refused(lambda: capi._check(L.sbwtgpu_unitigs_column_map_dev(u._h, C.byref(p), C.byref(q))), "SBWTGPU_UNITIGS_COLUMN_MAP")
        refused(lambda: capi._check(L.sbwtgpu_unitigs_links_info(None, C.byref(n))), "NULL")
        refused(lambda: capi._check(L.sbwtgpu_unitigs_graph_stats(None, None, None)), "NULL")
        refused(lambda: capi._check(L.sbwtgpu_unitigs_links_copy(None, ptr, ptr)), "NULL")
        refused(lambda: capi._check(L.sbwtgpu_unitigs_column_map_copy(None, ptr, ptr)), "NULL")
        refused(lambda: capi._check(L.sbwtgpu_unitigs_locate_batch(None, ptr, 1, ptr, ptr)), "NULL")
        # what the existing create calls refuse
        w = np.random.default_rng(1).integers(0, 2**64, size=4, dtype=np.uint64)
        ro = capi.Index.create(w, w, w, w, None, 256, 3)
        refused(ro.unitig_graph_dev, "only rank()")
        assert len(run_graph(s)["first"]) == len(s.unitigs()[2])                 # the object and the index are usable afterwards


def test_no_real_column_gives_no_links(gpu):
    for empty in (["ACG"], ["ACGTNACGT", "acgtacgtacgt"]):
        bits, idx = make_index(empty, 6)
        assert bits.n_kmers == 0
        with build_sets(idx, [empty]) as s:
            for owner in (idx, s):
                g = run_graph(owner)
                assert len(g["first"]) == 0 and g["link_off"].tolist() == [0] and len(g["link_to"]) == 0
                assert len(g["col_unitig"]) == idx.n_nodes and np.all(g["col_unitig"] == NONE) and np.all(g["col_offset"] == NONE)
        with idx.unitig_graph_dev(links=True, column_map=True) as u:
            lu, lr = u.locate(np.arange(idx.n_nodes, dtype=np.int64))
            assert np.all(lu == NONE) and np.all(lr == NONE)


# ---- 9. one moderate shape ------------------------------------------------------------------------------------------------------------------
def test_moderate_scale(gpu):
    """The 2 Mbp genome set with strains of tests/test_gpu_unitigs.py::test_moderate_scale, without the brute force: the rows
    of the matrix in numpy say which edges leave the last column of every unitig and where they go."""
    k = 31
    genomes = synth.coli3_like(700_000, 0.01)
    seqs = [g.tobytes() for g in genomes]
    bits = capi.build_bits_gpu(seqs, k, True, True)
    idx = index_of(bits, k)
    n = bits.n_nodes
    g = run_graph(idx)
    b, o, f, lo, lt = g["bases"], g["off"], g["first"], g["link_off"], g["link_to"]
    nu = len(f)
    res, out_off = check_located(idx, g, idx)                                 # the map by construction, every k-mer
    rows = [np.unpackbits(np.ascontiguousarray(c).view(np.uint8), bitorder="little")[:n] for c in bits.cols]
    marks = np.unpackbits(bits.ssup.view(np.uint8), bitorder="little")[:n].astype(bool)
    group_first = np.flatnonzero(marks)[np.cumsum(marks) - 1]                 # per column: the first column of its group
    real = np.zeros(n, dtype=bool)
    real[res] = True
    deg = rows[0].astype(np.int64) + rows[1] + rows[2] + rows[3]
    edges = int(deg[group_first[real]].sum())
    # the invariant
    assert len(lt) == lo[-1] == edges - (bits.n_kmers - nu) and len(lt) > 1000
    # the links from the rows: edge c out of the tail's group goes to column C[c] + rank_c, which is a first column
    tails = res[out_off[1:] - 1]
    gt = group_first[tails]
    Cc = 1 + np.concatenate([[0], np.cumsum([int(r.sum()) for r in rows])[:3]])
    src, tgt_col, chars = [], [], []
    for c in range(4):
        rank = np.cumsum(rows[c], dtype=np.int64) - rows[c]                   # ones before the column
        has = rows[c][gt] == 1
        src.append(np.flatnonzero(has))
        tgt_col.append(Cc[c] + rank[gt[has]])
        chars.append(np.full(int(has.sum()), c))
    src, tgt_col, chars = np.concatenate(src), np.concatenate(tgt_col), np.concatenate(chars)
    order = np.lexsort((chars, src))                                           # by source, then by character
    src, tgt_col = src[order], tgt_col[order]
    at = np.searchsorted(f, tgt_col)
    assert at.max() < nu and np.array_equal(f[at], tgt_col)                   # every target is a first column
    assert np.array_equal(lo, np.concatenate([[0], np.cumsum(np.bincount(src, minlength=nu))]))
    assert np.array_equal(lt, at.astype(np.uint32))
    # each (last k-mer, first k-mer) pair overlaps in k-1 bases
    for j in range(k - 1):
        assert np.array_equal(b[o[src + 1] - (k - 1) + j], b[o[lt] + j]), j
    # distinct ascending targets within a source
    same = src[1:] == src[:-1]
    assert np.all(lt[1:][same] > lt[:-1][same])
    # a coloured run on the same index: the breaks between the strains' stretches are links too
    refs = [[s] for s in seqs] + [[seqs[0][a:a + 700] for a in range(0, len(seqs[0]), 2000)]]
    with build_sets(idx, refs, True) as s:
        gc = run_graph(s)
        with s.unitigs_dev() as u:
            nb = u.color_info()["n_color_breaks"]
        check_located(idx, gc, s)
    assert nb > 1000 and len(gc["first"]) == nu + nb
    assert len(gc["link_to"]) == edges - (bits.n_kmers - len(gc["first"])) == len(lt) + nb
    srcc = np.repeat(np.arange(len(gc["first"])), np.diff(gc["link_off"]))
    for j in range(k - 1):
        assert np.array_equal(gc["bases"][gc["off"][srcc + 1] - (k - 1) + j], gc["bases"][gc["off"][gc["link_to"]] + j]), j


# ---- 10. the CLI ------------------------------------------------------------------------------------------------------------------------------
def run(cmd, timeout=300):
    return subprocess.run(cmd, capture_output=True, timeout=timeout)


def parse_gfa(data):
    lines = data.decode().split("\n")
    assert lines[-1] == "" and lines[0] == "H\tVN:Z:1.0"
    recs = [ln.split("\t") for ln in lines[1:-1]]
    n_seg = sum(1 for r in recs if r[0] == "S")
    assert all(r[0] == "S" for r in recs[:n_seg]) and all(r[0] == "L" for r in recs[n_seg:])       # links after all segments
    return recs[:n_seg], recs[n_seg:]


def test_cli_gfa(gpu, tmp_path):
    d = str(tmp_path)
    c = KATS["cli_end_to_end"]
    k, seqs, rc = c["k"], c["seqs"], c["add_reverse_complements"]
    with open(d + "/in.fna", "w") as fh:
        for i, s in enumerate(seqs):
            fh.write(">%d\n%s\n" % (i, s))
    p = run([SBWT, "build", "-i", d + "/in.fna", "-o", d + "/i.sbwt", "-k", str(k)] + (["--add-reverse-complements"] if rc else []))
    assert p.returncode == 0, p.stderr.decode()
    refs = pieces_as_references(seqs, 3, random.Random(14))
    with open(d + "/refs.txt", "w") as fh:
        for ci, mine in enumerate(refs):
            name = "%s/ref%d.fna" % (d, ci)
            with open(name, "w") as out:
                out.write("".join(">r%d_%d\n%s\n" % (ci, j, s) for j, s in enumerate(mine)))
            fh.write(name + "\n")
    p = run([SBWT, "build-colors", "-i", d + "/i.sbwt", "-r", d + "/refs.txt", "-o", d + "/c.colors", "--compress"] + (["--both-strands"] if rc else []))
    assert p.returncode == 0, p.stderr.decode()
    bits, idx = make_index(seqs, k, rc)
    B = BruteSBWT(text(seqs), k, rc)
    all_edges = {(x, x[1:] + ch) for x in B.kmers for ch in "ACGT" if x[1:] + ch in B.kmers}
    with build_sets(idx, refs, rc) as s:
        want_colored = run_graph(s)
    want_plain = run_graph(idx)
    for colored, want in ((False, want_plain), (True, want_colored)):
        extra = ["--colors", d + "/c.colors"] if colored else []
        # without --gfa: the FASTA file of today
        p = run([SBWT, "dump-unitigs", "-i", d + "/i.sbwt", "-o", d + "/u.fna"] + extra)
        assert p.returncode == 0, p.stderr.decode()
        U = split(want["bases"], want["off"])
        heads = [b"%d %d" % (i, z) for i, z in enumerate(want["set_id"])] if colored else [b"%d" % i for i in range(len(U))]
        fasta = open(d + "/u.fna", "rb").read()
        assert fasta == b"".join(b">%s\n%s\n" % (h, u) for h, u in zip(heads, U))
        for z in (False, True):
            out = d + "/u.gfa" + (".gz" if z else "")
            sets_out = ["--sets-out", d + "/sets.txt"] if colored else []
            p = run([SBWT, "dump-unitigs", "-i", d + "/i.sbwt", "-o", out, "--gfa"] + extra + sets_out + (["-z"] if z else []))
            assert p.returncode == 0, p.stderr.decode()
            assert b"%d links" % len(want["link_to"]) in p.stdout + p.stderr
            segs, links = parse_gfa(gzip.open(out).read() if z else open(out, "rb").read())
            # the segments are the FASTA records
            assert [r[1].encode() for r in segs] == [b"%d" % i for i in range(len(U))]
            assert [r[2].encode() for r in segs] == U
            if colored:
                assert [r[3] for r in segs] == ["cs:i:%d" % z_ for z_ in want["set_id"]] and all(len(r) == 4 for r in segs)
                assert open(d + "/sets.txt").read().startswith("0\n")
            else:
                assert all(len(r) == 3 for r in segs)
            # the links in link order
            src = np.repeat(np.arange(len(U)), np.diff(want["link_off"]))
            assert links == [["L", str(i), "+", str(j), "+", "%dM" % (k - 1)] for i, j in zip(src.tolist(), want["link_to"].tolist())]
            # within-segment pairs and the links' (last k-mer, first k-mer) pairs: the edge set, each edge once
            S = [r[2] for r in segs]
            got = [(u[r:r + k], u[r + 1:r + 1 + k]) for u in S for r in range(len(u) - k)]
            got += [(S[int(r[1])][-k:], S[int(r[3])][:k]) for r in links]
            assert len(got) == len(set(got)) and set(got) == all_edges
    assert len(want_colored["link_to"]) > len(want_plain["link_to"]) > 0
