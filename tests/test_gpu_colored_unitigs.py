"""GPU: coloured unitigs (sbwtgpu_unitigs_create_colored) byte for byte against the brute-force
restatement of their definition (tests/colored_unitig_brute.py), against numpy restatements where the brute force is too
slow, as a closed loop with search, build and ColorSets.from_arrays, and through the C++ CLI.  The helpers have the shapes of
those in tests/test_gpu_unitigs.py; colour-set objects come from ColorSetsBuilder unless a case says otherwise."""
import ctypes as C
import gzip
import json
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

import colorsets_brute as cb
from bruteforce import BruteSBWT
from colored_unitig_brute import brute_colored_unitigs, column_rows, row_of, sets_of_references
from unitig_brute import flatten
from sbwt_amd import capi, hostlib, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_kats.json")))


def as_bytes(seqs):
    return [s.encode() if isinstance(s, str) else s for s in seqs]


def index_of(bits, k):
    return capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)


def make_index(seqs, k, rc=False, ssup=True):
    bits = hostlib.build_bits(as_bytes(seqs), k, rc, ssup)
    return bits, index_of(bits, k)


def split(bases, off):
    b = bases.tobytes()
    return [b[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def circular(s, k):
    return s + s[:k - 1]


def build_sets(idx, refs, both=False, n_colors=None):
    """The canonical colour-set object of idx with colour c given the sequences refs[c]."""
    with capi.ColorSetsBuilder.create(idx, n_colors or max(1, len(refs))) as b:
        for c, seqs in enumerate(refs):
            b.add_reads(c, as_bytes(seqs), both)
        return b.finish()


def run_colored(s):
    """(bases, off, first_col, set_id, n_color_breaks, stats)"""
    with s.unitigs_dev() as u:
        b, o, f = u.copy()
        ci = u.color_info()
        assert (ci["n_sets"], ci["n_colors"]) == (s.n_sets, s.n_colors)
        assert u.n_unitigs == len(f) and u.total_bases == len(b) == o[-1]
        return b, o, f, u.set_ids(), ci["n_color_breaks"], u.stats()


def check_brute(idx, seqs, k, rc, refs, both, label):
    """ColorSets.unitigs() of the builder's object == the brute force, byte for byte; returns the API result."""
    B = BruteSBWT([s.decode() if isinstance(s, bytes) else s for s in seqs], k, rc)
    sets = sets_of_references(B.kmers, k, [[x.decode() if isinstance(x, bytes) else x for x in r] for r in refs], 2 if both else 1)
    U, Z, first, n_breaks = brute_colored_unitigs(B, sets)
    want_bases, want_off = flatten(U)
    want_ids = cb.canonical(column_rows(B, sets))[0]
    assert idx.n_nodes == len(B.nodes), label
    with build_sets(idx, refs, both) as s:
        b, o, f, sid, nb, _ = run_colored(s)
        ids, table = s.copy()
    assert o.tolist() == want_off, label
    assert b.tobytes() == want_bases, label
    assert f.tolist() == first, label
    assert sid.tolist() == [want_ids[c] for c in first], label
    assert [int.from_bytes(table[i].tobytes(), "little") for i in sid] == [row_of(z) for z in Z], label
    assert nb == n_breaks, label
    assert int((o[1:] - o[:-1] - (k - 1)).sum()) == len(B.kmers), label
    return b, o, f, sid, nb


def check_permutation(idx, n_kmers, bases, off, first_col):
    """streaming_search over the unitigs: no -1, unitig i starts at first_col[i], every real column exactly once."""
    res, out_off = idx.streaming_search(bases, off)
    assert len(res) == n_kmers
    if len(res):
        assert res.min() >= 0
        assert np.array_equal(res[out_off[:-1]], first_col)
        got = np.sort(res)
        assert np.all(got[1:] > got[:-1])
    return res, out_off


def check_round_trip(bits, bases, off, k):
    back = capi.build_bits_gpu(split(bases, off), k, False, True)
    assert (back.n_nodes, back.n_kmers) == (bits.n_nodes, bits.n_kmers)
    for c in range(4):
        assert np.array_equal(back.cols[c], bits.cols[c]), "ACGT"[c]
    assert np.array_equal(back.ssup, bits.ssup)


def same_as_plain(idx, got):
    want = idx.unitigs()
    for a, b in zip(want, got[:3]):
        assert a.dtype == b.dtype and np.array_equal(a, b)


# ---- 1. the worked examples and the reference inputs -------------------------------------------------------------------------
WORKED = [
    (["AACCG", "CCGGTT"], ["AACCG", "CCGGTT"], [(b"AACC", {0}), (b"CCG", {0, 1}), (b"CGGTT", {1})], 2),
    (["ACGTAC"], ["ACGTAC"], [(b"GTACGT", {0})], 0),
    (["ACGTAC"], ["ACGTAC", "CGTA"], [(b"TACG", {0}), (b"CGTA", {0, 1})], 2),
    (["ACGTAC"], ["ACGTAC", "GTAC"], [(b"GTAC", {0, 1}), (b"ACGT", {0})], 2),
    (["ACGTAC"], ["ACGTAC", "TACG"], [(b"TACG", {0, 1}), (b"CGTA", {0})], 2),
    (["ACGTAC", "GGG"], ["ACGTAC"], [(b"GTACGT", {0}), (b"GGG", set())], 0),
]


@pytest.mark.parametrize("case", range(len(WORKED)))
def test_worked_examples(gpu, case):
    seqs, refs, want, breaks = WORKED[case]
    _, idx = make_index(seqs, 3)
    b, o, f, sid, nb = check_brute(idx, seqs, 3, False, [[r] for r in refs], False, case)
    with build_sets(idx, [[r] for r in refs]) as s:
        table = s.copy()[1]
    got = [(u, {c for c in range(64) if (int(table[i, 0]) >> c) & 1}) for u, i in zip(split(b, o), sid)]
    assert got == want and nb == breaks


def pieces_as_references(seqs, n_refs, rng):
    """The sequences dealt out to n_refs references: whole, halves that overlap, and one shared by two."""
    refs = [[] for _ in range(n_refs)]
    for i, s in enumerate(seqs):
        refs[i % n_refs].append(s[: max(1, 2 * len(s) // 3)])
        refs[(i + 1) % n_refs].append(s[len(s) // 3:])
        if rng.random() < 0.3:
            refs[rng.randrange(n_refs)].append(s)
    return refs


def test_reference_inputs(gpu):
    rng = random.Random(1)
    cases = [("cli_end_to_end", KATS["cli_end_to_end"]["seqs"], KATS["cli_end_to_end"]["k"], KATS["cli_end_to_end"]["add_reverse_complements"]),
             ("redundant_dummies", KATS["redundant_dummies"]["seqs"], KATS["redundant_dummies"]["k"], False)]
    cases += [(c["name"], c["seqs"], c["k"], False) for c in KATS["small_cases"]["cases"] if c["k"] >= 2]
    for n_refs, (name, seqs, k, rc) in zip([2, 3, 4, 5] * len(cases), cases):
        bits, idx = make_index(seqs, k, rc)
        refs = pieces_as_references(seqs, n_refs, rng)
        b, o, f, sid, nb = check_brute(idx, seqs, k, rc, refs, rc, (name, n_refs))
        check_permutation(idx, bits.n_kmers, b, o, f)


# ---- 2. random sets ---------------------------------------------------------------------------------------------------------------
def random_seqs(rng, k):
    alphabet = "AC" if k <= 5 else "ACGT"
    seqs = ["".join(rng.choice(alphabet) for _ in range(rng.randint(1, 300))) for _ in range(rng.randint(1, 40))]
    seqs.append("".join(rng.choice(alphabet) for _ in range(max(1, k - 1))))          # shorter than k
    seqs += ["".join(rng.choice(alphabet) for _ in range(k)) for _ in range(3)]       # exactly k: dummy-heavy
    s = list("".join(rng.choice(alphabet) for _ in range(3 * k + 40)))
    s[len(s) // 3] = "N"
    s[2 * len(s) // 3] = s[2 * len(s) // 3].lower()
    seqs.append("".join(s))
    return seqs


def random_refs(rng, seqs, k):
    """1 to 6 references of overlapping random pieces and mutated copies; some k-mers end up in no reference."""
    alphabet = "AC" if k <= 5 else "ACGT"
    refs = []
    for _ in range(rng.randint(1, 6)):
        mine = []
        for _ in range(rng.randint(1, 12)):
            s = rng.choice(seqs)
            a = rng.randrange(len(s))
            piece = list(s[a:a + rng.randint(1, 200)])
            if rng.random() < 0.4 and piece:                                          # a mutated copy: the break falls inside
                piece[rng.randrange(len(piece))] = rng.choice(alphabet)
            mine.append("".join(piece))
        refs.append(mine)
    return refs


@pytest.mark.parametrize("k", [2, 3, 4, 5, 8, 16, 31, 32, 33, 63, 64])
@pytest.mark.parametrize("rc", [False, True])
def test_random_sets(gpu, k, rc):
    rng = random.Random(100 * k + rc)
    seqs = random_seqs(rng, k)
    refs = random_refs(rng, seqs, k)
    bits, idx = make_index(seqs, k, rc)
    b, o, f, sid, nb = check_brute(idx, seqs, k, rc, refs, rc, (k, rc))
    check_permutation(idx, bits.n_kmers, b, o, f)
    check_round_trip(bits, b, o, k)


# ---- 3. pure cycles ---------------------------------------------------------------------------------------------------------------
def de_bruijn(alphabet, n):
    """The de Bruijn sequence B(len(alphabet), n) (Lyndon words): every n-mer over the alphabet once, cyclically."""
    a, out, m = [0] * (len(alphabet) * n), [], len(alphabet)

    def db(t, p):
        if t > n:
            if n % p == 0:
                out.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, m):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return "".join(alphabet[i] for i in out)


def arcs_of(n_breaks):
    """The sets of the arcs round a cycle with n_breaks breaks (one break alone cannot be: the sets round a cycle are equal
    except across breaks); reference 0 holds the whole cycle."""
    return {0: [[0]], 2: [[0], [0, 1]], 3: [[0], [0, 1], [0, 2]], 7: [[0], [0, 1], [0], [0, 1], [0], [0, 1], [0, 2]]}[n_breaks]


@pytest.mark.parametrize("k", [5, 31])
def test_pure_cycles(gpu, k):
    rng = random.Random(k)
    cyc = de_bruijn("ACG", 4) if k == 5 else "".join(rng.choice("ACGT") for _ in range(150))    # 81 and 150 k-mers
    L = len(cyc)
    seq = circular(cyc, k)
    bits, idx = make_index([seq], k)
    pb_, po, pf = idx.unitigs()
    assert len(pf) == 1 and bits.n_kmers == L                                                   # a pure cycle
    plain = pb_.tobytes().decode()
    r = (cyc + cyc).index(plain[:k])                                                            # where the plain unitig is cut
    trip = cyc * 3
    for n_breaks in (0, 2, 3, 7):
        arcs = arcs_of(n_breaks)
        bounds = [(r - 5 + (L * i) // len(arcs)) % L for i in range(len(arcs))]                 # arc 0 runs across position r
        refs = [[seq], [], []]
        for i, arc in enumerate(arcs):
            a, z = bounds[i], bounds[(i + 1) % len(arcs)]
            n = (z - a) % L or L
            for c in arc:
                if c:
                    refs[c].append(trip[a:a + n + k - 1])
        b, o, f, sid, nb = check_brute(idx, [seq], k, False, refs, False, (k, n_breaks))
        assert nb == n_breaks and len(f) == max(1, n_breaks)
        check_permutation(idx, bits.n_kmers, b, o, f)
        check_round_trip(bits, b, o, k)
        if n_breaks == 0:
            assert b.tobytes().decode() == plain and f.tolist() == pf.tolist()
        else:
            assert any(u.decode() not in plain for u in split(b, o))                            # a piece crosses the old cut
    # a tail entering the cycle: the cycle is not pure; the tail's colour cuts it once more
    tail = "".join(rng.choice("T" if k == 5 else "ACGT") for _ in range(k + 4))
    seqs = [tail + seq]
    bits, idx = make_index(seqs, k)
    for refs in ([seqs], [seqs, [tail + seq[:k + 10]]], [[seq], [tail + seq[:12]], [trip[20:20 + k + 30]]]):
        b, o, f, sid, nb = check_brute(idx, seqs, k, False, refs, False, (k, "tail", len(refs)))
        check_permutation(idx, bits.n_kmers, b, o, f)


# ---- 4. no breaks means the plain call ---------------------------------------------------------------------------------------------
def test_no_breaks_is_the_plain_call(gpu):
    rng = random.Random(4)
    for k, rc in ((4, False), (21, True), (40, False)):
        seqs = random_seqs(rng, k) + [circular("".join(rng.choice("ACGT") for _ in range(k + 9)), k)]
        bits, idx = make_index(seqs, k, rc)
        with build_sets(idx, [seqs, seqs], rc) as s:           # every real column in the one set {0, 1}
            got = run_colored(s)
            ids = s.copy()[0]
            assert s.n_sets == 2 and int((ids != 0).sum()) == bits.n_kmers
        same_as_plain(idx, got)
        assert got[4] == 0 and np.all(got[3] == 1)
        with build_sets(idx, [], n_colors=3) as s:             # n_sets = 1: the empty set alone
            got = run_colored(s)
            assert s.n_sets == 1
        same_as_plain(idx, got)
        assert got[4] == 0 and np.all(got[3] == 0)


# ---- 5. and 6.: uploaded objects with duplicate rows; wide rows ------------------------------------------------------------------
def columns_along(idx, seq, k):
    res, _ = idx.streaming_search(np.frombuffer(seq, dtype=np.uint8), np.array([0, len(seq)], dtype=np.int64))
    assert res.min() >= 0 and len(np.unique(res)) == len(res)
    return res


def pieces_by_rows(seq, cols, rows_along, ids_along, k):
    """numpy restatement on one plain unitig: cut where the ROW along the sequence changes; (first_col, bases, id) sorted"""
    cut = np.nonzero(np.any(rows_along[1:] != rows_along[:-1], axis=1))[0] + 1
    lo = np.concatenate([[0], cut])
    hi = np.concatenate([cut, [len(cols)]])
    out = sorted((int(cols[a]), seq[a:z + k - 1], int(ids_along[a])) for a, z in zip(lo, hi))
    return out, len(cut)


def check_uploaded(idx, seq, k, n_colors, ids_along, table):
    cols = columns_along(idx, seq, k)
    ids = np.zeros(idx.n_nodes, dtype=np.uint32)
    ids[cols] = ids_along
    want, n_cut = pieces_by_rows(seq, cols, table[ids_along], ids_along, k)
    with capi.ColorSets.from_arrays(idx, n_colors, ids, table) as s:
        b, o, f, sid, nb, _ = run_colored(s)
    assert list(zip(f.tolist(), split(b, o), sid.tolist())) == want
    assert nb == n_cut
    return len(want)


def test_uploaded_object_with_duplicate_rows(gpu):
    k = 31
    seq = synth.random_genome(400, 21).tobytes()
    bits, idx = make_index([seq], k)
    assert len(idx.unitigs()[2]) == 1
    m = bits.n_kmers
    alt = (np.arange(m) % 2 + 1).astype(np.uint32)                                   # ids 1, 2, 1, 2, ... along the unitig
    assert check_uploaded(idx, seq, k, 5, alt, np.array([[0], [9], [9]], dtype=np.uint64)) == 1
    assert check_uploaded(idx, seq, k, 5, alt, np.array([[0], [9], [9], [6]], dtype=np.uint64)) == 1       # row 3 unused
    mixed = alt.copy()
    mixed[m // 2:] = 3                                                                # ... and a real break after them
    assert check_uploaded(idx, seq, k, 5, mixed, np.array([[0], [9], [9], [6]], dtype=np.uint64)) == 2


def test_wide_rows(gpu):
    k, n_colors, W = 31, 4096, 64
    seq = synth.random_genome(700, 22).tobytes()
    bits, idx = make_index([seq], k)
    m = bits.n_kmers
    table = np.zeros((6, W), dtype=np.uint64)
    table[1:, 5] = 1 << 17                                    # rows 1 .. 5 share a bit in the middle
    table[2, 63] = 1 << 63                                    # 1 | 2 differ in word 63 only (colour 4095)
    table[3, 63] = 1 << 63
    table[3, 0] = 1                                           # 2 | 3 differ in word 0 only
    table[4] = table[3]                                       # 3 == 4: a duplicate pair, no break
    table[5, 0] = 1                                           # 5 differs from 3 in word 63 only, from 1 in word 0 only
    ids_along = np.repeat(np.array([1, 2, 3, 4, 3, 4, 5, 1], dtype=np.uint32), (m + 7) // 8)[:m]
    assert check_uploaded(idx, seq, k, n_colors, ids_along, table) == 5              # 1 | 2 | 3 4 3 4 | 5 | 1


# ---- 7. a long unitig in many pieces -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_index(gpu):
    k = 31
    g = synth.random_genome(300_000, 11)
    bits = capi.build_bits_gpu([g.tobytes()], k, False, True)
    return k, g, bits, index_of(bits, k)


def test_long_unitig_many_pieces(long_index):
    k, g, bits, idx = long_index
    seq = g.tobytes()
    refs = [[seq[a:a + 1000] for a in range(c * 1000, len(seq), 2000)] for c in (0, 1)]
    with idx.unitigs_dev() as u:
        assert u.n_unitigs == 1
        plain_rounds = u.stats()["jump_rounds"]
    cols = columns_along(idx, seq, k)
    with build_sets(idx, refs) as s:
        ids, table = s.copy()
        b, o, f, sid, nb, stats = run_colored(s)
    ids_along = ids[cols]
    want, n_cut = pieces_by_rows(seq, cols, table[ids_along], ids_along, k)
    assert n_cut == 2 * 299 and nb == n_cut                  # 300 stretches, and 30 uncoloured k-mers across every boundary
    assert f.tolist() == [w[0] for w in want] and sid.tolist() == [w[2] for w in want]
    assert split(b, o) == [w[1] for w in want]
    assert stats["jump_rounds"] <= int(np.ceil(np.log2(idx.n_nodes))) + 2
    assert stats["jump_rounds"] < plain_rounds, (stats["jump_rounds"], plain_rounds)


# ---- 8. the closed loop ---------------------------------------------------------------------------------------------------------------
def test_closed_loop(gpu):
    rng = random.Random(8)
    k = 21
    seqs = random_seqs(rng, k) + [circular("".join(rng.choice("ACGT") for _ in range(k + 30)), k)]
    refs = random_refs(rng, seqs, k)
    bits, idx = make_index(seqs, k, True)
    with build_sets(idx, refs, True) as s:
        ids, table = s.copy()
        b, o, f, sid, nb, _ = run_colored(s)
        res, out_off = check_permutation(idx, bits.n_kmers, b, o, f)
        scattered = np.zeros(idx.n_nodes, dtype=np.uint32)
        scattered[res] = np.repeat(sid, np.diff(out_off))
        assert np.array_equal(scattered, ids)                 # (dummies: 0 on both sides)
        check_round_trip(bits, b, o, k)
        with capi.ColorSets.from_arrays(idx, s.n_colors, scattered, table) as t, s.expand() as es, t.expand() as et:
            assert np.array_equal(es.rows(), et.rows())


# ---- 9. layouts -----------------------------------------------------------------------------------------------------------------------
def test_image_layouts_and_marks(gpu):
    rng = random.Random(77)
    k = 15
    seqs = ["".join(rng.choice("ACGT") for _ in range(rng.randint(20, 300))) for _ in range(12)]
    seqs += [s[:80] + rng.choice("ACGT") + s[81:160] for s in seqs[:6]]               # branches
    seqs.append(circular("".join(rng.choice("ACGT") for _ in range(k + 9)), k))
    refs = random_refs(rng, seqs, k)
    bits, idx = make_index(seqs, k, True)
    assert 2000 <= idx.n_nodes <= 20000
    want = check_brute(idx, seqs, k, True, refs, True, "layouts")
    assert want[4] > 0
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
        with capi.ColorSets.from_arrays(other, n_colors, ids, table) as s:
            got = run_colored(s)
        for a, b in zip(want, got[:5]):
            assert np.array_equal(a, b), name


def test_mega_block_layout(gpu, tmp_path):
    """The MEGA instantiation of the coloured lengths kernel, through the test build with mega blocks of 2^12 columns (a fresh
    child loads it; tests/colored_unitig_mega_worker.py): the bytes the product build gives."""
    lib = os.path.join(ROOT, "sbwt_amd", "lib", "libsbwtgpu_mega12.so")
    assert os.path.exists(lib), "%s is missing: build it with `python -m sbwt_amd.build`" % lib
    k = 31
    g0 = synth.random_genome(40_000, 5)
    g1 = synth.mutate(g0, 0.03, 6)
    seqs = [g0.tobytes(), g1.tobytes()]
    bits = hostlib.build_bits(seqs, k, True, True)
    assert (bits.n_nodes >> 12) >= 30
    idx = index_of(bits, k)
    # (the two strains differ at branches, which cut anyway; the pieces of the third colour end inside unitigs, all over the columns)
    with build_sets(idx, [[seqs[0]], [seqs[1]], [seqs[0][a:a + 400] for a in range(0, 40_000, 1000)]], True) as s:
        ids, table = s.copy()
        want = run_colored(s)
    assert want[4] > 50
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, A=bits.cols[0], C=bits.cols[1], G=bits.cols[2], T=bits.cols[3], ssup=bits.ssup, ids=ids, table=table,
             meta=np.array([bits.n_nodes, k, bits.n_kmers, 3], dtype=np.int64))
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tests", "colored_unitig_mega_worker.py"), fin, fout],
                       env=dict(os.environ, SBWTGPU_LIB=lib), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-4000:]
    out = np.load(fout, allow_pickle=False)
    assert "mega_shift=12" in str(out["version"])
    for image in ("rel1", "rel0", "big1", "big0"):
        for a, key in zip(want, ("bases", "off", "first", "set_id")):
            assert np.array_equal(a, out["%s/%s" % (image, key)]), (image, key)
        assert int(out["%s/breaks" % image]) == want[4]


# ---- 10. moderate scale ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def moderate(gpu):
    """The 2 Mbp genome set with strains of tests/test_gpu_unitigs.py::test_moderate_scale: its index, the plain unitigs and
    the columns along them (pred of res[i] is res[i - 1] inside a unitig), shared by the two cases below."""
    k = 31
    genomes = synth.coli3_like(700_000, 0.01)
    seqs = [g.tobytes() for g in genomes]
    bits = capi.build_bits_gpu(seqs, k, True, True)
    idx = index_of(bits, k)
    pb_, po, pf = idx.unitigs()
    res, out_off = idx.streaming_search(pb_, po)
    return k, seqs, bits, idx, pf, res, out_off


# the strains as colours; and the strains plus a fourth colour in stretches of 700 of every 2000 bases of strain 0.  Whole
# strains change colour only where a bubble branches, so the first case has no break inside a plain unitig: the second has
@pytest.mark.parametrize("stretches", [False, True])
def test_moderate_scale(moderate, stretches):
    k, seqs, bits, idx, pf, res, out_off = moderate
    refs = [[s] for s in seqs] + ([[seqs[0][a:a + 700] for a in range(0, len(seqs[0]), 2000)]] if stretches else [])
    with build_sets(idx, refs, True) as s:
        ids, table = s.copy()
        assert len(np.unique(table, axis=0)) == len(table)    # canonical: equal sets have equal ids
        b, o, f, sid, nb, stats = run_colored(s)
    # the starts with numpy: a plain start (three random genomes hold no pure cycle), or ids[pred[v]] != ids[v]
    is_first = np.zeros(len(res), dtype=bool)
    is_first[out_off[:-1]] = True
    changed = np.zeros(len(res), dtype=bool)
    changed[1:] = ids[res[1:]] != ids[res[:-1]]
    start = is_first | changed
    want_first = np.sort(res[start])
    n_breaks = int((changed & ~is_first).sum())
    assert (n_breaks > 1000) if stretches else (n_breaks == 0)
    assert nb == n_breaks and len(f) == len(pf) + n_breaks
    assert np.array_equal(f, want_first)
    assert len(b) == o[-1] == bits.n_kmers + len(f) * (k - 1)
    assert stats["jump_rounds"] <= int(np.ceil(np.log2(idx.n_nodes))) + 2
    # every unitig is monochromatic: search, gather the ids, compare with the unitig's
    res2, out_off2 = check_permutation(idx, bits.n_kmers, b, o, f)
    assert np.array_equal(ids[res2], np.repeat(sid, np.diff(out_off2)))
    assert len(set(sid.tolist())) > 3


# ---- 11. determinism and bounds ---------------------------------------------------------------------------------------------------------
def test_determinism_and_bounds(gpu):
    rng = random.Random(5)
    k = 21
    seqs = random_seqs(rng, k)
    refs = random_refs(rng, seqs, k)
    bits, idx = make_index(seqs, k, True)
    with build_sets(idx, refs, True) as s:
        r1, r2 = run_colored(s), run_colored(s)
        for a, b in zip(r1[:5], r2[:5]):
            assert np.array_equal(a, b)
        b1, o1, f1, sid1 = r1[:4]
        assert int((o1[1:] - o1[:-1] - (k - 1)).sum()) == bits.n_kmers and o1[-1] == len(b1)
        with s.unitigs_dev() as u:
            n, total = u.n_unitigs, u.total_bases
            G = 64
            hb = np.full(total + 2 * G, 0xA5, dtype=np.uint8)
            ho = np.full(n + 1 + 2 * G, -7, dtype=np.int64)
            hf = np.full(n + 2 * G, -7, dtype=np.int64)
            hs = np.full(n + 2 * G, 0xA5A5A5A5, dtype=np.uint32)
            capi._check(capi.lib().sbwtgpu_unitigs_copy(u._h, hb[G:].ctypes.data, ho[G:].ctypes.data, hf[G:].ctypes.data))
            capi._check(capi.lib().sbwtgpu_unitigs_set_ids_copy(u._h, hs[G:].ctypes.data))
            for arr, m, fill in ((hb, total, 0xA5), (ho, n + 1, -7), (hf, n, -7), (hs, n, 0xA5A5A5A5)):
                assert np.all(arr[:G] == fill) and np.all(arr[G + m:] == fill)
            assert np.array_equal(hb[G:G + total], b1) and np.array_equal(ho[G:G + n + 1], o1)
            assert np.array_equal(hf[G:G + n], f1) and np.array_equal(hs[G:G + n], sid1)
            # the device pointer holds the same ids
            back = np.zeros(n, dtype=np.uint32)
            hip = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))      # the runtime the library loaded
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            assert hip.hipMemcpy(back.ctypes.data, u.set_ids_dev(), n * 4, 2) == 0          # (2: device to host)
            assert np.array_equal(back, sid1)


# ---- 12. two host threads -----------------------------------------------------------------------------------------------------------------
def test_two_host_threads(gpu):
    rng = random.Random(12)
    k = 17
    seqs = random_seqs(rng, k)
    bits, idx = make_index(seqs, k, True)
    with build_sets(idx, random_refs(rng, seqs, k), True) as s:
        want = run_colored(s)
        got, errors = [None, None], []

        def work(i):
            try:
                for _ in range(3):
                    got[i] = run_colored(s)
            except Exception as e:                # noqa: BLE001
                errors.append(e)
        threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for g in got:
            for a, b in zip(want[:5], g[:5]):
                assert np.array_equal(a, b)


# ---- 13. refusals and empties ---------------------------------------------------------------------------------------------------------
def refused(call, *words):
    with pytest.raises(capi.SbwtGpuError) as e:
        call()
    assert e.value.code == capi.ERR_INVALID_ARG, e.value
    for w in words:
        assert w in e.value.msg, e.value.msg


def test_refusals_and_empties(gpu):
    L = capi.lib()
    seqs = ["ACGTTGCATGCCGTAAGCTTAGGCATCGA", "TTTTGGGGCCCCAAAA"]
    bits, idx = make_index(seqs, 6)
    h = C.c_void_p()
    with build_sets(idx, [[seqs[0]]]) as s:
        refused(lambda: capi._check(L.sbwtgpu_unitigs_create_colored(None, C.byref(h))), "NULL")
        refused(lambda: capi._check(L.sbwtgpu_unitigs_create_colored(s.handle, None)), "NULL")
        with s.unitigs_dev() as u:
            refused(lambda: capi._check(L.sbwtgpu_unitigs_set_ids_dev(u._h, None)), "NULL")
            if u.n_unitigs:
                refused(lambda: capi._check(L.sbwtgpu_unitigs_set_ids_copy(u._h, None)), "NULL")
            capi._check(L.sbwtgpu_unitigs_color_info(u._h, None, None, None))
        nb, ns, nc = C.c_int64(), C.c_int64(), C.c_int32()
        p = C.c_void_p()
        refused(lambda: capi._check(L.sbwtgpu_unitigs_set_ids_dev(None, C.byref(p))), "NULL")
        refused(lambda: capi._check(L.sbwtgpu_unitigs_set_ids_copy(None, None)), "NULL")
        refused(lambda: capi._check(L.sbwtgpu_unitigs_color_info(None, C.byref(nb), C.byref(ns), C.byref(nc))), "NULL")
        # the three new calls on a plain handle
        with idx.unitigs_dev() as u:
            refused(u.set_ids, "sbwtgpu_unitigs_create_colored")
            refused(u.set_ids_dev, "sbwtgpu_unitigs_create_colored")
            refused(u.color_info, "sbwtgpu_unitigs_create_colored")
        assert len(s.unitigs()) == 4                           # the object and the index are usable afterwards
    # an index with no real column
    for empty in (["ACG"], ["ACGTNACGT", "acgtacgtacgt"]):
        b0, i0 = make_index(empty, 6)
        assert b0.n_kmers == 0
        with build_sets(i0, [empty]) as s:
            b, o, f, sid, nbk, _ = run_colored(s)
        assert len(b) == 0 and o.tolist() == [0] and len(f) == 0 and len(sid) == 0 and nbk == 0
    # every real column uncoloured: the plain call, every set id 0
    with build_sets(idx, [["GGGGGGGGGG"], []]) as s:
        got = run_colored(s)
        assert s.n_sets == 1
    same_as_plain(idx, got)
    assert got[4] == 0 and len(got[3]) > 0 and np.all(got[3] == 0)


# ---- 14. the CLI ------------------------------------------------------------------------------------------------------------------------
def run(cmd, timeout=300):
    return subprocess.run(cmd, capture_output=True, timeout=timeout)


def test_cli_dump_unitigs_colors(gpu, tmp_path):
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
    both = ["--both-strands"] if rc else []
    for name, extra, magic in (("col1", [], b"SBWTCOL1"), ("col2", ["--wide"], b"SBWTCOL2"), ("col3", ["--compress"], b"SBWTCOL3")):
        p = run([SBWT, "build-colors", "-i", d + "/i.sbwt", "-r", d + "/refs.txt", "-o", "%s/%s.colors" % (d, name)] + extra + both)
        assert p.returncode == 0, p.stderr.decode()
        assert open("%s/%s.colors" % (d, name), "rb").read(8) == magic
    _, idx = make_index(seqs, k, rc)
    with build_sets(idx, refs, rc) as s:
        b, o, f, sid, nb, _ = run_colored(s)
        table = s.copy()[1]
    assert nb > 0 and len(set(sid.tolist())) > 1
    want = b"".join(b">%d %d\n%s\n" % (i, z, u) for i, (u, z) in enumerate(zip(split(b, o), sid.tolist())))
    want_sets = "".join(" ".join([str(i)] + [str(cc) for cc in range(64) if (int(table[i, 0]) >> cc) & 1]) + "\n"
                        for i in range(len(table))).encode()
    assert want_sets.startswith(b"0\n")
    for name in ("col1", "col2", "col3"):
        p = run([SBWT, "dump-unitigs", "-i", d + "/i.sbwt", "-o", d + "/u.fna", "--colors", "%s/%s.colors" % (d, name),
                 "--sets-out", d + "/sets.txt"])
        assert p.returncode == 0, p.stderr.decode()
        assert open(d + "/u.fna", "rb").read() == want, name
        assert open(d + "/sets.txt", "rb").read() == want_sets, name
        log = (p.stdout + p.stderr).decode()
        assert "%d colour breaks" % nb in log and "%d colour sets" % len(table) in log, log
    p = run([SBWT, "dump-unitigs", "-i", d + "/i.sbwt", "-o", d + "/u.fna.gz", "-z", "--colors", d + "/col3.colors"])
    assert p.returncode == 0, p.stderr.decode()
    assert gzip.open(d + "/u.fna.gz").read() == want
    # without --colors: what it wrote before, the API's plain result
    pbases, poff, _ = idx.unitigs()
    p = run([SBWT, "dump-unitigs", "-i", d + "/i.sbwt", "-o", d + "/p.fna"])
    assert p.returncode == 0, p.stderr.decode()
    assert open(d + "/p.fna", "rb").read() == b"".join(b">%d\n%s\n" % (i, u) for i, u in enumerate(split(pbases, poff)))
    # the error exits: a colour file of another index, --sets-out without --colors, a file that is no colour file
    with open(d + "/other.fna", "w") as fh:
        fh.write(">0\n%s\n" % synth.random_genome(200, 3).tobytes().decode())
    p = run([SBWT, "build", "-i", d + "/other.fna", "-o", d + "/other.sbwt", "-k", str(k)])
    assert p.returncode == 0, p.stderr.decode()
    p = run([SBWT, "dump-unitigs", "-i", d + "/other.sbwt", "-o", d + "/x.fna", "--colors", d + "/col3.colors"])
    assert p.returncode != 0 and b"columns" in p.stderr
    p = run([SBWT, "dump-unitigs", "-i", d + "/i.sbwt", "-o", d + "/x.fna", "--sets-out", d + "/s.txt"])
    assert p.returncode != 0 and b"--sets-out" in p.stderr and b"--colors" in p.stderr
    p = run([SBWT, "dump-unitigs", "-i", d + "/i.sbwt", "-o", d + "/x.fna", "--colors", d + "/in.fna"])
    assert p.returncode != 0 and p.stderr
