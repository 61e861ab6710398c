"""GPU: sbwtgpu_colorsets_merge (sbwt_colormerge.hip: the colour sets of one or two coloured indexes carried onto another
index) against the colour-set builder on the target index, whose bytes the coloured union must give, and against the
definition (tests/colorsets_merge_brute.py): every kind of target, canonical form under colliding pairs, the shifted OR at
every word boundary, more than a thousand sets, launch edges, the queries of the result, every refusal, two host threads, the
C++ CLI and a bounded seeded fuzz.  All comparisons are exact.  (The refusal of indexes on different devices runs where
there are two devices.)"""
import random
import threading

import numpy as np
import pytest

import colorsets_brute as cb
import colorsets_merge_brute as mb
import pseudoalign_brute as pb
import pseudoalign_wide as pw
import test_gpu_pseudoalign_wide as tw          # its helpers: make_index, labels_of, refused, run, QUERIES
from bruteforce import kmer_set
from sbwt_amd import capi, hostlib

pytestmark = pytest.mark.gpu

QUERIES = tw.QUERIES
refused = tw.refused
OPS = ("union", "intersection", "difference", "symmetric-difference")


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def index_of(bits):
    return capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, bits.k, bits.n_kmers, 0)


def setop_index(ia, ib, op="union"):
    return index_of(ia.setop(ib, op)[0])


def built(idx, n_colors, adds):
    """The builder's ColorSets of idx: adds = (colour, sequences, both strands)"""
    with capi.ColorSetsBuilder.create(idx, n_colors) as b:
        for c, seqs, both in adds:
            b.add_reads(c, [s.encode() for s in seqs], both)
        return b.finish()


def colouring(idx, sets):
    """(labels, k-mer -> integer row, k-mer -> id) of a colour-set object of idx"""
    labels = tw.labels_of(idx)
    ids, table = sets.copy()
    return labels, mb.colouring_of(labels, ids.tolist(), pw.rows_ints(table)), mb.ids_of(labels, ids.tolist())


def check_against_brute(u, sa, sb, offset, label, labels_u=None):
    """merge(u, sa, sb, offset) == the definition: ids, table, n_colors, n_sets and the info counts"""
    labels_u = labels_u or tw.labels_of(u)
    dummy = ["$" in lab for lab in labels_u]
    _, col_a, ids_a = colouring(sa.index, sa)
    col_b = ids_b = None
    if sb is not None:
        _, col_b, ids_b = colouring(sb.index, sb)
    real_offset = offset if offset is not None else (sa.n_colors if sb is not None else 0)
    n_out = mb.n_colors_out(sa.n_colors, sb.n_colors if sb is not None else None, real_offset)
    want = mb.merge_arrays(labels_u, dummy, col_a, col_b, real_offset, n_out)
    with capi.ColorSets.merge(u, sa, sb, offset) as m:
        got = m.copy()
        assert same(got, want), (label, got[0].tolist()[:40], want[0].tolist()[:40])
        info = m.info()
        assert (info["n_columns"], info["k"], info["n_colors"], info["words"], info["n_sets"]) == \
            (u.n_nodes, u.k, n_out, pw.n_words(n_out), len(want[1])), label
        assert info["n_colored_columns"] == int((want[0] != 0).sum()), label
        counts = dict(mb.counts(labels_u, dummy, ids_a, ids_b), n_sets=len(want[1]))
        assert {f: m.merge_info[f] for f in counts} == counts, (label, m.merge_info)
        assert len(m.merge_info["pass_ms"]) == 4 and all(x >= 0 for x in m.merge_info["pass_ms"].values()), label
        cb.check_invariants(got[0].tolist(), pw.rows_ints(got[1]), n_out, dummy)
        return got, dict(m.merge_info)


def references(rng, k, n, alphabet="ACGT"):
    return [pw.rand_seq(rng, rng.randint(k + 2, 2 * k + 60), alphabet) for _ in range(n)]


def spread(n_colors, n_refs):
    """n_refs colours of n_colors, the first and the last among them"""
    if n_colors <= n_refs:
        return list(range(n_colors))
    return sorted({0, n_colors - 1} | {(i * n_colors) // n_refs for i in range(1, n_refs - 1)})


# ---- 1. the identity the feature exists for ------------------------------------------------------------------------------
COLOUR_COUNTS = ((1, 1), (63, 2), (64, 64), (65, 3), (100, 100), (4032, 64))


@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
@pytest.mark.parametrize("k", [2, 3, 31, 32, 33, 64])
def test_the_coloured_union_is_what_the_builder_gives_on_the_union(gpu, k, rc):
    rng = random.Random(100 * k + rc)
    alphabet = "AC" if k <= 3 else "ACGT"
    pool = references(rng, k, 9, alphabet)
    R1, R2 = pool[:6], pool[3:]                                 # three references on both sides
    R2 = R2 + [R1[0][1:k + 8]]                                  # ... and a piece of another
    a, b = tw.make_index(R1, k, rc), tw.make_index(R2, k, rc, ssup=False)
    u = setop_index(a, b)
    assert u.n_kmers == len(kmer_set(R1 + R2 + ([pb.revcomp(s) for s in R1 + R2] if rc else []), k))
    for n_a, n_b in COLOUR_COUNTS:
        ca, cbb = spread(n_a, len(R1)), spread(n_b, len(R2))
        # with fewer colours than references, the references share the colours round-robin
        adds_a = [(ca[i % len(ca)], [s], rc) for i, s in enumerate(R1)]
        adds_b = [(cbb[i % len(cbb)], [s], rc) for i, s in enumerate(R2)]
        # (a colour's sequences come in consecutive calls)
        adds_a.sort(key=lambda t: t[0])
        adds_b.sort(key=lambda t: t[0])
        with built(a, n_a, adds_a) as sa, built(b, n_b, adds_b) as sb:
            direct = adds_a + [(n_a + c, seqs, both) for c, seqs, both in adds_b]
            with built(u, n_a + n_b, direct) as want, capi.ColorSets.merge(u, sa, sb) as got:
                assert same(got.copy(), want.copy()), (k, rc, n_a, n_b)
                assert got.info() == want.info(), (k, rc, n_a, n_b)
                mi = got.merge_info
                assert (mi["n_real_u"], mi["n_from_a"], mi["n_from_b"], mi["n_sets"]) == (u.n_kmers, a.n_kmers, b.n_kmers, want.n_sets)
                assert mi["n_from_both"] == a.n_kmers + b.n_kmers - u.n_kmers
    for x in (a, b, u):
        x.close()


def test_both_strand_adds_on_forward_indexes_against_the_definition(gpu):
    # (the builder on the union would also colour k-mers that only the other side brought: the brute force is the reference here)
    k = 9
    rng = random.Random(77)
    R1, R2 = references(rng, k, 4), references(rng, k, 4)
    R2.append(pb.revcomp(R1[0]))                                # b holds reverse complements of a's k-mers
    a, b = tw.make_index(R1, k), tw.make_index(R2, k)
    u = setop_index(a, b)
    with built(a, 3, [(0, R1[:2], True), (2, R1[2:], True)]) as sa, built(b, 70, [(1, R2[:3], True), (69, R2[3:], True)]) as sb:
        check_against_brute(u, sa, sb, None, "both strands, forward indexes")
    for x in (a, b, u):
        x.close()


# ---- 2. every kind of u -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair(gpu):
    """two overlapping coloured indexes at k = 7: a with 3 colours, b with 70"""
    k = 7
    rng = random.Random(21)
    pool = references(rng, k, 10)
    R1, R2 = pool[:7], pool[4:]
    a, b = tw.make_index(R1, k), tw.make_index(R2, k)
    sa = built(a, 3, [(0, R1[:3], False), (1, R1[2:5], False), (2, R1[5:], False)])
    sb = built(b, 70, [(0, R2[:2], False), (64, R2[1:4], False), (69, R2[3:], False)])
    world = {"k": k, "R1": R1, "R2": R2, "a": a, "b": b, "sa": sa, "sb": sb}
    yield world
    for x in (sa, sb, a, b):
        x.close()


def test_every_kind_of_u(pair):
    a, b, sa, sb, k = pair["a"], pair["b"], pair["sa"], pair["sb"], pair["k"]
    for op in OPS:
        u = setop_index(a, b, op)
        assert u.n_kmers > 0, op
        got, info = check_against_brute(u, sa, sb, None, op)
        if op == "intersection":
            assert info["n_from_a"] == info["n_from_b"] == info["n_from_both"] == info["n_real_u"]
        if op == "difference":
            assert info["n_from_b"] == 0 and info["n_from_a"] == info["n_real_u"]
        assert np.array(["$" in lab for lab in tw.labels_of(u)]).sum() > 1 and got[0][0] == 0          # u has dummy columns
        check_against_brute(u, sa, sb, 0, (op, "shared colour space"))
        check_against_brute(u, sb, sa, 5, (op, "swapped, offset 5"))
        u.close()
    # a itself: the same object again; b itself; sb absent
    got, _ = check_against_brute(a, sa, None, None, "a itself")
    assert same(got, sa.copy())
    check_against_brute(a, sa, sb, None, "u is a")
    check_against_brute(b, sa, sb, None, "u is b")
    u = setop_index(a, b)
    check_against_brute(u, sa, None, None, "sb NULL")
    check_against_brute(u, sb, None, 0, "sb NULL, offset 0 given")
    # sa and sb the same object: every set beside a copy of itself 3 colours up; and OR-ed with itself
    check_against_brute(u, sa, sa, None, "the same object twice")
    got, info = check_against_brute(a, sa, sa, 0, "the same object twice, offset 0")
    assert same(got, sa.copy()) and info["n_pairs"] == sa.n_sets - 1
    u.close()
    # an index sharing no k-mer, and the root-only empty index
    other = tw.make_index(["G" * 30, "T" * 11], k)
    assert not kmer_set(["G" * 30, "T" * 11], k) & (kmer_set(pair["R1"], k) | kmer_set(pair["R2"], k))
    empty = tw.make_index(["ACG"], k)
    assert empty.n_nodes == 1
    for u, label in ((other, "unrelated"), (empty, "root only")):
        got, info = check_against_brute(u, sa, sb, None, label)
        assert not got[0].any() and got[1].shape == (1, 2) and info["n_sets"] == 1 and info["n_pairs"] == 0
        # ... and as an input: an object of it colours nothing
        with built(u, 2, []) as nothing:
            got, _ = check_against_brute(a, nothing, sa, None, (label, "as a"))
            check_against_brute(a, sa, nothing, None, (label, "as b"))
        u.close()


# ---- 3. canonical form under collisions -------------------------------------------------------------------------------
def test_colliding_pairs_and_non_canonical_inputs(gpu):
    k = 11
    rng = random.Random(3)
    idx = tw.make_index([pw.rand_seq(rng, 60) for _ in range(3)], k)
    labels = tw.labels_of(idx)
    real = [j for j, lab in enumerate(labels) if "$" not in lab]
    assert len(real) >= 100
    # uploaded objects with a duplicated row (1 and 3 of a) and an unused row (4), two colours, one colour space
    table_a = pw.rows_array([0, 0b01, 0b10, 0b01, 0b11], 1)
    table_b = pw.rows_array([0, 0b01, 0b10, 0b11, 0b10], 1)
    ids_a, ids_b = np.zeros(idx.n_nodes, dtype=np.uint32), np.zeros(idx.n_nodes, dtype=np.uint32)
    for r, j in enumerate(real):
        ids_a[j] = (r % 4)                         # 0 .. 3: some columns uncoloured in a
        ids_b[j] = ((r // 4) % 5)                  # 0 .. 4: row 4 is in use in b
    with capi.ColorSets.from_arrays(idx, 2, ids_a, table_a) as sa, capi.ColorSets.from_arrays(idx, 2, ids_b, table_b) as sb:
        got, info = check_against_brute(idx, sa, sb, 0, "collisions")
        # 19 pairs other than (0, 0) give the three rows 01, 10, 11
        assert info["n_pairs"] == 19 and info["n_sets"] == 4 and info["n_pairs"] > info["n_sets"] - 1
        rows = [int(table_a[ids_a[j], 0] | table_b[ids_b[j], 0]) for j in range(idx.n_nodes)]
        assert same(got, cb.arrays(*cb.canonical(rows), 2))
        # a non-canonical object merged onto its own index alone is re-canonicalised
        got, info = check_against_brute(idx, sa, None, None, "re-canonicalise")
        assert info["n_pairs"] == 3 and info["n_sets"] == 3
        check_against_brute(idx, sa, sb, 2, "non-canonical inputs, concatenated")
    idx.close()


# ---- 4. shifts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_b", [37, 64])
def test_shifts(gpu, n_b):
    k = 6
    b = tw.make_index(["ACGTTGCATG"], k)
    labels = tw.labels_of(b)
    real = [j for j, lab in enumerate(labels) if "$" not in lab]
    assert len(real) >= 3
    ids = np.zeros(b.n_nodes, dtype=np.uint32)
    ids[real[:3]] = (1, 2, 3)
    bits = (1, 1 << (n_b - 1), 1 << (n_b // 2))
    a = tw.make_index(["ACGTTGCATG"[:8]], k)
    with capi.ColorSets.from_arrays(b, n_b, ids, pw.rows_array((0,) + bits, pw.n_words(n_b))) as sb, built(a, 1, [(0, ["ACGTTGCA"], False)]) as sa:
        for offset in (0, 1, 63, 64, 65, 4032, 4096 - n_b):
            got, _ = check_against_brute(b, sa, sb, offset, (n_b, offset), labels)
            rows = pw.rows_ints(got[1][got[0]])
            for j, bit in zip(real[:3], bits):
                assert rows[j] & ~1 == (bit << offset) & ~1 and rows[j] >> offset & bit, (n_b, offset, j)
        refused(lambda: capi.ColorSets.merge(b, sa, sb, 4097 - n_b), "4097", "4096")
    a.close()
    b.close()


# ---- 5. many sets ---------------------------------------------------------------------------------------------------------
def test_many_sets(gpu):
    k = 15
    rng = random.Random(12)
    idx = tw.make_index([pw.rand_seq(rng, 5500)], k)
    assert 3000 <= idx.n_nodes <= 6000
    labels = tw.labels_of(idx)
    real = np.array(["$" not in lab for lab in labels])
    nrng = np.random.default_rng(12)
    objs = []
    for _ in range(2):
        m = nrng.integers(0, 1 << 12, size=(idx.n_nodes, 1), dtype=np.uint64)
        m[~real] = 0
        objs.append(capi.ColorSets.from_arrays(idx, 12, *cb.canonical_arrays(m)))
    got, info = check_against_brute(idx, objs[0], objs[1], None, "many sets", labels)
    assert info["n_pairs"] > 1024 and info["n_sets"] - 1 > 1024
    got, info = check_against_brute(idx, objs[0], objs[1], 0, "many sets, one colour space", labels)
    assert info["n_pairs"] > info["n_sets"] - 1 > 1024
    for o in objs:
        o.close()
    idx.close()


# ---- 6. launch edges ----------------------------------------------------------------------------------------------------
def distinct_walk(rng, k, m):
    """a sequence of m + k - 1 bases whose m k-mers are pairwise distinct"""
    for _ in range(1000):
        s = pw.rand_seq(rng, k)
        seen = {s}
        while len(seen) < m:
            nxt = [c for c in "ACGT" if s[-(k - 1):] + c not in seen]
            if not nxt:
                break
            s += rng.choice(nxt)
            seen.add(s[-k:])
        if len(seen) == m:
            return s
    raise AssertionError("no walk of %d distinct %d-mers" % (m, k))


def test_launch_edges(gpu):
    k = 5
    rng = random.Random(6)
    walk = distinct_walk(rng, k, 300)
    big, small = tw.make_index([walk], k), tw.make_index([walk[:14 + k - 1]], k)
    assert big.n_kmers == 300 and small.n_kmers == 14
    with built(big, 2, [(0, [walk], False), (1, [walk[100:180], walk[250:]], False)]) as s_big, \
            built(small, 65, [(0, [walk[:12]], False), (64, [walk[5:14 + k - 1]], False)]) as s_small:
        for m in (1, 63, 64, 65, 255, 256, 257):
            u = tw.make_index([walk[:m + k - 1]], k)
            assert u.n_kmers == m
            check_against_brute(u, s_big, s_small, None, ("a larger than u", m))
            check_against_brute(u, s_small, s_big, 7, ("u larger than a" if m > 14 else "u smaller than both", m))
            check_against_brute(u, s_small, None, None, ("small alone", m))
            u.close()
    big.close()
    small.close()


# ---- 7. the queries of the result -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
def test_queries_of_the_merged_object(gpu, rc):
    case = pw.Case(1, rc)
    k, st = case.k, case.strains
    R1, R2 = [st[0], case.X, case.P], [st[1], st[2], case.Y, case.P]
    a, b = tw.make_index(R1, k, rc), tw.make_index(R2, k, rc)
    u = setop_index(a, b)
    adds_a = [(c, [s], rc) for c, s in zip((0, 1, 65), R1)]
    adds_b = [(c, [s], rc) for c, s in zip((0, 1, 2, 3), R2)]
    reads = case.reads()
    with built(a, 66, adds_a) as sa, built(b, 4, adds_b) as sb, capi.ColorSets.merge(u, sa, sb) as got, \
            built(u, 70, adds_a + [(66 + c, s, both) for c, s, both in adds_b]) as want:
        assert same(got.copy(), want.copy())
        for strands in (1, 2):
            for ppm, den in QUERIES:
                res = got.pseudoalign_reads(reads, strands == 2, ppm, den, counts=True)
                assert same(res, want.pseudoalign_reads(reads, strands == 2, ppm, den, counts=True)), (strands, ppm, den)
        assert any(r["n_found"] for r in res[0])
        labels = tw.labels_of(u)
        _, col_a, _ = colouring(a, sa)
        _, col_b, _ = colouring(b, sb)
        with got.expand() as wide:
            assert np.array_equal(wide.rows(), pw.rows_array(mb.rows(labels, ["$" in x for x in labels], col_a, col_b, 66), 2))
    for x in (a, b, u):
        x.close()


# ---- 8. refusals, and two host threads --------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_leave_everything_usable(pair):
    a, b, sa, sb, k = pair["a"], pair["b"], pair["sa"], pair["sb"], pair["k"]
    L, vp, C = capi.lib(), capi.C.c_void_p, capi.C
    u = setop_index(a, b)
    reads = [s.encode() for s in pair["R1"][:3] + pair["R2"][-2:]]
    before = (sa.copy(), sb.copy(), sa.pseudoalign_reads(reads), sb.pseudoalign_reads(reads, True, 500_000, 1))

    def raw(u_, sa_, sb_, offset, out=True):
        h = vp()
        capi._check(L.sbwtgpu_colorsets_merge(u_, sa_, sb_, offset, C.byref(h) if out else None, None))
        L.sbwtgpu_colorsets_destroy(h)

    refused(lambda: raw(None, sa.handle, sb.handle, 3), "NULL")
    refused(lambda: raw(u.handle, None, sb.handle, 3), "NULL")
    refused(lambda: raw(u.handle, sa.handle, sb.handle, 3, out=False), "NULL")
    raw(u.handle, sa.handle, None, 0)                                          # sb and info may be NULL
    # different k among u, a, b
    other_k = tw.make_index(pair["R1"], k + 1)
    with built(other_k, 3, [(0, pair["R1"][:1], False)]) as s_other:
        refused(lambda: capi.ColorSets.merge(other_k, sa, sb), "differ in k", str(k + 1))
        refused(lambda: capi.ColorSets.merge(u, sa, s_other), "differ in k", str(k + 1))
        refused(lambda: capi.ColorSets.merge(u, s_other, sb), "differ in k", str(k + 1))
    other_k.close()
    # k outside 2 .. 64
    rng = random.Random(65)
    long_seqs = [pw.rand_seq(rng, 200)]
    k65 = tw.make_index(long_seqs, 65)
    with built(k65, 2, [(0, long_seqs, False)]) as s65:
        refused(lambda: capi.ColorSets.merge(k65, s65), "k = 65", "2 <= k <= 64")
    k65.close()
    # a rank-only u (a rank-only a or b cannot carry a colour-set object: create refuses it)
    bits = np.random.default_rng(1).integers(0, 2**64, size=4, dtype=np.uint64)
    ro = capi.Index.create(bits, bits, bits, bits, None, 256, k)
    refused(lambda: capi.ColorSets.merge(ro, sa, sb), "only rank()")
    refused(lambda: capi.ColorSetsBuilder.create(ro, 2), "only rank()")
    ro.close()
    # the offset and the number of colours
    refused(lambda: capi.ColorSets.merge(u, sa, sb, -1), "color_offset_b", "negative")
    refused(lambda: capi.ColorSets.merge(u, sa, None, 3), "color_offset_b", "without sb")
    refused(lambda: capi.ColorSets.merge(u, sa, sb, 4027), "4097", "4096")
    with capi.ColorSets.merge(u, sa, sb, 4026) as widest:
        assert widest.n_colors == 4096 and widest.words == 64
    if capi.device_count() >= 2:                                               # indexes on different devices
        bits = hostlib.build_bits([s.encode() for s in pair["R1"]], k, False, True)
        far = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0,
                                device=1)
        refused(lambda: capi.ColorSets.merge(far, sa, sb), "different devices")
        far.close()
    # everything still answers, and the inputs are what they were
    after = (sa.copy(), sb.copy(), sa.pseudoalign_reads(reads), sb.pseudoalign_reads(reads, True, 500_000, 1))
    assert all(same(x, y) for x, y in zip(before, after))
    assert len(a.search_reads(reads[:1])[0]) == len(reads[0]) - k + 1 and len(u.search_reads(reads[:1])[0]) == len(reads[0]) - k + 1
    check_against_brute(u, sa, sb, None, "after the refusals")
    u.close()


def test_an_index_of_2_pow_31_columns_is_refused_as_u(pair):
    n = 1 << 31
    w = np.zeros(n // 64, dtype=np.uint64)
    big = capi.Index.create(w, w, w, w, None, n, pair["k"], 0, 0)
    refused(lambda: capi.ColorSets.merge(big, pair["sa"], pair["sb"]), "2^31", "columns")
    big.close()


def test_two_host_threads_merge_the_same_inputs(pair):
    a, b, sa, sb = pair["a"], pair["b"], pair["sa"], pair["sb"]
    u = setop_index(a, b)
    with capi.ColorSets.merge(u, sa, sb) as m:
        want = m.copy()
    out, errs = [None, None], []

    def work(t):
        try:
            res = []
            for _ in range(3):
                with capi.ColorSets.merge(u, sa, sb, None if t == 0 else 3) as m:
                    res.append(m.copy())
            out[t] = res
        except Exception as e:        # noqa: BLE001 -- reported below
            errs.append(e)
    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    assert all(same(r, want) for res in out for r in res)
    u.close()


# ---- 9. the CLI -------------------------------------------------------------------------------------------------------------
def test_cli_merge_colors(gpu, tmp_path):
    d = str(tmp_path)
    k = 13
    rng = random.Random(9)
    pool = references(rng, k, 7)
    sides = {"a": pool[:4], "b": pool[2:]}
    SBWT = tw.SBWT

    def write_refs(name, seqs, first):
        with open("%s/%s.fna" % (d, name), "w") as fh, open("%s/%s.refs" % (d, name), "w") as lst:
            for i, s in enumerate(seqs):
                fh.write(">s%d\n%s\n" % (i, s))
                ref = "%s/ref%d.fna" % (d, first + i)
                with open(ref, "w") as one:
                    one.write(">r\n%s\n" % s)
                lst.write(ref + "\n")
    write_refs("a", sides["a"], 0)
    write_refs("b", sides["b"], 4)
    for name in ("a", "b"):
        p = tw.run([SBWT, "build", "-i", "%s/%s.fna" % (d, name), "-o", "%s/%s.sbwt" % (d, name), "-k", str(k), "--temp-dir", d])
        assert p.returncode == 0, p.stderr.decode()
        p = tw.run([SBWT, "build-colors", "--compress", "--stream", "-i", "%s/%s.sbwt" % (d, name), "-r", "%s/%s.refs" % (d, name),
                    "-o", "%s/%s.colors" % (d, name)])
        assert p.returncode == 0, p.stderr.decode()
    p = tw.run([SBWT, "set-op", "--op", "union", "-a", d + "/a.sbwt", "-b", d + "/b.sbwt", "-o", d + "/u.sbwt"])
    assert p.returncode == 0, p.stderr.decode()
    with open(d + "/u.refs", "w") as lst:
        lst.write(open(d + "/a.refs").read() + open(d + "/b.refs").read())
    p = tw.run([SBWT, "build-colors", "--compress", "--stream", "-i", d + "/u.sbwt", "-r", d + "/u.refs", "-o", d + "/want.colors"])
    assert p.returncode == 0, p.stderr.decode()
    want = open(d + "/want.colors", "rb").read()
    merge = [SBWT, "merge-colors", "-u", d + "/u.sbwt", "-a", d + "/a.sbwt", "--colors-a", d + "/a.colors", "-b", d + "/b.sbwt",
             "--colors-b", d + "/b.colors"]
    p = tw.run(merge + ["-o", d + "/got.colors"])
    assert p.returncode == 0, p.stderr.decode()
    assert open(d + "/got.colors", "rb").read() == want and want[:8] == b"SBWTCOL3"
    n_u = len(kmer_set(pool, k))
    line = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("merge-colors:")]
    assert len(line) == 1 and line[0].startswith("merge-colors: %d k-mers in u, %d from a, %d from b, " %
                                                 (n_u, len(kmer_set(sides["a"], k)), len(kmer_set(sides["b"], k)))), p.stdout
    # an explicit offset equal to the default; an "SBWTCOL1" file of a goes in through the device's compress
    p = tw.run([SBWT, "build-colors", "-i", d + "/a.sbwt", "-r", d + "/a.refs", "-o", d + "/a.col1"])
    assert p.returncode == 0 and open(d + "/a.col1", "rb").read(8) == b"SBWTCOL1", p.stderr.decode()
    p = tw.run([SBWT, "merge-colors", "-u", d + "/u.sbwt", "-a", d + "/a.sbwt", "--colors-a", d + "/a.col1", "-b", d + "/b.sbwt",
                "--colors-b", d + "/b.colors", "--color-offset", "4", "-o", d + "/got1.colors"])
    assert p.returncode == 0, p.stderr.decode()
    assert open(d + "/got1.colors", "rb").read() == want
    # one side alone: a's colours restricted to ... a itself gives a's file back
    p = tw.run([SBWT, "merge-colors", "-u", d + "/a.sbwt", "-a", d + "/a.sbwt", "--colors-a", d + "/a.colors", "-o", d + "/same.colors"])
    assert p.returncode == 0, p.stderr.decode()
    assert open(d + "/same.colors", "rb").read() == open(d + "/a.colors", "rb").read()
    # a colour file of the wrong index, and the library's refusals, end with the message and a non-zero exit
    p = tw.run([SBWT, "merge-colors", "-u", d + "/u.sbwt", "-a", d + "/a.sbwt", "--colors-a", d + "/b.colors", "-o", d + "/x.colors"], 60)
    assert p.returncode != 0 and b"columns at k =" in p.stderr
    p = tw.run(merge + ["--color-offset", "4095", "-o", d + "/x.colors"], 60)
    assert p.returncode != 0 and b"4096" in p.stderr
    p = tw.run(merge + ["--color-offset", "-2", "-o", d + "/x.colors"], 60)
    assert p.returncode != 0 and b"negative" in p.stderr
    p = tw.run(merge[:8] + ["--color-offset", "2", "-o", d + "/x.colors"], 60)
    assert p.returncode != 0 and b"--color-offset" in p.stderr


# ---- 10. a bounded seeded fuzz ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_fuzz(gpu, seed):
    rng = random.Random(9000 + seed)
    for case in range(5):
        k = rng.randint(2, 64)
        alphabet = "AC" if k <= 4 else "ACGT"
        rc = rng.random() < 0.3

        def seqs():
            out = [pw.rand_seq(rng, rng.randint(k, 2 * k + 80), alphabet) for _ in range(rng.randint(1, 4))]
            unit = pw.rand_seq(rng, rng.randint(1, 4), alphabet)
            out.append((unit * (3 * k))[:rng.randint(k, 3 * k)])           # a periodic one
            return out
        shared = seqs()
        Ra, Rb = seqs() + shared[:2], seqs() + shared[1:]
        a, b = tw.make_index(Ra, k, rc, rng.random() < 0.5), tw.make_index(Rb, k, rc and rng.random() < 0.5)
        n_a, n_b = (rng.choice([rng.randint(1, 64), rng.randint(65, 300), 4000]) for _ in range(2))
        offset = rng.choice([None, 0, rng.randint(0, 4096 - n_b), 4096 - n_b])
        op = rng.choice(OPS + ("a", "b"))
        u = a if op == "a" else b if op == "b" else setop_index(a, b, op)
        label = (seed, case, k, rc, n_a, n_b, offset, op)
        both = rng.random() < 0.5
        with built(a, n_a, [(c, s, both) for c, s in sorted(tw.fuzz_inputs(rng, Ra, k, n_a).items())]) as sa, \
                built(b, n_b, [(c, s, both) for c, s in sorted(tw.fuzz_inputs(rng, Rb, k, n_b).items())]) as sb:
            if offset is None and n_a + n_b > 4096:
                refused(lambda: capi.ColorSets.merge(u, sa, sb), "4096")
                offset = 4096 - n_b
            if rng.random() < 0.85:
                check_against_brute(u, sa, sb, offset, label)
            else:
                check_against_brute(u, sa, None, None, label)
        for x in {id(a): a, id(b): b, id(u): u}.values():
            x.close()
