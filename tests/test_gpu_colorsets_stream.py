"""GPU: the colour-set builder (sbwt_colorsets.hip, "the builder": colour sets made one colour at a time, without the wide
matrix) against the wide route -- WideColors coloured by the same adds, then ColorSets.from_colors -- whose bytes it must
give, against the definition (tests/colorsets_brute.py) and against its model (tests/colorsets_stream_model.py): every
n_colors that changes a path, closing orders, split calls, table growth, rows changed in place, chunking, strands, corners,
info between closes, every refusal, the queries of the finished object, the C++ CLI and a bounded seeded fuzz.  All
comparisons are exact."""
import gzip
import random

import numpy as np
import pytest

import colorsets_brute as cb
import colorsets_stream_model as sm
import pseudoalign_brute as pb
import pseudoalign_wide as pw
import test_gpu_pseudoalign_wide as tw          # its helpers: World, tuning, refused, run, the fuzz's colour inputs
from bruteforce import kmer_set
from sbwt_amd import capi

pytestmark = pytest.mark.gpu

QUERIES = tw.QUERIES
N_COLORS = (1, 64, 65, 200, 4096)
refused = tw.refused


@pytest.fixture(scope="module")
def worlds(gpu):
    made = {}

    def get(rc):
        if rc not in made:
            made[rc] = tw.World(rc)
        return made[rc]
    yield get
    for w in made.values():
        for _, col, _, _ in w.made.values():
            col.close()


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def wide_route(idx, n_colors, adds):
    """(ids, table, info) of ColorSets.from_colors of a WideColors coloured by adds: (colour, sequences, both strands)"""
    with capi.WideColors.create(idx, n_colors) as col:
        for c, seqs, both in adds:
            col.add_reads(c, [s.encode() for s in seqs], both)
        with capi.ColorSets.from_colors(col) as s:
            return s.copy() + (s.info(),)


def stream_route(idx, n_colors, adds):
    with capi.ColorSetsBuilder.create(idx, n_colors) as b:
        for c, seqs, both in adds:
            b.add_reads(c, [s.encode() for s in seqs], both)
        with b.finish() as s:
            return s.copy() + (s.info(),)


# ---- 1. canonical bytes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
@pytest.mark.parametrize("n_colors", N_COLORS)
def test_finish_gives_the_bytes_of_compress(worlds, n_colors, rc):
    w = worlds(rc)
    case, col, cs, _ = w.colours(n_colors)
    both = case.strands_add == 2
    matrix = col.rows()
    want = cb.canonical_arrays(matrix)
    with capi.ColorSets.from_colors(col) as s:
        assert same(s.copy(), want)
        want_info = s.info()
    per = [len(x) for x in cs]
    for order in ("ascending", "descending", "split"):
        colours = sorted(case.inputs, reverse=order == "descending")
        with capi.ColorSetsBuilder.create(w.idx, n_colors) as b:
            for c in colours:
                seqs = case.inputs[c]
                calls = [seqs] if order != "split" else [seqs[:1], [], seqs[1:], seqs[:1]]       # (and one batch again)
                for part in calls:
                    mine = [set() for _ in range(n_colors)]
                    assert b.add_reads(c, [x.encode() for x in part], both) == pb.add(mine, w.kmers, w.k, c, part, case.strands_add), (c, part)
            with b.finish() as s:
                got = s.copy()
                assert got[0].dtype == np.uint32 and got[1].dtype == np.uint64
                assert same(got, want), (n_colors, rc, order)
                assert s.info() == want_info == {"n_columns": w.idx.n_nodes, "k": w.k, "n_colors": n_colors, "words": pw.n_words(n_colors),
                                                 "n_sets": len(want[1]), "n_colored_columns": int(matrix.any(axis=1).sum()),
                                                 "device_bytes": 4 * w.idx.n_nodes + 8 * want[1].size}
                cb.check_invariants(got[0].tolist(), pw.rows_ints(got[1]), n_colors, ["$" in lab for lab in w.labels])
                with s.expand() as back:
                    assert np.array_equal(back.rows(), matrix) and back.info()["per_color"] == per
    assert np.array_equal(col.rows(), matrix)


# ---- 2. table growth --------------------------------------------------------------------------------------------------
def test_the_table_grows(worlds):
    w = worlds(False)
    n_colors = 4096
    real = [lab for lab in w.labels if "$" not in lab]
    assert len(real) > 1000
    # colour b gets the k-mers of the real columns whose rank among the real columns has bit b set; colour 4095 all of them
    adds = [(b, [lab for r, lab in enumerate(real) if (r >> b) & 1], False) for b in range(11)] + [(4095, real, False)]
    patterns = {r & 2047 for r in range(len(real))}
    with capi.ColorSetsBuilder.create(w.idx, n_colors) as b:
        for c, seqs, both in adds:
            assert b.add_reads(c, [s.encode() for s in seqs], both) == (len(seqs),) * 2
        before = b.info()                                       # colours 0 .. 10 are closed, 4095 is open
        cap = sm.FIRST_CAPACITY
        while cap < len(patterns):
            cap *= 2
        assert cap >= 1024 and before["n_sets"] == len(patterns)
        assert before["device_bytes"] == 4 * w.idx.n_nodes + 8 * ((w.idx.n_nodes + 63) // 64) + cap * (8 * 64 + 4)
        assert before["per_color"][:11] == [len(seqs) for _, seqs, _ in adds[:11]] and before["per_color"][4095] == 0
        with b.finish() as s:
            got = s.copy() + (s.info(),)
    assert got[2]["n_sets"] > 1000                              # the 64-row capacity doubled at least four times
    assert got[2]["n_sets"] == len(patterns) + 1 and got[2]["n_colored_columns"] == len(real)
    want = wide_route(w.idx, n_colors, adds)
    assert same(got[:2], want[:2]) and got[2] == want[2]
    rank = {lab: r for r, lab in enumerate(real)}
    rows = [(rank[lab] & 2047) | (1 << 4095) if lab in rank else 0 for lab in w.labels]
    assert same(got[:2], cb.arrays(*cb.canonical(rows), n_colors))


# ---- 3. rows changed in place -------------------------------------------------------------------------------------------
def test_in_place_rows(worlds):
    w = worlds(False)
    case = w.case0
    # colours 0 and 70 get exactly the same sequences: the rows {0, 70} only
    seqs = [case.strains[1], case.X, "ACGTN", ""]
    adds = [(0, seqs, False), (70, seqs, False)]
    got, want = stream_route(w.idx, 200, adds), wide_route(w.idx, 200, adds)
    assert same(got[:2], want[:2]) and got[2] == want[2]
    rows = pb.rows_of(w.labels, [set(kmer_set(seqs[:2], w.k)) if c in (0, 70) else set() for c in range(200)], w.kmers)
    assert got[2]["n_sets"] == len(cb.canonical(rows)[1]) == 2 and pw.rows_ints(got[1]) == [0, (1 << 70) | 1]
    # a colour given every sequence of the index after others have been closed: no set is added by that close
    with capi.ColorSetsBuilder.create(w.idx, 200) as b:
        for c in (5, 199, 64):
            b.add_reads(c, [x.encode() for x in case.inputs.get(c, [case.strains[c % 3][c:c + 150]])])
        b.add_reads(7, [case.strains[2][:200].encode()])
        b.add_reads(1, [s.encode() for s in case.seqs])            # closes 7
        before = b.info()
        b.add_reads(2, [b"ACGT"])                                  # closes 1: the empty set alone splits
        after = b.info()
        assert after["n_sets"] == before["n_sets"] + 1 and after["per_color"][1] == len(w.kmers) == after["n_colored_columns"]
        with b.finish() as s:
            assert s.n_sets == after["n_sets"]
            ids, table = s.copy()
            assert all(row & 2 for row in pw.rows_ints(table)[1:])


# ---- 4. chunking and strands ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [False, True], ids=["fwd-two-strands", "rc-one-strand"])
def test_chunking_and_strands(worlds, rc):
    w = worlds(rc)
    n_colors = 65
    case, col, cs, _ = w.colours(n_colors)
    assert case.strands_add == (1 if rc else 2)
    adds = [(c, seqs, case.strands_add == 2) for c, seqs in sorted(case.inputs.items())]
    with capi.ColorSets.from_colors(col) as s:
        want = s.copy()
    assert same(stream_route(w.idx, n_colors, adds)[:2], want)
    for budget in (64, 1):                                        # several chunks on two slots; every sequence a chunk
        with tw.tuning("pseudoalign_chunk_bases", budget, 0):
            assert same(stream_route(w.idx, n_colors, adds)[:2], want), budget
    # the other strand mode, against the wide route in that mode
    other = [(c, seqs, not both) for c, seqs, both in adds]
    got, wide = stream_route(w.idx, n_colors, other), wide_route(w.idx, n_colors, other)
    assert same(got[:2], wide[:2]) and got[2] == wide[2]


# ---- 5. corners -------------------------------------------------------------------------------------------------------
def test_corners(worlds):
    w = worlds(False)
    idx, case = w.idx, w.case0
    for n_colors in (1, 130):
        with capi.ColorSetsBuilder.create(idx, n_colors) as b, b.finish() as s:          # nothing added
            ids, table = s.copy()
            assert s.n_sets == 1 and not ids.any() and table.shape == (1, pw.n_words(n_colors)) and not table.any()
            assert s.info()["n_colored_columns"] == 0
    miss = pw.rand_seq(random.Random(3), 200)
    assert not kmer_set([miss], w.k) & w.kmers
    adds = [(3, [miss], True),                                                      # hits nothing
            (9, ["ACGTN", "", case.strains[0][:w.k - 1]], False),                    # shorter than k
            (129, [case.strains[0][:100]], False), (129, [case.strains[0][:100]], False),   # the identical batch again
            (0, [], False),                                                          # no sequence at all
            (64, [case.strains[0][50:160], miss], False)]
    with capi.ColorSetsBuilder.create(idx, 130) as b:
        assert b.add_reads(3, [miss.encode()], True) == (200 - w.k + 1, 0)
        assert b.add_reads(9, [b"ACGTN", b"", case.strains[0][:w.k - 1].encode()]) == (0, 0)
        assert b.add_reads(129, [case.strains[0][:100].encode()]) == (100 - w.k + 1,) * 2
        assert b.add_reads(129, [case.strains[0][:100].encode()]) == (100 - w.k + 1,) * 2
        assert b.add_reads(0, []) == (0, 0)
        assert b.info()["per_color"][129] == 100 - w.k + 1 and b.info()["per_color"][3] == 0 and b.info()["n_sets"] == 2
        assert b.add_reads(64, [case.strains[0][50:160].encode(), miss.encode()]) == (110 - w.k + 1 + 200 - w.k + 1, 110 - w.k + 1)
        with b.finish() as s:
            got = s.copy() + (s.info(),)
    want = wide_route(idx, 130, adds)
    assert same(got[:2], want[:2]) and got[2] == want[2] and got[2]["n_sets"] == 4


# ---- 6. info between closes -----------------------------------------------------------------------------------------------
def test_info_follows_the_model(worlds):
    w = worlds(True)
    n_colors = 200
    case = pw.Case(n_colors, True)
    where = {lab: j for j, lab in enumerate(w.labels) if "$" not in lab}
    n = w.idx.n_nodes
    model = sm.Builder(n, n_colors)
    order = sorted(case.inputs)
    random.Random(6).shuffle(order)
    with capi.ColorSetsBuilder.create(w.idx, n_colors) as b:
        fixed = {"n_columns": n, "k": w.k, "n_colors": n_colors, "words": 4}
        assert b.info() == dict(fixed, **model.info())
        for c in order:
            for part in (case.inputs[c][:1], case.inputs[c][1:]):
                one = [set() for _ in range(n_colors)]
                pb.add(one, w.kmers, w.k, c, part, 2)
                model.add(c, [where[x] for x in one[c]])
                b.add_reads(c, [x.encode() for x in part], True)
                assert b.info() == dict(fixed, **model.info()), c          # the open colour's marks are not yet visible
                assert b.info()["per_color"][c] == 0
            model.check()
        before = b.info()
        with b.finish() as s:
            ids, table = model.finish()
            assert same(s.copy(), cb.arrays(ids, table, n_colors))
            assert s.info()["n_colored_columns"] == model.n_colored >= before["n_colored_columns"]
    assert model.from_empty >= 1 and model.split >= 1


# ---- 7. refusals --------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_leave_everything_usable(worlds):
    w = worlds(False)
    idx, k, case = w.idx, w.k, w.case0
    L, vp = capi.lib(), capi.C.c_void_p
    a, bq, c3 = (case.strains[i].encode() for i in range(3))
    for nc in (0, 4097, -1):
        refused(lambda: capi.ColorSetsBuilder.create(idx, nc), "n_colors", "4096")
    bits = np.random.default_rng(1).integers(0, 2**64, size=4, dtype=np.uint64)
    ro = capi.Index.create(bits, bits, bits, bits, None, 256, 3)
    refused(lambda: capi.ColorSetsBuilder.create(ro, 65), "only rank()")
    ro.close()
    refused(lambda: capi._check(L.sbwtgpu_colorsets_builder_create(None, 65, capi.C.byref(vp()))), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_colorsets_builder_create(idx.handle, 65, None)), "NULL")
    b = capi.ColorSetsBuilder.create(idx, 65)
    assert b.add_reads(0, [a]) == (400 - k + 1,) * 2
    assert b.add_reads(64, [bq]) == (400 - k + 1,) * 2                              # closes 0
    refused(lambda: b.add_reads(0, [c3]), "colour 0", "consecutive calls")           # a closed colour reopened
    assert b.add_reads(64, [bq[:50]]) == (50 - k + 1,) * 2                          # ... and the open one goes on
    for colour in (65, 4096, -1):
        refused(lambda: b.add_reads(colour, [a]), "color %d" % colour, "65 colours")
    bases, off = capi.concat_reads([a])
    host = (bases.ctypes.data, off.ctypes.data, 1)
    nw, nh = capi.C.c_int64(), capi.C.c_int64()
    refused(lambda: capi._check(L.sbwtgpu_colorsets_builder_add_batch(b.handle, 1, *host, 3, capi.C.byref(nw), capi.C.byref(nh))), "strands")
    refused(lambda: capi._check(L.sbwtgpu_colorsets_builder_add_batch(None, 1, *host, 1, capi.C.byref(nw), capi.C.byref(nh))), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_colorsets_builder_add_batch(b.handle, 1, None, off.ctypes.data, 1, 1, None, None)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_colorsets_builder_add_batch(b.handle, 1, bases.ctypes.data, None, 1, 1, None, None)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_colorsets_builder_info(None, None, None, None, None, None, None, None, None)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_colorsets_builder_finish(b.handle, None)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_colorsets_builder_finish(None, capi.C.byref(vp()))), "NULL")
    L.sbwtgpu_colorsets_builder_destroy(None)
    capi._check(L.sbwtgpu_colorsets_builder_info(b.handle, None, None, None, None, None, None, None, None))      # every output may be NULL
    assert b.info()["per_color"][0] == len(kmer_set([a.decode()], k)) and b.info()["per_color"][64] == 0      # (the refused calls closed nothing: 64 is still open)
    assert capi._check(L.sbwtgpu_colorsets_builder_add_batch(b.handle, 64, *host, 2, None, None)) is None        # the counts may be NULL
    assert b.add_reads(1, [c3]) == (400 - k + 1,) * 2                               # a following add succeeds
    assert len(idx.search_reads([a])[0]) == 400 - k + 1                             # the index is usable
    adds = [(0, [a.decode()], False), (64, [bq.decode()], False), (64, [a.decode()], True), (1, [c3.decode()], False)]
    s = b.finish()
    want = wide_route(idx, 65, adds)
    assert same(s.copy(), want[:2]) and s.info() == want[2]
    # any call after finish is refused; the object it returned lives on
    refused(lambda: b.add_reads(2, [a]), "finish")
    refused(lambda: b.info(), "finish")
    refused(lambda: b.finish(), "finish")
    b.close()
    assert same(s.copy(), want[:2])
    s.close()


# ---- 8. the queries of the finished object ------------------------------------------------------------------------------
def test_queries_equal_the_wide_object(worlds):
    w = worlds(True)
    case, col, cs, exp = w.colours(200)
    reads = case.reads()
    with capi.ColorSetsBuilder.create(w.idx, 200) as b:
        for c, seqs in sorted(case.inputs.items(), reverse=True):
            b.add_reads(c, [s.encode() for s in seqs], case.strands_add == 2)
        with b.finish() as s:
            for strands in (1, 2):
                for ppm, den in QUERIES:
                    got = s.pseudoalign_reads(reads, strands == 2, ppm, den, counts=True)
                    assert same(got, col.pseudoalign_reads(reads, strands == 2, ppm, den, counts=True)), (strands, ppm, den)
                    assert same(s.pseudoalign_reads(reads, strands == 2, ppm, den), got[:2]), (strands, ppm, den)
            assert tw.as_lists(*s.pseudoalign_reads(reads[:40], True)) == \
                [exp.record_of(exp.window_sets(r, 2), 1_000_000, 0) for r in reads[:40]]


# ---- 9. the CLI ---------------------------------------------------------------------------------------------------------
def test_cli_stream(gpu, tmp_path):
    d = str(tmp_path)
    case = pw.Case(65, False)
    k, seqs = case.k, case.seqs
    with open(d + "/s.fna", "w") as fh:
        for i, s in enumerate(seqs):
            fh.write(">s%d\n%s\n" % (i, s))
    p = tw.run([tw.SBWT, "build", "-i", d + "/s.fna", "-o", d + "/fwd.sbwt", "-k", str(k), "--temp-dir", d])
    assert p.returncode == 0, p.stderr.decode()
    rng = random.Random(65)
    with open(d + "/refs.txt", "w") as fh:
        for c in range(65):                                   # 65 references, gzipped and plain FASTA; one without a k-mer
            if c in (0, 63, 64):
                mine = [s for s in case.inputs[c] if s]
            elif c == 30:
                mine = ["ACGT"]
            else:
                s = case.strains[c % 3]
                a = rng.randrange(0, 300)
                mine = [s[a:a + rng.randint(20, 100)]]
            text = "".join(">r%d_%d\n%s\n" % (c, j, s) for j, s in enumerate(mine)).encode()
            name = "%s/ref%d.fna%s" % (d, c, ".gz" if c % 2 else "")
            with (gzip.open if c % 2 else open)(name, "wb") as out:
                out.write(text)
            fh.write(name + "\n")
    reads = [r.upper() for r in case.reads() if r]
    with open(d + "/r.fq", "w") as fh:
        for j, r in enumerate(reads):
            fh.write("@r%d\n%s\n+\n%s\n" % (j, r.decode(), "I" * len(r)))
    for flags in ([], ["--both-strands"]):
        outs = {}
        for name, extra in (("wide", []), ("stream", ["--stream"])):
            path = "%s/%s%d.colors" % (d, name, len(flags))
            p = tw.run([tw.SBWT, "build-colors", "--compress", "-i", d + "/fwd.sbwt", "-r", d + "/refs.txt", "-o", path] + extra + flags)
            assert p.returncode == 0, p.stderr.decode()
            outs[name] = (open(path, "rb").read(), p.stdout)
        assert outs["stream"][0] == outs["wide"][0] and outs["stream"][0][:8] == b"SBWTCOL3"
        assert outs["stream"][1] == outs["wide"][1]
        lines = [ln for ln in outs["stream"][1].decode().splitlines() if ln.startswith("colour ")]
        assert len(lines) == 65 and lines[30].endswith(" 0 coloured columns") and not lines[64].endswith(" 0 coloured columns")
        got = []
        for name in ("wide", "stream"):
            p = tw.run([tw.SBWT, "pseudoalign", "-i", d + "/fwd.sbwt", "-c", "%s/%s%d.colors" % (d, name, len(flags)), "-q", d + "/r.fq",
                        "-o", d + "/o.out", "--threshold", "0.5"] + flags)
            assert p.returncode == 0, p.stderr.decode()
            got.append(open(d + "/o.out", "rb").read())
        assert got[0] == got[1] and len(got[0].splitlines()) == len(reads)
    # --stream alone is refused and says what it needs
    for extra in ([], ["--wide"]):
        p = tw.run([tw.SBWT, "build-colors", "--stream", "-i", d + "/fwd.sbwt", "-r", d + "/refs.txt", "-o", d + "/x.colors"] + extra, 60)
        assert p.returncode != 0 and b"--stream" in p.stderr and b"--compress" in p.stderr


# ---- 10. a bounded seeded fuzz --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_fuzz(gpu, seed):
    rng = random.Random(8000 + seed)
    for case in range(4):
        k = rng.randint(2, 64)
        rc, ssup = rng.random() < 0.5, rng.random() < 0.5
        n_colors = rng.choice([rng.randint(1, 64), rng.randint(65, 300), 4096])
        both = rng.random() < 0.5
        seqs = [pw.rand_seq(rng, rng.randint(k, 2 * k + 80)) for _ in range(rng.randint(1, 4))]
        label = (seed, case, k, rc, ssup, n_colors, both)
        idx = tw.make_index(seqs, k, rc, ssup)
        inputs = tw.fuzz_inputs(rng, seqs, k, n_colors)
        order = list(inputs)
        rng.shuffle(order)
        adds = []
        for c in order:                                         # a colour's sequences over one to three calls, some repeated
            mine = list(inputs[c])
            while mine:
                cut = rng.randint(1, len(mine))
                adds.append((c, mine[:cut], both))
                mine = mine[cut:]
            if rng.random() < 0.3:
                adds.append((c, inputs[c][:1], both))
        with tw.tuning("pseudoalign_chunk_bases", rng.choice([0, 1, 40]), 0):
            got = stream_route(idx, n_colors, adds)
        want = wide_route(idx, n_colors, adds)
        assert same(got[:2], want[:2]) and got[2] == want[2], label
        idx.close()
