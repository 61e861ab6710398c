"""CPU: the colour-set builder's algorithm (tests/colorsets_stream_model.py: ids, table, cnt, close, finish) against the
definition of the canonical form (tests/colorsets_brute.py) on the shared pan-genome of tests/pseudoalign_wide.py and on
small random colourings, in several closing orders; what its closes do; and the CLI's usage text."""
import os
import random
import subprocess

import pytest

import colorsets_brute as cb
import colorsets_stream_model as sm
import pseudoalign_brute as pb
import pseudoalign_wide as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")
N_COLORS = (1, 64, 65, 200, 4096)


def columns_of(kmers):
    """A column order for the k-mers of an index without the index: colex order, a dummy column in front and one after
    every 40 k-mers (no k-mer lives there, so no add marks them)."""
    labels, where = ["$"], {}
    for i, x in enumerate(sorted(kmers, key=lambda s: s[::-1])):
        where[x] = len(labels)
        labels.append(x)
        if i % 40 == 39:
            labels.append("$" + x[1:])
    return labels, where


def case_adds(case, kmers, where):
    """per colour of the case: the columns its sequences mark (the brute force's colouring of that colour alone), and all
    colour sets"""
    cs = [set() for _ in range(case.n_colors)]
    marks = {}
    for c, seqs in sorted(case.inputs.items()):
        pb.add(cs, kmers, case.k, c, seqs, case.strands_add)
        marks[c] = sorted(where[x] for x in cs[c])
    return marks, cs


def orders(colours, seed):
    shuffled = list(colours)
    random.Random(seed).shuffle(shuffled)
    return {"ascending": sorted(colours), "descending": sorted(colours, reverse=True), "shuffled": shuffled}


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(rc):
        if rc not in made:
            kmers = pw.Case(1, rc).index_kmers()
            made[rc] = (kmers,) + columns_of(kmers)
        return made[rc]
    return get


@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
@pytest.mark.parametrize("n_colors", N_COLORS)
def test_the_model_gives_the_canonical_form_in_every_closing_order(worlds, n_colors, rc):
    kmers, labels, where = worlds(rc)
    case = pw.Case(n_colors, rc)
    marks, cs = case_adds(case, kmers, where)
    want = cb.canonical(pb.rows_of(labels, cs, kmers))
    assert len(want[1]) >= 2
    for name, order in orders(list(marks), n_colors).items():
        adds = []
        for c in order:                                       # a colour's columns in two calls that overlap, the first one twice
            half = len(marks[c]) // 2
            adds += [(c, marks[c][:half + 3]), (c, marks[c][:half + 3]), (c, marks[c][half:])]
        ids, table, b = sm.build(len(labels), n_colors, adds, random.Random(n_colors))
        assert (ids, table) == want, (n_colors, rc, name)
        cb.check_invariants(ids, table, n_colors, ["$" in lab for lab in labels])
        assert b.per_color == [len(s) for s in cs] and b.n_colored == sum(1 for i in want[0] if i)
        if n_colors >= 64:                                    # every kind of close happens
            assert b.from_empty >= 1 and b.split >= 1 and b.in_place >= 1, (name, b.from_empty, b.split, b.in_place)
        assert b.from_empty + b.split == len(table) - 1      # a set is appended once and never dropped


def test_info_between_closes_and_refusals():
    b = sm.Builder(10, 70)
    assert b.info() == {"n_sets": 1, "n_colored_columns": 0, "per_color": [0] * 70, "device_bytes": 40 + 8 + 64 * 20}
    b.add(3, [1, 2, 3])
    b.add(3, [3, 4])
    assert b.info()["n_sets"] == 1 and b.info()["per_color"][3] == 0            # an open colour's marks are not yet visible
    b.add(69, [4, 5])                                                          # closes 3
    b.check()
    assert b.info()["n_sets"] == 2 and b.info()["per_color"][3] == 4 and b.info()["n_colored_columns"] == 4
    with pytest.raises(sm.Refused, match="consecutive"):
        b.add(3, [9])
    with pytest.raises(sm.Refused, match="range"):
        b.add(70, [9])
    b.add(0, [1, 2, 3, 4])                                                     # closes 69: {3} splits, 5 comes from the empty set
    b.check()
    assert sorted(b.table) == [0, 1 << 3, 1 << 69, (1 << 3) | (1 << 69)] and (b.from_empty, b.split, b.in_place) == (2, 1, 0)
    ids, table = b.finish()                                                    # closes 0: {3} and {3, 69} change in place
    b.check()
    assert (b.from_empty, b.split, b.in_place) == (2, 1, 2)
    assert (ids, table) == cb.canonical([0, 9, 9, 9, 9 | 1 << 69, 1 << 69, 0, 0, 0, 0])
    with pytest.raises(sm.Refused, match="finish"):
        b.add(5, [1])


def test_the_table_grows_by_doubling():
    n = 1 << 10                                               # column j gets colour b where bit b of j is set: 1023 sets
    adds = [(b, [j for j in range(n) if (j >> b) & 1]) for b in range(10)]
    ids, table, b = sm.build(n, 4096, adds + [(4095, range(1, n))])
    assert len(table) == n and b.cap == 1024 and b.grown == 4 and b.in_place == 1023
    assert (ids, table) == cb.canonical([j | (1 << 4095 if j else 0) for j in range(n)])
    assert b.info()["device_bytes"] == 4 * n + n // 8 + 1024 * (8 * 64 + 4)


@pytest.mark.parametrize("seed", range(6))
def test_fuzz_of_small_random_colourings(seed):
    rng = random.Random(9000 + seed)
    for _ in range(50):
        n = rng.randint(1, 40)
        n_colors = rng.choice([1, 2, 5, 64, 65, 130])
        pool = [rng.sample(range(n), rng.randint(0, n)) for _ in range(3)]      # few distinct column sets: sets get shared
        colours = rng.sample(range(n_colors), rng.randint(0, min(n_colors, 8)))
        rows = [0] * n
        adds = []
        for c in colours:
            cols = rng.choice(pool) if rng.random() < 0.6 else rng.sample(range(n), rng.randint(0, n))
            for j in cols:
                rows[j] |= 1 << c
            cut = rng.randint(0, len(cols))
            adds += [(c, cols[:cut]), (c, cols[cut:])] + ([(c, cols)] if rng.random() < 0.3 else [])
        ids, table, b = sm.build(n, n_colors, adds, rng)
        assert (ids, table) == cb.canonical(rows), (seed, n, n_colors, adds)


def test_the_usage_text_names_the_stream_flag():
    p = subprocess.run([SBWT, "build-colors", "--help"], capture_output=True, timeout=60)          # (no GPU is opened before it)
    assert b"--stream" in p.stdout + p.stderr and b"--compress" in p.stdout + p.stderr


def test_the_binding_lists_the_builder_calls():
    from sbwt_amd import capi
    for name in ("create", "add_batch", "info", "finish", "destroy"):
        sym = "sbwtgpu_colorsets_builder_" + name
        assert sym in capi.EXPORTED_SYMBOLS and hasattr(capi.lib(), sym), sym
    for name in ("create", "add_sequences", "add_reads", "info", "finish", "close", "__enter__", "__exit__"):
        assert callable(getattr(capi.ColorSetsBuilder, name)), name
