"""CPU: the numpy reference of the colour layer (tests/colors_scale_ref.py) against the brute forces on the small shared
pan-genome, and the scale world's own conditions: it must reach the second trip of the grid-stride loops, the contended
classes, the direct global path of the builder's counters and the long runs that tests/test_gpu_colors_scale.py is there
for.  Every condition is one on the committed draws; the figures are printed."""
import functools

import numpy as np
import pytest

import bench
import colors_scale_ref as R
import colorsets_brute as cb
import pseudoalign_brute as pb
import pseudoalign_wide as pw
from sbwt_amd import hostlib

NT = max(1, min(16, bench.effective_cores()))


def arrays_of(seqs):
    return [np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), dtype=np.uint8) for s in seqs]


@functools.lru_cache(maxsize=None)
def small_index(rc):
    """The shared pan-genome's index (its sequences do not depend on n_colors), both oracles, its labels and k-mers."""
    case = pw.Case(1, rc)
    bits = hostlib.build_bits([s.encode() for s in case.seqs], case.k, rc, True)
    orc, strict = R.oracles(bits, case.k)
    labels = [orc.get_kmer(j).decode() for j in range(bits.n_nodes)]
    return bits.n_nodes, strict, labels, case.index_kmers()


# ---- 1. the numpy reference against the brute forces -------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
@pytest.mark.parametrize("n_colors", [1, 64, 65, 200])
def test_reference_equals_the_brute_forces(n_colors, rc):
    n, strict, labels, kmers = small_index(rc)
    case = pw.Case(n_colors, rc)
    k, words = case.k, pw.n_words(n_colors)
    place = sorted(case.inputs)
    both = case.strands_add == 2
    # the add calls: window counts, and the keys they leave
    cs = [set() for _ in range(n_colors)]
    marks = []
    for i, c in enumerate(place):
        m, counts = R.mark(n, R.search(strict, *R.concat(arrays_of(case.inputs[c])), both, NT))
        assert counts == pb.add(cs, kmers, k, c, case.inputs[c], case.strands_add), c
        marks.append((i, m))
    keys = R.fill_keys(n, marks)
    want_matrix = pw.rows_array(pb.rows_of(labels, cs, kmers), words)
    assert np.array_equal(R.matrix(keys, place, n_colors), want_matrix)
    ids, table = R.canonical(keys, place, n_colors)
    want_ids, want_table = cb.canonical_arrays(want_matrix)
    assert ids.dtype == want_ids.dtype == np.uint32 and table.dtype == want_table.dtype == np.uint64
    assert np.array_equal(ids, want_ids) and np.array_equal(table, want_table)
    cb.check_invariants(ids.tolist(), pw.rows_ints(table), n_colors, ["$" in lab for lab in labels])
    assert R.per_color(keys, place, n_colors) == [len(x) for x in cs]
    assert R.n_colored_columns(keys) == int(want_matrix.any(axis=1).sum()) and R.n_sets(keys) == len(want_table)
    # a colouring that stops after the first colours: the keys restricted to them
    some = list(range((len(place) + 1) // 2))
    part = [cs[c] if c in [place[i] for i in some] else set() for c in range(n_colors)]
    part_matrix = pw.rows_array(pb.rows_of(labels, part, kmers), words)
    assert np.array_equal(R.matrix(R.restrict(keys, some), place, n_colors), part_matrix)
    assert R.n_sets(R.restrict(keys, some)) == len(cb.canonical_arrays(part_matrix)[1])
    # records, colour words and counts of the three queries, one and two strands
    exp = pw.Expected(cs, kmers, k)
    reads = case.reads()
    bases, off = R.concat(arrays_of(reads))
    for strands in (1, 2):
        sets = [exp.window_sets(r, strands) for r in reads]
        rcounts = R.read_counts(keys, R.search(strict, bases, off, strands == 2, NT), len(place))
        want_counts = np.array([exp.counts_of(s) for s in sets], dtype=np.int32).reshape(len(reads), n_colors)
        for ppm, den in R.QUERIES:
            rec, colors, cnt = R.expected(rcounts, place, n_colors, ppm, den, counts=True)
            assert rec.dtype == R.READ_FOUND_DTYPE and colors.dtype == np.uint64 and colors.shape == (len(reads), words)
            got = [(pw.words_to_row(c), int(r["n_kmers"]), int(r["n_found"])) for r, c in zip(rec, colors.tolist())]
            want = [exp.record_of(s, ppm, den) for s in sets]
            bad = [i for i in range(len(reads)) if got[i] != want[i]]
            assert not bad, (strands, ppm, den, reads[bad[0]][:80], got[bad[0]], want[bad[0]])
            assert cnt.dtype == np.int32 and np.array_equal(cnt, want_counts)
            if n_colors <= 64:
                narrow, ncnt = R.expected(rcounts, place, n_colors, ppm, den, narrow=True, counts=True)
                assert narrow.dtype == R.PSEUDOALIGNMENT_DTYPE and np.array_equal(ncnt, want_counts)
                assert [(int(x["colors"]), int(x["n_kmers"]), int(x["n_found"])) for x in narrow] == want
    assert any(w[0] >> 64 for w in want) or n_colors <= 64            # (some read carries a colour beyond the first word)


def test_placement():
    for n_colors, must in ((64, (0, 63)), (65, (0, 63, 64)), (130, (0, 63, 64, 127, 128, 129)),
                           (4096, (0, 63, 64, 2047, 2048, 4032, 4095))):
        place = R.placement(n_colors)
        assert len(place) == R.N_USED and place == sorted(set(place)) and place[-1] < n_colors
        assert set(must) <= set(place)


# ---- 2. the scale world is not vacuous ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scale():
    world = R.ScaleWorld()
    bits = hostlib.build_bits(world.index_seqs(), R.K, False, True, NT)
    orc, strict = R.oracles(bits, R.K)
    return bits, R.Reference(world, orc, strict, NT)


def test_scale_world_columns_and_sets(scale):
    bits, ref = scale
    n = bits.n_nodes
    ids, table = ref.canonical(64)
    per_set = np.bincount(ids, minlength=len(table))
    n_dummy = int(ref.dummy.sum())
    far = int((per_set[1024:] >= 64).sum())
    print("\nscale world: n_nodes %d, n_sets %d (x 64 words = %d), sets of >= 64 columns %d (of them with id >= 1024: %d), "
          "largest class %d columns, classes of one column %d, dummy columns %d (%d from column 2^21 on)"
          % (n, len(table), len(table) * 64, int((per_set[1:] >= 64).sum()), far, int(per_set[1:].max()),
             int((per_set == 1).sum()), n_dummy, int(ref.dummy[1 << 21:].sum())))
    assert n > (1 << 21) + (1 << 18)                                  # every grid-stride loop over columns goes round again
    assert len(table) * 64 > (1 << 21)                                # ... and those over the table's words at 4096 colours
    assert far > 1000                                                 # the builder's direct global path under contention
    assert per_set[1:].max() > 100_000                                # the atomicMin of one class
    assert (per_set == 1).sum() > 1000
    assert n_dummy > 0 and n_dummy == n - bits.n_kmers                # the columns without a colour are the dummy columns
    assert ref.dummy[:1 << 21].any() and ref.dummy[1 << 21:].any()    # dirt on dummy columns on both sides of 2^21
    assert len(table) == ref.n_sets_of(range(R.N_USED)) == R.n_sets(ref.keys)
    assert ref.n_colored_of(range(R.N_USED)) == n - n_dummy
    # the add calls
    windows = [c[0] for c in ref.add_counts]
    print("add calls (n_windows, n_hit_windows):", ref.add_counts)
    assert windows[7] > (1 << 21)                                     # k_col_mark and k_csb_mark go round again
    assert all(h == w for w, h in ref.add_counts)                     # (every window given is a k-mer of the index)
    assert ref.calls[3].both and not any(c.both for c in ref.calls if c.used != 3)
    # colour 3 came in by the second strand alone: its columns are those of sequence 3 all the same
    fwd = R.mark(n, R.search(ref.orc, *R.concat([ref.world.genomes[3]]), False, NT))[0]
    assert np.array_equal(fwd, ((ref.keys >> np.uint64(3)) & np.uint64(1)).astype(bool))


def test_scale_world_read_batches(scale):
    bits, ref = scale
    r = ref.results("main", False)
    rows = R.window_rows(ref.keys, r)
    n_reads = len(r.off) - 1
    run, most = R.longest_run(rows, r.off), R.most_keys_in_an_iteration(rows, r.off)
    longest = int(np.diff(r.off).max())
    print("\nmain batch: %d reads, %d windows (%.1f %% found), longest read %d windows, longest run of one key %d windows, "
          "most distinct keys in an iteration %d" % (n_reads, len(rows), 100 * (rows != 0).mean(), longest, run, most))
    assert n_reads == 120_004 and longest >= 999_970
    assert run > 10_000 and most >= 8
    bases, off = ref.batch("main")
    for ch in (ord("N"), ord("a"), 0, 0xFF):
        assert (bases == ch).sum() > 1000
    tb, to = ref.batch("tiny")
    lens = np.diff(to)
    print("tiny batch: %d reads of %d to %d bases" % (len(lens), lens.min(), lens.max()))
    assert len(lens) > (1 << 22) and lens.min() == 31 and lens.max() == 33
