"""GPU: the colour layer (sbwt_colors.hip, sbwt_colorsets.hip) at 2.57 million columns against its definition in numpy
(tests/colors_scale_ref.py, whose search results are the oracle's): the colour matrix narrow and wide, compress, the checks
of an uploaded object, the builder after every close, and the three reducers on every read of 120 004 reads (three of a
million bases, one of a single run of 375 000 windows) and of 4.3 million tiny reads.  The small worlds of the other colour
tests have fewer than 4 000 columns; here every grid-stride loop of the two sources goes round a second time (8192 x 256
lanes over 2 571 877 columns, 2048 or 8192 blocks over the builder's 40 186 bitmap words and the table's 2.7 million words
at 4096 colours, 16 384 x 4 waves over the columns in k_cs_insert_wave, 2^20 x 4 waves over the reads), classes of 345 693
columns meet in one slot's atomicMin, 3 923 sets with ids from 1024 on carry 64 columns and more, and the builder's table
grows from 64 rows to 65 536.  tests/test_colors_scale_ref_cpu.py holds the reference against the brute forces and asserts
those properties of the world.  All comparisons are exact.

The world: n_nodes = 2 571 877, n_sets = 42 386, 36 dummy columns, 20 used colours placed among 64, 65, 130 or 4096.
Seconds on an MI355X (the module's fixture -- index build on the GPU, both oracles, the keys -- 0.9 s; the expected
values of a batch are made by the first test that needs them and are in its time):
  matrix 64 / 130: 0.07 / 0.09      the 4096-colour matrix through info: 0.06      compress 64 / 130 / 4096: 0.15 / 0.19 / 0.17
  upload checks: 3.4 (of it about 3 s the oracle's strict search of the main batch on both strands)
  builder 130 / 4096, ascending and shuffled: 0.07 - 0.08 each
  main batch Colors-64 / WideColors-130 / ColorSets-130 / ColorSets-4096: 0.48 / 0.63 / 0.41 / 0.54
  more than 2^22 reads Colors-64 with counts / WideColors-65 / ColorSets-65: 4.3 (two arrays of 1.1 GB are made and compared) / 0.54 / 0.53
  chunking: 0.16                    the module: 13.4
"""
import random

import numpy as np
import pytest

import bench
import colors_scale_ref as R
import colorsets_stream_model as sm
from sbwt_amd import capi
from test_gpu_ms_scale import assert_same
from test_gpu_pseudoalign_wide import tuning

pytestmark = pytest.mark.gpu

NT = max(1, min(16, bench.effective_cores()))
TRIP = 1 << 21                      # columns, words or windows that 8192 blocks of 256 lanes take in one trip
READS_TRIP = 1 << 22                # reads that the reducers' 2^20 blocks of four waves take in one trip
QUERIES = R.QUERIES


class Scale:
    """The index on the device, the reference, and the coloured objects of every n_colors, made on demand and kept."""

    def __init__(self):
        self.world = R.ScaleWorld()
        bits = capi.build_bits_gpu(self.world.index_seqs(), R.K, False, True)
        self.idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, R.K,
                                     bits.n_kmers, 0)
        self.n = bits.n_nodes
        self.ref = R.Reference(self.world, *R.oracles(bits, R.K), NT)
        assert self.n > TRIP + (1 << 18) and int(self.ref.dummy.sum()) == self.n - bits.n_kmers
        self.real = np.flatnonzero(~self.ref.dummy)
        self.made = {}

    def coloured(self, cls, n_colors):
        """A Colors / WideColors object coloured by the add calls; every call returns the reference's counts."""
        key = (cls.__name__, n_colors)
        if key not in self.made:
            place = R.placement(n_colors)
            col = cls.create(self.idx, n_colors)
            self.made[key] = col
            for c, want in zip(self.ref.calls, self.ref.add_counts):
                assert col.add_sequences(place[c.used], c.bases, c.off, c.both) == want, (key, c.used)
        return self.made[key]

    def compressed(self, n_colors):
        key = ("ColorSets", n_colors)
        if key not in self.made:
            self.made[key] = capi.ColorSets.from_colors(self.coloured(capi.WideColors, n_colors))
        return self.made[key]

    def built(self, n_colors):
        """The colour-set object of the builder run in ascending order (checked after every close)."""
        key = ("built", n_colors)
        if key not in self.made:
            self.made[key] = run_builder(self, n_colors, list(range(R.N_USED)))
        return self.made[key]

    def close(self):
        for obj in self.made.values():
            obj.close()
        self.idx.close()


@pytest.fixture(scope="module")
def scale(gpu):
    s = Scale()
    yield s
    s.close()


def same(got, want, label, second_trip=None):
    """Equal dtype, shape and elements, field by field for records; the first differing slot in the message.  second_trip:
    the first read that only a second trip of the reducer's grid reaches -- those reads are compared and named apart."""
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, want.dtype, got.shape, want.shape)
    for name in got.dtype.names or (None,):
        g, w = (got, want) if name is None else (got[name], want[name])
        if second_trip is None:
            assert_same(g.ravel(), w.ravel(), (label, name))
        else:
            assert_same(g[:second_trip].ravel(), w[:second_trip].ravel(), (label, name, "reads of the first trip"))
            assert_same(g[second_trip:].ravel(), w[second_trip:].ravel(),
                        (label, name, "reads %d .. %d, which only the second trip of the grid reaches" % (second_trip, len(g) - 1)))


def check_info(info, scale, n_colors, used=range(R.N_USED)):
    place = R.placement(n_colors)
    assert (info["n_columns"], info["k"], info["n_colors"]) == (scale.n, R.K, n_colors)
    assert info["n_colored_columns"] == scale.ref.n_colored_of(used)
    if "per_color" in info:
        assert info["per_color"] == scale.ref.per_color_of(used, place, n_colors)


def check_batch(obj, scale, name, n_colors, narrow=False, strands=(1, 2), queries=QUERIES, counts=True, reads=None, second_trip=None):
    """Every read's record, colour words and counts against the reference.  reads: the first so many reads only."""
    bases, off = scale.ref.batch(name)
    n = len(off) - 1 if reads is None else reads
    bases, off = bases[:off[n]], off[:n + 1]
    place = R.placement(n_colors)
    for st in strands:
        rcounts = R.part(scale.ref.counts(name, st == 2), 0, n)
        for ppm, den in queries:
            got = obj.pseudoalign(bases, off, st == 2, ppm, den, counts=counts)
            want = R.expected(rcounts, place, n_colors, ppm, den, narrow=narrow, counts=counts)
            got, want = (got if isinstance(got, tuple) else (got,)), (want if isinstance(want, tuple) else (want,))
            assert len(got) == len(want)
            for what, g, w in zip(("records", "colour words", "counts") if not narrow else ("records", "counts"), got, want):
                same(g, w, (type(obj).__name__, n_colors, name, st, ppm, den, what), second_trip)


# ---- 1. the matrix, narrow and wide ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_colors", [64, 130])
def test_matrix_on_every_word_of_every_column(scale, n_colors):
    cls = capi.Colors if n_colors == 64 else capi.WideColors
    col = scale.coloured(cls, n_colors)                  # (every add call's (n_windows, n_hit_windows) is checked in there)
    want = scale.ref.matrix(n_colors)
    if n_colors == 64:
        want = want[:, 0]
    same(col.rows(), want, ("rows", n_colors))
    check_info(col.info(), scale, n_colors)
    # an uploaded matrix comes back clean: bits on dummy columns and bits >= n_colors, on either side of column 2^21
    dummy = np.flatnonzero(scale.ref.dummy)
    assert dummy[0] < TRIP < dummy[-1]
    dirty = want.copy()
    dirty[dummy] = np.uint64(2**64 - 1)
    if n_colors == 130:
        rng = np.random.default_rng(130)
        some = np.concatenate([rng.integers(0, TRIP, 500), rng.integers(TRIP, scale.n, 500), [0, TRIP - 1, TRIP, scale.n - 1]])
        dirty[some, 2] |= rng.integers(1, 2**62, len(some), dtype=np.uint64) << np.uint64(2)
        assert (dirty[some, 2] >> np.uint64(2)).all()
    with cls.from_rows(scale.idx, dirty, n_colors) as up:
        same(up.rows(), want, ("uploaded rows", n_colors))
        assert up.info() == col.info()


def test_wide_matrix_of_4096_colours_through_info(scale):
    col = scale.coloured(capi.WideColors, 4096)          # 1.3 GB on the device; its rows never come to the host
    assert col.words == 64
    check_info(col.info(), scale, 4096)


# ---- 2. compress ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_colors", [64, 130, 4096])
def test_compress_gives_the_canonical_bytes(scale, n_colors):
    col = scale.coloured(capi.Colors if n_colors == 64 else capi.WideColors, n_colors)
    want_ids, want_table = scale.ref.canonical(n_colors)
    assert len(want_table) * R.n_words(n_colors) > TRIP or n_colors != 4096
    s = scale.compressed(n_colors) if n_colors != 64 else capi.ColorSets.from_colors(col)
    ids, table = s.copy()
    same(ids, want_ids, ("ids", n_colors))
    same(table, want_table, ("table", n_colors))
    info = s.info()
    check_info(info, scale, n_colors)
    assert (info["words"], info["n_sets"], info["device_bytes"]) == (R.n_words(n_colors), len(want_table), 4 * scale.n + 8 * want_table.size)
    with capi.ColorSets.from_colors(col) as again:       # compressing twice gives equal bytes
        ids2, table2 = again.copy()
        assert ids2.tobytes() == ids.tobytes() and table2.tobytes() == table.tobytes()
    if n_colors == 130:
        with s.expand() as back:
            same(back.rows(), scale.ref.matrix(130), "expanded rows")
            assert back.info() == col.info()
    if n_colors == 64:
        s.close()


# ---- 3. the checks of an uploaded object ------------------------------------------------------------------------------------
def refused(fn, *needles):
    with pytest.raises(capi.SbwtGpuError) as ei:
        fn()
    assert ei.value.code == capi.ERR_INVALID_ARG, ei.value
    for s in needles:
        assert s in ei.value.msg, (s, ei.value.msg)


def test_upload_checks(scale):
    n_colors = 130
    ids, table = scale.ref.canonical(n_colors)
    n_sets = len(table)
    rng = np.random.default_rng(3)
    # another numbering of the sets, and non-zero ids on the dummy columns: accepted, and it answers like the canonical one
    perm = np.concatenate([[0], 1 + rng.permutation(n_sets - 1)]).astype(np.uint32)
    table2 = np.empty_like(table)
    table2[perm] = table
    ids2 = perm[ids]
    dummy = np.flatnonzero(scale.ref.dummy)
    ids2[dummy] = rng.integers(1, 2**32, len(dummy), dtype=np.uint32)
    with capi.ColorSets.from_arrays(scale.idx, n_colors, ids2, table2, R.K) as up:
        got_ids, got_table = up.copy()
        assert not got_ids[dummy].any()
        same(got_ids[scale.real], ids2[scale.real], "uploaded ids")
        same(got_table, table2, "uploaded table")
        info = up.info()
        check_info(info, scale, n_colors)
        assert info["n_sets"] == n_sets
        with up.expand() as back:
            same(back.rows(), scale.ref.matrix(n_colors), "rows of the permuted object")
        check_batch(up, scale, "main", n_colors, queries=QUERIES[1:2], reads=20_000)
    # ids not below n_sets on either side of column 2^21: the smaller column is named; then the one above alone
    lo, hi = int(scale.real[scale.real < TRIP][-7]), int(scale.real[-3])
    assert lo < TRIP < hi

    def with_ids(*cols):
        out = ids.copy()
        out[list(cols)] = n_sets
        return out
    refused(lambda: capi.ColorSets.from_arrays(scale.idx, n_colors, with_ids(lo, hi), table), "column %d " % lo, "n_sets = %d" % n_sets)
    refused(lambda: capi.ColorSets.from_arrays(scale.idx, n_colors, with_ids(hi), table), "column %d " % hi, "n_sets = %d" % n_sets)
    # the same for two all-zero rows of the table
    r_lo, r_hi = 5, n_sets - 3

    def with_rows(*rows):
        out = table.copy()
        out[list(rows)] = 0
        return out
    refused(lambda: capi.ColorSets.from_arrays(scale.idx, n_colors, ids, with_rows(r_lo, r_hi)), "row %d " % r_lo, "all zero")
    refused(lambda: capi.ColorSets.from_arrays(scale.idx, n_colors, ids, with_rows(r_hi)), "row %d " % r_hi, "all zero")
    with capi.ColorSets.from_arrays(scale.idx, n_colors, ids, table) as ok:          # and the object itself is accepted
        assert ok.n_sets == n_sets


# ---- 4. the builder ---------------------------------------------------------------------------------------------------------
def run_builder(scale, n_colors, order):
    """The add calls in `order`; after every close info() is the reference's of the colours closed so far.  Returns the
    finished object, whose bytes are the reference's."""
    ref, place, words = scale.ref, R.placement(n_colors), R.n_words(n_colors)
    spare = next(c for c in range(n_colors) if c not in place)
    fixed = {"n_columns": scale.n, "k": R.K, "n_colors": n_colors, "words": words}
    cap = sm.FIRST_CAPACITY
    with capi.ColorSetsBuilder.create(scale.idx, n_colors) as b:
        for step in range(len(order) + 1):
            if step < len(order):
                c = ref.calls[order[step]]
                assert b.add_sequences(place[c.used], c.bases, c.off, c.both) == ref.add_counts[c.used], (n_colors, c.used)
            else:
                assert b.add_reads(spare, []) == (0, 0)              # a colour without a sequence closes the last one
            closed = order[:step]
            n_sets = ref.n_sets_of(closed)
            while cap < n_sets:
                cap *= 2
            want = dict(fixed, n_sets=n_sets, n_colored_columns=ref.n_colored_of(closed), per_color=ref.per_color_of(closed, place, n_colors),
                        device_bytes=4 * scale.n + 8 * ((scale.n + 63) // 64) + cap * (8 * words + 4))
            got = b.info()
            assert got == want, (n_colors, step, {k: (got[k], want[k]) for k in got if got[k] != want[k] and k != "per_color"})
        assert cap >= 65_536                                         # the table's capacity doubled ten times
        s = b.finish()
    want_ids, want_table = ref.canonical(n_colors)
    ids, table = s.copy()
    same(ids, want_ids, ("builder ids", n_colors, order))
    same(table, want_table, ("builder table", n_colors, order))
    info = s.info()
    check_info(info, scale, n_colors)
    assert (info["n_sets"], info["device_bytes"]) == (len(want_table), 4 * scale.n + 8 * want_table.size)
    return s


@pytest.mark.parametrize("order", ["ascending", "shuffled"])
@pytest.mark.parametrize("n_colors", [130, 4096])
def test_builder_after_every_close(scale, n_colors, order):
    if order == "ascending":
        scale.built(n_colors)
    else:
        shuffled = list(range(R.N_USED))
        random.Random(5).shuffle(shuffled)
        assert shuffled != sorted(shuffled)
        run_builder(scale, n_colors, shuffled).close()


# ---- 5. pseudoalignment -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["Colors-64", "WideColors-130", "ColorSets-130", "ColorSets-4096"])
def test_main_batch_every_read(scale, kind):
    if kind == "Colors-64":
        check_batch(scale.coloured(capi.Colors, 64), scale, "main", 64, narrow=True)
    elif kind == "WideColors-130":
        check_batch(scale.coloured(capi.WideColors, 130), scale, "main", 130)
    elif kind == "ColorSets-130":
        check_batch(scale.compressed(130), scale, "main", 130)
    else:
        s = scale.built(4096)
        check_batch(s, scale, "main", 4096, counts=False)
        check_batch(s, scale, "main", 4096, reads=2000)            # (counts of every read would be 1.6 GB)


@pytest.mark.parametrize("kind", ["Colors-64", "WideColors-65", "ColorSets-65"])
def test_more_than_2_22_reads(scale, kind):
    bases, off = scale.ref.batch("tiny")
    assert len(off) - 1 > READS_TRIP + 100_000
    with tuning("pseudoalign_chunk_bases", 1 << 30, 0):              # one chunk, so one launch takes every read
        if kind == "Colors-64":
            check_batch(scale.coloured(capi.Colors, 64), scale, "tiny", 64, narrow=True, strands=(1,), queries=QUERIES[1:2],
                        second_trip=READS_TRIP)
        elif kind == "WideColors-65":
            check_batch(scale.coloured(capi.WideColors, 65), scale, "tiny", 65, strands=(1,), queries=QUERIES[:1], counts=False,
                        second_trip=READS_TRIP)
        else:
            check_batch(scale.compressed(65), scale, "tiny", 65, strands=(1,), queries=QUERIES[:1], counts=False,
                        second_trip=READS_TRIP)


def test_chunking_leaves_the_bytes_alone(scale):
    s = scale.compressed(130)
    bases, off = scale.ref.batch("main")
    whole = s.pseudoalign(bases, off, True, 500_000, 1, counts=True)
    with tuning("pseudoalign_chunk_bases", 1 << 20, 0):
        chunked = s.pseudoalign(bases, off, True, 500_000, 1, counts=True)
    for what, g, w in zip(("records", "colour words", "counts"), chunked, whole):
        same(g, w, ("chunks of 2^20 bases", what))
