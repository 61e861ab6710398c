"""CPU: wide colour files ("SBWTCOL2", include/sbwthost.h), the helpers of tests/pseudoalign_wide.py and its trap reads.
The traps are checked with the brute force alone (tests/pseudoalign_brute.py), so that the inputs of
tests/test_gpu_pseudoalign_wide.py cannot quietly lose what they are there for."""
import struct

import numpy as np
import pytest

import pseudoalign_brute as pb
import pseudoalign_wide as pw
from sbwt_amd import hostlib
from sbwt_amd.capi import MAX_COLORS, READ_FOUND_DTYPE, WideColors


def refused(fn, *needles):
    with pytest.raises(RuntimeError) as ei:
        fn()
    for s in needles:
        assert s in str(ei.value), (s, str(ei.value))


# ---- colour files -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_colors", [1, 64, 65, 128, 4096])
def test_wide_file_round_trip(tmp_path, n_colors):
    words = pw.n_words(n_colors)
    assert words == {1: 1, 64: 1, 65: 2, 128: 2, 4096: 64}[n_colors]
    rng = np.random.default_rng(n_colors)
    for n in (0, 1, 37):
        rows = rng.integers(0, 2**64, size=(n, words), dtype=np.uint64)
        path = str(tmp_path / ("c%d.colors" % n))
        hostlib.colors_write_wide(path, rows, n_colors, 31)
        raw = open(path, "rb").read()
        assert raw[:8] == b"SBWTCOL2" and struct.unpack("<4q", raw[8:40]) == (n, n_colors, 31, words)
        assert raw[40:] == rows.astype("<u8").tobytes()
        got, nc, k = hostlib.colors_read_wide(path)
        assert got.dtype == np.uint64 and got.shape == (n, words) and np.array_equal(got, rows) and (nc, k) == (n_colors, 31)
        # the 64-colour reader refuses the wide file, whatever its number of colours
        refused(lambda: hostlib.colors_read(path), "SBWTCOL1")


def test_read_wide_reads_a_64_colour_file(tmp_path):
    rows = np.random.default_rng(3).integers(0, 2**64, size=50, dtype=np.uint64)
    for n_colors in (1, 3, 64):
        path = str(tmp_path / "old.colors")
        hostlib.colors_write(path, rows, n_colors, 9)
        assert open(path, "rb").read(8) == b"SBWTCOL1"
        got, nc, k = hostlib.colors_read_wide(path)
        assert got.shape == (50, 1) and np.array_equal(got[:, 0], rows) and (nc, k) == (n_colors, 9)
        old, nc, k = hostlib.colors_read(path)                    # and the old reader reads what it always read
        assert np.array_equal(old, rows) and (nc, k) == (n_colors, 9)


def test_wide_file_refusals(tmp_path):
    rows = np.arange(10, dtype=np.uint64).reshape(5, 2)
    good = str(tmp_path / "good.colors")
    hostlib.colors_write_wide(good, rows, 100, 7)
    raw = open(good, "rb").read()
    assert len(raw) == 40 + 80

    def variant(data):
        p = str(tmp_path / "bad.colors")
        open(p, "wb").write(data)
        return p

    refused(lambda: hostlib.colors_read_wide(variant(raw[:-1])), "truncated")
    refused(lambda: hostlib.colors_read_wide(variant(raw[:40 + 16])), "truncated")
    refused(lambda: hostlib.colors_read_wide(variant(raw[:20])), "truncated", "header")
    refused(lambda: hostlib.colors_read_wide(variant(raw[:5])), "truncated", "magic")
    refused(lambda: hostlib.colors_read_wide(variant(b"")), "truncated")
    refused(lambda: hostlib.colors_read_wide(variant(raw + b"\0")), "after")
    refused(lambda: hostlib.colors_read_wide(variant(b"SBWTCOL3" + raw[8:])), "magic")
    refused(lambda: hostlib.colors_read_wide(variant(b"plain-ma" + raw[8:])), "magic")
    for nc in (0, 4097, -1):
        refused(lambda: hostlib.colors_read_wide(variant(raw[:8] + struct.pack("<4q", 5, nc, 7, 2) + raw[40:])), "n_colors", "4096")
    for w in (1, 3, 0):
        refused(lambda: hostlib.colors_read_wide(variant(raw[:8] + struct.pack("<4q", 5, 100, 7, w) + raw[40:])), "words_per_row")
    # a 64-colour file keeps its own bound
    refused(lambda: hostlib.colors_read_wide(variant(b"SBWTCOL1" + struct.pack("<3q", 5, 65, 7) + raw[40:80])), "n_colors", "64")
    refused(lambda: hostlib.colors_read_wide(str(tmp_path / "missing.colors")), "opening")
    # writing: n_colors outside 1 .. 4096, rows of another width
    for nc in (0, 4097):
        refused(lambda: hostlib.colors_write_wide(str(tmp_path / "x.colors"), rows, nc, 7), "n_colors")
    refused(lambda: hostlib.colors_write_wide(str(tmp_path / "x.colors"), rows, 200, 7), "words")
    refused(lambda: hostlib.colors_write_wide(str(tmp_path / "x.colors"), rows[:, 0], 100, 7), "words")
    # the existing pair stays as it is: 65 colours are refused, and so is the wide magic
    refused(lambda: hostlib.colors_write(str(tmp_path / "x.colors"), rows[:, 0], 65, 7), "n_colors", "64")
    refused(lambda: hostlib.colors_read(good), "SBWTCOL1")
    got, nc, k = hostlib.colors_read_wide(good)                   # and after all of that the good file still reads
    assert np.array_equal(got, rows) and (nc, k) == (100, 7)


# ---- the helper ---------------------------------------------------------------------------------------------------
def test_word_split_on_hand_written_cases():
    assert pw.row_to_words(0, 1) == [0] and pw.row_to_words(0, 3) == [0, 0, 0]
    assert pw.row_to_words(1, 2) == [1, 0]
    assert pw.row_to_words(1 << 63, 2) == [0x8000000000000000, 0]
    assert pw.row_to_words(1 << 64, 2) == [0, 1]
    assert pw.row_to_words((1 << 70) | (1 << 130) | 5, 3) == [5, 1 << 6, 1 << 2]
    assert pw.row_to_words((1 << 4095) | 1, 64) == [1] + [0] * 62 + [1 << 63]
    assert pw.row_to_words((1 << 128) - 1, 2) == [2**64 - 1, 2**64 - 1]
    with pytest.raises(AssertionError):
        pw.row_to_words(1 << 64, 1)
    for row, words in ((0, 1), (1 << 64, 2), ((1 << 70) | (1 << 130) | 5, 3), ((1 << 4095) | (1 << 64) | 1, 64)):
        assert pw.words_to_row(pw.row_to_words(row, words)) == row
    arr = pw.rows_array([1, 1 << 64, (1 << 127) | 2], 2)
    assert arr.dtype == np.uint64 and arr.tolist() == [[1, 0], [0, 1], [2, 1 << 63]]
    assert pw.rows_ints(arr) == [1, 1 << 64, (1 << 127) | 2]
    assert [pw.n_words(c) for c in (1, 64, 65, 128, 129, 4096)] == [1, 1, 2, 2, 3, 64]
    # the binding's side of the same layout: the cap, the 8-byte record beside the words, one class beside Colors
    assert MAX_COLORS == 4096 == max(pw.N_COLORS) and pw.n_words(MAX_COLORS) == 64
    assert READ_FOUND_DTYPE.itemsize == 8 and READ_FOUND_DTYPE.names == ("n_kmers", "n_found")
    assert all(hasattr(WideColors, name) for name in ("create", "from_rows", "add", "add_reads", "rows", "info", "pseudoalign",
                                                      "pseudoalign_reads", "pseudoalign_dev", "close"))


def test_format_lines_for_any_number_of_colours():
    assert pw.format_lines([0, 1, (1 << 64) | (1 << 3), (1 << 4095) | (1 << 63) | 1]) == b"0\n1 0\n2 3 64\n3 0 63 4095\n"
    # up to 64 colours these are the existing lines
    recs = [(0, 5, 0), (0b101, 5, 5), (1 << 63, 9, 2)]
    assert pw.format_lines([r[0] for r in recs]) == pb.format_lines(recs)


# ---- the cases and their traps, by the brute force alone ----------------------------------------------------------
@pytest.fixture(scope="module", params=[False, True], ids=["fwd", "rc"])
def cases(request):
    out = {}
    for n_colors in pw.N_COLORS:
        case = pw.Case(n_colors, request.param)
        kmers = case.index_kmers()
        cs, _ = case.colour_sets(kmers)
        out[n_colors] = (case, kmers, cs)
    return out


def test_cases_colour_what_they_say(cases):
    for n_colors, (case, kmers, cs) in cases.items():
        given = set(case.inputs)
        assert len(given) <= 12 and {c for c in (0, 63, 64, n_colors - 1) if c < n_colors} <= given
        assert all(bool(cs[c]) for c in (0, 63, 64, n_colors - 1) if c < n_colors)
        assert all(not cs[c] for c in range(n_colors) if c not in given)
        ms = {max(0, len(r) - case.k + 1) for r in case.reads()}
        assert {0, 1, 63, 64, 65, 129} <= ms and max(ms) >= 5000


def test_traps_are_traps(cases):
    for n_colors, (case, kmers, cs) in cases.items():
        k, words = case.k, case.words
        last = n_colors - 1
        traps = (case.trap_equal_word0(), case.trap_last_word_only(), case.trap_two_strands())
        if words == 1:
            assert traps == (None, None, None)
            continue
        # rows that agree in word 0 and differ in the last word, within one wave iteration
        sets = pb.window_sets(cs, kmers, k, traps[0], 1)
        assert len(sets) < 64
        kinds = {s for s in sets if s}
        assert len(kinds) >= 2 and len({s & pw.MASK64 for s in kinds}) == 1 and all(s & pw.MASK64 for s in kinds)
        lasts = {pw.row_to_words(s, words)[-1] for s in kinds}
        assert len(lasts) >= 2
        if n_colors in (127, 128, 200, 4096):                 # the last word holds two colours: both rows are non-zero there
            assert case.last2 == n_colors - 2 and 0 not in lasts
        else:
            assert case.last2 is None and 0 in lasts
        # hits whose rows are zero in word 0 and non-zero in the last word only: they are found
        sets = pb.window_sets(cs, kmers, k, traps[1], 1)
        hit = [s for s in sets if s]
        assert len(hit) == len(sets) > 0
        for s in hit:
            w = pw.row_to_words(s, words)
            assert w[-1] != 0 and not any(w[:-1]), hex(s)
        assert pb.record_of(sets, n_colors, 1_000_000, 0) == (1 << last, len(sets), len(sets))
        # two strands on a reverse-complement index: the forward hit in word 0, the reverse-complement hit in the last word
        if case.rc:
            one = pb.window_sets(cs, kmers, k, traps[2], 1)
            back = pb.window_sets(cs, kmers, k, pb.revcomp(traps[2].decode()), 1)[::-1]
            two = pb.window_sets(cs, kmers, k, traps[2], 2)
            assert all(s == 1 for s in one) and all(s == 1 << last for s in back) and all(s == 1 | (1 << last) for s in two)
        else:
            assert traps[2] is None


def test_expected_agrees_with_the_brute_force(cases):
    """pw.Expected is the brute force rearranged: the same sets, counts and records on reads short enough for the latter."""
    for n_colors, (case, kmers, cs) in cases.items():
        exp = pw.Expected(cs, kmers, case.k)
        reads, budget = [], 300_000 // n_colors            # (the brute force visits every colour of every window)
        for r in sorted(case.reads(), key=len):
            if len(r) <= budget:
                reads.append(r)
                budget -= len(r)
        assert len(reads) >= 8 and any(len(r) >= case.k for r in reads)
        for strands in (1, 2):
            for r in reads:
                sets = exp.window_sets(r, strands)
                assert sets == pb.window_sets(cs, kmers, case.k, r, strands)
                assert exp.counts_of(sets) == pb.counts_of(sets, n_colors)
                for ppm, den in ((1_000_000, 0), (500_000, 1), (1, 0)):
                    assert exp.record_of(sets, ppm, den) == pb.record_of(sets, n_colors, ppm, den)
