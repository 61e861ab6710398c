"""CPU: the definition of the coloured merge (tests/colorsets_merge_brute.py) on hand-written cases with the expected ids and
tables spelled out, its word-level shifted OR against Python's big-integer shifts, the binding and the CLI's usage text."""
import os
import random
import subprocess

import numpy as np
import pytest

import colorsets_brute as cb
import colorsets_merge_brute as mb
import pseudoalign_wide as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")

# a and b at k = 3; u's columns in colex order, with two dummy columns
A = {"AAC": 0b01, "ACG": 0b11, "CGT": 0b10, "GTA": 0}           # two colours; GTA is a k-mer of a without a colour
B = {"ACG": 0b1, "CGT": 0b1, "TTT": 0b1}                         # one colour
U = ["$", "GTA", "AAC", "$A", "ACG", "CGT", "TTT"]               # the union
DUMMY = ["$" in x for x in U]


def test_union_with_concatenated_colour_spaces():
    ids, table = mb.merge(U, DUMMY, A, B, 2)
    #                $  GTA AAC $A ACG      CGT      TTT
    assert ids == [0, 0, 1, 0, 2, 3, 4]
    assert table == [0, 0b001, 0b111, 0b110, 0b100]
    assert mb.n_colors_out(2, 1, 2) == 3
    assert mb.counts(U, DUMMY, {"AAC": 1, "ACG": 2, "CGT": 3, "GTA": 0}, {"ACG": 1, "CGT": 1, "TTT": 1}) == \
        {"n_real_u": 5, "n_from_a": 4, "n_from_b": 3, "n_from_both": 2, "n_pairs": 4}


def test_union_with_a_shared_colour_space():
    ids, table = mb.merge(U, DUMMY, A, B, 0)
    # AAC 01, ACG 11 | 1 = 11, CGT 10 | 1 = 11, TTT 1: ACG and CGT meet in one row, and so do AAC and TTT
    assert ids == [0, 0, 1, 0, 2, 2, 1]
    assert table == [0, 0b01, 0b11]
    assert mb.n_colors_out(2, 1, 0) == 2


def test_two_pairs_give_one_row():
    # offset 1: (id of 10, id of nothing) and (nothing, id of 1) and (10, 1) all give 10
    a = {"AAC": 0b10, "ACG": 0b10}
    b = {"ACG": 0b1, "CGT": 0b1}
    ids, table = mb.merge(U, DUMMY, a, b, 1)
    assert ids == [0, 0, 1, 0, 1, 1, 0] and table == [0, 0b10]
    got = mb.counts(U, DUMMY, {"AAC": 1, "ACG": 1}, {"ACG": 1, "CGT": 1})
    assert got["n_pairs"] == 3 > len(table) - 1


def test_restriction_to_an_intersection():
    u = ["$", "$A", "ACG", "CGT"]
    ids, table = mb.merge(u, [True, True, False, False], A, B, 2)
    assert ids == [0, 0, 1, 2] and table == [0, 0b111, 0b110]


def test_without_b():
    ids, table = mb.merge(U, DUMMY, A, None, 0)
    assert ids == [0, 0, 1, 0, 2, 3, 0] and table == [0, 0b01, 0b11, 0b10]
    assert mb.n_colors_out(2, None, 0) == 2
    assert mb.counts(U, DUMMY, {"AAC": 1, "ACG": 2, "CGT": 3, "GTA": 0}, None)["n_from_b"] == 0


def test_an_unrelated_u():
    u = ["$", "$G", "GGG"]
    ids, table = mb.merge(u, [True, True, False], A, B, 2)
    assert ids == [0, 0, 0] and table == [0]
    assert mb.counts(u, [True, True, False], {"AAC": 1}, {"ACG": 1}) == \
        {"n_real_u": 1, "n_from_a": 0, "n_from_b": 0, "n_from_both": 0, "n_pairs": 0}


def test_a_dummy_column_never_takes_a_colour():
    # a label that happens to be coloured does not colour a column flagged as a dummy
    ids, table = mb.merge(["AAC", "AAC"], [True, False], A, None, 0)
    assert ids == [0, 1] and table == [0, 1]


@pytest.mark.parametrize("n_b", [1, 63, 64, 65])
@pytest.mark.parametrize("offset", [0, 1, 63, 64, 65, 127, 128, 4032, 4095])
def test_the_word_level_shift_is_the_integer_shift(offset, n_b):
    if offset + n_b > mb.MAX_COLORS:
        n_b = mb.MAX_COLORS - offset              # (the widest b that this offset admits: 64 at 4032, 1 at 4095)
    rng = random.Random(offset * 100 + n_b)
    rows_b = [0, 1, 1 << (n_b - 1), (1 << n_b) - 1] + [rng.getrandbits(n_b) for _ in range(20)]
    n_a = rng.choice([1, 64, 65, 200])
    rows_a = [0] + [rng.getrandbits(n_a) | 1 for _ in range(5)]
    n_out = mb.n_colors_out(n_a, n_b, offset)
    w_out = pw.n_words(n_out)
    tb = pw.rows_array(rows_b, pw.n_words(n_b))
    got = mb.shift_rows(tb, offset, w_out)
    assert got.dtype == np.uint64 and got.shape == (len(rows_b), w_out)
    assert pw.rows_ints(got) == [r << offset for r in rows_b]
    ta = pw.rows_array(rows_a, pw.n_words(n_a))
    pairs = [(i, j) for i in range(len(rows_a)) for j in range(len(rows_b))]
    assert pw.rows_ints(mb.pair_rows(ta, tb, pairs, offset, w_out)) == [rows_a[i] | (rows_b[j] << offset) for i, j in pairs]
    assert pw.rows_ints(mb.pair_rows(ta, None, pairs, 0, pw.n_words(n_a))) == [rows_a[i] for i, _ in pairs]


def test_merge_arrays_are_the_canonical_arrays():
    ids, table = mb.merge_arrays(U, DUMMY, A, B, 70, 71)
    assert ids.dtype == np.uint32 and table.dtype == np.uint64 and table.shape == (5, 2)
    assert pw.rows_ints(table) == [0, 1, 3 | (1 << 70), 2 | (1 << 70), 1 << 70]
    cb.check_invariants(ids.tolist(), pw.rows_ints(table), 71, DUMMY)


def test_the_usage_text_names_merge_colors():
    p = subprocess.run([SBWT], capture_output=True, timeout=60)                                     # (no GPU is opened before it)
    assert b"merge-colors" in p.stdout + p.stderr
    p = subprocess.run([SBWT, "merge-colors", "--help"], capture_output=True, timeout=60)
    text = p.stdout + p.stderr
    for word in (b"--index-u", b"--colors-a", b"--colors-b", b"--color-offset", b"--out-file"):
        assert word in text, word


def test_the_binding_lists_the_merge_call():
    from sbwt_amd import capi
    assert "sbwtgpu_colorsets_merge" in capi.EXPORTED_SYMBOLS and hasattr(capi.lib(), "sbwtgpu_colorsets_merge")
    assert callable(capi.ColorSets.merge)
    assert [f for f, _ in capi.ColorsetsMergeInfoC._fields_] == ["n_real_u", "n_from_a", "n_from_b", "n_from_both", "n_pairs", "n_sets",
                                                                 "pass_ms"]
