"""CPU: the colour-set definition of tests/colorsets_brute.py on hand-written cases, and colour-set files ("SBWTCOL3",
include/sbwthost.h): the bytes of a small file, the round trip, every refusal of the reader, and the older readers'
refusal of the new magic."""
import struct

import numpy as np
import pytest

import colorsets_brute as cb
import pseudoalign_wide as pw
from sbwt_amd import hostlib


def refused(fn, *needles):
    with pytest.raises(RuntimeError) as ei:
        fn()
    for s in needles:
        assert s in str(ei.value), (s, str(ei.value))


# ---- the brute ------------------------------------------------------------------------------------------------------
def test_canonical_on_hand_written_cases():
    assert cb.canonical([]) == ([], [0])
    assert cb.canonical([0, 0, 0]) == ([0, 0, 0], [0])                                  # an all-zero matrix: n_sets = 1
    assert cb.canonical([5, 3, 9, 1]) == ([1, 2, 3, 4], [0, 5, 3, 9, 1])                # all rows distinct, in column order
    assert cb.canonical([0, 7, 0, 2, 7, 2, 0, 9]) == ([0, 1, 0, 2, 1, 2, 0, 3], [0, 7, 2, 9])
    # two rows differing only in the last word (bit 4095 against bit 4094) stay two sets
    a, b = 1 | (1 << 4095), 1 | (1 << 4094)
    assert cb.canonical([a, b, a]) == ([1, 2, 1], [0, a, b])
    rng = np.random.default_rng(7)
    for n_colors in (1, 64, 65, 200, 4096):
        words = pw.n_words(n_colors)
        pool = [0] + [int(x) % (1 << n_colors) or 1 for x in rng.integers(1, 2**62, size=5)] + [1 << (n_colors - 1)]
        rows = [pool[i] for i in rng.integers(0, len(pool), size=60)]
        ids, table = cb.canonical(rows)
        assert cb.expand(ids, table) == rows                                           # expand(canonical(M)) == M
        assert len(table) == 1 + len(set(rows) - {0}) and sorted(set(ids)) == list(range(len(table)))[(0 not in rows):]
        cb.check_invariants(ids, table, n_colors)
        ai, at = cb.arrays(ids, table, n_colors)
        assert ai.dtype == np.uint32 and at.dtype == np.uint64 and at.shape == (len(table), words)
        ci, ct = cb.canonical_arrays(pw.rows_array(rows, words))
        assert np.array_equal(ci, ai) and np.array_equal(ct, at)


def test_check_invariants_names_what_is_broken():
    cb.check_invariants([0, 1, 1, 2], [0, 6, 1], 3, [True, False, False, False])
    cb.check_invariants([2, 2, 1], [0, 6, 6, 5], 3)                                      # duplicate and unused rows are allowed
    for ids, table, nc, dummy, needle in (
            ([0, 1], [1, 2], 3, (), "row 0"),
            ([0, 1], [0, 0], 3, (), "all zero"),
            ([0, 1], [0, 8], 3, (), ">= n_colors"),
            ([0, 2], [0, 1], 3, (), "below n_sets"),
            ([1, 1], [0, 1], 3, (True, False), "dummy")):
        with pytest.raises(AssertionError) as ei:
            cb.check_invariants(ids, table, nc, dummy)
        assert needle in str(ei.value)


# ---- colour-set files -----------------------------------------------------------------------------------------------
def test_file_bytes_and_round_trip(tmp_path):
    # 5 columns (an odd number: 4 bytes of padding), 70 colours (2 words), 3 sets
    ids = np.array([0, 1, 2, 1, 0], dtype=np.uint32)
    table = np.array([[0, 0], [5, 0], [1 << 63, 1 << 5]], dtype=np.uint64)
    path = str(tmp_path / "s.colors")
    hostlib.colorsets_write(path, ids, table, 70, 13)
    raw = open(path, "rb").read()
    want = (b"SBWTCOL3" + struct.pack("<5q", 5, 70, 13, 2, 3) + struct.pack("<5I", 0, 1, 2, 1, 0) + b"\0\0\0\0" +
            struct.pack("<6Q", 0, 0, 5, 0, 1 << 63, 1 << 5))
    assert raw == want and len(raw) == 48 + 24 + 48
    gi, gt, nc, k = hostlib.colorsets_read(path)
    assert gi.dtype == np.uint32 and gt.dtype == np.uint64 and np.array_equal(gi, ids) and np.array_equal(gt, table) and (nc, k) == (70, 13)
    rng = np.random.default_rng(1)
    for n_colors in (1, 64, 65, 4096):
        words = pw.n_words(n_colors)
        for n in (0, 1, 36, 37):
            rows = [int(x) for x in rng.integers(0, 4, size=n)]                          # few distinct rows, as in a pan-genome
            rows = [r << (n_colors - 2) if n_colors > 1 else r & 1 for r in rows]
            i, t = cb.arrays(*cb.canonical(rows), n_colors)
            hostlib.colorsets_write(path, i, t, n_colors, 31)
            size = 48 + ((4 * n + 7) // 8) * 8 + 8 * words * len(t)
            assert len(open(path, "rb").read()) == size
            gi, gt, nc, k = hostlib.colorsets_read(path)
            assert np.array_equal(gi, i) and np.array_equal(gt, t) and (nc, k) == (n_colors, 31)
            assert cb.expand(gi.tolist(), pw.rows_ints(gt)) == rows


def test_reader_refusals(tmp_path):
    ids = np.array([0, 1, 2, 1, 0], dtype=np.uint32)
    table = np.array([[0, 0], [5, 0], [1 << 63, 1 << 5]], dtype=np.uint64)
    good = str(tmp_path / "good.colors")
    hostlib.colorsets_write(good, ids, table, 70, 13)
    raw = open(good, "rb").read()
    HEAD, IDS, PAD = 48, 20, 4

    def variant(data):
        p = str(tmp_path / "bad.colors")
        open(p, "wb").write(data)
        return p

    def header(n=5, nc=70, k=13, w=2, ns=3):
        return raw[:8] + struct.pack("<5q", n, nc, k, w, ns)

    # every truncation point class: inside the magic, the header, the ids, the padding, the table; and the empty file
    refused(lambda: hostlib.colorsets_read(variant(b"")), "truncated")
    refused(lambda: hostlib.colorsets_read(variant(raw[:5])), "truncated", "magic")
    refused(lambda: hostlib.colorsets_read(variant(raw[:30])), "truncated", "header")
    refused(lambda: hostlib.colorsets_read(variant(raw[:HEAD + 7])), "truncated")
    refused(lambda: hostlib.colorsets_read(variant(raw[:HEAD + IDS + 2])), "truncated")
    refused(lambda: hostlib.colorsets_read(variant(raw[:HEAD + IDS + PAD + 17])), "truncated")
    refused(lambda: hostlib.colorsets_read(variant(raw[:-1])), "truncated")
    refused(lambda: hostlib.colorsets_read(variant(raw + b"\0")), "after")               # trailing bytes
    refused(lambda: hostlib.colorsets_read(variant(b"SBWTCOL2" + raw[8:])), "magic", "SBWTCOL3")
    refused(lambda: hostlib.colorsets_read(str(tmp_path / "missing.colors")), "opening")
    body = raw[HEAD:]
    # an id >= n_sets
    bad_ids = struct.pack("<5I", 0, 1, 3, 1, 0) + body[IDS:]
    refused(lambda: hostlib.colorsets_read(variant(raw[:HEAD] + bad_ids)), "column 2", "n_sets = 3")
    # a non-zero row 0; a zero row at id != 0; a bit >= n_colors (bit 70 = bit 6 of word 1)
    t0 = IDS + PAD
    refused(lambda: hostlib.colorsets_read(variant(raw[:HEAD] + body[:t0] + struct.pack("<Q", 1) + body[t0 + 8:])), "row 0")
    refused(lambda: hostlib.colorsets_read(variant(raw[:HEAD] + body[:t0 + 16] + struct.pack("<2Q", 0, 0) + body[t0 + 32:])),
            "row 1", "all zero")
    refused(lambda: hostlib.colorsets_read(variant(raw[:HEAD] + body[:t0 + 40] + struct.pack("<Q", 1 << 6))), "row 2", "n_colors = 70")
    # padding that is not zero
    refused(lambda: hostlib.colorsets_read(variant(raw[:HEAD] + body[:IDS] + b"\1\0\0\0" + body[t0:])), "padding")
    # the header's ranges: a wrong W, n_colors 0 and 4097, n_sets 0, a negative or huge n_columns
    for w in (1, 3, 0):
        refused(lambda: hostlib.colorsets_read(variant(header(w=w) + body)), "words_per_row")
    for nc in (0, 4097, -1):
        refused(lambda: hostlib.colorsets_read(variant(header(nc=nc) + body)), "n_colors", "4096")
    for ns in (0, -1, 1 << 32):
        refused(lambda: hostlib.colorsets_read(variant(header(ns=ns) + body)), "n_sets")
    for n in (-1, 1 << 31):
        refused(lambda: hostlib.colorsets_read(variant(header(n=n) + body)), "n_columns")
    # the writer refuses what the reader refuses
    path = str(tmp_path / "x.colors")
    refused(lambda: hostlib.colorsets_write(path, np.array([0, 3], np.uint32), table, 70, 13), "n_sets")
    refused(lambda: hostlib.colorsets_write(path, ids, np.array([[1, 0], [5, 0], [1, 1]], np.uint64), 70, 13), "row 0")
    refused(lambda: hostlib.colorsets_write(path, ids, np.array([[0, 0], [0, 0], [1, 1]], np.uint64), 70, 13), "all zero")
    refused(lambda: hostlib.colorsets_write(path, ids, np.array([[0, 0], [5, 0], [1, 1 << 6]], np.uint64), 70, 13), "n_colors")
    refused(lambda: hostlib.colorsets_write(path, ids, table, 200, 13), "words")
    for nc in (0, 4097):
        refused(lambda: hostlib.colorsets_write(path, ids, table[:, :1], nc, 13), "n_colors")
    # the older readers refuse the new magic as they refuse any unknown one
    refused(lambda: hostlib.colors_read(good), "magic", "SBWTCOL1")
    refused(lambda: hostlib.colors_read_wide(good), "magic", "SBWTCOL1 or SBWTCOL2")
    # ... and after all of that the good file still reads
    gi, gt, nc, k = hostlib.colorsets_read(good)
    assert np.array_equal(gi, ids) and np.array_equal(gt, table) and (nc, k) == (70, 13)


def test_the_binding_lists_the_new_calls():
    from sbwt_amd import capi
    for name in ("sbwtgpu_colorsets_compress", "sbwtgpu_colorsets_create", "sbwtgpu_colorsets_expand", "sbwtgpu_colorsets_destroy",
                 "sbwtgpu_colorsets_info", "sbwtgpu_colorsets_copy", "sbwtgpu_colorsets_dev", "sbwtgpu_pseudoalign_sets_batch",
                 "sbwtgpu_pseudoalign_sets_dev"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(capi.lib(), name), name
    for name in ("from_colors", "from_arrays", "expand", "info", "copy", "pseudoalign", "pseudoalign_reads", "pseudoalign_dev", "close"):
        assert callable(getattr(capi.ColorSets, name)), name
