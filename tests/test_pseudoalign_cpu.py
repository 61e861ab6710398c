"""CPU: the pure-Python definition of colours and pseudoalignment (tests/pseudoalign_brute.py) on hand-written cases, the
colour file format of libsbwthost, the threshold parser, and the declarations of include/sbwtgpu.h."""
import os
import re
import struct

import numpy as np
import pytest

import pseudoalign_brute as pb
from sbwt_amd import capi, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 3


def two_colours():
    """index {ACG, CGT, GTA, TTT, GGG}; colour 0 = ACGT's k-mers, colour 1 = CGTA's: CGT is shared, GGG has no colour"""
    index = {"ACG", "CGT", "GTA", "TTT", "GGG"}
    cs = [set(), set()]
    assert pb.add(cs, index, K, 0, ["ACGT"]) == (2, 2)
    assert pb.add(cs, index, K, 1, ["CGTA", "CCC"]) == (3, 2)          # CCC is a window the index lacks
    return index, cs


def test_two_colours_sharing_a_kmer():
    index, cs = two_colours()
    assert cs == [{"ACG", "CGT"}, {"CGT", "GTA"}]
    labels = ["$$$", "$$A", "ACG", "GGG", "GTA", "CGT", "TTT"]
    assert pb.rows_of(labels, cs, index) == [0, 0, 1, 0, 2, 3, 0]
    assert pb.window_sets(cs, index, K, "ACGTA") == [1, 3, 2]
    assert pb.counts(cs, index, K, ["ACGTA"]) == [[2, 2]]
    # intersection over the found k-mers: no colour holds all three
    assert pb.records(cs, index, K, ["ACGTA"]) == [(0, 3, 3)]
    assert pb.records(cs, index, K, ["ACGT", "CGTA", "CGT"]) == [(1, 2, 2), (2, 2, 2), (3, 1, 1)]


def test_split_two_to_one_at_the_threshold_edges():
    index = {"AAA", "AAC", "ACC"}
    cs = [{"AAA", "AAC"}, {"ACC"}]
    read = "AAACC"                                   # windows AAA, AAC, ACC: colour 0 has 2 of 3, colour 1 has 1 of 3
    assert pb.counts(cs, index, K, [read]) == [[2, 1]]
    want = {666_666: 1, 666_667: 0, 500_000: 1, 1: 3, 333_333: 3, 333_334: 1}
    for ppm, colors in want.items():
        assert pb.records(cs, index, K, [read], threshold_ppm=ppm) == [(colors, 3, 3)], ppm


def test_denominators_with_a_miss_in_the_read():
    index = {"AAA", "AAC"}
    cs = [{"AAA", "AAC"}]
    read = "AAACG"                                   # AAA, AAC found; ACG is a miss
    assert pb.records(cs, index, K, [read], denominator=0) == [(1, 3, 2)]
    assert pb.records(cs, index, K, [read], denominator=1) == [(0, 3, 2)]
    assert pb.records(cs, index, K, [read], threshold_ppm=666_666, denominator=1) == [(1, 3, 2)]
    assert pb.records(cs, index, K, [read], threshold_ppm=666_667, denominator=1) == [(0, 3, 2)]


def test_nothing_found_and_no_window():
    index, cs = two_colours()
    for den in (0, 1):
        for ppm in (1, 1_000_000):
            assert pb.records(cs, index, K, ["CCCCC", "AC", "", "ACNGT", "acgt"], 1, ppm, den) == \
                [(0, 3, 0), (0, 0, 0), (0, 0, 0), (0, 3, 0), (0, 2, 0)]
    assert pb.counts(cs, index, K, ["", "AC"]) == [[0, 0], [0, 0]]


def test_both_strands_where_only_the_reverse_complement_is_indexed():
    index = {"AAC"}
    cs = [set()]
    assert pb.add(cs, index, K, 0, ["GTT"], strands=1) == (1, 0) and cs == [set()]
    assert pb.add(cs, index, K, 0, ["GTT"], strands=2) == (1, 1) and cs == [{"AAC"}]
    assert pb.records(cs, index, K, ["GTT"], strands=1) == [(0, 1, 0)]
    assert pb.records(cs, index, K, ["GTT"], strands=2) == [(1, 1, 1)]
    # a window counts once when both strands hit
    index2 = {"AAC", "GTT"}
    cs2 = [set()]
    assert pb.add(cs2, index2, K, 0, ["GTT"], strands=2) == (1, 1) and cs2 == [{"AAC", "GTT"}]
    # N is no base on either strand
    assert pb.records(cs, index, K, ["GNT"], strands=2) == [(0, 1, 0)]


def test_found_but_uncoloured_counts_as_a_miss():
    index, cs = two_colours()
    read = "ACGGG"                                   # ACG (colour 0), CGG (absent), GGG (indexed, no colour)
    assert pb.window_sets(cs, index, K, read) == [1, 0, 0]
    assert pb.records(cs, index, K, [read]) == [(1, 3, 1)]
    assert pb.records(cs, index, K, ["GGG"]) == [(0, 1, 0)]


def test_format_lines():
    assert pb.format_lines([(0, 1, 0), (5, 2, 2), (1 << 63, 1, 1), (3, 1, 1)]) == b"0\n1 0 2\n2 63\n3 0 1\n"
    assert pb.format_lines([]) == b""


def test_ppm_parser():
    assert pb.parse_ppm("1") == 1_000_000
    assert pb.parse_ppm("1.0") == 1_000_000
    assert pb.parse_ppm("0.7") == 700_000
    assert pb.parse_ppm("0.000001") == 1
    assert pb.parse_ppm("0.5000000") == 500_000
    for bad in ("0", "1.0000001", "abc", "", "0.0", "2", "-0.5", "0.0000001", ".5", "1e-3", "0.7 "):
        with pytest.raises(ValueError):
            pb.parse_ppm(bad)


def test_colour_file_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    for n, nc, k in ((1, 1, 2), (77, 3, 31), (1000, 64, 255), (0, 5, 4)):
        rows = rng.integers(0, 2**64, size=n, dtype=np.uint64)
        p = str(tmp_path / ("c%d.colors" % n))
        hostlib.colors_write(p, rows, nc, k)
        raw = open(p, "rb").read()
        assert raw[:8] == b"SBWTCOL1" and struct.unpack("<3q", raw[8:32]) == (n, nc, k)
        assert raw[32:] == rows.astype("<u8").tobytes()
        got, gnc, gk = hostlib.colors_read(p)
        assert got.dtype == np.uint64 and np.array_equal(got, rows) and (gnc, gk) == (nc, k)


def test_malformed_colour_files(tmp_path):
    rows = np.arange(10, dtype=np.uint64)
    good = str(tmp_path / "good.colors")
    hostlib.colors_write(good, rows, 4, 5)
    raw = open(good, "rb").read()

    def err_of(data, name):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        with pytest.raises(RuntimeError) as ei:
            hostlib.colors_read(p)
        return str(ei.value)
    assert "truncated" in err_of(raw[:-1], "short_rows")
    assert "truncated" in err_of(raw[:20], "short_header")
    assert "truncated" in err_of(raw[:5], "short_magic")
    assert "truncated" in err_of(b"", "empty")
    assert "magic" in err_of(b"SBWTCOL2" + raw[8:], "magic")
    assert "n_colors" in err_of(raw[:8] + struct.pack("<3q", 10, 65, 5) + raw[32:], "colors65")
    assert "n_colors" in err_of(raw[:8] + struct.pack("<3q", 10, 0, 5) + raw[32:], "colors0")
    assert "after" in err_of(raw + b"\0", "long")
    with pytest.raises(RuntimeError) as ei:
        hostlib.colors_read(str(tmp_path / "missing.colors"))
    assert "opening" in str(ei.value)
    for nc in (0, 65):
        with pytest.raises(RuntimeError) as ei:
            hostlib.colors_write(str(tmp_path / "w.colors"), rows, nc, 5)
        assert "n_colors" in str(ei.value)


def test_header_declares_the_colour_layer():
    text = open(os.path.join(ROOT, "include", "sbwtgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("sbwtgpu_colors_create", "sbwtgpu_colors_destroy", "sbwtgpu_colors_add_batch", "sbwtgpu_colors_info",
                 "sbwtgpu_colors_copy", "sbwtgpu_colors_dev", "sbwtgpu_pseudoalign_batch", "sbwtgpu_pseudoalign_workspace_bytes",
                 "sbwtgpu_pseudoalign_dev"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in capi.EXPORTED_SYMBOLS and hasattr(capi.lib(), name), name
    for t in ("sbwtgpu_colors_info_t", "sbwtgpu_pseudoalignment", "typedef struct sbwtgpu_colors sbwtgpu_colors"):
        assert t in code, t
    # the contract's text is part of the header
    for phrase in ("Colour matrix", "threshold_ppm", "idempotent", "must not run concurrently"):
        assert phrase in text, phrase
    assert capi.PSEUDOALIGNMENT_DTYPE.itemsize == 16
    # pure arithmetic, no GPU: the workspace grows with both arguments and holds the search workspace
    prev = -1
    for b in (0, 1, 1000, 1 << 20, (1 << 26) + 3, 1 << 30):
        w1, w2 = capi.pseudoalign_workspace_bytes(b, 1000), capi.pseudoalign_workspace_bytes(b, 1000, True)
        assert w2 > w1 >= capi.search_workspace_bytes(b) and w1 >= prev
        prev = w1
