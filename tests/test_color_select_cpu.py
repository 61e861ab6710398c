"""CPU: the definition of colour select (tests/color_select_brute.py) checked against itself -- the worked example of the
header, set identities between the families, verdicts on hand-written tables, and a replay of the seeded cases that
tests/test_gpu_color_select.py runs on the GPU, so that their coverage is known without one."""
import numpy as np

import color_select_brute as sb
import pseudoalign_wide as pw
from setop_brute import build_from_kmers, kmers_of, same_bits


def example():
    return sb.colour_world({0: ["AACCG"], 1: ["CCGGTT"]}, [], 3, False, 2)


def test_the_worked_example():
    seqs, kmers, col = example()
    assert kmers == {"AAC", "ACC", "CCG", "CGG", "GGT", "GTT"}
    assert col == {"AAC": frozenset({0}), "ACC": frozenset({0}), "CCG": frozenset({0, 1}), "CGG": frozenset({1}),
                   "GGT": frozenset({1}), "GTT": frozenset({1})}
    assert sb.select(col, [0, 1], None, 2) == {"CCG"}
    assert sb.select(col, [0], [1], 1) == {"AAC", "ACC"}
    assert sb.select(col, [0, 1], None, 1, 1) == {"AAC", "ACC", "CGG", "GGT", "GTT"}
    assert sb.select(col, [0, 1], None, 0, 0) == set()
    assert sb.counts(col, [0, 1], None, 1, 1) == {"n_real": 6, "n_selected": 5, "n_sets_matched": 2, "n_nopred": 2}
    # a min_in above popcount(include) is legal and selects nothing; the result is then the root column alone
    assert sb.select(col, [0], None, 2) == set()
    bits, c = sb.build(col, 3, [0], None, 2)
    assert (bits.n_nodes, bits.n_kmers, c["n_selected"], c["n_sets_matched"]) == (1, 0, 0, 0)
    # everything selected is the index itself
    bits, c = sb.build(col, 3, [0, 1], None, 0)
    assert same_bits(bits, build_from_kmers(kmers, 3)) and c["n_selected"] == 6


def test_core_and_accessory_partition_the_coloured_kmers():
    for k, rc in ((31, False), (32, True), (33, False)):
        k, rc, n_colors, by_color, extra = sb.seeded_world(k, rc)
        seqs, kmers, col = sb.colour_world(by_color, extra, k, rc, n_colors)
        used = sorted(by_color)
        core = sb.select(col, used, None, len(used))
        accessory = sb.select(col, used, None, 1, len(used) - 1)
        coloured = {x for x, cs in col.items() if cs}
        assert core | accessory == coloured and not core & accessory
        assert coloured != kmers                                    # the world has uncoloured k-mers
        assert sb.select(col, used, None, 0, 0) == kmers - coloured


def test_unique_is_set_arithmetic_on_the_colours_kmer_sets():
    for k, rc in ((31, False), (32, True), (63, False)):
        k, rc, n_colors, by_color, extra = sb.seeded_world(k, rc)
        seqs, kmers, col = sb.colour_world(by_color, extra, k, rc, n_colors)
        per_color = {c: {x for x, cs in col.items() if c in cs} for c in by_color}
        for g in by_color:
            others = set().union(*[per_color[c] for c in by_color if c != g])
            got = sb.select(col, [g], [c for c in range(n_colors) if c != g], 1)
            assert got == per_color[g] - others, (k, g)
            # without rc the colours' sets are the sequences' k-mer sets
            if not rc:
                assert per_color[g] == kmers_of(by_color[g], k)


def test_verdicts_on_hand_written_tables():
    # W = 1: bits 0 and 63
    t = pw.rows_array([0, 1, 1 << 63, (1 << 63) | 1, 0b110], 1)
    inc = sb.mask_words([0, 63], 1)
    assert sb.verdicts(t, inc, None, 1, 2).tolist() == [0, 1, 1, 1, 0]
    assert sb.verdicts(t, inc, None, 2, 2).tolist() == [0, 0, 0, 1, 0]
    assert sb.verdicts(t, inc, None, 0, 0).tolist() == [1, 0, 0, 0, 1]
    assert sb.verdicts(t, inc, sb.mask_words([1], 1), 0, 2).tolist() == [1, 1, 1, 1, 0]
    assert sb.verdicts(t, inc, sb.mask_words([63], 1), 1, 1).tolist() == [0, 1, 0, 0, 0]
    # W = 2: bits 63 and 64 sit in different words
    t = pw.rows_array([0, 1 << 63, 1 << 64, (1 << 63) | (1 << 64), 1 << 127], 2)
    inc = sb.mask_words([63, 64], 2)
    assert sb.verdicts(t, inc, None, 1, 1).tolist() == [0, 1, 1, 0, 0]
    assert sb.verdicts(t, inc, None, 2, 2).tolist() == [0, 0, 0, 1, 0]
    assert sb.verdicts(t, sb.mask_words([64, 127], 2), sb.mask_words([63], 2), 1, 2).tolist() == [0, 0, 1, 0, 1]
    # W = 64: bits 0, 63, 64 and 4095; rows that differ in the first or the last word only
    rows = [0, 1, 1 << 4095, 1 | (1 << 4095), (1 << 63) | (1 << 64), (1 << 4096) - 1]
    t = pw.rows_array(rows, 64)
    inc = sb.mask_words([0, 63, 64, 4095], 64)
    assert sb.verdicts(t, inc, None, 1, 1).tolist() == [0, 1, 1, 0, 0, 0]
    assert sb.verdicts(t, inc, None, 2, 4).tolist() == [0, 0, 0, 1, 1, 1]
    assert sb.verdicts(t, inc, None, 4, 4).tolist() == [0, 0, 0, 0, 0, 1]
    assert sb.verdicts(t, inc, sb.mask_words([4095], 64), 0, 4).tolist() == [1, 1, 0, 0, 1, 0]
    assert sb.verdicts(t, sb.mask_words(range(4096), 64), None, 4096, 4096).tolist() == [0, 0, 0, 0, 0, 1]
    # the verdicts are the set definition's
    for row, v in zip(rows, sb.verdicts(t, inc, sb.mask_words([64], 64), 1, 2).tolist()):
        colors = frozenset(c for c in (0, 63, 64, 4095) if (row >> c) & 1) | (frozenset([1]) if (row >> 1) & 1 else frozenset())
        assert bool(v) == sb.matches(colors, [0, 63, 64, 4095], [64], 1, 2)
    assert sb.popcounts(t).tolist() == [0, 1, 1, 2, 2, 4096]


def test_the_seeded_cases_of_the_gpu_test_cover_what_they_should():
    cases = sb.seeded_cases()
    assert len(cases) == len(sb.K_VALUES) * 2 * len(sb.FAMILIES)
    proper, nonempty = 0, {f: 0 for f in sb.FAMILIES}
    worlds = {}
    for label, k, rc, n_colors, by_color, extra, family, (inc, exc, lo, hi) in cases:
        if (k, rc) not in worlds:
            worlds[(k, rc)] = sb.colour_world(by_color, extra, k, rc, n_colors)
        seqs, kmers, col = worlds[(k, rc)]
        c = sb.counts(col, inc, exc, lo, hi)
        assert c["n_real"] == len(kmers)
        proper += 0 < c["n_selected"] < c["n_real"]
        nonempty[family] += c["n_selected"] > 0
    assert 4 * proper >= 3 * len(cases), (proper, len(cases))
    assert all(nonempty.values()), nonempty
    # both key widths, one to three words per row
    assert {pw.n_words(c[3]) for c in cases} == {1, 2, 3}
