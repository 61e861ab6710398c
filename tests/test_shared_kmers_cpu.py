"""CPU: the two definitions of the shared k-mer matrix (tests/shared_kmers_brute.py) held against each other and against
hand-written cases: the arrays of a colour-set object on one side, Python sets of k-mer strings (tests/pseudoalign_brute.py)
on the other.  No index structure and no GPU anywhere."""
import os
import random
import subprocess

import numpy as np
import pytest

import colorsets_brute as cb
import pseudoalign_brute as pb
import pseudoalign_wide as pw
import shared_kmers_brute as sk

SBWT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sbwt_amd", "bin", "sbwt")


def world(refs, k, extra=()):
    """An index of the k-mers of refs + extra, coloured by reference: (labels in column order with a dummy column in front,
    index k-mers, per-colour k-mer sets, ids, integer table rows)."""
    kmers = set()
    for s in list(refs) + list(extra):
        kmers |= {w for w in pb.windows(s, k) if pb.valid(w)}
    cs = [set() for _ in refs]
    for c, s in enumerate(refs):
        pb.add(cs, kmers, k, c, [s])
    labels = ["$" * k, "$" + "A" * (k - 1)] + sorted(kmers, key=lambda x: x[::-1])
    ids, table = cb.canonical(pb.rows_of(labels, cs, kmers))
    return labels, kmers, cs, ids, table


def both(refs, k, extra=()):
    labels, kmers, cs, ids, table = world(refs, k, extra)
    G = sk.shared(ids, table, len(refs))
    assert G == sk.shared_of_kmers(cs, kmers)
    arr_ids, arr_table = cb.arrays(ids, table, len(refs))
    assert sk.shared_np(arr_ids, arr_table, len(refs)).tolist() == G
    assert sk.set_sizes(ids, len(table))[0] >= 2 and sum(sk.set_sizes(ids, len(table))) == len(labels)
    return G


def test_two_references_that_share_nothing():
    assert both(["ACGTACGGT", "TTTTTCCCCC"], 4) == [[6, 0], [0, 5]]


def test_two_references_that_share_everything():
    assert both(["ACGTTGCAAT", "ACGTTGCAAT"], 4) == [[7, 7], [7, 7]]


def test_two_references_that_share_half():
    # ACGTTGCA: ACGT CGTT GTTG TTGC TGCA; the second keeps the first three windows and goes elsewhere
    assert both(["ACGTTGCA", "ACGTTGAAA"], 4) == [[5, 3], [3, 6]]


def test_kmers_of_no_reference_count_for_nothing():
    G = both(["ACGTTGCA", "ACGTTGAAA"], 4, extra=["GGGGGGCCCCCC"])
    assert G == [[5, 3], [3, 6]]


def test_a_duplicate_row_and_an_unused_row():
    # canonical: set 1 = {0}, set 2 = {0, 1}; the uploaded form splits set 2 into two equal rows and adds a row nobody carries
    ids = [0, 1, 1, 2, 2, 2, 0]
    table = [0, 0b01, 0b11]
    want = [[5, 3], [3, 3]]
    assert sk.shared(ids, table, 2) == want
    ids2 = [0, 1, 1, 2, 4, 2, 0]
    table2 = [0, 0b01, 0b11, 0b10, 0b11]
    assert sk.set_sizes(ids2, 5) == [2, 2, 2, 0, 1]
    assert sk.shared(ids2, table2, 2) == want
    assert sk.shared_np(*cb.arrays(ids2, table2, 2), 2).tolist() == want
    # a weight on the unused row counts: custom weights are the caller's, not the sizes
    assert sk.shared(ids2, table2, 2, [99, 1, 1, 10, 1]) == [[3, 2], [2, 12]]
    assert sk.shared_np(*cb.arrays(ids2, table2, 2), 2, weights=[99, 1, 1, 10, 1]).tolist() == [[3, 2], [2, 12]]


@pytest.mark.parametrize("n_colors", [1, 7, 64, 65, 130])
def test_python_and_numpy_agree_on_random_objects(n_colors):
    rng = random.Random(n_colors)
    n_sets = 40
    table = [0] + [rng.getrandbits(n_colors) | (1 << rng.randrange(n_colors)) for _ in range(n_sets - 1)]
    ids = [rng.randrange(n_sets) for _ in range(500)]
    arr = cb.arrays(ids, table, n_colors)
    G = sk.shared(ids, table, n_colors)
    assert sk.shared_np(arr[0], arr[1], n_colors).tolist() == G
    assert all(G[a][b] == G[b][a] for a in range(n_colors) for b in range(n_colors))
    w = [rng.choice((0, 1, 127, 128, 2**31 - 1)) for _ in range(n_sets)]
    assert sk.shared_np(arr[0], arr[1], n_colors, weights=w).tolist() == sk.shared(ids, table, n_colors, w)
    assert np.array_equal(sk.bits_of(arr[1], n_colors), np.array([[(r >> c) & 1 for c in range(n_colors)] for r in table]))
    assert pw.rows_ints(arr[1]) == table


def test_jaccard_ppm_and_the_text():
    G = [[5, 3, 0], [3, 6, 0], [0, 0, 0]]          # the third reference has no k-mer in the index: denominators of 0
    J = sk.jaccard_ppm(G)
    assert J == [[1_000_000, 375_000, 0], [375_000, 1_000_000, 0], [0, 0, 0]]
    assert sk.tsv(G) == b"5\t3\t0\n3\t6\t0\n0\t0\t0\n"
    assert sk.tsv(G, jaccard=True) == b"1000000\t375000\t0\n375000\t1000000\t0\n0\t0\t0\n"
    assert sk.jaccard_ppm([[3, 1], [1, 3]]) == [[1_000_000, 200_000], [200_000, 1_000_000]]
    assert sk.jaccard_ppm([[3, 2], [2, 4]])[0][1] == 400_000          # floor(2 * 10^6 / 5)
    big = 2**62                                                       # the products pass 2^64: Python integers do not care
    assert sk.jaccard_ppm([[big, big // 3], [big // 3, big]])[0][1] == (big // 3) * 1_000_000 // (2 * big - big // 3)


def test_the_usage_text_names_color_matrix():
    p = subprocess.run([SBWT], capture_output=True, timeout=60)                                     # (no GPU is opened before it)
    assert b"color-matrix" in p.stdout + p.stderr
    p = subprocess.run([SBWT, "color-matrix", "--help"], capture_output=True, timeout=60)
    text = p.stdout + p.stderr
    for word in (b"--index-file", b"--colors-file", b"--out-file", b"--jaccard-ppm"):
        assert word in text, word
