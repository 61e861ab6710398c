"""The brute-force restatement of the coloured unitig definition (tests/colored_unitig_brute.py): the worked examples of
DESIGN.md section 18 with their known answers, and the properties of the definition on random coloured k-mer sets."""
import random

import pytest

from bruteforce import BruteSBWT, colex_key, kmer_set
from colored_unitig_brute import (EMPTY, brute_colored_unitigs, colored_paths, colored_unitigs_of_kmers, column_rows, row_of,
                                  sets_of_references)
from unitig_brute import brute_unitigs, unitigs_of_kmers

# (index sequences, references, plain unitigs, coloured unitigs with their sets, breaks): the table of section 18, k = 3
WORKED = [
    (["AACCG", "CCGGTT"], ["AACCG", "CCGGTT"], ["AACCGGTT"], [("AACC", {0}), ("CCG", {0, 1}), ("CGGTT", {1})], 2),
    (["ACGTAC"], ["ACGTAC"], ["GTACGT"], [("GTACGT", {0})], 0),
    (["ACGTAC"], ["ACGTAC", "CGTA"], ["GTACGT"], [("TACG", {0}), ("CGTA", {0, 1})], 2),
    (["ACGTAC"], ["ACGTAC", "GTAC"], ["GTACGT"], [("GTAC", {0, 1}), ("ACGT", {0})], 2),
    (["ACGTAC"], ["ACGTAC", "TACG"], ["GTACGT"], [("TACG", {0, 1}), ("CGTA", {0})], 2),
    (["ACGTAC", "GGG"], ["ACGTAC"], ["GTACGT", "GGG"], [("GTACGT", {0}), ("GGG", set())], 0),
]


def run(index_seqs, refs, k):
    S = kmer_set(index_seqs, k)
    sets = sets_of_references(S, k, [[r] for r in refs])
    return S, sets, colored_unitigs_of_kmers(S, k, sets)


@pytest.mark.parametrize("case", range(len(WORKED)))
def test_worked_examples(case):
    index_seqs, refs, plain, colored, breaks = WORKED[case]
    S, sets, (U, Z, nb) = run(index_seqs, refs, 3)
    assert unitigs_of_kmers(S, 3) == plain
    assert list(zip(U, [set(z) for z in Z])) == colored
    assert nb == breaks


def test_a_piece_crosses_the_old_cut():
    for case in (2, 4):
        assert all("CGTA" not in p for p in WORKED[case][2]) and any(u == "CGTA" for u, _ in WORKED[case][3])


def test_self_loop():
    S, sets, (U, Z, nb) = run(["AAAA"], ["AAAA"], 3)
    assert (U, Z, nb) == (["AAA"], [frozenset({0})], 0)
    S, sets, (U, Z, nb) = run(["AAAA"], [], 3)
    assert (U, Z, nb) == (["AAA"], [EMPTY], 0)


def test_y_branch_with_arms_of_different_colours():
    # TGA -> GAA -> AAC, then AAC branches to ACG (colour 0) and ACT (colour 1); the stem carries both.  The branch cuts
    # already, so no edge is a colour break; a third reference that holds GAA alone cuts the stem twice
    S, sets, (U, Z, nb) = run(["TGAACG", "AACT"], ["TGAACG", "TGAACT"], 3)
    assert list(zip(U, [set(z) for z in Z])) == [("TGAAC", {0, 1}), ("ACG", {0}), ("ACT", {1})] and nb == 0
    S, sets, (U, Z, nb) = run(["TGAACG", "AACT"], ["TGAACG", "TGAACT", "GAA"], 3)
    assert sorted(zip(U, [tuple(sorted(z)) for z in Z])) == sorted(
        [("TGA", (0, 1)), ("GAA", (0, 1, 2)), ("AAC", (0, 1)), ("ACG", (0,)), ("ACT", (1,))]) and nb == 2


def test_a_cycle_cannot_have_one_break():
    # around a cycle the sets of neighbours are equal except across breaks, so one break alone would make S(v) != S(v)
    rng = random.Random(5)
    seen = set()
    for _ in range(200):
        cyc = "".join(rng.choice("ACGT") for _ in range(rng.randint(4, 12)))
        S = kmer_set([cyc + cyc[:3]], 4)
        if unitigs_of_kmers(S, 4) and len(unitigs_of_kmers(S, 4)) == 1 and len(S) == len(cyc):
            kmers = sorted(S)
            one = rng.random() < 0.3      # (one set on all of it: no break)
            sets = {x: frozenset(c for c in range(2) if one or rng.random() < 0.5) for x in kmers}
            seen.add(colored_paths(S, 4, sets)[1])
    assert 1 not in seen and 0 in seen and 2 in seen


def random_case(rng, k, rc):
    alphabet = "AC" if (k <= 5 and rng.random() < 0.5) else "ACGT"
    seqs = ["".join(rng.choice(alphabet) for _ in range(rng.randint(1, 120))) for _ in range(rng.randint(1, 8))]
    if rng.random() < 0.3:
        c = "".join(rng.choice("ACGT") for _ in range(k + 5))
        seqs.append(c + c[:k - 1])
    refs = []
    for _ in range(rng.randint(1, 5)):
        pieces = []
        for _ in range(rng.randint(1, 4)):
            s = rng.choice(seqs)
            a = rng.randrange(len(s))
            pieces.append(s[a:a + rng.randint(1, 80)])
        refs.append(pieces)
    return seqs, refs


@pytest.mark.parametrize("k", [2, 3, 4, 5, 8, 16, 31, 33])
@pytest.mark.parametrize("rc", [False, True])
def test_every_kmer_once_monochromatic_and_maximal(k, rc):
    rng = random.Random(11 * k + rc)
    for trial in range(4):
        seqs, refs = random_case(rng, k, rc)
        B = BruteSBWT(seqs, k, rc)
        sets = sets_of_references(B.kmers, k, refs, 2 if rc else 1)
        U, Z, first, nb = brute_colored_unitigs(B, sets)
        got = [u[i:i + k] for u in U for i in range(len(u) - k + 1)]
        assert len(got) == len(set(got)) == len(B.kmers) and set(got) == B.kmers
        assert first == sorted(first) and len(set(first)) == len(first)
        assert sum(len(u) - k + 1 for u in U) == len(B.kmers)
        rows = column_rows(B, sets)
        for u, z in zip(U, Z):            # monochromatic, and the set is the one of the matrix's rows
            assert all(sets[u[i:i + k]] == z for i in range(len(u) - k + 1))
            assert rows[B.rank_of[u[:k]]] == row_of(z)
        # maximal: joining a unitig with the one that follows its last k-mer would break the plain rule or change the set
        head_of = {u[:k]: i for i, u in enumerate(U)}
        breaks = 0
        for i, u in enumerate(U):
            last = u[-k:]
            nxt = [last[1:] + c for c in "ACGT" if last[1:] + c in B.kmers]
            if len(nxt) == 1 and nxt[0] in head_of and nxt[0] != u[:k]:
                n_in = len([c for c in "ACGT" if c + nxt[0][:-1] in B.kmers])
                assert n_in > 1 or Z[head_of[nxt[0]]] != Z[i]
                breaks += n_in == 1
            elif len(nxt) == 1 and nxt[0] == u[:k] and len([c for c in "ACGT" if c + nxt[0][:-1] in B.kmers]) == 1:
                pass                      # a pure cycle, cut at its smallest column
            elif len(nxt) == 1:
                assert nxt[0] in head_of  # a single edge that leaves a unitig enters a start
        assert breaks == nb
        # every coloured unitig lies inside a plain one, or (a cycle with a break) inside a rotation of one
        plain = unitigs_of_kmers(B.kmers, k)
        for u in U:
            assert any(u in p or u in p + p[k - 1:] for p in plain)


@pytest.mark.parametrize("k", [2, 3, 5, 8, 31])
def test_one_colour_on_everything_is_the_plain_result(k):
    rng = random.Random(k)
    for trial in range(4):
        seqs, _ = random_case(rng, k, False)
        B = BruteSBWT(seqs, k, trial % 2 == 1)
        for z in (frozenset({0}), EMPTY, frozenset({0, 3, 70})):
            U, Z, first, nb = brute_colored_unitigs(B, {x: z for x in B.kmers})
            assert (U, first) == brute_unitigs(B) and nb == 0 and all(y == z for y in Z)


def test_order_is_by_first_column():
    S, sets, (U, Z, nb) = run(["AACCG", "CCGGTT"], ["AACCG", "CCGGTT"], 3)
    assert [u[:3] for u in U] == sorted((u[:3] for u in U), key=lambda s: colex_key(s, 3))
