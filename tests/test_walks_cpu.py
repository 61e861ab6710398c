"""The brute-force restatement of the walks (tests/walks_brute.py): hand cases on the graphs of section
21's table with their known answers, and on random plain and coloured k-mer sets everything the definition says follows --
among it that every continuation is a link and that the offset-0 shortcut of the kernels agrees with the general rule."""
import itertools
import random

import pytest

from bruteforce import BruteSBWT, kmer_set
from colored_unitig_brute import sets_of_references
from test_colored_unitigs_cpu import random_case
from unitig_links_brute import brute_colored_links, brute_links
from walks_brute import brute_walks, check_consequences, random_reads, steps_by_shortcut, steps_of_read


def graph(seqs, refs, k):
    S = kmer_set(seqs, k)
    if refs is None:
        return brute_links(S, k)
    return brute_colored_links(S, k, sets_of_references(S, k, [[r] for r in refs]))


def test_branch_and_gap():
    # unitigs AAC, ACG, ACT; links AAC -> ACG, AAC -> ACT.  CGA and GAA are no k-mers of the set: a gap of two windows
    U, lo, lt, where = graph(["AACG", "AACT"], None, 3)
    assert U == ["AAC", "ACG", "ACT"]
    so, steps, cov = brute_walks(["AACGAACT"], 3, where, len(U))
    assert so == [0, 4] and steps == [(0, 0, 0, 1), (1, 0, 1, 1), (0, 0, 4, 1), (2, 0, 5, 1)]
    assert cov == [2, 1, 1]
    check_consequences(["AACGAACT"], 3, where, U, lo, lt, so, steps)


def test_twice_round_a_cut_cycle():
    # the cycle of ACGTACG is one unitig, GTACGT (k-mers GTA TAC ACG CGT), with its self-link
    U, lo, lt, where = graph(["ACGTACG"], None, 3)
    assert U == ["GTACGT"] and lt == [0]
    read = "ACGTACGTACGT"                  # ACG CGT | GTA TAC ACG CGT | GTA TAC ACG CGT
    so, steps, cov = brute_walks([read], 3, where, 1)
    assert steps == [(0, 2, 0, 2), (0, 0, 2, 4), (0, 0, 6, 4)] and cov == [10]
    check_consequences([read], 3, where, U, lo, lt, so, steps)


def test_colour_break_plain_against_coloured():
    seqs, refs, read = ["AACCG", "CCGGTT"], ["AACCG", "CCGGTT"], "AACCGGTT"
    U, lo, lt, where = graph(seqs, None, 3)
    assert brute_walks([read], 3, where, len(U))[1] == [(0, 0, 0, 6)]
    U, lo, lt, where = graph(seqs, refs, 3)
    assert U == ["AACC", "CCG", "CGGTT"]
    so, steps, cov = brute_walks([read], 3, where, len(U))
    assert steps == [(0, 0, 0, 2), (1, 0, 2, 1), (2, 0, 3, 3)] and cov == [2, 1, 3]
    check_consequences([read], 3, where, U, lo, lt, so, steps)


def test_not_upper_case_acgt_misses_and_short_reads_have_no_step():
    U, lo, lt, where = graph(["AACCGGTT"], None, 3)
    reads = ["AACCgGTT", "AACNGGTT", "AA", "", "TTTTT"]
    so, steps, cov = brute_walks(reads, 3, where, 1)
    assert so == [0, 2, 4, 4, 4, 4]
    assert steps == [(0, 0, 0, 2), (0, 5, 5, 1), (0, 0, 0, 1), (0, 4, 4, 2)]
    check_consequences(reads, 3, where, U, lo, lt, so, steps)


def test_all_64_3mers_every_window_is_a_step():
    S = {"".join(p) for p in itertools.product("ACGT", repeat=3)}
    U, lo, lt, where = brute_links(S, 3)
    rng = random.Random(3)
    reads = ["".join(rng.choice("ACGT") for _ in range(n)) for n in (3, 10, 64)]
    so, steps, cov = brute_walks(reads, 3, where, 64)
    assert so == [0, 1, 9, 71] and all(n == 1 and o == 0 for _, o, _, n in steps)
    check_consequences(reads, 3, where, U, lo, lt, so, steps)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 16, 31, 33])
@pytest.mark.parametrize("rc", [False, True])
def test_random_sets_plain_and_coloured(k, rc):
    rng = random.Random(23 * k + rc)
    continued = 0
    for trial in range(4):
        seqs, refs = random_case(rng, max(k, 2), rc)
        B = BruteSBWT(seqs, k, rc)
        sets = sets_of_references(B.kmers, k, refs, 2 if rc else 1)
        reads = random_reads(rng, seqs, k)
        for U, lo, lt, where in (brute_links(B.kmers, k), brute_colored_links(B.kmers, k, sets)):
            so, steps, cov = brute_walks(reads, k, where, len(U))
            check_consequences(reads, k, where, U, lo, lt, so, steps)
            assert sum(cov) == sum(s[3] for s in steps)
            for r in reads:
                mine = steps_of_read(r, k, where)
                assert steps_by_shortcut(r, k, where) == mine
                continued += sum(1 for a, b in zip(mine, mine[1:]) if a[2] + a[3] == b[2])
    assert continued > 0            # the reads do cross links
