"""The brute-force restatement of the unitig definition (tests/unitig_brute.py): hand-written cases with known answers, and
every k-mer exactly once on random sets."""
import random

import pytest

from bruteforce import BruteSBWT, colex_key, kmer_set, revcomp
from unitig_brute import brute_unitigs, flatten, unitigs_of_kmers


def circular(s, k):
    return s + s[:k - 1]


def test_four_cycle_k3():
    # ACG -> CGT -> GTA -> TAC -> ACG: no start; colex-smallest is GTA (read backwards: ATG)
    assert unitigs_of_kmers(kmer_set([circular("ACGT", 3)], 3), 3) == ["GTACGT"]


def test_self_loop():
    assert unitigs_of_kmers(kmer_set(["AAAAA"], 3), 3) == ["AAA"]
    assert unitigs_of_kmers(kmer_set(["A" * 40], 31), 31) == ["A" * 31]


def test_cycle_with_a_tail_entering_it():
    # CAC enters the cycle at ACG, which then has two in-neighbours: ACG is a start, the cycle is not pure, and the edge
    # TAC -> ACG is not internal
    assert unitigs_of_kmers(kmer_set(["CACGTACG"], 3), 3) == ["CAC", "ACGTAC"]


def test_y_branch():
    # TGA -> GAA -> AAC, then AAC branches to ACG and ACT
    assert unitigs_of_kmers(kmer_set(["TGAACG", "AACT"], 3), 3) == ["TGAAC", "ACG", "ACT"]


def test_complete_graph_of_3mers():
    all3 = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]
    U = unitigs_of_kmers(all3, 3)
    assert U == sorted(all3, key=lambda s: colex_key(s, 3)) and len(U) == 64


def test_two_disjoint_cycles_are_two_unitigs():
    U = unitigs_of_kmers(kmer_set([circular("ACGT", 3), circular("AAG", 3)], 3), 3)
    # AAG AGA GAA: the smallest is GAA (AAG backwards) -- and before GTA (ATG backwards)
    assert U == ["GAAGA", "GTACGT"]


@pytest.mark.parametrize("k", [2, 3, 4, 5, 8, 16, 31, 33])
@pytest.mark.parametrize("rc", [False, True])
def test_every_kmer_exactly_once(k, rc):
    rng = random.Random(7 * k + rc)
    for trial in range(4):
        alphabet = "AC" if (k <= 5 and trial % 2 == 0) else "ACGT"
        seqs = ["".join(rng.choice(alphabet) for _ in range(rng.randint(1, 120))) for _ in range(rng.randint(1, 8))]
        if trial == 3:
            seqs.append(circular("".join(rng.choice("ACGT") for _ in range(k + 5)), k))
        B = BruteSBWT(seqs, k, rc)
        U, first = brute_unitigs(B)
        got = [u[i:i + k] for u in U for i in range(len(u) - k + 1)]
        assert len(got) == len(set(got)) == len(B.kmers) and set(got) == B.kmers
        assert first == sorted(first) and len(set(first)) == len(first)
        assert all(len(B.nodes[c]) == k for c in first)
        bases, off = flatten(U)
        assert off[-1] == len(bases) == len(B.kmers) + len(U) * (k - 1)
        if rc:                            # the unitigs come in reverse-complement pairs (a palindrome pairs with itself);
            for u in U:                   # a cycle's partner may be cut at another k-mer
                if u[-k:][1:] + u[k - 1] != u[:k]:
                    assert revcomp(u) in U
        # maximal: no unitig's last k-mer has an internal edge to another unitig's first k-mer
        heads = {u[:k] for u in U}
        for u in U:
            last = u[-k:]
            nxt = [last[1:] + c for c in "ACGT" if last[1:] + c in B.kmers]
            if len(nxt) == 1 and nxt[0] in heads and nxt[0] != u[:k]:
                assert len([c for c in "ACGT" if c + nxt[0][:-1] in B.kmers]) > 1
