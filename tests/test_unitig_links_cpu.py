"""The brute-force restatement of the unitig graph (tests/unitig_links_brute.py): the hand cases of DESIGN.md section 21
with their known answers, and the invariant, the order and the distinctness of the links and the k-mer coordinates on random
plain and coloured k-mer sets."""
import itertools
import random

import pytest

from bruteforce import BruteSBWT, colex_key, kmer_set
from colored_unitig_brute import sets_of_references
from test_colored_unitigs_cpu import random_case
from unitig_links_brute import brute_colored_links, brute_links, column_map, n_edges

# (index sequences, references or None for the plain run, unitigs, link_off, link_to), k = 3
HAND = [
    (["AACG", "AACT"], None, ["AAC", "ACG", "ACT"], [0, 2, 2, 2], [1, 2]),
    (["AAAAA"], None, ["AAA"], [0, 1], [0]),
    (["ACGTACG"], None, ["GTACGT"], [0, 1], [0]),
    (["AACCG", "CCGGTT"], None, ["AACCGGTT"], [0, 0], []),
    (["AACCG", "CCGGTT"], ["AACCG", "CCGGTT"], ["AACC", "CCG", "CGGTT"], [0, 1, 2, 2], [1, 2]),
]


def run(seqs, refs, k):
    S = kmer_set(seqs, k)
    if refs is None:
        return S, brute_links(S, k)
    return S, brute_colored_links(S, k, sets_of_references(S, k, [[r] for r in refs]))


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_cases(case):
    seqs, refs, unitigs, link_off, link_to = HAND[case]
    S, (U, lo, lt, where) = run(seqs, refs, 3)
    assert (U, lo, lt) == (unitigs, link_off, link_to)
    assert len(lt) == n_edges(S) - (len(S) - len(U))


def test_all_64_3mers():
    S = {"".join(p) for p in itertools.product("ACGT", repeat=3)}
    U, lo, lt, where = brute_links(S, 3)
    assert len(U) == 64 and len(lt) == 256 and lo == list(range(0, 257, 4))
    assert n_edges(S) == 256
    for i, u in enumerate(U):                        # the four targets of a tail in character order
        assert [U[j] for j in lt[lo[i]:lo[i + 1]]] == [u[1:] + c for c in "ACGT"]


def check_properties(S, k, U, lo, lt, where):
    assert len(lo) == len(U) + 1 and lo[0] == 0 and lo[-1] == len(lt)
    assert len(lt) == n_edges(S) - (len(S) - len(U))                          # the invariant
    first_rank = [colex_key(u[:k], k) for u in U]
    for i, u in enumerate(U):
        t = lt[lo[i]:lo[i + 1]]
        assert len(set(t)) == len(t) and t == sorted(t)                       # distinct, ascending target id ...
        assert [first_rank[j] for j in t] == sorted(first_rank[j] for j in t)   # ... and ascending target column
        assert [U[j][k - 1] for j in t] == sorted(U[j][k - 1] for j in t)       # ... by edge character
        for j in t:
            assert U[j][:k - 1] == u[-(k - 1):] if k > 1 else True             # the k-1 overlap
    # within-unitig pairs and the links' pairs are the edge set, each edge once
    edges = [(u[r:r + k], u[r + 1:r + 1 + k]) for u in U for r in range(len(u) - k)]
    edges += [(u[-k:], U[j][:k]) for i, u in enumerate(U) for j in lt[lo[i]:lo[i + 1]]]
    assert len(edges) == len(set(edges)) == n_edges(S)
    assert set(edges) == {(x, x[1:] + c) for x in S for c in "ACGT" if x[1:] + c in S}
    # the coordinates spell the k-mer
    assert set(where) == S
    for x, (i, r) in where.items():
        assert U[i][r:r + k] == x


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 16, 31, 33])
@pytest.mark.parametrize("rc", [False, True])
def test_random_sets_plain_and_coloured(k, rc):
    rng = random.Random(17 * k + rc)
    for trial in range(4):
        seqs, refs = random_case(rng, max(k, 2), rc)
        B = BruteSBWT(seqs, k, rc)
        check_properties(B.kmers, k, *brute_links(B.kmers, k))
        sets = sets_of_references(B.kmers, k, refs, 2 if rc else 1)
        U, lo, lt, where = brute_colored_links(B.kmers, k, sets)
        check_properties(B.kmers, k, U, lo, lt, where)
        cu, co = column_map(B, where)
        assert len(cu) == len(B.nodes)
        for v, lab in enumerate(B.nodes):
            if len(lab) == k:
                assert U[cu[v]][co[v]:co[v] + k] == lab
            else:
                assert (cu[v], co[v]) == (0xFFFFFFFF, 0xFFFFFFFF)


def test_a_colour_break_is_a_link():
    S, (U, lo, lt, where) = run(*HAND[4][:2], 3)
    plain = brute_links(S, 3)
    assert len(plain[2]) == 0 and len(lt) == 2       # the two breaks of the one plain unitig


def test_columns_of_one_group_share_their_targets():
    # AAC and CAC end in the same k-1 characters: each is the tail of its own unitig, both link to ACG and ACT
    S, (U, lo, lt, where) = run(["AACG", "CACT", "AACT"], None, 3)
    a, c = where["AAC"][0], where["CAC"][0]
    assert a != c and lt[lo[a]:lo[a + 1]] == lt[lo[c]:lo[c + 1]] == [where["ACG"][0], where["ACT"][0]]
