"""CPU: the definition of a screen (tests/screen_brute.py) on hand-written cases worked out on paper, and its identities on
random inputs.  No device, no library call."""
import random

import pytest

import screen_brute as sb
import shared_kmers_brute as sk


def kmers_of(seqs, k):
    return {s[i:i + k] for s in seqs for i in range(len(s) - k + 1)}


# the k = 3 examples of the unitig-graph table as four references
REFS3 = ["AACG", "AACT", "AAAAA", "ACGTACG"]


def world3():
    cs = [kmers_of([r], 3) for r in REFS3]
    assert cs == [{"AAC", "ACG"}, {"AAC", "ACT"}, {"AAA"}, {"ACG", "CGT", "GTA", "TAC"}]
    return set().union(*cs), cs


def test_two_overlapping_references():
    # colour 0 = AACCG, colour 1 = CCGGTT: AAC and ACC carry {0}, CCG carries {0, 1}, CGG, GGT and GTT carry {1}
    cs = [kmers_of(["AACCG"], 3), kmers_of(["CCGGTT"], 3)]
    idx = cs[0] | cs[1]
    S = sb.Screen(idx, cs, 3, ["AACCGG"])
    assert (S.n_windows, S.n_hits, S.n_seen) == (4, 4, 4)
    assert (S.ref_kmers, S.ref_seen, S.ref_hits) == ([3, 4], [3, 2], [3, 2])
    S = sb.Screen(idx, cs, 3, ["AACCGG", "CCGCCG"])              # CCG twice more, CGC and GCC miss
    assert (S.n_windows, S.n_hits, S.n_seen) == (8, 6, 4)
    assert (S.ref_kmers, S.ref_seen, S.ref_hits) == ([3, 4], [3, 2], [5, 4])
    assert S.sets([0, 1, 3, 2]) == ([0, 2, 1, 3], [0, 2, 1, 1], [0, 2, 3, 1])
    assert S.sets([0, 2, 1, 3], n_dummies=5) == ([5, 3, 2, 1], [0, 1, 2, 1], [0, 1, 2, 3])
    assert sb.screen_tsv(S) == b"# windows 8 hits 6 seen 4\n0\t3\t3\t5\n1\t4\t2\t4\n"
    assert sb.sets_tsv(*S.sets([0, 1, 3, 2])) == b"0\t0\t0\t0\n1\t2\t2\t2\n2\t1\t1\t3\n3\t3\t1\t1\n"


def test_the_graph_examples_as_references():
    idx, cs = world3()
    S = sb.Screen(idx, cs, 3, ["AAAAAC"])                         # AAA three times, AAC once
    assert (S.n_windows, S.n_hits, S.n_seen) == (4, 4, 2)
    assert S.ref_kmers == [2, 2, 1, 4]
    assert S.ref_seen == [1, 1, 1, 0]
    assert S.ref_hits == [1, 1, 3, 0]
    assert S.hits_of == {"AAA": 3, "AAC": 1}


def test_a_read_that_misses_a_short_read_and_an_n():
    idx, cs = world3()
    S = sb.Screen(idx, cs, 3, ["GGGGG"])
    assert (S.n_windows, S.n_hits, S.n_seen) == (3, 0, 0) and S.ref_seen == [0] * 4 and S.ref_hits == [0] * 4
    assert S.ref_kmers == [2, 2, 1, 4]
    S = sb.Screen(idx, cs, 3, ["AC", "", "A"])
    assert (S.n_windows, S.n_hits, S.n_seen) == (0, 0, 0)
    S = sb.Screen(idx, cs, 3, ["AANAAAC"])                        # AAN, ANA, NAA count and miss; AAA and AAC hit
    assert (S.n_windows, S.n_hits, S.n_seen) == (5, 2, 2) and S.ref_hits == [1, 1, 1, 0]
    S = sb.Screen(idx, cs, 3, ["aaaaac"])                         # lower case is no base
    assert (S.n_windows, S.n_hits) == (4, 0)
    S = sb.Screen(idx, cs, 3, ["AANAAAC"], strands=2)             # + GTT, TTT, TTN... : none of them indexed
    assert (S.n_windows, S.n_hits, S.n_seen) == (10, 2, 2)


def test_a_palindromic_window_under_two_strands():
    cs = [kmers_of(["ACGTT"], 4)]                                 # ACGT (its own reverse complement) and CGTT
    idx = set(cs[0])
    S = sb.Screen(idx, cs, 4, ["ACGT"], strands=2)
    assert (S.n_windows, S.n_hits, S.n_seen) == (2, 2, 1) and S.hits_of == {"ACGT": 2}
    assert (S.ref_kmers, S.ref_seen, S.ref_hits) == ([2], [1], [2])
    S = sb.Screen(idx, cs, 4, ["AACG"], strands=2)                # AACG is not indexed, its reverse complement CGTT is
    assert (S.n_windows, S.n_hits, S.n_seen) == (2, 1, 1) and S.hits_of == {"CGTT": 1}
    S = sb.Screen(idx, cs, 4, ["AACG"], strands=1)
    assert (S.n_windows, S.n_hits, S.n_seen) == (1, 0, 0)


def test_an_index_kmer_of_no_reference_hits_set_0():
    idx, cs = world3()
    idx = idx | {"GGG"}
    S = sb.Screen(idx, cs, 3, ["GGGG", "AAAC"])
    assert (S.n_windows, S.n_hits, S.n_seen) == (4, 4, 3)
    rows = [0, 3, 9, 2, 4, 8]
    km, seen, hits = S.sets(rows, n_dummies=2)
    assert km == [1 + 2, 1, 1, 1, 1, 3] and seen == [1, 1, 0, 0, 1, 0] and hits == [2, 1, 0, 0, 1, 0]
    assert sum(hits) == S.n_hits and sum(seen) == S.n_seen
    assert S.ref_hits == [1, 1, 1, 0]                             # the hits on GGG are in no reference's count


def random_world(rng):
    k = rng.randint(2, 9)
    alphabet = "ACGT" if rng.random() < 0.5 else "AC"
    n_colors = rng.randint(1, 6)
    refs = [["".join(rng.choice(alphabet) for _ in range(rng.randint(0, 40))) for _ in range(rng.randint(1, 3))]
            for _ in range(n_colors)]
    cs = [kmers_of(r, k) for r in refs]
    extra = kmers_of(["".join(rng.choice(alphabet) for _ in range(30))], k)
    idx = set().union(extra, *cs)
    reads = []
    for _ in range(rng.randint(0, 12)):
        src = rng.choice(rng.choice(refs)) if rng.random() < 0.7 else "".join(rng.choice(alphabet) for _ in range(25))
        r = list(src[rng.randint(0, 5):])
        for i in range(len(r)):
            if rng.random() < 0.05:
                r[i] = rng.choice("ACGTNa")
        r = "".join(r)
        reads.append(sb.revcomp(r) if rng.random() < 0.3 else r)
    return k, cs, idx, reads


@pytest.mark.parametrize("seed", range(40))
def test_identities_on_random_inputs(seed):
    rng = random.Random(seed)
    k, cs, idx, reads = random_world(rng)
    for strands in (1, 2):
        S = sb.Screen(idx, cs, k, reads, strands)
        assert S.n_windows == strands * sum(max(0, len(r) - k + 1) for r in reads)
        rows = [0] + sorted(set(S.row.values()) - {0})
        km, seen, hits = S.sets(rows, n_dummies=3)
        assert sum(hits) == S.n_hits and sum(seen) == S.n_seen and sum(km) == len(idx) + 3
        assert all(0 <= s <= m and s <= h for m, s, h in zip(km, seen, hits))
        G = sk.shared_of_kmers(cs, idx)
        assert S.ref_kmers == [G[c][c] for c in range(len(cs))]
        assert all(0 <= a <= b for a, b in zip(S.ref_seen, S.ref_kmers)) and all(a <= b for a, b in zip(S.ref_seen, S.ref_hits))
        # the same from arrays: columns = two dummies, then the k-mers in some order
        labels = ["$$", "$A"] + sorted(idx)
        col = {x: v for v, x in enumerate(labels)}
        ids = [0, 0] + [rows.index(S.row[x]) for x in labels[2:]]
        M = sb.sample(reads, k, strands)
        results = [col.get(x, -1) if x is not None else -1 for x, n in M.items() for _ in range(n)]
        A = sb.from_arrays(ids, rows, len(cs), results)
        km2, _, _ = S.sets(rows, n_dummies=2)
        assert (A["n_windows"], A["n_hits"], A["n_seen"]) == (S.n_windows, S.n_hits, S.n_seen)
        assert (A["set_kmers"], A["set_seen"], A["set_hits"]) == (km2, seen, hits)
        assert (A["ref_kmers"], A["ref_seen"], A["ref_hits"]) == (S.ref_kmers, S.ref_seen, S.ref_hits)
        words = S.seen_bitmap(labels)
        assert [v for v in range(len(labels)) if (words[v >> 6] >> (v & 63)) & 1] == A["seen"]
    # two strands = one strand on the reads plus their reverse complements
    two = sb.Screen(idx, cs, k, reads, 2)
    both = sb.Screen(idx, cs, k, list(reads) + [sb.revcomp(r) for r in reads], 1)
    assert (two.n_windows, two.n_hits, two.hits_of) == (both.n_windows, both.n_hits, both.hits_of)
    assert (two.ref_kmers, two.ref_seen, two.ref_hits) == (both.ref_kmers, both.ref_seen, both.ref_hits)
