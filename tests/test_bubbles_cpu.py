"""No GPU: the brute force of the bubbles (tests/bubbles_brute.py; include/sbwtgpu.h, "bubbles") on hand-written cases whose
expected values are written out by hand, and on random genomes with planted SNPs.  All hand cases are at k = 4 on
g = CATTGACCGTAGGA, whose 3-mers are distinct: position 7 (the second C of GACC) is the variant site."""
import pytest

import bubbles_brute as bb
from bruteforce import kmer_set, revcomp

K = 4
G = "CATTGACCGTAGGA"
H = "CATTGACTGTAGGA"            # G with C -> T at position 7


def run(seqs, k=K):
    U, lo, lt, recs = bb.brute_bubbles(kmer_set(seqs, k), k)
    return U, lo, lt, recs


def circular(s, k):
    return s + s[:k - 1]


def test_one_snp():
    U, lo, lt, recs = run([G, H])
    # CATTGAC forks to GACC.. and GACT.., both spell four k-mers and meet again at GTAG
    assert U == ["GACCGTA", "GTAGGA", "GACTGTA", "CATTGAC"]
    assert (lo, lt) == ([0, 1, 1, 2, 4], [1, 1, 0, 2])
    assert bb.in_degrees(4, lt) == [1, 2, 1, 0]
    assert recs == [(3, 0, 2, 1, K, K, bb.SNP)]               # branch a by the smaller edge character: C before T
    assert bb.alleles(U, recs[0]) == ("CGTA", "TGTA")          # the variant bases first
    assert bb.snp_bases(U, recs) == [("C", "T")]


def test_insertion_of_three_bases():
    U, _, lt, recs = run([G, G[:7] + "TTA" + G[7:]])
    assert U == ["CGTAGGA", "GACCGT", "GACTTACGT", "CATTGAC"]
    assert recs == [(3, 1, 2, 0, 3, 6, bb.OTHER)]              # n_kmers differ by the three inserted bases
    assert bb.alleles(U, recs[0]) == ("CGT", "TTACGT")


def test_three_alleles_are_no_bubble():
    U, lo, lt, recs = run([G, H, G[:7] + "A" + G[8:]])
    assert lo[-1] - lo[-2] == 3 and bb.in_degrees(len(U), lt)[U.index("GTAGGA")] == 3
    assert recs == []


def test_a_path_that_joins_a_branch_cuts_it():
    # TTCGTA joins G's branch at CGTA, which becomes a unitig of its own with two in-links
    U, lo, lt, recs = run([G, H, "TTCGTA"])
    assert U == ["CGTA", "GACCGT", "GTAGGA", "TTCGT", "GACTGTA", "CATTGAC"]
    assert bb.in_degrees(6, lt) == [2, 1, 2, 0, 1, 0]
    assert recs == []                                          # the links of the two branches of CATTGAC go to CGTA and to GTAGGA


def test_diamond_whose_sink_has_a_third_in_link():
    # AGTA is a third in-neighbour of GTAG beside CGTA and TGTA: the diamond of test_one_snp stands, its sink has in-degree 3
    U, lo, lt, recs = run([G, H, "AAGTAGG"])
    t = U.index("GTAGGA")
    assert bb.in_degrees(len(U), lt)[t] == 3
    assert recs == []


def test_branch_with_a_second_out_link():
    U, lo, lt, recs = run([G, H, "ACCGG"])
    assert U == ["GACCG", "GTAGGA", "CCGG", "GACTGTA", "CCGTA", "CATTGAC"]
    assert lt[lo[0]:lo[1]] == [2, 4]                           # the branch GACCG goes on to CCGG and to CCGTA
    assert recs == []


def test_self_link_source():
    U, lo, lt, recs = run(["AAAAACGT"])
    assert U == ["AAAA", "AAACGT"] and (lo, lt) == ([0, 2, 2], [0, 1])     # out-degree 2, one of the links to itself
    assert recs == []


def test_bubble_on_a_cycle_has_source_equal_sink():
    c = "CATTGACCGTAGG"
    U, lo, lt, recs = run([circular(c, K), circular(c[:7] + "T" + c[8:], K)])
    assert U == ["GACCGTA", "GTAGGCATTGAC", "GACTGTA"]
    assert recs == [(1, 0, 2, 1, K, K, bb.SNP)]
    assert bb.alleles(U, recs[0]) == ("CGTA", "TGTA")


def test_two_snps_closer_than_k():
    # positions 7 and 10 differ: the branches cannot meet between them, so one bubble of 4 + 3 k-mers a side, kind OTHER
    g = "CATTGACCGTAGGAAGCTC"
    h = "CATTGACTGTCGGAAGCTC"
    U, _, _, recs = run([g, h])
    assert U == ["GGAAGCTC", "GACCGTAGGA", "GACTGTCGGA", "CATTGAC"]
    assert recs == [(3, 1, 2, 0, 7, 7, bb.OTHER)]
    assert bb.alleles(U, recs[0]) == ("CGTAGGA", "TGTCGGA")
    # a third haplotype with the first difference only nests a fork inside the branch: no simple bubble is left
    U, _, _, recs = run([g, h, "CATTGACTGTAGGAAGCTC"])
    assert len(U) == 7 and recs == []


def test_branch_colours():
    refs = [[G], [H], [G], ["ACTGT"]]                          # g, h, a copy of g, a fragment of h's branch (2 of its 4 k-mers)
    kmers = kmer_set([G, H], K)
    sets = {x: frozenset(c for c, r in enumerate(refs) if x in kmer_set(r, K)) for x in kmers}
    U, lo, lt, recs = run([G, H])
    col = bb.branch_colors(U, recs, K, sets)
    assert col == [((frozenset({0, 2}), frozenset({0, 2})), (frozenset({1}), frozenset({1, 3})))]
    assert bb.format_tsv(U, len(lt), recs, col) == "# unitigs 4 links 4 bubbles 1 snps 1\n3\t0\t2\t1\t4\t4\tSNP\tCGTA\tTGTA\t0,2\t1|1,3\n"
    assert bb.format_tsv(U, len(lt), recs) == "# unitigs 4 links 4 bubbles 1 snps 1\n3\t0\t2\t1\t4\t4\tSNP\tCGTA\tTGTA\n"
    assert bb.row_words(frozenset({0, 65}), 2) == [1, 2]
    # a k-mer nobody colours empties the intersection of its branch
    del sets["ACCG"]
    assert bb.branch_colors(U, recs, K, sets)[0][0] == (frozenset(), frozenset({0, 2}))


@pytest.mark.parametrize("k,length,n_snps,seed", [(15, 3000, 40, 1), (15, 3000, 40, 2), (31, 6000, 80, 3), (64, 8000, 50, 5)])
def test_planted_snps_are_found(k, length, n_snps, seed):
    g, h, sites = bb.planted(k, length, n_snps, seed)
    assert all(b - a >= 2 * k for (a, _, _), (b, _, _) in zip(sites, sites[1:])) and sites[0][0] >= 2 * k and sites[-1][0] < length - 2 * k
    want = sorted(tuple(sorted((x, y))) for _, x, y in sites)
    U, _, _, recs = run([g, h], k)
    assert len(recs) == n_snps and all(r[4:] == (k, k, bb.SNP) for r in recs)
    assert bb.snp_bases(U, recs) == want
    assert [r[0] for r in recs] == sorted(r[0] for r in recs)
    # with reverse complements every bubble appears once per strand
    U2, _, _, recs2 = run([g, h, revcomp(g), revcomp(h)], k)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    assert len(recs2) == 2 * n_snps and all(r[6] == bb.SNP for r in recs2)
    assert bb.snp_bases(U2, recs2) == sorted(want + [tuple(sorted((comp[x], comp[y]))) for x, y in want])
