"""No GPU: the brute force of the genotype object (tests/genotype_brute.py; include/sbwtgpu.h, "genotype") on hand-written cases
at k = 4 whose expected counters are written out by hand.  The cases are those of tests/test_bubbles_cpu.py:
g = CATTGACCGTAGGA and h = g with C -> T at position 7.  Their graph has the unitigs GACCGTA (branch a: GACC ACCG CCGT CGTA,
positions 0 .. 3), GACTGTA (branch b: GACT ACTG CTGT TGTA, positions 4 .. 7), the source CATTGAC and the sink GTAGGA."""
import pytest

import bubbles_brute as bb
import genotype_brute as gb
from bruteforce import kmer_set
from screen_brute import revcomp

K = 4
G = "CATTGACCGTAGGA"
H = "CATTGACTGTAGGA"


def snp():
    return gb.from_kmers(kmer_set([G, H], K), K)


def state(g):
    return g.kmer_hits, (g.n_windows, g.n_hits, g.n_site_hits), g.branches()


def test_layout_of_the_snp_case():
    g = snp()
    assert g.recs == [(3, 0, 2, 1, K, K, bb.SNP)]
    assert g.branch_off == [0, 4, 8] and g.P == 8 and g.slot_of == {0: 0, 2: 1}
    assert state(g) == ([0] * 8, (0, 0, 0), ([0, 0], [0, 0], [0, 0]))
    assert g.calls() == [0] and g.calls(1, 0) == [0]          # the smallest breadth still asks for one k-mer seen: 0 >= 1 * 4 fails
    assert g.info() == {"n_bubbles": 1, "n_branch_kmers": 8, "n_windows": 0, "n_hits": 0, "n_site_hits": 0, "n_colors": 0}


def test_reads_from_one_reference_call_its_allele():
    # g's eleven windows all hit, four of them on branch a (the smaller edge character, C)
    assert state(snp().add([G])) == ([1, 1, 1, 1, 0, 0, 0, 0], (11, 11, 4), ([4, 0], [4, 0], [1, 0]))
    assert snp().add([G]).calls() == [1]
    assert state(snp().add([H])) == ([0, 0, 0, 0, 1, 1, 1, 1], (11, 11, 4), ([0, 4], [0, 4], [0, 1]))
    assert snp().add([H]).calls() == [2]


def test_reads_from_both_references_call_both():
    g = snp().add([G, H])
    assert state(g) == ([1] * 8, (22, 22, 8), ([4, 4], [4, 4], [1, 1]))
    assert g.calls() == [3]
    assert snp().add([G]).add([H]).kmer_hits == g.kmer_hits     # batch boundaries do not matter


def test_a_branch_covered_but_for_one_kmer():
    g = snp().add(["GACCGT"])                                   # GACC ACCG CCGT: all of branch a but CGTA
    assert state(g) == ([1, 1, 1, 0, 0, 0, 0, 0], (3, 3, 3), ([3, 0], [3, 0], [0, 0]))
    assert g.calls(1_000_000, 0) == [0] and g.calls(1_000_000, 1) == [0]      # min_hits = 0, seen = n - 1: no call at full breadth
    assert g.calls(750_000, 0) == [1]                           # 3 * 10^6 >= 750 000 * 4 holds with equality
    assert g.calls(750_001, 0) == [0]
    assert g.calls(750_000, 1) == [0]                           # 3 hits on 4 k-mers: the mean depth is below 1
    assert g.add(["GACCGT"]).calls(750_000, 1) == [1]           # 6 hits


def test_one_window_sixty_five_times():
    g = snp().add(["GACC"] * 65)
    assert state(g) == ([65, 0, 0, 0, 0, 0, 0, 0], (65, 65, 65), ([1, 0], [65, 0], [0, 0]))
    assert g.calls(250_000, 1) == [1] and g.calls(250_001, 1) == [0]


def test_insertion_three_against_six_kmers():
    g2 = G[:7] + "TTA" + G[7:]
    g = gb.from_kmers(kmer_set([G, g2], K), K)
    assert g.unitigs == ["CGTAGGA", "GACCGT", "GACTTACGT", "CATTGAC"] and g.recs == [(3, 1, 2, 0, 3, 6, bb.OTHER)]
    assert g.branch_off == [0, 3, 9]
    assert state(g.add([G])) == ([1, 1, 1, 0, 0, 0, 0, 0, 0], (11, 11, 3), ([3, 0], [3, 0], [1, 0]))
    assert g.calls() == [1]
    g.reset()
    assert state(g.add([g2])) == ([0, 0, 0, 1, 1, 1, 1, 1, 1], (14, 14, 6), ([0, 6], [0, 6], [0, 1]))
    assert g.calls() == [2]
    # depth is per k-mer of the branch: five hits on the six k-mers of b are not depth 1
    g.reset()
    assert g.add(["GACTTACG"]).branches() == ([0, 5], [0, 5], [0, 0]) and g.calls(800_000, 1) == [0] and g.calls(800_000, 0) == [2]


def test_cycle_with_source_equal_sink():
    c = "CATTGACCGTAGG"
    ca, cb = c + c[:K - 1], c[:7] + "T" + c[8:] + c[:K - 1]
    g = gb.from_kmers(kmer_set([ca, cb], K), K)
    assert g.recs == [(1, 0, 2, 1, K, K, bb.SNP)]
    assert state(g.add([ca])) == ([1, 1, 1, 1, 0, 0, 0, 0], (13, 13, 4), ([4, 0], [4, 0], [1, 0]))
    assert g.calls() == [1]


def test_min_depth_at_its_boundary():
    g = snp().add([G, "GACCGT"])                                # 4 + 3 hits on the 4 k-mers of a: one below depth 2
    assert g.branches() == ([4, 0], [7, 0], [1, 0])
    assert g.calls(1_000_000, 2) == [0] and g.calls(1_000_000, 1) == [1]
    g.add(["CGTA"])                                             # the eighth
    assert g.branches() == ([4, 0], [8, 0], [2, 0])
    assert g.calls(1_000_000, 2) == [1] and g.calls(1_000_000, 3) == [0]
    assert g.calls(1_000_000, 2**62) == [0]


def test_reads_on_source_and_sink_only():
    g = snp().add(["CATTGAC", "GTAGGA"])
    assert state(g) == ([0] * 8, (7, 7, 0), ([0, 0], [0, 0], [0, 0]))
    assert g.calls() == [0]


def test_lower_case_n_and_short_reads():
    # gaccgta: four windows, none upper-case; GACNGTA: every window holds the N; GAC and the empty read: no window;
    # GACCgTA: GACC hits, the three windows with the g do not
    g = snp().add(["gaccgta", "GACNGTA", "GAC", "", "GACCgTA"])
    assert state(g) == ([1, 0, 0, 0, 0, 0, 0, 0], (12, 1, 1), ([1, 0], [1, 0], [0, 0]))


def test_two_strands():
    # the reverse complement of g read on both strands is g read on both strands: every window twice, once per strand
    want = ([1, 1, 1, 1, 0, 0, 0, 0], (22, 11, 4), ([4, 0], [4, 0], [1, 0]))
    assert not kmer_set([revcomp(G), revcomp(H)], K) & kmer_set([G, H], K)
    assert state(snp().add([G], 2)) == want and state(snp().add([revcomp(G)], 2)) == want
    assert state(snp().add([revcomp(G)], 1)) == ([0] * 8, (11, 0, 0), ([0, 0], [0, 0], [0, 0]))
    # on an index that holds both strands the twin bubble keeps its own counters
    g = gb.from_kmers(kmer_set([G, H, revcomp(G), revcomp(H)], K), K)
    assert len(g.recs) == 2 and g.P == 16
    g.add([G], 2)
    assert (g.n_windows, g.n_hits, g.n_site_hits) == (22, 22, 8)
    # g carries C, the smaller character, so allele a; its reverse complement carries G against h's A, so allele b of the twin
    assert sorted(g.calls()) == [1, 2] and sorted(g.branches()[1]) == [0, 0, 4, 4]


def test_colours():
    refs = [[G], [H], [G], ["ACTGT"]]                          # g = 0, h = 1, a copy of g = 2, a fragment of h's branch = 3
    kmers = kmer_set([G, H], K)
    sets = {x: frozenset(c for c, r in enumerate(refs) if x in kmer_set(r, K)) for x in kmers}
    g = snp()
    col = bb.branch_colors(g.unitigs, g.recs, K, sets)
    inter = gb.inter_sets(col)
    assert inter == [(frozenset({0, 2}), frozenset({1}))]       # colour 3 holds no whole allele: informative nowhere
    assert g.refs(inter, 4) == ([0] * 4, [0] * 4, [0] * 4)      # no call, no site
    g.add([G])
    assert g.refs(inter, 4) == ([1, 1, 1, 0], [1, 0, 1, 0], [1, 0, 1, 0])      # ref_only separates 0 and 2 from 1
    assert gb.format_tsv(g, 4, col) == ("# unitigs 4 links 4 bubbles 1 snps 1 windows 11 hits 11 site_hits 4\n"
                                        "3\t0\t2\t1\t4\t4\tSNP\tCGTA\tTGTA\t0,2\t1|1,3\t4\t4\t1\t0\t0\t0\ta\n")
    assert gb.format_tsv(g, 4) == ("# unitigs 4 links 4 bubbles 1 snps 1 windows 11 hits 11 site_hits 4\n"
                                   "3\t0\t2\t1\t4\t4\tSNP\tCGTA\tTGTA\t4\t4\t1\t0\t0\t0\ta\n")
    assert gb.refs_tsv(*g.refs(inter, 4)) == "0\t1\t1\t1\n1\t1\t0\t0\n2\t1\t1\t1\n3\t0\t0\t0\n"
    g.add([H])
    assert g.refs(inter, 4) == ([1, 1, 1, 0], [1, 1, 1, 0], [0, 0, 0, 0])      # both alleles: every reference matches, none alone
    assert gb.format_tsv(g, 4).endswith("\t4\t4\t1\t4\t4\t1\tab\n")
    g.reset()
    g.add([H])
    assert g.refs(inter, 4) == ([1, 1, 1, 0], [0, 1, 0, 0], [0, 1, 0, 0])
    # a colour on both alleles is informative nowhere
    assert g.refs([(frozenset({0, 1}), frozenset({1}))], 2) == ([1, 0], [0, 0], [0, 0])


def test_snps_only_filters_lines_not_counts():
    g2 = G[:7] + "TTA" + G[7:]
    g = gb.from_kmers(kmer_set([G, g2], K), K).add([G])
    assert gb.format_tsv(g, 4, snps_only=True) == "# unitigs 4 links 4 bubbles 1 snps 0 windows 11 hits 11 site_hits 3\n"
    assert gb.format_tsv(g, 4).count("\n") == 2


@pytest.mark.parametrize("length,step", [(6, 1), (6, 4), (14, 3), (20, 5)])
def test_tiles_cover_the_sequence(length, step):
    t = gb.tiles(G, length, step)
    assert t[0] == G[:length] and t[-1] == G[max(0, len(G) - length):] and all(len(x) == min(length, len(G)) for x in t)
