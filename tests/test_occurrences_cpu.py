"""CPU: the definition of the occurrence table and of the map over all occurrences (tests/occurrences_brute.py) on hand-written
cases at k = 4, every expected key and record written out.  A key is (seq << 32) | (pos << 1) | t; a record is
(start, seq, strand, votes, votes2, n_found, n_anchored)."""
import occurrences_brute as ob
import positions_brute as pb

K = 4
S1, S2 = 1 << 32, 2 << 32           # the sequence field of a key


def kmers_of(refs):
    out = set()
    for s in refs:
        out |= {s[i:i + K] for i in range(len(s) - K + 1) if pb.valid(s[i:i + K])}
    return out


def numbered(refs, strands=1):
    return [(i, s, strands) for i, s in enumerate(refs)]


# ACGG lies at 0 and 6 of sequence 0 and at 2 of sequence 2; CGGT at 1 of sequence 0 and at 1 of sequence 1
REPEAT = ["ACGGTTACGGA", "TCGGTC", "GGACGGC"]


def test_a_kmer_of_two_sequences_that_occurs_twice_in_one():
    kmers = kmers_of(REPEAT)
    occ = ob.table(kmers, K, numbered(REPEAT))
    assert occ["ACGG"] == [0 << 1, 6 << 1, S2 | (2 << 1)] == [0, 12, 8589934596]
    assert occ["CGGT"] == [1 << 1, S1 | (1 << 1)]
    assert occ == {"ACGG": [0, 12, S2 | 4], "CGGT": [2, S1 | 2], "GGTT": [4], "GTTA": [6], "TTAC": [8], "TACG": [10], "CGGA": [14],
                   "TCGG": [S1], "GGTC": [S1 | 4], "GGAC": [S2], "GACG": [S2 | 2], "CGGC": [S2 | 6]}
    assert ob.scalars(occ) == (15, 12, 3)                      # n_occurrences, n_positioned, max_count
    assert pb.scalars(kmers, K, numbered(REPEAT)) == (15, 15)  # n_windows, n_hits
    # the first key of every k-mer is the positions table, which forgets the repeat and the other sequence
    assert ob.first_of(occ) == pb.first_table(kmers, K, numbered(REPEAT))
    # adding a sequence twice under one number changes nothing; under two numbers both keys are there
    again = ob.table(kmers, K, numbered(REPEAT) + [(2, REPEAT[2], 1)])
    assert again == occ
    two = ob.table(kmers, K, numbered(REPEAT) + [(5, REPEAT[2], 1)])
    assert two["ACGG"] == [0, 12, S2 | 4, (5 << 32) | 4] and two["GGAC"] == [S2, 5 << 32]
    # the arrays in column order: dummy columns and k-mers without an occurrence are empty
    labels = ["$$$$", "ACGG", "AAAA", "CGGT", "GGTT"]
    assert ob.arrays(occ, labels) == ([0, 0, 3, 3, 5, 6], [0, 12, S2 | 4, 2, S1 | 2, 4])


def test_a_palindromic_window_one_strand_and_two():
    ref = ["AACGTT"]                                            # ACGT at 1 is its own reverse complement
    kmers = {"AACG", "ACGT", "CGTT"}
    assert ob.table(kmers, K, numbered(ref, 1)) == {"AACG": [0], "ACGT": [2], "CGTT": [4]}
    # two strands: both keys of the palindrome stay; rc(AACG) = CGTT, so those two windows offer each other a t = 1 key
    assert ob.table(kmers, K, numbered(ref, 2)) == {"AACG": [0, 5], "ACGT": [2, 3], "CGTT": [1, 4]}
    # the palindrome's two occurrences are two placements: t = 0 gives o = 0, t = 1 gives o = 1
    occ = ob.table(kmers, K, numbered(ref, 2))
    cnt, found, anchored = ob.votes(occ, kmers, K, "ACGT")
    assert cnt == {(0, 0, 1): 1, (0, 1, 1): 1} and (found, anchored) == (1, 1)
    assert ob.record(occ, kmers, K, "ACGT") == (1, 0, 0, 1, 1, 1, 1)


SHARED = "GATTACAGGC"
STRAINS = ["CC" + SHARED + "TT", "AAAAAAA", "TG" + SHARED + "AC"]      # GGCA, behind the stretch, is sequence 2's alone


def test_a_read_of_the_last_strain_lands_on_it():
    kmers = kmers_of(STRAINS)
    occ = ob.table(kmers, K, numbered(STRAINS))
    first = pb.first_table(kmers, K, numbered(STRAINS))
    assert occ["GATT"] == [2 << 1, S2 | (2 << 1)] and occ["AGGC"] == [16, S2 | 16] and occ["GGCA"] == [S2 | 18] and occ["GGCT"] == [18]
    assert occ["AAAA"] == [S1, S1 | 2, S1 | 4, S1 | 6]
    read = SHARED + "A"                                         # sequence 2's copy and the base behind it
    # the projection onto the first reference reports sequence 0: seven shared k-mers against the one that tells
    assert pb.record(first, kmers, K, read) == (2, 0, 0, 7, 1, 8, 8)
    # every occurrence votes: sequence 2 with all eight, and votes2 is the count of sequence 0's placement
    assert ob.votes(occ, kmers, K, read) == ({(2, 0, 2): 8, (0, 0, 2): 7}, 8, 8)
    assert ob.record(occ, kmers, K, read) == (2, 2, 0, 8, 7, 8, 8)
    # wholly inside the stretch: a tie, reported on the smallest sequence with votes2 == votes
    assert pb.record(first, kmers, K, SHARED) == (2, 0, 0, 7, 0, 7, 7)
    assert ob.record(occ, kmers, K, SHARED) == (2, 0, 0, 7, 7, 7, 7)
    # the reverse-complemented read, both strands searched: the same placements in orientation 1
    assert ob.record(occ, kmers, K, pb.revcomp(read), 2) == (2, 2, 1, 8, 7, 8, 8)
    assert ob.cli_columns(ob.record(occ, kmers, K, read)) == "2 0 2 8 7 8"


def test_max_occ_on_a_kmer_with_three_occurrences():
    kmers = kmers_of(REPEAT)
    occ = ob.table(kmers, K, numbered(REPEAT))
    read = "ACGGT"                                              # ACGG: three occurrences; CGGT: two
    assert ob.votes(occ, kmers, K, read, 1, 3) == ({(0, 0, 0): 2, (0, 0, 6): 1, (2, 0, 2): 1, (1, 0, 0): 1}, 2, 2)
    assert ob.record(occ, kmers, K, read, 1, 3) == (0, 0, 0, 2, 1, 2, 2)
    assert ob.votes(occ, kmers, K, read, 1, 2) == ({(0, 0, 0): 1, (1, 0, 0): 1}, 2, 1)
    assert ob.record(occ, kmers, K, read, 1, 2) == (0, 0, 0, 1, 1, 2, 1)
    assert ob.votes(occ, kmers, K, read, 1, 1) == ({}, 2, 0)
    assert ob.record(occ, kmers, K, read, 1, 1) == (0, -1, 0, 0, 0, 2, 0)      # found, not anchored: the empty record
    # n_anchored counts hits that voted, not votes cast
    assert sum(ob.votes(occ, kmers, K, read, 1, 3)[0].values()) == 5


def test_without_a_shared_kmer_the_record_is_the_projections():
    refs = ["ACGGTTAC", "CCCATGGA"]
    kmers = kmers_of(refs)
    occ = ob.table(kmers, K, numbered(refs))
    first = pb.first_table(kmers, K, numbered(refs))
    assert all(len(v) == 1 for v in occ.values()) and ob.first_of(occ) == first and len(occ) == 10
    want = {("CGGTTA", 1): (1, 0, 0, 3, 0, 3, 3), ("CCATGG", 1): (1, 1, 0, 3, 0, 3, 3), ("GTAACC", 1): (0, -1, 0, 0, 0, 0, 0),
            ("GTAACC", 2): (2, 0, 1, 3, 0, 3, 3), ("ACGGCATG", 1): (0, 0, 0, 1, 1, 2, 2)}
    for read in ("CGGTTA", "CCATGG", "GTAACC", "ACGGCATG", "ACG", ""):
        for strands in (1, 2):
            got = ob.record(occ, kmers, K, read, strands, 1 << 20)
            assert got == pb.record(first, kmers, K, read, strands), (read, strands)
            assert got == want.get((read, strands), got), (read, strands)
