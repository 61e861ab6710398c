"""CPU: the definition of the position table and of a read's map record (tests/positions_brute.py) on hand-written cases at
k = 4, every expected key and record written out.  Each case first asserts that it really is the situation it is named for.

The references (windows by offset):
  S0 = GATTACAGATTC   0 GATT  1 ATTA  2 TTAC  3 TACA  4 ACAG  5 CAGA  6 AGAT  7 GATT  8 ATTC
  S1 = CCGTGACTGGA    0 CCGT  1 CGTG  2 GTGA  3 TGAC  4 GACT  5 ACTG  6 CTGG  7 TGGA
  S2 = TGATTG         0 TGAT  1 GATT  2 ATTG
No window of them is the reverse complement of another (asserted below), so the forward index and the index with reverse
complements differ by exactly the 18 reverse complements."""
import bruteforce as bf
import positions_brute as pb

K = 4
S0, S1, S2 = "GATTACAGATTC", "CCGTGACTGGA", "TGATTG"
REFS = [S0, S1, S2]
FWD = bf.kmer_set(REFS, K)
BOTH = bf.kmer_set(REFS + [pb.revcomp(s) for s in REFS], K)
NUMBERED1 = [(i, s, 1) for i, s in enumerate(REFS)]
NUMBERED2 = [(i, s, 2) for i, s in enumerate(REFS)]
T1 = pb.first_table(FWD, K, NUMBERED1)           # forward-only index, one-strand table
T2 = pb.first_table(BOTH, K, NUMBERED2)          # index with reverse complements, two-strand table


def key(seq, pos, t=0):
    return (seq << 32) | (pos << 1) | t


def test_the_worlds_are_what_the_cases_assume():
    assert len(FWD) == 18 and len(BOTH) == 36 and not (FWD & {pb.revcomp(x) for x in FWD})
    assert pb.key(1, 5, 1) == (1 << 32) + 11 and pb.decode((2 << 32) | 7) == (2, 3, 1)
    assert pb.scalars(FWD, K, NUMBERED1) == (9 + 8 + 3, 20) and pb.scalars(FWD, K, NUMBERED2) == (40, 20)
    assert pb.scalars(BOTH, K, NUMBERED2) == (40, 40)
    # the whole forward table, written out
    assert T1 == {"GATT": key(0, 0), "ATTA": key(0, 1), "TTAC": key(0, 2), "TACA": key(0, 3), "ACAG": key(0, 4), "CAGA": key(0, 5),
                  "AGAT": key(0, 6), "ATTC": key(0, 8), "CCGT": key(1, 0), "CGTG": key(1, 1), "GTGA": key(1, 2), "TGAC": key(1, 3),
                  "GACT": key(1, 4), "ACTG": key(1, 5), "CTGG": key(1, 6), "TGGA": key(1, 7), "TGAT": key(2, 0), "ATTG": key(2, 2)}
    # a forward-only index with a two-strand table: the reverse complements are no k-mers of the index, nothing changes
    assert pb.first_table(FWD, K, NUMBERED2) == T1


def test_read_inside_sequence_1_forward():
    read = S1[2:9]
    assert read == "GTGACTG" and [T1[read[i:i + K]] for i in range(4)] == [key(1, 2), key(1, 3), key(1, 4), key(1, 5)]
    cnt, found, anchored = pb.votes(T1, FWD, K, read)
    assert cnt == {(1, 0, 2): 4} and (found, anchored) == (4, 4)
    assert pb.record(T1, FWD, K, read) == (2, 1, 0, 4, 0, 4, 4)
    assert pb.record(T1, FWD, K, read, 2) == (2, 1, 0, 4, 0, 4, 4)
    assert pb.cli_columns(pb.record(T1, FWD, K, read)) == "1 0 2 4 0 4"


def test_reverse_complemented_read_on_a_forward_table_with_two_strands():
    read = pb.revcomp(S1[2:9])
    assert read == "CAGTCAC" and not any(read[i:i + K] in FWD for i in range(4))
    # one strand: nothing found; two strands: window i is found as rc(x) = the reference window at 5 - i, t = 0, s = 1 -> o = 1,
    # start = pos - (W - 1 - i) = (5 - i) - (3 - i) = 2
    assert pb.record(T1, FWD, K, read, 1) == (0, -1, 0, 0, 0, 0, 0)
    cnt, found, anchored = pb.votes(T1, FWD, K, read, 2)
    assert cnt == {(1, 1, 2): 4} and (found, anchored) == (4, 4)
    assert pb.record(T1, FWD, K, read, 2) == (2, 1, 1, 4, 0, 4, 4)


def test_index_with_reverse_complements_and_a_two_strand_table():
    assert T2["ACTG"] == key(1, 5, 0) and T2["CAGT"] == key(1, 5, 1) == (1 << 32) + 11
    assert T2["TCAC"] == key(1, 2, 1) and T2["GTCA"] == key(1, 3, 1) and T2["AGTC"] == key(1, 4, 1)
    assert {x: f for x, f in T2.items() if x in FWD} == T1 and all(f & 1 for x, f in T2.items() if x not in FWD)
    read = "CAGTCAC"
    # one strand: window i hits the column of rc(reference window 5 - i), t = 1, s = 0 -> o = 1, start 2
    assert pb.votes(T2, BOTH, K, read, 1)[0] == {(1, 1, 2): 4}
    assert pb.record(T2, BOTH, K, read, 1) == (2, 1, 1, 4, 0, 4, 4)
    # two strands: the second search hits the forward column, t = 0, s = 1 -> the same placement; eight votes
    assert pb.record(T2, BOTH, K, read, 2) == (2, 1, 1, 8, 0, 8, 8)
    assert pb.record(T2, BOTH, K, S1[2:9], 2) == (2, 1, 0, 8, 0, 8, 8)


def test_read_overhanging_the_start_of_the_reference():
    read = "TT" + S1[:6]
    assert read == "TTCCGTGA" and "TTCC" not in FWD and "TCCG" not in FWD
    cnt, found, anchored = pb.votes(T1, FWD, K, read)
    assert cnt == {(1, 0, -2): 3} and (found, anchored) == (3, 3)
    assert pb.record(T1, FWD, K, read) == (-2, 1, 0, 3, 0, 3, 3)
    assert pb.cli_columns(pb.record(T1, FWD, K, read)) == "1 0 -2 3 0 3"
    # and the end, reverse-complemented: the read covers 5 .. 12 of a reference of 11 bases; window i is rc(reference window
    # 9 - i) for i = 2, 3, 4: start = (9 - i) - (4 - i) = 5
    read = pb.revcomp(S1[5:] + "AA")
    assert read == "TTTCCAGT" and pb.votes(T1, FWD, K, read, 2)[0] == {(1, 1, 5): 3}
    assert pb.record(T1, FWD, K, read, 2) == (5, 1, 1, 3, 0, 3, 3)


def test_a_kmer_of_sequences_0_and_2_twice_in_sequence_0_keeps_the_minimum_key():
    assert S0[0:4] == S0[7:11] == S2[1:5] == "GATT"
    assert T1["GATT"] == key(0, 0) == 0
    assert pb.first_table(FWD, K, [(2, S2, 1)])["GATT"] == key(2, 1) == (2 << 32) + 2
    assert pb.first_table(FWD, K, [(2, S2, 1), (0, S0[7:], 1)])["GATT"] == key(0, 0)
    assert pb.first_table(FWD, K, list(reversed(NUMBERED1))) == T1                # the order of the adds does not show
    assert pb.first_table(FWD, K, NUMBERED1 + NUMBERED1) == T1                    # adding twice changes nothing
    assert pb.first_table(FWD, K, [(3, S1, 1), (1, S1, 1)]) == {x: f for x, f in T1.items() if f >> 32 == 1}   # two numbers: the smaller
    # the projection: sequence 2 read back votes for sequence 0 where sequence 0 holds the k-mer first
    cnt, found, anchored = pb.votes(T1, FWD, K, S2)
    assert cnt == {(2, 0, 0): 2, (0, 0, -1): 1}
    assert pb.record(T1, FWD, K, S2) == (0, 2, 0, 2, 1, 3, 3)


def test_a_palindromic_window_keeps_t_0():
    ref = "AACGTC"
    kmers = bf.kmer_set([ref], K)
    assert pb.revcomp("ACGT") == "ACGT" and kmers == {"AACG", "ACGT", "CGTC"}
    first = pb.first_table(kmers, K, [(0, ref, 2)])
    assert first == {"AACG": key(0, 0), "ACGT": key(0, 1, 0), "CGTC": key(0, 2)}
    assert pb.scalars(kmers, K, [(0, ref, 2)]) == (6, 4)
    # the read ACGT under two strands: two hits on one column, o = 0 and o = 1, one vote each: the tie goes to o = 0
    cnt, found, anchored = pb.votes(first, kmers, K, "ACGT", 2)
    assert cnt == {(0, 0, 1): 1, (0, 1, 1): 1} and (found, anchored) == (2, 2)
    assert pb.record(first, kmers, K, "ACGT", 2) == (1, 0, 0, 1, 1, 2, 2)


def test_chimeric_reads_ties_and_the_runner_up():
    # five votes against four
    read = S0[0:8] + S1[4:11]
    assert read == "GATTACAGGACTGGA"
    assert pb.votes(T1, FWD, K, read)[0] == {(0, 0, 0): 5, (1, 0, -4): 4}
    assert pb.record(T1, FWD, K, read) == (0, 0, 0, 5, 4, 9, 9)
    # four against four: the smaller triple wins, whichever comes first on the read
    read = S0[1:8] + S1[4:11]
    assert pb.votes(T1, FWD, K, read)[0] == {(0, 0, 1): 4, (1, 0, -3): 4}
    assert pb.record(T1, FWD, K, read) == (1, 0, 0, 4, 4, 8, 8)
    read = S1[4:11] + S0[1:8]
    assert pb.votes(T1, FWD, K, read)[0] == {(1, 0, 4): 4, (0, 0, -6): 4}
    assert pb.record(T1, FWD, K, read) == (-6, 0, 0, 4, 4, 8, 8)
    # within one sequence and orientation the smaller start wins, compared as signed: -6 < 1
    read = S1[1:6] + "G" + S1[0:5]
    assert read == "CGTGAGCCGTG" and pb.votes(T1, FWD, K, read)[0] == {(1, 0, 1): 2, (1, 0, -6): 2}
    assert pb.record(T1, FWD, K, read) == (-6, 1, 0, 2, 2, 4, 4)
    # orientation before start: (1, 0, 4) < (1, 1, 0)
    read = S1[4:9] + pb.revcomp(S1[0:5])
    cnt = pb.votes(T1, FWD, K, read, 2)[0]
    assert read == "GACTGCACGG" and cnt == {(1, 0, 4): 2, (1, 1, 0): 2}
    assert pb.record(T1, FWD, K, read, 2)[:5] == (4, 1, 0, 2, 2)


def test_lower_case_n_and_reads_shorter_than_k():
    assert pb.record(T1, FWD, K, "gtgaCTGG") == (2, 1, 0, 1, 0, 1, 1)             # only CTGG is a window of upper-case ACGT
    assert pb.record(T1, FWD, K, "gtgaCTGG", 2) == (2, 1, 0, 1, 0, 1, 1)
    assert pb.record(T1, FWD, K, "GTGANTGG") == (2, 1, 0, 1, 0, 1, 1)             # only GTGA
    assert pb.record(T1, FWD, K, b"GTGA\x00TGGA") == (2, 1, 0, 2, 0, 2, 2)         # bytes: GTGA at 0 and TGGA at 5 agree on start 2
    for short in ("GTG", "", "A"):
        assert pb.record(T1, FWD, K, short, 2) == (0, -1, 0, 0, 0, 0, 0)
    assert pb.cli_columns((0, -1, 0, 0, 0, 0, 0)) == "-1 0 0 0 0 0"
    # lower case and N in a reference: those windows offer nothing, the offsets of the others stay
    first = pb.first_table(FWD, K, [(5, "CCGTnACTGGA", 1)])
    assert first == {"CCGT": key(5, 0), "ACTG": key(5, 5), "CTGG": key(5, 6), "TGGA": key(5, 7)}


def test_hits_without_an_anchor_on_a_partial_table():
    part = pb.first_table(FWD, K, [(1, S1, 1)])
    assert len(part) == 8 and "GATT" not in part
    read = S0[:7]
    assert all(read[i:i + K] in FWD for i in range(4))
    assert pb.record(part, FWD, K, read) == (0, -1, 0, 0, 0, 4, 0)
    # one anchored hit among five found
    read = S0[:7] + "X" + S1[:4]
    assert pb.record(part, FWD, K, read) == (-8, 1, 0, 1, 0, 5, 1)


def test_table_array_and_columns():
    b = bf.BruteSBWT(REFS, K)
    col = pb.columns_of(b)
    arr = pb.table_array(T1, b.nodes)
    assert len(arr) == len(b.nodes) and sum(1 for f in arr if f != pb.NONE) == 18
    assert all(arr[col[x]] == f for x, f in T1.items()) and arr[0] == pb.NONE     # (column 0 is the empty dummy)
    assert pb.n_placements(T1, FWD, K, S2) == 2
