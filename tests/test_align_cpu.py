"""CPU: the definition of the alignment of mapped reads (tests/align_brute.py; include/sbwtgpu.h, "alignment of mapped reads")
checked against hand-written alignments, the walk over the band of the lemma against the walk over the whole table, and the
properties the header lists.  No GPU and no library call."""
import random

import pytest

import align_brute as ab
import verify_brute as vb
from test_verify_cpu import REFS as VERIFY_REFS, rand_bytes, random_case

#        0         1         2
#        012345678901234567890123
# REFS[0] = GATTACAGGCTCATGCAAGTCCTA, [1] its first 16 with an N at 7, [2] with a lower-case g at 7; [3] matches no C
REFS = VERIFY_REFS + [b"AAAAAAAAAAAA"]

# (what, read, (seq, strand, start), band, ref_begin, CIGAR)
HAND = [
    ("exact", b"ACAGGCTC", (0, 0, 4), 0, 4, "8="),
    ("exact, a band around it", b"ACAGGCTC", (0, 0, 4), 2, 4, "8="),
    ("exact, placed two to the left: the band finds it", b"ACAGGCTC", (0, 0, 2), 2, 4, "8="),
    ("one substitution", b"ACAGCCTC", (0, 0, 4), 0, 4, "4=1X3="),
    ("one substitution, band 2", b"ACAGCCTC", (0, 0, 4), 2, 4, "4=1X3="),
    # REF0[4:8] + T + REF0[8:12]
    ("insertion, band 0", b"ACAGTGCTC", (0, 0, 4), 0, 4, "4=1I4="),
    ("insertion, band 1", b"ACAGTGCTC", (0, 0, 4), 1, 4, "4=1I4="),
    ("insertion, band 2", b"ACAGTGCTC", (0, 0, 4), 2, 4, "4=1I4="),
    # REF0[4:8] + REF0[9:13]: one of the two G at 7, 8 is missing.  Walking back, the diagonal comes first, so the read's G faces
    # coordinate 8 and the deletion is coordinate 7: the leftmost place in the homopolymer.  At band 0 the window ends at 12 and
    # the read's last base faces nothing.
    ("deletion in a homopolymer, band 0", b"ACAGCTCA", (0, 0, 4), 0, 4, "3=1D4=1I"),
    ("deletion in a homopolymer, band 1", b"ACAGCTCA", (0, 0, 4), 1, 4, "3=1D5="),
    ("deletion in a homopolymer, band 2", b"ACAGCTCA", (0, 0, 4), 2, 4, "3=1D5="),
    # REF0[4:8] + G + REF0[8:12]: a third G.  The inserted one is the first of the three in the read.
    ("insertion in a homopolymer", b"ACAGGGCTC", (0, 0, 4), 1, 4, "3=1I5="),
    # REF0[2:6] + REF0[7:13] (A at 6 deleted) with the C at 5 replaced by G: T T A g | G G C T C A.  Walking back, the diagonal
    # comes first: the read's g faces coordinate 6 as X, and the deletion is coordinate 5.
    ("a substitution beside a deletion", b"TTAGGGCTCA", (0, 0, 2), 2, 2, "3=1D1X6="),
    # REF0[2:6] + G + T + REF0[7:13]: two bases where the A at 6 was.  The diagonal comes first, so the T faces coordinate 6 as X
    # and the G before it is the insertion.
    ("a substitution beside an insertion", b"TTACGTGGCTCA", (0, 0, 2), 2, 2, "4=1I1X6="),
    ("overhang at the start: columns left of 0 are X", b"TTGATTAC", (0, 0, -2), 0, -2, "2X6="),
    ("overhang past the end: the smallest end leaves I", b"GTCCTAGG", (0, 0, 18), 0, 18, "6=2I"),
    ("overhang at the start, band 3", b"TTGATTAC", (0, 0, -2), 3, -2, "2X6="),
    ("N in the read", b"ACANGCTC", (0, 0, 4), 0, 4, "3=1X4="),
    ("N in the reference", b"ACAGGCTC", (1, 0, 4), 0, 4, "3=1X4="),
    ("N against N", b"ACANGCTC", (1, 0, 4), 0, 4, "3=1X4="),
    ("lower case in the read", b"ACAgGCTC", (0, 0, 4), 0, 4, "3=1X4="),
    ("lower case in the reference", b"ACAGGCTC", (2, 0, 4), 0, 4, "3=1X4="),
    ("lower case against lower case", b"ACAgGCTC", (2, 0, 4), 0, 4, "3=1X4="),
    ("strand 1", b"GAGCCTGT", (0, 1, 4), 0, 4, "8="),
    ("strand 1, one substitution", b"GAGGCTGT", (0, 1, 4), 3, 4, "4=1X3="),
    ("strand 1, a deletion", vb.rc(b"ACAGCTCA"), (0, 1, 4), 1, 4, "3=1D5="),
    ("one base that matches", b"C", (0, 0, 5), 0, 5, "1="),
    ("one base that does not: the empty substring, so I", b"G", (0, 0, 5), 0, 5, "1I"),
    ("one base that the band finds", b"G", (0, 0, 5), 2, 7, "1="),
    # nothing matches: D[L][0] = L is as good as any column and the smallest, so the read is one run of I at start - B
    ("a read that matches nothing", b"CCCC", (3, 0, 4), 1, 3, "4I"),
    ("a read that matches nothing, band 0", b"CCCC", (3, 0, 4), 0, 4, "4I"),
    ("all of it off the sequence", b"ACAG", (0, 0, (1 << 40) - 1), 1, (1 << 40) - 2, "4I"),
    # only the last base matches.  It matches at every column, and the smallest end is column 1: the three C are I, not X
    ("three I and a match at the window's first column", b"CCCA", (3, 0, 0), 0, 0, "3I1="),
]

# (what, read, (seq, strand, start), band, record)
SPECIAL = [
    ("no bases", b"", (0, 0, 5), 3, (2, 0, 0)),
    ("unverified: seq -1", b"ACAGGCTC", (-1, 0, 4), 0, (0, 0, 0)),
    ("unverified: seq = n_seqs", b"ACAGGCTC", (4, 0, 4), 0, (0, 0, 0)),
    ("unverified: strand 2", b"ACAGGCTC", (0, 2, 4), 0, (0, 0, 0)),
    ("unverified: strand -1", b"ACAGGCTC", (0, -1, 4), 0, (0, 0, 0)),
    ("unverified: start 2^40", b"ACAGGCTC", (0, 0, 1 << 40), 0, (0, 0, 0)),
    ("unverified: start -2^40", b"ACAGGCTC", (0, 0, -(1 << 40)), 0, (0, 0, 0)),
    ("unverified, no bases", b"", (7, 0, 4), 0, (0, 0, 0)),
    ("1025 bases", b"A" * 1025, (0, 0, 0), 8, (0, 0, 0)),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_written_alignments(case):
    _, read, rec, band, begin, cigar = case
    v, a, runs = ab.alignment(REFS, read, rec, band, table=ab.full_table)
    assert (a[0], ab.cigar(runs)) == (begin, cigar)
    assert ab.alignment(REFS, read, rec, band) == (v, a, runs)              # the numpy rows
    assert a[1] == len(runs) and a[2] == sum(n for n, op in runs if op == "=")
    r = vb.orient(read, rec[1])
    assert ab.align_banded(REFS[rec[0]], r, rec[2], band, v[2], v[0]) == (begin, runs)
    assert ab.replay(REFS[rec[0]], r, begin, runs) == v[0]


@pytest.mark.parametrize("case", SPECIAL, ids=[c[0] for c in SPECIAL])
def test_reads_without_an_alignment(case):
    _, read, rec, band, want = case
    v, a, runs = ab.alignment(REFS, read, rec, band)
    assert a == want and runs == []
    assert ab.cli_columns(v, a, runs).endswith(" %d *" % want[0])


def test_the_run_encoding_and_the_columns():
    runs = [(57, "="), (1, "X"), (92, "=")]
    assert ab.encode(runs) == [(57 << 4) | 7, (1 << 4) | 8, (92 << 4) | 7]
    assert ab.decode(ab.encode(runs)) == runs
    assert ab.encode([(2, "I"), (3, "D")]) == [0x21, 0x32]
    assert ab.cigar(runs) == "57=1X92=" and ab.cigar([]) == "*"
    assert ab.cli_columns((1187, 2, 2), (1035, 3, 150), [(80, "="), (2, "D"), (70, "=")]) == "2 2 1187 1035 80=2D70="
    assert ab.cli_columns((0, -1, -1), (0, 0, 0), []) == "-1 -1 0 0 *"
    assert ab.merge(["=", "=", "I", "X", "X"]) == [(2, "X"), (1, "I"), (2, "=")]


def check_properties(ref, read, strand, start, band, others):
    """every property of the header's list, for one read with bases"""
    r = vb.orient(read, strand)
    L = len(r)
    edit, end, begin, runs = ab.align_full(ref, r, start, band, table=ab.full_table)
    assert (edit, end) == vb.sellers_loop(ref, r, start, band)
    assert ab.full_table_numpy(ref, r, start, band).tolist() == ab.full_table(ref, r, start, band)
    count = {op: sum(n for n, o in runs if o == op) for op in "=XID"}
    assert count["="] + count["X"] + count["I"] == L
    assert count["="] + count["X"] + count["D"] == end - begin
    assert count["X"] + count["I"] + count["D"] == edit
    assert runs and runs[0][1] != "D" and runs[-1][1] != "D"
    assert 1 <= len(runs) <= 2 * edit + 1
    assert all(a[1] != b[1] and a[0] > 0 for a, b in zip(runs, runs[1:])) and runs[-1][0] > 0
    if edit == 0:
        assert runs == [(L, "=")] and begin == end - L
    assert begin >= start - band
    assert ab.replay(ref, r, begin, runs) == end
    # the band of the lemma, and any wider one, gives the same walk
    assert ab.align_banded(ref, r, start, band, edit, end) == (begin, runs)
    assert ab.align_banded(ref, r, start, band, edit, end, extra=2) == (begin, runs)
    # through the records: the reverse complement on the other strand, and other neighbours
    v, a, got = ab.alignment([ref], read, (0, strand, start), band)
    assert (v[0], v[2], a, got) == (end, edit, (begin, len(runs), count["="]), runs)
    assert ab.alignment([ref], vb.rc(read), (0, 1 - strand, start), band) == (v, a, got)
    assert ab.alignment(others, read, (1, strand, start), band) == (v, a, got)


def test_the_banded_walk_and_the_properties_on_random_cases():
    rng = random.Random(2901)
    n = 0
    while n < 300:
        ref, read, strand, start, _ = random_case(rng)
        if not read:
            continue
        n += 1
        others = [rand_bytes(rng, rng.randint(0, 9)), ref, rand_bytes(rng, rng.randint(0, 9))]
        for band in range(0, 6):
            check_properties(ref, read, strand, start, band, others)


def test_a_narrower_band_than_the_lemma_s_can_lose_the_walk():
    """the lemma's width is needed: two deleted bases and one diagonal either side, and the band no longer holds the path"""
    ref, r = REFS[0], vb.orient(b"TTACAGTCATGCAA", 0)      # REF0[2:8] + REF0[10:18]; the read's G faces coordinate 8, not 7
    edit, end, begin, runs = ab.align_full(ref, r, 2, 2)
    assert (edit, end, begin, ab.cigar(runs)) == (2, 18, 2, "5=1D1=1D8=")
    tE = end - (2 - 2)
    assert ab.banded_table(ref, r, 2, 2, 2, tE)[(len(r), tE)] == edit
    assert ab.banded_table(ref, r, 2, 2, 1, tE)[(len(r), tE)] > edit
