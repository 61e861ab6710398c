"""CPU: the definition of read verification (tests/verify_brute.py; include/sbwtgpu.h, "reference sequences and verification")
checked against hand-written records, its numpy form against the plain double loop, and the properties the header lists.  No
GPU and no library call."""
import random

import pytest

import verify_brute as vb

#        0         1         2
#        012345678901234567890123
REF0 = b"GATTACAGGCTCATGCAAGTCCTA"
REF1 = b"GATTACANGCTCATGC"                  # REF0[:16] with an N at 7
REF2 = b"GATTACAgGCTCATGC"                  # ... with a lower-case g at 7
REFS = [REF0, REF1, REF2]

# (what, read, (seq, strand, start), band, (ref_end, mismatches, edit))
HAND = [
    ("exact", b"ACAGGCTC", (0, 0, 4), 0, (12, 0, 0)),
    ("exact, a band around it", b"ACAGGCTC", (0, 0, 4), 2, (12, 0, 0)),
    ("one substitution", b"ACAGCCTC", (0, 0, 4), 0, (12, 1, 1)),
    ("one substitution, band 2", b"ACAGCCTC", (0, 0, 4), 2, (12, 1, 1)),
    # REF0[4:8] + T + REF0[8:12]: everything behind the inserted base is off the diagonal, the alignment ends where it should
    ("insertion, band 0", b"ACAGTGCTC", (0, 0, 4), 0, (12, 5, 1)),
    ("insertion, band 1", b"ACAGTGCTC", (0, 0, 4), 1, (12, 5, 1)),
    ("insertion, band 2", b"ACAGTGCTC", (0, 0, 4), 2, (12, 5, 1)),
    # REF0[4:8] + REF0[9:13]: the read's last base lies at coordinate 12, one past the window of band 0
    ("deletion, band 0", b"ACAGCTCA", (0, 0, 4), 0, (12, 4, 2)),
    ("deletion, band 1", b"ACAGCTCA", (0, 0, 4), 1, (13, 4, 1)),
    ("deletion, band 2", b"ACAGCTCA", (0, 0, 4), 2, (13, 4, 1)),
    ("overhang at the start", b"TTGATTAC", (0, 0, -2), 0, (6, 2, 2)),
    ("overhang past the end", b"GTCCTAGG", (0, 0, 18), 0, (24, 2, 2)),
    ("N in the read", b"ACANGCTC", (0, 0, 4), 0, (12, 1, 1)),
    ("N in the reference", b"ACAGGCTC", (1, 0, 4), 0, (12, 1, 1)),
    ("N against N", b"ACANGCTC", (1, 0, 4), 0, (12, 1, 1)),
    ("lower case in the read", b"ACAgGCTC", (0, 0, 4), 0, (12, 1, 1)),
    ("lower case in the reference", b"ACAGGCTC", (2, 0, 4), 0, (12, 1, 1)),
    ("lower case against lower case", b"ACAgGCTC", (2, 0, 4), 0, (12, 1, 1)),
    ("strand 1", b"GAGCCTGT", (0, 1, 4), 0, (12, 0, 0)),
    ("strand 1, one substitution", b"GAGGCTGT", (0, 1, 4), 3, (12, 1, 1)),
    ("no bases", b"", (0, 0, 5), 3, (2, 0, 0)),
    ("one base that matches", b"C", (0, 0, 5), 0, (6, 0, 0)),
    ("one base that matches, band 2", b"C", (0, 0, 5), 2, (6, 0, 0)),
    ("one base that does not: the empty substring is as good", b"G", (0, 0, 5), 0, (5, 1, 1)),
    ("one base that the band finds", b"G", (0, 0, 5), 2, (8, 1, 0)),
    ("unverified: seq -1", b"ACAGGCTC", (-1, 0, 4), 0, (0, -1, -1)),
    ("unverified: seq = n_seqs", b"ACAGGCTC", (3, 0, 4), 0, (0, -1, -1)),
    ("unverified: strand 2", b"ACAGGCTC", (0, 2, 4), 0, (0, -1, -1)),
    ("unverified: strand -1", b"ACAGGCTC", (0, -1, 4), 0, (0, -1, -1)),
    ("unverified: start 2^40", b"ACAGGCTC", (0, 0, 1 << 40), 0, (0, -1, -1)),
    ("unverified: start -2^40", b"ACAGGCTC", (0, 0, -(1 << 40)), 0, (0, -1, -1)),
    ("unverified, no bases", b"", (7, 0, 4), 0, (0, -1, -1)),
    ("the largest start: all of it off the sequence", b"ACAG", (0, 0, (1 << 40) - 1), 1, ((1 << 40) - 2, 4, 4)),
    # 7 of REF0's bases are A; no table for 1025 bases
    ("1025 bases", b"A" * 1025, (0, 0, 0), 8, (0, 1018, -1)),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_written_records(case):
    _, read, rec, band, want = case
    assert vb.record(REFS, read, rec, band, table=vb.sellers_loop) == want
    assert vb.record(REFS, read, rec, band) == want


def test_what_the_object_stores():
    assert vb.stored(b"ACGTNacgt\x00T") == b"ACGTNNNNNNT"
    assert vb.n_invalid([b"ACGTNacgt\x00T", b"", b"NN"]) == 8
    bits, val = vb.packed_words(b"ACGTN" + b"T" * 60)
    assert len(bits) == 4 and len(val) == 2                # 65 bases: two units of 64
    assert bits[0] & 0x3ff == 0b0011100100                  # A 0, C 1, G 2, T 3, the N's field zero
    assert val[0] == (1 << 64) - 1 - (1 << 4) and val[1] == 1
    assert bits[2] == 3 and bits[3] == 0                    # base 64 is T; padding is zero
    assert vb.packed_words(b"") == ([], [])


def test_the_oriented_read():
    assert vb.orient(b"ACGTNa", 0) == [65, 67, 71, 84, None, None]
    assert vb.orient(b"ACGTNa", 1) == [None, None, 65, 67, 71, 84]
    assert vb.rc(b"AACGNt") == b"tNCGTT"
    assert vb.cli_columns((12, 3, 2)) == "3 2 12"


def rand_bytes(rng, n, alphabet=b"ACGT", junk=0.0):
    return bytes(rng.choice(b"Nacgt\x00") if rng.random() < junk else rng.choice(alphabet) for _ in range(n))


def random_case(rng):
    """a short reference, a read cut from it (or not) and mutated, a record near its origin (or not)"""
    ref = rand_bytes(rng, rng.randint(0, 40), rng.choice([b"ACGT", b"AC", b"A"]), rng.choice([0.0, 0.1]))
    L = rng.randint(0, 14)
    if len(ref) >= L and rng.random() < 0.7:
        at = rng.randint(0, len(ref) - L)
        read = bytearray(ref[at:at + L])
    else:
        at = rng.randint(-5, 30)
        read = bytearray(rand_bytes(rng, L))
    for _ in range(rng.randint(0, 2)):
        if read and rng.random() < 0.5:
            read[rng.randrange(len(read))] = rng.choice(b"ACGTN")
        elif read and rng.random() < 0.5:
            del read[rng.randrange(len(read))]
        else:
            read.insert(rng.randint(0, len(read)), rng.choice(b"ACGT"))
    strand = rng.randint(0, 1)
    read = bytes(read)
    if strand:
        read = vb.rc(read)
    return ref, read, strand, at + rng.randint(-3, 3), rng.randint(0, 6)


def test_numpy_rows_equal_the_double_loop():
    rng = random.Random(2801)
    for _ in range(400):
        ref, read, strand, start, band = random_case(rng)
        r = vb.orient(read, strand)
        assert vb.sellers_numpy(ref, r, start, band) == vb.sellers_loop(ref, r, start, band), (ref, read, strand, start, band)


def occurs(ref, r, lo, hi):
    """whether the oriented read matches base for base somewhere in [lo, hi)"""
    return any(all(vb.matches(ref, s + j, rj) for j, rj in enumerate(r)) for s in range(lo, hi - len(r) + 1))


def test_properties_that_follow_from_the_definition():
    rng = random.Random(2802)
    for _ in range(300):
        ref, read, strand, start, _ = random_case(rng)
        others = [rand_bytes(rng, rng.randint(0, 9)), ref, rand_bytes(rng, rng.randint(0, 9))]
        prev = None
        for band in range(0, 6):
            end, mm, edit = vb.record([ref], read, (0, strand, start), band)
            assert 0 <= edit <= mm <= len(read)                                     # edit <= mismatches for every band
            assert prev is None or edit <= prev                                     # non-increasing in the band
            prev = edit
            if read:
                r = vb.orient(read, strand)
                assert (edit == 0) == occurs(ref, r, start - band, start + len(read) + band)
            assert start - band <= end <= start + len(read) + band
            # the reverse complement on the other strand is the same oriented read
            assert vb.record([ref], vb.rc(read), (0, 1 - strand, start), band) == (end, mm, edit)
            # the neighbours in the object do not matter
            assert vb.record(others, read, (1, strand, start), band) == (end, mm, edit)
