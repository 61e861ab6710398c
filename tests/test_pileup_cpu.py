"""CPU: the definition of the pileup (tests/pileup_brute.py) on hand-written cases, every record written out, and its listed
properties on random cases.  No device."""
import random

import pytest

import align_brute as ab
import pileup_brute as pb
import verify_brute as vb

#          0         1         2
#          0123456789012345678901234
REF = b"ACGTTGCAAGGCTTACCGATAGCTA"


def rec(depth=0, A=0, C=0, G=0, T=0, d=0, i=0, o=0):
    return (depth, A, C, G, T, d, i, o)


def match(ref, p):
    """the record of one = column at p"""
    r = [1, 0, 0, 0, 0, 0, 0, 0]
    r[1 + pb.CODE[ref[p]]] = 1
    return tuple(r)


def pile_one(refs, read, record, band=2, votes=pb.JUNK_VOTES, filt=pb.NO_FILTER):
    p = pb.Pile(refs)
    v, a, runs = ab.alignment(refs, read, record, band)
    p.add_alignment(read, record, votes, v, a, runs, filt)
    return p, (v, a, runs)


def table(p, seq=0):
    """{pos: record} of the bases that hold anything"""
    return {q: c for q, c in enumerate(p.counts(seq)) if c != pb.EMPTY}


def test_one_exact_read():
    p, (v, a, runs) = pile_one([REF], REF[5:13], (0, 0, 5))
    assert runs == [(8, "=")] and (a[0], v[0]) == (5, 13)
    assert table(p) == {5: rec(1, G=1), 6: rec(1, C=1), 7: rec(1, A=1), 8: rec(1, A=1), 9: rec(1, G=1), 10: rec(1, G=1), 11: rec(1, C=1),
                        12: rec(1, T=1)}
    assert p.scalars() == dict(n_offered=1, n_piled=1, n_columns=8, n_clipped=0, n_overhang=0)
    assert p.calls() == []


def test_one_substitution_on_either_strand():
    read = bytearray(REF[5:13])
    read[3] = ord("C")                                      # reference coordinate 8 holds A
    want = {5: rec(1, G=1), 6: rec(1, C=1), 7: rec(1, A=1), 8: rec(1, C=1), 9: rec(1, G=1), 10: rec(1, G=1), 11: rec(1, C=1), 12: rec(1, T=1)}
    p, (_, _, runs) = pile_one([REF], bytes(read), (0, 0, 5))
    assert runs == [(3, "="), (1, "X"), (4, "=")] and table(p) == want
    assert p.calls() == [(8, 0, 1, 0, 1, 1, 0)]
    # strand 1: the read as sequenced is the reverse complement, and holds G where the oriented read holds C
    back = vb.rc(bytes(read))
    assert back[len(back) - 1 - 3] == ord("G")
    p, (_, _, runs) = pile_one([REF], back, (0, 1, 5))
    assert runs == [(3, "="), (1, "X"), (4, "=")] and table(p) == want      # the COMPLEMENTED base at coordinate 8: C, not G
    assert p.calls() == [(8, 0, 1, 0, 1, 1, 0)]


def test_a_deletion_and_an_insertion_with_its_anchor():
    read = REF[3:9] + REF[10:16]                            # coordinate 9 (G) is missing from the read
    p, (v, a, runs) = pile_one([REF], read, (0, 0, 3))
    assert (a[0], v[0]) == (3, 16) and sum(n for n, op in runs if op == "D") == 1
    t = table(p)
    at = [q for q, c in t.items() if c[pb.N_DEL]]
    assert len(at) == 1 and t[at[0]] == rec(1, d=1) and at[0] in (9, 10)       # (G at 9 and 10: the walk's order picks one)
    assert all(t[q] == match(REF, q) for q in range(3, 16) if q != at[0]) and len(t) == 13
    assert p.calls() == [(at[0], 0, pb.DEL, 2, 1, 1, 0)]
    assert p.scalars() == dict(n_offered=1, n_piled=1, n_columns=13, n_clipped=0, n_overhang=0)
    read = REF[3:9] + b"T" + REF[9:15]                      # a T between coordinates 8 (A) and 9 (G)
    p, (v, a, runs) = pile_one([REF], read, (0, 0, 3))
    assert runs == [(6, "="), (1, "I"), (6, "=")] and (a[0], v[0]) == (3, 15)
    t = table(p)
    assert t[8] == rec(1, A=1, i=1)                         # the anchor: the column before the run
    assert all(t[q] == match(REF, q) for q in range(3, 15) if q != 8) and len(t) == 12
    assert p.calls() == [(8, 0, pb.INS, 0, 1, 1, 1)]
    assert p.scalars() == dict(n_offered=1, n_piled=1, n_columns=12, n_clipped=0, n_overhang=0)


def test_an_insertion_behind_the_last_base_and_clips():
    n = len(REF)
    # the alignment is given: the walk's own tie rules would make this I run a trailing clip
    p = pb.Pile([REF])
    read = REF[n - 4:n] + b"GG" + b"A"
    runs = [(4, "="), (2, "I"), (1, "X")]
    p.add_alignment(read, (0, 0, n - 4), pb.JUNK_VOTES, (n + 1, 3, 3), (n - 4, 3, 4), runs)
    assert table(p) == {n - 4: match(REF, n - 4), n - 3: match(REF, n - 3), n - 2: match(REF, n - 2), n - 1: rec(1, A=1, i=1)}
    assert p.scalars() == dict(n_offered=1, n_piled=1, n_columns=4, n_clipped=0, n_overhang=1)      # the X column at n
    # a leading and a trailing I run
    p = pb.Pile([REF])
    p.add_alignment(b"TT" + REF[4:9] + b"CCC", (0, 0, 2), pb.JUNK_VOTES, (9, 5, 5), (4, 3, 5), [(2, "I"), (5, "="), (3, "I")])
    assert table(p) == {q: match(REF, q) for q in range(4, 9)}
    assert p.scalars() == dict(n_offered=1, n_piled=1, n_columns=5, n_clipped=5, n_overhang=0)
    # an interior I run whose anchor lies before coordinate 0
    p = pb.Pile([REF])
    p.add_alignment(b"T" + b"GG" + REF[0:3], (0, 0, -1), pb.JUNK_VOTES, (3, 3, 3), (-1, 3, 3), [(1, "X"), (2, "I"), (3, "=")])
    assert table(p) == {q: match(REF, q) for q in range(0, 3)}
    assert p.scalars() == dict(n_offered=1, n_piled=1, n_columns=3, n_clipped=0, n_overhang=2) and p.overhang_columns == 1


def test_reads_overhanging_either_end():
    n = len(REF)
    p, (v, a, runs) = pile_one([REF], b"TT" + REF[0:6], (0, 0, -2), band=0)
    assert a[0] == -2 and runs == [(2, "X"), (6, "=")]
    assert table(p) == {q: match(REF, q) for q in range(0, 6)}
    assert p.scalars() == dict(n_offered=1, n_piled=1, n_columns=6, n_clipped=0, n_overhang=2)
    p = pb.Pile([REF])
    p.add_alignment(REF[n - 5:n] + b"AC", (0, 0, n - 5), pb.JUNK_VOTES, (n + 2, 2, 2), (n - 5, 2, 5), [(5, "="), (2, "X")])
    assert table(p) == {q: match(REF, q) for q in range(n - 5, n)}
    assert p.scalars() == dict(n_offered=1, n_piled=1, n_columns=5, n_clipped=0, n_overhang=2)
    pb.check_properties(p, 7)


def test_n_in_the_read_and_in_the_reference():
    read = bytearray(REF[5:13])
    read[3] = ord("N")
    for strand, rd in ((0, bytes(read)), (1, vb.rc(bytes(read)))):
        p, (_, _, runs) = pile_one([REF], rd, (0, strand, 5))
        assert runs == [(3, "="), (1, "X"), (4, "=")]
        assert table(p)[8] == rec(1, o=1) and p.calls() == []          # `other` is no allele
    ref = bytearray(REF)
    ref[8], ref[10] = ord("N"), ord("g")
    p, (_, _, runs) = pile_one([bytes(ref)], REF[5:13], (0, 0, 5))
    assert runs == [(3, "="), (1, "X"), (1, "="), (1, "X"), (2, "=")]
    t = table(p)
    assert t[8] == rec(1, A=1) and t[10] == rec(1, G=1)     # only what the X columns gave
    assert p.calls() == []                                  # no call at an invalid reference base
    assert "0\t8\tN\t1\t1\t0\t0\t0\t0\t0\t0\n" in p.pile_tsv() and "0\t10\tN\t1\t0\t0\t1\t0\t0\t0\t0\n" in p.pile_tsv()


def test_a_read_that_matches_nothing_is_all_clip():
    p, (v, a, runs) = pile_one([b"A" * 20], b"CCCCC", (0, 0, 5))
    assert runs == [(5, "I")] and v[2] == 5
    assert table(p) == {} and p.scalars() == dict(n_offered=1, n_piled=1, n_columns=0, n_clipped=5, n_overhang=0)


def test_each_filter_field_at_its_boundary():
    read = bytearray(REF[5:13])
    read[3] = ord("C")
    read = bytes(read)
    cases = [((7, 0, -1), (7, 0), True), ((8, 0, -1), (7, 0), False), ((0, 1, -1), (7, 6), True), ((0, 1, -1), (7, 7), False),
             ((0, 0, -1), (7, 7), True), ((0, 0, 1), (7, 0), True), ((0, 0, 0), (7, 0), False), ((0, 0, -1), (0, 0), True),
             ((-3, 0, -7), (-2, 5), True)]
    for filt, votes, want in cases:
        p, _ = pile_one([REF], read, (0, 0, 5), votes=votes, filt=filt)
        assert (p.n_piled, p.n_offered, bool(p.base)) == (int(want), 1, want), (filt, votes)
    # seq outside the pileup's sequences, an unverified record, an empty read: offered only
    for record, rd, n_seqs in (((1, 0, 5), read, 1), ((-1, 0, 5), read, 1), ((0, 2, 5), read, 1), ((0, 0, 5), b"", 1)):
        p = pb.Pile([REF, REF], n_seqs)
        assert p.add([rd], [record], 2) == [False] and p.scalars() == dict(n_offered=1, n_piled=0, n_columns=0, n_clipped=0, n_overhang=0)


def test_the_call_thresholds_at_equality():
    p = pb.Pile([REF])
    alt = bytearray(REF[5:13])
    alt[3] = ord("C")
    for i in range(8):
        p.add([bytes(alt) if i < 3 else REF[5:13]], [(0, 0, 5)], 2)
    assert p.record(0, 8) == rec(8, A=5, C=3)
    call = (8, 0, 1, 0, 8, 3, 5)
    assert p.calls() == [call] and p.calls(8, 3, 375000) == [call]             # 3 * 10^6 == 375000 * 8
    assert p.calls(8, 3, 375001) == [] and p.calls(9, 1, 0) == [] and p.calls(1, 4, 0) == []
    assert p.calls(1, 1, 10 ** 6) == [] and p.calls(8, 3, 0) == [call]
    assert p.calls_tsv(8, 3, 375000) == p.header_line() + "0\t8\tA\tC\t8\t3\n"
    assert p.header_line() == "# n_seqs=1 total_bases=25 n_offered=8 n_piled=8 n_columns=64 n_clipped=0 n_overhang=0\n"


def random_case(rng):
    refs = []
    for n in (rng.choice((1, 63, 64, 65, 128)), rng.randrange(40, 200)):
        s = bytearray(rng.choice(b"ACGT") for _ in range(n))
        for _ in range(rng.randrange(0, 3)):
            s[rng.randrange(n)] = rng.choice(b"Nacgt")
        refs.append(bytes(s))
    reads, recs = [], []
    for _ in range(rng.randrange(1, 9)):
        seq = rng.randrange(2)
        ref, L = refs[seq], rng.randrange(1, 40)
        at = rng.randrange(-5, len(ref) + 3)
        piece = bytearray(ref[max(at, 0):max(at, 0) + L].ljust(L, b"A")[:L])
        for _ in range(rng.randrange(0, 3)):
            q = rng.randrange(len(piece))
            kind = rng.randrange(3)
            if kind == 0:
                piece[q] = rng.choice(b"ACGTN")
            elif kind == 1 and len(piece) > 1:
                del piece[q]
            else:
                piece.insert(q, rng.choice(b"ACGT"))
        strand = rng.randrange(2)
        reads.append(vb.rc(bytes(piece)) if strand else bytes(piece))
        recs.append((seq, strand, at + rng.randrange(-2, 3)))
    return refs, reads, recs, rng.choice((0, 2, 5))


def test_the_listed_properties_on_random_cases():
    rng = random.Random(30)
    for case in range(300):
        refs, reads, recs, band = random_case(rng)
        alns = ab.alignments(refs, reads, recs, band)
        p = pb.Pile(refs)
        piled = p.add(reads, recs, band, alns=alns)
        pb.check_properties(p, sum(v[0] - a[0] for (v, a, _), ok in zip(alns, piled) if ok))
        for (seq, q), c in p.base.items():
            if not vb.valid(refs[seq][q]):
                assert c[pb.DEPTH] == sum(c[1:5]) + c[pb.N_DEL] + c[pb.N_OTHER]    # only X and D columns: add_alignment asserts every =
        # (rc(read), 1 - strand) piles as (read, strand)
        q = pb.Pile(refs)
        q.add([vb.rc(rd) for rd in reads], [(s, 1 - o, st) for s, o, st in recs], band)
        assert (q.base, q.scalars()) == (p.base, p.scalars()), case
        calls = p.calls()
        assert calls == sorted(calls, key=lambda c: (c[1], c[0], c[2]))


def test_invariance_under_splitting_and_shuffling():
    rng = random.Random(31)
    for case in range(40):
        refs, reads, recs, band = random_case(rng)
        whole = pb.Pile(refs)
        whole.add(reads, recs, band)
        order = list(range(len(reads)))
        rng.shuffle(order)
        parts = pb.Pile(refs)
        cut = rng.randrange(0, len(order) + 1)
        for piece in (order[:cut], order[cut:]):
            parts.add([reads[i] for i in piece], [recs[i] for i in piece], band)
        assert (parts.base, parts.scalars(), parts.calls(1, 1, 0)) == (whole.base, whole.scalars(), whole.calls(1, 1, 0))
        assert parts.pile_tsv() == whole.pile_tsv()
