"""What the tests of wide colour matrices (more than 64 colours, include/sbwtgpu.h "wide colour matrices") share.  The
definition stays tests/pseudoalign_brute.py, whose rows are Python integers of any width; here are
  - integer row <-> W little-endian 64-bit words,
  - `sbwt pseudoalign`'s lines for any number of colours,
  - a small pan-genome case with its colour inputs, probe reads and the trap reads a wide reduction can get wrong,
  - the expected records and counts of many reads at thousands of colours without visiting every colour of every window
    (checked against the brute force in tests/test_pseudoalign_wide_cpu.py).
Nothing here needs a GPU."""
from __future__ import annotations

import random
from typing import Dict, Iterable, List, Optional, Sequence, Set

import numpy as np

import pseudoalign_brute as pb

MASK64 = (1 << 64) - 1
N_COLORS = (1, 64, 65, 127, 128, 129, 200, 4096)
K_WIDE = 13


def n_words(n_colors: int) -> int:
    return (n_colors + 63) // 64


def row_to_words(row: int, words: int) -> List[int]:
    """Colour c is bit c & 63 of word c >> 6."""
    assert 0 <= row < (1 << (64 * words)), (row, words)
    return [(row >> (64 * w)) & MASK64 for w in range(words)]


def words_to_row(words: Iterable[int]) -> int:
    return sum(int(x) << (64 * w) for w, x in enumerate(words))


def rows_array(rows: Sequence[int], words: int) -> np.ndarray:
    """(len(rows), words) uint64 from integer rows"""
    return np.array([row_to_words(r, words) for r in rows], dtype=np.uint64).reshape(len(rows), words)


def rows_ints(arr) -> List[int]:
    return [words_to_row(r) for r in np.asarray(arr).tolist()]


def format_lines(colour_sets: Iterable[int]) -> bytes:
    """What `sbwt pseudoalign` writes: per read its 0-based number and the ids of its colours, ascending."""
    out = []
    for i, s in enumerate(colour_sets):
        s = int(s)
        ids = [c for c in range(s.bit_length()) if (s >> c) & 1]
        out.append(" ".join([str(i)] + [str(c) for c in ids]) + "\n")
    return "".join(out).encode()


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


class Case:
    """A pan-genome of three 400-base strains, a stretch given for no colour and four stretches X, Y, Z, P for the traps,
    indexed at k = 13 with or without reverse complements.  inputs: colour -> sequences (at most a dozen colours; 0, 63, 64 and
    n_colors - 1 among them where they exist), all added with `strands_add` strands."""

    def __init__(self, n_colors: int, rc: bool, seed: int = 5):
        rng = random.Random(seed)
        self.n_colors, self.rc, self.k, self.words = n_colors, rc, K_WIDE, n_words(n_colors)
        base = rand_seq(rng, 400)
        strains = [base]
        for _ in range(2):
            s = list(base)
            for _ in range(12):
                s[rng.randrange(len(s))] = rng.choice("ACGT")
            strains.append("".join(s))
        self.strains = strains
        self.extra = rand_seq(rng, 120)
        self.X, self.Y, self.Z, self.P = (rand_seq(rng, 90) for _ in range(4))
        self.seqs = strains + [self.extra, self.X, self.Y, self.Z, self.P]
        # a reverse-complement index is coloured one strand at a time, so that a k-mer and its reverse complement can carry
        # different colours (the two-strand trap)
        self.strands_add = 1 if rc else 2
        last = n_colors - 1
        # a second colour in the last word, where that word holds more than one: X gets it, so that in the last word the rows
        # of X and of Y are both non-zero and different
        self.last2 = last - 1 if last >= 65 and (last - 1) >> 6 == last >> 6 else None
        inputs: Dict[int, List[str]] = {}

        def give(c, *seqs):
            if 0 <= c < n_colors:
                inputs.setdefault(c, []).extend(seqs)
        give(0, strains[0], self.X, self.Y, self.P)
        give(1, strains[1])
        give(2, strains[2][:250])
        give(63, strains[2])
        give(64, strains[1])
        give(last, self.Y, self.Z, pb.revcomp(self.P))
        if self.last2 is not None:
            give(self.last2, self.X)
        crng = random.Random(1000 + n_colors)
        for c in sorted(crng.sample(range(n_colors), min(5, n_colors))):      # a few colours anywhere: pieces of the strains
            s = strains[c % 3]
            a = crng.randrange(0, 300)
            give(c, s[a:a + crng.randint(20, 100)], "ACGTN", "")
        assert len(inputs) <= 12
        self.inputs = inputs

    def index_kmers(self) -> Set[str]:
        from bruteforce import kmer_set
        return kmer_set(list(self.seqs) + ([pb.revcomp(s) for s in self.seqs] if self.rc else []), self.k)

    def colour_sets(self, kmers: Set[str]):
        """The brute force's colouring: (color_sets, {colour: (n_windows, n_hit_windows)})."""
        cs = [set() for _ in range(self.n_colors)]
        got = {c: pb.add(cs, kmers, self.k, c, seqs, self.strands_add) for c, seqs in sorted(self.inputs.items())}
        return cs, got

    # ---- the trap reads (None where the matrix has one word a row) ----
    def trap_equal_word0(self) -> Optional[bytes]:
        """Fewer than 64 windows, so one wave iteration: those inside X carry colour 0 and, where the last word holds two
        colours, the last but one; those inside Y colour 0 and the last colour -- rows that agree in word 0 and differ in the
        last word (both non-zero there where it holds two colours, zero against non-zero otherwise)."""
        return (self.X[:30] + self.Y[:30]).encode() if self.words > 1 else None

    def trap_last_word_only(self) -> Optional[bytes]:
        """Every hit's row is zero in word 0 and non-zero in the last word only (Z is given for the last colour alone)."""
        return self.Z[:50].encode() if self.words > 1 else None

    def trap_two_strands(self) -> Optional[bytes]:
        """Reverse-complement index, two strands: a window of P has its forward hit on a row with colour 0 (word 0) and its
        reverse-complement hit on a row with the last colour (word W - 1)."""
        return self.P[:60].encode() if self.words > 1 and self.rc else None

    def reads(self) -> List[bytes]:
        """Probe reads: exactly m in {0, 1, 63, 64, 65, 129} windows, a read of at least 5 000 windows with colours changing
        inside iterations, the traps, pieces with substitutions, N and lower case, reverse complements."""
        rng = random.Random(11)
        k, st = self.k, self.strains
        reads = [b"", b"A", st[0][:k - 1].encode(), b"N" * (k + 2), st[1][:k].encode()]
        assert len(reads[2]) - k + 1 == 0 and len(reads[4]) - k + 1 == 1
        for m in (63, 64, 65, 129):
            for s in (st[1], self.extra + st[2], self.Y + self.Z + st[0]):
                a = rng.randrange(0, len(s) - (m + k - 1) + 1)
                reads.append(s[a:a + m + k - 1].encode())
                assert len(reads[-1]) - k + 1 == m
            reads.append(pb.revcomp(st[0][:m + k - 1]).encode())
        long_read = (st[0] + self.Z + st[1][:333] + rand_seq(rng, 700) + pb.revcomp(st[2]) + self.extra + "N" + self.Y + st[2] * 3 +
                     self.X + pb.revcomp(self.P) + rand_seq(rng, 900) + st[1] * 3 + self.P + st[0][17:])
        assert len(long_read) - k + 1 >= 5000
        reads.append(long_read.encode())
        reads += [t for t in (self.trap_equal_word0(), self.trap_last_word_only(), self.trap_two_strands()) if t is not None]
        for s in self.seqs:
            reads += [s.encode(), pb.revcomp(s).encode()]
            for _ in range(2):
                a = rng.randrange(0, len(s))
                piece = list(s[a:a + rng.randint(0, k + 40)])
                for _ in range(rng.randint(0, 3)):
                    if piece:
                        piece[rng.randrange(len(piece))] = rng.choice("ACGTNacgt")
                reads.append("".join(piece).encode())
        return reads


class Expected:
    """Window sets, counts and records of reads as tests/pseudoalign_brute.py defines them, arranged for thousands of colours:
    a k-mer's row comes from pb.row_of_kmer once, and counts visit only the colours that occur in the read."""

    def __init__(self, color_sets, index_kmers: Set[str], k: int):
        self.n_colors, self.k, self.kmers = len(color_sets), k, index_kmers
        self.row = {x: pb.row_of_kmer(color_sets, x) for x in index_kmers}

    def window_sets(self, read, strands: int = 1) -> List[int]:
        out = []
        for w in pb.windows(read, self.k):
            s = 0
            if pb.valid(w):
                for x in ([w, pb.revcomp(w)] if strands == 2 else [w]):
                    s |= self.row.get(x, 0)
            out.append(s)
        return out

    def counts_of(self, sets: Sequence[int]) -> List[int]:
        out = [0] * self.n_colors
        seen = 0
        for s in sets:
            seen |= s
        for c in range(seen.bit_length()):
            if (seen >> c) & 1:
                out[c] = sum((s >> c) & 1 for s in sets)
        return out

    def record_of(self, sets: Sequence[int], threshold_ppm: int, denominator: int):
        """(colors, n_kmers, n_found), colors an integer of n_colors bits"""
        m = len(sets)
        n_found = sum(1 for s in sets if s != 0)
        D = m if denominator else n_found
        colors = 0
        for c, cnt in enumerate(self.counts_of(sets)):
            if cnt and D > 0 and cnt * 1_000_000 >= threshold_ppm * D:
                colors |= 1 << c
        return colors, m, n_found
