"""The definition of the colour matrix and of a read's pseudoalignment record (include/sbwtgpu.h, "colours and
pseudoalignment") in pure Python, from Python sets of k-mer strings: the index's k-mers, and per colour the k-mers given
for it.  Nothing here looks at an index structure; columns come in only through the list of column labels."""
from __future__ import annotations

import re
from typing import Iterable, List, Sequence, Set, Tuple

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s: str) -> str:
    """A <-> T, C <-> G on upper-case characters only; every other character stays what it is."""
    return "".join(COMP.get(c, c) for c in reversed(s))


def _text(s) -> str:
    return s.decode("latin-1") if isinstance(s, (bytes, bytearray)) else s


def windows(seq, k: int) -> List[str]:
    s = _text(seq)
    return [s[i:i + k] for i in range(len(s) - k + 1)]


def valid(w: str) -> bool:
    return all(c in "ACGT" for c in w)


def add(color_sets: List[Set[str]], index_kmers: Set[str], k: int, color: int, seqs: Iterable, strands: int = 1) -> Tuple[int, int]:
    """Colouring: every window of every sequence that the index holds goes into color_sets[color]; with two strands its
    reverse complement too, if the index holds that.  Returns (n_windows, n_hit_windows)."""
    n_windows = n_hit = 0
    for s in seqs:
        for w in windows(s, k):
            n_windows += 1
            if not valid(w):
                continue
            hit = False
            for x in ([w, revcomp(w)] if strands == 2 else [w]):
                if x in index_kmers:
                    color_sets[color].add(x)
                    hit = True
            n_hit += hit
    return n_windows, n_hit


def row_of_kmer(color_sets: Sequence[Set[str]], kmer: str) -> int:
    return sum(1 << c for c, S in enumerate(color_sets) if kmer in S)


def rows_of(index_kmers_in_column_order: Sequence, color_sets: Sequence[Set[str]], index_kmers: Set[str]) -> List[int]:
    """One row per column from the columns' labels ('$' in a label: a dummy column, row 0)."""
    out = []
    for lab in index_kmers_in_column_order:
        lab = _text(lab)
        out.append(row_of_kmer(color_sets, lab) if ("$" not in lab and lab in index_kmers) else 0)
    return out


def window_sets(color_sets: Sequence[Set[str]], index_kmers: Set[str], k: int, read, strands: int = 1) -> List[int]:
    """S_i of every window of the read."""
    out = []
    for w in windows(read, k):
        s = 0
        if valid(w):
            for x in ([w, revcomp(w)] if strands == 2 else [w]):
                if x in index_kmers:
                    s |= row_of_kmer(color_sets, x)
        out.append(s)
    return out


def counts_of(sets: Sequence[int], n_colors: int) -> List[int]:
    return [sum((s >> c) & 1 for s in sets) for c in range(n_colors)]


def record_of(sets: Sequence[int], n_colors: int, threshold_ppm: int, denominator: int) -> Tuple[int, int, int]:
    """(colors, n_kmers, n_found) from the colour sets of a read's windows."""
    m = len(sets)
    n_found = sum(1 for s in sets if s != 0)
    D = m if denominator else n_found
    colors = 0
    for c, cnt in enumerate(counts_of(sets, n_colors)):
        if D > 0 and cnt * 1_000_000 >= threshold_ppm * D:
            colors |= 1 << c
    return colors, m, n_found


def records(color_sets, index_kmers, k, reads, strands=1, threshold_ppm=1_000_000, denominator=0) -> List[Tuple[int, int, int]]:
    n_colors = len(color_sets)
    return [record_of(window_sets(color_sets, index_kmers, k, r, strands), n_colors, threshold_ppm, denominator) for r in reads]


def counts(color_sets, index_kmers, k, reads, strands=1) -> List[List[int]]:
    n_colors = len(color_sets)
    return [counts_of(window_sets(color_sets, index_kmers, k, r, strands), n_colors) for r in reads]


def format_lines(recs: Iterable[Sequence[int]]) -> bytes:
    """What `sbwt pseudoalign` writes: per read its 0-based number and the ids of its colours, ascending."""
    out = []
    for i, rec in enumerate(recs):
        out.append(" ".join([str(i)] + [str(c) for c in range(64) if (int(rec[0]) >> c) & 1]) + "\n")
    return "".join(out).encode()


def parse_ppm(text: str) -> int:
    """`--threshold` as parts per million from its decimal text, without floating point: digits, optionally '.' and digits;
    what follows the sixth decimal must be zeros; the value lies in (0, 1].  ValueError otherwise."""
    if not re.fullmatch(r"[0-9]{1,9}(\.[0-9]+)?", text):
        raise ValueError(text)
    ip, _, fp = text.partition(".")
    if fp[6:].strip("0"):
        raise ValueError(text)
    ppm = int(ip) * 1_000_000 + int((fp[:6] + "000000")[:6])
    if not 1 <= ppm <= 1_000_000:
        raise ValueError(text)
    return ppm
