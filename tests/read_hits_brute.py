"""The definition of a read's hit profile (include/sbwtgpu.h, "per-read hit profiles") in pure Python, from a k-mer set --
that of bruteforce.BruteSBWT, or any set of strings of length k.  covered_bases is literally the size of the union of the
intervals [i, i + k); covered_sum_min is the equivalent sum the header quotes, kept apart so that tests can hold the two
against each other."""
from __future__ import annotations

from typing import Iterable, List, Sequence, Set, Tuple

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s: str) -> str:
    """A <-> T, C <-> G on upper-case characters only; every other character stays what it is."""
    return "".join(COMP.get(c, c) for c in reversed(s))


def hits(kmers: Set[str], k: int, read: str, strands: int = 1) -> List[int]:
    out = []
    for i in range(len(read) - k + 1):
        w = read[i:i + k]
        if any(c not in "ACGT" for c in w):
            out.append(0)                  # a window holding any other byte is no hit on either strand
        else:
            out.append(1 if (w in kmers or (strands == 2 and revcomp(w) in kmers)) else 0)
    return out


def covered_union(hit: Sequence[int], k: int) -> int:
    cov = set()
    for i, h in enumerate(hit):
        if h:
            cov.update(range(i, i + k))
    return len(cov)


def covered_sum_min(hit: Sequence[int], k: int) -> int:
    pos = [i for i, h in enumerate(hit) if h]
    return sum(min(k, pos[j + 1] - pos[j]) for j in range(len(pos) - 1)) + (k if pos else 0)


def longest_run(hit: Sequence[int]) -> int:
    best = cur = 0
    for h in hit:
        cur = cur + 1 if h else 0
        best = max(best, cur)
    return best


def profile_of_hits(hit: Sequence[int], k: int) -> Tuple[int, int, int, int]:
    return (len(hit), sum(hit), covered_union(hit, k), longest_run(hit))


def profile(kmers: Set[str], k: int, read, strands: int = 1) -> Tuple[int, int, int, int]:
    """(n_kmers, n_found, covered_bases, longest_run) of one read (str, or bytes of any values)."""
    if isinstance(read, (bytes, bytearray)):
        read = read.decode("latin-1")
    return profile_of_hits(hits(kmers, k, read, strands), k)


def profiles(kmers: Set[str], k: int, reads: Iterable, strands: int = 1) -> List[Tuple[int, int, int, int]]:
    return [profile(kmers, k, r, strands) for r in reads]


def format_table(rows: Iterable[Sequence[int]]) -> bytes:
    """What `sbwt read-hits` writes: one line per read."""
    return b"".join(b"%d %d %d %d\n" % tuple(int(x) for x in r) for r in rows)
