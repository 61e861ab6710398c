"""The definition of a read's hit profile (include/sbwtgpu.h, "per-read hit profiles") in pure Python, from a k-mer set --
that of bruteforce.BruteSBWT, or any set of strings of length k.  covered_bases is literally the size of the union of the
intervals [i, i + k); covered_sum_min is the equivalent sum the header quotes, kept apart so that tests can hold the two
against each other."""
from __future__ import annotations

from typing import Iterable, List, Sequence, Set, Tuple

import numpy as np

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


# ---- a numpy reduction of search results: the sum-of-min form, reads as segments of one array ----
def reduce_hits(hit, oo, k):
    """(n_reads, 4) records from the hit flags of all windows (read r: hit[oo[r]:oo[r + 1]])."""
    n = len(oo) - 1
    W = int(oo[-1])
    m = np.diff(oo)
    out = np.zeros((n, 4), dtype=np.int64)
    out[:, 0] = m
    if W == 0:
        return out.astype(np.int32)
    h = hit.astype(np.int64)
    pos = np.arange(W, dtype=np.int64)
    start = np.repeat(oo[:-1], m)                                 # first window of the read of every window
    cs = np.concatenate([[0], np.cumsum(h)])
    out[:, 1] = cs[oo[1:]] - cs[oo[:-1]]
    last0 = np.maximum.accumulate(np.where(h == 0, pos, -1))      # last miss at or before p
    run = h * (pos - np.maximum(last0, start - 1))                # hits in a row that end at p
    lasthit = np.maximum.accumulate(np.where(h == 1, pos, -1))
    prev = np.concatenate([[-1], lasthit[:-1]])                   # last hit before p
    add = h * np.where(prev >= start, np.minimum(k, pos - prev), k)
    ca = np.concatenate([[0], np.cumsum(add)])
    out[:, 2] = ca[oo[1:]] - ca[oo[:-1]]
    ne = np.nonzero(m > 0)[0]
    out[ne, 3] = np.maximum.reduceat(run, oo[ne])
    return out.astype(np.int32)
