"""The unitig export's definition (include/sbwtgpu.h) over packed k-mers in numpy, for sets too large
for tests/unitig_brute.py (k <= 31: a k-mer is one 64-bit key).

Keys are the builder's: character i of the k-mer at bits 2i, so that ascending keys are ascending colex order, which is the
order of the real columns.  The neighbours of a k-mer are looked up by binary search in the sorted key array; the walk along
the internal edges is a plain loop over Python lists.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_CODE = np.full(256, 4, dtype=np.uint64)
_CODE[ACGT] = np.arange(4, dtype=np.uint64)


def window_keys(seq: np.ndarray, k: int) -> np.ndarray:
    """The keys of the windows of k upper-case ACGT bytes of one sequence (uint8 array), in text order."""
    assert 1 <= k <= 31
    n = len(seq) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint64)
    c = _CODE[seq]
    bad = np.concatenate([[0], np.cumsum(c > 3)])
    v = np.zeros(n, dtype=np.uint64)
    for j in range(k):
        v |= (c[j:j + n] & np.uint64(3)) << np.uint64(2 * j)
    return v[bad[k:] == bad[:-k]]


def key_set(seqs: Sequence[np.ndarray], k: int) -> np.ndarray:
    """The sorted distinct keys of the k-mers of the sequences."""
    parts = [window_keys(np.asarray(s, dtype=np.uint8), k) for s in seqs]
    return np.unique(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.uint64)


def graph(K: np.ndarray, k: int):
    """(nxt, is_start, outdeg, indeg) of the node-centric de Bruijn graph of the sorted keys K: nxt[x] = the index of the target
    of the internal edge out of x (its only out-neighbour, whose only in-neighbour is x) or -1; is_start[x] unless x has
    exactly one in-neighbour whose out-degree is 1."""
    assert 1 <= k <= 31
    n = len(K)
    if n == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, np.zeros(0, dtype=bool), z, z
    mask = np.uint64((1 << (2 * k)) - 1)
    two, top = np.uint64(2), np.uint64(2 * (k - 1))

    def find(q):
        i = np.minimum(np.searchsorted(K, q), n - 1)
        return i, K[i] == q
    outdeg, succ = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for d in range(4):                                   # x[1:] + d
        i, hit = find((K >> two) | (np.uint64(d) << top))
        outdeg += hit
        succ = np.where(hit, i, succ)
    indeg, pred = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for c in range(4):                                   # c + x[:-1]
        i, hit = find(((K << two) & mask) | np.uint64(c))
        indeg += hit
        pred = np.where(hit, i, pred)
    nxt = np.where((outdeg == 1) & (indeg[succ] == 1), succ, -1)
    is_start = ~((indeg == 1) & (outdeg[pred] == 1))
    return nxt, is_start, outdeg, indeg


def unitigs_of_keys(K: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(bases, off, first): the unitigs spelled out as the API returns them (uint8[total], int64[n + 1]) and, per unitig,
    the index into K of its first k-mer -- its rank among the real columns.  Ascending `first`."""
    nxt, is_start, _, _ = graph(K, k)
    n = len(K)
    nl = nxt.tolist()
    seen = bytearray(n)
    paths: List[List[int]] = []
    for x in np.flatnonzero(is_start).tolist():          # (an internal edge never enters a start: these walks end)
        path = [x]
        y = nl[x]
        while y >= 0:
            path.append(y)
            y = nl[y]
        for y in path:
            seen[y] = 1
        paths.append(path)
    for x in range(n):                                   # what no start reaches lies on a pure cycle; ascending: its smallest first
        if not seen[x]:
            path = [x]
            y = nl[x]
            while y != x:
                assert y >= 0 and not seen[y]
                path.append(y)
                y = nl[y]
            for y in path:
                seen[y] = 1
            paths.append(path)
    assert sum(len(p) for p in paths) == n
    paths.sort(key=lambda p: p[0])
    lens = np.array([len(p) for p in paths], dtype=np.int64)
    first = np.array([p[0] for p in paths], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens + (k - 1))]).astype(np.int64)
    bases = np.zeros(int(off[-1]), dtype=np.uint8)
    if n:
        order = np.array([y for p in paths for y in p], dtype=np.int64)
        uid = np.repeat(np.arange(len(paths), dtype=np.int64), lens)
        last = ACGT[((K[order] >> np.uint64(2 * (k - 1))) & np.uint64(3)).astype(np.int64)]
        bases[np.arange(n, dtype=np.int64) + (uid + 1) * (k - 1)] = last        # k-mer t of unitig i ends at t + (i + 1)(k - 1)
        for j in range(k - 1):
            bases[off[:-1] + j] = ACGT[((K[first] >> np.uint64(2 * j)) & np.uint64(3)).astype(np.int64)]
    return bases, off, first
