"""The definition of the shared k-mer matrix (include/sbwtgpu.h, "shared k-mers") twice over, neither looking at an index
structure:

  * from a colour-set object's arrays: size[t] = #{ j : ids[j] = t }, w = size unless weights are given, w[0] ignored,
    G[a][b] = the sum of w[t] over the sets t >= 1 whose row holds colours a and b -- shared() in pure Python integers,
    shared_np() the same in numpy for the sizes a GPU test uses;
  * from Python sets of k-mer strings: G[a][b] = |K_a & K_b| restricted to the index's k-mers -- shared_of_kmers().

Plus what `sbwt color-matrix` writes: tsv(), and jaccard_ppm() in Python integers."""
from __future__ import annotations

from typing import List, Optional, Sequence, Set

import numpy as np


def set_sizes(ids, n_sets: int) -> List[int]:
    out = [0] * n_sets
    for t in ids:
        out[int(t)] += 1
    return out


def shared(ids, rows: Sequence[int], n_colors: int, weights: Optional[Sequence[int]] = None) -> List[List[int]]:
    """rows: one Python integer per table row, colour c = bit c."""
    w = list(weights) if weights is not None else set_sizes(ids, len(rows))
    assert len(w) == len(rows)
    G = [[0] * n_colors for _ in range(n_colors)]
    for t in range(1, len(rows)):
        held = [c for c in range(n_colors) if (rows[t] >> c) & 1]
        for a in held:
            for b in held:
                G[a][b] += int(w[t])
    return G


def bits_of(table: np.ndarray, n_colors: int) -> np.ndarray:
    """(n_sets, W) uint64 -> (n_sets, n_colors) of 0 / 1, colour c = bit c & 63 of word c >> 6"""
    table = np.ascontiguousarray(table, dtype="<u8")
    return np.unpackbits(table.view(np.uint8), axis=1, bitorder="little")[:, :n_colors]


def shared_np(ids, table: np.ndarray, n_colors: int, weights=None) -> np.ndarray:
    """int64 (n_colors, n_colors).  The product runs in int64; where that would take long it runs in float64, which is exact
    here and checked to be: every entry and every partial sum is a non-negative integer of at most sum(w) < 2^53."""
    n_sets = len(table)
    w = np.bincount(np.asarray(ids, dtype=np.int64), minlength=n_sets).astype(np.int64) if weights is None \
        else np.array(weights, dtype=np.int64)
    assert w.shape == (n_sets,) and (w[1:] >= 0).all()
    w = w.copy()
    w[0] = 0
    B = bits_of(table, n_colors)
    if n_sets * n_colors * n_colors <= 50_000_000:
        Bi = B.astype(np.int64)
        return (Bi * w[:, None]).T @ Bi
    assert int(w.sum()) < 2**53
    Bf = B.astype(np.float64)
    G = (Bf * w[:, None].astype(np.float64)).T @ Bf
    out = G.astype(np.int64)
    assert (out == G).all()
    return out


def shared_of_kmers(color_sets: Sequence[Set[str]], index_kmers: Set[str]) -> List[List[int]]:
    K = [S & index_kmers for S in color_sets]
    return [[len(a & b) for b in K] for a in K]


def jaccard_ppm(G) -> List[List[int]]:
    """floor(10^6 G[a][b] / (G[a][a] + G[b][b] - G[a][b])), 0 where the denominator is 0"""
    n = len(G)
    out = [[0] * n for _ in range(n)]
    for a in range(n):
        for b in range(n):
            den = int(G[a][a]) + int(G[b][b]) - int(G[a][b])
            out[a][b] = int(G[a][b]) * 1_000_000 // den if den > 0 else 0
    return out


def tsv(G, jaccard: bool = False) -> bytes:
    M = jaccard_ppm(G) if jaccard else G
    return "".join("\t".join(str(int(x)) for x in row) + "\n" for row in M).encode()
