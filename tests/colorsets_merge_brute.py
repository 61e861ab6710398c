"""The definition of sbwtgpu_colorsets_merge (include/sbwtgpu.h, "colour sets carried onto another index") in pure Python,
written from sets of k-mer strings: the colour sets of one or two coloured indexes carried onto the columns of a third.  Rows
are Python integers of any width, as in tests/colorsets_brute.py, whose canonical() gives the result its form.  Beside it, a
word-level restatement of the shifted OR that the device computes, on (n_sets, W) uint64 arrays.  Nothing here needs a GPU."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import colorsets_brute as cb
import pseudoalign_wide as pw

MAX_COLORS = 4096


def n_colors_out(n_colors_a: int, n_colors_b: Optional[int], offset: int) -> int:
    return n_colors_a if n_colors_b is None else max(n_colors_a, offset + n_colors_b)


def rows(kmers_u_by_column: Sequence[str], dummy_u: Sequence[bool], colouring_a: Dict[str, int],
         colouring_b: Optional[Dict[str, int]], offset: int) -> List[int]:
    """The row of every column of u: S_a(x) | S_b(x) << offset for a real column of k-mer x, 0 for a dummy column.  A colouring
    maps every k-mer of its index to its row (an integer, 0 = no colour); a k-mer it lacks has the empty set."""
    out = []
    for x, dummy in zip(kmers_u_by_column, dummy_u):
        if dummy:
            out.append(0)
        else:
            out.append(colouring_a.get(x, 0) | ((colouring_b.get(x, 0) << offset) if colouring_b is not None else 0))
    return out


def merge(kmers_u_by_column: Sequence[str], dummy_u: Sequence[bool], colouring_a: Dict[str, int],
          colouring_b: Optional[Dict[str, int]], offset: int) -> Tuple[List[int], List[int]]:
    """(ids, table) of the merged object: the canonical form of rows()."""
    return cb.canonical(rows(kmers_u_by_column, dummy_u, colouring_a, colouring_b, offset))


def counts(kmers_u_by_column: Sequence[str], dummy_u: Sequence[bool], ids_a: Dict[str, int], ids_b: Optional[Dict[str, int]]) -> dict:
    """The info counts but n_sets: ids_a / ids_b map every k-mer of a / b to the id its column has in the input object."""
    real = [x for x, d in zip(kmers_u_by_column, dummy_u) if not d]
    in_a = [x in ids_a for x in real]
    in_b = [ids_b is not None and x in ids_b for x in real]
    pairs = {(ids_a.get(x, 0), ids_b.get(x, 0) if ids_b is not None else 0) for x in real}
    pairs.discard((0, 0))
    return {"n_real_u": len(real), "n_from_a": sum(in_a), "n_from_b": sum(in_b), "n_from_both": sum(p and q for p, q in zip(in_a, in_b)),
            "n_pairs": len(pairs)}


def colouring_of(labels: Sequence[str], ids: Sequence[int], table: Sequence[int]) -> Dict[str, int]:
    """k-mer -> row of a colour-set object (ids per column, integer table rows) over an index with these column labels"""
    return {lab: table[i] for lab, i in zip(labels, ids) if "$" not in lab}


def ids_of(labels: Sequence[str], ids: Sequence[int]) -> Dict[str, int]:
    return {lab: int(i) for lab, i in zip(labels, ids) if "$" not in lab}


# ---- the shifted OR, word by word ------------------------------------------------------------------------------------
def shift_rows(tb: np.ndarray, offset: int, words_out: int) -> np.ndarray:
    """(n, words_out) uint64: every row of tb ((n, Wb) uint64) moved up by `offset` bits.  With offset = 64 q + s, word w takes
    tb[w - q] << s and, for s != 0, tb[w - q - 1] >> (64 - s); words outside tb's width are 0."""
    tb = np.asarray(tb, dtype=np.uint64)
    n, wb = tb.shape
    q, s = offset >> 6, offset & 63
    out = np.zeros((n, words_out), dtype=np.uint64)
    for w in range(words_out):
        j = w - q
        if 0 <= j < wb:
            out[:, w] |= tb[:, j] << np.uint64(s)
        if s != 0 and 0 <= j - 1 < wb:
            out[:, w] |= tb[:, j - 1] >> np.uint64(64 - s)
    return out


def pair_rows(ta: np.ndarray, tb: Optional[np.ndarray], pairs: Sequence[Tuple[int, int]], offset: int, words_out: int) -> np.ndarray:
    """(len(pairs), words_out) uint64: row (id_a, id_b) = ta[id_a] | tb[id_b] shifted up by offset"""
    ta = np.asarray(ta, dtype=np.uint64)
    out = np.zeros((len(pairs), words_out), dtype=np.uint64)
    out[:, :ta.shape[1]] = ta[[p[0] for p in pairs]]                     # (words_out >= ta's width: n_colors_out >= n_colors_a)
    if tb is not None:
        out |= shift_rows(np.asarray(tb, dtype=np.uint64)[[p[1] for p in pairs]], offset, words_out)
    return out


def merge_arrays(kmers_u_by_column, dummy_u, colouring_a, colouring_b, offset, n_colors):
    """merge() as the arrays the C ABI holds: (ids uint32[n], table uint64[n_sets, W])"""
    ids, table = merge(kmers_u_by_column, dummy_u, colouring_a, colouring_b, offset)
    return np.array(ids, dtype=np.uint32), pw.rows_array(table, pw.n_words(n_colors))
