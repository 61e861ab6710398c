"""The definition of a colour-set object (include/sbwtgpu.h, "colour sets") in pure Python: one id per column and a table
of the distinct rows, rows being Python integers of any width as in tests/pseudoalign_brute.py.  Records and counts of a
query are those of the matrix the object means, so they stay with tests/pseudoalign_brute.py and
tests/pseudoalign_wide.py (re-exported here as pb and pw).  Nothing here needs a GPU."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

import pseudoalign_brute as pb          # noqa: F401  (records and counts of the matrix an object means)
import pseudoalign_wide as pw


def canonical(rows: Sequence[int]) -> Tuple[List[int], List[int]]:
    """(ids, table) of integer rows: the distinct non-zero rows numbered 1, 2, ... by first occurrence, row 0 the empty set."""
    ids, table, seen = [], [0], {0: 0}
    for r in rows:
        if r not in seen:
            seen[r] = len(table)
            table.append(r)
        ids.append(seen[r])
    return ids, table


def expand(ids: Sequence[int], table: Sequence[int]) -> List[int]:
    """The rows an object means."""
    return [table[i] for i in ids]


def check_invariants(ids: Sequence[int], table: Sequence[int], n_colors: int, dummy: Sequence[bool] = ()) -> None:
    """AssertionError naming the invariant that (ids, table) breaks; dummy[j] says that column j is a dummy column."""
    assert len(table) >= 1, "n_sets >= 1"
    assert table[0] == 0, "row 0 of the table is not all zero"
    for r, row in enumerate(table):
        assert r == 0 or row != 0, "row %d of the table is all zero" % r
        assert 0 <= row < (1 << n_colors), "row %d of the table has a bit >= n_colors" % r
    for j, i in enumerate(ids):
        assert 0 <= i < len(table), "the id of column %d is not below n_sets" % j
    for j, d in enumerate(dummy):
        assert not d or ids[j] == 0, "dummy column %d has id %d" % (j, ids[j])


def arrays(ids: Sequence[int], table: Sequence[int], n_colors: int):
    """(ids uint32[n], table uint64[n_sets, W]) as the C ABI and the files hold them"""
    return np.array(ids, dtype=np.uint32), pw.rows_array(table, pw.n_words(n_colors))


def canonical_arrays(matrix) -> Tuple[np.ndarray, np.ndarray]:
    """canonical() of an (n, W) uint64 matrix, as arrays"""
    matrix = np.asarray(matrix, dtype=np.uint64)
    ids, table = canonical(pw.rows_ints(matrix))
    return np.array(ids, dtype=np.uint32), pw.rows_array(table, matrix.shape[1])
