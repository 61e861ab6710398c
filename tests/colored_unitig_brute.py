"""Definition-level brute force of the coloured unitig export (include/sbwtgpu.h) in pure Python,
written like tests/unitig_brute.py: from the SET of k-mers and a dict k-mer -> frozenset of colours.  The out and in tests
are those of the plain unitigs; the internal-edge and the start rule gain the comparison of the two sets.  Which k-mer
carries which colours is what tests/pseudoalign_brute.py says (`sets_of_references`), so nothing is defined twice.
Tiny inputs only.
"""
from __future__ import annotations

from typing import Dict, FrozenSet, Iterable, List, Sequence, Tuple

import pseudoalign_brute as pb
from bruteforce import BruteSBWT, colex_key

EMPTY: FrozenSet[int] = frozenset()


def sets_of_references(index_kmers: Iterable[str], k: int, references: Sequence[Iterable], strands: int = 1) -> Dict[str, FrozenSet[int]]:
    """k-mer -> its colours, colour c being given the sequences references[c] (pseudoalign_brute.add)."""
    S = set(index_kmers)
    color_sets = [set() for _ in references]
    for c, seqs in enumerate(references):
        pb.add(color_sets, S, k, c, seqs, strands)
    return {x: frozenset(c for c, cs in enumerate(color_sets) if x in cs) for x in S}


def row_of(s: FrozenSet[int]) -> int:
    """The set as a row of the colour matrix (a Python integer, bit c = colour c)."""
    return sum(1 << c for c in s)


def colored_paths(kmers: Iterable[str], k: int, sets: Dict[str, FrozenSet[int]]) -> Tuple[List[List[str]], int]:
    """(paths, n_color_breaks): the coloured unitigs as lists of k-mers in the defined order, and the number of edges
    v -> w with outdeg(v) = 1, indeg(w) = 1 and S(v) != S(w).  A k-mer that `sets` does not name carries the empty set."""
    S = set(kmers)
    col = {x: sets.get(x, EMPTY) for x in S}
    outs: Dict[str, List[str]] = {x: [x[1:] + c for c in "ACGT" if x[1:] + c in S] for x in S}
    ins: Dict[str, List[str]] = {x: [c + x[:-1] for c in "ACGT" if c + x[:-1] in S] for x in S}

    def single_out(x):                   # the target of the one edge out of x that is the one edge into its target, or None
        if len(outs[x]) == 1 and len(ins[outs[x][0]]) == 1:
            return outs[x][0]
        return None

    def internal_out(x):                 # ... and both ends carry the same set
        y = single_out(x)
        return y if y is not None and col[y] == col[x] else None

    def is_start(x):                     # unless exactly one in-neighbour u, outdeg(u) = 1 and S(u) = S(x)
        return not (len(ins[x]) == 1 and len(outs[ins[x][0]]) == 1 and col[ins[x][0]] == col[x])

    n_breaks = sum(1 for x in S if single_out(x) is not None and col[single_out(x)] != col[x])
    order = sorted(S, key=lambda s: colex_key(s, k))
    paths: List[List[str]] = []
    seen = set()
    for x in order:                      # (a coloured internal edge never enters a start, so these walks end by themselves)
        if is_start(x):
            path = [x]
            while internal_out(path[-1]) is not None:
                path.append(internal_out(path[-1]))
            paths.append(path)
            seen.update(path)
    for x in order:                      # what no start reaches lies on a pure cycle of one set: its colex-smallest comes first
        if x not in seen:
            path = [x]
            while internal_out(path[-1]) != x:
                path.append(internal_out(path[-1]))
            paths.append(path)
            seen.update(path)
    assert len(seen) == len(S) == sum(len(p) for p in paths)
    paths.sort(key=lambda p: colex_key(p[0], k))
    return paths, n_breaks


def spell(path: List[str]) -> str:
    return path[0] + "".join(y[-1] for y in path[1:])


def colored_unitigs_of_kmers(kmers: Iterable[str], k: int, sets: Dict[str, FrozenSet[int]]):
    """(unitigs, their sets, n_color_breaks)"""
    paths, n_breaks = colored_paths(kmers, k, sets)
    return [spell(p) for p in paths], [sets.get(p[0], EMPTY) for p in paths], n_breaks


def brute_colored_unitigs(B: BruteSBWT, sets: Dict[str, FrozenSet[int]]):
    """(unitigs, sets, first_col, n_color_breaks) of a brute-force SBWT whose k-mers carry `sets`."""
    U, Z, n_breaks = colored_unitigs_of_kmers(B.kmers, B.k, sets)
    return U, Z, [B.rank_of[u[:B.k]] for u in U], n_breaks


def column_rows(B: BruteSBWT, sets: Dict[str, FrozenSet[int]]) -> List[int]:
    """One integer row per column of B (dummies: 0): the matrix that `sets` means."""
    return [row_of(sets.get(lab, EMPTY)) if len(lab) == B.k else 0 for lab in B.nodes]
