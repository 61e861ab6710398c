"""Definition-level brute force of the unitig export (include/sbwtgpu.h) in pure Python.

It works from the SET of k-mers: the real columns are the k-mers in colex order, so "ascending column" is "ascending colex
rank" and the smallest column of a cycle is its colex-smallest k-mer.  Out-neighbours of x are the k-mers x[1:] + c,
in-neighbours of y the k-mers c + y[:-1] -- what the suffix groups of the matrix store.  Tiny inputs only.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Tuple

from bruteforce import BruteSBWT, colex_key


def unitigs_of_kmers(kmers: Iterable[str], k: int) -> List[str]:
    """The unitigs of the node-centric de Bruijn graph of `kmers`, each spelled out, in the defined order."""
    S = set(kmers)
    outs: Dict[str, List[str]] = {x: [x[1:] + c for c in "ACGT" if x[1:] + c in S] for x in S}
    ins: Dict[str, List[str]] = {x: [c + x[:-1] for c in "ACGT" if c + x[:-1] in S] for x in S}

    def internal_out(x):                 # the target of the internal edge out of x, or None
        if len(outs[x]) == 1 and len(ins[outs[x][0]]) == 1:
            return outs[x][0]
        return None

    def is_start(x):                     # unless exactly one in-neighbour whose out-degree is 1
        return not (len(ins[x]) == 1 and len(outs[ins[x][0]]) == 1)

    order = sorted(S, key=lambda s: colex_key(s, k))
    paths: List[List[str]] = []
    seen = set()
    for x in order:                      # (an internal edge never enters a start, so these walks end by themselves)
        if is_start(x):
            path = [x]
            while internal_out(path[-1]) is not None:
                path.append(internal_out(path[-1]))
            paths.append(path)
            seen.update(path)
    for x in order:                      # what no start reaches lies on a pure cycle: the colex order meets its smallest first
        if x not in seen:
            path = [x]
            while internal_out(path[-1]) != x:
                path.append(internal_out(path[-1]))
            paths.append(path)
            seen.update(path)
    assert len(seen) == len(S) == sum(len(p) for p in paths)
    paths.sort(key=lambda p: colex_key(p[0], k))
    return [p[0] + "".join(y[-1] for y in p[1:]) for p in paths]


def brute_unitigs(B: BruteSBWT) -> Tuple[List[str], List[int]]:
    """(unitigs, first_col) of a brute-force SBWT: the column of a unitig's first k-mer from its colex order with dummies."""
    U = unitigs_of_kmers(B.kmers, B.k)
    return U, [B.rank_of[u[:B.k]] for u in U]


def flatten(unitigs: List[str]):
    """(bases, off) as the API returns them: bytes, list of len + 1 offsets."""
    off = [0]
    for u in unitigs:
        off.append(off[-1] + len(u))
    return "".join(unitigs).encode(), off
