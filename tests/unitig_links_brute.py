"""Definition-level brute force of the unitig graph (include/sbwtgpu.h) in pure Python, on top of
tests/unitig_brute.py and tests/colored_unitig_brute.py: those give the unitigs from the SET of k-mers, this adds the links
between them and the coordinate of every k-mer.  One dictionary k-mer -> (unitig, offset) serves both: the target of a link
is the unitig on which the out-neighbour lies, and the definition says it lies there at offset 0.  Tiny inputs only.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Tuple

from colored_unitig_brute import colored_unitigs_of_kmers
from unitig_brute import unitigs_of_kmers


def coordinates(unitigs: List[str], k: int) -> Dict[str, Tuple[int, int]]:
    """k-mer -> (number of its unitig, position of the k-mer in the spelling)"""
    where = {u[r:r + k]: (i, r) for i, u in enumerate(unitigs) for r in range(len(u) - k + 1)}
    assert len(where) == sum(len(u) - k + 1 for u in unitigs)            # every k-mer lies on one unitig, once
    return where


def links_of_unitigs(unitigs: List[str], kmers: Iterable[str], k: int):
    """(link_off, link_to, where): the links of the unitigs of the k-mer set in CSR form, by source and within a source by
    edge character; `where` is coordinates()."""
    S = set(kmers)
    where = coordinates(unitigs, k)
    assert set(where) == S
    link_off, link_to = [0], []
    for u in unitigs:
        last = u[-k:]
        for c in "ACGT":
            y = last[1:] + c
            if y in S:
                j, r = where[y]
                assert r == 0, (u, y)                                    # every target is a first k-mer
                link_to.append(j)
        link_off.append(len(link_to))
    return link_off, link_to, where


def n_edges(kmers: Iterable[str]) -> int:
    """The pairs (x, x[1:] + c) with both k-mers in the set."""
    S = set(kmers)
    return sum(1 for x in S for c in "ACGT" if x[1:] + c in S)


def brute_links(kmers: Iterable[str], k: int):
    """(unitigs, link_off, link_to, where) of the plain run."""
    U = unitigs_of_kmers(kmers, k)
    return (U,) + links_of_unitigs(U, kmers, k)


def brute_colored_links(kmers: Iterable[str], k: int, sets):
    """(unitigs, link_off, link_to, where) of the coloured run under `sets` (k-mer -> frozenset of colours)."""
    U = colored_unitigs_of_kmers(kmers, k, sets)[0]
    return (U,) + links_of_unitigs(U, kmers, k)


def column_map(B, where) -> Tuple[List[int], List[int]]:
    """(col_unitig, col_offset) per column of the brute-force SBWT B; 0xFFFFFFFF for a dummy."""
    NONE = 0xFFFFFFFF
    pairs = [where[lab] if len(lab) == B.k else (NONE, NONE) for lab in B.nodes]
    return [p[0] for p in pairs], [p[1] for p in pairs]
