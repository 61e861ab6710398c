"""Definition-level brute force of the bubbles of the plain unitig graph (include/sbwtgpu.h, "bubbles")
in pure Python, on top of tests/unitig_links_brute.py: that gives the unitigs and their links from the SET of k-mers, this
applies the definition of a bubble to (unitigs, link_off, link_to) word for word, cuts the alleles, and reduces the colours of
every branch from a dictionary k-mer -> frozenset of colours.  Also the planted-SNP inputs the CPU and GPU tests share, and
the text `sbwt bubbles` writes.  Tiny inputs only.
"""
from __future__ import annotations

import random
from typing import Dict, FrozenSet, Iterable, List, Tuple

from unitig_links_brute import brute_links, coordinates

OTHER, SNP = 0, 1
Record = Tuple[int, int, int, int, int, int, int]          # source, branch a, branch b, sink, n_kmers a, n_kmers b, kind


def in_degrees(n_unitigs: int, link_to: List[int]) -> List[int]:
    """in-degree of unitig j: the number of entries of link_to equal to j"""
    deg = [0] * n_unitigs
    for j in link_to:
        deg[j] += 1
    return deg


def bubbles(unitigs: List[str], link_off: List[int], link_to: List[int], k: int) -> List[Record]:
    """The records by ascending source."""
    n = len(unitigs)
    indeg = in_degrees(n, link_to)

    def out(i):
        return link_to[link_off[i]:link_off[i + 1]]
    recs = []
    for s in range(n):
        if len(out(s)) != 2:                                # outdeg(s) = 2, links in CSR order a, b
            continue
        a, b = out(s)
        assert a != b                                       # (the graph's own invariant)
        if indeg[a] != 1 or indeg[b] != 1 or len(out(a)) != 1 or len(out(b)) != 1:
            continue
        t = out(a)[0]
        if out(b)[0] != t or indeg[t] != 2:
            continue
        if a in (s, t) or b in (s, t):
            continue
        na, nb = len(unitigs[a]) - k + 1, len(unitigs[b]) - k + 1
        recs.append((s, a, b, t, na, nb, SNP if na == k and nb == k else OTHER))
    return recs


def alleles(unitigs: List[str], rec: Record) -> Tuple[str, str]:
    """the last n_kmers characters of each branch: what its k-mers add"""
    return unitigs[rec[1]][-rec[4]:], unitigs[rec[2]][-rec[5]:]


def branch_colors(unitigs: List[str], recs: List[Record], k: int, sets: Dict[str, FrozenSet[int]]):
    """Per record ((inter_a, uni_a), (inter_b, uni_b)) as frozensets: AND and OR of the k-mers' sets over each branch.  A
    k-mer that `sets` does not name carries the empty set."""
    where = coordinates(unitigs, k)
    on: Dict[int, List[str]] = {}
    for x, (i, _) in where.items():
        on.setdefault(i, []).append(x)
    out = []
    for rec in recs:
        pair = []
        for br in rec[1:3]:
            mine = [sets.get(x, frozenset()) for x in on[br]]
            assert len(mine) == len(unitigs[br]) - k + 1 >= 1
            pair.append((frozenset.intersection(*mine), frozenset.union(*mine)))
        out.append(tuple(pair))
    return out


def brute_bubbles(kmers: Iterable[str], k: int):
    """(unitigs, link_off, link_to, records) of the plain graph of the k-mer set"""
    U, lo, lt, _ = brute_links(kmers, k)
    return U, lo, lt, bubbles(U, lo, lt, k)


def row_words(s: FrozenSet[int], words: int) -> List[int]:
    v = sum(1 << c for c in s)
    return [(v >> (64 * w)) & (2**64 - 1) for w in range(words)]


def format_tsv(unitigs: List[str], n_links: int, recs: List[Record], colors=None, snps_only: bool = False) -> str:
    """What `sbwt bubbles` writes: the header, then one line per bubble; colors = branch_colors(...) adds the two colour fields."""
    def field(inter, uni):
        def lst(s):
            return ",".join(str(c) for c in sorted(s)) if s else "-"
        return lst(inter) + ("|" + lst(uni) if uni != inter else "")
    lines = ["# unitigs %d links %d bubbles %d snps %d" % (len(unitigs), n_links, len(recs), sum(1 for r in recs if r[6] == SNP))]
    for i, r in enumerate(recs):
        if snps_only and r[6] != SNP:
            continue
        f = [str(x) for x in r[:6]] + ["SNP" if r[6] == SNP else "OTHER"] + list(alleles(unitigs, r))
        if colors is not None:
            f += [field(*colors[i][0]), field(*colors[i][1])]
        lines.append("\t".join(f))
    return "\n".join(lines) + "\n"


# ---- planted SNPs ---------------------------------------------------------------------------------------------------------------
def planted(k: int, length: int, n_snps: int, seed: int):
    """(g, h, sites): a random genome g drawn base by base, and h = g with n_snps single-base substitutions placed evenly, at
    least 2k apart and 2k from the ends; sites = [(position, base of g, base of h)]."""
    rng = random.Random(seed)
    g = [rng.choice("ACGT") for _ in range(length)]
    step = (length - 4 * k) // n_snps
    assert step >= 2 * k
    h, sites = list(g), []
    for i in range(n_snps):
        p = 2 * k + i * step
        h[p] = rng.choice([c for c in "ACGT" if c != g[p]])
        sites.append((p, g[p], h[p]))
    return "".join(g), "".join(h), sites


def snp_bases(unitigs: List[str], recs: List[Record]) -> List[Tuple[str, str]]:
    """The variant bases (allele[0] of each branch) of the SNP records, as sorted pairs, sorted"""
    return sorted(tuple(sorted(a[0] for a in alleles(unitigs, r))) for r in recs if r[6] == SNP)
