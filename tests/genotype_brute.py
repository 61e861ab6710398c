"""The definition of a genotype object (include/sbwtgpu.h, "genotype") in pure Python, on top of
tests/bubbles_brute.py and tests/unitig_links_brute.py: those give the unitigs, the bubble records and the colours of every
branch from the SET of k-mers; this walks every window of every read (and of its reverse complement for two strands, by the
complement rule of the read-hit profiles), applies the upper-case-ACGT rule, and counts.  Nothing here looks at an index
structure or calls the library.  Also the text `sbwt bubbles -q` and `--refs-out` write.  Tiny inputs only.
"""
from __future__ import annotations

from typing import Dict, FrozenSet, Iterable, List, Optional, Sequence, Tuple

import bubbles_brute as bb
from screen_brute import revcomp
from unitig_links_brute import coordinates

CALL_TEXT = {0: ".", 1: "a", 2: "b", 3: "ab"}


def _text(s) -> str:
    return s.decode("latin-1") if isinstance(s, (bytes, bytearray)) else s


class Genotype:
    """Everything the object holds and derives, for the plain graph (unitigs, records) of an index at k.

      branch_off              2 B + 1: the exclusive prefix sum of n_kmers in slot order (slot 2 i + j = branch j of bubble i)
      kmer_hits               P counters, position branch_off[s] + the k-mer's offset in its branch
      n_windows, n_hits, n_site_hits
    add() may be called any number of times; the derived values are functions that look at the state as it is.
    """

    def __init__(self, unitigs: List[str], recs: List[bb.Record], k: int):
        self.k, self.unitigs, self.recs = k, unitigs, recs
        self.where: Dict[str, Tuple[int, int]] = coordinates(unitigs, k)
        self.slot_of: Dict[int, int] = {}
        self.n_kmers: List[int] = []
        for i, r in enumerate(recs):
            for j in range(2):
                assert r[1 + j] not in self.slot_of                 # a branch belongs to exactly one bubble
                self.slot_of[r[1 + j]] = 2 * i + j
                assert r[4 + j] == len(unitigs[r[1 + j]]) - k + 1
                self.n_kmers.append(r[4 + j])
        self.branch_off = [0]
        for n in self.n_kmers:
            self.branch_off.append(self.branch_off[-1] + n)
        self.P = self.branch_off[-1]
        self.reset()

    def reset(self) -> None:
        self.kmer_hits = [0] * self.P
        self.n_windows = self.n_hits = self.n_site_hits = 0

    def add(self, reads: Iterable, strands: int = 1) -> "Genotype":
        assert strands in (1, 2)
        k = self.k
        for r in reads:
            s = _text(r)
            for i in range(len(s) - k + 1):
                w = s[i:i + k]
                for x in ([w, revcomp(w)] if strands == 2 else [w]):
                    self.n_windows += 1
                    if not all(c in "ACGT" for c in x) or x not in self.where:
                        continue
                    self.n_hits += 1
                    u, o = self.where[x]
                    if u in self.slot_of:
                        self.n_site_hits += 1
                        self.kmer_hits[self.branch_off[self.slot_of[u]] + o] += 1
        return self

    def info(self, n_colors: int = 0) -> dict:
        return {"n_bubbles": len(self.recs), "n_branch_kmers": self.P, "n_windows": self.n_windows, "n_hits": self.n_hits,
                "n_site_hits": self.n_site_hits, "n_colors": n_colors}

    def _branch(self, s: int) -> List[int]:
        return self.kmer_hits[self.branch_off[s]:self.branch_off[s + 1]]

    def branches(self):
        """(seen, hits, min_hits), 2 B entries each"""
        S = range(2 * len(self.recs))
        return ([sum(1 for h in self._branch(s) if h > 0) for s in S], [sum(self._branch(s)) for s in S],
                [min(self._branch(s)) for s in S])

    def calls(self, breadth_ppm: int = 1_000_000, min_depth: int = 1) -> List[int]:
        assert 1 <= breadth_ppm <= 1_000_000 and min_depth >= 0
        seen, hits, _ = self.branches()
        out = []
        for i in range(len(self.recs)):
            c = 0
            for j in range(2):
                s = 2 * i + j
                if seen[s] * 1_000_000 >= breadth_ppm * self.n_kmers[s] and hits[s] >= min_depth * self.n_kmers[s]:
                    c |= 1 << j
            out.append(c)
        return out

    def refs(self, inter: Sequence[Tuple[FrozenSet[int], FrozenSet[int]]], n_colors: int, breadth_ppm: int = 1_000_000,
             min_depth: int = 1):
        """(ref_sites, ref_match, ref_only) from the inter sets of the two branches of every bubble"""
        call = self.calls(breadth_ppm, min_depth)
        sites, match, only = [0] * n_colors, [0] * n_colors, [0] * n_colors
        for i, (ia, ib) in enumerate(inter):
            for c in range(n_colors):
                if (c in ia) == (c in ib) or call[i] == 0:            # not informative, or no call
                    continue
                j = 0 if c in ia else 1
                sites[c] += 1
                match[c] += (call[i] >> j) & 1
                only[c] += call[i] == 1 << j
        return sites, match, only


def inter_sets(colors) -> List[Tuple[FrozenSet[int], FrozenSet[int]]]:
    """bubbles_brute.branch_colors' result -> per bubble (inter a, inter b)"""
    return [(pair[0][0], pair[1][0]) for pair in colors]


def from_kmers(kmers: Iterable[str], k: int) -> Genotype:
    U, _, _, recs = bb.brute_bubbles(kmers, k)
    return Genotype(U, recs, k)


def format_tsv(G: Genotype, n_links: int, colors=None, snps_only: bool = False, breadth_ppm: int = 1_000_000, min_depth: int = 1) -> str:
    """What `sbwt bubbles -q` writes: bubbles_brute.format_tsv with the three scalars on the header and seven fields a line."""
    base = bb.format_tsv(G.unitigs, n_links, G.recs, colors, snps_only).split("\n")[:-1]
    seen, hits, mn = G.branches()
    call = G.calls(breadth_ppm, min_depth)
    out = [base[0] + " windows %d hits %d site_hits %d" % (G.n_windows, G.n_hits, G.n_site_hits)]
    kept = [i for i, r in enumerate(G.recs) if not (snps_only and r[6] != bb.SNP)]
    assert len(kept) == len(base) - 1
    for line, i in zip(base[1:], kept):
        out.append(line + "\t" + "\t".join(str(x) for x in (seen[2 * i], hits[2 * i], mn[2 * i], seen[2 * i + 1], hits[2 * i + 1],
                                                                 mn[2 * i + 1])) + "\t" + CALL_TEXT[call[i]])
    return "\n".join(out) + "\n"


def refs_tsv(sites, match, only) -> str:
    """What --refs-out writes: colour, sites, match, only."""
    return "".join("%d\t%d\t%d\t%d\n" % (c, a, b, d) for c, (a, b, d) in enumerate(zip(sites, match, only)))


def tiles(s: str, length: int, step: int) -> List[str]:
    """Reads of `length` bases every `step` bases over s, and one that ends at its end"""
    starts = list(range(0, max(1, len(s) - length + 1), step))
    if starts[-1] != max(0, len(s) - length):
        starts.append(max(0, len(s) - length))
    return [s[a:a + length] for a in starts]
