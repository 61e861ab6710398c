"""The definition of a screen (include/sbwtgpu.h, "screen") in pure Python, from Python sets of k-mer strings: the index's
k-mers, per reference (colour) the k-mers it holds, and the sample's reads.  Nothing here looks at an index structure or
calls the library.

The sample M is the multiset of the windows of the reads; a window with a byte other than upper-case A/C/G/T never hits; with
two strands M also holds the reverse complement of every window, so a window is two occurrences (a palindromic one two
occurrences of one k-mer).  An occurrence that is an index k-mer is a HIT on it.  Index k-mers are grouped by their colour row
(a Python integer, colour c = bit c); a colour-set object's set t stands for the row table[t], and set 0 also carries the
dummy columns, which are columns of the index but no k-mers."""
from __future__ import annotations

from collections import Counter
from typing import Dict, Iterable, List, Sequence, Set

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s: str) -> str:
    """A <-> T, C <-> G on upper-case characters only; every other character stays what it is."""
    return "".join(COMP.get(c, c) for c in reversed(s))


def _text(s) -> str:
    return s.decode("latin-1") if isinstance(s, (bytes, bytearray)) else s


def sample(reads: Iterable, k: int, strands: int = 1) -> Counter:
    """The multiset M as a Counter of window strings, invalid windows (which count but never hit) under the key None."""
    M: Counter = Counter()
    for r in reads:
        s = _text(r)
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            for x in ([w, revcomp(w)] if strands == 2 else [w]):
                M[x if all(c in "ACGT" for c in x) else None] += 1
    return M


def row_of(color_sets: Sequence[Set[str]], kmer: str) -> int:
    return sum(1 << c for c, S in enumerate(color_sets) if kmer in S)


class Screen:
    """Everything the object holds and derives, for index k-mers `index_kmers`, references `color_sets` (only their index
    k-mers count) and the sample of `reads`.

      n_windows, n_hits, n_seen
      seen_kmers              the index k-mers with at least one hit
      hits_of                 Counter: index k-mer -> its hits
      row_kmers, row_seen, row_hits   dicts: colour row -> the index k-mers that carry it, those seen, the hits on them
      ref_kmers, ref_seen, ref_hits   lists over the colours
    """

    def __init__(self, index_kmers: Set[str], color_sets: Sequence[Set[str]], k: int, reads: Iterable, strands: int = 1):
        M = sample(reads, k, strands)
        self.n_colors = len(color_sets)
        self.n_windows = sum(M.values())
        self.hits_of = Counter({x: n for x, n in M.items() if x is not None and x in index_kmers})
        self.n_hits = sum(self.hits_of.values())
        self.seen_kmers = set(self.hits_of)
        self.n_seen = len(self.seen_kmers)
        self.row = {x: row_of(color_sets, x) for x in index_kmers}
        self.row_kmers: Dict[int, int] = Counter(self.row.values())
        self.row_seen: Dict[int, int] = Counter(self.row[x] for x in self.seen_kmers)
        self.row_hits: Dict[int, int] = Counter()
        for x, n in self.hits_of.items():
            self.row_hits[self.row[x]] += n
        C = self.n_colors
        self.ref_kmers = [sum(n for r, n in self.row_kmers.items() if (r >> c) & 1) for c in range(C)]
        self.ref_seen = [sum(n for r, n in self.row_seen.items() if (r >> c) & 1) for c in range(C)]
        self.ref_hits = [sum(n for r, n in self.row_hits.items() if (r >> c) & 1) for c in range(C)]

    def sets(self, table_rows: Sequence[int], n_dummies: int = 0):
        """(set_kmers, set_seen, set_hits) for an object whose table rows are the given integers, pairwise distinct with row
        0 = 0: set 0 also counts the n_dummies dummy columns among its k-mers."""
        assert table_rows[0] == 0 and len(set(table_rows)) == len(table_rows)
        assert set(self.row_kmers) <= set(table_rows)
        km = [self.row_kmers.get(r, 0) for r in table_rows]
        km[0] += n_dummies
        return km, [self.row_seen.get(r, 0) for r in table_rows], [self.row_hits.get(r, 0) for r in table_rows]

    def seen_bitmap(self, labels: Sequence) -> List[int]:
        """The bitmap's words from the columns' labels in column order ('$' in a label: a dummy column, never seen)."""
        words = [0] * ((len(labels) + 63) // 64)
        for v, lab in enumerate(labels):
            if _text(lab) in self.seen_kmers:
                words[v >> 6] |= 1 << (v & 63)
        return words


def from_arrays(ids, rows: Sequence[int], n_colors: int, results: Iterable[int]):
    """The same from a colour-set object's arrays and the search results of the sample's occurrences (a column, or a negative
    number for a miss): the per-set vectors follow the ids as they are, duplicate rows included.  Returns a dict."""
    n_sets = len(rows)
    set_kmers, set_seen, set_hits = [0] * n_sets, [0] * n_sets, [0] * n_sets
    for t in ids:
        set_kmers[int(t)] += 1
    hits = Counter(int(v) for v in results)
    n_windows = sum(hits.values())
    seen = sorted(v for v in hits if v >= 0)
    for v in seen:
        set_seen[int(ids[v])] += 1
        set_hits[int(ids[v])] += hits[v]

    def ref(vec):
        return [sum(vec[t] for t in range(1, n_sets) if (rows[t] >> c) & 1) for c in range(n_colors)]

    return {"n_windows": n_windows, "n_hits": sum(set_hits), "n_seen": len(seen), "seen": seen, "set_kmers": set_kmers,
            "set_seen": set_seen, "set_hits": set_hits, "ref_kmers": ref(set_kmers), "ref_seen": ref(set_seen),
            "ref_hits": ref(set_hits)}


def screen_tsv(S: "Screen") -> bytes:
    """What `sbwt screen` writes to -o."""
    out = ["# windows %d hits %d seen %d\n" % (S.n_windows, S.n_hits, S.n_seen)]
    for c in range(S.n_colors):
        out.append("%d\t%d\t%d\t%d\n" % (c, S.ref_kmers[c], S.ref_seen[c], S.ref_hits[c]))
    return "".join(out).encode()


def sets_tsv(set_kmers, set_seen, set_hits) -> bytes:
    """What `sbwt screen` writes to --sets-out."""
    return "".join("%d\t%d\t%d\t%d\n" % (t, a, b, c) for t, (a, b, c) in enumerate(zip(set_kmers, set_seen, set_hits))).encode()
