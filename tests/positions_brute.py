"""The definition of the position table and of a read's map record (include/sbwtgpu.h, "positions") in pure Python, from
strings: the index's k-mers as a set, the reference sequences with the numbers the caller gave them, and the reads.  Nothing
here looks at an index structure or calls the library.

A key is (seq << 32) | (pos << 1) | t.  A window holding a byte other than upper-case A/C/G/T never hits, on either strand.
A placement is the triple (seq, o, start); a record is the tuple (start, seq, strand, votes, votes2, n_found, n_anchored)."""
from __future__ import annotations

from collections import Counter
from typing import Dict, Iterable, List, Optional, Sequence, Set, Tuple

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
NONE = 0xFFFFFFFFFFFFFFFF
EMPTY = (0, -1, 0, 0, 0)          # (start, seq, strand, votes, votes2) of a read without an anchored hit


def revcomp(s: str) -> str:
    """A <-> T, C <-> G on upper-case characters only; every other character stays what it is."""
    return "".join(COMP.get(c, c) for c in reversed(s))


def _text(s) -> str:
    return s.decode("latin-1") if isinstance(s, (bytes, bytearray)) else s


def valid(w: str) -> bool:
    return all(c in "ACGT" for c in w)


def key(seq: int, pos: int, t: int) -> int:
    return (seq << 32) | (pos << 1) | t


def decode(f: int) -> Tuple[int, int, int]:
    """(seq, pos, t) of a key"""
    return f >> 32, (f & 0xFFFFFFFF) >> 1, f & 1


def first_table(index_kmers: Set[str], k: int, numbered: Iterable[Tuple[int, object, int]]) -> Dict[str, int]:
    """k-mer -> the minimum of the keys offered to it, over the (sequence number, sequence, strands) triples.  Only k-mers of
    the index get a position."""
    first: Dict[str, int] = {}
    for seq, s, strands in numbered:
        s = _text(s)
        for pos in range(len(s) - k + 1):
            x = s[pos:pos + k]
            if not valid(x):
                continue
            for t, y in ((0, x), (1, revcomp(x)))[:strands]:
                if y in index_kmers:
                    f = key(seq, pos, t)
                    if f < first.get(y, NONE):
                        first[y] = f
    return first


def table_array(first: Dict[str, int], labels: Sequence[str]) -> List[int]:
    """first[] in column order from the columns' labels ('$' in a label: a dummy column, never positioned)"""
    return [first.get(_text(lab), NONE) for lab in labels]


def columns_of(brute) -> Dict[str, int]:
    """k-mer -> column from a bruteforce.BruteSBWT"""
    return {x: brute.rank_of[x] for x in brute.kmers}


def votes(first: Dict[str, int], index_kmers: Set[str], k: int, read, strands: int = 1):
    """(Counter of placements, n_found, n_anchored) of one read"""
    s = _text(read)
    W = len(s) - k + 1
    cnt: Counter = Counter()
    found = anchored = 0
    for i in range(max(W, 0)):
        x = s[i:i + k]
        if not valid(x):
            continue
        for sidx, y in ((0, x), (1, revcomp(x)))[:strands]:
            if y not in index_kmers:
                continue
            found += 1
            f = first.get(y, NONE)
            if f == NONE:
                continue
            anchored += 1
            seq, pos, t = decode(f)
            o = sidx ^ t
            cnt[(seq, o, pos - i if o == 0 else pos - (W - 1 - i))] += 1
    return cnt, found, anchored


def record_of_votes(cnt: Counter, found: int, anchored: int):
    if anchored == 0:
        return EMPTY + (found, 0)
    best = max(cnt.values())
    win = min(p for p, c in cnt.items() if c == best)
    rest = [c for p, c in cnt.items() if p != win]
    return (win[2], win[0], win[1], best, max(rest) if rest else 0, found, anchored)


def record(first: Dict[str, int], index_kmers: Set[str], k: int, read, strands: int = 1):
    return record_of_votes(*votes(first, index_kmers, k, read, strands))


def records(first, index_kmers, k, reads, strands: int = 1):
    return [record(first, index_kmers, k, r, strands) for r in reads]


def n_placements(first, index_kmers, k, read, strands: int = 1) -> int:
    return len(votes(first, index_kmers, k, read, strands)[0])


def as_tuples(arr) -> list:
    """a structured array of sbwtgpu_read_map records as the tuples of record()"""
    return [(int(r["start"]), int(r["seq"]), int(r["strand"]), int(r["votes"]), int(r["votes2"]), int(r["n_found"]),
             int(r["n_anchored"])) for r in arr]


def cli_columns(rec) -> str:
    """the six columns `sbwt read-hits --positions` appends to a read's line: seq strand start votes votes2 n_anchored"""
    start, seq, strand, v, v2, _found, anchored = rec
    return "%d %d %d %d %d %d" % (seq, strand, start, v, v2, anchored)


def scalars(index_kmers: Set[str], k: int, numbered: Iterable[Tuple[int, object, int]]) -> Tuple[int, int]:
    """(n_windows, n_hits) of the adds: windows offered once per strand searched, misses and invalid windows counted"""
    nw = nh = 0
    for _seq, s, strands in numbered:
        s = _text(s)
        for pos in range(len(s) - k + 1):
            x = s[pos:pos + k]
            nw += strands
            if valid(x):
                nh += sum(1 for y in (x, revcomp(x))[:strands] if y in index_kmers)
    return nw, nh
