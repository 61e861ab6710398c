"""The definition of the occurrence table and of a read's map record over all occurrences (include/sbwtgpu.h, "occurrences") in
pure Python, from strings: the index's k-mers as a set, the reference sequences with the numbers the caller gave them, and the
reads.  Nothing here looks at an index structure or calls the library.

Keys, placements and records are those of positions_brute: a key is (seq << 32) | (pos << 1) | t, a placement the triple
(seq, o, start), a record the tuple (start, seq, strand, votes, votes2, n_found, n_anchored)."""
from __future__ import annotations

from collections import Counter
from typing import Dict, Iterable, List, Sequence, Set, Tuple

from positions_brute import _text, cli_columns, decode, key, record_of_votes, revcomp, valid  # noqa: F401  (cli_columns: the same six)


def table(index_kmers: Set[str], k: int, numbered: Iterable[Tuple[int, object, int]]) -> Dict[str, List[int]]:
    """k-mer -> the sorted list of the distinct keys offered to it, over the (sequence number, sequence, strands) triples.  Only
    k-mers of the index get occurrences."""
    occ: Dict[str, set] = {}
    for seq, s, strands in numbered:
        s = _text(s)
        for pos in range(len(s) - k + 1):
            x = s[pos:pos + k]
            if not valid(x):
                continue
            for t, y in ((0, x), (1, revcomp(x)))[:strands]:
                if y in index_kmers:
                    occ.setdefault(y, set()).add(key(seq, pos, t))
    return {y: sorted(v) for y, v in occ.items()}


def arrays(occ: Dict[str, List[int]], labels: Sequence[str]) -> Tuple[List[int], List[int]]:
    """(off, keys) in column order from the columns' labels ('$' in a label: a dummy column, never positioned)"""
    off, keys = [0], []
    for lab in labels:
        keys += occ.get(_text(lab), [])
        off.append(len(keys))
    return off, keys


def first_of(occ: Dict[str, List[int]]) -> Dict[str, int]:
    """the positions table that the same adds give: the smallest key of every k-mer"""
    return {y: v[0] for y, v in occ.items()}


def votes(occ: Dict[str, List[int]], index_kmers: Set[str], k: int, read, strands: int = 1, max_occ: int = 1024):
    """(Counter of placements, n_found, n_anchored) of one read: a hit on a k-mer of 1 .. max_occ occurrences is anchored and
    casts one vote per occurrence"""
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
            keys = occ.get(y, [])
            if not keys or len(keys) > max_occ:
                continue
            anchored += 1
            for f in keys:
                seq, pos, t = decode(f)
                o = sidx ^ t
                cnt[(seq, o, pos - i if o == 0 else pos - (W - 1 - i))] += 1
    return cnt, found, anchored


def record(occ, index_kmers, k, read, strands: int = 1, max_occ: int = 1024):
    return record_of_votes(*votes(occ, index_kmers, k, read, strands, max_occ))


def records(occ, index_kmers, k, reads, strands: int = 1, max_occ: int = 1024):
    return [record(occ, index_kmers, k, r, strands, max_occ) for r in reads]


def n_placements(occ, index_kmers, k, read, strands: int = 1, max_occ: int = 1024) -> int:
    return len(votes(occ, index_kmers, k, read, strands, max_occ)[0])


def scalars(occ: Dict[str, List[int]]) -> Tuple[int, int, int]:
    """(n_occurrences, n_positioned, max_count); n_windows and n_hits are positions_brute.scalars'"""
    return sum(len(v) for v in occ.values()), len(occ), max((len(v) for v in occ.values()), default=0)
