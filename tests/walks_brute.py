"""Definition-level brute force of the walks (include/sbwtgpu.h) in pure Python, on top of
tests/unitig_links_brute.py: that gives the dictionary k-mer -> (unitig, offset) of the plain or the coloured graph, this
threads reads through it.  Steps come from the GENERAL rule of the definition -- the next window hits, on the same unitig, at
the next offset -- and never from the offset-0 shortcut the kernels use; steps_by_shortcut() is that shortcut, so that a CPU
test can compare the two.  Tiny inputs only.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

Step = Tuple[int, int, int, int]          # (unitig, offset, read_pos, n_kmers)


def text(read) -> str:
    return read.decode("latin-1") if isinstance(read, (bytes, bytearray)) else read


def coordinates_of_read(read, k: int, where: Dict[str, Tuple[int, int]]):
    """Per window: (unitig, offset), or None for a miss.  A window holding anything but upper-case ACGT is no k-mer of the
    dictionary, so it misses."""
    s = text(read)
    return [where.get(s[i:i + k]) for i in range(max(0, len(s) - k + 1))]


def steps_of_read(read, k: int, where) -> List[Step]:
    co = coordinates_of_read(read, k, where)
    steps, i = [], 0
    while i < len(co):
        if co[i] is None:
            i += 1
            continue
        n = 1
        while i + n < len(co) and co[i + n] is not None and co[i + n] == (co[i][0], co[i][1] + n):
            n += 1
        steps.append((co[i][0], co[i][1], i, n))
        i += n
    return steps


def steps_by_shortcut(read, k: int, where) -> List[Step]:
    """The kernels' rule: inside a run of hits a step starts exactly where the offset is 0."""
    co = coordinates_of_read(read, k, where)
    steps = []
    for i, c in enumerate(co):
        if c is None:
            continue
        if i == 0 or co[i - 1] is None or c[1] == 0:
            steps.append([c[0], c[1], i, 1])
        else:
            steps[-1][3] += 1
    return [tuple(s) for s in steps]


def brute_walks(reads: Sequence, k: int, where, n_unitigs: int):
    """(step_off, steps, coverage): the CSR layout of the definition and the k-mer hits per unitig, by summation."""
    step_off, steps = [0], []
    coverage = [0] * n_unitigs
    for r in reads:
        mine = steps_of_read(r, k, where)
        steps += mine
        step_off.append(len(steps))
        for u, _, _, n in mine:
            coverage[u] += n
    return step_off, steps, coverage


def check_consequences(reads: Sequence, k: int, where, unitigs: List[str], link_off, link_to, step_off, steps) -> None:
    """Everything the definition says follows, asserted on a result in the layout of brute_walks()."""
    assert step_off[0] == 0 and len(step_off) == len(reads) + 1 and step_off[-1] == len(steps)
    n_kmers_of = [len(u) - k + 1 for u in unitigs]
    links = {(i, j) for i in range(len(unitigs)) for j in link_to[link_off[i]:link_off[i + 1]]}
    for r, read in enumerate(reads):
        co = coordinates_of_read(read, k, where)
        mine = steps[step_off[r]:step_off[r + 1]]
        runs = sum(1 for i, c in enumerate(co) if c is not None and (i == 0 or co[i - 1] is None))
        fresh = 0
        for s, (u, o, p, n) in enumerate(mine):
            assert n >= 1 and 0 <= p and p + n <= len(co) and o + n <= n_kmers_of[u]
            assert all(co[p + j] == (u, o + j) for j in range(n))
            if s and mine[s - 1][2] + mine[s - 1][3] == p:            # continues its predecessor
                pu, po, _, pn = mine[s - 1]
                assert po + pn == n_kmers_of[pu] and o == 0 and (pu, u) in links, (r, s)
            else:
                fresh += 1
                if s:
                    assert mine[s - 1][2] + mine[s - 1][3] < p        # no overlap: a gap of at least one window ...
                assert p == 0 or co[p - 1] is None                     # ... which misses
        assert sum(n for _, _, _, n in mine) == sum(c is not None for c in co)     # read_hits' n_found
        assert fresh == runs


def random_reads(rng, seqs: Sequence[str], k: int, n: int = 12) -> List[str]:
    """Reads for a k-mer set given by its sequences: pieces of them (whole runs along unitigs and across links), pieces glued
    together (gaps), substitutions, an N, a lower-case base, reads shorter than k and an empty one."""
    seqs = [text(s) for s in seqs]
    reads = []
    for _ in range(n):
        parts = []
        for _ in range(rng.randint(1, 3)):
            s = rng.choice(seqs)
            a = rng.randrange(len(s))
            parts.append(s[a:a + rng.randint(1, 4 * k + 40)])
        r = list("".join(parts))
        for _ in range(rng.randint(0, 2)):
            if r:
                r[rng.randrange(len(r))] = rng.choice("ACGTNa")
        reads.append("".join(r))
    reads += ["", rng.choice(seqs)[:k - 1], rng.choice(seqs)]
    rng.shuffle(reads)
    return reads
