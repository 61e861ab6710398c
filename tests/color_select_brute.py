"""The definition of colour select (include/sbwtgpu.h, "colour select") in pure Python, from k-mer
strings: a dict from k-mer to the frozenset of its colours (made with tests/pseudoalign_brute.py), the predicate with Python
sets, and the selected k-mers through setop_brute.build_from_kmers.  Per-row verdicts in numpy on a table.  Also the seeded
cases that tests/test_gpu_color_select.py runs on the GPU and tests/test_color_select_cpu.py replays without one."""
from __future__ import annotations

import random
from typing import Dict, FrozenSet, Iterable, List, Optional, Sequence, Set

import numpy as np

import pseudoalign_brute as pb
import pseudoalign_wide as pw
from setop_brute import build_from_kmers, kmers_of


# ---- the definition -----------------------------------------------------------------------------------------------------
def colouring(index_kmers: Set[str], color_sets: Sequence[Set[str]]) -> Dict[str, FrozenSet[int]]:
    """k-mer of the index -> the colours it was given for (color_sets: pseudoalign_brute.add's)"""
    return {x: frozenset(c for c, S in enumerate(color_sets) if x in S) for x in index_kmers}


def colour_world(seqs_by_color: Dict[int, Sequence[str]], extra: Sequence[str], k: int, rc: bool, n_colors: int):
    """(index sequences, index k-mers, k-mer -> colours) of an index over every sequence, coloured as the builder colours it:
    colour c = the k-mers of seqs_by_color[c], on both strands when the index holds reverse complements"""
    seqs = [s for c in sorted(seqs_by_color) for s in seqs_by_color[c]] + list(extra)
    kmers = kmers_of(seqs, k, rc)
    cs: List[Set[str]] = [set() for _ in range(n_colors)]
    for c, ss in sorted(seqs_by_color.items()):
        pb.add(cs, kmers, k, c, ss, 2 if rc else 1)
    return seqs, kmers, colouring(kmers, cs)


def matches(colors: FrozenSet[int], include: Iterable[int], exclude: Optional[Iterable[int]], min_in: int, max_in: int) -> bool:
    if exclude is not None and colors & set(exclude):
        return False
    return min_in <= len(colors & set(include)) <= max_in


def default_max(include: Iterable[int], min_in: int, max_in: Optional[int]) -> int:
    """max_in = None means popcount(include) (and at least min_in: a min_in above it is legal and selects nothing)"""
    return max(len(set(include)), min_in) if max_in is None else max_in


def select(col: Dict[str, FrozenSet[int]], include, exclude=None, min_in: int = 1, max_in: Optional[int] = None) -> Set[str]:
    max_in = default_max(include, min_in, max_in)
    return {x for x, cs in col.items() if matches(cs, include, exclude, min_in, max_in)}


def n_nopred(kmers: Set[str]) -> int:
    """the k-mers whose (k-1)-prefix is the (k-1)-suffix of none of them"""
    suffixes = {x[1:] for x in kmers}
    return sum(1 for x in kmers if x[:-1] not in suffixes)


def counts(col: Dict[str, FrozenSet[int]], include, exclude=None, min_in: int = 1, max_in: Optional[int] = None) -> dict:
    sel = select(col, include, exclude, min_in, max_in)
    return {"n_real": len(col), "n_selected": len(sel), "n_sets_matched": len({col[x] for x in sel}), "n_nopred": n_nopred(sel)}


def build(col, k: int, include, exclude=None, min_in: int = 1, max_in: Optional[int] = None, streaming_support: bool = True):
    """(bits, counts) of the definition"""
    sel = select(col, include, exclude, min_in, max_in)
    return build_from_kmers(sel, k, streaming_support), counts(col, include, exclude, min_in, max_in)


# ---- verdicts on a table ------------------------------------------------------------------------------------------------
def mask_words(colors: Iterable[int], words: int) -> np.ndarray:
    m = 0
    for c in colors:
        m |= 1 << c
    return pw.rows_array([m], words)[0]


def popcounts(a: np.ndarray) -> np.ndarray:
    """per row of a (n, W) uint64 array"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(a.shape[0], -1), axis=1).sum(axis=1, dtype=np.int64)


def verdicts(table: np.ndarray, include: np.ndarray, exclude: Optional[np.ndarray], min_in: int, max_in: int) -> np.ndarray:
    """uint8[n_sets] from word arrays: (row & exclude) == 0 and min_in <= popcount(row & include) <= max_in"""
    table = np.ascontiguousarray(table, dtype=np.uint64)
    pop = popcounts(table & include[None, :])
    ok = (pop >= min_in) & (pop <= max_in)
    if exclude is not None:
        ok &= ~(table & exclude[None, :]).any(axis=1)
    return ok.astype(np.uint8)


# ---- the seeded cases of the GPU test -----------------------------------------------------------------------------------
K_VALUES = (2, 3, 31, 32, 33, 63, 64)
FAMILIES = ("core", "unique", "accessory", "soft-core", "absent")
N_COLORS = {2: 0, 3: 0, 31: 0, 32: 64, 33: 65, 63: 130, 64: 0}        # 0: as many colours as references


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def seeded_world(k: int, rc: bool):
    """References that share whole segments of a pool: (k, rc, n_colors, colour -> sequences, uncoloured sequences)"""
    rng = random.Random(7000 + 10 * k + rc)
    n_refs = rng.randint(2, 5)
    if k <= 3:
        pool = [rand_seq(rng, rng.randint(k, k + 1), "ACG") for _ in range(8)]
    else:
        pool = [rand_seq(rng, rng.randint(k + 2, 2 * k + 60)) for _ in range(10)]
    n_colors = N_COLORS[k] or n_refs
    # the first and the last colour are among the used ones
    used = sorted({0, n_colors - 1} | {(i * n_colors) // n_refs for i in range(1, n_refs - 1)}) if n_colors > n_refs else list(range(n_refs))
    by_color = {}
    for c in used:
        mine = [s for s in pool[:-1] if rng.random() < 0.55]
        by_color[c] = mine or [pool[0]]
    return k, rc, n_colors, by_color, [pool[-1]]               # the pool's last segment is in the index and in no colour


def family_predicate(family: str, used: Sequence[int], n_colors: int):
    """(include, exclude, min_in, max_in) of a family over the used colours of a world"""
    used = list(used)
    if family == "core":
        return used, None, len(used), None
    if family == "unique":
        return [used[0]], [c for c in range(n_colors) if c != used[0]], 1, None
    if family == "accessory":
        return used, None, 1, len(used) - 1
    if family == "soft-core":
        return used, None, min(2, len(used)), None
    if family == "absent":
        return used[::2], None, 0, 0
    raise ValueError(family)


def seeded_cases():
    """(label, k, rc, n_colors, colour -> sequences, uncoloured sequences, family, predicate) of every seeded case"""
    out = []
    for k in K_VALUES:
        for rc in (False, True):
            k_, rc_, n_colors, by_color, extra = seeded_world(k, rc)
            for family in FAMILIES:
                out.append(("k%d-%s-%s" % (k, "rc" if rc else "fwd", family), k, rc, n_colors, by_color, extra, family,
                            family_predicate(family, sorted(by_color), n_colors)))
    return out
