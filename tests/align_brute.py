"""The definition of "alignment of mapped reads" (include/sbwtgpu.h) in pure Python on top of
tests/verify_brute.py: Sellers' whole table and the walk back over it, the same walk over the band of the lemma only, the
record with its special cases, the runs as uint32, the CIGAR string and the two columns the CLI appends.

An alignment is the tuple (ref_begin, runs) with runs a list of (length, letter) in read order; a record is
(ref_begin, n_ops, n_eq)."""
import numpy as np

import verify_brute as vb

INF = 1 << 30
CODES = {"I": 1, "D": 2, "=": 7, "X": 8}
LETTERS = {v: k for k, v in CODES.items()}
NO_ALIGNMENT = (0, 0, 0)


def full_table(ref: bytes, r, start: int, band: int):
    """D[i][t] for i = 0 .. L, t = 0 .. L + 2 band; column t >= 1 stands for coordinate start - band + t - 1"""
    L, lo, n_cols = len(r), start - band, len(r) + 2 * band
    D = [[0] * (n_cols + 1)]
    for i in range(1, L + 1):
        prev, cur = D[-1], [i] + [0] * n_cols
        for t in range(1, n_cols + 1):
            c = 0 if vb.matches(ref, lo + t - 1, r[i - 1]) else 1
            cur[t] = min(prev[t - 1] + c, prev[t] + 1, cur[t - 1] + 1)
        D.append(cur)
    return D


def full_table_numpy(ref: bytes, r, start: int, band: int):
    """The same table as a numpy array, row by row as verify_brute.sellers_numpy does it: for reads of a thousand bases"""
    L, lo, n_cols = len(r), start - band, len(r) + 2 * band
    win = np.array([vb.text_at(ref, lo + t) or 0 for t in range(n_cols)], dtype=np.int64)       # 0: matches nothing
    idx = np.arange(n_cols + 1, dtype=np.int64)
    D = np.zeros((L + 1, n_cols + 1), dtype=np.int64)
    for i in range(1, L + 1):
        rj = r[i - 1] or -1                                                                 # -1: matches nothing
        x = np.empty(n_cols + 1, dtype=np.int64)
        x[0] = i
        x[1:] = np.minimum(D[i - 1, :-1] + (win != rj), D[i - 1, 1:] + 1)
        D[i] = np.minimum.accumulate(x - idx) + idx
    return D


def merge(ops):
    """the operations in the walk's order (last first) -> runs in read order"""
    runs = []
    for op in reversed(ops):
        if runs and runs[-1][1] == op:
            runs[-1] = (runs[-1][0] + 1, op)
        else:
            runs.append((1, op))
    return runs


def walk(cell, ref: bytes, r, start: int, band: int, tE: int):
    """The walk of the definition from (L, tE) over cell(i, t) -> D[i][t] (INF for a cell that is not there): at each cell the
    first step that applies.  -> (ref_begin, runs)"""
    lo = start - band
    i, t, ops = len(r), tE, []
    while i > 0:
        here = cell(i, t)
        c = 0 if t > 0 and vb.matches(ref, lo + t - 1, r[i - 1]) else 1
        if t > 0 and cell(i - 1, t - 1) + c == here:
            ops.append("=" if c == 0 else "X")
            i, t = i - 1, t - 1
        elif cell(i - 1, t) + 1 == here:
            ops.append("I")
            i -= 1
        else:
            assert t > 0 and cell(i, t - 1) + 1 == here, (i, t)
            ops.append("D")
            t -= 1
    return lo + t, merge(ops)


def align_full(ref: bytes, r, start: int, band: int, table=full_table_numpy):
    """(edit, ref_end, ref_begin, runs) from the whole table; L > 0"""
    D = table(ref, r, start, band)
    last = [int(v) for v in D[-1]]
    edit = min(last)
    tE = last.index(edit)
    begin, runs = walk(lambda i, t: int(D[i][t]) if t >= 0 else INF, ref, r, start, band, tE)
    return edit, start - band + tE, begin, runs


def banded_table(ref: bytes, r, start: int, band: int, edit: int, tE: int):
    """The table on the diagonals d = t - i with |d - (tE - L)| <= edit only, every other cell infinite (a dict of the cells
    that are there).  Columns right of tE's band are never needed; columns left of 0 do not exist."""
    L, lo, n_cols = len(r), start - band, len(r) + 2 * band
    d0 = tE - L
    T = {}
    for i in range(L + 1):
        for d in range(d0 - edit, d0 + edit + 1):
            t = i + d
            if t < 0 or t > n_cols:
                continue
            if i == 0:
                T[(i, t)] = 0
            elif t == 0:
                T[(i, t)] = min(T.get((i - 1, t), INF) + 1, INF)    # (i where the column above is in the band, as the kernel has it)
            else:
                c = 0 if vb.matches(ref, lo + t - 1, r[i - 1]) else 1
                T[(i, t)] = min(T.get((i - 1, t - 1), INF) + c, T.get((i - 1, t), INF) + 1, T.get((i, t - 1), INF) + 1)
    return T


def align_banded(ref: bytes, r, start: int, band: int, edit: int, ref_end: int, extra: int = 0):
    """(ref_begin, runs) from the band of the lemma alone, given the forward pass's edit and ref_end (extra: a wider band,
    which changes nothing)"""
    tE = ref_end - (start - band)
    T = banded_table(ref, r, start, band, edit + extra, tE)
    return walk(lambda i, t: T.get((i, t), INF), ref, r, start, band, tE)


def alignment(refs, read: bytes, rec, band: int, table=full_table_numpy):
    """(verify record, align record, runs) of one read; refs: the sequences as byte strings; rec: (seq, strand, start)"""
    v = vb.record(refs, read, rec, band)
    seq, strand, start = rec
    if v[2] < 0:
        return v, NO_ALIGNMENT, []
    if len(read) == 0:
        return v, (start - band, 0, 0), []
    r = vb.orient(read, strand)
    edit, end, begin, runs = align_full(refs[seq], r, start, band, table)
    assert (end, edit) == (v[0], v[2])
    return v, (begin, len(runs), sum(n for n, op in runs if op == "=")), runs


def alignments(refs, reads, recs, band: int):
    return [alignment(refs, rd, rc, band) for rd, rc in zip(reads, recs)]


def encode(runs):
    """the runs as uint32, as in BAM"""
    return [(n << 4) | CODES[op] for n, op in runs]


def decode(ops):
    return [(int(o) >> 4, LETTERS[int(o) & 15]) for o in ops]


def cigar(runs) -> str:
    return "".join("%d%s" % (n, op) for n, op in runs) if runs else "*"


def cli_columns(v, a, runs) -> str:
    """what `sbwt read-hits --refs --cigar` appends to a line: mismatches edit ref_end ref_begin cigar"""
    return "%s %d %s" % (vb.cli_columns(v), a[0], cigar(runs))


def replay(ref: bytes, r, begin: int, runs):
    """Replays the runs from coordinate `begin` against the oriented read: every = column matches, every X column does not, and
    the runs consume exactly the read.  -> the exclusive end coordinate"""
    p, j = begin, 0
    for n, op in runs:
        for _ in range(n):
            if op == "=":
                assert vb.matches(ref, p, r[j]), (p, j)
            elif op == "X":
                assert not vb.matches(ref, p, r[j]), (p, j)
            if op in "=XI":
                j += 1
            if op in "=XD":
                p += 1
    assert j == len(r)
    return p
