"""Brute force of the set operations on two indexes, which IS their definition (include/sbwtgpu.h): take the k-mer sets of two
sequence lists (reverse complements included where asked), apply Python's set operation, spell the result's k-mers as
sequences of length k and build them with the host builder, add_revcomp = 0.  Also the builder's key format in Python."""
from __future__ import annotations

from typing import Iterable, List, Set

import numpy as np

import re

from bruteforce import revcomp
from sbwt_amd import hostlib

OPS = ("union", "intersection", "difference", "symmetric-difference")
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def as_str(seqs) -> List[str]:
    return [s.decode("latin-1") if isinstance(s, (bytes, bytearray)) else s for s in seqs]


_memo: dict = {}


def kmers_of(seqs, k: int, rc: bool = False) -> Set[str]:
    """The k-mer set the builders index: windows of upper-case ACGT, of the sequences and (rc) their reverse complements.
    (bruteforce.kmer_set's definition, by runs of ACGT; the last few results are kept: the tests ask again per operation.)"""
    seqs = as_str(seqs)
    key = (tuple(seqs), k, rc)
    if key in _memo:
        return _memo[key]
    if rc:
        seqs = seqs + [revcomp(s) for s in seqs]
    out = set()
    for s in seqs:
        for m in re.finditer("[ACGT]+", s):
            run = m.group()
            out.update(run[i:i + k] for i in range(len(run) - k + 1))
    if len(_memo) >= 8:
        _memo.pop(next(iter(_memo)))
    _memo[key] = out
    return out


def apply_op(A: Set[str], B: Set[str], op: str) -> Set[str]:
    if op == "union":
        return A | B
    if op == "intersection":
        return A & B
    if op == "difference":
        return A - B
    if op == "symmetric-difference":
        return A ^ B
    raise ValueError(op)


def build_from_kmers(kmers: Iterable[str], k: int, streaming_support: bool = True):
    """hostlib.build_bits of the k-mers as sequences of length k (sorted: the input order does not matter to the result)."""
    return hostlib.build_bits([w.encode() for w in sorted(kmers)], k, False, streaming_support)


def brute_setop(seqs_a, seqs_b, k: int, op: str, rc_a: bool = False, rc_b: bool = False, streaming_support: bool = True):
    """(bits, result k-mer set) of the operation on the k-mer sets of the two sequence lists."""
    R = apply_op(kmers_of(seqs_a, k, rc_a), kmers_of(seqs_b, k, rc_b), op)
    return build_from_kmers(R, k, streaming_support), R


def brute_counts(seqs_a, seqs_b, k: int, rc_a: bool = False, rc_b: bool = False):
    A, B = kmers_of(seqs_a, k, rc_a), kmers_of(seqs_b, k, rc_b)
    return {"n_a": len(A), "n_b": len(B), "n_both": len(A & B), "n_either": len(A | B)}


def key_of(kmer: str) -> int:
    """The device builder's key: character i of the k-mer at bits 2i, so that integer order is colexicographic order."""
    v = 0
    for i, c in enumerate(kmer):
        v |= CODE[c] << (2 * i)
    return v


def packed_keys(kmers: Iterable[str], k: int) -> np.ndarray:
    """The sorted keys as sbwtgpu_index_kmer_keys returns them: uint64[n] for k <= 32, (n, 2) uint64 (low, high) above.
    (key_of for every k-mer, in numpy: sets of 10^5 k-mers take a moment instead of seconds.)"""
    kmers = list(kmers)
    n = len(kmers)
    if n == 0:
        return np.zeros(0 if k <= 32 else (0, 2), dtype=np.uint64)
    lut = np.zeros(256, dtype=np.uint64)
    for c, v in CODE.items():
        lut[ord(c)] = v
    codes = lut[np.frombuffer("".join(kmers).encode(), dtype=np.uint8).reshape(n, k)]
    lo, hi = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    for i in range(k):
        if i < 32:
            lo |= codes[:, i] << np.uint64(2 * i)
        else:
            hi |= codes[:, i] << np.uint64(2 * (i - 32))
    order = np.lexsort((lo, hi))
    if k <= 32:
        return lo[order]
    return np.stack([lo[order], hi[order]], axis=1)


def same_bits(a, b) -> bool:
    """rows, marks, n_nodes, n_kmers of two builder results (hostlib.IndexBits / capi.BuiltBits)"""
    if (a.n_nodes, a.n_kmers) != (b.n_nodes, b.n_kmers) or (a.ssup is None) != (b.ssup is None):
        return False
    if any(not np.array_equal(a.cols[c], b.cols[c]) for c in range(4)):
        return False
    return a.ssup is None or np.array_equal(a.ssup, b.ssup)
