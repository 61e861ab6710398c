"""CPU: the set-operation ABI is declared and exported, the brute force that the GPU tests compare against
(tests/setop_brute.py) equals the definition-level BruteSBWT on hand-written cases, and the Python packing of the builder's
keys orders k-mers as the columns of an index are ordered (no GPU)."""
import os
import random
import re

import numpy as np
import pytest

from bruteforce import BruteSBWT, int_to_words
from setop_brute import OPS, apply_op, brute_counts, brute_setop, build_from_kmers, key_of, kmers_of, packed_keys
from sbwt_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETOP_SYMBOLS = ["sbwtgpu_index_setop", "sbwtgpu_index_setop_counts", "sbwtgpu_index_kmer_keys"]


def test_setop_symbols_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "sbwtgpu.h")).read()
    for name in ("SBWTGPU_SETOP_UNION 0", "SBWTGPU_SETOP_INTERSECTION 1", "SBWTGPU_SETOP_DIFFERENCE 2",
                 "SBWTGPU_SETOP_SYMMETRIC_DIFFERENCE 3"):
        assert re.search(r"#define\s+%s\b" % name.replace(" ", r"\s+"), text), name
    assert "bit for bit what sbwtgpu_build_plain_matrix returns" in text          # the contract sentence
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = capi.lib()
    for name in SETOP_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(L, name), name
    assert "sbwtgpu_setop_info" in text
    assert (capi.SETOP_UNION, capi.SETOP_INTERSECTION, capi.SETOP_DIFFERENCE, capi.SETOP_SYMMETRIC_DIFFERENCE) == (0, 1, 2, 3)


def test_cli_lists_the_command():
    src = open(os.path.join(ROOT, "sbwt_amd", "csrc", "host", "sbwt_cli.cpp")).read()
    assert '"set-op"' in src


def _same_as_definition(bits, kmers, k):
    """the host builder's bits of the k-mers == the columns of BruteSBWT over the same k-mers"""
    B = BruteSBWT(sorted(kmers), k)
    n = len(B.nodes)
    assert (bits.n_nodes, bits.n_kmers) == (n, len(kmers))
    cols, sg = B.columns()
    for c in range(4):
        assert np.array_equal(bits.cols[c], int_to_words(cols[c], n)), "ACGT"[c]
    assert np.array_equal(bits.ssup, int_to_words(sg, n))


HAND_CASES = {
    "identical": (["ACGTACGGT", "TTTACG"], ["TTTACG", "ACGTACGGT"]),
    "disjoint": (["AAAAACAAAA"], ["AGAGAGAGGG"]),
    "b inside a": (["ACGTACGGTCA", "GATTACA"], ["GTACGG"]),
    "a has no k-mer": (["AC"], ["ACGTACGGT"]),
    "b has no k-mer": (["ACGTNCGGT", "GATTACA"], ["ACG", "acgtacgt"]),
    "both empty": (["AC", "G"], ["T"]),
}


@pytest.mark.parametrize("name", sorted(HAND_CASES))
@pytest.mark.parametrize("k", [2, 4])
def test_brute_against_definition_on_hand_cases(name, k):
    sa, sb = HAND_CASES[name]
    if "no k-mer" in name or name == "both empty":
        k = 4                                                        # (the sequences are chosen shorter than this k)
    for rc in (False, True):
        A, B = kmers_of(sa, k, rc), kmers_of(sb, k, rc)
        if name == "identical":
            assert A == B and len(A) > 0
        if name == "disjoint":
            assert not (A & B) and A and B
        if name == "b inside a":
            assert B < A
        if name == "a has no k-mer":
            assert not A and B
        if name == "both empty":
            assert not A and not B
        c = brute_counts(sa, sb, k, rc, rc)
        assert c["n_a"] + c["n_b"] == c["n_both"] + c["n_either"]
        for op in OPS:
            bits, R = brute_setop(sa, sb, k, op, rc, rc)
            assert R == apply_op(A, B, op)
            _same_as_definition(bits, R, k)
        if name == "identical":
            assert brute_setop(sa, sb, k, "difference", rc, rc)[0].n_nodes == 1          # the empty index: the root alone
            assert brute_setop(sa, sb, k, "symmetric-difference", rc, rc)[1] == set()
        if name == "both empty":
            for op in OPS:
                bits, R = brute_setop(sa, sb, k, op, rc, rc)
                assert (bits.n_nodes, bits.n_kmers, R) == (1, 0, set())


def test_empty_result_without_marks():
    bits = build_from_kmers([], 5, streaming_support=False)
    assert (bits.n_nodes, bits.n_kmers) == (1, 0) and bits.ssup is None
    assert all(int(bits.cols[c][0]) == 0 for c in range(4))


@pytest.mark.parametrize("k", [2, 3, 5, 31, 32, 33, 64])
def test_key_format_orders_kmers_like_columns(k):
    """Index-free: the keys packed in Python, sorted as integers, list the k-mers in the order of the real columns of the
    definition-level index; one word for k <= 32 with character 31 in the top bits, two words above."""
    rng = random.Random(k)
    alphabet = "AC" if k <= 5 else "ACGT"
    seqs = ["".join(rng.choice(alphabet) for _ in range(rng.randint(k, k + 30))) for _ in range(4)]
    kmers = kmers_of(seqs, k, True)
    B = BruteSBWT(seqs, k, True)
    real = [s for s in B.nodes if len(s) == k]
    assert sorted(kmers, key=key_of) == real
    assert len({key_of(w) for w in kmers}) == len(kmers)
    P = packed_keys(kmers, k)
    assert P.dtype == np.uint64 and P.shape == ((len(kmers),) if k <= 32 else (len(kmers), 2))
    assert [int(x) if k <= 32 else int(x[0]) | (int(x[1]) << 64) for x in P] == [key_of(w) for w in real]
    w = real[-1]
    got = int(P[-1]) if k <= 32 else int(P[-1, 0]) | (int(P[-1, 1]) << 64)
    assert got == key_of(w) and got < (1 << (2 * k))
    assert [(got >> (2 * i)) & 3 for i in range(k)] == ["ACGT".index(c) for c in w]
    assert key_of("C") == 1 and key_of("AC") == 4 and key_of("TA") == 3 and key_of("A" * 31 + "T") == 3 << 62
