"""CPU: the matching-statistics ABI is declared and exported, and the brute force that the GPU tests compare against checks
itself against the definition (no GPU)."""
import os
import random
import re

import pytest

from bruteforce import BruteSBWT, kmer_set
from ms_brute import BruteMS, format_ms, lcs_array, suffix_intervals
from sbwt_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS_SYMBOLS = ["sbwtgpu_index_build_lcs", "sbwtgpu_index_get_lcs", "sbwtgpu_matching_statistics_batch",
              "sbwtgpu_ms_workspace_bytes", "sbwtgpu_matching_statistics_dev", "sbwtgpu_ms_workspace_stats"]


def test_ms_symbols_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "sbwtgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = capi.lib()
    for name in MS_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(L, name), name
    assert capi.ms_workspace_bytes(0) >= 40 and capi.ms_workspace_bytes(1 << 30) % 16 == 0


def test_cli_lists_the_command():
    src = open(os.path.join(ROOT, "sbwt_amd", "csrc", "host", "sbwt_cli.cpp")).read()
    assert "matching-statistics" in src


def _random_case(rng, k, rc):
    seqs = ["".join(rng.choice("ACGT") for _ in range(rng.randint(k, 3 * k + 8))) for _ in range(rng.randint(1, 4))]
    return seqs, BruteSBWT(seqs, k, rc)


@pytest.mark.parametrize("k", list(range(1, 9)))
@pytest.mark.parametrize("rc", [False, True])
def test_label_suffixes_are_kmer_substrings(k, rc):
    rng = random.Random(1000 * k + rc)
    for _ in range(6):
        seqs, B = _random_case(rng, k, rc)
        kmers = B.kmers
        subs = {w[a:b] for w in kmers for a in range(k) for b in range(a + 1, k + 1)}
        sfx = {w for w in suffix_intervals(B) if w}
        assert sfx == subs
        lcs = lcs_array(B)
        assert lcs[0] == 0 and all(0 <= v <= k - 1 for v in lcs)


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8])
def test_brute_ms_invariants(k):
    rng = random.Random(77 + k)
    for _ in range(4):
        seqs, B = _random_case(rng, k, k % 2 == 0)
        M = BruteMS(B)
        n = len(B.nodes)
        reads = [seqs[0].encode(), "".join(rng.choice("ACGTN") for _ in range(40)).encode(), b"ACGTacgtNNACG\x00T", b""]
        for s in reads:
            L, F, S = M.read(s)
            assert len(L) == len(s)
            for i in range(len(s)):
                assert 0 <= L[i] <= k
                if i + 1 < len(s):
                    assert L[i + 1] <= L[i] + 1
                if L[i] == 0:
                    assert (F[i], S[i]) == (0, n - 1)
                else:
                    w = s[i - L[i] + 1:i + 1].decode()
                    assert all(B.nodes[j].endswith(w) for j in range(F[i], S[i] + 1))
                if L[i] == k:
                    assert F[i] == S[i] == B.search(s[i - k + 1:i + 1].decode())
                elif i - L[i] >= 0 and s[i - L[i]] in b"ACGT":
                    assert s[i - L[i]:i + 1].decode() not in M.iv
        # every indexed k-mer inside its own source reaches len == k
        L, F, S = M.read(seqs[0].encode())
        assert all(L[i] == k for i in range(k - 1, len(seqs[0])))


def test_format_ms_layout():
    assert format_ms([0, 1, 2]) == b"0 1 2 \n"
    assert format_ms([1], [3], [4]) == b"1,3,4 \n"
    assert format_ms([]) == b"\n"
