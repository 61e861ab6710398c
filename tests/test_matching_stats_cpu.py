"""CPU: the matching-statistics ABI is declared and exported, the brute force that the GPU tests compare against checks
itself against the definition, and the oracle's definition-level matching statistics and LCS array -- what the GPU tests
compare against at scale -- equal the brute force, with and without their len[i-1] + 1 shortcut (no GPU)."""
import json
import os
import random
import re

import numpy as np
import pytest

from bruteforce import BruteSBWT, int_to_words, kmer_set
from ms_brute import BruteMS, format_ms, lcs_array, probe_reads, suffix_intervals
from oracle import OracleIndex
from sbwt_amd import capi, hostlib, synth

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



# ---- the oracle's definition-level matching statistics and LCS (oracle/sbwt_oracle.c), which the GPU tests at scale use ----
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_kats.json")))


def _oracle_from_brute(B, precalc_k=0):
    """The columns straight from the definition (so k = 1 works too: the host builder starts at k = 2)."""
    cols, sg = B.columns()
    n = len(B.nodes)
    w = [int_to_words(c, n) for c in cols]
    return OracleIndex.from_bits(w[0], w[1], w[2], w[3], int_to_words(sg, n), n, B.k, len(B.kmers), precalc_k)


def _check_oracle_against_brute(B, reads, label):
    M = BruteMS(B)
    want = [M.read(r) for r in reads]
    want_lcs = np.array(lcs_array(B), dtype=np.uint8)
    bases, off = capi.concat_reads(reads)
    for pk in sorted({0, min(B.k, 2), min(B.k, 5)}):          # update_interval alone, and from the precalc table
        orc = _oracle_from_brute(B, pk)
        assert np.array_equal(orc.lcs(n_threads=3), want_lcs), (label, pk)
        cols = np.arange(len(B.nodes))[::-1].copy()
        assert np.array_equal(orc.lcs(cols), want_lcs[cols]), (label, pk)
        for exhaustive in (False, True):
            ln, f, s, _ = orc.matching_statistics(bases, off, n_threads=3, exhaustive=exhaustive)
            ln2, _ = orc.matching_statistics(bases, off, intervals=False, exhaustive=exhaustive)
            assert np.array_equal(ln, ln2)
            for r, read in enumerate(reads):
                a, b = off[r], off[r + 1]
                L, F, S = want[r]
                assert list(ln[a:b]) == L, (label, pk, exhaustive, read)
                assert list(f[a:b]) == F and list(s[a:b]) == S, (label, pk, exhaustive, read)


def test_oracle_ms_and_lcs_on_fixture_indexes():
    rng = random.Random(3)
    c = KATS["cli_end_to_end"]
    B = BruteSBWT(c["seqs"], c["k"], c["add_reverse_complements"])
    _check_oracle_against_brute(B, [q.encode() for q in c["queries"]] + probe_reads(c["seqs"], c["k"], rng), "cli_end_to_end")
    c = KATS["redundant_dummies"]
    _check_oracle_against_brute(BruteSBWT(c["seqs"], c["k"]), probe_reads(c["seqs"], c["k"], rng), "redundant_dummies")
    for case in KATS["small_cases"]["cases"]:
        B = BruteSBWT(case["seqs"], case["k"])
        _check_oracle_against_brute(B, probe_reads(case["seqs"], case["k"], rng), case["name"])


@pytest.mark.parametrize("k", [1, 2, 3, 7, 31, 32, 63, 64])
def test_oracle_ms_and_lcs_on_random_small_indexes(k):
    rng = random.Random(5 * k + 1)
    for trial in range(3):
        seqs = ["".join(rng.choice("ACGT") for _ in range(rng.randint(k, 2 * k + 60))) for _ in range(rng.randint(1, 3))]
        B = BruteSBWT(seqs, k, trial == 1)
        _check_oracle_against_brute(B, probe_reads(seqs, k, rng), (k, trial))


def test_oracle_ms_shortcut_equals_exhaustive_at_scale():
    """The len[i-1] + 1 start of the fast mode against the exhaustive start at min(k, run): ~200 k positions on ~1 M columns
    built by the host builder, reads with substitutions, N, lower case, other bytes, and random reads."""
    k = 31
    g = synth.repeat_genome(500_000, 41, 0.2)
    bits = hostlib.build_bits([g.tobytes()], k, True, True, n_threads=8)
    assert 800_000 < bits.n_nodes < 3_000_000, bits.n_nodes
    orc = OracleIndex.from_bits(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k,
                                bits.n_kmers, 6)
    b1, o1 = synth.sample_reads([g, synth.revcomp(g)], 1000, 150, 0.03, 42)
    b1 = synth.inject(synth.inject(synth.inject(b1, 1500, ord("N"), 43), 600, ord("a"), 44), 200, 0, 45)
    b2, o2 = synth.random_reads(300, 150, 46)
    reads = [b1[o1[r]:o1[r + 1]].tobytes() for r in range(len(o1) - 1)] + [b2[o2[r]:o2[r + 1]].tobytes() for r in range(300)]
    reads += [g[1000:40_000].tobytes(), b"", b"\xff" + g[7:99].tobytes()]
    bases, off = capi.concat_reads(reads)
    assert 150_000 < len(bases) < 300_000
    fast = orc.matching_statistics(bases, off, n_threads=8)
    slow = orc.matching_statistics(bases, off, n_threads=8, exhaustive=True)
    for a, b in zip(fast[:3], slow[:3]):
        assert np.array_equal(a, b)
    ln = fast[0]
    assert (ln == k).mean() > 0.2 and (ln == 0).any() and ((ln > 0) & (ln < k)).mean() > 0.1
