"""CPU: the references of the k >= 64 GPU tests (tests/test_gpu_long_k.py) agree with each other before the GPU is compared
with them (no GPU).

  - the C oracle over columns it did not build (OracleIndex.from_bits; its own constructor stops at k = 64) against the
    definition-level brute force at k = 65, 128 and 255, on indexes of a few hundred columns: every function the GPU tests
    call;
  - the oracle's own builder and the host builder give the same rows and marks on the k = 64 case, and the definition-level
    verifier accepts them;
  - the shared cases (tests/long_k_cases.py) are not vacuous at any k of the sweep;
  - the Python view of the image header matches the offsets the other tests read by hand."""
import random

import numpy as np
import pytest

import long_k_cases
import sbwt_verify
from bruteforce import BruteSBWT, int_to_words
from ms_brute import BruteMS, lcs_array, probe_reads
from oracle import OracleIndex
from sbwt_amd import capi


def tiny(k):
    rng = random.Random(k)
    g = "".join(rng.choice("ACGT") for _ in range(k + 70))
    a, b = 20, k + 40
    g2 = g[:a] + ("A" if g[a] != "A" else "C") + g[a + 1:b] + ("G" if g[b] != "G" else "T") + g[b + 1:]
    seqs = [g, g2, g[30:30 + k + 2], "".join(rng.choice("ACGT") for _ in range(k + 1))]
    B = BruteSBWT(seqs, k)
    cols, ssup = B.columns()
    n = len(B.nodes)
    words = [int_to_words(c, n) for c in cols]
    return rng, seqs, B, words, int_to_words(ssup, n), n


@pytest.mark.parametrize("precalc", [0, 3])
@pytest.mark.parametrize("k", [65, 128, 255])
def test_oracle_beyond_its_constructors_limit_equals_the_definition(k, precalc):
    rng, seqs, B, words, ssup, n = tiny(k)
    assert 200 <= n <= 1500 and any(len(e) >= 2 for e in B.edges) and 0 in B.ssup
    orc = OracleIndex.from_bits(*words, ssup, n, k, len(B.kmers), precalc)
    plain = OracleIndex.from_bits(*words, None, n, k, len(B.kmers), precalc)
    assert OracleIndex.build([s.encode() for s in seqs], 64).k == 64
    with pytest.raises(RuntimeError):
        OracleIndex.build([s.encode() for s in seqs], k)           # the one stated limit: its constructor
    reads = probe_reads(seqs, k, rng)
    # search, streaming search
    for r in reads:
        want = np.array(B.search_all(r.decode("latin-1")), dtype=np.int64)
        assert np.array_equal(orc.search_all(r), want) and np.array_equal(plain.search_all(r), want)
        if r == r.upper():                                          # (a lower-case base: the two loops differ by design)
            assert np.array_equal(orc.streaming_search(r), want)
    assert sum((orc.search_all(r) >= 0).sum() for r in reads) > 100
    # matching statistics, exhaustive and with the len[i - 1] + 1 shortcut
    M = BruteMS(B)
    bases, off = capi.concat_reads(reads)
    want = [np.concatenate([np.array(M.read(r)[j], dtype=np.int64) for r in reads]) for j in range(3)]
    for exhaustive in (True, False):
        ln, first, second, _ = orc.matching_statistics(bases, off, 2, exhaustive)
        assert np.array_equal(ln, want[0]) and np.array_equal(first, want[1]) and np.array_equal(second, want[2])
    assert want[0].max() == k
    # LCS, labels, marks
    assert np.array_equal(orc.lcs(), np.array(lcs_array(B), dtype=np.uint8))
    for j, lab in enumerate(B.nodes):
        assert orc.get_kmer(j) == ("$" * (k - len(lab)) + lab).encode()
    assert np.array_equal(plain.mark_suffix_groups(), ssup)
    # select, forward
    for ci, ch in enumerate("ACGT"):
        ones = [i for i, e in enumerate(B.edges) if ch in e]
        for j, col in enumerate(ones):
            assert orc.select(j + 1, ch.encode()) == col
    group = 0
    for v, lab in enumerate(B.nodes):
        group = v if B.ssup[v] else group
        for ch in "ACGT":
            nxt = (lab + ch)[-k:]
            assert orc.forward(v, ch.encode()) == (B.rank_of[nxt] if ch in B.edges[group] else -1)
    # update_interval from the whole range and partial_search: the interval of the labels that end with the pattern
    g = seqs[0]
    for L in (1, 30, 31, 32, 33, 63, 64, 65, k - 1, k):
        for s in (g[7:7 + L], g[k - 3:k - 3 + L], seqs[1][15:15 + L], "".join(rng.choice("ACGT") for _ in range(L))):
            s = s[:L]
            assert orc.update_interval(s.encode(), 0, n - 1) == M.iv.get(s, (-1, -1))
            m = max(j for j in range(len(s) + 1) if s[:j] in M.iv)
            assert orc.partial_search(s.encode()) == (M.iv[s[:m]], m)
            assert orc.partial_search(s.lower().encode()) == (M.iv[s[:m]], m)


def test_builders_agree_at_k_64_on_the_shared_case():
    case = long_k_cases.build_case(64)
    own = OracleIndex.build(case.seqs, 64, True, case.revcomp, 0)
    assert own.n_nodes == case.bits.n_nodes and own.n_kmers == case.bits.n_kmers
    for a, b in zip(own.columns(), case.bits.cols):
        assert np.array_equal(a, b)
    assert np.array_equal(own.ssup_words(), case.bits.ssup)
    assert np.array_equal(case.orc_nomarks.mark_suffix_groups(), case.bits.ssup)
    sbwt_verify.check_build(case.seqs, 64, case.revcomp, case.bits, host=None, verify=True)


@pytest.mark.parametrize("k", long_k_cases.KS)
def test_shared_cases_are_not_vacuous(k):
    case = long_k_cases.build_case(k)
    c = long_k_cases.check_non_vacuous(case)
    print("long-k case:", c)
    lens = np.diff(case.off)
    for L in (0, k - 1, k, k + 1, 480, 1500):
        assert (lens == L).any(), L
    assert lens.max() == 1500 and (lens[lens > 0].min() <= k - 1)
    present = set(np.unique(case.bases).tolist())
    assert {0, ord("N"), ord("a"), ord("n"), 0x80, 0xFF} <= present
    assert len(case.want_streaming) == len(case.want_search) == int(case.out_off[-1])
    # the marks the case carries are the ones the oracle derives from the rows alone
    assert np.array_equal(case.orc_nomarks.mark_suffix_groups(), case.bits.ssup)
    # reverse complements: in the index only where it was built with them
    g = case.strains[0][100:100 + k + 20]
    from sbwt_amd import synth
    rc_found = (case.orc.search_all(synth.revcomp(g).tobytes()) >= 0).all()
    assert (case.orc.search_all(g.tobytes()) >= 0).all() and rc_found == case.revcomp


def test_image_header_view_matches_the_offsets_read_by_hand():
    # (tests/test_gpu_parity.py reads big_layout at byte 160, tools/ab_step.py off_pos at byte 176)
    H = capi.ImageHeader
    assert H.big_layout.offset == 160 and H.off_pos.offset == 176 and H.k.offset == 24 and H.n_mega.offset == 88
