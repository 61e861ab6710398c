"""The definition of the per-read hit profile (tests/read_hits_brute.py) on hand-written cases and on random sets, and the
declaration of the feature in the C ABI.  No GPU."""
import os
import random
import re

from bruteforce import BruteSBWT
from read_hits_brute import covered_sum_min, covered_union, hits, longest_run, profile, revcomp
from sbwt_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K3 = {"ACG", "CGT", "GTA", "TTT", "GGG", "GGC"}


def test_hand_written_cases_k3():
    k = 3
    # two runs whose covers overlap: hits at 0, 1 (ACG, CGT) and at 3 (TTT): [0, 5) and [3, 6) -> 6 bases
    assert hits(K3, k, "ACGTTT") == [1, 1, 0, 1]
    assert profile(K3, k, "ACGTTT") == (4, 3, 6, 2)
    # two runs whose covers do not overlap: hits at 0 and at 4: [0, 3) and [4, 7)
    assert hits(K3, k, "ACGATTT") == [1, 0, 0, 0, 1]
    assert profile(K3, k, "ACGATTT") == (5, 2, 6, 1)
    # all hits; no hits
    assert profile(K3, k, "ACGTA") == (3, 3, 5, 3)
    assert profile(K3, k, "TTTTTT") == (4, 4, 6, 4)
    assert profile(K3, k, "CCCCCC") == (4, 0, 0, 0)
    # L < k; L = k; the empty read
    assert profile(K3, k, "AC") == (0, 0, 0, 0)
    assert profile(K3, k, "") == (0, 0, 0, 0)
    assert profile(K3, k, "ACG") == (1, 1, 3, 1)
    assert profile(K3, k, "ACC") == (1, 0, 0, 0)
    # N and lower case inside a window: no hit, in either mode
    assert hits(K3, k, "ACGNTTT") == [1, 0, 0, 0, 1]
    assert hits(K3, k, "ACgTTT") == [0, 0, 0, 1]
    assert hits(K3, k, "ACgTTT", 2) == [0, 0, 0, 1]
    assert profile(K3, k, b"ACG\x00TTT") == (5, 2, 6, 1)
    # a read that hits only as its reverse complement: rc(GCC) = GGC, rc(CCC) = GGG
    assert profile(K3, k, "GCCC") == (2, 0, 0, 0)
    assert profile(K3, k, "GCCC", 2) == (2, 2, 4, 2)
    # the complement is defined on upper-case bytes only
    assert revcomp("ACGTNacgt") == "tgcaNACGT"
    assert profile(K3, k, "GcCC", 2) == (2, 0, 0, 0)


def random_read(rng, n):
    return "".join(rng.choice("ACGT" if rng.random() < 0.97 else "Nacgt") for _ in range(n))


def test_sum_min_form_equals_union_form():
    rng = random.Random(3)
    for trial in range(300):
        k = rng.randint(1, 12)
        n = rng.randint(0, 120)
        dens = rng.random()
        hit = [1 if rng.random() < dens else 0 for _ in range(n)]
        assert covered_sum_min(hit, k) == covered_union(hit, k), (k, hit)
        assert longest_run(hit) == max([len(x) for x in "".join(map(str, hit)).split("0")] + [0])
    for k in (2, 3, 5, 8):
        B = BruteSBWT(["".join(rng.choice("ACGT") for _ in range(200)) for _ in range(3)], k)
        for _ in range(40):
            read = random_read(rng, rng.randint(0, 80))
            for strands in (1, 2):
                h = hits(B.kmers, k, read, strands)
                assert covered_sum_min(h, k) == covered_union(h, k)
                assert len(h) == max(0, len(read) - k + 1)


def test_strand_symmetries():
    rng = random.Random(4)
    for k in (2, 3, 4, 7):
        seqs = ["".join(rng.choice("ACGT") for _ in range(60)) for _ in range(3)]
        fwd, closed = BruteSBWT(seqs, k), BruteSBWT(seqs, k, True)
        assert closed.kmers == fwd.kmers | {revcomp(x) for x in fwd.kmers}
        for _ in range(60):
            read = random_read(rng, rng.randint(0, 50))
            # on a reverse-complement-closed set the second strand adds nothing
            assert profile(closed.kmers, k, read, 2) == profile(closed.kmers, k, read, 1)
            # the profile of rc(read) under both strands is that of the read: the hits are mirrored
            assert profile(fwd.kmers, k, revcomp(read), 2) == profile(fwd.kmers, k, read, 2)
            assert hits(fwd.kmers, k, revcomp(read), 2) == hits(fwd.kmers, k, read, 2)[::-1]
            # both strands on a forward-only set = one strand on its closure
            assert hits(fwd.kmers, k, read, 2) == hits(closed.kmers, k, read, 1)
            assert profile(fwd.kmers, k, read, 2)[1] >= profile(fwd.kmers, k, read, 1)[1]


def test_abi_declares_read_hits():
    header = open(os.path.join(ROOT, "include", "sbwtgpu.h")).read()
    names = ("sbwtgpu_read_hits_batch", "sbwtgpu_read_hits_workspace_bytes", "sbwtgpu_read_hits_dev")
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS
        getattr(capi.lib(), name)              # exported by the built library
    assert re.search(r"int32_t\s+n_kmers,\s*n_found,\s*covered_bases,\s*longest_run;\s*}\s*sbwtgpu_read_hits;", header)
    # sizing needs no device: non-decreasing in the bases and in the reads, larger for two strands
    w = [capi.read_hits_workspace_bytes(b, 1000) for b in (0, 1, 1000, 10**6, 10**6 + 1, 10**9)]
    assert w == sorted(w) and w[0] > 0
    assert capi.read_hits_workspace_bytes(10**6, 10**5) >= capi.read_hits_workspace_bytes(10**6, 1000)
    assert capi.read_hits_workspace_bytes(10**6, 1000, True) > capi.read_hits_workspace_bytes(10**6, 1000)
    assert capi.read_hits_workspace_bytes(10**6, 1000) >= capi.search_workspace_bytes(10**6) + 8 * 10**6
