"""The CPU half of tools/fuzz_derived.py alone: the committed seeds' draws are replayed, every expected value is computed
(where a case has two references of one thing -- the oracle's matching statistics and LCS against ms_brute, the numpy unitigs
against unitig_brute -- expected() holds them against each other), and the fuzz is shown not to be vacuous: every category
below occurs in three cases at least.  These are conditions on the draws, chosen with the seeds; none is a measurement."""
import ast
import os
import random
import sys

import numpy as np
import pytest

from bruteforce import BruteSBWT
from unitig_brute import brute_unitigs, flatten
import unitig_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_derived as F          # noqa: E402

KNOB_VALUES = ["path_lookahead=0", "path_lookahead=1", "path_safe=0", "path_safe=1", "image_level=1", "image_level=2", "path_stitch=0",
               "path_stitch_min=4", "path_stitch_min=16", "force_mega=1", "big_path=2", "derive_ssup=0"]
REQUIRED = (["shape_" + s for s in F.SHAPES] + ["k<=4", "k=31", "k=32", "k=33", "k>=63", "rc", "no_marks"] + KNOB_VALUES +
            ["branching>=50", "dummy_heavy", "pure_cycle"] + ["b_" + b for b in F.B_KINDS] +
            ["op_empty", "op_equals_a", "op_between", "strands_differ", "windows>=4096", "read<k", "empty_read", "unitigs>=2", "unitigs=1"] +
            # and what the tool adds to the list: both references of a pair present, the loop through a device-made index, the
            # read-hit tunings, N / lower case in the input
            ["ms_brute", "unitig_refs_both", "device_index", "read_hits_tuning", "injected"])


def test_first_half_imports_nothing_of_the_gpu_path():
    tree = ast.parse(open(os.path.join(ROOT, "tools", "fuzz_derived.py")).read())
    names = []
    for node in tree.body:
        if isinstance(node, ast.Import):
            names += [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            names += ["%s.%s" % (node.module, a.name) for a in node.names]
    assert names and not [n for n in names if "capi" in n or "torch" in n], names


@pytest.fixture(scope="module")
def replay():
    """(case, expected) of every committed case; the references are computed once for the tests below"""
    return [(c, F.expected(c, n_threads=4)) for seed in F.SEEDS for c in (F.draw_case(seed, no) for no in range(1, F.N_CASES + 1))]


def test_draws_are_reproducible_and_within_the_limits(replay):
    for c, e in replay:
        again = F.draw_case(c.seed, c.no)
        assert again.seqs == c.seqs and again.seqs_b == c.seqs_b and again.knobs == c.knobs and again.extra_knob == c.extra_knob
        assert np.array_equal(again.bases, c.bases) and np.array_equal(again.off, c.off) and again.query_seed == c.query_seed
        assert e.bits.n_nodes <= 200_000 and e.bits_b.n_nodes <= 200_000 and len(c.bases) <= 2_000_000
        assert all(want.n_nodes <= 200_000 for want, _ in e.setops.values()) or "setop_device_index" not in e.applies
        assert e.unitigs, "a case without a unitig reference"
        assert c.k in F.K_CHOICES and 300 <= len(c.off) - 1 <= 1500 + 11


def test_the_fuzz_is_not_vacuous(replay):
    count = {t: sum(t in e.tags for _, e in replay) for t in REQUIRED}
    print("\n%d cases (seeds %s x %d); cases per category:" % (len(replay), list(F.SEEDS), F.N_CASES))
    for t in REQUIRED:
        print("  %-20s %d" % (t, count[t]))
    short = {t: n for t, n in count.items() if n < 3}
    assert not short, "categories in fewer than three cases: %s" % short


def test_references_were_held_against_each_other(replay):
    """expected() asserts the agreement; here: that it had pairs to compare, and that both unitig references were present
    wherever both apply"""
    assert sum(e.ref_checks for _, e in replay) >= 6
    for c, e in replay:
        assert ("numpy" in e.unitigs) == (c.k <= 31) and ("brute" in e.unitigs) == (e.bits.n_kmers <= 20_000)
        assert ("ms_brute" in e.applies) == (c.k <= 16 and e.bits.n_nodes < 3000)


def circular(s, k):
    return s + s[:k - 1]


@pytest.mark.parametrize("k", [2, 3, 5, 16, 31])
def test_numpy_unitigs_equal_the_brute_force(k):
    rng = random.Random(k)
    alphabet = "AC" if k <= 5 else "ACGT"

    def rnd(n):
        return "".join(rng.choice(alphabet) for _ in range(n))
    sets = [[rnd(rng.randint(1, 200)) for _ in range(rng.randint(1, 12))] + [rnd(k)] for _ in range(4)]
    sets += [[circular(rnd(k + 7), k)], [circular(rnd(k + 7), k), rnd(k + 3) + circular(rnd(k + 11), k)], ["A" * (k + 2)], ["ACNGT" * k]]
    for seqs in sets:
        seqs[0] = seqs[0][: len(seqs[0]) // 2] + "n" + seqs[0][len(seqs[0]) // 2:]
        B = BruteSBWT(seqs, k)
        U, first = brute_unitigs(B)
        K = unitig_numpy.key_set([np.frombuffer(s.encode(), dtype=np.uint8) for s in seqs], k)
        assert len(K) == len(B.kmers)
        bases, off, idx = unitig_numpy.unitigs_of_keys(K, k)
        real = [j for j, s in enumerate(B.nodes) if len(s) == k]
        assert (bases.tobytes(), off.tolist()) == flatten(U)
        assert [real[i] for i in idx] == first
