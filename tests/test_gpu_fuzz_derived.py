"""GPU fuzz of the derived queries under the -m gpu suite (tools/fuzz_derived.py, bounded by a case count): on random indexes
(k 2..64, the shapes of the search fuzz plus purely periodic inputs and sequences of k and k + 1 bases, with and without
reverse complements, marks, a prefix table, the image knobs) the column API, the LCS array, matching statistics, read hits on
one and two strands, the unitigs and the set operations with a second random index are held bit for bit against values
computed on the CPU.  The seeds and the case count are the tool's (SEEDS, N_CASES); tests/test_fuzz_derived_cpu.py shows what
they cover.  One case replays with `SEED=n python tools/fuzz_derived.py 5 case_no`."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_derived          # noqa: E402

ALWAYS = [f for f in fuzz_derived.FEATURES if f not in ("ms_brute", "unitigs_numpy", "unitigs_brute", "setop_device_index")]


@pytest.mark.parametrize("seed", fuzz_derived.SEEDS)
def test_derived_queries_equal_their_definitions(gpu, seed):
    stats = {}
    n = fuzz_derived.fuzz(seed, fuzz_derived.N_CASES, stats)
    print("\nseed %d: %d cases, %.1f s, of them %.1f s the expected values on the CPU" % (seed, n, stats["seconds"], stats["cpu_seconds"]))
    assert n == stats["cases"] == fuzz_derived.N_CASES
    # every feature was compared in every case it applies to: nothing left out on the way
    assert stats["compared"] == stats["applies"], stats
    for f in ALWAYS:
        assert stats["compared"][f] == fuzz_derived.N_CASES, (f, stats)
    assert stats["compared"]["unitigs_numpy"] + stats["compared"]["unitigs_brute"] >= fuzz_derived.N_CASES
