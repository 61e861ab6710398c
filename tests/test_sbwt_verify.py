"""The definition-level verifier (sbwt_verify.py) itself, without a GPU: it accepts what three independent constructions
give (the pure-Python brute force, the oracle's restatement of the reference constructor, the threaded host builder --
the host builder on the benchmark's config-2 input and on the read sets of test_gpu_build_scale.py at reduced size),
and sbwt_verify.check_build -- the function the device builder's tests call -- refuses every kind of damage a builder
could do: through the verifier alone, and through the bit-for-bit comparison alone."""
import json
import os
import sys

import numpy as np
import pytest

import sbwt_verify as V
from bruteforce import BruteSBWT, int_to_words
from oracle import OracleIndex
from sbwt_amd import hostlib, synth

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "ref_kats.json")))


def cores():
    sys.path.insert(0, os.path.dirname(HERE))
    import bench
    return bench.effective_cores()


class Rows:
    """Five rows as one bit per byte, to damage them column by column."""

    def __init__(self, src):
        n = src.n_nodes
        self.n_nodes, self.n_kmers = n, src.n_kmers
        self.bits = [np.unpackbits(np.asarray(w, dtype=np.uint64)[:(n + 63) // 64].view(np.uint8),
                                   bitorder="little")[:n].copy() for w in list(src.cols) + [src.ssup]]

    @staticmethod
    def _words(b):
        pad = np.zeros((-len(b)) % 64, dtype=np.uint8)
        return np.packbits(np.concatenate([b, pad]), bitorder="little").view(np.uint64)

    @property
    def cols(self):
        return [self._words(b) for b in self.bits[:4]]

    @property
    def ssup(self):
        return self._words(self.bits[4])

    def copy(self):
        r = Rows.__new__(Rows)
        r.n_nodes, r.n_kmers, r.bits = self.n_nodes, self.n_kmers, [b.copy() for b in self.bits]
        return r

    def without_column(self, j):
        r = self.copy()
        r.bits = [np.delete(b, j) for b in r.bits]
        r.n_nodes -= 1
        return r


def brute_rows(seqs, k, rc):
    b = BruteSBWT([s.decode("latin-1") for s in seqs], k, rc)
    cols, ssup = b.columns()
    n = len(b.nodes)

    class R:
        pass
    r = R()
    r.cols, r.ssup, r.n_nodes, r.n_kmers = [int_to_words(c, n) for c in cols], int_to_words(ssup, n), n, len(b.kmers)
    return r, b


def oracle_rows(seqs, k, rc):
    o = OracleIndex.build(seqs, k, True, rc, 0)

    class R:
        pass
    r = R()
    r.cols, r.ssup, r.n_nodes, r.n_kmers = o.columns(), o.ssup_words(), o.n_nodes, o.n_kmers
    return r


def test_accepts_reference_known_answers():
    kat = KATS["cli_end_to_end"]
    seqs = [s.encode() for s in kat["seqs"]]
    for r in (brute_rows(seqs, kat["k"], True)[0], oracle_rows(seqs, kat["k"], True)):
        assert (r.n_nodes, r.n_kmers) == (87, 73)
        V.verify_plain_matrix(seqs, kat["k"], True, r.cols, r.ssup, r.n_nodes, r.n_kmers)
    for case in KATS["small_cases"]["cases"]:
        seqs = [s.encode() for s in case["seqs"]]
        for rc in (False, True):
            r, b = brute_rows(seqs, case["k"], rc)
            lab = V.verify_plain_matrix(seqs, case["k"], rc, r.cols, r.ssup, r.n_nodes, r.n_kmers)
            got = [row.tobytes().decode() for row in V.labels_ascii(lab, case["k"], 0, r.n_nodes)]
            assert got == ["$" * (case["k"] - len(x)) + x for x in b.nodes], case["name"]
            r = oracle_rows(seqs, case["k"], rc)
            V.verify_plain_matrix(seqs, case["k"], rc, r.cols, r.ssup, r.n_nodes, r.n_kmers)


def build_test_seqs(k, rc):
    """The input of test_gpu_build.py::test_random_inputs_equal_oracle_constructor."""
    rng = np.random.default_rng(100 * k + rc)
    g0 = synth.random_genome(3000, 5 + k)
    seqs = [g0.tobytes(), synth.mutate(g0, 0.03, 9).tobytes()]
    for _ in range(30):
        L = int(rng.integers(0, 3 * k + 5))
        seqs.append(synth.random_genome(L, int(rng.integers(1, 1 << 30))).tobytes())
    noisy = bytearray(synth.random_genome(400, 77).tobytes())
    noisy[50] = ord("N"); noisy[51] = ord("N"); noisy[200] = ord("a"); noisy[399] = ord("$")
    return seqs + [bytes(noisy), b"", b"ACGT" * 40, b"A" * 70]


@pytest.mark.parametrize("k", [2, 3, 7, 16, 21, 30, 31, 32, 33, 48, 63, 64])
@pytest.mark.parametrize("rc", [False, True])
def test_accepts_brute_force_oracle_and_host_builder(k, rc):
    seqs = build_test_seqs(k, rc)
    r, b = brute_rows(seqs, k, rc)
    lab = V.verify_plain_matrix(seqs, k, rc, r.cols, r.ssup, r.n_nodes, r.n_kmers)
    got = [row.tobytes().decode() for row in V.labels_ascii(lab, k, 0, r.n_nodes)]
    assert got == ["$" * (k - len(x)) + x for x in b.nodes]
    o = oracle_rows(seqs, k, rc)
    V.verify_plain_matrix(seqs, k, rc, o.cols, o.ssup, o.n_nodes, o.n_kmers)
    h = hostlib.build_bits(seqs, k, rc, True, n_threads=2)
    V.check_build(seqs, k, rc, h, host=o)
    V.check_build(seqs, k, rc, hostlib.build_bits(seqs, k, rc, False), host=o)      # without ssup


def test_host_builder_on_config2_input():
    """The benchmark's config-2 index (coli3_like(5 Mbp), k = 30; 12.8 M columns) from the host builder."""
    seqs = [g.tobytes() for g in synth.coli3_like(5_000_000)]
    h = hostlib.build_bits(seqs, 30, False, True, n_threads=cores())
    assert h.n_nodes > 12_000_000
    V.check_build(seqs, 30, False, h)


# the inputs of test_gpu_build_scale.py at a size the CPU suite can afford
SMALL_INPUTS = {
    "random_reads_k31": lambda: (V.random_read_set(20_000, 100, 31, 7), 31, False),
    "random_reads_k40": lambda: (V.random_read_set(20_000, 100, 40, 7), 40, False),
    "sampled_reads": lambda: (V.sampled_read_set(100_000, 40_000, 11), 31, False),
    "repeated_genome": lambda: (V.repeated_genome_set(200_000, 5), 31, True),
    "coli_k32_rc": lambda: ([g.tobytes() for g in synth.coli3_like(100_000)], 32, True),
    "coli_k63": lambda: ([g.tobytes() for g in synth.coli3_like(100_000)], 63, False),
    "coli_k33_rc": lambda: ([g.tobytes() for g in synth.coli3_like(100_000)], 33, True),
    "no_kmers": lambda: (V.no_kmer_set(5_000, 31), 31, False),
}


@pytest.mark.parametrize("name", sorted(SMALL_INPUTS))
def test_host_builder_on_scale_inputs_at_reduced_size(name):
    seqs, k, rc = SMALL_INPUTS[name]()
    h = hostlib.build_bits(seqs, k, rc, True, n_threads=cores())
    V.check_build(seqs, k, rc, h)
    if name.startswith("random_reads"):
        # dummy-heavy as meant: 20 000 random prefixes of 12 or more chars (4^12 = 1.7e7 values) are nearly all distinct
        assert h.n_nodes - h.n_kmers > 0.99 * 20_000 * (k - 12)
    if name == "no_kmers":
        assert (h.n_nodes, h.n_kmers) == (1, 0)


# ---- mutations: check_build must refuse each, by the verifier alone and by the bit-for-bit comparison alone ----
def _group_with_two_columns_and_a_one(r):
    ssup = r.bits[4]
    for j in range(1, r.n_nodes - 1):
        if ssup[j] and not ssup[j + 1]:
            for c in range(4):
                if r.bits[c][j]:
                    return j, c
    raise AssertionError("no group of two columns with an edge")


def mutations(r, lab, k):
    """(name, damaged rows) for every kind of damage of the issue's list, at places taken from the accepted rows."""
    full = lab.length == k
    kmer_cols, dummy_cols = np.flatnonzero(full), np.flatnonzero(~full)
    out = []
    j = int(kmer_cols[len(kmer_cols) // 2])
    for c in range(4):                                     # one edge bit flipped: a one cleared, a zero set
        m = r.copy(); m.bits[c][j] ^= 1
        out.append(("edge bit %d of column %d flipped" % (c, j), m))
    for jj in (1, j, r.n_nodes - 1):
        m = r.copy(); m.bits[4][jj] ^= 1
        out.append(("ssup bit %d flipped" % jj, m))
    for jj in (int(dummy_cols[-1]), j, int(kmer_cols[0]) - 1):    # two neighbours swapped (all five rows)
        # swapping two columns with the same five bits changes nothing: take the nearest pair that differs
        near = sorted(range(1, r.n_nodes - 1), key=lambda x: abs(x - jj))
        jj = next(x for x in near if any(b[x] != b[x + 1] for b in r.bits))
        m = r.copy()
        for b in m.bits:
            b[jj], b[jj + 1] = b[jj + 1], b[jj]
        out.append(("columns %d and %d swapped" % (jj, jj + 1), m))
    for jj in (int(dummy_cols[1]), int(dummy_cols[len(dummy_cols) // 2]), int(dummy_cols[-1])):
        out.append(("dummy column %d removed" % jj, r.without_column(jj)))
    for jj in (int(kmer_cols[0]), j, int(kmer_cols[-1])):
        out.append(("k-mer column %d removed" % jj, r.without_column(jj)))
        m = r.without_column(jj); m.n_kmers -= 1
        out.append(("k-mer column %d removed and n_kmers lowered" % jj, m))
    g, c = _group_with_two_columns_and_a_one(r)
    m = r.copy(); m.bits[c][g] = 0; m.bits[c][g + 1] = 1
    out.append(("one of row %d moved from group start %d to the next column" % (c, g), m))
    for d in (-1, 1):
        m = r.copy(); m.n_kmers += d
        out.append(("n_kmers off by %d" % d, m))
    return out


MUTATION_INPUTS = {
    "random_reads_k31": lambda: (V.random_read_set(3_000, 100, 31, 7), 31, False),
    "random_reads_k40": lambda: (V.random_read_set(3_000, 100, 40, 7), 40, False),
    "sampled_reads": lambda: (V.sampled_read_set(30_000, 6_000, 11), 31, False),
    "repeated_genome": lambda: (V.repeated_genome_set(50_000, 5), 31, True),
    "coli_k30": lambda: ([g.tobytes() for g in synth.coli3_like(50_000)], 30, False),
    "coli_k32_rc": lambda: ([g.tobytes() for g in synth.coli3_like(50_000)], 32, True),
    "coli_k63": lambda: ([g.tobytes() for g in synth.coli3_like(50_000)], 63, False),
    "coli_k33_rc": lambda: ([g.tobytes() for g in synth.coli3_like(50_000)], 33, True),
}


def mutation_input(name):
    """The input + two sequences that differ in their first base only: a suffix group of two columns with an edge, which
    unrelated random reads would not have."""
    seqs, k, rc = MUTATION_INPUTS[name]()
    core = synth.random_genome(k + 3, 99).tobytes()
    return seqs + [b"A" + core, b"C" + core], k, rc


@pytest.mark.parametrize("name", sorted(MUTATION_INPUTS))
def test_check_build_refuses_every_mutation(name):
    seqs, k, rc = mutation_input(name)
    host = hostlib.build_bits(seqs, k, rc, True, n_threads=2)
    r = Rows(host)
    lab = V.check_build(seqs, k, rc, r, host=host)                       # the undamaged rows pass both
    muts = mutations(r, lab, k)
    assert len(muts) == 22
    for what, m in muts:
        with pytest.raises(V.VerifyError):
            V.check_build(seqs, k, rc, m, host=None, verify=True)
            pytest.fail("the verifier accepts: " + what)
        with pytest.raises(V.VerifyError):
            V.check_build(seqs, k, rc, m, host=host, verify=False)
            pytest.fail("the bit-for-bit comparison accepts: " + what)


def test_check_build_refuses_without_streaming_support_too():
    """ssup is None: the rows alone must still be refused when damaged."""
    seqs, k, rc = mutation_input("random_reads_k31")
    host = hostlib.build_bits(seqs, k, rc, True, n_threads=2)
    r = Rows(host)
    lab = V.check_build(seqs, k, rc, r, host=host)

    class NoSsup:
        def __init__(self, m):
            self.cols, self.ssup, self.n_nodes, self.n_kmers = m.cols, None, m.n_nodes, m.n_kmers
    V.check_build(seqs, k, rc, NoSsup(r), host=host)
    for what, m in mutations(r, lab, k):
        if what.startswith("ssup"):
            continue
        with pytest.raises(V.VerifyError):
            V.check_build(seqs, k, rc, NoSsup(m), host=None, verify=True)
            pytest.fail("the verifier accepts: " + what)
        with pytest.raises(V.VerifyError):
            V.check_build(seqs, k, rc, NoSsup(m), host=host, verify=False)
            pytest.fail("the bit-for-bit comparison accepts: " + what)


def test_rows_shorter_or_dirtier_than_n_nodes_are_refused():
    seqs = [b"ACGTACGGTCA"]
    h = hostlib.build_bits(seqs, 4, False, True)
    V.check_build(seqs, 4, False, h)
    with pytest.raises(V.VerifyError):
        V.verify_plain_matrix(seqs, 4, False, [c[:0] for c in h.cols], h.ssup, h.n_nodes, h.n_kmers)
    dirty = [c.copy() for c in h.cols]
    dirty[2][-1] |= np.uint64(1) << np.uint64(63)                        # a bit beyond column n_nodes - 1
    assert h.n_nodes % 64 != 0
    with pytest.raises(V.VerifyError):
        V.verify_plain_matrix(seqs, 4, False, dirty, h.ssup, h.n_nodes, h.n_kmers)
