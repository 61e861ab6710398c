"""Shared cases of the k >= 64 tests (tests/test_long_k_cpu.py, tests/test_gpu_long_k.py): one branching, multi-block index
and one batch of reads per k of the sweep, with the oracle's answers, built once per process.

From k = 64 the device image has no second-level sparse table, batches leave the wide fused kernel for the general path
kernel and the paths carry no safe bits.  An index of a few hundred columns with one substitution cannot tell whether that
route is right, so every case here has

  index   four strains of one random genome (synth.random_genome + synth.mutate at 2, 2.5 and 3 %), one stretch of k + 50
          bases written into every strain at the same two places (a repeat longer than k, and a stretch all strains share), six
          unrelated sequences of k .. k + 3 bases (k dummy columns each), and N_STUBS sequences of k + 1 .. k + 3 bases that
          start with a k-mer of a strain and go on differently.  The stubs are there because substitutions alone cannot make a
          small index branch at large k: a column branches where a substitution follows k unchanged bases, which at 2 % happens
          with probability exp(-0.02 k) -- one substitution in 3.6 at k = 64, one in 160 at k = 255.  `branch_natural` of a case
          is the number of branching columns without the stubs.
          Columns come from the host builder (sbwt_amd.hostlib), with and without suffix-group marks; K_REVCOMP is built with
          reverse complements.  The reference index is OracleIndex.from_bits over those columns.
  reads   ragged reads of k - 2 .. 4 k + 60 bases, reads of 480 and of 1500 bases, all sampled from the strains at 0.5 %
          substitutions; reads of exactly k - 1, k and k + 1 bases and empty reads; reads that hop from one strain to another
          inside the shared stretch; reads of random sequence; the reverse complements of some reads; then N, lower case, NUL
          and bytes >= 0x80 written over random positions.

check_non_vacuous() asserts that a case is what it is meant to be; build_case() calls it, so no test can use a vacuous case.
"""
from __future__ import annotations

import functools
import os
from types import SimpleNamespace

import numpy as np

from oracle import OracleIndex
from sbwt_amd import capi, hostlib, synth

KS = (64, 65, 96, 128, 255)
K_REVCOMP = 96                  # this k's index holds reverse complements
GENOME_LEN = 8000
N_STUBS = 130
ORACLE_PRECALC = 8
N_THREADS = max(1, min(16, os.cpu_count() or 1))


def _sequences(k: int):
    g0 = synth.random_genome(GENOME_LEN, 1000 + k)
    strains = [g0] + [synth.mutate(g0, rate, 2000 + 10 * k + i) for i, rate in enumerate((0.02, 0.025, 0.03))]
    shared = synth.random_genome(k + 50, 3000 + k)
    at = (GENOME_LEN // 5, (3 * GENOME_LEN) // 5)
    for s in strains:
        for a in at:
            s[a:a + len(shared)] = shared
    rng = np.random.default_rng(4000 + k)
    lone = [synth.random_genome(k + (i % 4), 5000 + 10 * k + i) for i in range(6)]
    stubs = []
    for i in range(N_STUBS):
        s = strains[i % 4]
        a = int(rng.integers(0, GENOME_LEN - k - 4))
        tail = s[a + k:a + k + 1 + (i % 3)].copy()
        tail[0] = synth.mutate(tail[:1], 1.0, i)[0]                 # a base the strain does not have there
        stubs.append(np.concatenate([s[a:a + k], tail]))
    return strains, shared, at, lone, stubs


def _reads(k: int, strains, shared, at):
    rng = np.random.default_rng(6000 + k)
    parts = []

    def add(bases, off):
        parts.extend(bases[off[r]:off[r + 1]] for r in range(len(off) - 1))
    add(*synth.ragged_reads(strains, 700, k - 2, 4 * k + 60, 0.005, 7000 + k))
    add(*synth.sample_reads(strains, 120, 480, 0.005, 7100 + k))
    add(*synth.sample_reads(strains, 50, 1500, 0.005, 7200 + k))
    for L in (k - 1, k, k + 1):
        add(*synth.sample_reads(strains, 20, L, 0.0, 7300 + k + L))
    parts.extend(np.zeros(0, dtype=np.uint8) for _ in range(8))
    hop = []
    for i in range(60):                                             # strain a up to the shared stretch, strain b after it
        a, b = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        p = at[i % 2]
        cut = p + int(rng.integers(0, len(shared)))
        lo, hi = p - int(rng.integers(k // 2, 2 * k)), p + len(shared) + int(rng.integers(k // 2, 2 * k))
        hop.append(np.concatenate([strains[a][lo:cut], strains[b][cut:hi]]))
    parts.extend(hop)
    add(*synth.random_reads(60, 2 * k, 7400 + k))
    n_plain = len(parts)
    for r in rng.choice(n_plain, size=100, replace=False):
        if len(parts[r]):
            parts.append(synth.revcomp(parts[r]))
    order = rng.permutation(len(parts))                             # the kinds of reads interleaved: ragged batches
    parts = [parts[i] for i in order]
    bases, off = capi.concat_reads([p.tobytes() for p in parts])
    bases = synth.inject(bases, 40, ord("N"), 7500 + k)
    for j, ch in enumerate(b"acgtn"):
        bases = synth.inject(bases, 8, ch, 7600 + k + j)
    bases = synth.inject(bases, 10, 0, 7700 + k)
    for j, ch in enumerate((0x80, 0x81, 0xC1, 0xE7, 0xFF)):          # (0xC1, 0xE7: 'A' and 'g' with bit 7 set)
        bases = synth.inject(bases, 4, ch, 7800 + k + j)
    return bases, off


def oracle_of(bits, with_marks: bool = True, precalc: int = ORACLE_PRECALC) -> OracleIndex:
    return OracleIndex.from_bits(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup if with_marks else None,
                                 bits.n_nodes, bits.k, bits.n_kmers, precalc)


def oracle_results(orc: OracleIndex, bases, off):
    """orc.streaming_search (an oracle with marks) or orc.search_all (one without) of every read, by threads."""
    out, _ = orc.batch_search(bases, off, capi.out_offsets(off, orc.k), N_THREADS)
    return out


def branching_columns(bits) -> int:
    n = bits.n_nodes
    deg = sum(np.unpackbits(c.view(np.uint8), bitorder="little")[:n].astype(np.int8) for c in bits.cols)
    return int((deg >= 2).sum())


def conditions(case) -> dict:
    """The numbers the non-vacuity conditions are about."""
    bits, k = case.bits, case.k
    hit = case.want_search >= 0
    oo = case.out_off
    both = regain = 0
    for r in range(len(oo) - 1):
        h = hit[oo[r]:oo[r + 1]]
        if len(h) and h.any() and not h.all():
            both += 1
            first_miss = int(np.argmin(h))
            if h[:first_miss].any() and h[first_miss:].any():
                regain += 1
    marks = int(np.unpackbits(bits.ssup.view(np.uint8), bitorder="little")[:bits.n_nodes].sum())
    return {"k": k, "columns": bits.n_nodes, "kmers": bits.n_kmers, "dummies": bits.n_nodes - 1 - bits.n_kmers,
            "branching": branching_columns(bits), "branching_without_stubs": case.branch_natural,
            "groups_larger_than_one": bits.n_nodes - marks, "reads": len(case.off) - 1, "queried": int(len(hit)),
            "found_share": float(hit.mean()), "reads_with_hit_and_miss": both, "reads_regaining_hits": regain}


def check_non_vacuous(case) -> dict:
    c = conditions(case)
    assert c["columns"] >= 20_000, c
    assert c["dummies"] > 0, c
    assert c["branching"] >= 100, c
    assert c["groups_larger_than_one"] >= 1, c
    assert 0.20 <= c["found_share"] <= 0.95, c
    assert c["reads_with_hit_and_miss"] >= 100, c
    assert c["reads_regaining_hits"] >= 50, c
    return c


@functools.lru_cache(maxsize=None)
def build_case(k: int):
    strains, shared, at, lone, stubs = _sequences(k)
    revcomp = k == K_REVCOMP
    seqs = [s.tobytes() for s in strains + lone + stubs]
    bits = hostlib.build_bits(seqs, k, revcomp, True, n_threads=4)
    bits_nomarks = hostlib.build_bits(seqs, k, revcomp, False, n_threads=4)
    assert bits_nomarks.ssup is None and bits_nomarks.n_nodes == bits.n_nodes
    assert all(np.array_equal(a, b) for a, b in zip(bits.cols, bits_nomarks.cols))
    natural = hostlib.build_bits([s.tobytes() for s in strains + lone], k, revcomp, True, n_threads=4)
    bases, off = _reads(k, strains, shared, at)
    orc, orc_nomarks = oracle_of(bits), oracle_of(bits, False)
    case = SimpleNamespace(k=k, revcomp=revcomp, strains=strains, seqs=seqs, bits=bits, bits_nomarks=bits_nomarks, orc=orc,
                           orc_nomarks=orc_nomarks, bases=bases, off=off, out_off=capi.out_offsets(off, k),
                           branch_natural=branching_columns(natural))
    case.want_streaming = oracle_results(orc, bases, off)           # SBWT::streaming_search of every read
    case.want_search = oracle_results(orc_nomarks, bases, off)      # SBWT::search of every k-mer
    case.reads = [bases[off[r]:off[r + 1]].tobytes() for r in range(len(off) - 1)]
    case.conditions = check_non_vacuous(case)
    return case
