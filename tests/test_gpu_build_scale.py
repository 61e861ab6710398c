"""GPU: the device index builder (sbwtgpu_build_plain_matrix) at the sizes the benchmark and the full-size tests trust
it at, and on read sets, where the predecessor-less k-mers are not few.

Every input is compared on ALL columns with at least one independent reference, through sbwt_verify.check_build (the
function whose rejections test_sbwt_verify.py proves on damaged rows of the same inputs at reduced size):
  (a) the definition-level numpy verifier, where the index has at most about 3 x 10^7 columns: the config-2 genomes at
      k = 30, 32 (+rc), 63 and 33 (+rc) (12.8 M .. 26.3 M columns), the repeated genome (10 M) and the input without
      k-mers (1 column);
  (b) the threaded host builder, bit for bit on the four rows, ssup, n_nodes and n_kmers: every input.  The read sets
      (90.8 M, 90.8 M and 86.0 M columns) and the 65-genome pan-genome (142 M columns) have (b) alone;
  and the rows built without streaming support (ssup is None) are the same rows.

Then the two C ABI kernels that read an index column by column, on the config-2 index and on the dummy-heavy read-set
index, against numpy on the rows: get_kmers of every column, select of every one of every row, rank at every block
boundary, at every position of the last two blocks and at n_nodes."""
import os
import sys
import time

import numpy as np
import pytest

import sbwt_verify as V
from sbwt_amd import capi, hostlib, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 4_000_000                       # columns per get_kmers / select call


def cores():
    sys.path.insert(0, ROOT)
    import bench
    return bench.effective_cores()


def build_and_check(name, seqs, k, rc, verify):
    """Host builder, device builder with and without streaming support, check_build; prints the times NOTES.md quotes."""
    t0 = time.time()
    host = hostlib.build_bits(seqs, k, rc, True, n_threads=cores())
    t1 = time.time()
    got = capi.build_bits_gpu(seqs, k, rc, True)
    t2 = time.time()
    lab = V.check_build(seqs, k, rc, got, host=host, verify=verify)
    t3 = time.time()
    no_ssup = capi.build_bits_gpu(seqs, k, rc, False)
    assert no_ssup.ssup is None
    V.check_build(seqs, k, rc, no_ssup, host=host, verify=False)
    print("\n[build-scale] %s k=%d rc=%d: %d columns = %d k-mers + %d dummies; host builder %.1f s, device builder %.1f s, "
          "%s %.1f s" % (name, k, rc, got.n_nodes, got.n_kmers, got.n_nodes - got.n_kmers, t1 - t0, t2 - t1,
                         "verifier + comparison" if verify else "comparison", t3 - t2), flush=True)
    return got, lab


def column_api_equals_numpy(got, k, lab):
    """get_kmers / select / rank over the whole index against numpy on the rows."""
    n = got.n_nodes
    idx = capi.Index.create(got.cols[0], got.cols[1], got.cols[2], got.cols[3], got.ssup, n, k, got.n_kmers, 8)
    t0 = time.time()
    for lo in range(0, n, CHUNK):
        hi = min(n, lo + CHUNK)
        kmers = idx.get_kmers(np.arange(lo, hi, dtype=np.int64))
        assert np.array_equal(kmers, V.labels_ascii(lab, k, lo, hi)), "get_kmers differs in columns [%d, %d)" % (lo, hi)
    t1 = time.time()
    edge = np.concatenate([np.arange(0, n + 1, 64), np.arange(max(0, (n // 64 - 1) * 64), n + 1), [n]]).astype(np.int64)
    for c, ch in enumerate(b"ACGT"):
        bits = np.unpackbits(got.cols[c].view(np.uint8), bitorder="little")[:n]
        ones = np.flatnonzero(bits)
        for lo in range(0, len(ones), CHUNK):
            hi = min(len(ones), lo + CHUNK)
            sel = idx.select(np.arange(lo + 1, hi + 1, dtype=np.int64), np.full(hi - lo, ch, dtype=np.uint8))
            assert np.array_equal(sel, ones[lo:hi]), "select differs in row %s, ones [%d, %d)" % (chr(ch), lo, hi)
        with pytest.raises(capi.SbwtGpuError):
            idx.select(np.array([len(ones) + 1]), np.array([ch], dtype=np.uint8))
        before = np.concatenate([[0], np.cumsum(bits, dtype=np.int64)])      # ones in [0, pos)
        assert np.array_equal(idx.rank(edge, np.full(len(edge), ch, dtype=np.uint8)), before[edge]), chr(ch)
    print("[build-scale] column API over %d columns: get_kmers %.1f s, select + rank %.1f s"
          % (n, t1 - t0, time.time() - t1), flush=True)
    idx.close()


def coli_seqs():
    return [g.tobytes() for g in synth.coli3_like(5_000_000)]


def test_config2_index_k30_and_its_column_api(gpu):
    seqs = coli_seqs()
    got, lab = build_and_check("coli3_like(5M)", seqs, 30, False, verify=True)
    assert got.n_nodes > 12_000_000
    column_api_equals_numpy(got, 30, lab)


@pytest.mark.parametrize("k,rc", [(32, True), (63, False), (33, True)])
def test_config2_genomes_at_the_key_width_edges(gpu, k, rc):
    """k = 32 fills the 64-bit key and the sort's last digit; 63 and 33 are 128-bit keys (63: config 5's index)."""
    got, _ = build_and_check("coli3_like(5M)", coli_seqs(), k, rc, verify=True)
    assert got.n_nodes > 14_000_000


def test_config3_pangenome_equals_host_builder(gpu):
    """synth.pan_like(64, 5 Mbp), k = 31: the 142 M-column index test_gpu_fullsize.py builds its oracle from."""
    seqs = [g.tobytes() for g in synth.pan_like(64, 5_000_000)]
    got, _ = build_and_check("pan_like(64, 5M)", seqs, 31, False, verify=False)
    assert got.n_nodes > 140_000_000


def test_random_reads_k31_and_the_column_api_on_skewed_rows(gpu):
    """1 M unrelated reads: 20.8 M dummy columns through the host-made dummy list and the merged emission.  The `$`-padded
    region holds most of the zeros of the rows: select's interpolated first guess is far off there."""
    seqs = V.random_read_set(1_000_000, 100, 31, 7)
    got, _ = build_and_check("random_read_set(1M x 100)", seqs, 31, False, verify=False)
    # prefixes of 14 .. k-1 chars (4^14 = 2.7e8 values) of 1 M random reads are nearly all distinct: 17 lengths at k = 31
    assert got.n_nodes - got.n_kmers > 0.99 * 17 * 1_000_000
    del seqs
    lab, _, _ = V.labels_from_rows(got.cols, got.n_nodes, 31)           # the rows are the host builder's, bit for bit
    column_api_equals_numpy(got, 31, lab)


def test_random_reads_k40(gpu):
    seqs = V.random_read_set(1_000_000, 100, 40, 7)
    got, _ = build_and_check("random_read_set(1M x 100)", seqs, 40, False, verify=False)
    assert got.n_nodes - got.n_kmers > 0.99 * 26 * 1_000_000               # lengths 14 .. 39


def test_sampled_reads_with_substitutions(gpu):
    """2 M x 150 bases at 1 % substitutions from the config-2 genomes: deep overlap, dummies where errors and coverage
    gaps leave a k-mer without a predecessor."""
    seqs = V.sampled_read_set(5_000_000, 2_000_000, 11)
    got, _ = build_and_check("sampled_read_set(5M, 2M x 150)", seqs, 31, False, verify=False)
    assert got.n_nodes - got.n_kmers > 100_000                         # the genomes themselves have about 100


def test_one_genome_eighteen_times(gpu):
    """nv = 18 x nk: the distinct-compaction with long runs of equal keys."""
    seqs = V.repeated_genome_set(5_000_000, 5)
    got, _ = build_and_check("repeated_genome_set(5M)", seqs, 31, True, verify=True)
    assert got.n_kmers > 9_900_000


def test_a_million_sequences_without_a_kmer(gpu):
    seqs = V.no_kmer_set(1_000_000, 31)
    got, _ = build_and_check("no_kmer_set(1M)", seqs, 31, True, verify=True)
    assert (got.n_nodes, got.n_kmers) == (1, 0) and int(got.ssup[0]) == 1
    assert all(int(c[0]) == 0 for c in got.cols)
