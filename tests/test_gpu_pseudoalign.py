"""GPU: the colour matrix and pseudoalignment (sbwt_colors.hip) against the definition-level brute force
(tests/pseudoalign_brute.py): every column of the matrix, the records and counts of probe reads, invariance under chunking,
image levels and the device entry point, every refusal, two host threads, the C++ CLI and a bounded seeded fuzz.
All comparisons are exact."""
import gzip
import json
import os
import random
import subprocess
import threading

import numpy as np
import pytest

import pseudoalign_brute as pb
from bruteforce import kmer_set
from sbwt_amd import capi, hostlib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_kats.json")))


def make_index(seqs, k, rc=False, ssup=True):
    bits = hostlib.build_bits([s.encode() if isinstance(s, str) else s for s in seqs], k, rc, ssup)
    return capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)


def index_kmers(seqs, k, rc):
    return kmer_set(list(seqs) + ([pb.revcomp(s) for s in seqs] if rc else []), k)


def labels_of(idx):
    return [bytes(row).decode() for row in idx.get_kmers(np.arange(idx.n_nodes))]


class tuning:
    """set_tuning for the length of a with-block"""

    def __init__(self, key, value, back):
        self.key, self.value, self.back = key, value, back

    def __enter__(self):
        capi.set_tuning(self.key, self.value)

    def __exit__(self, *exc):
        capi.set_tuning(self.key, self.back)


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def colour_inputs(rng, seqs, k, n_colors):
    """Per colour a few sequences: pieces of the indexed sequences (so colours overlap), of their reverse complements, and
    pieces with a substitution, an N or a lower-case letter -- windows the index lacks or that are no k-mers."""
    out = []
    for _ in range(n_colors):
        mine = []
        for _ in range(rng.randint(1, 3)):
            s = rng.choice(seqs)
            a = rng.randrange(0, max(1, len(s) - k + 1))
            piece = list(s[a:a + rng.randint(k, k + 30)])
            if rng.random() < 0.3:
                piece[rng.randrange(len(piece))] = rng.choice("ACGTNacgt")
            piece = "".join(piece)
            mine.append(pb.revcomp(piece) if rng.random() < 0.3 else piece)
        if rng.random() < 0.2:
            mine.append(rand_seq(rng, k + 5))
        if rng.random() < 0.1:
            mine.append("")
        out.append(mine)
    if n_colors > 8:                                     # many colours: nine of them are given sequences, the last bit among them
        keep = set(rng.sample(range(n_colors), 7)) | {0, n_colors - 1}
        out = [mine if c in keep else [] for c, mine in enumerate(out)]
    return out


def colour_both(idx, kmers, k, inputs, strands):
    """The GPU's colours object and the brute force's colour sets of the same colouring; the window counts must agree."""
    n_colors = len(inputs)
    col = capi.Colors.create(idx, n_colors)
    cs = [set() for _ in range(n_colors)]
    for c, seqs in enumerate(inputs):
        if not seqs:
            continue
        got = col.add_reads(c, [s.encode() for s in seqs], strands == 2)
        assert got == pb.add(cs, kmers, k, c, seqs, strands), (c, seqs)
    return col, cs


def check_matrix(idx, col, cs, kmers, label):
    labels = labels_of(idx)
    want = np.array(pb.rows_of(labels, cs, kmers), dtype=np.uint64)
    got = col.rows()
    assert got.dtype == np.uint64 and got.shape == want.shape, label
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (label, int(bad[0]), labels[bad[0]], hex(int(got[bad[0]])), hex(int(want[bad[0]])))
    assert all(got[j] == 0 for j, lab in enumerate(labels) if "$" in lab), label
    info = col.info()
    assert info["n_columns"] == idx.n_nodes and info["k"] == idx.k and info["n_colors"] == len(cs), label
    assert info["n_colored_columns"] == int((want != 0).sum()), label
    assert info["per_color"] == [int(((want >> np.uint64(c)) & np.uint64(1)).sum()) for c in range(len(cs))], label


N_COLORS = (1, 2, 3, 63, 64)


def matrices_of_case(seqs, k, seed, shift):
    """Four indexes (with / without reverse complements x with / without suffix-group marks), each with all five colour
    counts; the strands alternate so that every (n_colors, strands) pair meets every kind of index over the cases."""
    rng = random.Random(seed)
    for j, (rc, ssup) in enumerate(((False, True), (False, False), (True, True), (True, False))):
        idx = make_index(seqs, k, rc, ssup)
        kmers = index_kmers(seqs, k, rc)
        for i, n_colors in enumerate(N_COLORS):
            strands = 1 + (i + j + shift) % 2
            col, cs = colour_both(idx, kmers, k, colour_inputs(rng, seqs, k, n_colors), strands)
            check_matrix(idx, col, cs, kmers, (k, rc, ssup, n_colors, strands))
            col.close()


# ---- 1. the colour matrix on every column -------------------------------------------------------------------
def test_matrix_on_reference_known_answer_inputs(gpu):
    cases = [KATS["cli_end_to_end"]] + KATS["small_cases"]["cases"] + [KATS["redundant_dummies"], KATS["api_example"]]
    for n, case in enumerate(cases):
        matrices_of_case(case["seqs"], case["k"], 100 + n, n)


@pytest.mark.parametrize("shift,k", list(enumerate([2, 5, 31, 32, 33, 64])))
def test_matrix_on_random_kmer_sets(gpu, shift, k):
    rng = random.Random(7 * k)
    seqs = [rand_seq(rng, rng.randint(k, 2 * k + 50)) for _ in range(rng.randint(2, 4))]
    matrices_of_case(seqs, k, k, shift)


# ---- a shared small pan-genome: three strains that differ by substitutions ----------------------------------------
K_PAN = 9


@pytest.fixture(scope="module")
def pan():
    rng = random.Random(5)
    base = rand_seq(rng, 400)
    strains = [base]
    for _ in range(2):
        s = list(base)
        for _ in range(12):
            s[rng.randrange(len(s))] = rng.choice("ACGT")
        strains.append("".join(s))
    extra = rand_seq(rng, 120)                           # indexed, given for no colour
    seqs = strains + [extra]
    idx = make_index(seqs, K_PAN, False)
    kmers = index_kmers(seqs, K_PAN, False)
    assert idx.n_nodes < 5000
    return {"strains": strains, "extra": extra, "seqs": seqs, "idx": idx, "kmers": kmers, "k": K_PAN}


def pan_colour_inputs(pan, n_colors):
    """colour c < 3: strain c; the colours above (64 colours) get pieces of the strains"""
    rng = random.Random(n_colors)
    inputs = [[pan["strains"][c % 3]] for c in range(min(n_colors, 3))]
    for c in range(3, n_colors):
        s = pan["strains"][c % 3]
        a = rng.randrange(0, 300)
        inputs.append([s[a:a + rng.randint(20, 100)]])
    return inputs


def probe_reads(seqs, k, rng):
    """Reads that exercise a small index: its sequences and pieces of them, their reverse complements, substitutions, N and
    lower case, reads shorter than k, of exactly k bases and empty."""
    reads = [b"", b"A", b"ACGT"[:k - 1], b"N" * (k + 2)]
    for s in seqs:
        reads += [s.encode(), pb.revcomp(s).encode(), s[:k].encode(), s[-k:].encode()]
        for _ in range(6):
            a = rng.randrange(0, len(s))
            piece = list(s[a:a + rng.randint(0, k + 40)])
            for _ in range(rng.randint(0, 3)):
                if piece:
                    piece[rng.randrange(len(piece))] = rng.choice("ACGTNacgt")
            piece = "".join(piece)
            reads += [piece.encode(), pb.revcomp(piece).encode()]
    reads.append(rand_seq(rng, 3 * k + 70).encode())
    return reads


def pan_reads(pan):
    rng = random.Random(11)
    k, strains = pan["k"], pan["strains"]
    reads = probe_reads(pan["seqs"], k, rng)
    for m in (63, 64, 65, 127, 128, 129):                 # exactly m windows: one wave iteration more or less
        for s in (strains[1], pan["extra"] + strains[2]):
            a = rng.randrange(0, len(s) - (m + k - 1) + 1)
            reads.append(s[a:a + m + k - 1].encode())
            assert len(reads[-1]) - k + 1 == m
        reads.append(pb.revcomp(strains[0][:m + k - 1]).encode())
    # at least 5 000 windows: strains, their reverse complements, noise and an N, with colours changing inside iterations
    long_read = (strains[0] + strains[1][:333] + rand_seq(rng, 700) + pb.revcomp(strains[2]) + pan["extra"] + "N" + strains[2] * 3 +
                 rand_seq(rng, 900) + strains[1] * 3 + strains[0][17:])
    assert len(long_read) - k + 1 >= 5000
    reads.insert(len(reads) // 2, long_read.encode())
    return reads


def as_tuples(rec):
    return [(int(r["colors"]), int(r["n_kmers"]), int(r["n_found"])) for r in rec]


# ---- 2. colouring details ---------------------------------------------------------------------------------
def test_colouring_details(gpu, pan):
    idx, kmers, k, strains = pan["idx"], pan["kmers"], pan["k"], pan["strains"]
    odd = [strains[0][:50] + "N" + strains[0][50:120], strains[1][:60].lower(), strains[1][60:90] + "acg" + strains[1][93:150],
           rand_seq(random.Random(1), 80), strains[2][:k - 1], "", pb.revcomp(strains[2][100:180])]
    for strands in (1, 2):
        # N, lower case and absent k-mers: the counts and the matrix are the brute force's
        col, cs = colour_both(idx, kmers, k, [odd, [strains[1]]], strands)
        assert 0 < pb.add([set(), set()], kmers, k, 0, odd, strands)[1] < pb.add([set(), set()], kmers, k, 0, odd, strands)[0]
        check_matrix(idx, col, cs, kmers, ("odd", strands))
        rows = col.rows()
        # adding twice changes nothing; the counts are those of the first time
        again = col.add_reads(0, [s.encode() for s in odd], strands == 2)
        assert again == pb.add([set(), set()], kmers, k, 0, odd, strands)
        assert np.array_equal(col.rows(), rows)
        # two calls equal one call, in either order
        with capi.Colors.create(idx, 2) as split:
            split.add_reads(1, [strains[1].encode()], strands == 2)
            split.add_reads(0, [s.encode() for s in odd[3:]], strands == 2)
            split.add_reads(0, [s.encode() for s in odd[:3]], strands == 2)
            assert np.array_equal(split.rows(), rows)
        # from_rows(rows()) reproduces the rows
        with capi.Colors.from_rows(idx, rows, 2) as copy:
            assert np.array_equal(copy.rows(), rows)
            assert copy.info() == col.info()
        col.close()
    # an upload with bits >= n_colors and with set dummy rows: both are cleared, the rest stays
    labels = labels_of(idx)
    dummy = np.array(["$" in lab for lab in labels])
    assert dummy.any() and not dummy.all()
    rng = np.random.default_rng(4)
    for n_colors in (1, 3, 63, 64):
        dirty = rng.integers(0, 2**64, size=idx.n_nodes, dtype=np.uint64)
        dirty[0] = np.uint64(2**64 - 1)
        keep = np.uint64(2**64 - 1) if n_colors == 64 else np.uint64((1 << n_colors) - 1)
        with capi.Colors.from_rows(idx, dirty, n_colors) as up:
            got = up.rows()
        assert np.array_equal(got, np.where(dummy, np.uint64(0), dirty & keep)), n_colors


# ---- 3. records and counts ---------------------------------------------------------------------------------
PPMS = (1, 500_000, 666_667, 1_000_000)


@pytest.mark.parametrize("n_colors", [1, 3, 64])
def test_records_and_counts(gpu, pan, n_colors):
    idx, kmers, k = pan["idx"], pan["kmers"], pan["k"]
    reads = pan_reads(pan)
    col, cs = colour_both(idx, kmers, k, pan_colour_inputs(pan, n_colors), 1)
    seen = set()
    for strands in (1, 2):
        sets = [pb.window_sets(cs, kmers, k, r, strands) for r in reads]
        want_counts = np.array([pb.counts_of(s, n_colors) for s in sets], dtype=np.int32).reshape(len(reads), n_colors)
        for ppm in PPMS:
            for den in (0, 1):
                want = [pb.record_of(s, n_colors, ppm, den) for s in sets]
                rec, cnt = col.pseudoalign_reads(reads, strands == 2, ppm, den, counts=True)
                got = as_tuples(rec)
                bad = [i for i in range(len(reads)) if got[i] != want[i]]
                assert not bad, (strands, ppm, den, reads[bad[0]][:80], got[bad[0]], want[bad[0]])
                assert cnt.dtype == np.int32 and np.array_equal(cnt, want_counts), (strands, ppm, den)
                assert as_tuples(col.pseudoalign_reads(reads, strands == 2, ppm, den)) == want          # without counts
                seen.update(w[0] for w in want)
    if n_colors >= 3:
        assert {0, 1, 2, 4, 7} <= {s & 7 for s in seen}       # none, single strains and all three occur
    col.close()


# ---- 4. invariance -----------------------------------------------------------------------------------------
def test_chunking_gives_the_same_records(gpu, pan):
    idx, kmers, k = pan["idx"], pan["kmers"], pan["k"]
    reads = pan_reads(pan)
    for strands in (1, 2):
        inputs = pan_colour_inputs(pan, 3)
        col, cs = colour_both(idx, kmers, k, inputs, strands)
        want, want_cnt = col.pseudoalign_reads(reads, strands == 2, 500_000, 1, counts=True)
        assert as_tuples(want) == pb.records(cs, kmers, k, reads, strands, 500_000, 1)
        for budget in (1, 700):                               # every read a chunk; a few reads per chunk
            with tuning("pseudoalign_chunk_bases", budget, 0):
                got, cnt = col.pseudoalign_reads(reads, strands == 2, 500_000, 1, counts=True)
                assert got.tobytes() == want.tobytes() and np.array_equal(cnt, want_cnt), (strands, budget)
                with capi.Colors.create(idx, 3) as chunked:  # colouring in chunks: the same matrix and the same counts
                    for c, seqs in enumerate(inputs):
                        many = seqs + [s[:40] for s in seqs] + ["", "ACG"]
                        assert chunked.add_reads(c, [s.encode() for s in many], strands == 2) == \
                            pb.add([set() for _ in range(3)], kmers, k, c, many, strands)
                    assert np.array_equal(chunked.rows(), col.rows())
        assert len(col.pseudoalign(np.zeros(0, np.uint8), np.zeros(1, np.int64))) == 0               # n_reads = 0
        assert as_tuples(col.pseudoalign_reads([b"", b"ACG", b""], strands == 2)) == [(0, 0, 0)] * 3  # no window at all
        col.close()


@pytest.mark.parametrize("knob", [("image_level", 1, 0), ("image_level", 2, 0), ("big_path", 2, 1)])
def test_layouts_and_image_levels(gpu, pan, knob):
    key, val, back = knob
    kmers, k = pan["kmers"], pan["k"]
    reads = pan_reads(pan)
    inputs = pan_colour_inputs(pan, 3)
    base_col, _ = colour_both(pan["idx"], kmers, k, inputs, 2)
    with tuning(key, val, back):
        idx = make_index(pan["seqs"], k, False)
        nomarks = make_index(pan["seqs"], k, False, False)
    if key == "image_level":
        assert idx.image_level >= val
    for other in (idx, nomarks):
        col, _ = colour_both(other, kmers, k, inputs, 2)
        assert np.array_equal(col.rows(), base_col.rows())
        for strands in (1, 2):
            a, ca = base_col.pseudoalign_reads(reads, strands == 2, 666_667, 0, counts=True)
            b, cb = col.pseudoalign_reads(reads, strands == 2, 666_667, 0, counts=True)
            assert a.tobytes() == b.tobytes() and np.array_equal(ca, cb), (knob, strands)
        col.close()
    base_col.close()


def test_device_entry_point(gpu, pan):
    import torch
    idx, kmers, k = pan["idx"], pan["kmers"], pan["k"]
    dev = torch.device("cuda", 0)
    reads = pan_reads(pan)
    bases, off = capi.concat_reads(reads)
    n = len(reads)
    lead = 37                                                        # d_read_off[0] != 0: bases nobody asks about in front
    shifted = np.concatenate([np.frombuffer(b"ACGTN" * 8, dtype=np.uint8)[:lead], bases])
    tb, to = torch.from_numpy(shifted).to(dev), torch.from_numpy(off + lead).to(dev)
    T = len(shifted)
    G = 5                                                            # guard words on either side
    PAT64, PAT32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
    for n_colors in (3, 64):
        col, cs = colour_both(idx, kmers, k, pan_colour_inputs(pan, n_colors), 1)
        for strands in (1, 2):
            want, want_cnt = col.pseudoalign(bases, off, strands == 2, 500_000, 0, counts=True)
            assert as_tuples(want) == pb.records(cs, kmers, k, reads, strands, 500_000, 0)
            need = capi.pseudoalign_workspace_bytes(T, n, strands == 2)
            assert need >= capi.search_workspace_bytes(T)
            ws = torch.zeros(need, dtype=torch.uint8, device=dev)
            rec = torch.full((2 * n + 2 * G,), PAT64, dtype=torch.int64, device=dev)
            cnt = torch.full((n * n_colors + 2 * G,), PAT32, dtype=torch.int32, device=dev)
            st = torch.cuda.Stream(dev)
            torch.cuda.synchronize(dev)
            for with_counts in (True, False):
                rec.fill_(PAT64)
                cnt.fill_(PAT32)
                torch.cuda.synchronize(dev)
                col.pseudoalign_dev(tb.data_ptr(), T, to.data_ptr(), n, rec.data_ptr() + 8 * G, cnt.data_ptr() + 4 * G if with_counts else 0,
                                    ws.data_ptr(), need, strands == 2, 500_000, 0, st.cuda_stream)
                torch.cuda.synchronize(dev)
                hr, hc = rec.cpu().numpy(), cnt.cpu().numpy()
                assert (hr[:G] == PAT64).all() and (hr[-G:] == PAT64).all()              # guards intact
                assert (hc[:G] == PAT32).all() and (hc[-G:] == PAT32).all()
                assert hr[G:-G].tobytes() == want.tobytes(), (n_colors, strands, with_counts)
                if with_counts:
                    assert np.array_equal(hc[G:-G].reshape(n, n_colors), want_cnt)
                else:
                    assert (hc == PAT32).all()
                assert idx.workspace_status(ws.data_ptr(), st.cuda_stream) == 0
            # a workspace one byte short is an error, and nothing is written
            rec.fill_(PAT64)
            with pytest.raises(capi.SbwtGpuError) as ei:
                col.pseudoalign_dev(tb.data_ptr(), T, to.data_ptr(), n, rec.data_ptr() + 8 * G, 0, ws.data_ptr(), need - 1, strands == 2,
                                    500_000, 0, st.cuda_stream)
            assert ei.value.code == capi.ERR_INVALID_ARG and "workspace" in ei.value.msg
            torch.cuda.synchronize(dev)
            assert (rec.cpu().numpy() == PAT64).all()
        col.close()


# ---- 5. workspace ------------------------------------------------------------------------------------------
def test_workspace_is_monotone():
    sizes = [0, 1, 31, 1000, 1 << 20, (1 << 25) + 1, 1 << 28, (1 << 30) + 5] + [int(1.9 ** e) for e in range(3, 34)]
    reads = [0, 1, 1023, 1024, 1025, 10**6, 10**7 + 3, 2**31 - 1]
    for both in (False, True):
        for nr in reads:
            prev = -1
            for b in sorted(sizes):
                w = capi.pseudoalign_workspace_bytes(b, nr, both)
                assert w >= prev and w >= capi.search_workspace_bytes(b) and w % 256 == 0, (b, nr, both)
                prev = w
        for b in sizes:
            prev = -1
            for nr in reads:
                w = capi.pseudoalign_workspace_bytes(b, nr, both)
                assert w >= prev, (b, nr, both)
                prev = w
    assert capi.pseudoalign_workspace_bytes(1000, 10, True) > capi.pseudoalign_workspace_bytes(1000, 10, False)


# ---- 6. refusals -------------------------------------------------------------------------------------------
def refused(fn, *needles):
    with pytest.raises(capi.SbwtGpuError) as ei:
        fn()
    assert ei.value.code == capi.ERR_INVALID_ARG, ei.value
    for s in needles:
        assert s in ei.value.msg, (s, ei.value.msg)


def test_refusals_leave_everything_usable(gpu, pan):
    idx, kmers, k = pan["idx"], pan["kmers"], pan["k"]
    reads = pan_reads(pan)[:40]
    col, cs = colour_both(idx, kmers, k, pan_colour_inputs(pan, 3), 1)
    want = pb.records(cs, kmers, k, reads)
    rows = col.rows()

    def still_fine():
        assert as_tuples(col.pseudoalign_reads(reads)) == want
        assert np.array_equal(col.rows(), rows)
        assert len(idx.search_reads([pan["strains"][0].encode()])[0]) == 400 - k + 1

    # rank-only indexes
    w = np.random.default_rng(1).integers(0, 2**64, size=4, dtype=np.uint64)
    ro = capi.Index.create(w, w, w, w, None, 256, 3)
    refused(lambda: capi.Colors.create(ro, 2), "only rank()")
    # n_colors outside 1 .. 64
    for nc in (0, 65, -1):
        refused(lambda: capi.Colors.create(idx, nc), "n_colors")
        refused(lambda: capi.Colors.from_rows(idx, rows, nc), "n_colors")
    still_fine()
    # color >= n_colors
    for c in (3, 64, -1):
        refused(lambda: col.add_reads(c, [b"ACGTACGTACGT"]), "color", "3 colours")
    still_fine()
    # threshold and denominator out of range, strands
    for ppm in (0, 1_000_001, -5):
        refused(lambda: col.pseudoalign_reads(reads, False, ppm, 0), "threshold_ppm")
    for den in (2, -1):
        refused(lambda: col.pseudoalign_reads(reads, False, 1_000_000, den), "denominator")
    bases, off = capi.concat_reads(reads)
    out = np.zeros(len(reads), dtype=capi.PSEUDOALIGNMENT_DTYPE)
    refused(lambda: capi._check(capi.lib().sbwtgpu_pseudoalign_batch(col.handle, bases.ctypes.data, off.ctypes.data, len(reads), 3,
                                                                     1_000_000, 0, out.ctypes.data, None)), "strands")
    still_fine()
    # a colours object (its rows) used with an index of another n_nodes or k
    other = make_index(pan["seqs"][:2], k, False)
    assert other.n_nodes != idx.n_nodes
    refused(lambda: capi.Colors.from_rows(other, rows, 3), "columns", "k =")
    refused(lambda: capi.Colors.from_rows(idx, rows, 3, k + 1), "columns", "k =")
    refused(lambda: capi.Colors.from_rows(idx, rows[:-1], 3), "columns")
    still_fine()
    col.close()


def test_index_of_2_pow_31_columns_is_refused(gpu):
    # (any bits make an index that answers rank(); the colour layer must refuse it for its size before anything else)
    n = 1 << 31
    w = np.zeros(n // 64, dtype=np.uint64)
    big = capi.Index.create(w, w, w, w, None, n, 31, 0, 0)
    refused(lambda: capi.Colors.create(big, 2), "2^31", "columns")
    big.close()


# ---- 7. two host threads -------------------------------------------------------------------------------------
def test_two_host_threads(gpu, pan):
    idx, kmers, k = pan["idx"], pan["kmers"], pan["k"]
    col, cs = colour_both(idx, kmers, k, pan_colour_inputs(pan, 64), 2)
    allr = pan_reads(pan)
    batches = [allr[: len(allr) // 2], allr[len(allr) // 2:]]
    want = [col.pseudoalign_reads(b, True, 500_000, 1, counts=True) for b in batches]
    out, errs = [None, None], []

    def work(t):
        try:
            out[t] = [col.pseudoalign_reads(batches[t], True, 500_000, 1, counts=True) for _ in range(3)]
        except Exception as e:        # noqa: BLE001 -- reported below
            errs.append(e)
    with tuning("pseudoalign_chunk_bases", 2000, 0):
        th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    assert not errs, errs
    for t in range(2):
        assert as_tuples(want[t][0]) == pb.records(cs, kmers, k, batches[t], 2, 500_000, 1)
        for rec, cnt in out[t]:
            assert rec.tobytes() == want[t][0].tobytes() and np.array_equal(cnt, want[t][1])
    col.close()


# ---- 8. the CLI ---------------------------------------------------------------------------------------------
def test_cli_build_colors_and_pseudoalign(gpu, tmp_path):
    kat = KATS["cli_end_to_end"]
    d = str(tmp_path)
    k = kat["k"]
    seqs = kat["seqs"]
    assert len(seqs) == 3
    with open(d + "/s.fna", "w") as fh:
        for i, s in enumerate(seqs):
            fh.write(">s%d\n%s\n" % (i, s))
    p = subprocess.run([SBWT, "build", "-i", d + "/s.fna", "-o", d + "/fwd.sbwt", "-k", str(k), "--temp-dir", d], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    # three reference files, one plain FASTA, one gzipped, one FASTQ; the second also holds a piece of the first
    refs = [[seqs[0]], [seqs[1], seqs[0][:k + 2]], [seqs[2]]]
    with open(d + "/ref0.fna", "w") as fh:
        fh.write(">a\n%s\n" % refs[0][0])
    with gzip.open(d + "/ref1.fna.gz", "wt") as fh:
        for j, s in enumerate(refs[1]):
            fh.write(">b%d\n%s\n" % (j, s))
    with open(d + "/ref2.fq", "w") as fh:
        fh.write("@c\n%s\n+\n%s\n" % (refs[2][0], "I" * len(refs[2][0])))
    with open(d + "/refs.txt", "w") as fh:
        fh.write("%s/ref0.fna\n%s/ref1.fna.gz\n%s/ref2.fq\n" % (d, d, d))
    kmers = kmer_set(seqs, k)
    rng = random.Random(81)
    # (the sequence reader upper-cases what it reads: the expected lines are those of the upper-cased reads)
    reads = [q.encode() for q in kat["queries"]] + [r.upper() for r in probe_reads(seqs, k, rng) if r]
    with open(d + "/r.fq", "w") as fh:
        for j, r in enumerate(reads):
            fh.write("@r%d\n%s\n+\n%s\n" % (j, r.decode(), "I" * len(r)))
    with open(d + "/r.fq", "rb") as src, gzip.open(d + "/r.fq.gz", "wb") as dst:
        dst.write(src.read())
    for both in (False, True):
        strands = 2 if both else 1
        cs = [set() for _ in range(3)]
        counts = [pb.add(cs, kmers, k, c, refs[c], strands) for c in range(3)]
        colors = "%s/idx%d.colors" % (d, both)
        p = subprocess.run([SBWT, "build-colors", "-i", d + "/fwd.sbwt", "-r", d + "/refs.txt", "-o", colors] +
                           (["--both-strands"] if both else []), capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode()
        rows, n_colors, kk = hostlib.colors_read(colors)
        assert (n_colors, kk) == (3, k)
        per_color = [int(((rows >> np.uint64(c)) & np.uint64(1)).sum()) for c in range(3)]
        assert per_color == [len(s) for s in cs]
        lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("colour ")]
        assert lines == ["colour %d: %d windows, %d hit windows, %d coloured columns" % (c, counts[c][0], counts[c][1], per_color[c])
                         for c in range(3)]
        for opts, ppm, den in (([], 1_000_000, 0), (["--threshold", "0.5", "--all-kmers"], 500_000, 1)):
            want = pb.format_lines(pb.records(cs, kmers, k, reads, strands, ppm, den))
            for q in ("r.fq", "r.fq.gz"):
                for z in (False, True):
                    out = "%s/%s.%d%d%d.out" % (d, q, z, both, den)
                    cmd = [SBWT, "pseudoalign", "-i", d + "/fwd.sbwt", "-c", colors, "-q", d + "/" + q, "-o", out] + opts
                    cmd += (["-z"] if z else []) + (["--both-strands"] if both else [])
                    p = subprocess.run(cmd, capture_output=True, timeout=300)
                    assert p.returncode == 0, p.stderr.decode()
                    text = gzip.open(out).read() if z else open(out, "rb").read()
                    assert text == want, (q, z, both, opts)
        assert any(len(ln.split()) > 1 for ln in want.decode().splitlines())
    # small batches give the same lines (the read numbers run on over the batches)
    p = subprocess.run([SBWT, "pseudoalign", "-i", d + "/fwd.sbwt", "-c", colors, "-q", d + "/r.fq", "-o", d + "/small.out",
                        "--threshold", "0.5", "--all-kmers", "--both-strands", "--batch-bases", "100"], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    assert open(d + "/small.out", "rb").read() == want
    # a refs.txt of 65 lines is refused, as are a threshold that is no fraction and colours of another index
    with open(d + "/refs65.txt", "w") as fh:
        fh.write(("%s/ref0.fna\n" % d) * 65)
    p = subprocess.run([SBWT, "build-colors", "-i", d + "/fwd.sbwt", "-r", d + "/refs65.txt", "-o", d + "/x.colors"], capture_output=True, timeout=60)
    assert p.returncode != 0 and b"65" in p.stderr and b"64" in p.stderr
    for bad in ("0", "1.0000001", "abc"):
        p = subprocess.run([SBWT, "pseudoalign", "-i", d + "/fwd.sbwt", "-c", colors, "-q", d + "/r.fq", "-o", d + "/x.out", "--threshold", bad],
                           capture_output=True, timeout=60)
        assert p.returncode != 0 and b"threshold" in p.stderr, bad
    hostlib.colors_write(d + "/other.colors", rows[:-1], 3, k)
    p = subprocess.run([SBWT, "pseudoalign", "-i", d + "/fwd.sbwt", "-c", d + "/other.colors", "-q", d + "/r.fq", "-o", d + "/x.out"],
                       capture_output=True, timeout=60)
    assert p.returncode != 0 and b"columns" in p.stderr
    p = subprocess.run([SBWT], capture_output=True, timeout=60)
    assert b"build-colors" in p.stderr and b"pseudoalign" in p.stderr


# ---- 9. a bounded seeded fuzz ----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz(gpu, seed):
    rng = random.Random(1000 + seed)
    for case in range(5):
        k = rng.randint(2, 64)
        rc, ssup = rng.random() < 0.5, rng.random() < 0.5
        n_colors = rng.choice([1, 2, 3, rng.randint(4, 62), 63, 64])
        strands_add, strands_q = rng.randint(1, 2), rng.randint(1, 2)
        ppm, den = rng.choice([1, rng.randint(1, 1_000_000), 500_000, 666_667, 1_000_000]), rng.randint(0, 1)
        seqs = [rand_seq(rng, rng.randint(k, 2 * k + 80)) for _ in range(rng.randint(1, 4))]
        label = (seed, case, k, rc, ssup, n_colors, strands_add, strands_q, ppm, den)
        idx = make_index(seqs, k, rc, ssup)
        kmers = index_kmers(seqs, k, rc)
        col, cs = colour_both(idx, kmers, k, colour_inputs(rng, seqs, k, n_colors), strands_add)
        check_matrix(idx, col, cs, kmers, label)
        reads = probe_reads(seqs, k, rng)
        rng.shuffle(reads)
        chunk = rng.choice([0, 1, 300])
        with tuning("pseudoalign_chunk_bases", chunk, 0):
            rec, cnt = col.pseudoalign_reads(reads, strands_q == 2, ppm, den, counts=True)
        want = pb.records(cs, kmers, k, reads, strands_q, ppm, den)
        got = as_tuples(rec)
        bad = [i for i in range(len(reads)) if got[i] != want[i]]
        assert not bad, (label, reads[bad[0]], got[bad[0]], want[bad[0]])
        assert np.array_equal(cnt, np.array(pb.counts(cs, kmers, k, reads, strands_q), dtype=np.int32).reshape(len(reads), n_colors)), label
        col.close()
        idx.close()


# ---- k > 64: one case through the host builder (the search routes there are tests/test_gpu_long_k.py's) --------------
def test_k_65(gpu):
    k = 65
    rng = random.Random(65)
    base = rand_seq(rng, 300)
    other = list(base)
    for _ in range(4):
        other[rng.randrange(300)] = rng.choice("ACGT")
    seqs = [base, "".join(other)]
    for rc in (False, True):
        idx = make_index(seqs, k, rc)
        kmers = index_kmers(seqs, k, rc)
        for strands in (1, 2):
            col, cs = colour_both(idx, kmers, k, [[seqs[0]], [seqs[1], pb.revcomp(seqs[0][:100])]], strands)
            check_matrix(idx, col, cs, kmers, (k, rc, strands))
            reads = probe_reads(seqs, k, rng)
            for den in (0, 1):
                rec, cnt = col.pseudoalign_reads(reads, strands == 2, 666_667, den, counts=True)
                assert as_tuples(rec) == pb.records(cs, kmers, k, reads, strands, 666_667, den), (rc, strands, den)
                assert np.array_equal(cnt, np.array(pb.counts(cs, kmers, k, reads, strands), dtype=np.int32).reshape(len(reads), 2))
            col.close()
