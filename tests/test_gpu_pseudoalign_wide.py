"""GPU: wide colour matrices (more than 64 colours: W words per column, sbwt_colors.hip's k_pa_reduce_wide) against the
definition-level brute force (tests/pseudoalign_brute.py, arranged for thousands of colours by tests/pseudoalign_wide.py):
every word of every column, the records, colour words and counts of probe reads with the traps a wide reduction can fall
into, agreement with the 64-colour API, invariance under chunking, the device entry point and image levels, every refusal,
the C++ CLI and a bounded seeded fuzz.  All comparisons are exact."""
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import pseudoalign_brute as pb
import pseudoalign_wide as pw
from bruteforce import kmer_set
from sbwt_amd import capi, hostlib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")
QUERIES = ((1_000_000, 0), (500_000, 1), (1, 0))


def make_index(seqs, k, rc=False, ssup=True):
    bits = hostlib.build_bits([s.encode() if isinstance(s, str) else s for s in seqs], k, rc, ssup)
    return capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)


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


class borrowed:
    """An object of the other Python class on the same handle, for the length of a with-block; its owner closes the handle."""

    def __init__(self, cls, owner):
        self.obj = cls(owner.handle, owner.index, owner.n_colors)

    def __enter__(self):
        return self.obj

    def __exit__(self, *exc):
        self.obj._h = None


def colour_both(idx, kmers, k, n_colors, inputs, strands, cls=None):
    """The GPU's colours object and the brute force's colour sets of the same colouring (inputs: colour -> sequences); the
    window counts of every add call must agree."""
    col = (cls or capi.WideColors).create(idx, n_colors)
    cs = [set() for _ in range(n_colors)]
    for c, seqs in sorted(inputs.items()):
        got = col.add_reads(c, [s.encode() for s in seqs], strands == 2)
        assert got == pb.add(cs, kmers, k, c, seqs, strands), (c, seqs)
    return col, cs


def check_matrix(idx, labels, col, cs, kmers, label):
    n_colors, words = len(cs), pw.n_words(len(cs))
    want_rows = pb.rows_of(labels, cs, kmers)
    want = pw.rows_array(want_rows, words)
    got = col.rows()
    assert got.dtype == np.uint64 and got.shape == (idx.n_nodes, words) == want.shape, label
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (label, bad[0].tolist(), labels[bad[0][0]], hex(int(got[tuple(bad[0])])), hex(int(want[tuple(bad[0])])))
    dummy = np.array(["$" in lab for lab in labels])
    assert dummy.any() and not got[dummy].any(), label
    info = col.info()
    assert (info["n_columns"], info["k"], info["n_colors"], info["words"]) == (idx.n_nodes, idx.k, n_colors, words), label
    assert info["n_colored_columns"] == sum(1 for r in want_rows if r), label
    per = [0] * n_colors
    for r in want_rows:
        while r:
            low = r & -r
            per[low.bit_length() - 1] += 1
            r ^= low
    assert info["per_color"] == per, label
    return want


class World:
    """One index of the shared pan-genome (tests/pseudoalign_wide.py's Case; its sequences do not depend on n_colors) and,
    made on demand and kept, the coloured matrix of every n_colors with the brute force's colour sets."""

    def __init__(self, rc):
        self.rc = rc
        self.case0 = pw.Case(1, rc)
        self.k = self.case0.k
        self.idx = make_index(self.case0.seqs, self.k, rc)
        assert 300 < self.idx.n_nodes < 4000
        self.kmers = self.case0.index_kmers()
        self.labels = labels_of(self.idx)
        self.made = {}

    def colours(self, n_colors):
        if n_colors not in self.made:
            case = pw.Case(n_colors, self.rc)
            assert case.seqs == self.case0.seqs
            col, cs = colour_both(self.idx, self.kmers, self.k, n_colors, case.inputs, case.strands_add)
            self.made[n_colors] = (case, col, cs, pw.Expected(cs, self.kmers, self.k))
        return self.made[n_colors]


@pytest.fixture(scope="module")
def worlds(gpu):
    made = {}

    def get(rc):
        if rc not in made:
            made[rc] = World(rc)
        return made[rc]
    yield get
    for w in made.values():
        for _, col, _, _ in w.made.values():
            col.close()


def as_lists(rec, colors):
    return [(pw.words_to_row(c), int(r["n_kmers"]), int(r["n_found"])) for r, c in zip(rec, colors.tolist())]


def check_query(col, exp, reads, sets, strands, ppm, den, label):
    """records, colour words and counts of the host call, with and without counts"""
    want = [exp.record_of(s, ppm, den) for s in sets]
    want_counts = np.array([exp.counts_of(s) for s in sets], dtype=np.int32).reshape(len(reads), exp.n_colors)
    rec, colors, cnt = col.pseudoalign_reads(reads, strands == 2, ppm, den, counts=True)
    assert rec.dtype == capi.READ_FOUND_DTYPE and colors.dtype == np.uint64 and colors.shape == (len(reads), col.words), label
    got = as_lists(rec, colors)
    bad = [i for i in range(len(reads)) if got[i] != want[i]]
    assert not bad, (label, reads[bad[0]][:80], got[bad[0]], want[bad[0]])
    assert cnt.dtype == np.int32 and cnt.shape == want_counts.shape and np.array_equal(cnt, want_counts), label
    rec2, colors2 = col.pseudoalign_reads(reads, strands == 2, ppm, den)
    assert rec2.tobytes() == rec.tobytes() and np.array_equal(colors2, colors), label
    return rec, colors, cnt


# ---- 1. the matrix ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
@pytest.mark.parametrize("n_colors", pw.N_COLORS)
def test_matrix_on_every_word_of_every_column(worlds, n_colors, rc):
    w = worlds(rc)
    case, col, cs, _ = w.colours(n_colors)              # (every add call's (n_windows, n_hit_windows) is checked in there)
    assert col.words == pw.n_words(n_colors) == case.words
    want = check_matrix(w.idx, w.labels, col, cs, w.kmers, (n_colors, rc))
    assert all((want[:, c >> 6] & np.uint64(1 << (c & 63))).any() for c in (0, 63, 64, n_colors - 1) if c < n_colors)
    # adding the same sequences twice changes nothing, and the counts are those of the first time
    for c in (0, n_colors - 1):
        again = col.add(c, *capi.concat_reads([s.encode() for s in case.inputs[c]]), case.strands_add == 2)
        assert again == pb.add([set() for _ in range(n_colors)], w.kmers, w.k, c, case.inputs[c], case.strands_add)
    assert np.array_equal(col.rows(), want)


# ---- 2. uploaded rows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_colors", pw.N_COLORS)
def test_uploaded_rows_are_cleaned(worlds, n_colors, tmp_path):
    w = worlds(n_colors % 2 == 1)
    idx, words = w.idx, pw.n_words(n_colors)
    dummy = np.array(["$" in lab for lab in w.labels])
    rng = np.random.default_rng(n_colors)
    dirty = rng.integers(0, 2**64, size=(idx.n_nodes, words), dtype=np.uint64)     # junk everywhere, dummy columns included
    dirty[0, :] = np.uint64(2**64 - 1)
    keep = np.full(words, 2**64 - 1, dtype=np.uint64)
    if n_colors % 64:
        keep[-1] = np.uint64((1 << (n_colors % 64)) - 1)
    want = np.where(dummy[:, None], np.uint64(0), dirty & keep[None, :])
    with capi.WideColors.from_rows(idx, dirty, n_colors) as up:
        got = up.rows()
        assert np.array_equal(got, want), n_colors
        info = up.info()
        assert info["n_colored_columns"] == int(want.any(axis=1).sum())
        assert info["per_color"] == [int(((want[:, c >> 6] >> np.uint64(c & 63)) & np.uint64(1)).sum()) for c in range(n_colors)]
    # a colour file -> from_rows gives the same matrix
    case, col, _, _ = w.colours(n_colors)
    path = str(tmp_path / "m.colors")
    hostlib.colors_write_wide(path, col.rows(), n_colors, idx.k)
    rows, nc, k = hostlib.colors_read_wide(path)
    assert (nc, k) == (n_colors, idx.k)
    with capi.WideColors.from_rows(idx, rows, nc, k) as back:
        assert np.array_equal(back.rows(), col.rows()) and back.info() == col.info()


# ---- the device entry point, with guards and sentinels ------------------------------------------------------------
PAT64, PAT32, GUARD = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A, 5


def run_dev(col, reads, strands, ppm, den, with_counts, short_by=0):
    """sbwtgpu_pseudoalign_wide_dev on buffers filled with a pattern, guard words either side: (records, colour words, the
    whole counts buffer, workspace status)."""
    import torch
    dev = torch.device("cuda", 0)
    bases, off = capi.concat_reads(reads)
    n, words, nc = len(reads), col.words, col.n_colors
    lead = 37                                                        # d_read_off[0] != 0: bases nobody asks about in front
    shifted = np.concatenate([np.frombuffer(b"ACGTN" * 8, dtype=np.uint8)[:lead], bases])
    tb, to = torch.from_numpy(shifted).to(dev), torch.from_numpy(off + lead).to(dev)
    T = len(shifted)
    need = capi.pseudoalign_workspace_bytes(T, n, strands == 2)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    rec = torch.full((n + 2 * GUARD,), PAT64, dtype=torch.int64, device=dev)
    colw = torch.full((n * words + 2 * GUARD,), PAT64, dtype=torch.int64, device=dev)
    cnt = torch.full((n * nc + 2 * GUARD,), PAT32, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    try:
        col.pseudoalign_dev(tb.data_ptr(), T, to.data_ptr(), n, rec.data_ptr() + 8 * GUARD, colw.data_ptr() + 8 * GUARD,
                            cnt.data_ptr() + 4 * GUARD if with_counts else 0, ws.data_ptr(), need - short_by, strands == 2, ppm, den,
                            st.cuda_stream)
    finally:
        torch.cuda.synchronize(dev)
    status = col.index.workspace_status(ws.data_ptr(), st.cuda_stream)
    hr, hw, hc = rec.cpu().numpy(), colw.cpu().numpy(), cnt.cpu().numpy()
    for h, pat in ((hr, PAT64), (hw, PAT64), (hc, PAT32)):
        assert (h[:GUARD] == pat).all() and (h[-GUARD:] == pat).all()                # guards intact
    return (hr[GUARD:-GUARD].view(capi.READ_FOUND_DTYPE), hw[GUARD:-GUARD].view(np.uint64).reshape(n, words), hc, status)


# ---- 3. records, colour words and counts ----------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
@pytest.mark.parametrize("n_colors", pw.N_COLORS)
def test_records_words_and_counts(worlds, n_colors, rc):
    w = worlds(rc)
    case, col, cs, exp = w.colours(n_colors)
    reads = case.reads()
    last = n_colors - 1
    for strands in (1, 2):
        sets = [exp.window_sets(r, strands) for r in reads]
        for ppm, den in QUERIES:
            rec, colors, cnt = check_query(col, exp, reads, sets, strands, ppm, den, (n_colors, rc, strands, ppm, den))
        # counts off on the device entry point: the counts buffer keeps its sentinel, records and words are the same
        drec, dcol, dcnt, status = run_dev(col, reads, strands, ppm, den, False)
        assert status == 0 and drec.tobytes() == rec.tobytes() and np.array_equal(dcol, colors)
        assert (dcnt == PAT32).all()
        if case.words > 1:                                   # what the traps are there for, spelt out
            got = dict(zip(reads, as_lists(*col.pseudoalign_reads(reads, strands == 2, 1_000_000, 0))))
            t = case.trap_last_word_only()
            assert got[t] == (1 << last, len(t) - w.k + 1, len(t) - w.k + 1)
            t = case.trap_equal_word0()
            assert got[t][0] == 1 and got[t][2] == 2 * (30 - w.k + 1)         # colour 0 on every found window, the last on half
            if rc:
                t = case.trap_two_strands()
                assert got[t][0] == (1 | (1 << last) if strands == 2 else 1)


# ---- 4. agreement with the 64-colour API --------------------------------------------------------------------------
@pytest.mark.parametrize("n_colors", [3, 64])
def test_agreement_with_the_64_colour_api(worlds, n_colors):
    for rc in (False, True):
        w = worlds(rc)
        case = pw.Case(n_colors, rc)
        reads = case.reads()
        wide, cs = colour_both(w.idx, w.kmers, w.k, n_colors, case.inputs, case.strands_add)
        old, cs2 = colour_both(w.idx, w.kmers, w.k, n_colors, case.inputs, case.strands_add, capi.Colors)
        assert cs == cs2 and wide.words == 1
        assert wide.rows().shape == (w.idx.n_nodes, 1) and np.array_equal(wide.rows()[:, 0], old.rows())
        oi, wi = old.info(), wide.info()
        assert all(oi[key] == wi[key] for key in oi)
        # either object through either set of calls: one object type serves both
        with borrowed(capi.WideColors, old) as old_as_wide, borrowed(capi.Colors, wide) as wide_as_old:
            for strands in (1, 2):
                for ppm, den in QUERIES:
                    a, ca = old.pseudoalign_reads(reads, strands == 2, ppm, den, counts=True)
                    if ppm == 500_000:
                        assert [(int(x["colors"]), int(x["n_kmers"]), int(x["n_found"])) for x in a] == \
                            pb.records(cs, w.kmers, w.k, reads, strands, ppm, den)
                    for obj in (wide, old_as_wide):
                        rec, colors, cnt = obj.pseudoalign_reads(reads, strands == 2, ppm, den, counts=True)
                        assert np.array_equal(rec["n_kmers"], a["n_kmers"]) and np.array_equal(rec["n_found"], a["n_found"])
                        assert np.array_equal(colors[:, 0], a["colors"]) and np.array_equal(cnt, ca), (n_colors, rc, strands, ppm, den)
                    b, cb = wide_as_old.pseudoalign_reads(reads, strands == 2, ppm, den, counts=True)
                    assert b.tobytes() == a.tobytes() and np.array_equal(cb, ca)
        wide.close()
        old.close()


# ---- 5. invariance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_colors", [65, 200, 4096])
def test_chunking_and_the_device_entry_point(worlds, n_colors):
    w = worlds(n_colors != 200)
    case, col, cs, exp = w.colours(n_colors)
    reads = case.reads()
    total = sum(len(r) for r in reads)
    for strands in (1, 2):
        want = col.pseudoalign_reads(reads, strands == 2, 500_000, 1, counts=True)
        for budget in (1, total // 4):                        # every read a chunk; at least three chunks
            with tuning("pseudoalign_chunk_bases", budget, 0):
                got = col.pseudoalign_reads(reads, strands == 2, 500_000, 1, counts=True)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), (strands, budget)
                with capi.WideColors.create(w.idx, n_colors) as chunked:     # colouring in chunks: the same matrix
                    for c, seqs in sorted(case.inputs.items()):
                        chunked.add_reads(c, [s.encode() for s in seqs], case.strands_add == 2)
                    assert np.array_equal(chunked.rows(), col.rows())
        drec, dcol, dcnt, status = run_dev(col, reads, strands, 500_000, 1, True)
        assert status == 0 and drec.tobytes() == want[0].tobytes() and np.array_equal(dcol, want[1])
        assert np.array_equal(dcnt[GUARD:-GUARD].reshape(len(reads), n_colors), want[2])
        # a workspace one byte short is an error, and nothing is written
        with pytest.raises(capi.SbwtGpuError) as ei:
            run_dev(col, reads, strands, 500_000, 1, True, short_by=1)
        assert ei.value.code == capi.ERR_INVALID_ARG and "workspace" in ei.value.msg
        assert len(col.pseudoalign(np.zeros(0, np.uint8), np.zeros(1, np.int64))[0]) == 0               # n_reads = 0
        rec, colors = col.pseudoalign_reads([b"", b"ACG", b""], strands == 2)                            # no window at all
        assert as_lists(rec, colors) == [(0, 0, 0)] * 3
    assert capi.pseudoalign_workspace_bytes(total, len(reads), True) > capi.pseudoalign_workspace_bytes(total, len(reads), False)


def test_a_lower_image_level(worlds):
    w = worlds(True)
    n_colors = 129
    case, col, cs, exp = w.colours(n_colors)
    reads = case.reads()
    with tuning("image_level", 1, 0):
        idx = make_index(case.seqs, w.k, True)
        nomarks = make_index(case.seqs, w.k, True, False)
    assert idx.image_level >= 1
    for other in (idx, nomarks):
        c2, _ = colour_both(other, w.kmers, w.k, n_colors, case.inputs, case.strands_add)
        assert np.array_equal(c2.rows(), col.rows())
        for strands in (1, 2):
            a = col.pseudoalign_reads(reads, strands == 2, 500_000, 0, counts=True)
            b = c2.pseudoalign_reads(reads, strands == 2, 500_000, 0, counts=True)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), strands
        c2.close()
        other.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------
def refused(fn, *needles):
    with pytest.raises(capi.SbwtGpuError) as ei:
        fn()
    assert ei.value.code == capi.ERR_INVALID_ARG, ei.value
    for s in needles:
        assert s in ei.value.msg, (s, ei.value.msg)


def test_refusals_leave_everything_usable(worlds):
    w = worlds(False)
    idx, k = w.idx, w.k
    case, col, cs, exp = w.colours(65)
    reads = case.reads()[:30]
    want = [exp.record_of(exp.window_sets(r), 1_000_000, 0) for r in reads]
    rows = col.rows()

    def still_fine():
        assert as_lists(*col.pseudoalign_reads(reads)) == want
        assert np.array_equal(col.rows(), rows)
        assert len(idx.search_reads([case.strains[0].encode()])[0]) == 400 - k + 1

    # n_colors outside 1 .. 4096
    for nc in (0, 4097, -1):
        refused(lambda: capi.WideColors.create(idx, nc), "n_colors", "4096")
        refused(lambda: capi.WideColors.from_rows(idx, rows, nc), "n_colors", "4096")
    still_fine()
    # color >= n_colors
    for c in (65, 128, 4096, -1):
        refused(lambda: col.add_reads(c, [b"ACGTACGTACGTACGT"]), "color", "65 colours")
    still_fine()
    # the 64-colour calls on an object of 65 colours: refused, and the message names the wide call
    with borrowed(capi.Colors, col) as narrow:
        refused(lambda: narrow.pseudoalign_reads(reads), "65", "sbwtgpu_pseudoalign_wide_batch")
        refused(lambda: narrow.info(), "65", "sbwtgpu_colors_info_wide")
        refused(lambda: narrow.pseudoalign_dev(0, 0, 0, 1, 0, 0, 0, 0), "65", "sbwtgpu_pseudoalign_wide_dev")
        assert narrow.rows_dev() != 0                            # (what does not depend on the width still works)
    # ... and the 64-colour create still stops at 64, now pointing at the wide one
    refused(lambda: capi.Colors.create(idx, 65), "n_colors", "64", "sbwtgpu_colors_create_wide")
    still_fine()
    # rows of the wrong shape, of another index, of another k
    refused(lambda: capi.WideColors.from_rows(idx, rows[:, 0], 65), "shape")
    refused(lambda: capi.WideColors.from_rows(idx, rows[:, :1], 65), "shape")
    refused(lambda: capi.WideColors.from_rows(idx, np.zeros((idx.n_nodes, 3), np.uint64), 65), "shape")
    refused(lambda: capi.WideColors.from_rows(idx, rows[:-1], 65), "columns")
    refused(lambda: capi.WideColors.from_rows(idx, rows, 65, k + 1), "columns", "k =")
    other = make_index(case.seqs[:2], k, False)
    assert other.n_nodes != idx.n_nodes
    refused(lambda: capi.WideColors.from_rows(other, rows, 65), "columns")
    other.close()
    still_fine()
    # rank-only indexes; strands = 3; threshold and denominator out of range
    bits = np.random.default_rng(1).integers(0, 2**64, size=4, dtype=np.uint64)
    ro = capi.Index.create(bits, bits, bits, bits, None, 256, 3)
    refused(lambda: capi.WideColors.create(ro, 100), "only rank()")
    bases, off = capi.concat_reads(reads)
    out = np.zeros(len(reads), dtype=capi.READ_FOUND_DTYPE)
    colw = np.zeros((len(reads), 2), dtype=np.uint64)
    refused(lambda: capi._check(capi.lib().sbwtgpu_pseudoalign_wide_batch(col.handle, bases.ctypes.data, off.ctypes.data, len(reads), 3,
                                                                          1_000_000, 0, out.ctypes.data, colw.ctypes.data, None)), "strands")
    nw, nh = capi.C.c_int64(0), capi.C.c_int64(0)
    refused(lambda: capi._check(capi.lib().sbwtgpu_colors_add_batch(col.handle, 0, bases.ctypes.data, off.ctypes.data, len(reads), 3,
                                                                    capi.C.byref(nw), capi.C.byref(nh))), "strands")
    for ppm in (0, 1_000_001):
        refused(lambda: col.pseudoalign_reads(reads, False, ppm, 0), "threshold_ppm")
    refused(lambda: col.pseudoalign_reads(reads, False, 1_000_000, 2), "denominator")
    still_fine()
    # NULL pointers at the C calls themselves: the object, the records, the colour words (host and device entry points)
    import torch
    L, n = capi.lib(), len(reads)
    dev = torch.device("cuda", 0)
    d_rec = torch.zeros(n, dtype=torch.int64, device=dev)
    d_col = torch.zeros(n * 2, dtype=torch.int64, device=dev)
    d_bases, d_off = torch.from_numpy(bases.copy()).to(dev), torch.from_numpy(off.copy()).to(dev)
    need = capi.pseudoalign_workspace_bytes(len(bases), n, False)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    host = (bases.ctypes.data, off.ctypes.data, n, 1, 1_000_000, 0)
    refused(lambda: capi._check(L.sbwtgpu_pseudoalign_wide_batch(None, *host, out.ctypes.data, colw.ctypes.data, None)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_pseudoalign_wide_batch(col.handle, *host, None, colw.ctypes.data, None)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_pseudoalign_wide_batch(col.handle, *host, out.ctypes.data, None, None)), "NULL")
    device = (d_bases.data_ptr(), len(bases), d_off.data_ptr(), n, 1, 1_000_000, 0)
    tail = (None, ws.data_ptr(), need, None)
    refused(lambda: capi._check(L.sbwtgpu_pseudoalign_wide_dev(None, *device, d_rec.data_ptr(), d_col.data_ptr(), *tail)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_pseudoalign_wide_dev(col.handle, *device, None, d_col.data_ptr(), *tail)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_pseudoalign_wide_dev(col.handle, *device, d_rec.data_ptr(), None, *tail)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_pseudoalign_wide_dev(col.handle, d_bases.data_ptr(), len(bases), None, n, 1, 1_000_000, 0,
                                                               d_rec.data_ptr(), d_col.data_ptr(), *tail)), "NULL")
    torch.cuda.synchronize(dev)
    assert not d_rec.any().item() and not d_col.any().item()          # and nothing was written
    refused(lambda: capi._check(L.sbwtgpu_colors_create_wide(idx.handle, 65, None, None)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_colors_create_wide(None, 65, None, capi.C.byref(capi.C.c_void_p()))), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_colors_info_wide(None, None, None, None, None, None)), "NULL")
    assert L.sbwtgpu_colors_words(None) == 0
    # the same device call with every pointer in place is the host call's answer
    capi._check(L.sbwtgpu_pseudoalign_wide_dev(col.handle, *device, d_rec.data_ptr(), d_col.data_ptr(), *tail))
    torch.cuda.synchronize(dev)
    assert as_lists(d_rec.cpu().numpy().view(capi.READ_FOUND_DTYPE), d_col.cpu().numpy().view(np.uint64).reshape(n, 2)) == want
    still_fine()


# ---- 7. the CLI ---------------------------------------------------------------------------------------------------
def run(cmd, timeout=300):
    return subprocess.run(cmd, capture_output=True, timeout=timeout)


def test_cli_wide(gpu, tmp_path):
    d = str(tmp_path)
    case = pw.Case(70, False)
    k, seqs = case.k, case.seqs
    with open(d + "/s.fna", "w") as fh:
        for i, s in enumerate(seqs):
            fh.write(">s%d\n%s\n" % (i, s))
    p = run([SBWT, "build", "-i", d + "/s.fna", "-o", d + "/fwd.sbwt", "-k", str(k), "--temp-dir", d])
    assert p.returncode == 0, p.stderr.decode()
    # 70 reference files: the traps' colours 0, 68 and 69 as in the case, every other file a piece of a strain
    rng = random.Random(70)
    refs = []
    for c in range(70):
        if c in (0, 63, 64, 68, 69):
            refs.append([s for s in case.inputs[c] if s])
        else:
            s = case.strains[c % 3]
            a = rng.randrange(0, 300)
            refs.append([s[a:a + rng.randint(20, 100)]])
    with open(d + "/refs.txt", "w") as fh:
        for c, mine in enumerate(refs):
            name = "%s/ref%d.fna" % (d, c)
            with open(name, "w") as out:
                for j, s in enumerate(mine):
                    out.write(">r%d_%d\n%s\n" % (c, j, s))
            fh.write(name + "\n")
    kmers = kmer_set(seqs, k)
    # (the sequence reader upper-cases what it reads: the expected lines are those of the upper-cased reads)
    reads = [r.upper() for r in case.reads() if r]
    with open(d + "/r.fq", "w") as fh:
        for j, r in enumerate(reads):
            fh.write("@r%d\n%s\n+\n%s\n" % (j, r.decode(), "I" * len(r)))
    for both in (False, True):
        strands = 2 if both else 1
        cs = [set() for _ in range(70)]
        counts = [pb.add(cs, kmers, k, c, refs[c], strands) for c in range(70)]
        exp = pw.Expected(cs, kmers, k)
        colors = "%s/wide%d.colors" % (d, both)
        p = run([SBWT, "build-colors", "--wide", "-i", d + "/fwd.sbwt", "-r", d + "/refs.txt", "-o", colors] + (["--both-strands"] if both else []))
        assert p.returncode == 0, p.stderr.decode()
        assert open(colors, "rb").read(8) == b"SBWTCOL2"
        rows, n_colors, kk = hostlib.colors_read_wide(colors)
        assert (n_colors, kk, rows.shape[1]) == (70, k, 2)
        per_color = [int(((rows[:, c >> 6] >> np.uint64(c & 63)) & np.uint64(1)).sum()) for c in range(70)]
        assert per_color == [len(s) for s in cs]
        lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("colour ")]
        assert lines == ["colour %d: %d windows, %d hit windows, %d coloured columns" % (c, counts[c][0], counts[c][1], per_color[c])
                         for c in range(70)]
        for opts, ppm, den in (([], 1_000_000, 0), (["--threshold", "0.5", "--all-kmers"], 500_000, 1)):
            want = pw.format_lines(exp.record_of(exp.window_sets(r, strands), ppm, den)[0] for r in reads)
            for z in (False, True):
                out = "%s/w.%d%d%d.out" % (d, z, both, den)
                p = run([SBWT, "pseudoalign", "-i", d + "/fwd.sbwt", "-c", colors, "-q", d + "/r.fq", "-o", out] + opts +
                        (["-z"] if z else []) + (["--both-strands"] if both else []))
                assert p.returncode == 0, p.stderr.decode()
                text = gzip.open(out).read() if z else open(out, "rb").read()
                assert text == want, (z, both, opts)
        assert any(int(c) >= 64 for ln in want.decode().splitlines() for c in ln.split()[1:])
        assert any(len(ln.split()) > 2 for ln in want.decode().splitlines())
    # small batches give the same lines
    p = run([SBWT, "pseudoalign", "-i", d + "/fwd.sbwt", "-c", colors, "-q", d + "/r.fq", "-o", d + "/small.out", "--threshold", "0.5",
             "--all-kmers", "--both-strands", "--batch-bases", "100"])
    assert p.returncode == 0, p.stderr.decode()
    assert open(d + "/small.out", "rb").read() == want
    # --wide with three references writes the wide magic too; without the flag the file and the lines are what they were, and
    # both files give the same bytes
    with open(d + "/refs3.txt", "w") as fh:
        fh.write("".join("%s/ref%d.fna\n" % (d, c) for c in (0, 63, 64)))
    cs3 = [set() for _ in range(3)]
    for i, c in enumerate((0, 63, 64)):
        pb.add(cs3, kmers, k, i, refs[c], 1)
    want3 = pb.format_lines(pb.records(cs3, kmers, k, reads, 1, 1_000_000, 0))
    for flag, magic in (([], b"SBWTCOL1"), (["--wide"], b"SBWTCOL2")):
        name = d + "/three%d.colors" % len(flag)
        p = run([SBWT, "build-colors", "-i", d + "/fwd.sbwt", "-r", d + "/refs3.txt", "-o", name] + flag)
        assert p.returncode == 0, p.stderr.decode()
        assert open(name, "rb").read(8) == magic
        p = run([SBWT, "pseudoalign", "-i", d + "/fwd.sbwt", "-c", name, "-q", d + "/r.fq", "-o", d + "/three.out"])
        assert p.returncode == 0, p.stderr.decode()
        assert open(d + "/three.out", "rb").read() == want3, flag
    assert np.array_equal(hostlib.colors_read(d + "/three0.colors")[0], hostlib.colors_read_wide(d + "/three1.colors")[0][:, 0])
    # 70 lines without --wide: refused as before, and the message points at the flag; 4097 lines with it: refused
    p = run([SBWT, "build-colors", "-i", d + "/fwd.sbwt", "-r", d + "/refs.txt", "-o", d + "/x.colors"], 60)
    assert p.returncode != 0 and b"70" in p.stderr and b"64" in p.stderr and b"--wide" in p.stderr
    with open(d + "/refs4097.txt", "w") as fh:
        fh.write(("%s/ref0.fna\n" % d) * 4097)
    p = run([SBWT, "build-colors", "--wide", "-i", d + "/fwd.sbwt", "-r", d + "/refs4097.txt", "-o", d + "/x.colors"], 60)
    assert p.returncode != 0 and b"4097" in p.stderr and b"4096" in p.stderr
    # a wide colour file of another index is refused
    hostlib.colors_write_wide(d + "/other.colors", rows[:-1], 70, k)
    p = run([SBWT, "pseudoalign", "-i", d + "/fwd.sbwt", "-c", d + "/other.colors", "-q", d + "/r.fq", "-o", d + "/x.out"], 60)
    assert p.returncode != 0 and b"columns" in p.stderr


# ---- 8. a bounded seeded fuzz ---------------------------------------------------------------------------------------
def fuzz_inputs(rng, seqs, k, n_colors):
    """At most eight colours, 0, 63, 64 and the last among them where they exist: pieces of the indexed sequences, of their
    reverse complements, pieces with a substitution, an N or a lower-case letter."""
    chosen = {c for c in (0, 63, 64, n_colors - 1) if c < n_colors} | set(rng.sample(range(n_colors), min(4, n_colors)))
    inputs = {}
    for c in sorted(chosen):
        mine = []
        for _ in range(rng.randint(1, 3)):
            s = rng.choice(seqs)
            a = rng.randrange(0, max(1, len(s) - k + 1))
            piece = list(s[a:a + rng.randint(k, k + 30)])
            if rng.random() < 0.3:
                piece[rng.randrange(len(piece))] = rng.choice("ACGTNacgt")
            piece = "".join(piece)
            mine.append(pb.revcomp(piece) if rng.random() < 0.3 else piece)
        inputs[c] = mine
    return inputs


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz(gpu, seed):
    rng = random.Random(4000 + seed)
    for case in range(4):
        k = rng.randint(2, 40)
        rc, ssup = rng.random() < 0.5, rng.random() < 0.5
        n_colors = rng.choice(pw.N_COLORS)
        strands_add, strands_q = rng.randint(1, 2), rng.randint(1, 2)
        ppm, den = rng.choice([1, rng.randint(1, 1_000_000), 500_000, 1_000_000]), rng.randint(0, 1)
        seqs = [pw.rand_seq(rng, rng.randint(k, 2 * k + 80)) for _ in range(rng.randint(1, 4))]
        label = (seed, case, k, rc, ssup, n_colors, strands_add, strands_q, ppm, den)
        idx = make_index(seqs, k, rc, ssup)
        kmers = kmer_set(list(seqs) + ([pb.revcomp(s) for s in seqs] if rc else []), k)
        col, cs = colour_both(idx, kmers, k, n_colors, fuzz_inputs(rng, seqs, k, n_colors), strands_add)
        check_matrix_any(idx, col, cs, kmers, label)
        exp = pw.Expected(cs, kmers, k)
        reads = [b"", b"A" * (k - 1)]
        for s in seqs:
            reads += [s.encode(), pb.revcomp(s).encode(), s[:k].encode()]
            for _ in range(4):
                a = rng.randrange(0, len(s))
                piece = list(s[a:a + rng.randint(0, k + 70)])
                for _ in range(rng.randint(0, 2)):
                    if piece:
                        piece[rng.randrange(len(piece))] = rng.choice("ACGTNacgt")
                reads.append("".join(piece).encode())
        reads.append("".join(seqs).encode() * 2)
        rng.shuffle(reads)
        with tuning("pseudoalign_chunk_bases", rng.choice([0, 1, 300]), 0):
            check_query(col, exp, reads, [exp.window_sets(r, strands_q) for r in reads], strands_q, ppm, den, label)
        col.close()
        idx.close()


def check_matrix_any(idx, col, cs, kmers, label):
    """check_matrix for an index that may have no dummy column to look at"""
    labels = labels_of(idx)
    want = pw.rows_array(pb.rows_of(labels, cs, kmers), pw.n_words(len(cs)))
    got = col.rows()
    assert got.shape == want.shape and np.array_equal(got, want), label
    info = col.info()
    assert info["n_colored_columns"] == int(want.any(axis=1).sum()), label
    assert info["per_color"] == [int(((want[:, c >> 6] >> np.uint64(c & 63)) & np.uint64(1)).sum()) for c in range(len(cs))], label
