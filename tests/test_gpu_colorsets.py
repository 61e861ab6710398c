"""GPU: deduplicated colour sets (one id per column and a table of the distinct rows: sbwt_colorsets.hip) against the
definition (tests/colorsets_brute.py), the wide calls on the matrix an object means, and the brute force of
tests/pseudoalign_brute.py as tests/pseudoalign_wide.py arranges it: compress gives the canonical form byte for byte,
create takes any object that keeps the invariants and names what breaks them, the queries return the wide calls' records,
colour words and counts -- on the shared pan-genome, on uploaded tables that steer k_pa_reduce_sets into its corners, under
chunking, through the device entry point, from two threads, through the C++ CLI and in a bounded seeded fuzz.  All
comparisons are exact."""
import gzip
import random
import threading

import numpy as np
import pytest

import colorsets_brute as cb
import pseudoalign_brute as pb
import pseudoalign_wide as pw
import test_gpu_pseudoalign_wide as tw          # its helpers: the shared worlds, check_query, run_dev, the fuzz's colour inputs
from bruteforce import kmer_set
from sbwt_amd import capi, hostlib

pytestmark = pytest.mark.gpu

QUERIES = tw.QUERIES
N_COLORS = (1, 64, 65, 200, 4096)


@pytest.fixture(scope="module")
def worlds(gpu):
    """tw.World per strand mode (index, brute-force colour sets and wide matrix of every n_colors), made on demand"""
    made = {}

    def get(rc):
        if rc not in made:
            made[rc] = tw.World(rc)
        return made[rc]
    yield get
    for w in made.values():
        for _, col, _, _ in w.made.values():
            col.close()


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def check_against_wide(sets, wide, reads, label, queries=QUERIES):
    """every query of the colour-set object gives the bytes of the wide call on the matrix it means"""
    for strands in (1, 2):
        for ppm, den in queries:
            got = sets.pseudoalign_reads(reads, strands == 2, ppm, den, counts=True)
            want = wide.pseudoalign_reads(reads, strands == 2, ppm, den, counts=True)
            assert same(got, want), (label, strands, ppm, den)
            assert same(sets.pseudoalign_reads(reads, strands == 2, ppm, den), want[:2]), (label, strands, ppm, den)


# ---- 1. compress ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
@pytest.mark.parametrize("n_colors", N_COLORS)
def test_compress_gives_the_canonical_form(worlds, n_colors, rc):
    w = worlds(rc)
    case, col, cs, _ = w.colours(n_colors)
    matrix = col.rows()
    want_ids, want_table = cb.canonical_arrays(matrix)
    with capi.ColorSets.from_colors(col) as s, capi.ColorSets.from_colors(col) as again:
        ids, table = s.copy()
        assert ids.dtype == np.uint32 and table.dtype == np.uint64
        assert ids.shape == want_ids.shape and table.shape == want_table.shape == (s.n_sets, pw.n_words(n_colors))
        assert np.array_equal(ids, want_ids) and np.array_equal(table, want_table)
        assert 2 <= s.n_sets == 1 + len(set(pw.rows_ints(matrix)) - {0})
        ids2, table2 = again.copy()                                  # compressing twice gives equal bytes
        assert ids2.tobytes() == ids.tobytes() and table2.tobytes() == table.tobytes()
        dummy = ["$" in lab for lab in w.labels]
        cb.check_invariants(ids.tolist(), pw.rows_ints(table), n_colors, dummy)
        info = s.info()
        assert info == {"n_columns": w.idx.n_nodes, "k": w.k, "n_colors": n_colors, "words": pw.n_words(n_colors), "n_sets": len(want_table),
                        "n_colored_columns": int(matrix.any(axis=1).sum()), "device_bytes": 4 * w.idx.n_nodes + 8 * want_table.size}
        assert s.dev_ptrs()[0] != 0 and s.dev_ptrs()[1] != 0
        with s.expand() as back:                                     # every word of every column
            assert back.words == col.words and np.array_equal(back.rows(), matrix)
            assert back.info() == col.info()
        assert np.array_equal(col.rows(), matrix)                    # the colours object is unchanged ...
    assert np.array_equal(col.rows(), matrix)                        # ... and outlives the objects made from it


def test_compress_special_matrices(worlds):
    w = worlds(False)
    idx, n = w.idx, w.idx.n_nodes
    real = np.array(["$" not in lab for lab in w.labels])
    # an all-zero matrix
    for n_colors in (1, 130):
        with capi.WideColors.create(idx, n_colors) as empty, capi.ColorSets.from_colors(empty) as s:
            ids, table = s.copy()
            assert s.n_sets == 1 and not ids.any() and table.shape == (1, pw.n_words(n_colors)) and not table.any()
            assert s.info()["n_colored_columns"] == 0
            with s.expand() as back:
                assert not back.rows().any()
            rec, colors = s.pseudoalign_reads(w.case0.reads()[:20], True)
            assert not rec["n_found"].any() and not colors.any()
    # every real column distinct: row = column number + 1, spread over the W words four bits at a time
    for n_colors in (64, 190, 4096):
        words = pw.n_words(n_colors)
        v = np.arange(1, n + 1, dtype=np.uint64)
        assert n < 1 << 12
        m = np.zeros((n, words), dtype=np.uint64)
        for x in range(3):                                           # (into the first, the middle and the last word)
            m[:, x * (words - 1) // 2] |= v & np.uint64(15 << (4 * x))
        with capi.WideColors.from_rows(idx, m, n_colors) as up, capi.ColorSets.from_colors(up) as s:
            cleaned = up.rows()
            assert np.array_equal(cleaned[real], m[real]) and not cleaned[~real].any()
            ids, table = s.copy()
            assert s.n_sets == 1 + int(real.sum()) == 1 + s.info()["n_colored_columns"]
            want = cb.canonical_arrays(cleaned)
            assert np.array_equal(ids, want[0]) and np.array_equal(table, want[1])
            assert np.array_equal(ids[real], np.arange(1, 1 + real.sum(), dtype=np.uint32))
    # rows that differ only in word W - 1 stay distinct
    for n_colors in (70, 4096):
        words = pw.n_words(n_colors)
        m = np.zeros((n, words), dtype=np.uint64)
        m[:, :-1] = np.uint64(0x8000000000000001)
        m[:, -1] = (np.arange(n, dtype=np.uint64) % np.uint64(5)) << np.uint64(0 if n_colors == 70 else 59)
        with capi.WideColors.from_rows(idx, m, n_colors) as up, capi.ColorSets.from_colors(up) as s:
            ids, table = s.copy()
            want = cb.canonical_arrays(up.rows())
            assert s.n_sets == 6 and np.array_equal(ids, want[0]) and np.array_equal(table, want[1])
            assert len(set(table[1:, -1].tolist())) == 5 and (table[1:, :-1] == np.uint64(0x8000000000000001)).all()


# ---- 2. create ------------------------------------------------------------------------------------------------------
def test_a_non_canonical_upload_answers_like_its_canonical_form(worlds):
    for n_colors, rc in ((200, True), (64, False)):
        w = worlds(rc)
        case, col, cs, exp = w.colours(n_colors)
        reads = case.reads()
        matrix = col.rows()
        ids, table = cb.canonical_arrays(matrix)
        n_sets = len(table)
        rng = np.random.default_rng(n_colors)
        # every row twice and shuffled, rows nobody uses in between, and a column takes either copy of its row
        unused = np.zeros((3, table.shape[1]), dtype=np.uint64)
        unused[:, -1] = np.uint64(1) << np.uint64((n_colors - 1) & 63)
        unused[1, 0] = np.uint64(5)
        pool = np.concatenate([table[1:], table[1:], unused])
        origin = np.concatenate([np.arange(1, n_sets), np.arange(1, n_sets), [-1, -1, -1]])
        perm = rng.permutation(len(pool))
        table2 = np.concatenate([table[:1], pool[perm]])
        places = {o: [1 + p for p in range(len(perm)) if origin[perm[p]] == o] for o in range(1, n_sets)}
        ids2 = np.array([0 if i == 0 else places[int(i)][int(rng.integers(0, 2))] for i in ids], dtype=np.uint32)
        # junk ids on the dummy columns, out of range included: create sets them to 0
        dummy = np.array(["$" in lab for lab in w.labels])
        ids2[dummy] = rng.integers(0, 2**32, size=int(dummy.sum()), dtype=np.uint32)
        ids2[0] = 0xFFFFFFFF
        with capi.ColorSets.from_arrays(w.idx, n_colors, ids2, table2, w.k) as up, capi.ColorSets.from_colors(col) as canon:
            got_ids, got_table = up.copy()
            assert not got_ids[dummy].any() and np.array_equal(got_ids[~dummy], ids2[~dummy]) and np.array_equal(got_table, table2)
            assert up.n_sets == len(table2) and up.info()["n_colored_columns"] == canon.info()["n_colored_columns"]
            with up.expand() as back:
                assert np.array_equal(back.rows(), matrix)
                with capi.ColorSets.from_colors(back) as recompressed:   # compressing what it means gives the canonical form
                    assert same(recompressed.copy(), canon.copy())
            check_against_wide(up, col, reads, ("non-canonical", n_colors))
            for strands in (1, 2):
                for ppm, den in QUERIES:
                    assert same(up.pseudoalign_reads(reads, strands == 2, ppm, den, counts=True),
                                canon.pseudoalign_reads(reads, strands == 2, ppm, den, counts=True))


def refused(fn, *needles):
    with pytest.raises(capi.SbwtGpuError) as ei:
        fn()
    assert ei.value.code == capi.ERR_INVALID_ARG, ei.value
    for s in needles:
        assert s in ei.value.msg, (s, ei.value.msg)


def test_refusals_name_their_cause_and_leave_everything_usable(worlds, tmp_path):
    w = worlds(False)
    idx, k = w.idx, w.k
    case, col, cs, exp = w.colours(65)
    reads = case.reads()[:30]
    want = [exp.record_of(exp.window_sets(r), 1_000_000, 0) for r in reads]
    good = capi.ColorSets.from_colors(col)
    ids, table = good.copy()
    real = np.flatnonzero(np.array(["$" not in lab for lab in w.labels]))

    def still_fine():
        assert tw.as_lists(*good.pseudoalign_reads(reads)) == want
        assert tw.as_lists(*col.pseudoalign_reads(reads)) == want
        assert same(good.copy(), (ids, table))
        assert len(idx.search_reads([case.strains[0].encode()])[0]) == 400 - k + 1

    def with_id(j, v):
        out = ids.copy()
        out[j] = v
        return out

    def with_row(r, row):
        out = table.copy()
        out[r] = row
        return out

    # every invariant but the dummy columns' ids
    j = int(real[7])
    refused(lambda: capi.ColorSets.from_arrays(idx, 65, with_id(j, good.n_sets), table), "column %d" % j, "n_sets = %d" % good.n_sets)
    refused(lambda: capi.ColorSets.from_arrays(idx, 65, with_id(j, 0xFFFFFFFF), table), "column %d" % j, "n_sets")
    refused(lambda: capi.ColorSets.from_arrays(idx, 65, ids, with_row(0, [0, 1])), "row 0", "not all zero")
    refused(lambda: capi.ColorSets.from_arrays(idx, 65, ids, with_row(2, [0, 0])), "row 2", "all zero")
    refused(lambda: capi.ColorSets.from_arrays(idx, 65, ids, with_row(good.n_sets - 1, [1, 2])), "row %d" % (good.n_sets - 1), "n_colors = 65")
    with capi.ColorSets.from_arrays(idx, 65, ids, with_row(good.n_sets - 1, [1, 1])) as ok:          # (bit 64 is a colour of 65)
        assert ok.n_sets == good.n_sets
    still_fine()
    # shapes, ranges, another index, another k
    for nc in (0, 4097, -1):
        refused(lambda: capi.ColorSets.from_arrays(idx, nc, ids, table), "n_colors", "4096")
    refused(lambda: capi.ColorSets.from_arrays(idx, 65, ids, table[:, :1]), "table", "2 words")
    refused(lambda: capi.ColorSets.from_arrays(idx, 65, ids, table[:0]), "table")
    refused(lambda: capi.ColorSets.from_arrays(idx, 65, ids[:-1], table), "columns")
    refused(lambda: capi.ColorSets.from_arrays(idx, 65, ids, table, k + 1), "columns", "k =")
    other = tw.make_index(case.seqs[:2], k, False)
    assert other.n_nodes != idx.n_nodes
    refused(lambda: capi.ColorSets.from_arrays(other, 65, ids, table), "columns")
    other.close()
    L, vp = capi.lib(), capi.C.c_void_p
    refused(lambda: capi._check(L.sbwtgpu_colorsets_create(idx.handle, 65, ids.ctypes.data, 0, table.ctypes.data, capi.C.byref(vp()))), "n_sets")
    # rank-only indexes
    bits = np.random.default_rng(1).integers(0, 2**64, size=4, dtype=np.uint64)
    ro = capi.Index.create(bits, bits, bits, bits, None, 256, 3)
    refused(lambda: capi.ColorSets.from_arrays(ro, 65, np.zeros(256, np.uint32), table), "only rank()")
    still_fine()
    # strands, threshold, denominator
    bases, off = capi.concat_reads(reads)
    n = len(reads)
    out, colw = np.zeros(n, dtype=capi.READ_FOUND_DTYPE), np.zeros((n, 2), dtype=np.uint64)
    host = (bases.ctypes.data, off.ctypes.data, n)
    refused(lambda: capi._check(L.sbwtgpu_pseudoalign_sets_batch(good.handle, *host, 3, 1_000_000, 0, out.ctypes.data, colw.ctypes.data, None)),
            "strands")
    for ppm in (0, 1_000_001):
        refused(lambda: good.pseudoalign_reads(reads, False, ppm, 0), "threshold_ppm")
    refused(lambda: good.pseudoalign_reads(reads, False, 1_000_000, 2), "denominator")
    # NULL pointers at the C calls themselves
    import torch
    dev = torch.device("cuda", 0)
    d_rec, d_col = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n * 2, dtype=torch.int64, device=dev)
    d_bases, d_off = torch.from_numpy(bases.copy()).to(dev), torch.from_numpy(off.copy()).to(dev)
    need = capi.pseudoalign_workspace_bytes(len(bases), n, False)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    q = (1, 1_000_000, 0)
    refused(lambda: capi._check(L.sbwtgpu_pseudoalign_sets_batch(None, *host, *q, out.ctypes.data, colw.ctypes.data, None)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_pseudoalign_sets_batch(good.handle, *host, *q, None, colw.ctypes.data, None)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_pseudoalign_sets_batch(good.handle, *host, *q, out.ctypes.data, None, None)), "NULL")
    device = (d_bases.data_ptr(), len(bases), d_off.data_ptr(), n, *q)
    tail = (None, ws.data_ptr(), need, None)
    refused(lambda: capi._check(L.sbwtgpu_pseudoalign_sets_dev(None, *device, d_rec.data_ptr(), d_col.data_ptr(), *tail)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_pseudoalign_sets_dev(good.handle, *device, None, d_col.data_ptr(), *tail)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_pseudoalign_sets_dev(good.handle, *device, d_rec.data_ptr(), None, *tail)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_pseudoalign_sets_dev(good.handle, d_bases.data_ptr(), len(bases), None, n, *q, d_rec.data_ptr(),
                                                               d_col.data_ptr(), *tail)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_pseudoalign_sets_dev(good.handle, *device, d_rec.data_ptr(), d_col.data_ptr(), None, ws.data_ptr(),
                                                               need - 1, None)), "workspace")
    torch.cuda.synchronize(dev)
    assert not d_rec.any().item() and not d_col.any().item()          # and nothing was written
    out_h = vp()
    refused(lambda: capi._check(L.sbwtgpu_colorsets_compress(None, capi.C.byref(out_h))), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_colorsets_compress(col.handle, None)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_colorsets_create(None, 65, ids.ctypes.data, good.n_sets, table.ctypes.data, capi.C.byref(out_h))), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_colorsets_create(idx.handle, 65, None, good.n_sets, table.ctypes.data, capi.C.byref(out_h))), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_colorsets_create(idx.handle, 65, ids.ctypes.data, good.n_sets, None, capi.C.byref(out_h))), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_colorsets_create(idx.handle, 65, ids.ctypes.data, good.n_sets, table.ctypes.data, None)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_colorsets_expand(None, capi.C.byref(out_h))), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_colorsets_expand(good.handle, None)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_colorsets_info(None, None, None, None, None, None, None, None)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_colorsets_copy(None, ids.ctypes.data, table.ctypes.data)), "NULL")
    refused(lambda: capi._check(L.sbwtgpu_colorsets_dev(None, None, None)), "NULL")
    L.sbwtgpu_colorsets_destroy(None)
    capi._check(L.sbwtgpu_colorsets_info(good.handle, None, None, None, None, None, None, None))          # every output may be NULL
    # the same device call with every pointer in place is the host call's answer
    capi._check(L.sbwtgpu_pseudoalign_sets_dev(good.handle, *device, d_rec.data_ptr(), d_col.data_ptr(), *tail))
    torch.cuda.synchronize(dev)
    assert tw.as_lists(d_rec.cpu().numpy().view(capi.READ_FOUND_DTYPE), d_col.cpu().numpy().view(np.uint64).reshape(n, 2)) == want
    # a colour-set file -> from_arrays gives the same object
    path = str(tmp_path / "s.colors")
    hostlib.colorsets_write(path, ids, table, 65, k)
    fi, ft, nc, kk = hostlib.colorsets_read(path)
    with capi.ColorSets.from_arrays(idx, nc, fi, ft, kk) as back:
        assert same(back.copy(), (ids, table)) and back.info() == good.info()
    still_fine()
    good.close()


# ---- 3. the queries against the wide call and the brute ----------------------------------------------------------------
@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
@pytest.mark.parametrize("n_colors", N_COLORS)
def test_records_words_and_counts(worlds, n_colors, rc):
    w = worlds(rc)
    case, col, cs, exp = w.colours(n_colors)
    reads = case.reads()                                  # m in {0, 1, 63, 64, 65, 129}, the 5 000-window read and the traps
    with capi.ColorSets.from_colors(col) as s, s.expand() as wide:
        for strands in (1, 2):
            sets = [exp.window_sets(r, strands) for r in reads]
            for ppm, den in QUERIES:
                label = (n_colors, rc, strands, ppm, den)
                got = tw.check_query(s, exp, reads, sets, strands, ppm, den, label)                  # the brute
                assert same(got, wide.pseudoalign_reads(reads, strands == 2, ppm, den, counts=True)), label
                assert same(got, col.pseudoalign_reads(reads, strands == 2, ppm, den, counts=True)), label
            # counts off on the device entry point: the counts buffer keeps its sentinel, records and words are the same
            drec, dcol, dcnt, status = tw.run_dev(s, reads, strands, ppm, den, False)
            assert status == 0 and drec.tobytes() == got[0].tobytes() and np.array_equal(dcol, got[1])
            assert (dcnt == tw.PAT32).all()


# ---- 4. kernel corners via uploaded tables -----------------------------------------------------------------------------
class Corner:
    """An index of one random sequence S whose windows are all different: window i of S sits in column col_f[i], its reverse
    complement (rc indexes) in col_r[i], so a test chooses the id of every window of a read that is a piece of S."""

    def __init__(self, rc, k=13, length=470, seed=21):
        rng = random.Random(seed)
        self.k, self.rc = k, rc
        self.S = pw.rand_seq(rng, length)
        self.wins = pb.windows(self.S, k)
        assert len(set(self.wins)) == len(self.wins) and not set(self.wins) & {pb.revcomp(x) for x in self.wins}
        self.idx = tw.make_index([self.S], k, rc)
        self.where = {lab: j for j, lab in enumerate(tw.labels_of(self.idx)) if "$" not in lab}
        self.col_f = [self.where[x] for x in self.wins]
        self.col_r = [self.where[pb.revcomp(x)] for x in self.wins] if rc else None
        assert 300 < self.idx.n_nodes < 3000

    def upload(self, n_colors, table, ids_f, ids_r=None):
        """table: integer rows (row 0 = 0); ids_f / ids_r: window number -> id of its column / of its reverse complement's"""
        ids = np.zeros(self.idx.n_nodes, dtype=np.uint32)
        for i, v in ids_f.items():
            ids[self.col_f[i]] = v
        for i, v in (ids_r or {}).items():
            ids[self.col_r[i]] = v
        self.ids, self.table, self.n_colors = ids, list(table), n_colors
        self.exp = pw.Expected([set() for _ in range(n_colors)], set(), self.k)          # (for record_of and counts_of alone)
        return capi.ColorSets.from_arrays(self.idx, n_colors, ids, pw.rows_array(table, pw.n_words(n_colors)), self.k)

    def window_sets(self, read, strands):
        out = []
        for x in pb.windows(read, self.k):
            s = 0
            for y in ([x, pb.revcomp(x)] if strands == 2 else [x]):
                if pb.valid(x) and y in self.where:
                    s |= self.table[int(self.ids[self.where[y]])]
            out.append(s)
        return out

    def piece(self, lo, hi):
        """the read whose windows are windows lo .. hi - 1 of S"""
        return self.S[lo:hi + self.k - 1].encode()

    def check(self, obj, reads, label, strands=(1, 2)):
        """records, words and counts against the table by hand and against the wide call on the expanded object; returns the
        records of the last strand mode as lists"""
        with obj.expand() as wide:
            for st in strands:
                sets = [self.window_sets(r, st) for r in reads]
                for ppm, den in QUERIES:
                    got = tw.check_query(obj, self.exp, reads, sets, st, ppm, den, (label, st, ppm, den))
                    assert same(got, wide.pseudoalign_reads(reads, st == 2, ppm, den, counts=True)), (label, st, ppm, den)
        return tw.as_lists(*obj.pseudoalign_reads(reads, strands[-1] == 2, 1, 0))


@pytest.fixture(scope="module")
def corners(gpu):
    made = {}

    def get(rc):
        if rc not in made:
            made[rc] = Corner(rc)
        return made[rc]
    yield get
    for c in made.values():
        c.idx.close()


def bits(*cs):
    return sum(1 << c for c in cs)


@pytest.mark.parametrize("n_colors", [1, 130, 4096])
def test_an_iteration_with_64_distinct_ids(corners, n_colors):
    c = corners(False)
    last = n_colors - 1
    # set r: a colour of its own where there are that many, the last colour for the even ones, colour 0 for every third
    table = [0] + [bits(*{(r * 61) % n_colors, last if r % 2 == 0 else (r * 61) % n_colors, 0 if r % 3 == 0 else (r * 61) % n_colors})
                   for r in range(1, 65)]
    ids_f = {i: 1 + (i % 64) for i in range(256)}
    ids_f.update({i: 64 - (i % 64) for i in range(256, 320)})
    with c.upload(n_colors, table, ids_f) as obj:
        reads = [c.piece(0, 64), c.piece(0, 65), c.piece(1, 65), c.piece(0, 256), c.piece(30, 320), c.piece(63, 64), c.piece(200, 400)]
        got = c.check(obj, reads, ("64 ids", n_colors), strands=(1,))
        assert got[0][1:] == (64, 64) and got[6][1:] == (200, 120)
        if n_colors == 4096:
            assert got[0][0] == bits(*{(r * 61) % 4096 for r in range(1, 65)} | {0, 4095})


@pytest.mark.parametrize("n_colors", [64, 200])
def test_runs_and_the_pending_key(corners, n_colors):
    c = corners(False)
    last = n_colors - 1
    A, B = bits(0, last), bits(1, last, n_colors // 2)
    table = [0, A, B, A]                                       # (row 3 repeats row 1: another key, the same set)
    ids_f = {}
    ids_f.update({i: 1 for i in range(0, 150)})                # a run over three iterations that changes key inside the third
    ids_f.update({i: 2 for i in range(150, 200)})
    ids_f.update({i: 1 for i in range(200, 264)})              # the pending key again after an all-miss iteration (id 0) ...
    ids_f.update({i: 0 for i in range(264, 328)})
    ids_f.update({i: 1 for i in range(328, 392)})
    ids_f.update({i: 3 for i in range(392, 420)})              # ... and the same set under another id
    with c.upload(n_colors, table, ids_f) as obj:
        miss = bytearray(c.piece(200, 392))                      # the same with true misses: N in every window 264 .. 327
        miss[64 + c.k - 1:128] = b"N" * (128 - (64 + c.k - 1))
        reads = [c.piece(0, 200), c.piece(0, 150), c.piece(149, 151), c.piece(200, 392), bytes(miss), c.piece(328, 420), c.piece(0, 420),
                 c.piece(100, 300)]
        got = c.check(obj, reads, ("runs", n_colors), strands=(1,))
        assert got[0] == (A | B, 200, 200) and got[3] == (A, 192, 128) and got[4] == (A, 192, 128) and got[5] == (A, 92, 92)
        rec, colors, cnt = obj.pseudoalign_reads(reads, False, 1_000_000, 0, counts=True)
        assert cnt[0, 0] == 150 and cnt[0, 1] == 50 and cnt[0, last] == 200 and cnt[3, 0] == 128 and cnt[4, last] == 128


def test_two_strands_pair_keys(corners):
    c = corners(True)
    n_colors = 4096
    a, b = 1, 2
    table = [0, bits(3, 4095), bits(70, 4095, 2000), bits(4095)]          # (row 3: colour 4095 alone, word 0 zero)
    ids_f, ids_r = {}, {}
    # windows 0 .. 99 in runs of 20: (a, b), (b, a), (a, 0), (0, a), (a, a); then all five kinds inside one iteration
    kinds = [(a, b), (b, a), (a, 0), (0, a), (a, a)]
    for i in range(100):
        ids_f[i], ids_r[i] = kinds[i // 20]
    for i in range(100, 164):
        ids_f[i], ids_r[i] = kinds[i % 5]
    for i in range(164, 228):                                   # the set whose only bit is colour 4095, from either strand
        ids_f[i], ids_r[i] = (3, 0) if i % 2 else (0, 3)
    with c.upload(n_colors, table, ids_f, ids_r) as obj:
        reads = [c.piece(0, 100), c.piece(0, 40), c.piece(40, 80), c.piece(80, 100), c.piece(100, 164), c.piece(164, 228), c.piece(0, 228),
                 pb.revcomp(c.S[:150]).encode(), c.piece(20, 60)]
        got = c.check(obj, reads, "pairs")
        ab = table[a] | table[b]
        assert got[1] == (ab, 40, 40) and got[2] == (table[a], 40, 40) and got[3] == (table[a], 20, 20)
        assert got[5] == (bits(4095), 64, 64)
        one = tw.as_lists(*obj.pseudoalign_reads(reads, False, 1, 0))
        assert one[1] == (ab, 40, 40) and one[2] == (table[a], 40, 20) and one[5] == (bits(4095), 64, 32)
        rec, colors, cnt = obj.pseudoalign_reads(reads, True, 1_000_000, 0, counts=True)
        assert cnt[0, 3] == 100 and cnt[0, 70] == 40 and cnt[0, 4095] == 100 and cnt[5, 4095] == 64 and cnt[5, :4095].sum() == 0


def test_nothing_leaks_between_the_reads_of_one_wave(gpu):
    """More than 8 x 2^20 reads of one window each in one launch: the grid is capped at 2^20 blocks of four waves, so wave r
    takes reads r, r + 2^22 and r + 2^23 -- set A, a miss, set B."""
    k, n_colors = 5, 70
    seq = "ACGTTGCAAGGCTATCCGATAGCAT"
    idx = tw.make_index([seq], k, False)
    where = {lab: j for j, lab in enumerate(tw.labels_of(idx)) if "$" not in lab}
    ka, kb, miss = seq[0:5], seq[9:14], "TTTTT"
    assert ka != kb and miss not in where
    A, B = bits(0, 69), bits(1, 68)
    ids = np.zeros(idx.n_nodes, dtype=np.uint32)
    ids[where[ka]], ids[where[kb]] = 1, 2
    N1, extra = 1 << 22, 300
    n = 2 * N1 + extra
    bases = np.empty((n, k), dtype=np.uint8)
    bases[:N1], bases[N1:2 * N1], bases[2 * N1:] = (np.frombuffer(x.encode(), dtype=np.uint8) for x in (ka, miss, kb))
    off = np.arange(n + 1, dtype=np.int64) * k
    with capi.ColorSets.from_arrays(idx, n_colors, ids, pw.rows_array([0, A, B], 2)) as obj, tw.tuning("pseudoalign_chunk_bases", 1 << 30, 0):
        rec, colors = obj.pseudoalign(bases.reshape(-1), off, False, 1_000_000, 0)
    assert (rec["n_kmers"] == 1).all()
    assert (rec["n_found"][:N1] == 1).all() and not rec["n_found"][N1:2 * N1].any() and (rec["n_found"][2 * N1:] == 1).all()
    for part, row in ((colors[:N1], A), (colors[N1:2 * N1], 0), (colors[2 * N1:], B)):
        assert (part == pw.rows_array([row], 2)[0]).all()
    idx.close()


# ---- 5. plumbing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_colors", [65, 4096])
def test_chunking_and_the_device_entry_point(worlds, n_colors):
    w = worlds(n_colors != 65)
    case, col, cs, exp = w.colours(n_colors)
    reads = case.reads()
    total = sum(len(r) for r in reads)
    with capi.ColorSets.from_colors(col) as s:
        for strands in (1, 2):
            want = s.pseudoalign_reads(reads, strands == 2, 500_000, 1, counts=True)
            assert same(want, col.pseudoalign_reads(reads, strands == 2, 500_000, 1, counts=True))
            for budget in (1, total // 4):                        # every read a chunk; at least three chunks
                with tw.tuning("pseudoalign_chunk_bases", budget, 0):
                    assert same(s.pseudoalign_reads(reads, strands == 2, 500_000, 1, counts=True), want), (strands, budget)
            drec, dcol, dcnt, status = tw.run_dev(s, reads, strands, 500_000, 1, True)
            assert status == 0 and drec.tobytes() == want[0].tobytes() and np.array_equal(dcol, want[1])
            assert np.array_equal(dcnt[tw.GUARD:-tw.GUARD].reshape(len(reads), n_colors), want[2])
            assert len(s.pseudoalign(np.zeros(0, np.uint8), np.zeros(1, np.int64))[0]) == 0               # n_reads = 0
            rec, colors = s.pseudoalign_reads([b"", b"ACG", b""], strands == 2)                            # no window at all
            assert tw.as_lists(rec, colors) == [(0, 0, 0)] * 3


def test_a_lower_image_level_and_two_threads(worlds):
    w = worlds(True)
    n_colors = 200
    case, col, cs, exp = w.colours(n_colors)
    reads = case.reads()
    ids, table = cb.canonical_arrays(col.rows())
    with capi.ColorSets.from_colors(col) as s:
        want = {st: s.pseudoalign_reads(reads, st == 2, 500_000, 0, counts=True) for st in (1, 2)}
        with tw.tuning("image_level", 1, 0):
            low = tw.make_index(case.seqs, w.k, True)
        assert low.image_level >= 1
        with capi.ColorSets.from_arrays(low, n_colors, ids, table, w.k) as s2:
            assert same(s2.copy(), s.copy())
            for st in (1, 2):
                assert same(s2.pseudoalign_reads(reads, st == 2, 500_000, 0, counts=True), want[st]), st
        low.close()
        # two host threads query one object
        bad = []

        def worker(st):
            try:
                for _ in range(4):
                    if not same(s.pseudoalign_reads(reads, st == 2, 500_000, 0, counts=True), want[st]):
                        bad.append(st)
            except Exception as e:                              # noqa: BLE001  (reported by the assertion below)
                bad.append(repr(e))
        threads = [threading.Thread(target=worker, args=(st,)) for st in (1, 2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not bad, bad


# ---- 6. the CLI -------------------------------------------------------------------------------------------------------
def test_cli(gpu, tmp_path):
    d = str(tmp_path)
    case = pw.Case(70, False)
    k, seqs = case.k, case.seqs
    with open(d + "/s.fna", "w") as fh:
        for i, s in enumerate(seqs):
            fh.write(">s%d\n%s\n" % (i, s))
    p = tw.run([tw.SBWT, "build", "-i", d + "/s.fna", "-o", d + "/fwd.sbwt", "-k", str(k), "--temp-dir", d])
    assert p.returncode == 0, p.stderr.decode()
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
    reads = [r.upper() for r in case.reads() if r]
    with open(d + "/r.fq", "w") as fh:
        for j, r in enumerate(reads):
            fh.write("@r%d\n%s\n+\n%s\n" % (j, r.decode(), "I" * len(r)))
    for both in (False, True):
        strands = 2 if both else 1
        flags = ["--both-strands"] if both else []
        cs = [set() for _ in range(70)]
        for c in range(70):
            pb.add(cs, kmers, k, c, refs[c], strands)
        exp = pw.Expected(cs, kmers, k)
        wide, sets, conv = ("%s/%s%d.colors" % (d, name, both) for name in ("wide", "sets", "conv"))
        p = tw.run([tw.SBWT, "build-colors", "--wide", "-i", d + "/fwd.sbwt", "-r", d + "/refs.txt", "-o", wide] + flags)
        assert p.returncode == 0, p.stderr.decode()
        pw_lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("colour ")]
        p = tw.run([tw.SBWT, "build-colors", "--compress", "-i", d + "/fwd.sbwt", "-r", d + "/refs.txt", "-o", sets] + flags)
        assert p.returncode == 0, p.stderr.decode()
        assert [ln for ln in p.stdout.decode().splitlines() if ln.startswith("colour ")] == pw_lines and len(pw_lines) == 70
        assert open(sets, "rb").read(8) == b"SBWTCOL3"
        # the file holds the canonical form of the wide file's matrix
        rows, n_colors, kk = hostlib.colors_read_wide(wide)
        ids, table, nc2, k2 = hostlib.colorsets_read(sets)
        assert (nc2, k2) == (n_colors, kk) == (70, k)
        want_ids, want_table = cb.canonical_arrays(rows)
        assert np.array_equal(ids, want_ids) and np.array_equal(table, want_table)
        # compress-colors of the wide file gives the same bytes
        p = tw.run([tw.SBWT, "compress-colors", "-i", d + "/fwd.sbwt", "-c", wide, "-o", conv])
        assert p.returncode == 0, p.stderr.decode()
        assert open(conv, "rb").read() == open(sets, "rb").read()
        for opts, ppm, den in (([], 1_000_000, 0), (["--threshold", "0.5", "--all-kmers"], 500_000, 1)):
            want = pw.format_lines(exp.record_of(exp.window_sets(r, strands), ppm, den)[0] for r in reads)
            for z in ((False, True) if not both and not opts else (False,)):          # (-z once)
                outs = []
                for colors in (wide, sets):
                    out = "%s/o.%d%d%d%d.out" % (d, z, both, den, colors == sets)
                    p = tw.run([tw.SBWT, "pseudoalign", "-i", d + "/fwd.sbwt", "-c", colors, "-q", d + "/r.fq", "-o", out] + opts +
                               (["-z"] if z else []) + flags)
                    assert p.returncode == 0, p.stderr.decode()
                    outs.append(gzip.open(out).read() if z else open(out, "rb").read())
                assert outs[0] == outs[1] == want, (z, both, opts)          # byte-identical to the --wide file's output
        assert any(int(c) >= 64 for ln in want.decode().splitlines() for c in ln.split()[1:])
    # small batches give the same lines
    p = tw.run([tw.SBWT, "pseudoalign", "-i", d + "/fwd.sbwt", "-c", sets, "-q", d + "/r.fq", "-o", d + "/small.out", "--threshold", "0.5",
                "--all-kmers", "--both-strands", "--batch-bases", "100"])
    assert p.returncode == 0, p.stderr.decode()
    assert open(d + "/small.out", "rb").read() == want
    # a 64-colour file ("SBWTCOL1") converts too, and answers as it did
    with open(d + "/refs3.txt", "w") as fh:
        fh.write("".join("%s/ref%d.fna\n" % (d, c) for c in (0, 63, 64)))
    for name, cmd in (("three1", ["build-colors"]), ("three3", ["build-colors", "--compress"])):
        p = tw.run([tw.SBWT] + cmd + ["-i", d + "/fwd.sbwt", "-r", d + "/refs3.txt", "-o", "%s/%s.colors" % (d, name)])
        assert p.returncode == 0, p.stderr.decode()
    p = tw.run([tw.SBWT, "compress-colors", "-i", d + "/fwd.sbwt", "-c", d + "/three1.colors", "-o", d + "/three13.colors"])
    assert p.returncode == 0, p.stderr.decode()
    assert open(d + "/three1.colors", "rb").read(8) == b"SBWTCOL1"
    assert open(d + "/three13.colors", "rb").read() == open(d + "/three3.colors", "rb").read()
    outs = []
    for name in ("three1", "three3"):
        p = tw.run([tw.SBWT, "pseudoalign", "-i", d + "/fwd.sbwt", "-c", "%s/%s.colors" % (d, name), "-q", d + "/r.fq", "-o", d + "/t.out"])
        assert p.returncode == 0, p.stderr.decode()
        outs.append(open(d + "/t.out", "rb").read())
    assert outs[0] == outs[1] and len(outs[0].splitlines()) == len(reads)
    # 4097 lines are refused; a colour-set file of another index is refused; a colour-set file is no input of compress-colors
    with open(d + "/refs4097.txt", "w") as fh:
        fh.write(("%s/ref0.fna\n" % d) * 4097)
    p = tw.run([tw.SBWT, "build-colors", "--compress", "-i", d + "/fwd.sbwt", "-r", d + "/refs4097.txt", "-o", d + "/x.colors"], 60)
    assert p.returncode != 0 and b"4097" in p.stderr and b"4096" in p.stderr
    hostlib.colorsets_write(d + "/other.colors", ids[:-1], table, 70, k)
    p = tw.run([tw.SBWT, "pseudoalign", "-i", d + "/fwd.sbwt", "-c", d + "/other.colors", "-q", d + "/r.fq", "-o", d + "/x.out"], 60)
    assert p.returncode != 0 and b"columns" in p.stderr
    p = tw.run([tw.SBWT, "compress-colors", "-i", d + "/fwd.sbwt", "-c", sets, "-o", d + "/x.colors"], 60)
    assert p.returncode != 0 and b"magic" in p.stderr


# ---- 7. a bounded seeded fuzz -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz(gpu, seed):
    rng = random.Random(7000 + seed)
    for case in range(5):
        k = rng.randint(2, 64)
        rc, ssup = rng.random() < 0.5, rng.random() < 0.5
        n_colors = rng.randint(1, 200)
        strands_add, strands_q = rng.randint(1, 2), rng.randint(1, 2)
        ppm, den = rng.choice([1, rng.randint(1, 1_000_000), 500_000, 1_000_000]), rng.randint(0, 1)
        seqs = [pw.rand_seq(rng, rng.randint(k, 2 * k + 80)) for _ in range(rng.randint(1, 4))]
        label = (seed, case, k, rc, ssup, n_colors, strands_add, strands_q, ppm, den)
        idx = tw.make_index(seqs, k, rc, ssup)
        kmers = kmer_set(list(seqs) + ([pb.revcomp(s) for s in seqs] if rc else []), k)
        col, cs = tw.colour_both(idx, kmers, k, n_colors, tw.fuzz_inputs(rng, seqs, k, n_colors), strands_add)
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
        matrix = col.rows()
        with capi.ColorSets.from_colors(col) as s:
            assert same(s.copy(), cb.canonical_arrays(matrix)), label
            with s.expand() as back:
                assert np.array_equal(back.rows(), matrix), label
            with tw.tuning("pseudoalign_chunk_bases", rng.choice([0, 1, 300]), 0):
                got = tw.check_query(s, exp, reads, [exp.window_sets(r, strands_q) for r in reads], strands_q, ppm, den, label)
                assert same(got, col.pseudoalign_reads(reads, strands_q == 2, ppm, den, counts=True)), label
        col.close()
        idx.close()
