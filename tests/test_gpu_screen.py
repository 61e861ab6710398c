"""GPU: sbwtgpu_screen_* (sbwt_screen.hip: a read set screened against the references of a colour-set object) against the
definition in tests/screen_brute.py.  Real colour sets are compared with the brute force over k-mer strings; uploaded objects
(free n_sets, n_colors and ids) with the definition over their arrays, fed with the columns the library's own search gives
for the sample's windows.  Every comparison is exact."""
import gzip
import random
import threading

import numpy as np
import pytest

import pseudoalign_brute as pb
import pseudoalign_wide as pw
import screen_brute as sb
import test_gpu_pseudoalign_wide as tw          # its helpers: make_index, labels_of, refused, run, tuning, SBWT
from sbwt_amd import capi

pytestmark = pytest.mark.gpu

K = 15
GUARD, PAT = 4096, 0x5A


def enc(reads):
    return [r.encode() if isinstance(r, str) else r for r in reads]


def mutate(rng, s, p=0.03, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) if rng.random() < p else c for c in s)


class World:
    """One index of some 25 000 columns with the real colour sets of five strains, and a sample of reads from them."""

    def __init__(self):
        rng = random.Random(2323)
        base = pw.rand_seq(rng, 10000)
        self.refs = [mutate(rng, base) + pw.rand_seq(rng, 800) for _ in range(5)]
        self.refs[4] = self.refs[4][:3000]
        self.extra = pw.rand_seq(rng, 500)                       # k-mers of the index that no reference colours
        self.seqs = self.refs + [self.extra]
        self.idx = tw.make_index(self.seqs, K)
        self.n = self.idx.n_nodes
        self.labels = tw.labels_of(self.idx)
        self.kmers = {lab for lab in self.labels if "$" not in lab}
        self.n_dummies = self.n - len(self.kmers)
        self.cs = [set() for _ in self.refs]
        with capi.ColorSetsBuilder.create(self.idx, len(self.refs)) as b:
            for c, s in enumerate(self.refs):
                b.add_reads(c, [s.encode()])
                pb.add(self.cs, self.kmers, K, c, [s])
            self.sets = b.finish()
        self.ids, self.table = self.sets.copy()
        self.rows = pw.rows_ints(self.table)
        # the sample: pieces of the strains with substitutions, an N here and there, some from the uncoloured stretch, some
        # reverse-complemented, some random, one shorter than k, one empty
        self.reads = []
        for i in range(120):
            src = self.extra if i % 10 == 9 else self.refs[i % 5]
            a = rng.randrange(0, len(src) - 30)
            r = mutate(rng, src[a:a + rng.randint(K, 220)], 0.02, "ACGTN" if i % 7 == 0 else "ACGT")
            self.reads.append(sb.revcomp(r) if i % 4 == 3 else r)
        self.reads += [pw.rand_seq(rng, 100), "ACGT", "", self.refs[0][:K], self.refs[1][5:5 + K + 1]]

    def want(self, reads, strands=1):
        return sb.Screen(self.kmers, self.cs, K, reads, strands)

    def upload(self, n_sets, n_colors, seed, ids=None):
        """A random object on the world's index: rows of density 1/4, every row but 0 non-zero, the last colour in use (in
        set 1, and with it the last word of a row), ids uniform over the sets unless given.  Returns the object, its ids as
        the device holds them (dummy columns 0) and its rows as integers."""
        rng = np.random.default_rng(seed)
        words = pw.n_words(n_colors)
        table = rng.integers(0, 2**64, size=(n_sets, words), dtype=np.uint64) & rng.integers(0, 2**64, size=(n_sets, words), dtype=np.uint64)
        if n_colors % 64:
            table[:, -1] &= np.uint64((1 << (n_colors % 64)) - 1)
        one = rng.integers(0, n_colors, size=n_sets)
        table[np.arange(n_sets), one >> 6] |= np.uint64(1) << (one & 63).astype(np.uint64)
        if n_sets > 1:
            table[1, (n_colors - 1) >> 6] |= np.uint64(1) << np.uint64((n_colors - 1) & 63)
        table[0] = 0
        if ids is None:
            ids = rng.integers(0, n_sets, size=self.n)
        s = capi.ColorSets.from_arrays(self.idx, n_colors, np.asarray(ids, dtype=np.uint32), table)
        return s, s.copy()[0], pw.rows_ints(table)

    def results(self, reads, strands=1, idx=None):
        """the columns (or -1) of the sample's occurrences, from the library's own search"""
        reads = list(reads) + ([sb.revcomp(r) for r in reads] if strands == 2 else [])
        bases, off = capi.concat_reads(enc(reads))
        return (idx or self.idx).search(bases, off)[0]


@pytest.fixture(scope="module")
def world(gpu):
    w = World()
    assert 20000 <= w.n <= 30000 and w.n_dummies > 0 and len(w.rows) > 8
    yield w
    w.sets.close()
    w.idx.close()


@pytest.fixture(scope="module")
def truth(world):
    """the brute force of the world's sample, computed once: one strand and two"""
    return {1: world.want(world.reads, 1), 2: world.want(world.reads, 2)}


def state(scr):
    return scr.info(), [v.tolist() for v in scr.sets()], [v.tolist() for v in scr.colors()], scr.seen().tolist()


def check_real(scr, S, w, label=None):
    """a screen on the world's real colour sets against the brute force S"""
    info = scr.info()
    assert (info["n_windows"], info["n_hits"], info["n_seen"]) == (S.n_windows, S.n_hits, S.n_seen), (label, info)
    assert (info["n_sets"], info["n_colors"]) == (len(w.rows), len(w.cs)), label
    got = scr.sets()
    assert all(v.dtype == np.int64 and v.shape == (len(w.rows),) for v in got), label
    want = S.sets(w.rows, w.n_dummies)
    for name, g, x in zip(("set_kmers", "set_seen", "set_hits"), got, want):
        assert g.tolist() == x, (label, name)
    got = scr.colors()
    for name, g, x in zip(("ref_kmers", "ref_seen", "ref_hits"), got, (S.ref_kmers, S.ref_seen, S.ref_hits)):
        assert g.dtype == np.int64 and g.tolist() == x, (label, name)
    assert [int(x) for x in scr.seen()] == S.seen_bitmap(w.labels), label


def check_arrays(scr, ids, rows, n_colors, results, label=None):
    """a screen on an uploaded object against the definition over its arrays"""
    A = sb.from_arrays(ids.tolist(), rows, n_colors, results.tolist())
    info = scr.info()
    assert (info["n_windows"], info["n_hits"], info["n_seen"]) == (A["n_windows"], A["n_hits"], A["n_seen"]), (label, info)
    for name, g in zip(("set_kmers", "set_seen", "set_hits"), scr.sets()):
        assert g.tolist() == A[name], (label, name)
    for name, g in zip(("ref_kmers", "ref_seen", "ref_hits"), scr.colors()):
        assert g.tolist() == A[name], (label, name)
    seen = scr.seen()
    bits = np.unpackbits(seen.view(np.uint8), bitorder="little")
    assert np.flatnonzero(bits).tolist() == A["seen"], label
    return A


# ---- 1. the definition: known answers, and random k-mer sets at every k ----------------------------------------------
def small_world(refs, extra, k):
    idx = tw.make_index(refs + extra, k)
    labels = tw.labels_of(idx)
    kmers = {lab for lab in labels if "$" not in lab}
    cs = [set() for _ in refs]
    with capi.ColorSetsBuilder.create(idx, len(refs)) as b:
        for c, s in enumerate(refs):
            b.add_reads(c, [s.encode()])
            pb.add(cs, kmers, k, c, [s])
        sets = b.finish()
    return idx, labels, kmers, cs, sets


class Small:
    def __init__(self, refs, extra, k):
        self.idx, self.labels, self.kmers, self.cs, self.sets = small_world(refs, extra, k)
        self.rows = pw.rows_ints(self.sets.copy()[1])
        self.n_dummies = self.idx.n_nodes - len(self.kmers)

    def close(self):
        self.sets.close()
        self.idx.close()


def test_known_answers(gpu):
    # the k = 3 examples of the unitig-graph table as references (tests/test_screen_cpu.py has the numbers on paper)
    w = Small(["AACG", "AACT", "AAAAA", "ACGTACG"], ["GGG"], 3)
    for reads, strands, numbers in (([b"AAAAAC"], 1, (4, 4, 2)), ([b"GGGGG"], 1, (3, 3, 1)), ([b"AC", b"", b"A"], 1, (0, 0, 0)),
                                    ([b"AANAAAC"], 1, (5, 2, 2)), ([b"AANAAAC"], 2, (10, 2, 2)), ([b"TTTTT", b"CCCCC"], 1, (6, 0, 0)),
                                    ([b"GGGG", b"AAAC"], 1, (4, 4, 3))):
        with w.sets.screen() as scr:
            scr.add_reads(reads, strands)
            S = sb.Screen(w.kmers, w.cs, 3, reads, strands)
            assert (S.n_windows, S.n_hits, S.n_seen) == numbers, reads
            check_real(scr, S, w, reads)
    with w.sets.screen() as scr:
        scr.add_reads([b"AAAAAC"])
        assert [v.tolist() for v in scr.colors()] == [[2, 2, 1, 4], [1, 1, 1, 0], [1, 1, 3, 0]]
        scr.add_reads([b"GGGG"])                                  # a k-mer of the index that no reference holds: set 0 gets the hits
        assert scr.sets()[2][0] == 2 and [v.tolist() for v in scr.colors()] == [[2, 2, 1, 4], [1, 1, 1, 0], [1, 1, 3, 0]]
    w.close()
    # a palindromic window under two strands: two occurrences of one k-mer
    w = Small(["ACGTT"], [], 4)
    for reads, strands, numbers in (([b"ACGT"], 2, (2, 2, 1)), ([b"AACG"], 2, (2, 1, 1)), ([b"AACG"], 1, (1, 0, 0))):
        with w.sets.screen() as scr:
            scr.add_reads(reads, strands)
            S = sb.Screen(w.kmers, w.cs, 4, reads, strands)
            assert (S.n_windows, S.n_hits, S.n_seen) == numbers, reads
            check_real(scr, S, w, reads)
    w.close()


@pytest.mark.parametrize("k", [2, 3, 4, 7, 16, 31, 32, 33, 63, 64])
def test_random_kmer_sets(gpu, k):
    rng = random.Random(100 + k)
    alphabet = "ACGT" if k > 4 else "AC"
    base = pw.rand_seq(rng, 300 + 4 * k, alphabet)
    refs = [mutate(rng, base, 0.05, alphabet) + pw.rand_seq(rng, 40, alphabet) for _ in range(3)]
    w = Small(refs, [pw.rand_seq(rng, 60 + k, alphabet)], k)
    reads = []
    for i in range(25):
        src = rng.choice(refs)
        a = rng.randrange(0, len(src) - k)
        r = mutate(rng, src[a:a + rng.randint(k - 1, 3 * k + 20)], 0.02, alphabet + ("N" if i % 5 == 0 else ""))
        reads.append(sb.revcomp(r) if i % 3 == 0 else r)
    for strands in (1, 2):
        with w.sets.screen() as scr:
            scr.add_reads(enc(reads), strands)
            S = sb.Screen(w.kmers, w.cs, k, reads, strands)
            assert S.n_hits > 0
            check_real(scr, S, w, (k, strands))
    w.close()


# ---- 2. the world's real sets, one strand and two; strands 2 = strands 1 on the reads and their reverse complements ----
def test_real_sets_both_strand_modes(world, truth):
    states = {}
    for strands in (1, 2):
        with world.sets.screen() as scr:
            scr.add_reads(enc(world.reads), strands)
            check_real(scr, truth[strands], world, strands)
            states[strands] = state(scr)
    assert truth[2].n_hits > truth[1].n_hits > 0 and truth[1].row_hits.get(0, 0) > 0
    with world.sets.screen() as scr:
        scr.add_reads(enc(world.reads + [sb.revcomp(r) for r in world.reads]), 1)
        assert state(scr) == states[2]


# ---- 3. colour counts: W = 1, 2 and 64 ------------------------------------------------------------------------------
@pytest.mark.parametrize("n_colors", [3, 64, 70, 4096])
def test_colour_counts(world, n_colors):
    n_sets = 60 if n_colors == 4096 else 333
    s, ids, rows = world.upload(n_sets, n_colors, 3000 + n_colors)
    assert rows[1] >> (n_colors - 1) == 1
    with s, s.screen() as scr:
        scr.add_reads(enc(world.reads), 2)
        A = check_arrays(scr, ids, rows, n_colors, world.results(world.reads, 2), n_colors)
        assert A["ref_hits"][n_colors - 1] > 0 and A["ref_seen"][n_colors - 1] > 0


# ---- 4. set counts: one non-empty set, several, and more than the kernels' LDS counters hold ---------------------------
@pytest.mark.parametrize("n_sets", [1, 2, 1024, 1025, 5000])
def test_set_counts(world, n_sets):
    s, ids, rows = world.upload(n_sets, 70, 4000 + n_sets)
    with s, s.screen() as scr:
        scr.add_reads(enc(world.reads), 1)
        A = check_arrays(scr, ids, rows, 70, world.results(world.reads), n_sets)
        assert A["n_hits"] > 3000 and sum(A["set_hits"]) == A["n_hits"] and sum(A["set_seen"]) == A["n_seen"]
        if n_sets == 5000:
            assert sum(A["set_hits"][1024:]) > 1000             # (ids beyond the LDS counters were hit)


def test_runs_that_never_end_and_runs_of_one(world):
    long_read = world.refs[0][:5000 + K - 1]
    # every column its own id, so consecutive windows (almost) never share one; then a single non-empty set for everything
    for name, ids in (("every window", np.arange(world.n) % 4999 + 1), ("never", np.ones(world.n, dtype=np.int64))):
        s, ids, rows = world.upload(5000 if name == "every window" else 2, 3, 77, ids)
        with s, s.screen() as scr:
            scr.add_reads([long_read.encode()] + enc(world.reads[:20]))
            A = check_arrays(scr, ids, rows, 3, world.results([long_read] + world.reads[:20]), name)
            assert A["n_hits"] >= 5000
            if name == "never":
                assert A["set_hits"][1] == A["n_hits"]


# ---- 5. window counts at the edges of a wave iteration, and one long read ------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 127, 128, 129, 5000])
def test_window_counts(world, m):
    read = world.refs[2][100:100 + m + K - 1]
    for strands in (1, 2):
        with world.sets.screen() as scr:
            scr.add_reads([read.encode()], strands)
            S = world.want([read], strands)
            assert S.n_windows == strands * m and S.n_hits >= m
            check_real(scr, S, world, (m, strands))


# ---- 6. the bitmap's word edges: hits on columns 63, 64, 65 and on the last column ------------------------------------
def test_bitmap_word_edges(gpu):
    k = 4
    kmers = ["".join("ACGT"[(i >> (2 * j)) & 3] for j in range(k)) for i in range(4 ** k)]
    idx = tw.make_index(kmers, k)                               # all 256 4-mers: the root and 256 real columns
    labels = tw.labels_of(idx)
    n = idx.n_nodes
    assert n >= 257 and n % 64 != 0
    ids = np.arange(n) % 7
    table = np.arange(7, dtype=np.uint64).reshape(7, 1)
    with capi.ColorSets.from_arrays(idx, 3, ids.astype(np.uint32), table) as s, s.screen() as scr:
        ids = s.copy()[0]
        cols = [63, 64, 65, n - 1]
        assert all("$" not in labels[v] for v in cols)
        reads = [labels[v].encode() for v in cols]
        scr.add_reads(reads)
        assert [r.tolist() for r in idx.search_reads(reads)] == [[v] for v in cols]
        seen = scr.seen()
        want = [0] * ((n + 63) // 64)
        for v in cols:
            want[v >> 6] |= 1 << (v & 63)
        assert want[0] == 1 << 63 and want[1] == 3 and want[-1] == 1 << ((n - 1) & 63)
        assert [int(x) for x in seen] == want
        assert scr.info()["n_seen"] == 4
        check_arrays(scr, ids, pw.rows_ints(table), 3, np.array(cols), "edges")
        scr.add_reads(reads + [b"AAAAAAAA"], 2)                  # again, and the other strand: bits stay, more appear
        res = np.concatenate([np.array(cols), idx.search(*capi.concat_reads(reads + [b"AAAAAAAA"] + [sb.revcomp(r.decode()).encode() for r in reads + [b"AAAAAAAA"]]))[0]])
        check_arrays(scr, ids, pw.rows_ints(table), 3, res, "edges twice")
    idx.close()


# ---- 7. every hit on one column and one set -----------------------------------------------------------------------------
def test_a_homopolymer(gpu):
    k = 9
    w = Small(["A" * 12 + "CGTACGTTGCA", "CCCCCCCCCCCGT"], [], k)
    read = "A" * (5000 + k - 1)
    with w.sets.screen() as scr:
        scr.add_reads([read.encode()])
        S = sb.Screen(w.kmers, w.cs, k, [read])
        assert (S.n_windows, S.n_hits, S.n_seen) == (5000, 5000, 1)
        check_real(scr, S, w, "A^L")
        assert sorted(scr.sets()[2].tolist())[-2:] == [0, 5000]
        scr.add_reads([read.encode()], 2)                         # T^L misses
        info = scr.info()
        assert (info["n_windows"], info["n_hits"], info["n_seen"]) == (15000, 10000, 1)
    w.close()


# ---- 8. batches without a hit, without a read, without a window -------------------------------------------------------------
def test_empty_batches(world, truth):
    with world.sets.screen() as scr:
        zero = state(scr)
        assert zero[0]["n_windows"] == 0 and not any(zero[1][1]) and not any(zero[1][2]) and not any(zero[3])
        assert zero[1][0] == world.sets.set_sizes().tolist()      # (the k-mers are there before any read)
        scr.add(np.zeros(0, np.uint8), np.zeros(1, np.int64))    # no read
        scr.add_reads([b"ACGT", b"", b"ACGTACGTACGTAC"])         # no window
        assert state(scr) == zero
        miss = [b"N" * 40, b"acgtacgtacgtacgtacgtacgt", bytes(range(1, 60))]
        scr.add_reads(miss, 2)                                    # windows, no hit
        st = state(scr)
        assert st[0]["n_windows"] == 2 * sum(len(r) - K + 1 for r in miss) and st[0]["n_hits"] == 0 and st[0]["n_seen"] == 0
        assert st[1:] == zero[1:]
        scr.add_reads(enc(world.reads))
        assert scr.info()["n_windows"] == st[0]["n_windows"] + truth[1].n_windows
        assert [v.tolist() for v in scr.colors()] == [truth[1].ref_kmers, truth[1].ref_seen, truth[1].ref_hits]


# ---- 9. the state does not depend on batch boundaries or chunking; reset; queries between adds ------------------------------
def test_batch_boundaries_chunking_reset_and_repeated_queries(world, truth):
    reads = enc(world.reads)
    with world.sets.screen() as scr:
        scr.add_reads(reads, 2)
        whole = state(scr)
        assert state(scr) == whole                                # twice: the queries leave the object as it is
        for parts in (2, 7):
            scr.reset()
            assert scr.info()["n_windows"] == 0 and not scr.seen().any()
            cut = [len(reads) * i // parts for i in range(parts + 1)]
            for a, b in zip(cut, cut[1:]):
                scr.add_reads(reads[a:b], 2)
                scr.sets(), scr.colors()                          # between adds
            assert state(scr) == whole, parts
        scr.reset()
        with tw.tuning("screen_chunk_bases", 1, 0):              # every read is its own chunk
            scr.add_reads(reads, 2)
        assert state(scr) == whole
        # the partial states are the brute force's, too
        scr.reset()
        scr.add_reads(reads[:50])
        check_real(scr, world.want(world.reads[:50]), world, "first 50")
        scr.add_reads(reads[50:])
        check_real(scr, truth[1], world, "all")


# ---- 10. the device entry point on a stream of the caller's, guard bytes around the workspace --------------------------------
def test_add_dev_on_a_stream_with_guards(world, truth):
    import torch
    dev = torch.device("cuda", 0)
    bases, off = capi.concat_reads(enc(world.reads))
    lead = 37                                                     # d_read_off[0] != 0: bases nobody asks about in front
    shifted = np.concatenate([np.frombuffer(b"ACGTN" * 8, dtype=np.uint8)[:lead], bases])
    tb, to = torch.from_numpy(shifted).to(dev), torch.from_numpy(off + lead).to(dev)
    T, n = len(shifted), len(world.reads)
    for strands in (1, 2):
        need = capi.screen_workspace_bytes(T, n, strands)
        assert need >= capi.search_workspace_bytes(T) and need % 256 == 0
        buf = torch.full((need + 2 * GUARD,), PAT, dtype=torch.uint8, device=dev)
        ws = buf.data_ptr() + GUARD
        assert ws % 16 == 0
        st = torch.cuda.Stream(dev)
        with world.sets.screen() as scr:
            torch.cuda.synchronize(dev)
            scr.add_dev(tb.data_ptr(), T, to.data_ptr(), n, ws, need, strands, st.cuda_stream)
            st.synchronize()
            assert world.idx.workspace_status(ws, st.cuda_stream) == 0
            h = buf.cpu().numpy()
            assert (h[:GUARD] == PAT).all() and (h[-GUARD:] == PAT).all()
            check_real(scr, truth[strands], world, ("dev", strands))
            tw.refused(lambda: scr.add_dev(tb.data_ptr(), T, to.data_ptr(), n, ws, need - 1, strands, st.cuda_stream), "workspace")
            check_real(scr, truth[strands], world, ("dev after a refusal", strands))
    sizes = [capi.screen_workspace_bytes(b, r, s) for s in (1, 2) for b in (0, 1, 1000, 10**6, 10**9) for r in (0, 1, 1000, 10**6)]
    assert all(x > 0 for x in sizes)
    for s in (1, 2):
        for r in (0, 1, 1000, 10**6):
            col = [capi.screen_workspace_bytes(b, r, s) for b in (0, 1, 1000, 10**6, 10**9)]
            assert col == sorted(col)
        for b in (0, 1, 1000, 10**6, 10**9):
            row = [capi.screen_workspace_bytes(b, r, s) for r in (0, 1, 1000, 10**6)]
            assert row == sorted(row)


# ---- 11. two host threads on one object ------------------------------------------------------------------------------------
def test_two_threads_add_disjoint_halves(world, truth):
    reads = enc(world.reads)
    half = len(reads) // 2
    with world.sets.screen() as scr:
        errors = []

        def work(part):
            try:
                for _ in range(3):
                    scr.add_reads(part, 2)
            except Exception as e:                                # noqa: BLE001
                errors.append(e)

        th = [threading.Thread(target=work, args=(p,)) for p in (reads[:half], reads[half:])]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors, errors
        both = state(scr)
        scr.reset()
        for _ in range(3):
            scr.add_reads(reads, 2)
        assert state(scr) == both
        S = truth[2]
        assert both[0]["n_hits"] == 3 * S.n_hits and both[0]["n_seen"] == S.n_seen
        assert both[2] == [S.ref_kmers, S.ref_seen, [3 * x for x in S.ref_hits]]


# ---- 12. every image level -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 2])
def test_image_levels(world, truth, level):
    with tw.tuning("image_level", level, 0):
        low = tw.make_index(world.seqs, K)
    assert low.image_level >= level and low.n_nodes == world.n
    with capi.ColorSets.from_arrays(low, len(world.cs), world.ids, world.table) as s, s.screen() as scr:
        scr.add_reads(enc(world.reads), 2)
        check_real(scr, truth[2], world, level)
    low.close()


# ---- 13. an uploaded object with duplicate rows and another numbering ---------------------------------------------------------
def test_duplicate_rows_and_a_permuted_numbering(world, truth):
    rng = np.random.default_rng(5)
    n_sets = len(world.rows)
    perm = np.concatenate([[0], 1 + rng.permutation(n_sets - 1)])      # new id of old set t (set 0 stays the empty set)
    table = np.zeros((2 * n_sets - 1, 1), dtype=np.uint64)
    table[perm] = world.table
    table[n_sets:] = world.table[1:]                                    # a second copy of every row but 0 ...
    ids = perm[world.ids]
    twin = (rng.random(world.n) < 0.5) & (world.ids != 0)               # ... which half of the columns use
    ids = np.where(twin, n_sets + world.ids - 1, ids)
    with capi.ColorSets.from_arrays(world.idx, len(world.cs), ids.astype(np.uint32), table) as s, s.screen() as scr:
        scr.add_reads(enc(world.reads), 2)
        S = truth[2]
        assert [v.tolist() for v in scr.colors()] == [S.ref_kmers, S.ref_seen, S.ref_hits]       # the canonical object's
        A = check_arrays(scr, s.copy()[0], pw.rows_ints(table), len(world.cs), world.results(world.reads, 2), "twins")
        assert any(A["set_hits"][n_sets:]) and (A["n_hits"], A["n_seen"]) == (S.n_hits, S.n_seen)
        assert [int(x) for x in scr.seen()] == S.seen_bitmap(world.labels)


# ---- 14. cross-checks with the calls that were there before -------------------------------------------------------------------
def test_cross_checks_with_the_existing_calls(world):
    reads = enc(world.reads)
    for strands in (1, 2):
        with world.sets.screen() as scr:
            scr.add_reads(reads, strands)
            info = scr.info()
            set_kmers, set_seen, set_hits = scr.sets()
            ref_kmers, ref_seen, ref_hits = scr.colors()
            both = reads + ([sb.revcomp(r.decode("latin-1")).encode("latin-1") for r in reads] if strands == 2 else [])
            prof = world.idx.read_hits_reads(both)               # columns: n_kmers, n_found, covered_bases, longest_run
            assert info["n_hits"] == int(prof[:, 1].sum()) and info["n_windows"] == int(prof[:, 0].sum())
            assert set_kmers.tolist() == world.sets.set_sizes().tolist()
            assert ref_kmers.tolist() == np.diag(world.sets.shared_kmers()).tolist()
            assert ref_seen.tolist() == np.diag(world.sets.shared_kmers(set_seen)).tolist()
            assert ref_hits.tolist() == np.diag(world.sets.shared_kmers(set_hits)).tolist()
            cols = world.results(world.reads, strands)
            want = np.zeros((world.n + 63) // 64 * 64, dtype=np.uint8)
            want[cols[cols >= 0]] = 1
            assert np.array_equal(np.packbits(want, bitorder="little").view(np.uint64), scr.seen())
            assert int(want.sum()) == info["n_seen"] and int((cols >= 0).sum()) == info["n_hits"]


# ---- 15. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_usable(world, truth):
    import torch
    L, C = capi.lib(), capi.C
    reads = enc(world.reads)
    bases, off = capi.concat_reads(reads)
    n = len(reads)
    with world.sets.screen() as scr:
        scr.add_reads(reads)
        h = scr.handle
        host = (bases.ctypes.data, off.ctypes.data)
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_create(None, C.byref(C.c_void_p()))), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_create(world.sets.handle, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_add_batch(None, *host, n, 1)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_add_batch(h, bases.ctypes.data, None, n, 1)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_add_batch(h, None, off.ctypes.data, n, 1)), "NULL")
        for strands in (0, 3, -1):
            tw.refused(lambda: capi._check(L.sbwtgpu_screen_add_batch(h, *host, n, strands)), "strands")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_add_batch(h, *host, -1, 1)), "n_reads")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_add_batch(h, *host, 1 << 31, 1)), "2^31 reads")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_info(None, None, None, None, None, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_sets(None, None, None, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_colors(None, None, None, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_seen_copy(h, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_seen_copy(None, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_seen_dev(h, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_reset(None)), "NULL")
        L.sbwtgpu_screen_destroy(None)
        # the device entry point: NULL pointers, strands, n_reads, the workspace
        dev = torch.device("cuda", 0)
        d_bases, d_off = torch.from_numpy(bases.copy()).to(dev), torch.from_numpy(off.copy()).to(dev)
        need = capi.screen_workspace_bytes(len(bases), n, 2)
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        good = (d_bases.data_ptr(), len(bases), d_off.data_ptr(), n)
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_add_dev(None, *good, 1, ws.data_ptr(), need, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_add_dev(h, None, len(bases), d_off.data_ptr(), n, 1, ws.data_ptr(), need, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_add_dev(h, d_bases.data_ptr(), len(bases), None, n, 1, ws.data_ptr(), need, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_add_dev(h, *good, 1, None, need, None)), "workspace")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_add_dev(h, *good, 2, ws.data_ptr(), capi.screen_workspace_bytes(len(bases), n, 1), None)),
                   "workspace")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_add_dev(h, *good, 3, ws.data_ptr(), need, None)), "strands")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_add_dev(h, d_bases.data_ptr(), len(bases), d_off.data_ptr(), -1, 1, ws.data_ptr(), need, None)),
                   "n_reads")
        tw.refused(lambda: capi._check(L.sbwtgpu_screen_add_dev(h, d_bases.data_ptr(), -1, d_off.data_ptr(), n, 1, ws.data_ptr(), need, None)),
                   "negative")
        torch.cuda.synchronize(dev)
        # any output may be NULL
        nh = C.c_int64(-1)
        capi._check(L.sbwtgpu_screen_info(h, None, C.byref(nh), None, None, None))
        assert nh.value == truth[1].n_hits
        capi._check(L.sbwtgpu_screen_sets(h, None, None, None))
        only = np.zeros(len(world.cs), dtype=np.int64)
        capi._check(L.sbwtgpu_screen_colors(h, None, only.ctypes.data, None))
        assert only.tolist() == truth[1].ref_seen
        p = C.c_void_p()
        capi._check(L.sbwtgpu_screen_seen_dev(h, C.byref(p)))
        assert p.value and scr.seen_dev() == p.value
        check_real(scr, truth[1], world, "after the refusals")    # nothing of it changed the object
    # what the colour-set queries refuse for the object's index: an object that outlived a change of its index is not
    # constructible from Python; a rank-only index refuses the colour sets themselves
    bits = np.random.default_rng(1).integers(0, 2**64, size=4, dtype=np.uint64)
    ro = capi.Index.create(bits, bits, bits, bits, None, 256, 3)
    tw.refused(lambda: capi.ColorSetsBuilder.create(ro, 3), "only rank()")
    ro.close()
    # a read of 2^31 bases or more, from the offsets alone
    with world.sets.screen() as scr:
        big = np.array([0, 1 << 31], dtype=np.int64)
        with pytest.raises(capi.SbwtGpuError) as ei:
            capi._check(L.sbwtgpu_screen_add_batch(scr.handle, bases.ctypes.data, big.ctypes.data, 1, 1))
        assert ei.value.code == capi.ERR_READ_TOO_LONG
        assert scr.info()["n_windows"] == 0


# ---- 16. the CLI ----------------------------------------------------------------------------------------------------------
def test_cli_screen(gpu, tmp_path):
    d = str(tmp_path)
    k = 11
    rng = random.Random(16)
    core = pw.rand_seq(rng, 300)
    refs = [core[:200] + pw.rand_seq(rng, 60), core[100:] + pw.rand_seq(rng, 30), pw.rand_seq(rng, 150), core]
    extra = pw.rand_seq(rng, 80)                                 # k-mers of the index that no reference colours
    SBWT = tw.SBWT
    with open(d + "/all.fna", "w") as fh, open(d + "/refs.txt", "w") as lst:
        for i, s in enumerate(refs + [extra]):
            fh.write(">s%d\n%s\n" % (i, s))
        for i, s in enumerate(refs):
            with open("%s/ref%d.fna" % (d, i), "w") as one:
                one.write(">r\n%s\n" % s)
            lst.write("%s/ref%d.fna\n" % (d, i))
    reads = []
    for i in range(40):
        src = (refs + [extra])[i % 5]
        a = rng.randrange(0, len(src) - 20)
        r = mutate(rng, src[a:a + rng.randint(8, 90)], 0.03, "ACGTN" if i % 6 == 0 else "ACGT")
        reads.append(sb.revcomp(r) if i % 3 == 2 else r)
    fastq = "".join("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)) for i, r in enumerate(reads))
    with open(d + "/reads.fastq", "w") as fh:
        fh.write(fastq)
    with gzip.open(d + "/reads.fastq.gz", "wt") as fh:
        fh.write(fastq)
    p = tw.run([SBWT, "build", "-i", d + "/all.fna", "-o", d + "/i.sbwt", "-k", str(k), "--temp-dir", d])
    assert p.returncode == 0, p.stderr.decode()
    for flag, name in (("--compress", "sets"), ("--wide", "wide"), (None, "narrow")):
        p = tw.run([SBWT, "build-colors"] + ([flag] if flag else []) + ["-i", d + "/i.sbwt", "-r", d + "/refs.txt", "-o", "%s/%s.colors" % (d, name)])
        assert p.returncode == 0, p.stderr.decode()
    kmers = set()
    for s in refs + [extra]:
        kmers |= set(pb.windows(s, k))
    cs = [set() for _ in refs]
    for c, s in enumerate(refs):
        pb.add(cs, kmers, k, c, [s])
    for strands in (1, 2):
        S = sb.Screen(kmers, cs, k, reads, strands)
        assert S.n_hits > 100 and S.row_hits.get(0, 0) > 0
        for name, query in (("sets", "reads.fastq"), ("wide", "reads.fastq.gz"), ("narrow", "reads.fastq"), ("sets", "reads.fastq.gz")):
            out, sets_out = "%s/%s.%d.tsv" % (d, name, strands), "%s/%s.%d.sets.tsv" % (d, name, strands)
            cmd = [SBWT, "screen", "-i", d + "/i.sbwt", "-c", "%s/%s.colors" % (d, name), "-q", d + "/" + query, "-o", out,
                   "--sets-out", sets_out, "--batch-bases", "300"] + (["--both-strands"] if strands == 2 else [])
            p = tw.run(cmd)
            assert p.returncode == 0, p.stderr.decode()
            assert open(out, "rb").read() == sb.screen_tsv(S), (name, query, strands)
            # the sets file: the numbering is the canonical one (by first column), the brute force knows the sets by their rows
            lines = [[int(x) for x in ln.split("\t")] for ln in open(sets_out).read().splitlines()]
            assert [ln[0] for ln in lines] == list(range(len(lines))) and len(lines) == 1 + len(set(S.row.values()) - {0})
            assert lines[0][1] >= S.row_kmers.get(0, 0) and lines[0][2:] == [S.row_seen.get(0, 0), S.row_hits.get(0, 0)]
            rows = sorted(set(S.row.values()) - {0})
            assert sorted(ln[1:] for ln in lines[1:]) == sorted([S.row_kmers[r], S.row_seen.get(r, 0), S.row_hits.get(r, 0)] for r in rows)
            assert sum(ln[3] for ln in lines) == S.n_hits and sum(ln[2] for ln in lines) == S.n_seen
    p = tw.run([SBWT, "screen", "-i", d + "/i.sbwt", "-c", d + "/sets.colors", "-q", d + "/reads.fastq", "-o", d + "/plain.tsv"])
    assert p.returncode == 0 and open(d + "/plain.tsv", "rb").read() == sb.screen_tsv(sb.Screen(kmers, cs, k, reads, 1))
    p = tw.run([SBWT], 60)
    assert b"screen" in p.stderr
