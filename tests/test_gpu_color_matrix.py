"""GPU: sbwtgpu_colorsets_set_sizes and sbwtgpu_colorsets_shared_kmers (sbwt_colormatrix.hip: the colours' weighted Gram matrix)
against the definition (tests/shared_kmers_brute.py).  One random index of some 25 000 columns carries real colour sets of five
references; every other object is uploaded onto it with ColorSets.from_arrays, so that n_sets and n_colors are free.  Every
case runs on both kernels (the plain one and the matrix cores, "gram_mfma_min_sets"), and every comparison is exact."""
import random

import numpy as np
import pytest

import pseudoalign_brute as pb
import pseudoalign_wide as pw
import shared_kmers_brute as sk
import test_gpu_pseudoalign_wide as tw          # its helpers: make_index, labels_of, refused, run, tuning, SBWT
from sbwt_amd import capi

pytestmark = pytest.mark.gpu

K = 15
MIN_SETS_DEFAULT, FLUSH_DEFAULT, FLUSH_MAX = 512, 65536, 16909320
ROUTES = (("plain", 1 << 40), ("mfma", 0))
W_MAX = 2**31 - 1


class World:
    def __init__(self):
        rng = random.Random(2024)
        base = pw.rand_seq(rng, 10000)
        self.refs = []
        for _ in range(5):                                   # strains: 3 % substitutions and a stretch of their own
            s = "".join(rng.choice("ACGT") if rng.random() < 0.03 else c for c in base)
            self.refs.append(s + pw.rand_seq(rng, 800))
        self.refs[4] = self.refs[4][:3000]                   # ... one of them much shorter
        self.idx = tw.make_index(self.refs, K)
        self.n = self.idx.n_nodes
        self.labels = tw.labels_of(self.idx)
        self.dummy = np.array(["$" in lab for lab in self.labels])
        self.kmers = {lab for lab in self.labels if "$" not in lab}
        self.cs = [set() for _ in self.refs]
        with capi.ColorSetsBuilder.create(self.idx, len(self.refs)) as b:
            for c, s in enumerate(self.refs):
                b.add_reads(c, [s.encode()])
                pb.add(self.cs, self.kmers, K, c, [s])
            self.sets = b.finish()
        self.G = np.array(sk.shared_of_kmers(self.cs, self.kmers), dtype=np.int64)

    def upload(self, n_sets, n_colors, seed, ids=None):
        """A random object: rows of density 1/4 (every row but 0 non-zero), ids uniform over the sets unless given.  Returns the
        object, its ids as the device holds them (dummy columns 0) and the table."""
        rng = np.random.default_rng(seed)
        words = pw.n_words(n_colors)
        table = rng.integers(0, 2**64, size=(n_sets, words), dtype=np.uint64) & rng.integers(0, 2**64, size=(n_sets, words), dtype=np.uint64)
        if n_colors % 64:
            table[:, -1] &= np.uint64((1 << (n_colors % 64)) - 1)
        one = rng.integers(0, n_colors, size=n_sets)
        table[np.arange(n_sets), one >> 6] |= np.uint64(1) << (one & 63).astype(np.uint64)
        table[0] = 0
        if ids is None:
            ids = rng.integers(0, n_sets, size=self.n)
        s = capi.ColorSets.from_arrays(self.idx, n_colors, np.asarray(ids, dtype=np.uint32), table)
        return s, s.copy()[0], table


@pytest.fixture(scope="module")
def world(gpu):
    w = World()
    assert 20000 <= w.n <= 30000 and w.dummy.any()
    yield w
    w.sets.close()
    w.idx.close()


def on_both_routes(s, want, weights=None, label=None):
    """shared_kmers on the plain kernel and on the matrix cores: both equal `want`, byte for byte"""
    for name, min_sets in ROUTES:
        with tw.tuning("gram_mfma_min_sets", min_sets, MIN_SETS_DEFAULT):
            got = s.shared_kmers(weights)
        assert got.dtype == np.int64 and got.shape == want.shape, (label, name)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (label, name, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))
        info = s.shared_info
        assert info["used_mfma"] == (name == "mfma") and (info["n_colors"], info["words"]) == (s.n_colors, s.words), (label, name, info)
        w = np.array(weights if weights is not None else s.set_sizes())[1:]
        assert info["n_sets_used"] == int((w > 0).sum()), (label, name, info)
        top = int(w.max()) if len(w) else 0
        assert info["n_limbs"] == (top.bit_length() + 6) // 7, (label, name, info)
        assert len(info["pass_ms"]) == 4 and all(x >= 0 for x in info["pass_ms"].values()), (label, name)


def random_weights(n_sets, seed):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 2**31, size=n_sets, dtype=np.int64) >> rng.integers(0, 31, size=n_sets)      # every magnitude
    w[rng.integers(0, n_sets, size=max(1, n_sets // 8))] = 0
    return w


# ---- 1. colour counts: the edges of a word, of a 16- and a 64-wide tile, and of W -----------------------------------------
@pytest.mark.parametrize("n_colors", [1, 2, 15, 16, 17, 63, 64, 65, 100, 129, 4096])
def test_colour_counts(world, n_colors):
    n_sets = 300 if n_colors == 4096 else 333
    s, ids, table = world.upload(n_sets, n_colors, 1000 + n_colors)
    with s:
        on_both_routes(s, sk.shared_np(ids, table, n_colors), None, n_colors)
        w = random_weights(n_sets, n_colors)
        on_both_routes(s, sk.shared_np(ids, table, n_colors, w), w, (n_colors, "weights"))


# ---- 2. set counts: the edges of a K block of 64 sets, and several blocks -------------------------------------------------
@pytest.mark.parametrize("n_sets", [1, 2, 63, 64, 65, 129, 1000, 5000])
def test_set_counts(world, n_sets):
    n_colors = 70                                            # two tiles: the tile (0, 1) is not symmetric
    s, ids, table = world.upload(n_sets, n_colors, 2000 + n_sets)
    with s:
        want = sk.shared_np(ids, table, n_colors)
        if n_sets == 1:
            assert not want.any()
        else:
            assert (want != want.T).sum() == 0 and (n_sets < 63 or want[:64, 64:].any())
        on_both_routes(s, want, None, n_sets)
        w = random_weights(n_sets, n_sets)
        w[0] = -5                                            # (w[0] is ignored, whatever it is)
        want = sk.shared_np(ids, table, n_colors, np.where(np.arange(n_sets) == 0, 0, w))
        for name, min_sets in ROUTES:
            with tw.tuning("gram_mfma_min_sets", min_sets, MIN_SETS_DEFAULT):
                assert np.array_equal(s.shared_kmers(w), want), (n_sets, name)


# ---- 3. real sets from references -----------------------------------------------------------------------------------------
def test_real_sets_against_the_kmer_strings(world):
    s = world.sets
    ids, table = s.copy()
    assert np.array_equal(sk.shared_np(ids, table, s.n_colors), world.G)
    assert sk.shared(ids.tolist(), pw.rows_ints(table), s.n_colors) == world.G.tolist()
    on_both_routes(s, world.G, None, "real")
    assert np.array_equal(world.G, world.G.T) and (np.diag(world.G) == [len(x) for x in world.cs]).all()
    assert world.G[0, 1] > 0 and world.G[0, 1] < world.G[0, 0]
    with s.expand() as wide:
        assert np.array_equal(np.diag(world.G), np.asarray(wide.info()["per_color"])[:s.n_colors])
    sizes = s.set_sizes()
    assert sizes.dtype == np.int64 and sizes.tolist() == sk.set_sizes(ids.tolist(), s.n_sets)
    assert sizes.sum() == world.n and sizes[0] >= world.dummy.sum() and (sizes[1:] > 0).all()


# ---- 4. custom weights: every limb of the arithmetic ----------------------------------------------------------------------
def test_custom_weights(world):
    n_sets, n_colors = 700, 100
    s, ids, table = world.upload(n_sets, n_colors, 4)
    with s:
        w = np.full(n_sets, W_MAX, dtype=np.int64)
        on_both_routes(s, sk.shared_np(ids, table, n_colors, w), w, "all maximal")
        edges = [128**l + d for l in (1, 2, 3, 4) for d in (-1, 0, 1)]
        w = np.array([edges[t % len(edges)] for t in range(n_sets)], dtype=np.int64)
        on_both_routes(s, sk.shared_np(ids, table, n_colors, w), w, "limb edges")
        for e in edges:                                      # ... and each edge alone, so that no other weight covers for it
            w = np.full(n_sets, e, dtype=np.int64)
            on_both_routes(s, sk.shared_np(ids, table, n_colors, w), w, ("edge", e))
        w = np.zeros(n_sets, dtype=np.int64)
        on_both_routes(s, np.zeros((n_colors, n_colors), dtype=np.int64), w, "all zero")


def test_a_real_size_reaches_the_third_limb(world):
    n_sets, n_colors = 600, 65
    rng = np.random.default_rng(5)
    ids = rng.integers(0, n_sets, size=world.n)
    real = np.flatnonzero(~world.dummy)
    ids[real[:17000]] = 3
    s, ids, table = world.upload(n_sets, n_colors, 5, ids)
    with s:
        sizes = s.set_sizes()
        assert sizes[3] > 16384 and sizes.tolist() == np.bincount(ids, minlength=n_sets).tolist()
        on_both_routes(s, sk.shared_np(ids, table, n_colors), None, "third limb")
        assert s.shared_info["n_limbs"] == 3


# ---- 5. flushes -----------------------------------------------------------------------------------------------------------
def test_flushes(world):
    n_sets, n_colors = 1000, 100
    s, ids, table = world.upload(n_sets, n_colors, 6)
    with s:
        w = np.full(n_sets, W_MAX, dtype=np.int64)
        want = sk.shared_np(ids, table, n_colors, w)
        on_both_routes(s, want, w, "default interval")
        for v in (64, 200, FLUSH_MAX):
            with tw.tuning("gram_flush_sets", v, FLUSH_DEFAULT):
                on_both_routes(s, want, w, ("flush", v))
                on_both_routes(s, sk.shared_np(ids, table, n_colors), None, ("flush, sizes", v))


# ---- 6. form independence -------------------------------------------------------------------------------------------------
def test_form_independence(world):
    s = world.sets
    ids, table = s.copy()
    rng = np.random.default_rng(7)
    n0 = s.n_sets
    perm = np.concatenate([[0], 1 + rng.permutation(n0 - 1)])            # old id -> new id
    t2 = np.zeros((2 * n0 + 3, s.words), dtype=np.uint64)
    t2[perm] = table
    t2[n0:2 * n0] = t2[:n0]                                              # duplicates: row n0 + i = row i (row n0 is unused: a zero row is refused)
    t2[n0] = t2[1]
    t2[2 * n0:] = np.uint64(0b10101)                                     # rows that no column carries
    ids2 = perm[ids].astype(np.uint32)
    dup = rng.random(world.n) < 0.5
    ids2 = np.where(dup & (ids2 != 0), ids2 + n0, ids2).astype(np.uint32)
    with capi.ColorSets.from_arrays(world.idx, s.n_colors, ids2, t2) as up:
        assert up.n_sets == 2 * n0 + 3
        sizes = up.set_sizes()
        assert sizes.sum() == world.n and not sizes[2 * n0:].any() and sizes[n0] == 0
        assert sizes.tolist() == np.bincount(up.copy()[0], minlength=up.n_sets).tolist()
        on_both_routes(up, world.G, None, "uploaded")
        with capi.ColorSets.merge(world.idx, up) as canon:
            got = canon.copy()
            assert got[0].tobytes() == ids.tobytes() and got[1].tobytes() == table.tobytes()
            on_both_routes(canon, world.G, None, "canonicalised")


# ---- 7. the device entry point ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_dev_call(world, route):
    import torch
    dev = torch.device("cuda", 0)
    n_sets, n_colors = 900, 130
    s, ids, table = world.upload(n_sets, n_colors, 8)
    w = random_weights(n_sets, 8)
    with s, tw.tuning("gram_mfma_min_sets", route[1], MIN_SETS_DEFAULT):
        need = s.shared_workspace_bytes()
        assert need > 0
        st = torch.cuda.Stream(dev)
        dw = torch.from_numpy(w).to(dev)
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        for weights, d_w in ((w, dw.data_ptr()), (None, 0)):
            host = s.shared_kmers(weights)
            assert np.array_equal(host, sk.shared_np(ids, table, n_colors, weights))
            runs = []
            for _ in range(2):
                out = torch.full((n_colors, n_colors), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
                torch.cuda.synchronize()
                s.shared_kmers_dev(d_w, out.data_ptr(), ws.data_ptr(), need, st.cuda_stream)
                st.synchronize()
                assert ws[:8].cpu().numpy().view(np.int64)[0] == -1
                runs.append(out.cpu().numpy())
            assert runs[0].tobytes() == runs[1].tobytes() == host.tobytes(), (route[0], weights is None)
        # an out-of-range weight cannot come back through the return value: the status word names the smallest such set
        bad = w.copy()
        bad[[40, 17]] = (-1, 2**31)
        out = torch.zeros((n_colors, n_colors), dtype=torch.int64, device=dev)
        s.shared_kmers_dev(torch.from_numpy(bad).to(dev).data_ptr(), out.data_ptr(), ws.data_ptr(), need, st.cuda_stream)
        st.synchronize()
        assert ws[:8].cpu().numpy().view(np.int64)[0] == 17
        tw.refused(lambda: s.shared_kmers_dev(dw.data_ptr(), out.data_ptr(), ws.data_ptr(), need - 1, st.cuda_stream), "workspace",
                   str(need), str(need - 1))


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_usable(world):
    n_sets, n_colors = 600, 20
    s, ids, table = world.upload(n_sets, n_colors, 9)
    L = capi.lib()
    out = np.zeros((n_colors, n_colors), dtype=np.int64)
    with s:
        want = sk.shared_np(ids, table, n_colors)
        for name, min_sets in ROUTES:
            with tw.tuning("gram_mfma_min_sets", min_sets, MIN_SETS_DEFAULT):
                w = np.ones(n_sets, dtype=np.int64)
                w[[9, 300]] = -1
                tw.refused(lambda: s.shared_kmers(w), "weight of set 9 is -1", "2^31 - 1")
                w[9] = 2**31
                tw.refused(lambda: s.shared_kmers(w), "weight of set 9 is 2147483648")
                w[[9, 300]] = W_MAX
                assert np.array_equal(s.shared_kmers(w), sk.shared_np(ids, table, n_colors, w)), name
                assert np.array_equal(s.shared_kmers(), want), name
        tw.refused(lambda: s.shared_kmers(np.ones(n_sets - 1, dtype=np.int64)), "weights of shape")
        for rc in (L.sbwtgpu_colorsets_shared_kmers(None, None, out.ctypes.data, None),
                   L.sbwtgpu_colorsets_shared_kmers(s.handle, None, None, None),
                   L.sbwtgpu_colorsets_set_sizes(None, out.ctypes.data),
                   L.sbwtgpu_colorsets_set_sizes(s.handle, None),
                   L.sbwtgpu_colorsets_shared_kmers_dev(None, None, 1 << 20, 1 << 20, 1 << 30, None),
                   L.sbwtgpu_colorsets_shared_kmers_dev(s.handle, None, None, 1 << 20, 1 << 30, None),
                   L.sbwtgpu_colorsets_shared_kmers_dev(s.handle, None, 1 << 20, None, 1 << 30, None)):
            assert rc == capi.ERR_INVALID_ARG and b"NULL" in L.sbwtgpu_last_error()
        assert L.sbwtgpu_colorsets_shared_workspace_bytes(None) == 0
        for v in (FLUSH_MAX + 1, 2**31, 2**40, 0, -1):
            tw.refused(lambda: capi.set_tuning("gram_flush_sets", v), "gram_flush_sets", "2^31")
        capi.set_tuning("gram_flush_sets", FLUSH_MAX)
        capi.set_tuning("gram_flush_sets", FLUSH_DEFAULT)
        on_both_routes(s, want, None, "after the refusals")


# ---- 9. the CLI -------------------------------------------------------------------------------------------------------------
def test_cli_color_matrix(gpu, tmp_path):
    d = str(tmp_path)
    k = 11
    rng = random.Random(10)
    core = pw.rand_seq(rng, 300)
    refs = [core[:200] + pw.rand_seq(rng, 60), core[100:] + pw.rand_seq(rng, 30), pw.rand_seq(rng, 150), core]
    extra = pw.rand_seq(rng, 80)                             # k-mers of the index that no reference colours
    SBWT = tw.SBWT
    with open(d + "/all.fna", "w") as fh, open(d + "/refs.txt", "w") as lst:
        for i, s in enumerate(refs + [extra]):
            fh.write(">s%d\n%s\n" % (i, s))
        for i, s in enumerate(refs):
            with open("%s/ref%d.fna" % (d, i), "w") as one:
                one.write(">r\n%s\n" % s)
            lst.write("%s/ref%d.fna\n" % (d, i))
        lst.write(d + "/none.fna\n")                         # a fifth reference without a k-mer: Jaccard denominators of 0
    with open(d + "/none.fna", "w") as one:
        one.write(">r\n%s\n" % pw.rand_seq(rng, 40))
    p = tw.run([SBWT, "build", "-i", d + "/all.fna", "-o", d + "/i.sbwt", "-k", str(k), "--temp-dir", d])
    assert p.returncode == 0, p.stderr.decode()
    for flag, name, magic in (("--compress", "sets", b"SBWTCOL3"), ("--wide", "wide", b"SBWTCOL2"), (None, "narrow", b"SBWTCOL1")):
        p = tw.run([SBWT, "build-colors"] + ([flag] if flag else []) + ["-i", d + "/i.sbwt", "-r", d + "/refs.txt", "-o", "%s/%s.colors" % (d, name)])
        assert p.returncode == 0 and open("%s/%s.colors" % (d, name), "rb").read(8) == magic, p.stderr.decode()
    kmers = set()
    for s in refs + [extra]:
        kmers |= set(pb.windows(s, k))
    cs = [set() for _ in range(5)]
    for c, s in enumerate(refs):
        pb.add(cs, kmers, k, c, [s])
    G = sk.shared_of_kmers(cs, kmers)
    assert G[4] == [0] * 5 and G[0][1] > 0 and G[0][2] == 0
    for jaccard in (False, True):
        want = sk.tsv(G, jaccard)
        for name in ("sets", "wide", "narrow"):
            out = "%s/%s.%d.tsv" % (d, name, jaccard)
            p = tw.run([SBWT, "color-matrix", "-i", d + "/i.sbwt", "-c", "%s/%s.colors" % (d, name), "-o", out] + (["--jaccard-ppm"] if jaccard else []))
            assert p.returncode == 0, p.stderr.decode()
            assert open(out, "rb").read() == want, (name, jaccard)
    # a colour file of another index is refused before anything runs
    p = tw.run([SBWT, "build", "-i", d + "/ref0.fna", "-o", d + "/other.sbwt", "-k", str(k), "--temp-dir", d])
    assert p.returncode == 0, p.stderr.decode()
    p = tw.run([SBWT, "color-matrix", "-i", d + "/other.sbwt", "-c", d + "/sets.colors", "-o", d + "/x.tsv"], 60)
    assert p.returncode != 0 and b"columns at k =" in p.stderr
    p = tw.run([SBWT], 60)
    assert b"color-matrix" in p.stderr
