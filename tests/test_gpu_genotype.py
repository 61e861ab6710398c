"""GPU: genotyping a read set at the bubbles (sbwtgpu_genotype_*) exactly against the brute-force
restatement of the definition (tests/genotype_brute.py): kmer_hits, the three scalars, the per-branch vectors, the calls and
the per-colour vectors, on the hand cases of tests/test_genotype_cpu.py, on planted SNPs at k = 2 ... 64 and on the
40 000-base case whose 698 bubbles spread the branch columns over many words of the bitmap; batches that put one position on
every lane of a wave and across its span; the independence of batch boundaries, chunking, threads and image layout; the
device entry point; colours up to 4096; the refusals; and the C++ CLI.  The helpers are those of tests/test_gpu_bubbles.py."""
import ctypes as C
import gzip
import threading

import numpy as np
import pytest

import bubbles_brute as bb
import genotype_brute as gb
import test_bubbles_cpu as hand
import test_gpu_bubbles as tb
from bruteforce import kmer_set, revcomp
from test_gpu_colored_unitigs import refused
from test_gpu_pseudoalign_wide import tuning
from test_gpu_unitigs import make_index
from sbwt_amd import capi

pytestmark = pytest.mark.gpu

SBWT = tb.SBWT
PARAMS = [(1_000_000, 1), (500_000, 0), (1_000_000, 3)]
GUARD, PAT = 4096, 0x5A


def enc(reads):
    return [r.encode() if isinstance(r, str) else r for r in reads]


class Dev:
    """The plain graph handle of an index, its bubbles (with the colours of `sets`) and a genotype object over them."""

    def __init__(self, idx, sets=None, keep_bubbles=True):
        self.idx = idx
        self.u = idx.unitig_graph_dev(links=True, column_map=True)
        self.b = self.u.bubbles(sets)
        self.rec = tb.as_tuples(self.b.records())
        self.g = self.u.genotype(idx, self.b)
        if not keep_bubbles:
            self.b.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.g.close()
        self.b.close()
        self.u.close()


def state(g):
    """Everything an object says of itself, as bytes and dicts: equal states are byte-identical"""
    off, hits = g.kmer_hits()
    return g.info(), off.tobytes(), hits.tobytes(), tuple(v.tobytes() for v in g.branches())


def check(g, G, label, inter=None, n_colors=0):
    """The object == the brute force, exactly: scalars, kmer_hits, branch vectors, calls and (inter given) colour vectors"""
    B = len(G.recs)
    assert g.info() == G.info(n_colors), label
    off, hits = g.kmer_hits()
    assert off.dtype == np.int64 and hits.dtype == np.uint64 and off.tolist() == G.branch_off, label
    bad = np.flatnonzero(hits != np.array(G.kmer_hits, dtype=np.uint64))
    assert len(bad) == 0, (label, bad[:5].tolist(), hits[bad[:5]].tolist(), [G.kmer_hits[i] for i in bad[:5]])
    got = g.branches()
    assert all(v.dtype == np.int64 and v.shape == (2 * B,) for v in got), label
    assert [v.tolist() for v in got] == list(G.branches()), label
    for ppm, depth in PARAMS:
        out = g.calls(ppm, depth)
        assert out[0].dtype == np.uint8 and out[0].tolist() == G.calls(ppm, depth), (label, ppm, depth)
        if inter is None:
            assert out[1:] == (None, None, None), label
        else:
            assert [v.tolist() for v in out[1:]] == list(G.refs(inter, n_colors, ppm, depth)), (label, ppm, depth)


def brute(seqs, k, rc):
    kmers = tb.index_kmers(seqs, k, rc)
    U, lo, lt, recs = bb.brute_bubbles(kmers, k)
    return kmers, U, lt, gb.Genotype(U, recs, k)


# ---- 1. the hand cases of the CPU file ----------------------------------------------------------------------------------------
G4, H4 = hand.G, hand.H
INS = G4[:7] + "TTA" + G4[7:]
CYC = [hand.circular("CATTGACCGTAGG", 4), hand.circular("CATTGACTGTAGG", 4)]
HAND = {
    "snp": ([G4, H4], [[G4], [H4], [G4, H4], ["GACCGT"], ["GACC"] * 65, [G4, "GACCGT"], [G4, "GACCGT", "CGTA"], ["CATTGAC", "GTAGGA"],
                       ["gaccgta", "GACNGTA", "GAC", "", "GACCgTA"], [revcomp(G4)], [revcomp(H4), G4]]),
    "insertion": ([G4, INS], [[G4], [INS], ["GACTTACG"], [G4, INS, INS]]),
    "cycle": (CYC, [[CYC[0]], [CYC[1], CYC[1]], CYC]),
    "no bubble": ([G4, H4, G4[:7] + "A" + G4[8:]], [[G4, H4]]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(gpu, name):
    seqs, read_sets = HAND[name]
    for rc in (False, True):
        _, idx = make_index(seqs, hand.K, rc)
        _, _, _, G = brute(seqs, hand.K, rc)
        with Dev(idx) as d:
            assert d.rec == G.recs, (name, rc)
            if name == "no bubble" and not rc:
                assert d.g.n_bubbles == 0 and d.g.n_branch_kmers == 0
            check(d.g, G, (name, rc, "fresh"))
            for reads in read_sets:
                for strands in (1, 2):
                    d.g.reset()
                    G.reset()
                    d.g.add_reads(enc(reads), strands)
                    check(d.g, G.add(reads, strands), (name, rc, reads, strands))


def test_hand_values(gpu):
    """The counters written out in tests/test_genotype_cpu.py, from the device"""
    _, idx = make_index([G4, H4], hand.K)
    with Dev(idx) as d:
        g = d.g
        assert g.info() == {"n_bubbles": 1, "n_branch_kmers": 8, "n_windows": 0, "n_hits": 0, "n_site_hits": 0, "n_colors": 0}
        g.add_reads([b"GACCGT"])
        assert g.kmer_hits()[1].tolist() == [1, 1, 1, 0, 0, 0, 0, 0] and g.kmer_hits()[0].tolist() == [0, 4, 8]
        assert [v.tolist() for v in g.branches()] == [[3, 0], [3, 0], [0, 0]]
        assert g.calls(1_000_000, 0)[0].tolist() == [0] and g.calls(750_000, 0)[0].tolist() == [1]
        assert g.calls(750_001, 0)[0].tolist() == [0] and g.calls(750_000, 1)[0].tolist() == [0]
        g.add_reads([G4.encode()])                               # 7 hits on a's four k-mers: one below depth 2
        assert g.calls(1_000_000, 2)[0].tolist() == [0]
        g.add_reads([b"CGTA"])
        assert [v.tolist() for v in g.branches()] == [[4, 0], [8, 0], [2, 0]]
        assert g.calls(1_000_000, 2)[0].tolist() == [1] and g.calls(1_000_000, 3)[0].tolist() == [0]
        assert g.calls(1_000_000, 2**62)[0].tolist() == [0]      # hits >= min_depth * n without the product
        assert g.info()["n_windows"] == 3 + 11 + 1 and g.info()["n_site_hits"] == 8
        g.reset()
        g.add_reads([b"GACC"] * 65)
        assert g.kmer_hits()[1].tolist() == [65, 0, 0, 0, 0, 0, 0, 0] and g.calls(250_000, 1)[0].tolist() == [1]


def test_hand_colours(gpu):
    """g = 0, h = 1, a copy of g = 2, a fragment of h's branch = 3: colour 3 is informative nowhere"""
    _, idx = make_index([G4, H4], hand.K)
    refs = [[G4], [H4], [G4], ["ACTGT"]]
    kmers, U, lt, G = brute([G4, H4], hand.K, False)
    inter = gb.inter_sets(bb.branch_colors(U, G.recs, hand.K, tb.brute_sets(kmers, hand.K, refs, 1)))
    assert inter == [(frozenset({0, 2}), frozenset({1}))]
    with tb.build_sets(idx, refs) as s, Dev(idx, s) as d:
        check(d.g, G, "no reads", inter, 4)
        d.g.add_reads([G4.encode()])
        check(d.g, G.add([G4]), "g", inter, 4)
        assert [v.tolist() for v in d.g.calls()[1:]] == [[1, 1, 1, 0], [1, 0, 1, 0], [1, 0, 1, 0]]
        d.g.add_reads([H4.encode()])
        check(d.g, G.add([H4]), "g and h", inter, 4)
        assert [v.tolist() for v in d.g.calls()[1:]] == [[1, 1, 1, 0], [1, 1, 1, 0], [0, 0, 0, 0]]


# ---- 2. planted SNPs, k = 2 ... 64 -----------------------------------------------------------------------------------------------
def planted_reads(g, h, k):
    """60-base tiles at step 7 over g alone, over h alone and over both; above k = 40 also tiles of k + 20 bases, which have
    windows where the 60-base ones have few or none"""
    sets = {"g": gb.tiles(g, 60, 7), "h": gb.tiles(h, 60, 7)}
    sets["both"] = sets["g"] + sets["h"]
    if k > 40:
        sets["long g"] = gb.tiles(g, k + 20, 7)
        sets["long both"] = sets["long g"] + gb.tiles(h, k + 20, 7)
    return sets


@pytest.mark.parametrize("k", [2, 3, 4, 5, 8, 15, 16, 31, 32, 33, 63, 64])
@pytest.mark.parametrize("rc", [False, True])
def test_planted_snps(gpu, k, rc):
    g, h, _ = bb.planted(k, 30 * k + 60, 5, 1000 + k)
    _, idx = make_index([g, h], k, rc)
    _, _, _, G = brute([g, h], k, rc)
    with Dev(idx) as d:
        assert d.rec == G.recs
        check(d.g, G, (k, rc, "fresh"))                          # (B = 0 at the smallest k: the empty outputs)
        for name, reads in planted_reads(g, h, k).items():
            strands = 2 if (rc and name != "h") else 1
            d.g.reset()
            G.reset()
            d.g.add_reads(enc(reads), strands)
            check(d.g, G.add(reads, strands), (k, rc, name))
            if k >= 15 and name in ("g", "long g") and (k <= 40 or name == "long g"):
                assert G.calls() and set(G.calls()) <= {1, 2}    # g carries a or b, by the variant base, never both


@pytest.fixture(scope="module")
def big(gpu):
    """k = 15, 40 000 bases, 700 planted SNPs: 698 bubbles, 2 x 698 x 15 branch columns among some 80 000"""
    k = 15
    g, h, _ = bb.planted(k, 40_000, 700, 6)
    kmers = kmer_set([g, h], k)
    U, lo, lt, recs = bb.brute_bubbles(kmers, k)
    assert len(recs) == 698
    _, idx = make_index([g, h], k)
    yield k, g, h, idx, U, recs
    idx.close()


def test_many_words_of_the_bitmap(big):
    k, g, h, idx, U, recs = big
    G = gb.Genotype(U, recs, k)
    with Dev(idx) as d:
        assert d.rec == recs and d.g.n_branch_kmers == 2 * 698 * 15
        for name, reads in planted_reads(g, h, k).items():
            d.g.reset()
            G.reset()
            d.g.add_reads(enc(reads))
            check(d.g, G.add(reads), ("big", name))
        assert G.calls().count(3) == 698                         # (both: every allele)


# ---- 3. wave and span edges -------------------------------------------------------------------------------------------------------
def test_equal_positions_in_one_iteration_and_across_a_span(big):
    k, g, h, idx, U, recs = big
    G = gb.Genotype(U, recs, k)
    a, b = U[recs[300][1]][3:3 + k], U[recs[300][2]][:k]        # a k-mer of each branch of one bubble
    miss = "ACGT" * k
    miss = next(miss[i:i + k] for i in range(4) if miss[i:i + k] not in G.where)
    with Dev(idx) as d:
        for n in (1, 63, 64, 65, 2047, 2048, 2049):
            for name, reads in (("one", [a] * n), ("mixed", [a, b, miss] * n)):
                d.g.reset()
                G.reset()
                d.g.add_reads(enc(reads))
                check(d.g, G.add(reads), (name, n))
                assert G.n_hits == G.n_site_hits == (n if name == "one" else 2 * n)
        long_read = h[100:100 + 5000 + k - 1]                    # one read of 5000 windows along h
        d.g.reset()
        G.reset()
        d.g.add_reads([long_read.encode()])
        check(d.g, G.add([long_read]), "one long read")
        assert G.n_windows == 5000 == G.n_hits and 0 < G.n_site_hits < 5000


# ---- 4. the state does not depend on how the reads arrive ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(gpu):
    """k = 15, 3000 bases, 40 SNPs and an insertion, both strands indexed; reads with mismatches, Ns and short ones"""
    k = 15
    g, h, _ = bb.planted(k, 3000, 40, 1)
    seqs = [g, h, g[:723] + "ACG" + g[723:1500]]
    rng = np.random.default_rng(3)
    reads = []
    for i in range(300):
        src = seqs[i % 3]
        p = int(rng.integers(0, len(src) - 80))
        r = list(src[p:p + int(rng.integers(10, 80))])
        if i % 7 == 0:
            r[len(r) // 2] = "N"
        if i % 11 == 0:
            r[0] = r[0].lower()
        r = "".join(r)
        reads.append(revcomp(r) if i % 3 == 1 else r)
    _, idx = make_index(seqs, k, True)
    kmers, U, lt, G = brute(seqs, k, True)
    G.add(reads, 2)
    assert G.n_site_hits > 500 and len(G.recs) > 80
    yield k, seqs, reads, idx, U, lt, G
    idx.close()


def test_batch_boundaries_chunking_reset_and_repeated_queries(small):
    k, seqs, reads, idx, U, lt, G = small
    r = enc(reads)
    with Dev(idx) as d:
        g = d.g
        g.add_reads(r, 2)
        check(g, G, "one batch")
        whole = state(g)
        assert state(g) == whole                                 # the queries leave the object as it is
        g.reset()
        assert g.info()["n_windows"] == 0 and not g.kmer_hits()[1].any()
        for a, b in ((0, 100), (100, 101), (101, 300)):          # three batches, queries between them
            g.add_reads(r[a:b], 2)
            g.branches(), g.calls()
        assert state(g) == whole
        g.reset()
        for x in r:                                              # read by read
            g.add_reads([x], 2)
        assert state(g) == whole
        g.reset()
        with tuning("genotype_chunk_bases", 1, 0):               # every read is its own chunk
            g.add_reads(r, 2)
        assert state(g) == whole
        g.reset()                                                # the same adds after a reset
        g.add_reads(r, 2)
        assert state(g) == whole


def test_two_threads_add_halves(small):
    k, seqs, reads, idx, U, lt, G = small
    r = enc(reads)
    with Dev(idx) as d:
        errors = []

        def work(part):
            try:
                for _ in range(3):
                    d.g.add_reads(part, 2)
            except Exception as e:                               # noqa: BLE001 (reported below, in the main thread)
                errors.append(e)

        th = [threading.Thread(target=work, args=(p,)) for p in (r[:150], r[150:])]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors, errors
        both = state(d.g)
        d.g.reset()
        for _ in range(3):
            d.g.add_reads(r, 2)
        assert state(d.g) == both
        assert d.g.kmer_hits()[1].tolist() == [3 * x for x in G.kmer_hits] and both[0]["n_hits"] == 3 * G.n_hits


@pytest.mark.parametrize("key,val,back", [("image_level", 1, 0), ("image_level", 2, 0), ("force_mega", 1, 0), ("big_path", 2, 1)])
def test_image_layouts(small, key, val, back):
    k, seqs, reads, idx, U, lt, G = small
    with tuning(key, val, back):
        _, other = make_index(seqs, k, True)
    with Dev(other) as d:
        d.g.add_reads(enc(reads), 2)
        check(d.g, G, (key, val))
    other.close()


def test_the_bubbles_may_go_before_the_first_add(small):
    k, seqs, reads, idx, U, lt, G = small
    with Dev(idx, keep_bubbles=False) as d:
        d.g.add_reads(enc(reads), 2)
        check(d.g, G, "bubbles destroyed")


# ---- 5. the device entry point on a stream of the caller's, guard bytes around the workspace --------------------------------------
def test_add_dev_on_a_stream_with_guards(small):
    import torch
    k, seqs, reads, idx, U, lt, G = small
    dev = torch.device("cuda", 0)
    bases, off = capi.concat_reads(enc(reads))
    lead = 37                                                    # d_read_off[0] != 0: bases nobody asks about in front
    shifted = np.concatenate([np.frombuffer(b"ACGTN" * 8, dtype=np.uint8)[:lead], bases])
    tbs, to = torch.from_numpy(shifted).to(dev), torch.from_numpy(off + lead).to(dev)
    T, n = len(shifted), len(reads)
    zero = torch.zeros(2, dtype=torch.int64, device=dev)
    G1 = gb.Genotype(U, G.recs, k).add(reads, 1)
    for strands, want in ((1, G1), (2, G)):
        need = capi.genotype_workspace_bytes(T, n, strands)
        assert need >= capi.search_workspace_bytes(T) and need % 256 == 0
        buf = torch.full((need + 2 * GUARD,), PAT, dtype=torch.uint8, device=dev)
        ws = buf.data_ptr() + GUARD
        assert ws % 16 == 0
        st = torch.cuda.Stream(dev)
        with Dev(idx) as d:
            torch.cuda.synchronize(dev)
            d.g.add_dev(tbs.data_ptr(), T, to.data_ptr(), n, ws, need, strands, st.cuda_stream)
            st.synchronize()
            assert idx.workspace_status(ws, st.cuda_stream) == 0
            hb = buf.cpu().numpy()
            assert (hb[:GUARD] == PAT).all() and (hb[-GUARD:] == PAT).all()
            check(d.g, want, ("dev", strands))
            refused(lambda: d.g.add_dev(tbs.data_ptr(), T, to.data_ptr(), n, ws, need - 1, strands, st.cuda_stream), "workspace")
            d.g.add_dev(tbs.data_ptr(), T, to.data_ptr(), 0, ws, need, strands, st.cuda_stream)      # the empty batch
            d.g.add_dev(0, 0, zero.data_ptr(), 1, ws, need, strands, st.cuda_stream)                 # one read, no base
            st.synchronize()
            check(d.g, want, ("dev after a refusal and two empty batches", strands))
    with Dev(idx) as d:                                          # the host entry: no read, reads without a window
        d.g.add_reads([], 2)
        d.g.add_reads([b"", b"ACGT"], 2)
        assert d.g.info()["n_windows"] == 0 and not d.g.kmer_hits()[1].any()


# ---- 6. colours ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def coloured(gpu):
    k = 15
    g, h, _ = bb.planted(k, 3000, 40, 2)
    _, idx = make_index([g, h], k, True)
    kmers, U, lt, G = brute([g, h], k, True)
    reads = gb.tiles(g, 60, 7) + gb.tiles(h[:1000], 60, 7) + [h[2000:2040]]   # g everywhere, h at a third of the sites
    G.add(reads, 2)
    assert len(set(G.calls())) >= 2
    yield k, g, h, idx, kmers, U, G, reads
    idx.close()


@pytest.mark.parametrize("n_colors", [3, 64, 65, 70, 4096])
def test_colour_vectors(coloured, n_colors):
    k, g, h, idx, kmers, U, G, reads = coloured
    refs = tb.snp_refs(g, h, k, n_colors)
    inter = gb.inter_sets(bb.branch_colors(U, G.recs, k, tb.brute_sets(kmers, k, refs, 2)))
    with tb.build_sets(idx, refs, True, n_colors) as s, Dev(idx, s, keep_bubbles=False) as d:
        assert d.g.n_colors == n_colors
        d.g.add_reads(enc(reads), 2)
        check(d.g, G, n_colors, inter, n_colors)
        sites, match, only = (v.tolist() for v in d.g.calls()[1:])
        assert sites[0] == sites[1] > 0 and only[0] > only[1] and all(o <= m <= s_ for o, m, s_ in zip(only, match, sites))
        if n_colors > 3:
            mid = n_colors // 2                                  # the copy of g follows g
            assert (sites[mid], match[mid], only[mid]) == (sites[0], match[0], only[0])
        # any output may be NULL
        one = np.full(n_colors, -1, dtype=np.int64)
        capi._check(capi.lib().sbwtgpu_genotype_calls(d.g.handle, 1_000_000, 1, None, None, one.ctypes.data, None))
        assert one.tolist() == match


def test_uploaded_object_with_duplicates_and_another_numbering(coloured):
    k, g, h, idx, kmers, U, G, reads = coloured
    refs = tb.snp_refs(g, h, k, 70)
    inter = gb.inter_sets(bb.branch_colors(U, G.recs, k, tb.brute_sets(kmers, k, refs, 2)))
    with tb.build_sets(idx, refs, True, 70) as s:
        ids, table = s.copy()
    rng = np.random.default_rng(5)
    n_sets = len(table)
    table2 = np.concatenate([table, table[1:]])                  # every non-zero row twice, half of the columns on the copy
    ids2 = ids.copy()
    move = (ids2 > 0) & (rng.random(len(ids2)) < 0.5)
    ids2[move] += n_sets - 1
    perm = np.concatenate([[0], 1 + rng.permutation(len(table2) - 1)]).astype(np.uint32)
    table3 = np.empty_like(table2)
    table3[perm] = table2
    with capi.ColorSets.from_arrays(idx, 70, perm[ids2], table3) as up, Dev(idx, up) as d:
        d.g.add_reads(enc(reads), 2)
        check(d.g, G, "uploaded", inter, 70)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_leave_everything_usable(small):
    import torch
    k, seqs, reads, idx, U, lt, G = small
    L = capi.lib()
    r = enc(reads)
    bases, off = capi.concat_reads(r)
    n = len(r)
    out = C.c_void_p()
    _, other_n = make_index(seqs + ["ACGTTGCATGCCAAGGTT"], k, True)
    _, other_k = make_index(seqs, k + 1, True)
    _, tiny = make_index([G4, H4], hand.K)
    with tb.build_sets(idx, [[seqs[0]], [seqs[1]]], True) as s, Dev(idx) as d:
        g, h = d.g, d.g.handle
        g.add_reads(r, 2)
        # create
        refused(lambda: capi._check(L.sbwtgpu_genotype_create(None, d.u._h, d.b._h, C.byref(out))), "NULL")
        refused(lambda: capi._check(L.sbwtgpu_genotype_create(idx._h, None, d.b._h, C.byref(out))), "NULL")
        refused(lambda: capi._check(L.sbwtgpu_genotype_create(idx._h, d.u._h, None, C.byref(out))), "NULL")
        refused(lambda: capi._check(L.sbwtgpu_genotype_create(idx._h, d.u._h, d.b._h, None)), "NULL")
        with s.unitig_graph_dev(links=True, column_map=True) as cu:
            refused(lambda: cu.genotype(idx, d.b), "coloured handle", "plain handle")
        with idx.unitig_graph_dev(links=False, column_map=True) as nu:
            refused(lambda: nu.genotype(idx, d.b), "SBWTGPU_UNITIGS_LINKS")
        with idx.unitig_graph_dev(links=True, column_map=False) as nu:
            refused(lambda: nu.genotype(idx, d.b), "SBWTGPU_UNITIGS_COLUMN_MAP")
        refused(lambda: d.u.genotype(other_n, d.b), "was not made from this index", "columns")
        refused(lambda: d.u.genotype(other_k, d.b), "was not made from this index", "k = 16")
        # bubbles of another handle.  Of a larger graph: a record names a unitig the handle does not have.  Of a graph with
        # as many unitigs: the insertion case has unitigs 0 and 2 like the SNP case, but unitig 2 holds 6 k-mers, not 4.
        # Where indices and k-mer counts all fit -- the cycle's branches 0 and 2 are the SNP case's -- nothing can tell,
        # as the header says: the object is made, and counts at those unitigs.
        _, ins = make_index([G4, INS], hand.K)
        _, cyc = make_index(CYC, hand.K)
        with Dev(tiny) as t:
            assert t.rec == [(3, 0, 2, 1, 4, 4, 1)]
            refused(lambda: t.u.genotype(tiny, d.b), "do not fit the handle", "another handle")
            with Dev(ins) as i:
                assert i.rec == [(3, 1, 2, 0, 3, 6, 0)] and i.u.n_unitigs == t.u.n_unitigs == 4
                refused(lambda: i.u.genotype(ins, t.b), "do not fit the handle", "n_kmers is not that unitig's k-mer count")
                refused(lambda: t.u.genotype(tiny, i.b), "do not fit the handle", "n_kmers is not that unitig's k-mer count")
                assert i.g.info()["n_branch_kmers"] == 9
            with Dev(cyc) as c, c.u.genotype(cyc, t.b) as fits:
                assert c.rec == [(1, 0, 2, 1, 4, 4, 1)] and fits.info()["n_branch_kmers"] == 8
                fits.add_reads([CYC[0].encode()])
                assert fits.kmer_hits()[1].tolist() == [1, 1, 1, 1, 0, 0, 0, 0]
            assert t.g.info()["n_bubbles"] == 1
        ins.close()
        cyc.close()
        bits = np.random.default_rng(1).integers(0, 2**64, size=4, dtype=np.uint64)
        ro = capi.Index.create(bits, bits, bits, bits, None, 256, 3)
        refused(lambda: d.u.genotype(ro, d.b), "only rank()")
        ro.close()
        # adds from host buffers
        host = (bases.ctypes.data, off.ctypes.data)
        refused(lambda: capi._check(L.sbwtgpu_genotype_add_batch(None, *host, n, 1)), "NULL")
        refused(lambda: capi._check(L.sbwtgpu_genotype_add_batch(h, bases.ctypes.data, None, n, 1)), "NULL", "read_off")
        refused(lambda: capi._check(L.sbwtgpu_genotype_add_batch(h, None, off.ctypes.data, n, 1)), "NULL", "bases")
        for strands in (0, 3, -1):
            refused(lambda: capi._check(L.sbwtgpu_genotype_add_batch(h, *host, n, strands)), "strands")
        refused(lambda: capi._check(L.sbwtgpu_genotype_add_batch(h, *host, -1, 1)), "n_reads")
        refused(lambda: capi._check(L.sbwtgpu_genotype_add_batch(h, *host, 1 << 31, 1)), "2^31 reads")
        with pytest.raises(capi.SbwtGpuError) as ei:
            capi._check(L.sbwtgpu_genotype_add_batch(h, bases.ctypes.data, np.array([0, 1 << 31], dtype=np.int64).ctypes.data, 1, 1))
        assert ei.value.code == capi.ERR_READ_TOO_LONG
        # the device entry point
        dev = torch.device("cuda", 0)
        d_bases, d_off = torch.from_numpy(bases.copy()).to(dev), torch.from_numpy(off.copy()).to(dev)
        need = capi.genotype_workspace_bytes(len(bases), n, 2)
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        good = (d_bases.data_ptr(), len(bases), d_off.data_ptr(), n)
        refused(lambda: capi._check(L.sbwtgpu_genotype_add_dev(None, *good, 1, ws.data_ptr(), need, None)), "NULL")
        refused(lambda: capi._check(L.sbwtgpu_genotype_add_dev(h, None, len(bases), d_off.data_ptr(), n, 1, ws.data_ptr(), need, None)), "NULL")
        refused(lambda: capi._check(L.sbwtgpu_genotype_add_dev(h, d_bases.data_ptr(), len(bases), None, n, 1, ws.data_ptr(), need, None)), "NULL")
        refused(lambda: capi._check(L.sbwtgpu_genotype_add_dev(h, *good, 1, None, need, None)), "workspace")
        refused(lambda: capi._check(L.sbwtgpu_genotype_add_dev(h, *good, 2, ws.data_ptr(), capi.genotype_workspace_bytes(len(bases), n, 1), None)),
                "workspace")
        refused(lambda: capi._check(L.sbwtgpu_genotype_add_dev(h, *good, 3, ws.data_ptr(), need, None)), "strands")
        refused(lambda: capi._check(L.sbwtgpu_genotype_add_dev(h, d_bases.data_ptr(), len(bases), d_off.data_ptr(), -1, 1, ws.data_ptr(), need, None)),
                "n_reads")
        refused(lambda: capi._check(L.sbwtgpu_genotype_add_dev(h, d_bases.data_ptr(), -1, d_off.data_ptr(), n, 1, ws.data_ptr(), need, None)),
                "negative")
        torch.cuda.synchronize(dev)
        # the queries
        for ppm in (0, -1, 1_000_001):
            refused(lambda: g.calls(ppm, 1), "breadth_ppm")
        refused(lambda: g.calls(1_000_000, -1), "min_depth")
        one = np.zeros(8, dtype=np.int64)
        refused(lambda: capi._check(L.sbwtgpu_genotype_calls(h, 1_000_000, 1, None, one.ctypes.data, None, None)), "without colours")
        refused(lambda: capi._check(L.sbwtgpu_genotype_info(None, None, None, None, None, None, None)), "NULL")
        refused(lambda: capi._check(L.sbwtgpu_genotype_branches(None, None, None, None)), "NULL")
        refused(lambda: capi._check(L.sbwtgpu_genotype_kmer_hits_copy(None, None, None)), "NULL")
        refused(lambda: capi._check(L.sbwtgpu_genotype_reset(None)), "NULL")
        L.sbwtgpu_genotype_destroy(None)
        # any output may be NULL
        nh = C.c_int64(-1)
        capi._check(L.sbwtgpu_genotype_info(h, None, None, None, C.byref(nh), None, None))
        assert nh.value == G.n_hits
        capi._check(L.sbwtgpu_genotype_branches(h, None, None, None))
        mn = np.full(2 * len(G.recs), -1, dtype=np.int64)
        capi._check(L.sbwtgpu_genotype_branches(h, None, None, mn.ctypes.data))
        assert mn.tolist() == G.branches()[2]
        capi._check(L.sbwtgpu_genotype_kmer_hits_copy(h, None, None))
        capi._check(L.sbwtgpu_genotype_calls(h, 1_000_000, 1, None, None, None, None))
        check(g, G, "after the refusals")                        # nothing of it changed the object
        with d.u.bubbles() as again:                             # ... nor the handle or the index
            assert tb.as_tuples(again.records()) == d.rec
        assert len(idx.search_reads([seqs[0].encode()])[0]) == len(seqs[0]) - k + 1
    for x in (other_n, other_k, tiny):
        x.close()


# ---- 8. the CLI ------------------------------------------------------------------------------------------------------------------
def test_cli(gpu, tmp_path):
    d = str(tmp_path)
    k = 15
    g, h, _ = bb.planted(k, 3000, 40, 2)
    seqs = [g, h, g[:723] + "ACG" + g[723:1500]]                # 40 SNPs and an insertion
    with open(d + "/in.fna", "w") as fh:
        fh.write("".join(">%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    p = tb.run([SBWT, "build", "-i", d + "/in.fna", "-o", d + "/i.sbwt", "-k", str(k)])
    assert p.returncode == 0, p.stderr.decode()
    refs = [[g], [h], [seqs[2]], [h[a:a + 20] for a in range(0, len(h) - 20, 31)]]
    with open(d + "/refs.txt", "w") as fh:
        for ci, mine in enumerate(refs):
            name = "%s/ref%d.fna" % (d, ci)
            with open(name, "w") as out:
                out.write("".join(">r%d_%d\n%s\n" % (ci, j, s) for j, s in enumerate(mine)))
            fh.write(name + "\n")
    # g everywhere; h's first 1200 bases from the other strand; 9 of the 15 k-mers of h's allele at the site at 2220
    reads = gb.tiles(g, 60, 7) + [revcomp(x) for x in gb.tiles(h[:1200], 50, 9)] + ["ACGTNACGTACGTACGTACGT", "acgt", h[700:760], h[2200:2229]]
    fastq = "".join("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)) for i, r in enumerate(reads))
    with open(d + "/reads.fastq", "w") as fh:
        fh.write(fastq)
    with gzip.open(d + "/reads.fastq.gz", "wt") as fh:
        fh.write(fastq)
    kmers = kmer_set(seqs, k)
    U, lo, lt, recs = bb.brute_bubbles(kmers, k)
    col = bb.branch_colors(U, recs, k, tb.brute_sets(kmers, k, refs, 1))
    inter = gb.inter_sets(col)
    want = {s: gb.Genotype(U, recs, k).add(reads, s) for s in (1, 2)}
    assert want[2].n_site_hits > want[1].n_site_hits > 0 and len(set(want[2].calls())) >= 3
    assert want[1].calls(500_000, 0) != want[1].calls() != want[1].calls(1_000_000, 8)
    # (colour file, its flags, [(both strands, snps only, gzip, breadth, depth, query file)])
    plans = (("c3.colors", ["--compress"], [(False, False, False, None, None, "reads.fastq"), (True, True, True, "0.5", "0", "reads.fastq.gz"),
                                           (True, False, False, "1.0", "8", "reads.fastq")]),
             (None, None, [(False, True, False, None, None, "reads.fastq.gz"), (True, False, True, "0.500000", None, "reads.fastq")]),
             ("c1.colors", [], [(True, False, False, None, "2", "reads.fastq")]), ("c2.colors", ["--wide"], [(False, False, False, "0.75", None, "reads.fastq")]))
    for colors_file, flags, runs in plans:
        if colors_file:
            p = tb.run([SBWT, "build-colors", "-i", d + "/i.sbwt", "-r", d + "/refs.txt", "-o", d + "/" + colors_file] + flags)
            assert p.returncode == 0, p.stderr.decode()
        extra = ["-c", d + "/" + colors_file, "--refs-out", d + "/refs.tsv"] if colors_file else []
        for both, snps_only, z, breadth, depth, query in runs:
            ppm = {None: 1_000_000, "0.5": 500_000, "1.0": 1_000_000, "0.500000": 500_000, "0.75": 750_000}[breadth]
            dep = int(depth) if depth is not None else 1
            G = want[2 if both else 1]
            out = d + "/b.tsv" + (".gz" if z else "")
            cmd = [SBWT, "bubbles", "-i", d + "/i.sbwt", "-o", out, "-q", d + "/" + query, "--batch-bases", "700"] + extra
            cmd += (["--both-strands"] if both else []) + (["--snps-only"] if snps_only else []) + (["-z"] if z else [])
            cmd += (["--min-breadth", breadth] if breadth else []) + (["--min-depth", depth] if depth else [])
            p = tb.run(cmd)
            assert p.returncode == 0, p.stderr.decode()
            got = (gzip.open(out).read() if z else open(out, "rb").read()).decode()
            assert got == gb.format_tsv(G, len(lt), col if colors_file else None, snps_only, ppm, dep), (colors_file, both, snps_only, z, breadth, depth)
            if colors_file:
                assert open(d + "/refs.tsv").read() == gb.refs_tsv(*G.refs(inter, 4, ppm, dep)), (colors_file, both, breadth, depth)
    # without -q: byte for byte the text of section 24
    for colors_file in ("c3.colors", None):
        p = tb.run([SBWT, "bubbles", "-i", d + "/i.sbwt", "-o", d + "/plain.tsv"] + (["-c", d + "/" + colors_file] if colors_file else []))
        assert p.returncode == 0, p.stderr.decode()
        assert open(d + "/plain.tsv").read() == bb.format_tsv(U, len(lt), recs, col if colors_file else None)
    p = tb.run([SBWT, "bubbles", "-i", d + "/i.sbwt", "-o", d + "/e.tsv", "-q", d + "/reads.fastq", "--refs-out", d + "/r.tsv"])
    assert p.returncode == 1 and b"--refs-out needs a colour file" in p.stderr
