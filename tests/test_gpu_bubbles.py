"""GPU: bubbles of the plain unitig graph and the colours of their branches (sbwtgpu_bubbles_*) exactly
against the brute-force restatement of the definition (tests/bubbles_brute.py): records, n_snps, in-degrees, alleles and the
inter / uni rows, on the hand cases of tests/test_bubbles_cpu.py, on planted SNPs at k = 2 ... 64 and on the 40 000-base case
whose 2105 unitigs and 698 bubbles cross workgroup and wave boundaries; every layout the unitig tests cover, the refusals, two
host threads, and the C++ CLI.  The helpers are those of tests/test_gpu_unitigs.py and tests/test_gpu_colored_unitigs.py."""
import ctypes as C
import gzip
import os
import subprocess
import threading

import numpy as np
import pytest

import bubbles_brute as bb
import test_bubbles_cpu as hand
from bruteforce import kmer_set, revcomp
from colored_unitig_brute import sets_of_references
from test_gpu_colored_unitigs import refused
from test_gpu_unitig_links import from_device, hip_runtime
from test_gpu_unitigs import make_index, split
from unitig_brute import flatten
from sbwt_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")
NONE = 0xFFFFFFFF


def text(seqs):
    return [s.decode() if isinstance(s, bytes) else s for s in seqs]


def index_kmers(seqs, k, rc):
    return kmer_set(text(seqs) + ([revcomp(s) for s in text(seqs)] if rc else []), k)


def build_sets(idx, refs, both=False, n_colors=None):
    """The builder's colour-set object of idx with colour c given the sequences refs[c] (colours without a sequence stay new)."""
    with capi.ColorSetsBuilder.create(idx, n_colors or max(1, len(refs))) as b:
        for c, seqs in enumerate(refs):
            if seqs:
                b.add_reads(c, [x.encode() if isinstance(x, str) else x for x in seqs], both)
        return b.finish()


def brute_sets(kmers, k, refs, strands):
    """sets_of_references over the colours that have a sequence (4096 colours: most have none)"""
    used = [c for c, r in enumerate(refs) if r]
    sub = sets_of_references(kmers, k, [text(refs[c]) for c in used], strands)
    return {x: frozenset(used[c] for c in z) for x, z in sub.items()}


def run_bubbles(idx, sets=None):
    """Everything the bubble calls give for the plain graph of idx (with the colours of `sets`), as a dict of arrays."""
    with idx.unitig_graph_dev(links=True, column_map=True) as u:
        r = {"indeg": u.in_degrees()}
        r["bases"], r["off"], _ = u.copy()
        r["link_off"], r["link_to"] = u.links()
        with u.bubbles(sets) as b:
            r["info"] = b.info()
            r["rec"] = b.records()
            r["inter"], r["uni"] = b.branch_colors()
            assert (b.n_bubbles, b.n_snps) == (r["info"]["n_bubbles"], r["info"]["n_snps"])
            ms = b.stats()["pass_ms"]
            assert list(ms) == ["in_degrees", "detect", "compact", "branch_colors"] and all(v >= 0 for v in ms.values())
    return r


def as_tuples(rec):
    assert rec.dtype == capi.BUBBLE and not rec["reserved"].any()
    return [(int(r["source"]), int(r["branch"][0]), int(r["branch"][1]), int(r["sink"]), int(r["n_kmers"][0]), int(r["n_kmers"][1]),
             int(r["kind"])) for r in rec]


def check_invariants(r, k):
    rec, lo, lt, indeg = r["rec"], r["link_off"], r["link_to"], r["indeg"]
    n = len(lo) - 1
    assert indeg.dtype == np.uint32 and len(indeg) == n and int(indeg.sum()) == len(lt)
    assert np.array_equal(indeg, np.bincount(lt, minlength=n))
    assert np.all(np.diff(rec["source"].astype(np.int64)) > 0)                     # ascending by source
    outdeg = np.diff(lo)
    br = rec["branch"].reshape(-1)
    assert np.all(indeg[br] == 1) and np.all(outdeg[br] == 1) and len(set(br.tolist())) == len(br)
    assert np.all(outdeg[rec["source"]] == 2) and np.all(indeg[rec["sink"]] == 2)
    assert np.array_equal(rec["n_kmers"], (r["off"][br + 1] - r["off"][br] - (k - 1)).reshape(-1, 2))
    assert np.array_equal(rec["kind"] == capi.BUBBLE_SNP, np.all(rec["n_kmers"] == k, axis=1))
    assert r["info"]["n_bubbles"] == len(rec) and r["info"]["n_snps"] == int((rec["kind"] == capi.BUBBLE_SNP).sum())


def device_alleles(r):
    U = split(r["bases"], r["off"])
    return [tuple(U[int(x["branch"][j])][-int(x["n_kmers"][j]):].decode() for j in (0, 1)) for x in r["rec"]]


def check_brute(idx, seqs, k, rc, label, refs=None, n_colors=None, brute=None):
    """The bubble calls on idx == the brute force, exactly; refs: the sequences of every colour.  Returns (device, brute)."""
    kmers = index_kmers(seqs, k, rc)
    U, lo, lt, recs = brute or bb.brute_bubbles(kmers, k)
    assert idx.n_kmers == len(kmers), label
    if refs is None:
        r = run_bubbles(idx)
        assert r["info"]["n_colors"] == 0 and r["info"]["words"] == 0 and r["inter"].shape == (len(recs), 2, 0), label
    else:
        n_colors = n_colors or len(refs)
        W = (n_colors + 63) // 64
        with build_sets(idx, refs, rc, n_colors) as s:
            r = run_bubbles(idx, s)
        assert (r["info"]["n_colors"], r["info"]["words"]) == (n_colors, W), label
        col = bb.branch_colors(U, recs, k, brute_sets(kmers, k, refs, 2 if rc else 1))
        want_i = np.array([[bb.row_words(c[j][0], W) for j in (0, 1)] for c in col], dtype=np.uint64).reshape(len(recs), 2, W)
        want_u = np.array([[bb.row_words(c[j][1], W) for j in (0, 1)] for c in col], dtype=np.uint64).reshape(len(recs), 2, W)
        assert r["inter"].dtype == np.uint64 and np.array_equal(r["inter"], want_i), label
        assert np.array_equal(r["uni"], want_u), label
    assert (r["bases"].tobytes(), r["off"].tolist()) == flatten(U), label
    assert r["link_off"].tolist() == lo and r["link_to"].tolist() == lt, label
    assert r["indeg"].tolist() == bb.in_degrees(len(U), lt), label
    assert as_tuples(r["rec"]) == recs, label
    assert r["info"]["n_snps"] == sum(1 for x in recs if x[6] == bb.SNP), label
    assert device_alleles(r) == [bb.alleles(U, x) for x in recs], label
    check_invariants(r, k)
    return r, (U, lo, lt, recs)


def snp_refs(g, h, k, n_colors):
    """g on colour 0, h on colour 1, pieces of h (some cover part of a branch) on the last colour, and from four colours on
    a copy of g in the middle: the first word, the last word and the bits above n_colors all matter."""
    refs = [[] for _ in range(n_colors)]
    refs[0], refs[1] = [g], [h]
    refs[n_colors - 1] = refs[n_colors - 1] + [h[a:a + k + max(1, k // 3)] for a in range(0, len(h) - k, 2 * k + 1)]
    if n_colors > 3:
        refs[n_colors // 2] = [g]
    return refs


# ---- 1. the hand cases of the CPU file ----------------------------------------------------------------------------------------
HAND = {
    "one snp": ([hand.G, hand.H], 1),
    "insertion": ([hand.G, hand.G[:7] + "TTA" + hand.G[7:]], 1),
    "three alleles": ([hand.G, hand.H, hand.G[:7] + "A" + hand.G[8:]], 0),
    "joined branch": ([hand.G, hand.H, "TTCGTA"], 0),
    "sink with three in-links": ([hand.G, hand.H, "AAGTAGG"], 0),
    "branch with two out-links": ([hand.G, hand.H, "ACCGG"], 0),
    "self-link source": (["AAAAACGT"], 0),
    "cycle": ([hand.circular("CATTGACCGTAGG", 4), hand.circular("CATTGACTGTAGG", 4)], 1),
    "two close": (["CATTGACCGTAGGAAGCTC", "CATTGACTGTCGGAAGCTC"], 1),
    "nested": (["CATTGACCGTAGGAAGCTC", "CATTGACTGTCGGAAGCTC", "CATTGACTGTAGGAAGCTC"], 0),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(gpu, name):
    seqs, n_bubbles = HAND[name]
    for rc in (False, True):
        _, idx = make_index(seqs, hand.K, rc)
        r, _ = check_brute(idx, seqs, hand.K, rc, (name, rc))
        if not rc:
            assert len(r["rec"]) == n_bubbles
        check_brute(idx, seqs, hand.K, rc, (name, rc, "colours"), [[s] for s in seqs] + [[seqs[0]]])


def test_hand_colours(gpu):
    """g = 0, h = 1, a copy of g = 2, a fragment of h's branch = 3: inter {0,2} / {1}, uni {0,2} / {1,3}."""
    _, idx = make_index([hand.G, hand.H], hand.K)
    r, _ = check_brute(idx, [hand.G, hand.H], hand.K, False, "colours", [[hand.G], [hand.H], [hand.G], ["ACTGT"]])
    assert r["inter"].tolist() == [[[0b0101], [0b0010]]] and r["uni"].tolist() == [[[0b0101], [0b1010]]]
    assert as_tuples(r["rec"]) == [(3, 0, 2, 1, 4, 4, 1)] and device_alleles(r) == [("CGTA", "TGTA")]


# ---- 2. planted SNPs, k = 2 ... 64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 4, 5, 8, 15, 16, 31, 32, 33, 63, 64])
@pytest.mark.parametrize("rc", [False, True])
def test_planted_snps(gpu, k, rc):
    n_colors = [3, 64, 65, 70, 4096, 4][(k + rc) % 6]
    g, h, sites = bb.planted(k, 30 * k + 60, 5, 1000 + k)
    _, idx = make_index([g, h], k, rc)
    r, _ = check_brute(idx, [g, h], k, rc, (k, rc))
    if k >= 15:                                                # (a short k has repeats: whatever the definition gives)
        assert len(r["rec"]) == (10 if rc else 5) and r["info"]["n_snps"] == len(r["rec"])
    check_brute(idx, [g, h], k, rc, (k, rc, n_colors), snp_refs(g, h, k, n_colors), n_colors)


@pytest.mark.parametrize("n_colors", [3, 64, 65, 70, 4096])
def test_row_widths(gpu, n_colors):
    """W = 1, 2 and 64, a full last word and the bits above n_colors."""
    k = 15
    g, h, _ = bb.planted(k, 3000, 40, 1)
    _, idx = make_index([g, h], k)
    r, _ = check_brute(idx, [g, h], k, False, n_colors, snp_refs(g, h, k, n_colors), n_colors)
    assert len(r["rec"]) == 40 and r["inter"].shape == (40, 2, (n_colors + 63) // 64)
    top = (n_colors - 1) % 64
    assert int(r["uni"][:, :, -1].max()) >> top == 1                                  # the last colour is used, nothing above it
    assert not np.array_equal(r["inter"], r["uni"])                                   # a fragment covers part of a branch


@pytest.fixture(scope="module")
def big():
    """k = 15, 40 000 bases, 700 planted SNPs: 2105 unitigs and 698 bubbles (repeated 14-mers merge two)."""
    k = 15
    g, h, _ = bb.planted(k, 40_000, 700, 6)
    brute = bb.brute_bubbles(kmer_set([g, h], k), k)
    assert len(brute[0]) == 2105 and len(brute[3]) == 698
    return k, g, h, brute


def test_many_workgroups(gpu, big):
    k, g, h, brute = big
    _, idx = make_index([g, h], k)
    r, _ = check_brute(idx, [g, h], k, False, "big", brute=brute)
    assert len(r["rec"]) == 698 and len(r["indeg"]) == 2105
    r2, _ = check_brute(idx, [g, h], k, False, "big colours", snp_refs(g, h, k, 70), 70, brute=brute)
    # byte-identical between runs
    for key in ("rec", "inter", "uni", "indeg"):
        assert run_bubbles(idx)[key].tobytes() == r[key].tobytes(), key
    with build_sets(idx, snp_refs(g, h, k, 70), False, 70) as s:
        again = run_bubbles(idx, s)
    for key in ("rec", "inter", "uni"):
        assert again[key].tobytes() == r2[key].tobytes(), key


def test_k9_repeats(gpu):
    k = 9
    g, h, _ = bb.planted(k, 400, 6, 4)
    for rc in (False, True):
        _, idx = make_index([g, h], k, rc)
        r, _ = check_brute(idx, [g, h], k, rc, ("k9", rc), snp_refs(g, h, k, 65), 65)
        if not rc:
            assert len(r["rec"]) == 5                              # 5 of the 6 planted


# ---- 3. an uploaded object with duplicate rows and permuted ids -------------------------------------------------------------------
def test_uploaded_object_with_duplicates_and_another_numbering(gpu):
    k = 15
    g, h, _ = bb.planted(k, 3000, 40, 2)
    _, idx = make_index([g, h], k, True)
    refs = snp_refs(g, h, k, 70)
    want, _ = check_brute(idx, [g, h], k, True, "canonical", refs, 70)
    with build_sets(idx, refs, True, 70) as s:
        ids, table = s.copy()
    rng = np.random.default_rng(5)
    n_sets = len(table)
    assert n_sets >= 3
    # every non-zero row twice, half of the columns moved to the copy, then all rows but row 0 renumbered
    table2 = np.concatenate([table, table[1:]])
    ids2 = ids.copy()
    move = (ids2 > 0) & (rng.random(len(ids2)) < 0.5)
    ids2[move] += n_sets - 1
    perm = np.concatenate([[0], 1 + rng.permutation(len(table2) - 1)]).astype(np.uint32)
    table3 = np.empty_like(table2)
    table3[perm] = table2
    with capi.ColorSets.from_arrays(idx, 70, perm[ids2], table3) as up:
        got = run_bubbles(idx, up)
    for key in ("rec", "inter", "uni"):
        assert got[key].tobytes() == want[key].tobytes(), key


# ---- 4. layouts, marks given and derived ------------------------------------------------------------------------------------------
def test_image_layouts_and_marks(gpu):
    k = 15
    g, h, _ = bb.planted(k, 3000, 40, 1)
    seqs = [g, h, g[:723] + "ACG" + g[723:1500]]                                      # SNPs and an insertion
    refs = snp_refs(g, h, k, 66)
    bits, idx = make_index(seqs, k, True)
    want, _ = check_brute(idx, seqs, k, True, "layouts", refs, 66)
    assert len(want["rec"]) > 80 and 0 < want["info"]["n_snps"] < len(want["rec"])
    with build_sets(idx, refs, True, 66) as s:
        ids, table = s.copy()
    variants = []
    for key, val, back in (("image_level", 1, 0), ("image_level", 2, 0), ("force_mega", 1, 0), ("big_path", 2, 1)):
        capi.set_tuning(key, val)
        try:
            variants.append(((key, val), make_index(seqs, k, True)[1]))
        finally:
            capi.set_tuning(key, back)
    for derive in (1, 0):               # no marks given: derived into the image, or into the call's scratch
        capi.set_tuning("derive_ssup", derive)
        try:
            for level in (0, 2):
                capi.set_tuning("image_level", level)
                variants.append((("no marks", derive, level), make_index(seqs, k, True, ssup=False)[1]))
        finally:
            capi.set_tuning("derive_ssup", 1)
            capi.set_tuning("image_level", 0)
    for name, other in variants:
        with capi.ColorSets.from_arrays(other, 66, ids, table) as s:
            got = run_bubbles(other, s)
        for key in ("rec", "inter", "uni", "indeg"):
            assert got[key].tobytes() == want[key].tobytes(), (name, key)
        assert np.array_equal(run_bubbles(other)["rec"], want["rec"]), name


# ---- 5. edges --------------------------------------------------------------------------------------------------------------------
def test_no_bubble_no_real_column_no_links(gpu):
    cases = {"no bubble": (["CATTGACCGTAGGA", "TTCGTA"], 4, True), "no links": (["AACCG", "CCGGTT"], 3, False),
             "no real column": (["ACG"], 6, False), "nothing valid": (["ACGTNACGT", "acgtacgtacgt"], 6, False)}
    for name, (seqs, k, links) in cases.items():
        bits, idx = make_index(seqs, k)
        with build_sets(idx, [seqs, seqs[:1]]) as s:
            for sets in (None, s):
                r = run_bubbles(idx, sets)
                assert (len(r["link_to"]) > 0) == links, name
                assert r["info"]["n_bubbles"] == 0 == r["info"]["n_snps"] and len(r["rec"]) == 0, name
                assert r["inter"].shape == (0, 2, 0 if sets is None else 1) and len(r["indeg"]) == len(r["off"]) - 1, name
                assert int(r["indeg"].sum()) == len(r["link_to"]), name
            with idx.unitig_graph_dev(links=True, column_map=True) as u, u.bubbles(s) as b:
                assert b.dev_ptrs() == (0, 0, 0), name
                capi._check(capi.lib().sbwtgpu_bubbles_copy(b._h, None, None, None))
        if name == "no real column":
            assert bits.n_kmers == 0


def test_device_pointers(gpu):
    k = 15
    g, h, _ = bb.planted(k, 3000, 40, 2)
    _, idx = make_index([g, h], k)
    hip = hip_runtime()
    with build_sets(idx, snp_refs(g, h, k, 65), False, 65) as s, idx.unitig_graph_dev(links=True, column_map=True) as u:
        with u.bubbles() as b:
            d_rec, d_i, d_u = b.dev_ptrs()
            assert d_rec and d_i == 0 and d_u == 0
            assert from_device(hip, d_rec, 40, capi.BUBBLE).tobytes() == b.records().tobytes()
            capi._check(capi.lib().sbwtgpu_bubbles_dev(b._h, C.byref(C.c_void_p()), None, None))
        with u.bubbles(s) as b:
            d_rec, d_i, d_u = b.dev_ptrs()
            inter, uni = b.branch_colors()
            assert from_device(hip, d_i, 40 * 2 * 2, np.uint64).tobytes() == inter.tobytes()
            assert from_device(hip, d_u, 40 * 2 * 2, np.uint64).tobytes() == uni.tobytes()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_leave_the_handle_usable(gpu):
    k = 15
    g, h, _ = bb.planted(k, 3000, 40, 1)
    _, idx = make_index([g, h], k)
    _, other_n = make_index([g, h, "ACGTTGCATGCCAAGGTT"], k)
    _, other_k = make_index([g, h], k + 1)
    L = capi.lib()
    out, n, ptr = C.c_void_p(), C.c_int64(0), np.zeros(4096, dtype=np.uint64).ctypes.data
    with build_sets(idx, [[g], [h]]) as s, build_sets(other_n, [[g], [h]]) as sn, build_sets(other_k, [[g], [h]]) as sk:
        with idx.unitig_graph_dev(links=True, column_map=True) as u:
            want = u.bubbles(s)
            rec, inter = want.records(), want.branch_colors()[0]
            refused(lambda: capi._check(L.sbwtgpu_bubbles_create(None, None, C.byref(out))), "NULL")
            refused(lambda: capi._check(L.sbwtgpu_bubbles_create(u._h, None, None)), "NULL")
            refused(lambda: u.bubbles(sn), "columns")
            refused(lambda: u.bubbles(sk), "k = 16")
            refused(lambda: capi._check(L.sbwtgpu_bubbles_info(want._h, None, C.byref(n), None, None)), "NULL", "n_bubbles")
            refused(lambda: capi._check(L.sbwtgpu_bubbles_dev(want._h, None, None, None)), "NULL", "d_rec")
            refused(lambda: capi._check(L.sbwtgpu_bubbles_copy(want._h, None, ptr, ptr)), "NULL", "rec")
            refused(lambda: capi._check(L.sbwtgpu_bubbles_copy(want._h, ptr, None, ptr)), "NULL", "inter")
            refused(lambda: capi._check(L.sbwtgpu_bubbles_copy(want._h, ptr, ptr, None)), "NULL", "uni")
            refused(lambda: capi._check(L.sbwtgpu_bubbles_in_degrees_copy(u._h, None)), "NULL", "indeg")
            refused(lambda: capi._check(L.sbwtgpu_bubbles_info(None, C.byref(n), None, None, None)), "NULL")
            refused(lambda: capi._check(L.sbwtgpu_bubbles_stats(None, None)), "NULL")
            capi._check(L.sbwtgpu_bubbles_stats(want._h, None))
            capi._check(L.sbwtgpu_bubbles_info(want._h, C.byref(n), None, None, None))
            assert n.value == 40
            with u.bubbles() as plain:                                                # no object: the row arguments may be NULL
                back = np.zeros(40, dtype=capi.BUBBLE)
                capi._check(L.sbwtgpu_bubbles_copy(plain._h, back.ctypes.data, None, None))
                assert back.tobytes() == rec.tobytes()
            # the handle, the object and the index are usable afterwards
            with u.bubbles(s) as again:
                assert again.records().tobytes() == rec.tobytes() and np.array_equal(again.branch_colors()[0], inter)
            want.close()
        with idx.unitig_graph_dev(links=True, column_map=False) as u:                 # an object needs the column map
            refused(lambda: u.bubbles(s), "SBWTGPU_UNITIGS_COLUMN_MAP")
            with u.bubbles() as b:
                assert b.records().tobytes() == rec.tobytes()
            assert u.in_degrees().sum() == u.n_links()
        for make in (idx.unitigs_dev, lambda: idx.unitig_graph_dev(links=False, column_map=True)):
            with make() as u:                                                         # no links
                refused(u.bubbles, "SBWTGPU_UNITIGS_LINKS")
                refused(lambda: u.bubbles(s), "SBWTGPU_UNITIGS_LINKS")
                refused(u.in_degrees, "SBWTGPU_UNITIGS_LINKS")
                assert len(u.copy()[2]) == u.n_unitigs
        with s.unitig_graph_dev(links=True, column_map=True) as u:                    # a coloured handle
            refused(u.bubbles, "coloured handle", "plain handle", "colour-set object")
            refused(lambda: u.bubbles(s), "coloured handle")
            refused(u.in_degrees, "coloured handle")
            assert u.n_links() > 0
        assert len(idx.search_reads([g.encode()])[0]) == len(g) - k + 1


# ---- 7. two host threads on one handle ---------------------------------------------------------------------------------------------
def test_two_threads_on_one_handle(gpu, big):
    k, g, h, brute = big
    _, idx = make_index([g, h], k)
    with build_sets(idx, snp_refs(g, h, k, 70), False, 70) as s, idx.unitig_graph_dev(links=True, column_map=True) as u:
        with u.bubbles(s) as b:
            want = (b.records().tobytes(),) + tuple(x.tobytes() for x in b.branch_colors())
        got, errors = [None, None], []

        def work(i):
            try:
                for _ in range(3):
                    with u.bubbles(s if i else None) as b:
                        got[i] = (b.records().tobytes(),) + tuple(x.tobytes() for x in b.branch_colors())
                    assert u.in_degrees().sum() == u.n_links()
            except Exception as e:                                                    # (reported below, in the main thread)
                errors.append(e)
        threads = [threading.Thread(target=work, args=(i,)) for i in (0, 1)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        assert got[1] == want and got[0] == (want[0], b"", b"")


# ---- 8. the CLI ------------------------------------------------------------------------------------------------------------------
def run(cmd, timeout=300):
    return subprocess.run(cmd, capture_output=True, timeout=timeout)


def test_cli(gpu, tmp_path):
    d = str(tmp_path)
    k = 15
    g, h, _ = bb.planted(k, 3000, 40, 2)
    seqs = [g, h, g[:723] + "ACG" + g[723:1500]]                                      # 40 SNPs and an insertion
    with open(d + "/in.fna", "w") as fh:
        fh.write("".join(">%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    p = run([SBWT, "build", "-i", d + "/in.fna", "-o", d + "/i.sbwt", "-k", str(k)])
    assert p.returncode == 0, p.stderr.decode()
    refs = [[g], [h], [seqs[2]], [h[a:a + 20] for a in range(0, len(h) - 20, 31)]]
    with open(d + "/refs.txt", "w") as fh:
        for ci, mine in enumerate(refs):
            name = "%s/ref%d.fna" % (d, ci)
            with open(name, "w") as out:
                out.write("".join(">r%d_%d\n%s\n" % (ci, j, s) for j, s in enumerate(mine)))
            fh.write(name + "\n")
    kmers = kmer_set(seqs, k)
    U, lo, lt, recs = bb.brute_bubbles(kmers, k)
    col = bb.branch_colors(U, recs, k, brute_sets(kmers, k, refs, 1))
    assert len(recs) == 41 and sum(1 for r in recs if r[6] == bb.SNP) == 40
    assert any(c[j][0] != c[j][1] for c in col for j in (0, 1))                       # some line carries a "|"
    # every option on the colour-set file and without colours; the two other colour file kinds once each
    plans = (("c3.colors", ["--compress"], [(False, False), (True, True)]), (None, None, [(False, True), (True, False)]),
             ("c1.colors", [], [(False, False)]), ("c2.colors", ["--wide"], [(False, False)]))
    for colors_file, flags, runs in plans:
        if colors_file:
            p = run([SBWT, "build-colors", "-i", d + "/i.sbwt", "-r", d + "/refs.txt", "-o", d + "/" + colors_file] + flags)
            assert p.returncode == 0, p.stderr.decode()
        extra = ["-c", d + "/" + colors_file] if colors_file else []
        for snps_only, z in runs:
            want = bb.format_tsv(U, len(lt), recs, col if colors_file else None, snps_only)
            out = d + "/b.tsv" + (".gz" if z else "")
            p = run([SBWT, "bubbles", "-i", d + "/i.sbwt", "-o", out] + extra + (["--snps-only"] if snps_only else []) + (["-z"] if z else []))
            assert p.returncode == 0, p.stderr.decode()
            got = (gzip.open(out).read() if z else open(out, "rb").read()).decode()
            assert got == want, (colors_file, snps_only, z)
            assert got.count("\n") == (41 if snps_only else 42)
    p = run([SBWT])
    assert p.returncode == 0 and b" bubbles" in p.stderr
