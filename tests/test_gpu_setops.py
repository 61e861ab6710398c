"""GPU: set operations on two indexes (sbwt_setops.hip) bit for bit against the brute-force restatement of their definition
(tests/setop_brute.py): the four rows, the marks, n_nodes and n_kmers; the extracted keys against a Python packing; the
algebra of the operations at a medium size against independent paths (the device builder, streaming_search over unitigs);
errors that leave both inputs usable; the C++ CLI."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from setop_brute import OPS, apply_op, brute_counts, brute_setop, build_from_kmers, kmers_of, packed_keys, same_bits
from sbwt_amd import capi, hostlib, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_kats.json")))
COUNT_KEYS = ("n_a", "n_b", "n_both", "n_either")


def as_bytes(seqs):
    return [s.encode() if isinstance(s, str) else s for s in seqs]


def index_of(bits, k):
    return capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)


def make_index(seqs, k, rc=False, ssup=True):
    bits = hostlib.build_bits(as_bytes(seqs), k, rc, ssup)
    return bits, index_of(bits, k)


def check_ops(ia, ib, sa, sb, k, rca, rcb, label, ops=OPS, marks=(True,)):
    """every operation of the two indexes == the brute force, bit for bit; the counts too"""
    want_counts = brute_counts(sa, sb, k, rca, rcb)
    got_counts = ia.setop_counts(ib)
    assert {f: got_counts[f] for f in COUNT_KEYS} == want_counts, label
    for op in ops:
        for m in marks:
            want, R = brute_setop(sa, sb, k, op, rca, rcb, m)
            got, info = ia.setop(ib, op, m)
            assert same_bits(got, want), (label, op, m)
            assert got.k == k and info["n_result"] == len(R) == got.n_kmers, (label, op)
            assert {f: info[f] for f in COUNT_KEYS} == want_counts, (label, op)
            assert info["n_a"] + info["n_b"] == info["n_both"] + info["n_either"]


def random_seqs(rng, k):
    alphabet = "AC" if k <= 5 else "ACGT"
    seqs = ["".join(rng.choice(alphabet) for _ in range(rng.randint(1, 300))) for _ in range(rng.randint(1, 40))]
    seqs.append("".join(rng.choice(alphabet) for _ in range(max(1, k - 1))))          # shorter than k
    seqs += ["".join(rng.choice(alphabet) for _ in range(k)) for _ in range(3)]       # exactly k: dummy-heavy
    s = list("".join(rng.choice(alphabet) for _ in range(3 * k + 40)))
    s[len(s) // 3] = "N"
    s[2 * len(s) // 3] = s[2 * len(s) // 3].lower()
    seqs.append("".join(s))
    return seqs


def overlapping_sets(rng, k):
    """two sequence lists that share about a third of their sequences, and pieces of others"""
    pool = random_seqs(rng, k) + random_seqs(rng, k)
    n = len(pool)
    sa, sb = pool[: 2 * n // 3], pool[n // 3:]
    long = max(sa, key=len)
    sb = sb + [long[len(long) // 4: 3 * len(long) // 4]]
    return sa, sb


def test_reference_inputs(gpu):
    cases = [(KATS["cli_end_to_end"]["seqs"], KATS["cli_end_to_end"]["k"], KATS["cli_end_to_end"]["add_reverse_complements"]),
             (KATS["redundant_dummies"]["seqs"], KATS["redundant_dummies"]["k"], False)]
    cases += [(c["seqs"], c["k"], False) for c in KATS["small_cases"]["cases"] if c["k"] >= 2]
    for seqs, k, rc in cases:
        h = (len(seqs) + 1) // 2
        sa, sb = seqs[:h], seqs[h:]
        _, ia = make_index(sa, k, rc)
        _, ib = make_index(sb, k, rc)
        check_ops(ia, ib, sa, sb, k, rc, rc, (seqs[0][:12], k))
        check_ops(ib, ia, sb, sa, k, rc, rc, ("swapped", k), ops=("difference",))
        _, iw = make_index(seqs, k, rc)
        check_ops(iw, ib, seqs, sb, k, rc, rc, ("whole against half", k))


@pytest.mark.parametrize("k", [2, 3, 4, 5, 8, 16, 31, 32, 33, 63, 64])
@pytest.mark.parametrize("rc", [False, True])
def test_random_sets(gpu, k, rc):
    rng = random.Random(1000 * k + rc)
    sa, sb = overlapping_sets(rng, k)
    assert kmers_of(sa, k, rc) & kmers_of(sb, k, rc)
    _, ia = make_index(sa, k, rc, ssup=True)
    _, ib = make_index(sb, k, rc, ssup=False)                     # neither index needs marks
    check_ops(ia, ib, sa, sb, k, rc, rc, (k, rc), marks=(True, False))
    check_ops(ib, ia, sb, sa, k, rc, rc, (k, rc, "swapped"), ops=("difference",))
    # one side with reverse complements, the other without
    _, ic = make_index(sb, k, not rc)
    check_ops(ia, ic, sa, sb, k, rc, not rc, (k, rc, "mixed strands"), ops=("intersection", "symmetric-difference"))


@pytest.mark.parametrize("k", [7, 31, 32, 33, 64])
def test_kmer_keys(gpu, k):
    """kmer_keys() == the packed sorted k-mer set, on indexes whose column count sits on the block and workgroup edges"""
    g = synth.random_genome(6000, 3 + k).tobytes()
    for target in (63, 64, 65, 255, 256, 257, 4000):
        # one sequence of L bases has L - k + 1 k-mers + k dummies (root included): L + 1 columns when no k-mer repeats
        seqs = [g[: target - 1]] if target - 1 >= k else [g[:k]]
        bits, idx = make_index(seqs, k)
        if k >= 31 and target - 1 >= k:
            assert bits.n_nodes == target
        keys = idx.kmer_keys()
        want = packed_keys(kmers_of(seqs, k), k)
        assert keys.dtype == np.uint64 and keys.shape == want.shape and len(keys) == bits.n_kmers == idx.n_kmers
        assert np.array_equal(keys, want), (k, target)
    bits, idx = make_index([g, g[100:900] + b"N" + g[:300]], k, True)
    assert np.array_equal(idx.kmer_keys(), packed_keys(kmers_of([g, g[100:900], g[:300]], k, True), k))
    # an index that does not know its n_kmers (0 in the descriptor)
    unknown = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], None, bits.n_nodes, k, 0, 0)
    assert np.array_equal(unknown.kmer_keys(), idx.kmer_keys())


def test_kmer_keys_small_k_and_empty(gpu):
    rng = random.Random(9)
    for k in (2, 3, 5, 16, 63):
        seqs = random_seqs(rng, k)
        for rc in (False, True):
            _, idx = make_index(seqs, k, rc)
            assert np.array_equal(idx.kmer_keys(), packed_keys(kmers_of(seqs, k, rc), k)), (k, rc)
    _, idx = make_index(["ACG", "ACNTACGA"], 6)
    assert idx.kmer_keys().shape == (0,)
    _, idx = make_index(["ACG"], 40)
    assert idx.kmer_keys().shape == (0, 2)


def rand_seqs_2k(rng, n):
    return ["".join(rng.choice("ACGT") for _ in range(2000)) for _ in range(n)]


@pytest.mark.parametrize("k", [12, 16])
def test_merge_edges(gpu, k):
    """lists of tens of thousands of keys, several merge tiles long"""
    rng = random.Random(k)
    seqs = rand_seqs_2k(rng, 24)
    sa, sb = seqs[:14], seqs[10:]
    _, ia = make_index(sa, k)
    _, ib = make_index(sb, k)
    assert ia.n_kmers > 20_000 and ib.n_kmers > 20_000
    check_ops(ia, ib, sa, sb, k, False, False, "overlap")
    check_ops(ia, ia, sa, sa, k, False, False, "a == b, one handle")
    _, ia2 = make_index(list(reversed(sa)), k)
    check_ops(ia, ia2, sa, sa, k, False, False, "a == b, two handles")
    # disjoint and interleaved: the even and the odd keys of one sorted list
    words = sorted(kmers_of(seqs, k), key=lambda w: w[::-1])
    ev, od = words[0::2], words[1::2]
    _, ie = make_index(ev, k)
    _, io = make_index(od, k)
    check_ops(ie, io, ev, od, k, False, False, "interleaved")
    # a entirely below b: colex order is decided by the last character
    lo, hi = [w for w in words if w[-1] in "AC"], [w for w in words if w[-1] in "GT"]
    _, il = make_index(lo, k)
    _, ih = make_index(hi, k)
    check_ops(il, ih, lo, hi, k, False, False, "a below b")
    check_ops(ih, il, hi, lo, k, False, False, "b below a", ops=("union", "difference"))
    # |a| = 1 against a long b: present, absent, below everything, above everything
    for one in (words[len(words) // 2], "ACGT" * (k // 4), "A" * k, "T" * k):
        _, i1 = make_index([one], k)
        check_ops(i1, ib, [one], sb, k, False, False, ("one", one))
        check_ops(ib, i1, sb, [one], k, False, False, ("one, swapped", one), ops=("difference", "intersection"))


def test_merge_tile_boundaries(gpu):
    """the equal keys move across the merge's tiles as the shared prefix of the sequence set grows"""
    k = 13
    rng = random.Random(131)
    seqs = rand_seqs_2k(rng, 12)
    own = rand_seqs_2k(rng, 3)
    for shared in range(0, 12, 2):
        for cut in (0, 517):
            sa = seqs[:shared] + [s[cut:] for s in seqs[shared:shared + 1]] + own[:1]
            sb = seqs[:shared + 1] + own[1:]
            _, ia = make_index(sa, k)
            _, ib = make_index(sb, k)
            check_ops(ia, ib, sa, sb, k, False, False, (shared, cut))


def test_image_levels_and_layouts(gpu):
    rng = random.Random(78)
    for k in (4, 15, 31, 40):
        sa, sb = overlapping_sets(rng, k)
        want = {op: brute_setop(sa, sb, k, op, True, True)[0] for op in OPS}
        want_keys = packed_keys(kmers_of(sa, k, True), k)
        plain_b = make_index(sb, k, True)[1]
        variants = []
        for key, val, back in (("image_level", 1, 0), ("image_level", 2, 0), ("force_mega", 1, 0), ("big_path", 2, 1)):
            capi.set_tuning(key, val)
            try:
                variants.append(((key, val), make_index(sa, k, True)[1]))
            finally:
                capi.set_tuning(key, back)
        for derive in (1, 0):           # no marks given: derived into the image, or absent
            capi.set_tuning("derive_ssup", derive)
            try:
                for level in (0, 2):
                    capi.set_tuning("image_level", level)
                    variants.append((("no marks", derive, level), make_index(sa, k, True, ssup=False)[1]))
            finally:
                capi.set_tuning("derive_ssup", 1)
                capi.set_tuning("image_level", 0)
        # a and b built with different settings: every variant of a against the plain b, and against the next variant of b
        others = [plain_b]
        for key, val, back in (("image_level", 2, 0), ("big_path", 2, 1), ("force_mega", 1, 0)):
            capi.set_tuning(key, val)
            try:
                others.append(make_index(sb, k, True, ssup=(key != "big_path"))[1])
            finally:
                capi.set_tuning(key, back)
        for i, (name, ia) in enumerate(variants):
            assert np.array_equal(ia.kmer_keys(), want_keys), (k, name)
            ib = others[i % len(others)]
            for op in OPS:
                got, _ = ia.setop(ib, op)
                assert same_bits(got, want[op]), (k, name, op)
            got, _ = ib.setop(ia, "union")
            assert same_bits(got, want["union"]), (k, name, "swapped")


def test_mega_block_layout(gpu, tmp_path):
    """The MEGA instantiations, through the test build with mega blocks of 2^12 columns (a fresh child loads it): two
    indexes of some 40 mega blocks give the bits the product build gives."""
    lib = os.path.join(ROOT, "sbwt_amd", "lib", "libsbwtgpu_mega12.so")
    assert os.path.exists(lib), "%s is missing: build it with `python -m sbwt_amd.build`" % lib
    k = 31
    g0 = synth.random_genome(40_000, 5)
    sa = [g0.tobytes(), synth.mutate(g0, 0.03, 6).tobytes()]
    sb = [sa[1], synth.mutate(g0, 0.03, 7).tobytes()]
    ba, bb = hostlib.build_bits(sa, k, True, True), hostlib.build_bits(sb, k, True, True)
    assert (ba.n_nodes >> 12) >= 30 and (bb.n_nodes >> 12) >= 30
    ia, ib = index_of(ba, k), index_of(bb, k)
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    arrays = {"meta": np.array([k], dtype=np.int64)}
    for name, b in (("a", ba), ("b", bb)):
        arrays.update({name + "/A": b.cols[0], name + "/C": b.cols[1], name + "/G": b.cols[2], name + "/T": b.cols[3],
                       name + "/ssup": b.ssup, name + "/meta": np.array([b.n_nodes, b.n_kmers], dtype=np.int64)})
    np.savez(fin, **arrays)
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tests", "setop_mega_worker.py"), fin, fout],
                       env=dict(os.environ, SBWTGPU_LIB=lib), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-4000:]
    out = np.load(fout, allow_pickle=False)
    assert "mega_shift=12" in str(out["version"])
    keys = ia.kmer_keys()
    for op in OPS:
        want, info = ia.setop(ib, op)
        for image in ("rel1", "rel0", "big1", "big0"):
            pre = "%s/%s/" % (image, op)
            assert [int(x) for x in out[pre + "meta"]] == [want.n_nodes, want.n_kmers, info["n_both"], info["n_either"]], (image, op)
            for c in range(4):
                assert np.array_equal(out[pre + "ACGT"[c]], want.cols[c]), (image, op, c)
            assert np.array_equal(out[pre + "ssup"], want.ssup), (image, op)
    for image in ("rel1", "rel0", "big1", "big0"):
        assert np.array_equal(out[image + "/keys"], keys), image


def pack31(genome, k=31):
    """every k-mer of an ACGT array as the builder's key (character i at bits 2i), k <= 32"""
    code = np.zeros(256, dtype=np.uint64)
    code[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4, dtype=np.uint64)
    c = code[genome]
    v = np.zeros(len(genome) - k + 1, dtype=np.uint64)
    for j in range(k):
        v |= c[j:j + len(v)] << np.uint64(2 * j)
    return v


def count_nopred(keys, k=31):
    """k-mers of a sorted key set whose (k-1)-prefix is the (k-1)-suffix of none"""
    if len(keys) == 0:
        return 0
    suf = np.unique(keys >> np.uint64(2))
    pre = keys & np.uint64((1 << (2 * k - 2)) - 1)
    i = np.minimum(np.searchsorted(suf, pre), len(suf) - 1)
    return int(np.sum(suf[i] != pre))


def test_algebra_medium(gpu):
    """Two strain sets on a 2 Mbp genome, k = 31.  The shapes: three strains that differ from the base by 0.1 % substitutions
    (some 2000 each); a = {s1, s2}, b = {s2, s3}.  Every substitution ends a shared stretch, so the intersection and the
    differences have a few thousand predecessor-less k-mers: x 31 far below 2^26, which the brute key sets confirm first."""
    k = 31
    base = synth.random_genome(2_000_000, 21)
    s1, s2, s3 = (synth.mutate(base, 0.001, 22 + i) for i in range(3))
    sa, sb = [s1.tobytes(), s2.tobytes()], [s2.tobytes(), s3.tobytes()]
    KA = np.unique(np.concatenate([pack31(s1), pack31(s2)]))
    KB = np.unique(np.concatenate([pack31(s2), pack31(s3)]))
    brute = {"union": np.union1d(KA, KB), "intersection": np.intersect1d(KA, KB), "difference": np.setdiff1d(KA, KB),
             "symmetric-difference": np.setxor1d(KA, KB)}
    nopred = {op: count_nopred(v) for op, v in brute.items()}
    assert max(nopred.values()) * k < (1 << 26) // 100, nopred
    ba, bb = capi.build_bits_gpu(sa, k, False, True), capi.build_bits_gpu(sb, k, False, True)
    ia, ib = index_of(ba, k), index_of(bb, k)
    assert np.array_equal(ia.kmer_keys(), KA) and np.array_equal(ib.kmer_keys(), KB)
    res = {}
    for op in OPS:
        res[op], info = ia.setop(ib, op)
        assert info["n_nopred"] * k < (1 << 26) and info["n_nopred"] == nopred[op], (op, info)
        assert (info["n_a"], info["n_b"], info["n_both"], info["n_either"]) == (len(KA), len(KB), len(brute["intersection"]),
                                                                                 len(brute["union"]))
        assert info["n_a"] + info["n_b"] == info["n_both"] + info["n_either"]
        assert res[op].n_kmers == info["n_result"] == len(brute[op]), op
    c = ia.setop_counts(ib)
    assert abs(c["jaccard"] - len(brute["intersection"]) / len(brute["union"])) < 1e-12
    # a with itself
    assert same_bits(ia.setop(ia, "union")[0], ba) and same_bits(ia.setop(ia, "intersection")[0], ba)
    empty, info = ia.setop(ia, "difference")
    assert (empty.n_nodes, empty.n_kmers, info["n_result"], info["n_both"]) == (1, 0, 0, len(KA))
    assert all(int(empty.cols[c][0]) == 0 for c in range(4)) and int(empty.ssup[0]) == 1
    # union == the device builder on both inputs
    assert same_bits(res["union"], capi.build_bits_gpu(sa + sb, k, False, True))
    # union(a minus b, b) == union(a, b)
    idiff = index_of(res["difference"], k)
    assert same_bits(idiff.setop(ib, "union")[0], res["union"])
    # |a and b| from an independent path: b's answers over a's unitigs; the intersection index answers exactly those
    ub, uo, _ = ia.unitigs()
    in_b, _ = ib.streaming_search(ub, uo)
    assert int((in_b >= 0).sum()) == len(brute["intersection"])
    iint = index_of(res["intersection"], k)
    in_i, _ = iint.streaming_search(ub, uo)
    assert np.array_equal(in_i >= 0, in_b >= 0)
    # and nothing else: b's own unitigs hit the intersection exactly where they hit a
    vb, vo, _ = ib.unitigs()
    assert np.array_equal(iint.streaming_search(vb, vo)[0] >= 0, ia.streaming_search(vb, vo)[0] >= 0)


def split(bases, off):
    b = bases.tobytes()
    return [b[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def test_closed_loop(gpu):
    """Index.create on a result searches like an index built from the result's unitigs"""
    rng = random.Random(4)
    for k in (9, 31, 47):
        sa, sb = overlapping_sets(rng, k)
        _, ia = make_index(sa, k, True)
        _, ib = make_index(sb, k, True)
        queries = as_bytes(sa[:6] + sb[-6:])
        qb, qo = capi.concat_reads(queries)
        for op in OPS:
            bits, _ = ia.setop(ib, op)
            ir = index_of(bits, k)
            ub, uo, _ = ir.unitigs()
            back = capi.build_bits_gpu(split(ub, uo), k, False, True)
            assert same_bits(back, bits), (k, op)
            i2 = index_of(back, k)
            for fn in ("streaming_search", "search"):
                assert np.array_equal(getattr(ir, fn)(qb, qo)[0], getattr(i2, fn)(qb, qo)[0]), (k, op, fn)
            R = apply_op(kmers_of(sa, k, True), kmers_of(sb, k, True), op)
            clean = [q for q in queries if set(q) <= set(b"ACGT")]
            cb, co = capi.concat_reads(clean)
            hits = ir.streaming_search(cb, co)[0] >= 0
            want = [q[i:i + k].decode() in R for q in clean for i in range(len(q) - k + 1)]
            assert len(want) > 100 and hits.tolist() == want, (k, op)


def test_errors_leave_the_inputs_usable(gpu):
    rng = random.Random(6)
    k = 21
    sa, sb = overlapping_sets(rng, k)
    _, ia = make_index(sa, k, True)
    _, ib = make_index(sb, k, True)
    qb, qo = capi.concat_reads(as_bytes(sa[:5] + sb[:5]))
    before = [ia.streaming_search(qb, qo)[0], ib.streaming_search(qb, qo)[0]]

    def unchanged():
        assert np.array_equal(ia.streaming_search(qb, qo)[0], before[0]) and np.array_equal(ib.streaming_search(qb, qo)[0], before[1])

    L = capi.lib()
    out, info = capi.PlainMatrixBitsC(), capi.SetopInfoC()
    _, other_k = make_index(sb, k + 1, True)
    with pytest.raises(capi.SbwtGpuError) as e:
        ia.setop(other_k, "union")
    assert e.value.code == capi.ERR_INVALID_ARG and "differ in k" in e.value.msg and str(k + 1) in e.value.msg
    unchanged()
    with pytest.raises(capi.SbwtGpuError) as e:
        ia.setop_counts(other_k)
    assert e.value.code == capi.ERR_INVALID_ARG
    # k = 65 and above: an index of the host builder
    long_seqs = ["".join(rng.choice("ACGT") for _ in range(200)) for _ in range(3)]
    for kk in (65, 80):
        _, il = make_index(long_seqs, kk)
        with pytest.raises(capi.SbwtGpuError) as e:
            il.setop(il, "union")
        assert e.value.code == capi.ERR_INVALID_ARG and "k = %d" % kk in e.value.msg
        with pytest.raises(capi.SbwtGpuError) as e:
            il.kmer_keys()
        assert e.value.code == capi.ERR_INVALID_ARG
    # NULL arguments
    assert L.sbwtgpu_index_setop(None, ib.handle, 0, 1, capi.C.byref(out), capi.C.byref(info)) == capi.ERR_INVALID_ARG
    assert L.sbwtgpu_index_setop(ia.handle, None, 0, 1, capi.C.byref(out), None) == capi.ERR_INVALID_ARG
    assert L.sbwtgpu_index_setop(ia.handle, ib.handle, 0, 1, None, None) == capi.ERR_INVALID_ARG
    assert L.sbwtgpu_index_setop_counts(ia.handle, ib.handle, None) == capi.ERR_INVALID_ARG
    assert L.sbwtgpu_index_setop_counts(None, ib.handle, capi.C.byref(info)) == capi.ERR_INVALID_ARG
    assert L.sbwtgpu_index_kmer_keys(None, None, 0, None, None) == capi.ERR_INVALID_ARG
    unchanged()
    # info may be NULL on a call that succeeds
    assert L.sbwtgpu_index_setop(ia.handle, ib.handle, 1, 1, capi.C.byref(out), None) == capi.OK
    assert same_bits(capi._take_bits(out), brute_setop(sa, sb, k, "intersection", True, True)[0])
    # an op out of range
    for op in (-1, 4, 100):
        with pytest.raises(capi.SbwtGpuError) as e:
            ia.setop(ib, op)
        assert e.value.code == capi.ERR_INVALID_ARG and "operation" in e.value.msg
    unchanged()
    # cap_bytes too small: an error, the two numbers, and not a byte written
    n, kb = capi.C.c_int64(0), capi.C.c_int(0)
    buf = np.full(ia.n_kmers + 16, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    assert L.sbwtgpu_index_kmer_keys(ia.handle, buf.ctypes.data, 8 * ia.n_kmers - 1, capi.C.byref(n), capi.C.byref(kb)) == capi.ERR_INVALID_ARG
    assert "cap_bytes" in L.sbwtgpu_last_error().decode() and (n.value, kb.value) == (ia.n_kmers, 8)
    assert np.all(buf == np.uint64(0xA5A5A5A5A5A5A5A5))
    assert L.sbwtgpu_index_kmer_keys(ia.handle, None, 0, capi.C.byref(n), capi.C.byref(kb)) == capi.OK and n.value == ia.n_kmers
    assert L.sbwtgpu_index_kmer_keys(ia.handle, buf.ctypes.data, 8 * ia.n_kmers, capi.C.byref(n), capi.C.byref(kb)) == capi.OK
    assert np.array_equal(buf[:ia.n_kmers], ia.kmer_keys()) and np.all(buf[ia.n_kmers:] == np.uint64(0xA5A5A5A5A5A5A5A5))
    unchanged()
    # a rank-only index
    w = np.random.default_rng(1).integers(0, 2**64, size=4, dtype=np.uint64)
    ro = capi.Index.create(w, w, w, w, None, 256, k)
    with pytest.raises(capi.SbwtGpuError) as e:
        ia.setop(ro, "union")
    assert e.value.code == capi.ERR_INVALID_ARG and "only rank()" in e.value.msg
    # after successes too
    for op in OPS:
        ia.setop(ib, op)
    unchanged()


def test_dummy_limit(gpu):
    """The builder's host-side limit n_nopred x k <= 2^26, met by a difference of two well-connected indexes: a is one
    genome, b the same genome with every 65th base substituted, k = 64.  Of a's k-mers only every 65th is free of a
    substitution, so a minus b is one run of 64 k-mers per substitution, each run with one predecessor-less k-mer: 2^20 + 2^12
    of them x 64 exceed 2^26.  (No smaller pair of indexes reaches the limit: a result with that many predecessor-less
    k-mers has them in a, whose columns they are.)"""
    k = 64
    n_sub = (1 << 20) + (1 << 12)
    g = synth.random_genome(65 * n_sub + k, 31)
    h = g.copy()
    pos = np.arange(n_sub, dtype=np.int64) * 65 + 64
    code = np.zeros(256, dtype=np.uint8)
    code[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4, dtype=np.uint8)
    h[pos] = np.frombuffer(b"ACGT", dtype=np.uint8)[(code[g[pos]] + 1) & 3]
    capi.set_tuning("image_level", 2)
    try:
        ia = index_of(capi.build_bits_gpu([g.tobytes()], k, False, True), k)
        ib = index_of(capi.build_bits_gpu([h.tobytes()], k, False, True), k)
    finally:
        capi.set_tuning("image_level", 0)
    c = ia.setop_counts(ib)
    assert c["n_a"] == c["n_b"] == len(g) - k + 1 and c["n_a"] - c["n_both"] == 64 * n_sub
    with pytest.raises(capi.SbwtGpuError) as e:
        ia.setop(ib, "difference")
    assert e.value.code == capi.ERR_OOM and "2^26" in e.value.msg and "fragmented" in e.value.msg
    assert e.value.info["n_nopred"] == n_sub and e.value.info["n_result"] == 64 * n_sub
    assert e.value.info["n_nopred"] * k > (1 << 26)
    # both inputs answer as before, and an operation below the limit still works
    q = g[: 3 * 65 + k]
    ra, _ = ia.search(q, np.array([0, len(q)]))
    rb, _ = ib.search(q, np.array([0, len(q)]))
    assert ra.min() >= 0 and int((rb >= 0).sum()) == 3 + 1
    again = ia.setop_counts(ib)
    assert {f: again[f] for f in COUNT_KEYS} == {f: c[f] for f in COUNT_KEYS}


def test_determinism(gpu):
    rng = random.Random(8)
    for k in (14, 50):
        sa, sb = overlapping_sets(rng, k)
        _, ia = make_index(sa, k, True)
        _, ib = make_index(sb, k, True)
        for op in OPS:
            r1, i1 = ia.setop(ib, op)
            r2, i2 = ia.setop(ib, op)
            assert same_bits(r1, r2) and all(a.tobytes() == b.tobytes() for a, b in zip(r1.cols + [r1.ssup], r2.cols + [r2.ssup]))
            assert {f: i1[f] for f in i1 if f != "pass_ms"} == {f: i2[f] for f in i2 if f != "pass_ms"}
        assert ia.kmer_keys().tobytes() == ia.kmer_keys().tobytes()


def test_cli_set_op(gpu, tmp_path):
    d = str(tmp_path)
    k = 17
    rng = random.Random(12)
    pool = ["".join(rng.choice("ACGT") for _ in range(rng.randint(k, 400))) for _ in range(30)] + ["ACGT"]
    sa, sb = pool[:20], pool[10:] + [pool[0][5:60]]
    for name, seqs in (("a", sa), ("b", sb), ("ab", sa + sb)):
        with open("%s/%s.fna" % (d, name), "w") as fh:
            for i, s in enumerate(seqs):
                fh.write(">%d\n%s\n" % (i, s))
        p = subprocess.run([SBWT, "build", "-i", "%s/%s.fna" % (d, name), "-o", "%s/%s.sbwt" % (d, name), "-k", str(k),
                            "--precalc-length", "5"], capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode()
    p = subprocess.run([SBWT, "set-op", "-a", d + "/a.sbwt", "-b", d + "/b.sbwt", "--op", "union", "-o", d + "/u.sbwt",
                        "--precalc-length", "5"], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    assert open(d + "/u.sbwt", "rb").read() == open(d + "/ab.sbwt", "rb").read()
    assert b"Jaccard" in p.stderr + p.stdout
    # another operation, read back through the index file
    p = subprocess.run([SBWT, "set-op", "-a", d + "/a.sbwt", "-b", d + "/b.sbwt", "--op", "difference", "-o", d + "/d.sbwt",
                        "--precalc-length", "5"], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    f = hostlib.read_index_file(d + "/d.sbwt")
    want = brute_setop(sa, sb, k, "difference")[0]
    assert (f.n_nodes, f.n_kmers) == (want.n_nodes, want.n_kmers)
    assert all(np.array_equal(f.cols[c], want.cols[c]) for c in range(4)) and np.array_equal(f.ssup, want.ssup)
    p = subprocess.run([SBWT, "set-op", "-a", d + "/a.sbwt", "-b", d + "/b.sbwt", "--counts-only"], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    c = brute_counts(sa, sb, k)
    assert p.stdout.decode().split() == [str(c[f]) for f in COUNT_KEYS]
    p = subprocess.run([SBWT, "set-op", "-a", d + "/a.sbwt", "-b", d + "/b.sbwt", "--op", "nonsense", "-o", d + "/x.sbwt"],
                       capture_output=True, timeout=300)
    assert p.returncode != 0 and b"unknown set operation" in p.stderr
    p = subprocess.run([SBWT], capture_output=True, timeout=60)
    assert b"set-op" in p.stderr + p.stdout
