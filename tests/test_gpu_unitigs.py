"""GPU: the unitig export (sbwt_unitigs.hip) byte for byte against the brute-force restatement of its definition
(tests/unitig_brute.py), as the inverse of the builders, as a permutation of the real columns under streaming_search, and
through the C++ CLI."""
import gzip
import json
import os
import random
import subprocess

import numpy as np
import pytest

from bruteforce import BruteSBWT
from unitig_brute import brute_unitigs, flatten
from unitig_numpy import graph, key_set
from sbwt_amd import capi, hostlib, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_kats.json")))


def as_bytes(seqs):
    return [s.encode() if isinstance(s, str) else s for s in seqs]


def make_index(seqs, k, rc=False, ssup=True):
    bits = hostlib.build_bits(as_bytes(seqs), k, rc, ssup)
    return bits, capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k,
                                   bits.n_kmers, 0)


def split(bases, off):
    b = bases.tobytes()
    return [b[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def check_brute(idx, seqs, k, rc, label):
    """Index.unitigs() == the brute force, byte for byte; returns the API result."""
    B = BruteSBWT([s.decode() if isinstance(s, bytes) else s for s in seqs], k, rc)
    U, first = brute_unitigs(B)
    want_bases, want_off = flatten(U)
    bases, off, first_col = idx.unitigs()
    assert idx.n_nodes == len(B.nodes), label
    assert off.tolist() == want_off, label
    assert bases.tobytes() == want_bases, label
    assert first_col.tolist() == first, label
    return bases, off, first_col


def check_permutation(idx, bits, bases, off, first_col, k):
    """streaming_search over the unitigs: no -1, unitig i starts at first_col[i], every real column exactly once."""
    res, out_off = idx.streaming_search(bases, off)
    assert len(res) == bits.n_kmers
    if len(res) == 0:
        return
    assert res.min() >= 0
    assert np.array_equal(res[out_off[:-1]], first_col)
    got = np.sort(res)
    assert np.all(got[1:] > got[:-1])
    # the real columns are those get_kmer labels without '$': on small indexes compare the sets themselves
    if idx.n_nodes <= 5000:
        labels = idx.get_kmers(np.arange(idx.n_nodes, dtype=np.int64)).reshape(idx.n_nodes, k)
        real = np.nonzero(~(labels == ord("$")).any(axis=1))[0]
        assert np.array_equal(got, real)


def check_round_trip(bits, bases, off, k, host=False):
    """build(unitigs) with add_revcomp = 0 == the index, bit for bit."""
    seqs = split(bases, off)
    back = hostlib.build_bits(seqs, k, False, True) if host else capi.build_bits_gpu(seqs, k, False, True)
    assert (back.n_nodes, back.n_kmers) == (bits.n_nodes, bits.n_kmers)
    for c in range(4):
        assert np.array_equal(back.cols[c], bits.cols[c]), "ACGT"[c]
    if bits.ssup is not None:
        assert np.array_equal(back.ssup, bits.ssup)


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


def test_reference_inputs(gpu):
    c = KATS["cli_end_to_end"]
    bits, idx = make_index(c["seqs"], c["k"], c["add_reverse_complements"])
    b, o, f = check_brute(idx, c["seqs"], c["k"], c["add_reverse_complements"], "cli_end_to_end")
    check_permutation(idx, bits, b, o, f, c["k"])
    check_round_trip(bits, b, o, c["k"])
    c = KATS["redundant_dummies"]
    bits, idx = make_index(c["seqs"], c["k"])
    b, o, f = check_brute(idx, c["seqs"], c["k"], False, "redundant_dummies")
    check_round_trip(bits, b, o, c["k"])
    for case in KATS["small_cases"]["cases"]:
        bits, idx = make_index(case["seqs"], case["k"])
        b, o, f = check_brute(idx, case["seqs"], case["k"], False, case["name"])
        check_permutation(idx, bits, b, o, f, case["k"])
        if case["k"] >= 2:
            check_round_trip(bits, b, o, case["k"])


@pytest.mark.parametrize("k", [2, 3, 4, 5, 8, 16, 31, 32, 33, 63, 64])
@pytest.mark.parametrize("rc", [False, True])
def test_random_sets(gpu, k, rc):
    rng = random.Random(100 * k + rc)
    seqs = random_seqs(rng, k)
    bits, idx = make_index(seqs, k, rc)
    b, o, f = check_brute(idx, seqs, k, rc, (k, rc))
    check_permutation(idx, bits, b, o, f, k)
    check_round_trip(bits, b, o, k)
    with idx.unitigs_dev() as u:
        assert u.n_kmers == bits.n_kmers and u.n_unitigs == len(f) and u.total_bases == len(b)


def circular(s, k):
    return s + s[:k - 1]


@pytest.mark.parametrize("k", [3, 8, 31])
def test_pure_cycles(gpu, k):
    rng = random.Random(k)

    def rnd(n):
        return "".join(rng.choice("ACGT") for _ in range(n))
    one, two = rnd(k + 20), rnd(k + 33)
    cases = {
        "one cycle": [circular(one, k)],
        "two cycles": [circular(one, k), circular(two, k)],
        "self-loop": ["A" * (k + 3)],
        "self-loop and cycle": ["C" * k, circular(one, k)],
        "cycle and tail": [rnd(k + 4) + circular(one, k)],
    }
    if k == 3:                # (random strings of 23 bases repeat 2-mers: the hand-written cycles instead)
        cases = {"one cycle": [circular("ACGT", 3)], "two cycles": [circular("ACGT", 3), circular("AAG", 3)],
                 "self-loop": ["AAAAA"], "cycle and tail": ["CACGTACG"]}
    for name, seqs in cases.items():
        for rc in (False, True):
            bits, idx = make_index(seqs, k, rc)
            b, o, f = check_brute(idx, seqs, k, rc, (name, rc))
            check_permutation(idx, bits, b, o, f, k)
            check_round_trip(bits, b, o, k)
    if k == 3:
        _, idx = make_index(cases["one cycle"], 3)
        assert split(*idx.unitigs()[:2]) == [b"GTACGT"]
    else:
        _, idx = make_index(cases["one cycle"], k)
        b, o, f = idx.unitigs()
        assert len(f) == 1 and len(b) == len(one) + k - 1                    # one unitig, not closed again
        _, idx = make_index(cases["cycle and tail"], k)
        assert len(idx.unitigs()[2]) == 2                                    # the tail, and the cycle from where it enters


def test_image_layouts_and_marks(gpu):
    rng = random.Random(77)
    for k in (4, 15, 31, 40):
        seqs = random_seqs(rng, k) + [circular("".join(rng.choice("ACGT") for _ in range(k + 9)), k)]
        bits, idx = make_index(seqs, k, True)
        want = check_brute(idx, seqs, k, True, k)
        variants = []
        for key, val, back in (("image_level", 1, 0), ("image_level", 2, 0), ("force_mega", 1, 0), ("big_path", 2, 1)):
            capi.set_tuning(key, val)
            try:
                variants.append(((key, val), make_index(seqs, k, True)[1]))
            finally:
                capi.set_tuning(key, back)
        for derive in (1, 0):           # no marks given: derived into the image, or into the call's scratch
            capi.set_tuning("derive_ssup", derive)
            try:
                for level in (0, 2):
                    capi.set_tuning("image_level", level)
                    variants.append((("no marks", derive, level), make_index(seqs, k, True, ssup=False)[1]))
            finally:
                capi.set_tuning("derive_ssup", 1)
                capi.set_tuning("image_level", 0)
        for name, other in variants:
            got = other.unitigs()
            for a, b in zip(want, got):
                assert np.array_equal(a, b), (k, name)


def test_determinism_and_bounds(gpu):
    import torch
    rng = random.Random(5)
    seqs = random_seqs(rng, 21)
    bits, idx = make_index(seqs, 21, True)
    b1, o1, f1 = idx.unitigs()
    b2, o2, f2 = idx.unitigs()
    assert np.array_equal(b1, b2) and np.array_equal(o1, o2) and np.array_equal(f1, f2)
    with idx.unitigs_dev() as u:
        n, total = u.n_unitigs, u.total_bases
        # guard bytes around the caller's host buffers
        G = 64
        hb = np.full(total + 2 * G, 0xA5, dtype=np.uint8)
        ho = np.full(n + 1 + 2 * G, -7, dtype=np.int64)
        hf = np.full(n + 2 * G, -7, dtype=np.int64)
        capi._check(capi.lib().sbwtgpu_unitigs_copy(u._h, hb[G:].ctypes.data, ho[G:].ctypes.data, hf[G:].ctypes.data))
        for arr, m, fill in ((hb, total, 0xA5), (ho, n + 1, -7), (hf, n, -7)):
            assert np.all(arr[:G] == fill) and np.all(arr[G + m:] == fill)
        assert np.array_equal(hb[G:G + total], b1) and np.array_equal(ho[G:G + n + 1], o1) and np.array_equal(hf[G:G + n], f1)
        # first_col may be NULL
        ho2 = np.empty(n + 1, dtype=np.int64)
        capi._check(capi.lib().sbwtgpu_unitigs_copy(u._h, hb[G:].ctypes.data, ho2.ctypes.data, None))
        assert np.array_equal(ho2, o1)
        # the device pointers hold the same bytes
        d_b, d_o, d_f = u.dev_ptrs()

        def alias(ptr, count, typestr):
            class _Alias:
                __cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (ptr, False), "version": 3, "strides": None}
            return torch.as_tensor(_Alias(), device=torch.device("cuda", 0)).cpu().numpy()
        assert np.array_equal(alias(d_b, total, "|u1"), b1)
        assert np.array_equal(alias(d_o, n + 1, "<i8"), o1) and np.array_equal(alias(d_f, n, "<i8"), f1)


def test_long_unitig(gpu):
    k = 31
    g = synth.random_genome(300_000, 11)
    bits = capi.build_bits_gpu([g.tobytes()], k, False, True)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)
    with idx.unitigs_dev() as u:
        b, o, f = u.copy()
        rounds = u.stats()["jump_rounds"]
    assert o.tolist() == [0, len(g)] and np.array_equal(b, g)
    assert f.tolist() == [int(idx.streaming_search(g[:k], np.array([0, k]))[0][0])]
    n_bits = int(np.ceil(np.log2(idx.n_nodes)))
    assert 18 <= rounds <= n_bits + 2, rounds


def test_long_pure_cycle(gpu):
    k = 31
    L = 100_000
    g = synth.random_genome(L, 12)
    s = np.concatenate([g, g[:k - 1]])
    bits = capi.build_bits_gpu([s.tobytes()], k, False, True)
    assert bits.n_kmers == L
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)
    with idx.unitigs_dev() as u:
        b, o, f = u.copy()
        rounds = u.stats()["jump_rounds"]
    assert rounds <= int(np.ceil(np.log2(idx.n_nodes))) + 2
    assert o.tolist() == [0, L + k - 1]
    # the rotation starts at the smallest column: search every k-mer of the cycle, take the argmin
    res, _ = idx.streaming_search(s, np.array([0, len(s)]))
    r = int(np.argmin(res))
    assert f.tolist() == [int(res[r])]
    assert np.array_equal(b, g[(r + np.arange(L + k - 1)) % L])
    # and the brute force says the same
    B = BruteSBWT([s.tobytes().decode()], k)
    U, first = brute_unitigs(B)
    assert [b.tobytes().decode()] == U and f.tolist() == first
    check_round_trip(bits, b, o, k)


@pytest.mark.parametrize("k", [65, 72, 80, 128, 255])
def test_round_trip_long_k_host_builder(gpu, k):
    rng = random.Random(k)
    seqs = ["".join(rng.choice("ACGT") for _ in range(rng.randint(k, 400))) for _ in range(6)]
    seqs.append(circular("".join(rng.choice("ACGT") for _ in range(k + 50)), k))
    for rc in (False, True):
        bits, idx = make_index(seqs, k, rc)
        b, o, f = check_brute(idx, seqs, k, rc, (k, rc))
        check_permutation(idx, bits, b, o, f, k)
        check_round_trip(bits, b, o, k, host=True)


def test_moderate_scale(gpu):
    k = 31
    genomes = synth.coli3_like(700_000, 0.01)
    seqs = [g.tobytes() for g in genomes]
    bits = capi.build_bits_gpu(seqs, k, True, True)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)
    with idx.unitigs_dev() as u:
        b, o, f = u.copy()
        assert u.n_kmers == bits.n_kmers
        assert u.stats()["jump_rounds"] <= int(np.ceil(np.log2(idx.n_nodes))) + 2
    assert np.all(f[1:] > f[:-1])
    check_permutation(idx, bits, b, o, f, k)
    check_round_trip(bits, b, o, k)
    # the start rule over packed 62-bit k-mers (tests/unitig_numpy.py): x is a start unless it has exactly one in-neighbour
    # whose out-degree is 1
    K = key_set(list(genomes) + [synth.revcomp(g) for g in genomes], k)
    assert len(K) == bits.n_kmers
    n_starts = int(graph(K, k)[1].sum())
    # (a pure cycle would add a unitig without a start: three random genomes hold none)
    assert len(f) == n_starts


def test_errors_and_empty(gpu):
    w = np.random.default_rng(1).integers(0, 2**64, size=4, dtype=np.uint64)
    ro = capi.Index.create(w, w, w, w, None, 256, 3)                           # arbitrary bits: a rank-only index
    with pytest.raises(capi.SbwtGpuError) as e:
        ro.unitigs()
    assert e.value.code == capi.ERR_INVALID_ARG and "only rank()" in e.value.msg
    for seqs in (["ACG"], ["ACGTNACGT", "acgtacgtacgt"]):
        bits, idx = make_index(seqs, 6)
        assert bits.n_kmers == 0
        b, o, f = idx.unitigs()
        assert len(b) == 0 and o.tolist() == [0] and len(f) == 0
        with idx.unitigs_dev() as u:
            assert (u.n_unitigs, u.total_bases, u.n_kmers) == (0, 0, 0)


def test_cli_dump_unitigs(gpu, tmp_path):
    d = str(tmp_path)
    c = KATS["cli_end_to_end"]
    k = c["k"]
    with open(d + "/in.fna", "w") as fh:
        for i, s in enumerate(c["seqs"]):
            fh.write(">%d\n%s\n" % (i, s))
    cmd = [SBWT, "build", "-i", d + "/in.fna", "-o", d + "/i.sbwt", "-k", str(k)]
    cmd += ["--add-reverse-complements"] if c["add_reverse_complements"] else []
    p = subprocess.run(cmd, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    _, idx = make_index(c["seqs"], k, c["add_reverse_complements"])
    b, o, f = idx.unitigs()
    want = b"".join(b">%d\n%s\n" % (i, u) for i, u in enumerate(split(b, o)))
    assert len(f) > 0
    for z in (False, True):
        out = d + "/u.fna" + (".gz" if z else "")
        p = subprocess.run([SBWT, "dump-unitigs", "-i", d + "/i.sbwt", "-o", out] + (["-z"] if z else []), capture_output=True,
                           timeout=300)
        assert p.returncode == 0, p.stderr.decode()
        assert (gzip.open(out).read() if z else open(out, "rb").read()) == want, z


def test_mega_block_layout(gpu, tmp_path):
    """The MEGA instantiations, through the test build with mega blocks of 2^12 columns (a fresh child loads it): an index
    of some 40 mega blocks gives the bytes the product build gives."""
    import sys
    lib = os.path.join(ROOT, "sbwt_amd", "lib", "libsbwtgpu_mega12.so")
    assert os.path.exists(lib), "%s is missing: build it with `python -m sbwt_amd.build`" % lib
    k = 31
    g0 = synth.random_genome(40_000, 5)
    seqs = [g0.tobytes(), synth.mutate(g0, 0.03, 6).tobytes()]
    bits = hostlib.build_bits(seqs, k, True, True)
    assert (bits.n_nodes >> 12) >= 30
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, k, bits.n_kmers, 0)
    want = idx.unitigs()
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, A=bits.cols[0], C=bits.cols[1], G=bits.cols[2], T=bits.cols[3], ssup=bits.ssup,
             meta=np.array([bits.n_nodes, k, bits.n_kmers], dtype=np.int64))
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tests", "unitig_mega_worker.py"), fin, fout],
                       env=dict(os.environ, SBWTGPU_LIB=lib), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-4000:]
    out = np.load(fout, allow_pickle=False)
    assert "mega_shift=12" in str(out["version"])
    for image in ("rel1", "rel0", "big1", "big0"):
        for a, key in zip(want, ("bases", "off", "first")):
            assert np.array_equal(a, out["%s/%s" % (image, key)]), (image, key)
