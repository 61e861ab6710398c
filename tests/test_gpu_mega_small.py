"""GPU: the mega-block count layout (sbwt_device.h) on real SBWTs, through a TEST build of the library whose mega blocks hold
2^12 columns instead of 2^31 (sbwt_amd/lib/libsbwtgpu_mega12.so, built by sbwt_amd/build.py from the same sources with
-DSBWT_MEGA_SHIFT=12).  An index of 200 k columns then spans some 50 mega blocks with distinct non-zero 64-bit bases, and
every kernel's MEGA / WIDE instantiation runs with the index arithmetic (pos >> SHIFT, blk >> (SHIFT - 6), the c * n_mega
stride) that the product build only meets beyond 2^31 columns.

The library is loaded by a fresh child per index case (tests/mega_small_worker.py, under its own `timeout -k 10`): it proves
from the version string which build it loaded, calls the library and stores raw outputs.  Inputs and expectations are made
here -- seeded synth generators, the CPU host builder, the oracle and numpy -- and everything is compared here, bit for bit.
A child that fails, or is killed, fails every test of its case with its output; neither it nor the child of another case is
started after that.

Two images per case where it says so: the default one (relative 32-bit counts + the mega table, blocks and dense table
only: what an index beyond 2^32 - 2^24 columns gets), and "big_path" 2 (absolute counts, a mega table of zeros, the full
image from the builders' <true> instantiations: what the 2.25 x 10^9-column index of test_gpu_fullsize.py gets)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sbwt_verify as V
from oracle import OracleIndex
from sbwt_amd import capi, hostlib, synth
from test_gpu_parity import oracle_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "mega_small_worker.py")
SHIFT = 12
MB = 1 << SHIFT
LIB = os.path.join(ROOT, "sbwt_amd", "lib", "libsbwtgpu_mega%d.so" % SHIFT)
MARKER = "mega_shift=%d" % SHIFT
CHILD_LIMIT = 240                       # seconds; a child takes 5-20
NT = max(1, min(16, len(os.sched_getaffinity(0))))
SYMS = np.frombuffer(b"ACGT", dtype=np.uint8)
VARIANTS = [-1, 0, 1, 4, 5]             # every "search_variant" (include/sbwtgpu.h; 2 and 3 mean 4), -1 = the image's default
ENTRY_POINTS = ("h64", "h32", "d64", "d32")
GUARD, FILL = 64, 77                    # (mega_small_worker.py)
ALL = ["rank", "select", "kmers", "forward", "update_interval", "partial", "precalc", "search", "ms", "adopt"]
NO_FWD = [w for w in ALL if w != "forward"]           # forward needs the file's marks (SBWT.hh:368)


def big_image():
    return dict(name="big", tunings=[["big_path", 2]], restore=[["big_path", 1]], do=["search", "ms"])


# name -> (k, marks in the file, kind of input, images)
CASES = {
    "k31_marks": (31, True, "genomes", [dict(name="rel", do=ALL), big_image()]),
    "k31_no_marks": (31, False, "genomes", [dict(name="rel", tunings=[["derive_ssup", 1]], do=NO_FWD),
                                            dict(name="underived", tunings=[["derive_ssup", 0]], restore=[["derive_ssup", 1]],
                                                 do=["rank", "update_interval", "search", "ms"])]),
    "k63_no_marks": (63, False, "genomes", [dict(name="rel", do=NO_FWD), big_image()]),
    "k20_marks": (20, True, "genomes", [dict(name="rel", do=ALL)]),
    "reads_k31": (31, True, "reads", [dict(name="rel", do=ALL)]),
}
IMAGES = [(c, cfg["name"]) for c in CASES for cfg in CASES[c][3]]


def bits_of(words, n):
    return np.unpackbits(np.ascontiguousarray(words, dtype=np.uint64).view(np.uint8), bitorder="little")[:n]


def ones_before(bits):
    """before[p] = ones in [0, p), for p in 0 .. n."""
    return np.concatenate([[0], np.cumsum(bits, dtype=np.int64)])


def boundary_positions(n, rng, n_random):
    """Every multiple of the mega block and its neighbours -1, +1, +63, +64, every multiple of 64, every position of the last
    two blocks, n, and random ones."""
    m = np.arange(0, n + 1, MB, dtype=np.int64)
    pos = np.concatenate([m, m - 1, m + 1, m + 63, m + 64, np.arange(0, n + 1, 64), np.arange(max(0, (n // 64 - 1) * 64), n + 1),
                          [n], rng.integers(0, n + 1, size=n_random)]).astype(np.int64)
    return pos[(pos >= 0) & (pos <= n)]


def dirty(bases, seed):
    """One base in 400 an N, one in 400 lower case."""
    b = synth.inject(bases, max(1, len(bases) // 400), ord("N"), seed)
    at = np.random.default_rng(seed + 1).integers(0, len(b), size=max(1, len(b) // 400))
    b[at] |= 0x20
    return b


def partial_search_queries(g, rng):
    """The query mix of test_gpu_api_neighbours.test_partial_search_batch."""
    queries = []
    for _ in range(3000):
        L = int(rng.integers(0, 80))
        s = int(rng.integers(0, len(g) - 100))
        q = bytearray(g[s:s + L].tobytes())
        r = rng.random()
        if L and r < 0.3:
            q[int(rng.integers(0, L))] = ord("ACGT"[int(rng.integers(0, 4))])
        elif L and r < 0.4:
            q[int(rng.integers(0, L))] = ord("N")
        elif L and r < 0.5:
            q = bytearray(bytes(q).lower())
        queries.append(bytes(q))
    return queries + [b"", b"N", b"a", b"$", b"ACGT" * 30]


def update_interval_queries(orc, g, seq_starts, rng):
    """5000 starting intervals (those of 0-12 genome bases; one in 30 is (-1, -1)) extended by the 0-40 bases that follow, some
    with a substitution, an N or a lower-case base; and the whole range extended by 1-30 bases from the start of a
    sequence, which ends on that prefix's `$`-padded column."""
    n = orc.n_nodes
    first, second, ext = [], [], []
    for _ in range(5000):
        s = int(rng.integers(0, len(g) - 60))
        l0, le = int(rng.integers(0, 13)), int(rng.integers(0, 41))
        f, sec = orc.update_interval(g[s:s + l0].tobytes(), 0, n - 1)
        e = bytearray(g[s + l0:s + l0 + le].tobytes())
        r = rng.random()
        if le and r < 0.15:
            e[int(rng.integers(0, le))] = ord("ACGT"[int(rng.integers(0, 4))])
        elif le and r < 0.20:
            e[int(rng.integers(0, le))] = ord("N")
        elif le and r < 0.25:
            e[int(rng.integers(0, le))] |= 0x20
        if r > 0.967:
            f, sec = -1, -1
        first.append(f), second.append(sec), ext.append(bytes(e))
    for s in seq_starts:
        first.append(0), second.append(n - 1), ext.append(g[s:s + int(rng.integers(1, 31))].tobytes())
    return np.array(first, dtype=np.int64), np.array(second, dtype=np.int64), ext


def prepare(case):
    """(inputs of the child, expectations) of one index case."""
    k, marks, kind, configs = CASES[case]
    seed = 1000 + 17 * k + (0 if marks else 5)
    if kind == "genomes":
        g0 = synth.random_genome(60_000, seed)
        sources = [g0, synth.mutate(g0, 0.03, seed + 1)]
        seqs, rc = [g.tobytes() for g in sources], True
        src = np.concatenate(sources)
        seq_starts = [0, 60_000]
    else:                                   # 20 k unrelated reads of 40 bases: three columns in four are `$`-padded
        rb, ro = synth.random_reads(20_000, 40, seed)
        seqs, rc = V.split_reads(rb, ro), False
        src, sources = rb, [rb]
        seq_starts = list(range(0, 2000 * 40, 40))
    bits = hostlib.build_bits(seqs, k, rc, marks, n_threads=NT)
    n = bits.n_nodes
    orc = OracleIndex.from_bits(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, n, k, bits.n_kmers, 6)
    rng = np.random.default_rng(seed + 2)
    inp = dict(A=bits.cols[0], C=bits.cols[1], G=bits.cols[2], T=bits.cols[3])
    if marks:
        inp["ssup"] = bits.ssup
    exp = dict(n=n, n_mega=(n >> SHIFT) + 1, k=k, marks=marks)
    rows = [bits_of(bits.cols[c], n) for c in range(4)]
    before = [ones_before(r) for r in rows]
    ones = [np.flatnonzero(r) for r in rows]
    Carr = np.cumsum([1] + [len(o) for o in ones])
    assert list(Carr[:4]) == orc.C
    # rank: the five symbols at every position of the list
    pos = boundary_positions(n, rng, 20_000)
    inp["rank_pos"] = np.tile(pos, 5)
    inp["rank_sym"] = np.repeat(np.frombuffer(b"ACGTN", dtype=np.uint8), len(pos))
    exp["rank"] = np.concatenate([before[c][pos] for c in range(4)] + [np.zeros(len(pos), dtype=np.int64)])
    chk = rng.integers(0, len(inp["rank_pos"]), size=2000)
    assert np.array_equal(orc.batch_rank(inp["rank_pos"][chk], inp["rank_sym"][chk])[0], exp["rank"][chk])
    # select: every one of every row; one past the last is refused
    inp["sel_j"] = np.concatenate([np.arange(1, len(o) + 1, dtype=np.int64) for o in ones])
    inp["sel_sym"] = np.concatenate([np.full(len(o), SYMS[c], dtype=np.uint8) for c, o in enumerate(ones)])
    exp["select"] = np.concatenate(ones)
    inp["sel_bad_j"] = np.array([len(o) + 1 for o in ones], dtype=np.int64)
    inp["sel_bad_sym"] = SYMS.copy()
    # get_kmer: every column, from the rows by the definition-level verifier
    lab, _, _ = V.labels_from_rows(bits.cols, n, k)
    exp["kmers"] = V.labels_ascii(lab, k, 0, n)
    chk = rng.integers(0, n, size=300)
    assert all(exp["kmers"][v].tobytes() == orc.get_kmer(int(v)) for v in chk)
    # forward: every (column, symbol) pair and every column with an N.  numpy on the rows (the start of the column's suffix
    # group, the bit there, C[c] + ones before it); the oracle's forward on a seeded sample of 20 000 pairs vouches for it
    if marks:
        sg = bits_of(bits.ssup, n).astype(bool)
        start = np.maximum.accumulate(np.where(sg, np.arange(n), 0))
        inp["fwd_node"] = np.tile(np.arange(n, dtype=np.int64), 5)
        inp["fwd_sym"] = np.repeat(np.frombuffer(b"ACGTN", dtype=np.uint8), n)
        exp["forward"] = np.concatenate([np.where(rows[c][start] == 1, Carr[c] + before[c][start], -1) for c in range(4)]
                                        + [np.full(n, -1, dtype=np.int64)])
        chk = rng.integers(0, 4 * n, size=20_000)
        assert np.array_equal(exp["forward"][chk], np.array([orc.forward(int(inp["fwd_node"][i]), bytes([int(inp["fwd_sym"][i])]))
                                                             for i in chk]))
    # update_interval
    f0, s0, ext = update_interval_queries(orc, src, seq_starts, rng)
    inp["ui_first"], inp["ui_second"] = f0, s0
    inp["ui_bases"], inp["ui_off"] = capi.concat_reads(ext)
    want = [orc.update_interval(e, int(a), int(b)) for e, a, b in zip(ext, f0, s0)]
    exp["ui_first"], exp["ui_second"] = (np.array([w[j] for w in want], dtype=np.int64) for j in (0, 1))
    # partial_search
    qs = partial_search_queries(src, rng)
    inp["ps_bases"], inp["ps_off"] = capi.concat_reads(qs)
    want = [orc.partial_search(q) for q in qs]
    exp["ps_first"], exp["ps_second"], exp["ps_matched"] = (np.array(x, dtype=np.int64) for x in
                                                            ([w[0][0] for w in want], [w[0][1] for w in want], [w[1] for w in want]))
    exp["precalc"] = orc.precalc()
    # search: reads of 150, of 250 and of 20-700 bases with 1 % substitutions, N and lower case, and random reads
    batches = [synth.sample_reads(sources, 300, 150, 0.01, seed + 3), synth.sample_reads(sources, 150, 250, 0.01, seed + 4),
               synth.ragged_reads(sources, 150, 20, 700, 0.01, seed + 5), synth.random_reads(100, 150, seed + 6)]
    batches = [(dirty(b, seed + 7 + j) if j < 3 else b, o) for j, (b, o) in enumerate(batches)]
    exp["n_batches"] = len(batches)
    for j, (b, o) in enumerate(batches):
        inp["sb%d_bases" % j], inp["sb%d_off" % j] = b, o
        exp["search/b%d/s0" % j] = oracle_batch(orc, b, o, False)
        if marks:
            exp["search/b%d/s1" % j] = oracle_batch(orc, b, o, True)
    # matching statistics and the LCS array, on the same reads
    inp["ms_bases"] = np.concatenate([b for b, _ in batches])
    shift = np.cumsum([0] + [len(b) for b, _ in batches])
    inp["ms_off"] = np.concatenate([batches[0][1]] + [o[1:] + shift[j] for j, (_, o) in enumerate(batches) if j > 0])
    exp["ms_len"], exp["ms_first"], exp["ms_second"] = orc.matching_statistics(inp["ms_bases"], inp["ms_off"], n_threads=NT)[:3]
    exp["lcs"] = orc.lcs(n_threads=NT)
    for cfg in configs:
        cfg.setdefault("variants", VARIANTS)
        cfg.setdefault("streaming", [1, 0] if marks else [0])
    inp["meta"] = np.array(json.dumps(dict(mode="sbwt", marker=MARKER, k=k, n_nodes=n, n_kmers=bits.n_kmers, precalc_k=6,
                                           n_batches=len(batches), configs=configs)))
    return inp, exp


RANK_ONLY_SIZES = [MB - 1, MB, MB + 1, 5 * MB, 5 * MB + 63, 1_000_003]
RANK_ONLY_BATCHES = [1, 2, 3, 5, 7, 1023, 20_001]          # n % 4 != 0: the scalar tail beside the 4-wide kernel


def prepare_rank_only():
    inp, exp = {}, {}
    for i, n_bits in enumerate(RANK_ONLY_SIZES):
        rng = np.random.default_rng(n_bits)
        nw = (n_bits + 63) // 64
        cols = [rng.integers(0, 2**64, size=nw, dtype=np.uint64) for _ in range(4)]
        before = [ones_before(bits_of(c, n_bits)) for c in cols]
        code = np.full(256, 4, dtype=np.int64)
        code[SYMS] = np.arange(4)
        for c, ch in enumerate("ACGT"):
            inp["r%d_%s" % (i, ch)] = cols[c]
        for j, m in enumerate(RANK_ONLY_BATCHES):
            pos = rng.integers(0, n_bits + 1, size=m)
            if m == 20_001:                                # every mega block boundary and its neighbours among them
                edge = boundary_positions(n_bits, rng, 0)
                edge = edge[rng.permutation(len(edge))[:m - 1]]
                pos[:len(edge)] = edge
            pos[0], pos[-1] = n_bits, 0
            sym = rng.choice(np.frombuffer(b"ACGTNacgt$\x00\xff", dtype=np.uint8), size=m)
            inp["r%d_pos%d" % (i, j)], inp["r%d_sym%d" % (i, j)] = pos.astype(np.int64), sym
            table = np.stack(before + [np.zeros(n_bits + 1, dtype=np.int64)])
            exp["r%d_out%d" % (i, j)] = table[code[sym], pos]
    inp["meta"] = np.array(json.dumps(dict(mode="rank_only", marker=MARKER, sizes=RANK_ONLY_SIZES, n_batches=len(RANK_ONLY_BATCHES))))
    return inp, exp


class Run:
    def __init__(self, exp, out):
        self.exp, self.out = exp, out


@pytest.fixture(scope="module")
def children(gpu, tmp_path_factory):
    """children(case) -> Run: prepares the case, runs its child ONCE (the result, or the failure, is kept for the module)."""
    # (the module takes 35 s on an MI355X: 5 s per case -- the oracle 1-2 s, the child 3-4 s -- charged to the case's first test)
    done = {}

    def get(case):
        if case not in done:
            # a child that died may have faulted the GPU: no further child is started, in this case or another
            died = [c for c in done if isinstance(done[c], str)]
            done[case] = start(case) if not died else "not started: the child of case %s failed before:\n%s" % (died[0], done[died[0]])
        if isinstance(done[case], str):
            pytest.fail(done[case], pytrace=False)
        return done[case]

    def start(case):
        if not os.path.exists(LIB):
            return "%s is missing: build it with `python -m sbwt_amd.build`" % LIB
        inp, exp = prepare_rank_only() if case == "rank_only" else prepare(case)
        d = tmp_path_factory.mktemp("mega_" + case)
        fin, fout = str(d / "in.npz"), str(d / "out.npz")
        np.savez(fin, **inp)
        env = dict(os.environ, SBWTGPU_LIB=LIB)
        p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, WORKER, fin, fout], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        if p.returncode != 0 or not os.path.exists(fout):
            return "the child of case %s ended with status %d (124 / 137: time limit); its output:\n%s" % (
                case, p.returncode, p.stdout.decode(errors="replace")[-6000:])
        out = np.load(fout, allow_pickle=False)
        assert MARKER in str(out["version"])
        return Run(exp, out)
    return get


def same(got, want, label):
    """Equal arrays, or the first differing slot in the message."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (label, "%d entries differ, first at %s: got %s want %s"
                           % (len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def info(run, image):
    return json.loads(str(run.out[image + "/info"]))


def does(case, image, what):
    return [cfg for cfg in CASES[case][3] if cfg["name"] == image and what in cfg["do"]] != []


def images_doing(what):
    return [im for im in IMAGES if does(im[0], im[1], what)]


# ---- the cases reach every mega block ----
@pytest.mark.parametrize("case", list(CASES))
def test_expected_columns_reach_every_mega_block(children, case):
    """The oracle's found columns and interval ends fall into at least n_mega - 1 mega blocks, and the index has dozens."""
    e = children(case).exp
    cols = [e[key] for key in e if key.startswith("search/")] + [e["ui_first"], e["ui_second"], e["ps_first"], e["ps_second"],
                                                                 e["ms_first"], e["ms_second"]]
    cols = np.concatenate(cols)
    touched = np.unique(cols[cols >= 0] >> SHIFT)
    assert e["n_mega"] >= 40 and len(touched) >= e["n_mega"] - 1, (e["n"], e["n_mega"], len(touched))
    found = np.concatenate([e[key] for key in e if key.startswith("search/")])
    assert 0.1 < (found >= 0).mean() < 0.95


@pytest.mark.parametrize("case,image", IMAGES)
def test_image_is_the_one_meant(children, case, image):
    """Default "big_path": blocks and dense table only, relative counts -- not the fused route.  "big_path" 2: the full image."""
    run = children(case)
    i = info(run, image)
    assert i["n_nodes"] == run.exp["n"] and i["has_streaming_support"] == run.exp["marks"] and i["precalc_k"] == 6
    if image == "big":
        assert i["image_level"] == 0 and i["default_search_variant"] == 5 and i["n_paths"] > 0, i
    else:
        assert i["n_paths"] == 0 and i["image_level"] == 2 and i["default_search_variant"] != 5, i


# ---- the default image: relative counts, one base per mega block ----
@pytest.mark.parametrize("case,image", images_doing("rank"))
def test_rank(children, case, image):
    run = children(case)
    same(run.out[image + "/rank"], run.exp["rank"], (case, image))


@pytest.mark.parametrize("case,image", images_doing("select"))
def test_select_every_one_of_every_row(children, case, image):
    run = children(case)
    same(run.out[image + "/select"], run.exp["select"], (case, image))
    assert list(run.out[image + "/select_bad_rc"]) == [capi.ERR_INVALID_ARG] * 4


@pytest.mark.parametrize("case,image", images_doing("kmers"))
def test_get_kmer_every_column(children, case, image):
    """As test_gpu_build_scale.column_api_equals_numpy: the labels the definition-level verifier reads back from the rows."""
    run = children(case)
    same(run.out[image + "/kmers"], run.exp["kmers"], (case, image))
    if case == "reads_k31":
        assert (run.exp["kmers"][:, -1] == ord("$")).sum() == 1 and (run.exp["kmers"][:, 0] == ord("$")).mean() > 0.7


@pytest.mark.parametrize("case,image", images_doing("forward"))
def test_forward_every_column_and_symbol(children, case, image):
    """EVERY (column, symbol) pair, and every column with an N, against numpy on the rows; prepare() checks that expectation
    against the oracle's forward on a seeded sample of 20 000 pairs (the oracle takes a call per pair)."""
    run = children(case)
    same(run.out[image + "/forward"], run.exp["forward"], (case, image))
    want = run.exp["forward"]
    assert len(np.unique(want[want >= 0])) == run.exp["n"] - 1          # every column but the root is somebody's successor


@pytest.mark.parametrize("case,image", images_doing("update_interval"))
def test_update_interval(children, case, image):
    run = children(case)
    same(run.out[image + "/ui_first"], run.exp["ui_first"], (case, image, "first"))
    same(run.out[image + "/ui_second"], run.exp["ui_second"], (case, image, "second"))
    assert 0.2 < (run.exp["ui_first"] >= 0).mean() < 0.95


@pytest.mark.parametrize("case,image", images_doing("partial"))
def test_partial_search(children, case, image):
    run = children(case)
    for what in ("ps_first", "ps_second", "ps_matched"):
        same(run.out[image + "/" + what], run.exp[what], (case, image, what))


@pytest.mark.parametrize("case,image", images_doing("precalc"))
def test_prefix_table_computed_on_the_device(children, case, image):
    run = children(case)
    same(run.out[image + "/precalc"], run.exp["precalc"], (case, image))
    assert (run.exp["precalc"][:, 0] >= 0).mean() > 0.9


@pytest.mark.parametrize("case,image", images_doing("search"))
def test_search_every_variant_and_entry_point(children, case, image):
    """streaming_search and search, every "search_variant", host and device entry points, int64 and int32 results, results
    poisoned first; the device arrays' guard slots keep their fill."""
    run = children(case)
    cfg = [c for c in CASES[case][3] if c["name"] == image][0]
    for b in range(run.exp["n_batches"]):
        for s in cfg["streaming"]:
            want = run.exp["search/b%d/s%d" % (b, s)]
            for v in cfg["variants"]:
                for ep in ENTRY_POINTS:
                    got = run.out["%s/search/b%d/v%d/s%d/%s" % (image, b, v, s, ep)]
                    assert got.dtype == (np.int32 if ep.endswith("32") else np.int64)
                    if ep[0] == "d":
                        assert len(got) == len(want) + GUARD and (got[len(want):] == FILL).all(), (case, image, b, s, v, ep)
                        got = got[:len(want)]
                    same(got.astype(np.int64), want, (case, image, b, s, v, ep))


@pytest.mark.parametrize("case,image", images_doing("ms"))
def test_matching_statistics_and_lcs(children, case, image):
    run = children(case)
    same(run.out[image + "/lcs"], run.exp["lcs"], (case, image, "lcs"))
    for what in ("ms_len", "ms_first", "ms_second"):
        same(run.out[image + "/" + what], run.exp[what], (case, image, what))
    same(run.out[image + "/ms_len_only"], run.exp["ms_len"], (case, image, "len only"))
    assert 0.05 < (run.exp["ms_len"] == run.exp["k"]).mean() < 0.95


@pytest.mark.parametrize("case,image", images_doing("adopt"))
def test_exported_image_adopted(children, case, image):
    """index_export_header + copy_blob -> index_adopt: the header carries n_mega, the replica answers the same."""
    run = children(case)
    hdr = run.out[image + "/header"]
    # SbwtBlobHeader (sbwt_device.h): magic, n_nodes, n_kmers, k, p_file, p_dev, C[4], n_blocks, n_mega -- 8 bytes each
    fields = hdr[:96].view(np.int64)
    assert (fields[1], fields[3], fields[10], fields[11]) == (run.exp["n"], run.exp["k"], run.exp["n"] // 64 + 1, run.exp["n_mega"])
    for s in ([1, 0] if run.exp["marks"] else [0]):
        same(run.out["%s/adopt/s%d" % (image, s)], run.exp["search/b0/s%d" % s], (case, image, s))
    same(run.out[image + "/adopt/rank"], run.exp["rank"], (case, image, "rank"))


# ---- rank-only images of arbitrary bit vectors ----
@pytest.mark.parametrize("i", range(len(RANK_ONLY_SIZES)), ids=[str(s) for s in RANK_ONLY_SIZES])
def test_rank_only_bit_vectors(children, i):
    """Four unrelated random rows of 2^12 - 1 .. 10^6 bits: one mega block, exactly two, a last one of 0, 1 or 63 columns."""
    run = children("rank_only")
    for j in range(len(RANK_ONLY_BATCHES)):
        same(run.out["r%d_out%d" % (i, j)], run.exp["r%d_out%d" % (i, j)], (RANK_ONLY_SIZES[i], RANK_ONLY_BATCHES[j]))
