"""GPU fuzz of the derived queries: on random indexes (the shapes of tools/fuzz_gpu.py and two more, k from 2 to 64, with and
without reverse complements, marks, a prefix table, the image knobs) every answer of the column API (get_kmers, select, rank,
forward, partial_search, update_interval), the LCS array, matching statistics, read hits on one and two strands, the unitigs
and the set operations with a second random index is held bit for bit against a value computed on the CPU: the oracle, numpy
on the rows, the host builder and the brute forces of tests/.

The module has two halves.  The first draws a case and computes every expected value and imports nothing of the GPU path
(tests/test_fuzz_derived_cpu.py runs it alone); the second runs sbwt_amd.capi and compares.  A case's draws depend on
(seed, case number) alone, so one case replays without the ones before it.

Usage: SEED=n python tools/fuzz_derived.py [cases] [case_no]       (case_no: that case alone)
tests/test_gpu_fuzz_derived.py runs fuzz() under the -m gpu suite."""
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from sbwt_amd import hostlib, synth                      # noqa: E402
from oracle import OracleIndex                           # noqa: E402
from bruteforce import BruteSBWT                         # noqa: E402
import ms_brute                                          # noqa: E402
import read_hits_brute                                   # noqa: E402
import setop_brute                                       # noqa: E402
import unitig_brute                                      # noqa: E402
import unitig_numpy                                      # noqa: E402


class FuzzMismatch(AssertionError):
    pass


K_CHOICES = [2, 3, 4, 7, 12, 16, 21, 30, 31, 32, 33, 40, 63, 64]
SHAPES = ("single", "related", "tandem", "short", "star", "periodic", "k_and_k1")
B_KINDS = ("mutated", "subset_plus", "cut", "same", "foreign")
EXTRA_KNOBS = (("force_mega", 1, 0), ("big_path", 2, 1), ("derive_ssup", 0, 1))          # (key, drawn value, default)
FEATURES = ("get_kmers", "select", "rank", "forward", "partial_search", "update_interval", "lcs", "ms", "ms_lengths", "ms_brute",
            "read_hits_1", "read_hits_2", "unitigs_numpy", "unitigs_brute", "unitigs_round_trip", "unitigs_permutation",
            "kmer_keys", "setop_counts", "setops", "setop_device_index")
# what tests/test_gpu_fuzz_derived.py runs and tests/test_fuzz_derived_cpu.py replays: chosen on the CPU so that every category of
# the latter occurs in three cases at least, N_CASES so that a seed's expected values take about 5 s
SEEDS = (13, 23, 24, 33, 38, 44)
N_CASES = 5
MAX_KMERS = 60_000          # k-mers of index A (reverse complements included); MAX_KMERS_BRUTE above k = 31, where the brute
MAX_KMERS_BRUTE = 18_000    # force is the unitigs' only reference (it takes 20 000)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.arange(256, dtype=np.uint8)
COMP[ACGT] = np.frombuffer(b"TGCA", dtype=np.uint8)


# =====================================================================================================================
# First half: the draws and the expected values (CPU only)
# =====================================================================================================================
def seed_of(rng):
    return int(rng.integers(1, 1 << 30))


def draw_case(seed, case_no):
    """Everything a case draws: the sequences of A and B, the knobs, the reads, the queries' random choices."""
    rng = np.random.default_rng([seed, case_no])
    c = types.SimpleNamespace(seed=seed, no=case_no)
    k = c.k = int(rng.choice(K_CHOICES))
    c.shape = int(rng.integers(0, len(SHAPES)))
    c.rc = bool(rng.integers(0, 2))
    c.marks = bool(rng.integers(0, 2))
    c.precalc = int(rng.choice([0, 2, min(k, 8)]))
    glen = int(rng.integers(2_000, 30_001))
    # the drawn length is cut so that the index stays below MAX_KMERS k-mers, strands and strains counted
    n_strains = {1: 2, 4: 5}.get(c.shape, 1)
    glen = max(2_000, min(glen, (MAX_KMERS_BRUTE if k > 31 else MAX_KMERS) // (n_strains * (2 if c.rc else 1))))
    g0 = synth.random_genome(glen, seed_of(rng))
    name = SHAPES[c.shape]
    if name == "single":
        genomes = [g0]
    elif name == "related":
        genomes = [g0, synth.mutate(g0, float(rng.choice([0.001, 0.01, 0.05])), seed_of(rng))]
    elif name == "tandem":            # tandem repeats and a low-complexity stretch
        unit = g0[: int(rng.integers(3, 40))]
        genomes = [np.concatenate([g0[:500], np.tile(unit, 60), g0[500:1500], np.frombuffer(b"AC" * 200, dtype=np.uint8), g0[1500:]])]
    elif name == "short":             # several short sequences (many dummy nodes)
        genomes = [g0[i:i + int(rng.integers(k, 4 * k + 10))].copy() for i in range(0, min(glen, 20_000), 997)]
    elif name == "star":              # star of related genomes
        genomes = [g0] + [synth.mutate(g0, 0.02, seed_of(rng)) for _ in range(4)]
    elif name == "periodic":          # one to three purely periodic sequences: cycles and a dummy chain
        genomes = []
        for _ in range(int(rng.choice([1, 1, 2, 3]))):
            u = int(rng.integers(1, 41))
            a = int(rng.integers(0, glen - u))
            total = max(3 * k, u + k) + int(rng.integers(1, 200))
            genomes.append(np.tile(g0[a:a + u], total // u + 1)[:total].copy())
    else:                             # sequences of exactly k and k + 1 bases: every k-mer with its own dummy path
        genomes, pos, i = [], 0, 0
        while pos + k + 1 <= glen:
            genomes.append(g0[pos:pos + k + (i & 1)].copy())
            pos += k + (i & 1) + int(rng.integers(0, 3))
            i += 1
    c.injected = int(rng.integers(0, 4)) == 0
    if c.injected:                    # N and lower-case bytes in the input: the builders take runs of upper-case ACGT
        genomes = [g.copy() for g in genomes]
        for _ in range(int(rng.integers(1, 8))):
            g = genomes[int(rng.integers(0, len(genomes)))]
            p = int(rng.integers(0, len(g)))
            g[p] = ord("N") if rng.integers(0, 2) else (g[p] | 0x20)
    c.genomes = genomes
    c.seqs = [g.tobytes() for g in genomes]
    # knobs that must not change results
    c.knobs = {"path_lookahead": int(rng.choice([0, 1, 8])), "path_safe": int(rng.choice([0, 1, 2, 2])),
               "image_level": int(rng.choice([0, 0, 0, 1, 2])), "path_stitch": int(rng.choice([1, 1, 1, 0])),
               "path_stitch_min": int(rng.choice([1, 1, 4, 16]))}
    c.extra_knob = EXTRA_KNOBS[int(rng.integers(0, len(EXTRA_KNOBS)))] if int(rng.integers(0, 4)) == 0 else None
    # ---- index B ----
    c.b_kind = int(rng.integers(0, len(B_KINDS)))
    c.rc_b = bool(rng.integers(0, 2))
    c.marks_b = bool(rng.integers(0, 2))
    kind = B_KINDS[c.b_kind]
    foreign = synth.random_genome(min(glen, 8_000), seed_of(rng))
    if kind == "mutated":
        rate = float(rng.uniform(0.01, 0.05))
        gb = [synth.mutate(g, rate, seed_of(rng)) for g in genomes]
    elif kind == "subset_plus":       # a proper subset of A's sequences, and foreign ones
        if len(genomes) >= 2:
            keep = rng.permutation(len(genomes))[: int(rng.integers(1, len(genomes)))]
            gb = [genomes[int(i)] for i in sorted(keep)]
        else:
            gb = [genomes[0][: len(genomes[0]) // 2]]
        gb = gb + [foreign[:3000], foreign[3000:]]
    elif kind == "cut":               # the pieces between random cuts: the k-mers across a cut go, every piece starts a dummy path
        gb = []
        for g in genomes:
            cuts = np.sort(rng.integers(0, len(g) + 1, size=int(rng.integers(1, 6))))
            gb += [g[a:b] for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(g)]]))]
    elif kind == "same":              # A itself through a second handle
        gb, c.rc_b = list(genomes), c.rc
    else:
        gb = [foreign]
    c.seqs_b = [g.tobytes() for g in gb]
    c.device_index_of = int(rng.integers(0, 4)) if int(rng.integers(0, 3)) == 0 else None        # an operation, one case in three
    # ---- reads ----
    cat = np.concatenate(genomes)
    nr = int(rng.integers(300, 1501))
    if rng.integers(0, 2):
        L = int(rng.integers(max(k - 2, 1), int(rng.choice([4 * k + 60, 480, 1500]))))
        L = min(L, max(len(g) for g in genomes))
        bases, off = synth.sample_reads([g for g in genomes if len(g) >= L], nr, L, float(rng.choice([0, 0.005, 0.02, 0.1])), seed_of(rng))
    else:                             # ragged lengths from 0
        lens = np.minimum(rng.integers(0, int(rng.choice([3 * k + 40, 330, 460, 2000])), size=nr), len(cat))
        st = (rng.random(nr) * (len(cat) - lens + 1)).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        bases = cat[np.repeat(st - off[:-1], lens) + np.arange(int(off[-1]), dtype=np.int64)] if off[-1] else np.zeros(0, np.uint8)
        flip = rng.random(len(bases)) < 0.01
        bases[flip] = ACGT[rng.integers(0, 4, size=int(flip.sum()))]
    parts = [bases[off[r]:off[r + 1]] for r in range(len(off) - 1)]
    if rng.integers(0, 4) == 0:       # a few long reads, some with lower-case stretches
        extra = []
        for _ in range(int(rng.integers(1, 12))):
            ln = int(min(rng.integers(260, 6000), len(cat)))
            s0 = int(rng.integers(0, len(cat) - ln + 1))
            rd = cat[s0:s0 + ln].copy()
            for _ in range(int(rng.integers(0, 4))):
                a0 = int(rng.integers(0, ln))
                a1 = min(ln, a0 + int(rng.integers(1, 400)))
                rd[a0:a1] |= 0x20
            extra.append(rd)
        pos = int(rng.integers(0, len(parts) + 1))
        parts[pos:pos] = extra
    parts[1::2] = [COMP[p[::-1]] for p in parts[1::2]]          # every other read from the reverse strand
    bases = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    if len(bases) > 100:
        bases = synth.inject(bases, int(rng.integers(0, 30)), ord("N"), seed_of(rng))
        bases = synth.inject(bases, int(rng.integers(0, 30)), int(rng.choice(list(b"acgtn"))), seed_of(rng))
    c.bases, c.off = np.ascontiguousarray(bases), off
    c.read_hits_tuning = ((int(rng.choice([1, 64, 128, 300])), int(rng.choice([1, 1000, 20_000])))
                          if int(rng.integers(0, 3)) == 0 else None)            # (read_hits_wave_min, read_hits_chunk_bases)
    c.query_seed = seed_of(rng)
    return c


def unpack_rows(cols, n):
    return [np.unpackbits(np.ascontiguousarray(w).view(np.uint8), bitorder="little")[:n] for w in cols]


def partial_search_queries(g, rng, n=500):
    """The query mix of test_gpu_mega_small.partial_search_queries."""
    queries = []
    for _ in range(n):
        L = int(rng.integers(0, 80))
        s = int(rng.integers(0, max(len(g) - 100, 1)))
        q = bytearray(g[s:s + L].tobytes())
        L = len(q)
        r = rng.random()
        if L and r < 0.3:
            q[int(rng.integers(0, L))] = ord("ACGT"[int(rng.integers(0, 4))])
        elif L and r < 0.4:
            q[int(rng.integers(0, L))] = ord("N")
        elif L and r < 0.5:
            q = bytearray(bytes(q).lower())
        queries.append(bytes(q))
    return queries + [b"", b"N", b"a", b"$", b"ACGT" * 30]


def update_interval_queries(orc, g, seq_starts, rng, n=500):
    """The mix of test_gpu_mega_small.update_interval_queries: starting intervals of 0-12 bases (one in 30 is (-1, -1)),
    extended by the 0-40 bases that follow; and the whole range extended from the start of a sequence."""
    nn = orc.n_nodes
    first, second, ext = [], [], []
    for _ in range(n):
        s = int(rng.integers(0, max(len(g) - 60, 1)))
        l0, le = int(rng.integers(0, 13)), int(rng.integers(0, 41))
        f, sec = orc.update_interval(g[s:s + l0].tobytes(), 0, nn - 1)
        e = bytearray(g[s + l0:s + l0 + le].tobytes())
        le = len(e)
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
        first.append(0), second.append(nn - 1), ext.append(g[s:s + int(rng.integers(1, 31))].tobytes())
    return np.array(first, dtype=np.int64), np.array(second, dtype=np.int64), ext


def concat(reads):
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), off


def out_offsets(off, k):
    return np.concatenate([[0], np.cumsum(np.maximum(np.diff(off) - k + 1, 0))]).astype(np.int64)


def expected(c, n_threads=16):
    """Every expected value of a case, from the CPU alone; e.applies: the features the case compares; e.tags: what the case
    is an example of (tests/test_fuzz_derived_cpu.py counts them)."""
    e = types.SimpleNamespace(applies=set(FEATURES), tags=set(), ref_checks=0)
    k = c.k
    bits = e.bits = hostlib.build_bits(c.seqs, k, c.rc, True, n_threads=4)
    bits_b = e.bits_b = hostlib.build_bits(c.seqs_b, k, c.rc_b, True, n_threads=4)
    n = bits.n_nodes
    assert n <= 200_000 and bits_b.n_nodes <= 200_000 and len(c.bases) <= 2_000_000
    orc = e.orc = OracleIndex.from_bits(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, n, k, bits.n_kmers, 0)
    rows = unpack_rows(bits.cols, n)
    rng = np.random.default_rng(c.query_seed)
    # ---- column API ----
    e.labels = np.frombuffer(b"".join(orc.get_kmer(j) for j in range(n)), dtype=np.uint8).reshape(n, k)
    real_cols = np.flatnonzero(~(e.labels == ord("$")).any(axis=1))
    assert len(real_cols) == bits.n_kmers
    ones = [np.flatnonzero(r) for r in rows]
    cum = [np.concatenate([[0], np.cumsum(r, dtype=np.int64)]) for r in rows]
    m = 2000
    # select: (j, symbol) with 1 <= j <= ones of the row, both ends included; a symbol without a row gives 0
    row = rng.integers(0, 5, size=m)
    row[:8] = [0, 0, 1, 1, 2, 2, 3, 3]
    row = np.where((row < 4) & (np.array([len(o) for o in ones] + [1])[row] == 0), 4, row)          # (a row without ones: no valid j)
    cnt = np.array([len(o) for o in ones] + [5])[row]
    j = rng.integers(1, cnt + 1)
    j[:8:2], j[1:8:2] = 1, cnt[1:8:2]
    e.select_j = j.astype(np.int64)
    e.select_sym = np.where(row < 4, np.frombuffer(b"ACGTN", dtype=np.uint8)[row], rng.choice(np.frombuffer(b"N$a", dtype=np.uint8), size=m))
    e.select_want = np.array([ones[r][jj - 1] if r < 4 else 0 for r, jj in zip(row, j)], dtype=np.int64)
    # ... and outside it the documented refusal: j = 0 and j = ones + 1 (of the first row that has ones)
    r0 = int(np.argmax([len(o) > 0 for o in ones]))
    e.select_refused = [(0, b"ACGT"[r0]), (len(ones[r0]) + 1, b"ACGT"[r0])]
    # rank: pos in [0, n_nodes], non-ACGT symbols give 0
    pos = rng.integers(0, n + 1, size=m)
    pos[0], pos[1], pos[-1] = n, n, 0
    syms = np.frombuffer(b"ACGTNacgt$\x00\xff", dtype=np.uint8)
    e.rank_pos, e.rank_sym = pos.astype(np.int64), rng.choice(syms, size=m)
    e.rank_sym[0], e.rank_sym[1] = ord("T"), ord("N")
    code = np.full(256, 4, dtype=np.int64)
    code[ACGT] = np.arange(4)
    cum5 = np.stack(cum + [np.zeros(n + 1, dtype=np.int64)])
    e.rank_want = cum5[code[e.rank_sym], e.rank_pos]
    # forward
    node = rng.integers(0, n, size=m)
    node[0], node[-1] = 0, n - 1
    e.fwd_node, e.fwd_sym = node.astype(np.int64), rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=m)
    e.fwd_want = np.array([orc.forward(int(a), bytes([int(s)])) for a, s in zip(e.fwd_node, e.fwd_sym)], dtype=np.int64)
    # partial_search, update_interval
    cat = np.concatenate(c.genomes)
    e.ps_queries = partial_search_queries(cat, rng)
    w = [orc.partial_search(q) for q in e.ps_queries]
    e.ps_want = (np.array([x[0][0] for x in w]), np.array([x[0][1] for x in w]), np.array([x[1] for x in w]))
    starts = np.concatenate([[0], np.cumsum([len(g) for g in c.genomes])])[:-1][:20]
    e.ui_first, e.ui_second, e.ui_ext = update_interval_queries(orc, cat, [int(s) for s in starts], rng)
    w = [orc.update_interval(q, int(f), int(s)) for q, f, s in zip(e.ui_ext, e.ui_first, e.ui_second)]
    e.ui_want = (np.array([x[0] for x in w]), np.array([x[1] for x in w]))
    # ---- LCS, matching statistics ----
    e.lcs = orc.lcs(n_threads=n_threads)
    e.ms = orc.matching_statistics(c.bases, c.off, n_threads=n_threads)[:3]
    B = None
    strs = [s.decode("latin-1") for s in c.seqs]
    if k <= 16 and n < 3000:
        B = BruteSBWT(strs, k, c.rc)
        assert len(B.nodes) == n
        M = ms_brute.BruteMS(B)
        L, F, S = [], [], []
        for r in range(len(c.off) - 1):
            a, b, s_ = M.read(c.bases[c.off[r]:c.off[r + 1]].tobytes())
            L += a
            F += b
            S += s_
        e.ms_brute = (np.array(L, dtype=np.uint8), np.array(F, dtype=np.int64), np.array(S, dtype=np.int64))
        e.lcs_brute = np.array(ms_brute.lcs_array(B), dtype=np.uint8)
        # the two references against each other
        for name, a, b in zip(("len", "first", "second"), e.ms, e.ms_brute):
            assert np.array_equal(a, b), ("oracle and brute-force matching statistics differ", c.seed, c.no, name)
        assert np.array_equal(e.lcs, e.lcs_brute), ("oracle and brute-force LCS differ", c.seed, c.no)
        e.ref_checks += 1
        e.tags.add("ms_brute")
    else:
        e.applies.discard("ms_brute")
    # ---- read hits: reduce_hits over the oracle's search, the second strand from the mirrored batch ----
    # (the oracle without marks: its batch_search is then the per-k-mer search, for which a window holding a lower-case byte
    # is absent -- the definition of a hit; the streaming search upper-cases the base it steps by, as the reference does)
    plain = OracleIndex.from_bits(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], None, n, k, bits.n_kmers, 0)
    oo = out_offsets(c.off, k)
    hit = plain.batch_search(c.bases, c.off, oo, n_threads)[0] >= 0
    T = len(c.bases)
    roff = (T - c.off[::-1]).astype(np.int64)
    rhit = (plain.batch_search(np.ascontiguousarray(COMP[c.bases[::-1]]), roff, out_offsets(roff, k), n_threads)[0] >= 0)[::-1]
    e.hits = {1: read_hits_brute.reduce_hits(hit, oo, k), 2: read_hits_brute.reduce_hits(hit | rhit, oo, k)}
    # ---- unitigs ----
    e.unitigs = {}
    if k <= 31:
        arrs = list(c.genomes) + ([COMP[g[::-1]] for g in c.genomes] if c.rc else [])
        K = unitig_numpy.key_set(arrs, k)
        assert len(K) == bits.n_kmers
        ub, uo, first = unitig_numpy.unitigs_of_keys(K, k)
        e.unitigs["numpy"] = (ub, uo, real_cols[first])
    else:
        e.applies.discard("unitigs_numpy")
    if bits.n_kmers <= 20_000:
        B = B or BruteSBWT(strs, k, c.rc)
        U, first = unitig_brute.brute_unitigs(B)
        ub, uo = unitig_brute.flatten(U)
        e.unitigs["brute"] = (np.frombuffer(ub, dtype=np.uint8), np.array(uo, dtype=np.int64), np.array(first, dtype=np.int64))
    else:
        e.applies.discard("unitigs_brute")
    assert e.unitigs, "no unitig reference applies"
    if len(e.unitigs) == 2:
        for a, b in zip(e.unitigs["numpy"], e.unitigs["brute"]):
            assert np.array_equal(a, b), ("numpy and brute-force unitigs differ", c.seed, c.no)
        e.ref_checks += 1
        e.tags.add("unitig_refs_both")
    # ---- set operations ----
    KA, KB = setop_brute.kmers_of(c.seqs, k, c.rc), setop_brute.kmers_of(c.seqs_b, k, c.rc_b)
    assert len(KA) == bits.n_kmers and len(KB) == bits_b.n_kmers
    e.keys_a, e.keys_b = setop_brute.packed_keys(KA, k), setop_brute.packed_keys(KB, k)
    e.counts = {"n_a": len(KA), "n_b": len(KB), "n_both": len(KA & KB), "n_either": len(KA | KB)}
    e.setops = {}
    for op in setop_brute.OPS:
        R = setop_brute.apply_op(KA, KB, op)
        want = setop_brute.build_from_kmers(R, k, True)
        assert want.n_kmers == len(R)
        e.setops[op] = (want, R)
        e.tags.add("op_empty" if not R else "op_equals_a" if R == KA else "op_between" if R < KA else "op_other")
    if c.device_index_of is not None:
        op = setop_brute.OPS[c.device_index_of]
        if e.setops[op][0].n_nodes > 200_000:
            op = "intersection"
        e.device_op = op
        e.device_keys = setop_brute.packed_keys(e.setops[op][1], k)
        e.tags.add("device_index")
    else:
        e.applies.discard("setop_device_index")
    # ---- what the case is an example of ----
    t = e.tags
    t.add("shape_" + SHAPES[c.shape])
    t.add("b_" + B_KINDS[c.b_kind])
    for cond, tag in ((k <= 4, "k<=4"), (k == 31, "k=31"), (k == 32, "k=32"), (k == 33, "k=33"), (k >= 63, "k>=63"), (c.rc, "rc"),
                      (not c.marks, "no_marks"), (c.injected, "injected"), (c.precalc > 0, "precalc")):
        if cond:
            t.add(tag)
    for key, default in (("path_lookahead", 8), ("path_safe", 2), ("image_level", 0), ("path_stitch", 1), ("path_stitch_min", 1)):
        if c.knobs[key] != default:
            t.add("%s=%d" % (key, c.knobs[key]))
    if c.extra_knob:
        t.add("%s=%d" % c.extra_knob[:2])
    if c.read_hits_tuning:
        t.add("read_hits_tuning")
    per_col = rows[0].astype(np.int64) + rows[1] + rows[2] + rows[3]
    if int((per_col >= 2).sum()) >= 50:
        t.add("branching>=50")
    if 3 * (n - bits.n_kmers) > n:
        t.add("dummy_heavy")
    if bits.n_kmers > 0 and n == bits.n_kmers + 1 and int(per_col.sum()) == bits.n_kmers and int(per_col.max()) == 1:
        t.add("pure_cycle")         # no dummy but the root, every k-mer with one successor: the graph is disjoint cycles
    lens = np.diff(c.off)
    if (e.hits[1] != e.hits[2]).any():
        t.add("strands_differ")
    for cond, tag in (((lens - k + 1 >= 4096).any(), "windows>=4096"), (((lens > 0) & (lens < k)).any(), "read<k"), ((lens == 0).any(), "empty_read")):
        if cond:
            t.add(tag)
    n_unitigs = len(next(iter(e.unitigs.values()))[2])
    t.add("unitigs>=2" if n_unitigs >= 2 else "unitigs=1" if n_unitigs == 1 else "unitigs=0")
    return e


# =====================================================================================================================
# Second half: the GPU path against the expected values
# =====================================================================================================================
def reset_tuning():
    from sbwt_amd import capi
    capi.set_tuning("path_lookahead", 8); capi.set_tuning("path_safe", 2); capi.set_tuning("image_level", 0)
    capi.set_tuning("path_stitch", 1); capi.set_tuning("path_stitch_min", 1)
    for key, _, default in EXTRA_KNOBS:
        capi.set_tuning(key, default)
    capi.set_tuning("read_hits_wave_min", 1024); capi.set_tuning("read_hits_chunk_bases", 0)


def fuzz(seed, n_cases, stats=None, only=None):
    """Checks cases 1 .. n_cases of `seed` (only: that case number alone); returns the number of cases checked.  Raises
    FuzzMismatch with seed, case, feature and the first differing element.  stats: a dict that receives "cases",
    "applies" and "compared" (feature -> number of cases the feature applies to / was compared in) and "cpu_seconds"
    (the expected values) / "seconds" (everything)."""
    stats = {} if stats is None else stats
    stats.update(cases=0, applies={f: 0 for f in FEATURES}, compared={f: 0 for f in FEATURES}, cpu_seconds=0.0, seconds=0.0)
    t0 = time.time()
    try:
        for no in range(1, n_cases + 1) if only is None else [only]:
            c = draw_case(seed, no)
            t1 = time.time()
            e = expected(c)
            stats["cpu_seconds"] += time.time() - t1
            for f in e.applies:
                stats["applies"][f] += 1
            run_case(c, e, stats["compared"])
            stats["cases"] += 1
    finally:
        reset_tuning()
        stats["seconds"] = time.time() - t0
    return stats["cases"]


def run_case(c, e, compared):
    from sbwt_amd import capi
    k, bits, bits_b = c.k, e.bits, e.bits_b
    where = "seed %d case %d (k %d, shape %s, rc %s, marks %s, precalc %d, knobs %s %s, B %s)" % (
        c.seed, c.no, k, SHAPES[c.shape], c.rc, c.marks, c.precalc, c.knobs, c.extra_knob, B_KINDS[c.b_kind])

    def differ(feature, what, got, want, element=None):
        """raises at the first difference of two arrays; element(i) names the read / column / unitig of flat index i"""
        got, want = np.asarray(got), np.asarray(want)
        if got.shape != want.shape:
            raise FuzzMismatch("MISMATCH %s: %s has shape %s, want %s; %s" % (feature, what, got.shape, want.shape, where))
        bad = np.flatnonzero(got.ravel() != want.ravel())
        if len(bad):
            i = int(bad[0])
            raise FuzzMismatch("MISMATCH %s: %s differs at %s (element %d, %d in all): got %s want %s; %s" % (
                feature, what, element(i) if element else "element %d" % i, i, len(bad), got.ravel()[i], want.ravel()[i], where))

    def same_bits(feature, what, got, want, marks):
        if (got.n_nodes, got.n_kmers) != (want.n_nodes, want.n_kmers):
            raise FuzzMismatch("MISMATCH %s: %s has n_nodes %d n_kmers %d, want %d %d; %s" % (
                feature, what, got.n_nodes, got.n_kmers, want.n_nodes, want.n_kmers, where))
        if (got.ssup is not None) != marks:
            raise FuzzMismatch("MISMATCH %s: %s marks %s, asked %s; %s" % (feature, what, got.ssup is not None, marks, where))
        for r in range(4):
            differ(feature, "%s row %s (words)" % (what, "ACGT"[r]), got.cols[r], want.cols[r], lambda i: "columns %d..%d" % (64 * i, 64 * i + 63))
        if marks:
            differ(feature, "%s marks (words)" % what, got.ssup, want.ssup, lambda i: "columns %d..%d" % (64 * i, 64 * i + 63))

    def make(b, marks, precalc):
        return capi.Index.create(b.cols[0], b.cols[1], b.cols[2], b.cols[3], b.ssup if marks else None, b.n_nodes, k, b.n_kmers, precalc)

    for key, val in c.knobs.items():
        capi.set_tuning(key, val)
    if c.extra_knob:
        capi.set_tuning(c.extra_knob[0], c.extra_knob[1])
    idx = make(bits, c.marks, c.precalc)
    n = bits.n_nodes
    # ---- column API ----
    differ("get_kmers", "label", idx.get_kmers(np.arange(n, dtype=np.int64)), e.labels, lambda i: "column %d base %d" % (i // k, i % k))
    compared["get_kmers"] += 1
    differ("select", "select(j, sym)", idx.select(e.select_j, e.select_sym), e.select_want,
           lambda i: "j %d symbol %r" % (e.select_j[i], chr(e.select_sym[i])))
    for j, sym in e.select_refused:
        try:
            got = idx.select([j], [sym])
        except capi.SbwtGpuError as ex:
            if ex.code != capi.ERR_INVALID_ARG:
                raise
        else:
            raise FuzzMismatch("MISMATCH select: j %d symbol %r answered %s, want the refusal (invalid argument); %s" % (j, chr(sym), got, where))
    compared["select"] += 1
    differ("rank", "rank(pos, sym)", idx.rank(e.rank_pos, e.rank_sym), e.rank_want, lambda i: "pos %d symbol %r" % (e.rank_pos[i], chr(e.rank_sym[i])))
    compared["rank"] += 1
    if c.marks:
        differ("forward", "forward(column, sym)", idx.forward(e.fwd_node, e.fwd_sym), e.fwd_want,
               lambda i: "column %d symbol %r" % (e.fwd_node[i], chr(e.fwd_sym[i])))
    else:
        try:
            got = idx.forward(e.fwd_node, e.fwd_sym)
        except capi.SbwtGpuError as ex:
            if ex.code != capi.ERR_NO_STREAMING:
                raise
        else:
            raise FuzzMismatch("MISMATCH forward: an index without marks answered %s..., want the refusal (no streaming support); %s" % (got[:4], where))
    compared["forward"] += 1
    qb, qo = concat(e.ps_queries)
    for name, got, want in zip(("first", "second", "matched"), idx.partial_search(qb, qo), e.ps_want):
        differ("partial_search", name, got, want, lambda i: "query %d %r" % (i, e.ps_queries[i]))
    compared["partial_search"] += 1
    qb, qo = concat(e.ui_ext)
    for name, got, want in zip(("first", "second"), idx.update_interval(qb, qo, e.ui_first, e.ui_second), e.ui_want):
        differ("update_interval", name, got, want, lambda i: "query %d (%d, %d) + %r" % (i, e.ui_first[i], e.ui_second[i], e.ui_ext[i]))
    compared["update_interval"] += 1
    # ---- LCS, matching statistics ----
    got_lcs = idx.lcs()
    differ("lcs", "lcs", got_lcs, e.lcs, lambda i: "column %d" % i)
    compared["lcs"] += 1

    def base_of(i):
        r = int(np.searchsorted(c.off, i, side="right") - 1)
        return "read %d base %d" % (r, i - int(c.off[r]))
    got_ms = idx.matching_statistics(c.bases, c.off)
    for name, got, want in zip(("len", "first", "second"), got_ms, e.ms):
        differ("ms", name, got, want, base_of)
    compared["ms"] += 1
    got_len = idx.matching_statistics(c.bases, c.off, intervals=False)
    differ("ms_lengths", "len", got_len, e.ms[0], base_of)
    compared["ms_lengths"] += 1
    if "ms_brute" in e.applies:
        for name, got, want in zip(("len", "first", "second"), got_ms, e.ms_brute):
            differ("ms_brute", name, got, want, base_of)
        differ("ms_brute", "len (lengths only)", got_len, e.ms_brute[0], base_of)
        differ("ms_brute", "lcs", got_lcs, e.lcs_brute, lambda i: "column %d" % i)
        compared["ms_brute"] += 1
    # ---- read hits ----
    if c.read_hits_tuning:
        capi.set_tuning("read_hits_wave_min", c.read_hits_tuning[0])
        capi.set_tuning("read_hits_chunk_bases", c.read_hits_tuning[1])
    for strands in (1, 2):
        differ("read_hits_%d" % strands, "record (n_kmers, n_found, covered_bases, longest_run)", idx.read_hits(c.bases, c.off, strands == 2),
               e.hits[strands], lambda i: "read %d (%d bases) field %d" % (i // 4, c.off[i // 4 + 1] - c.off[i // 4], i % 4))
        compared["read_hits_%d" % strands] += 1
    capi.set_tuning("read_hits_wave_min", 1024)
    capi.set_tuning("read_hits_chunk_bases", 0)
    # ---- unitigs ----
    ub, uo, uf = idx.unitigs()
    for ref, want in e.unitigs.items():
        differ("unitigs_" + ref, "number of unitigs", [len(uf)], [len(want[2])])
        differ("unitigs_" + ref, "offsets", uo, want[1], lambda i: "unitig %d" % i)
        differ("unitigs_" + ref, "bases", ub, want[0], lambda i: "unitig %d base %d" % (np.searchsorted(uo, i, side="right") - 1, i - uo[np.searchsorted(uo, i, side="right") - 1]))
        differ("unitigs_" + ref, "first_col", uf, want[2], lambda i: "unitig %d" % i)
        compared["unitigs_" + ref] += 1
    # two properties that need no reference of the unitigs: the host builder makes A's bits of them, and the oracle's
    # streaming search over them visits every real column once, unitig i from first_col[i]
    b = ub.tobytes()
    back = hostlib.build_bits([b[uo[i]:uo[i + 1]] for i in range(len(uf))], k, False, True, n_threads=4)
    same_bits("unitigs_round_trip", "build(unitigs)", back, bits, True)
    compared["unitigs_round_trip"] += 1
    res = e.orc.batch_search(ub, uo, out_offsets(uo, k), 16)[0]
    differ("unitigs_permutation", "number of k-mers of the unitigs", [len(res)], [bits.n_kmers])
    if len(res):
        real = np.flatnonzero(~(e.labels == ord("$")).any(axis=1))
        differ("unitigs_permutation", "sorted columns of the unitigs' k-mers", np.sort(res), real, lambda i: "rank %d" % i)
        differ("unitigs_permutation", "column of the first k-mer", res[out_offsets(uo, k)[:-1]], uf, lambda i: "unitig %d" % i)
    compared["unitigs_permutation"] += 1
    # ---- set operations and keys ----
    idx_b = make(bits if B_KINDS[c.b_kind] == "same" else bits_b, c.marks_b, 0)
    key_of = (lambda i: "key %d" % i) if k <= 32 else (lambda i: "key %d word %d" % (i // 2, i % 2))
    differ("kmer_keys", "A.kmer_keys()", idx.kmer_keys(), e.keys_a, key_of)
    differ("kmer_keys", "B.kmer_keys()", idx_b.kmer_keys(), e.keys_b, key_of)
    compared["kmer_keys"] += 1
    names = ("n_a", "n_b", "n_both", "n_either")
    got = idx.setop_counts(idx_b)
    differ("setop_counts", "(n_a, n_b, n_both, n_either)", [got[f] for f in names], [e.counts[f] for f in names], lambda i: names[i])
    compared["setop_counts"] += 1
    results = {}
    for op in setop_brute.OPS:
        want, R = e.setops[op]
        for marks in (True, False):
            got, info = idx.setop(idx_b, op, marks)
            same_bits("setops", "%s (marks %s)" % (op, marks), got, want, marks)
            differ("setops", "%s info" % op, [info[f] for f in names] + [info["n_result"], got.k], [e.counts[f] for f in names] + [len(R), k],
                   lambda i: (names + ("n_result", "k"))[i])
            if not R and (got.n_nodes, got.n_kmers) != (1, 0):
                raise FuzzMismatch("MISMATCH setops: the empty %s has %d columns, want the root alone; %s" % (op, got.n_nodes, where))
            if marks:
                results[op] = got
    compared["setops"] += 1
    if "setop_device_index" in e.applies:
        r = results[e.device_op]
        made = capi.Index.create(r.cols[0], r.cols[1], r.cols[2], r.cols[3], r.ssup, r.n_nodes, k, r.n_kmers, 0)
        differ("setop_device_index", "kmer_keys() of the %s as an index" % e.device_op, made.kmer_keys(), e.device_keys, key_of)
        compared["setop_device_index"] += 1
    reset_tuning()


if __name__ == "__main__":
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    only = int(sys.argv[2]) if len(sys.argv) > 2 else None
    seed = int(os.environ.get("SEED", 1))
    st = {}
    try:
        from sbwt_amd import capi
        capi.set_tuning("poison_results", 1)
        n = fuzz(seed, n_cases, st, only)
    except FuzzMismatch as ex:
        print(ex)
        sys.exit(1)
    print("fuzz_derived ok: seed %d, %d cases, %.1f s (%.1f s of them the CPU's expected values)" % (seed, n, st["seconds"], st["cpu_seconds"]))
