"""GPU: colour select (sbwt_colorselect.hip; sbwtgpu_colorsets_match_sets / _select_counts / _select) against numpy for the
verdicts and against the definition from k-mer strings (tests/color_select_brute.py) for the selected index, bit for bit:
every row width and launch edge of the verdict kernel, both key widths, alternating survivors across wave and block edges,
the empty and the full selection, uncoloured columns beside dummy columns, uploaded objects in another numbering, the closed
loop through Index and ColorSets.merge, the old route over coloured unitigs, image levels and layouts, determinism, guard
bytes, two host threads, every refusal and the C++ CLI.  All comparisons are exact."""
import json
import os
import random
import threading

import numpy as np
import pytest

import color_select_brute as sb
import pseudoalign_brute as pb
import pseudoalign_wide as pw
import test_gpu_pseudoalign_wide as tw          # its helpers: make_index, labels_of, refused, run, as_lists
from setop_brute import build_from_kmers, same_bits
from sbwt_amd import capi, hostlib, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_kats.json")))
refused = tw.refused
COUNTS = ("n_real", "n_selected", "n_sets_matched")


def index_of(bits):
    return capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, bits.k, bits.n_kmers, 0)


def built(idx, n_colors, adds):
    """The builder's ColorSets of idx: adds = (colour, sequences, both strands)"""
    with capi.ColorSetsBuilder.create(idx, n_colors) as b:
        for c, seqs, both in adds:
            b.add_reads(c, [s.encode() for s in seqs], both)
        return b.finish()


def world(by_color, extra, k, rc, n_colors):
    """(index, builder's object, k-mer -> colours) of a coloured index over the colours' sequences and `extra`"""
    seqs, kmers, col = sb.colour_world(by_color, extra, k, rc, n_colors)
    idx = tw.make_index(seqs, k, rc)
    assert idx.n_kmers == len(kmers)
    return idx, built(idx, n_colors, [(c, by_color[c], rc) for c in sorted(by_color)]), col


def check_select(sets, col, k, pred, label, marks=True):
    """select and select_counts == the definition: bits, n_selected, n_sets_matched, n_nopred"""
    inc, exc, lo, hi = pred
    want_bits, want = sb.build(col, k, inc, exc, lo, hi, marks)
    got_bits, info = sets.select(inc, exc, lo, hi, marks)
    print(label, {f: info[f] for f in want}, want)
    assert same_bits(got_bits, want_bits), label
    assert got_bits.k == k and got_bits.n_kmers == want["n_selected"], label
    assert {f: info[f] for f in want} == want, (label, info)
    assert len(info["pass_ms"]) == 3 and all(x >= 0 for x in info["pass_ms"].values()), label
    c = sets.select_counts(inc, exc, lo, hi)
    assert {f: c[f] for f in COUNTS} == {f: want[f] for f in COUNTS} and c["n_nopred"] == 0, (label, c)
    return got_bits, info


def uploaded_colouring(labels, ids, table):
    """k-mer -> colours of an uploaded object, from the labels of the columns"""
    rows = pw.rows_ints(table)
    sets = [frozenset(c for c in range(row.bit_length()) if (row >> c) & 1) for row in rows]
    return {lab: sets[ids[j]] for j, lab in enumerate(labels) if "$" not in lab}


# ---- 1. the verdict kernel against numpy --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(gpu):
    idx = tw.make_index(["ACGTTGCATGGA"], 6)
    yield idx
    idx.close()


def random_table(rng, n_sets, C):
    """row 0 empty, no other row empty, no bit at or above C; dense and sparse rows; with room, rows that differ from their
    neighbour only in word 0 or only in the last word, and duplicate rows"""
    W = pw.n_words(C)
    t = rng.integers(0, 2**64, size=(n_sets, W), dtype=np.uint64)
    t[::3] &= rng.integers(0, 2**64, size=t[::3].shape, dtype=np.uint64) & rng.integers(0, 2**64, size=t[::3].shape, dtype=np.uint64)
    if C & 63:
        t[:, W - 1] &= np.uint64((1 << (C & 63)) - 1)
    for r in range(1, n_sets):
        t[r, (r % C) >> 6] |= np.uint64(1) << np.uint64((r % C) & 63)
    t[0] = 0
    if n_sets >= 8:
        t[3] = t[2]
        t[3, 0] ^= np.uint64(1)                                  # differs in word 0 only (bit 0: below C whatever C is)
        t[5] = t[4]
        t[5, W - 1] ^= np.uint64(1) << np.uint64((C - 1) & 63)   # differs in the last word only
        t[7] = t[6]                                              # a duplicate row
        for r in (3, 5):
            if not t[r].any():
                t[r, 0] = np.uint64(1 if C == 1 else 2)
    return t


@pytest.mark.parametrize("C", [1, 63, 64, 65, 128, 4095, 4096])
def test_match_sets_against_numpy(tiny, C):
    rng = np.random.default_rng(C)
    W = pw.n_words(C)
    L = capi.lib()
    ids = np.zeros(tiny.n_nodes, dtype=np.uint32)
    for n_sets in (1, 2, 63, 64, 65, 1000, 5000):
        table = random_table(rng, n_sets, C)
        with capi.ColorSets.from_arrays(tiny, C, ids, table) as s:          # (every row but 0 is unused: allowed)
            colours = rng.permutation(C)
            inc = sb.mask_words(sorted(colours[:max(1, C // 2)].tolist()), W)
            exc = sb.mask_words(sorted(colours[-max(1, C // 5):].tolist()), W)
            n_inc = int(sb.popcounts(inc[None, :])[0])
            full = sb.mask_words(range(C), W)
            preds = [(inc, None, 1, n_inc), (inc, exc, 0, n_inc), (inc, None, 0, 0), (inc, None, n_inc, n_inc), (inc, None, n_inc + 1, n_inc + 7),
                     (full, None, 1, C - 1 if C > 1 else 1), (full, exc, max(1, C // 3), C), (sb.mask_words([0], W), sb.mask_words([C - 1], W), 0, 1),
                     (sb.mask_words([C - 1], W), None, 1, 1)]
            # bounds in the middle of the rows' counts, and a single excluded colour: about half of the rows match
            med = int(np.median(sb.popcounts(table & inc[None, :])))
            preds += [(inc, None, med, med + 2), (inc, None, 0, med), (inc, sb.mask_words([int(colours[-1])], W), 1, n_inc)]
            mixed = 0
            for i, (a, b, lo, hi) in enumerate(preds):
                want = sb.verdicts(table, a, b, lo, hi)
                mixed += 0 < int(want.sum()) < n_sets
                got = s.match_sets(a, b, lo, hi)
                assert got.dtype == np.uint8 and np.array_equal(got, want), (C, n_sets, i, np.nonzero(got != want)[0][:5])
            assert mixed >= (3 if C > 1 and n_sets >= 63 else 1) or n_sets == 1, (C, n_sets, mixed)
            # colour numbers in the place of words, and max_in = None = popcount(include)
            some = sorted(colours[:3].tolist())
            assert np.array_equal(s.match_sets(some, None, 1), sb.verdicts(table, sb.mask_words(some, W), None, 1, len(some)))
            # guard bytes round match_out
            buf = np.full(n_sets + 128, 0xA5, dtype=np.uint8)
            p = capi.ColorPredicateC(inc.ctypes.data, exc.ctypes.data, 0, n_inc)
            assert L.sbwtgpu_colorsets_match_sets(s.handle, capi.C.byref(p), buf[64:].ctypes.data) == capi.OK
            assert np.all(buf[:64] == 0xA5) and np.all(buf[64 + n_sets:] == 0xA5)
            assert np.array_equal(buf[64:64 + n_sets], sb.verdicts(table, inc, exc, 0, n_inc))


# ---- 2. select against the definition -----------------------------------------------------------------------------------
def test_the_worked_example(gpu):
    idx, s, col = world({0: ["AACCG"], 1: ["CCGGTT"]}, [], 3, False, 2)
    with s:
        for pred, want in ((([0, 1], None, 2, None), {"CCG"}), (([0], [1], 1, None), {"AAC", "ACC"}),
                           (([0, 1], None, 1, 1), {"AAC", "ACC", "CGG", "GGT", "GTT"}), (([0, 1], None, 0, 0), set())):
            bits, info = check_select(s, col, 3, pred, pred)
            assert same_bits(bits, build_from_kmers(want, 3)) and info["n_selected"] == len(want)
    idx.close()


def test_reference_inputs_split_into_references(gpu):
    cases = [(KATS["cli_end_to_end"]["seqs"], KATS["cli_end_to_end"]["k"], KATS["cli_end_to_end"]["add_reverse_complements"]),
             (KATS["redundant_dummies"]["seqs"], KATS["redundant_dummies"]["k"], False)]
    cases += [(c["seqs"], c["k"], False) for c in KATS["small_cases"]["cases"] if c["k"] >= 2]
    for i, (seqs, k, rc) in enumerate(cases):
        n_refs = 2 + i % 4
        # (fewer sequences than references: the others get the first half of the first sequence)
        by_color = {c: seqs[c::n_refs] or [seqs[0][:max(k, len(seqs[0]) // 2)]] for c in range(n_refs)}
        idx, s, col = world(by_color, [], k, rc, n_refs)
        with s:
            for family in sb.FAMILIES:
                check_select(s, col, k, sb.family_predicate(family, range(n_refs), n_refs), (i, k, family))
        idx.close()


@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
@pytest.mark.parametrize("k", sb.K_VALUES)
def test_seeded_cases(gpu, k, rc):
    k, rc, n_colors, by_color, extra = sb.seeded_world(k, rc)
    idx, s, col = world(by_color, extra, k, rc, n_colors)
    with s:
        assert s.words == pw.n_words(n_colors)
        for family in sb.FAMILIES:
            check_select(s, col, k, sb.family_predicate(family, sorted(by_color), n_colors), (k, rc, family), marks=(family != "unique"))
    idx.close()


# every second set survives: by key, by wave of 64 keys and by block of 256 keys
@pytest.mark.parametrize("m,k,steps", [(64, 15, (1, 64)), (65, 15, (1, 64)), (3000, 15, (1, 64, 256)), (300_000, 31, (1, 256))])
def test_alternating_survivors_at_every_size(gpu, m, k, steps):
    seq = synth.random_genome(m + k - 1, 40 + k).tobytes().decode()
    idx = tw.make_index([seq], k)
    assert idx.n_kmers == m                                       # (no k-mer twice in a random sequence at these k)
    labels = tw.labels_of(idx)
    real = np.array(["$" not in lab for lab in labels])
    r = np.cumsum(real) - 1                                       # the number of a real column among the real columns
    # rows: 1 and 3 hold colour 0 alone (a duplicate), 2 colour 1, 4 both; row 5 is unused
    table = pw.rows_array([0, 0b01, 0b10, 0b01, 0b11, 0b10], 1)
    for step in steps:
        ids = np.where(real, 1 + (r // step) % 4, 0).astype(np.uint32)
        col = uploaded_colouring(labels, ids.tolist(), table)
        with capi.ColorSets.from_arrays(idx, 2, ids, table) as s:
            # sets 1 and 3 survive, 2 and 4 do not: one distinct row
            bits, info = check_select(s, col, k, ([0], [1], 1, None), (m, step))
            assert info["n_sets_matched"] == 1 and info["n_selected"] == int(np.isin(ids, (1, 3)).sum())
            if step == 1 and m <= 3000:
                check_select(s, col, k, ([1], None, 1, None), (m, step, "sets 2 and 4"))
    idx.close()


# ---- 3. edges -----------------------------------------------------------------------------------------------------------
def test_empty_and_full_selection_and_an_object_of_one_set(gpu):
    k, rc, n_colors, by_color, extra = sb.seeded_world(31, False)
    idx, s, col = world(by_color, extra, k, rc, n_colors)
    used = sorted(by_color)
    with s:
        empty, info = check_select(s, col, k, (used, None, len(used) + 1, len(used) + 1), "nothing")
        assert (empty.n_nodes, empty.n_kmers, info["n_selected"], info["n_sets_matched"], info["n_nopred"]) == (1, 0, 0, 0, 0)
        assert all(int(empty.cols[c][0]) == 0 for c in range(4)) and int(empty.ssup[0]) == 1
        full, info = check_select(s, col, k, (used, None, 0, None), "everything")
        assert same_bits(full, idx.setop(idx, "union")[0]) and info["n_selected"] == info["n_real"] == idx.n_kmers
        assert info["n_sets_matched"] == s.n_sets                  # the builder's object is canonical, and some k-mers are uncoloured
    with built(idx, 2, []) as nothing:
        assert nothing.n_sets == 1
        assert nothing.match_sets([0, 1], None, 0).tolist() == [1] and nothing.match_sets([0, 1]).tolist() == [0]
        col0 = {x: frozenset() for x in col}
        check_select(nothing, col0, k, ([0, 1], None, 1, None), "one set, nothing")
        bits, info = check_select(nothing, col0, k, ([0, 1], None, 0, None), "one set, everything")
        assert same_bits(bits, full) and info["n_sets_matched"] == 1
    idx.close()


@pytest.fixture(scope="module")
def read_set(gpu):
    """A read set: a few hundred reads of k .. k + 3 bases, so that the index has several dummy columns per k-mer; every
    second read is coloured, the others are not"""
    k = 21
    rng = random.Random(5)
    reads = [pw.rand_seq(rng, rng.randint(k, k + 3)) for _ in range(300)]
    by_color = {0: reads[0::4], 2: reads[2::4]}
    idx, s, col = world(by_color, reads[1::2], k, False, 3)
    yield k, reads, idx, s, col
    s.close()
    idx.close()


def test_uncoloured_columns_are_selected_and_dummy_columns_never(read_set):
    k, reads, idx, s, col = read_set
    n_dummy = idx.n_nodes - idx.n_kmers
    uncoloured = sum(1 for cs in col.values() if not cs)
    assert n_dummy > idx.n_kmers and uncoloured > 100
    # set 0 is shared by the dummy columns and the uncoloured real columns
    assert int(s.set_sizes()[0]) == n_dummy + uncoloured
    bits, info = check_select(s, col, k, ([0, 1, 2], None, 0, 0), "uncoloured")
    assert info["n_selected"] == uncoloured and info["n_sets_matched"] == 1 and bits.n_kmers == uncoloured
    c = s.select_counts([0, 1, 2], None, 0, 0)
    assert (c["n_real"], c["n_selected"], c["n_sets_matched"]) == (idx.n_kmers, uncoloured, 1)
    check_select(s, col, k, ([0], None, 0, 0), "colour 0 absent")
    check_select(s, col, k, ([0, 2], None, 1, None), "coloured")


# ---- 4. meaning, not numbering --------------------------------------------------------------------------------------------
def test_an_uploaded_copy_in_another_numbering_selects_the_same(gpu):
    k, rc, n_colors, by_color, extra = sb.seeded_world(33, True)
    idx, s, col = world(by_color, extra, k, rc, n_colors)
    used = sorted(by_color)
    ids, table = s.copy()
    n = len(table)
    assert n >= 4
    rng = np.random.default_rng(4)
    # new numbering: every old row twice (at 1 + perm and at n + perm), unused rows between and behind
    perm = rng.permutation(n - 1)
    new_table = np.zeros((2 * n + 3, table.shape[1]), dtype=np.uint64)
    new_table[1 + perm] = table[1:]
    new_table[n + 1 + perm] = table[1:]
    new_table[n] = table[1]
    new_table[2 * n:] = (table[1], table[n - 1], table[1])
    first = np.concatenate([[0], 1 + perm]).astype(np.uint32)
    second = np.concatenate([[0], n + 1 + perm]).astype(np.uint32)
    new_ids = np.where(np.arange(len(ids)) % 2 == 0, first[ids], second[ids]).astype(np.uint32)
    with s, capi.ColorSets.from_arrays(idx, n_colors, new_ids, new_table) as up:
        for family in sb.FAMILIES:
            pred = sb.family_predicate(family, used, n_colors)
            want, wi = s.select(*pred)
            got, gi = check_select(up, col, k, pred, ("uploaded", family))
            assert same_bits(got, want) and all(x.tobytes() == y.tobytes() for x, y in zip(got.cols + [got.ssup], want.cols + [want.ssup]))
            assert {f: gi[f] for f in COUNTS + ("n_nopred",)} == {f: wi[f] for f in COUNTS + ("n_nopred",)}
            # the verdicts follow the rows
            assert np.array_equal(up.match_sets(*pred)[1 + perm], s.match_sets(*pred)[1:])
    idx.close()


# ---- 5. the closed loop -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
def test_closed_loop_through_index_and_merge(gpu, rc):
    k, rc, n_colors, by_color, extra = sb.seeded_world(32, rc)
    idx, s, col = world(by_color, extra, k, rc, n_colors)
    used = sorted(by_color)
    reads = [x for c in used for x in by_color[c][:2]] + extra
    with s:
        for family in ("soft-core", "accessory", "absent"):
            pred = sb.family_predicate(family, used, n_colors)
            sel = sb.select(col, *pred)
            assert sel
            bits, _ = s.select(*pred)
            v = index_of(bits)
            with capi.ColorSets.merge(v, s) as merged:
                labels = tw.labels_of(v)
                ids, table = merged.copy()
                rows = pw.rows_ints(table)
                assert {lab for lab in labels if "$" not in lab} == sel
                for j, lab in enumerate(labels):
                    want_row = sum(1 << c for c in col[lab]) if "$" not in lab else 0
                    assert rows[ids[j]] == want_row, (family, j, lab)
                distinct = {col[x] for x in sel if col[x]}
                assert merged.n_sets == 1 + len(distinct) and len(set(rows)) == len(rows) and rows[0] == 0
                assert sorted(set(ids.tolist())) == list(range(merged.n_sets))           # no row unused
                # pseudoalignment on (v, merged) == the definition on the selected k-mers
                cs = [{x for x in sel if c in col[x]} for c in range(n_colors)]
                for strands in (1, 2):
                    rec, colors = merged.pseudoalign_reads([r.encode() for r in reads], strands == 2)
                    assert tw.as_lists(rec, colors) == pb.records(cs, sel, k, reads, strands), (family, strands)
            v.close()
    idx.close()


# ---- 6. the old route ---------------------------------------------------------------------------------------------------------
def old_route(sets, k, include, exclude, min_in, max_in):
    """coloured unitigs, a host filter on the set id, the device builder on the surviving strings"""
    bases, off, first_col, set_id = sets.unitigs()
    _, table = sets.copy()
    W = sets.words
    keep = sb.verdicts(table, sb.mask_words(include, W), sb.mask_words(exclude, W) if exclude is not None else None, min_in,
                       sb.default_max(include, min_in, max_in))[set_id].astype(bool)
    raw = bases.tobytes()
    return capi.build_bits_gpu([raw[off[i]:off[i + 1]] for i in np.nonzero(keep)[0]], k, False, True)


def test_the_old_route_gives_the_same_bits(gpu):
    k = 31
    g0 = synth.random_genome(200_000, 9)
    genomes = [g0] + [synth.mutate(g0, 0.01, 10 + i) for i in range(3)]
    bits = capi.build_bits_gpu([g.tobytes() for g in genomes], k, False, True)
    idx = index_of(bits)
    with capi.ColorSetsBuilder.create(idx, 4) as bld:
        for c, g in enumerate(genomes):
            bld.add_sequences(c, g, np.array([0, len(g)], dtype=np.int64))
        s = bld.finish()
    with s:
        sizes = s.set_sizes()
        for name, pred in (("core", ([0, 1, 2, 3], None, 4, None)), ("unique", ([0], [1, 2, 3], 1, None)),
                           ("accessory", ([0, 1, 2, 3], None, 1, 3))):
            got, info = s.select(*pred)
            assert same_bits(got, old_route(s, k, *pred)), name
            m = s.match_sets(*pred).astype(bool)
            assert 0 < info["n_selected"] < info["n_real"] == bits.n_kmers and info["n_selected"] == int(sizes[1:][m[1:]].sum()), name
            assert info["n_sets_matched"] == int(m.sum())
    idx.close()


# ---- 7. robustness --------------------------------------------------------------------------------------------------------------
def test_image_levels_and_layouts(gpu):
    for k, rc in ((31, True), (63, False)):
        k, rc, n_colors, by_color, extra = sb.seeded_world(k, rc)
        seqs, kmers, col = sb.colour_world(by_color, extra, k, rc, n_colors)
        idx, s, _ = world(by_color, extra, k, rc, n_colors)
        used = sorted(by_color)
        preds = [sb.family_predicate(f, used, n_colors) for f in ("core", "accessory")]
        with s:
            ids, table = s.copy()
            want = [s.select(*p) for p in preds]
        variants = []
        for key, val, back in (("image_level", 1, 0), ("image_level", 2, 0), ("force_mega", 1, 0), ("big_path", 2, 1)):
            capi.set_tuning(key, val)
            try:
                variants.append(((key, val), tw.make_index(seqs, k, rc)))
            finally:
                capi.set_tuning(key, back)
        for derive in (1, 0):               # no marks given: derived into the image, or absent
            capi.set_tuning("derive_ssup", derive)
            try:
                for level in (0, 2):
                    capi.set_tuning("image_level", level)
                    variants.append((("no marks", derive, level), tw.make_index(seqs, k, rc, ssup=False)))
            finally:
                capi.set_tuning("derive_ssup", 1)
                capi.set_tuning("image_level", 0)
        for name, other in variants:
            with capi.ColorSets.from_arrays(other, n_colors, ids, table) as so:
                for p, (wb, wi) in zip(preds, want):
                    gb, gi = so.select(*p)
                    assert same_bits(gb, wb) and {f: gi[f] for f in COUNTS} == {f: wi[f] for f in COUNTS}, (k, name)
                    c = so.select_counts(*p)
                    assert {f: c[f] for f in COUNTS} == {f: wi[f] for f in COUNTS}, (k, name)
            other.close()
        idx.close()


def test_determinism(read_set):
    k, reads, idx, s, col = read_set
    for pred in (([0, 2], None, 1, None), ([0, 1, 2], None, 0, 0), ([0], [2], 1, 1)):
        (a, ia), (b, ib) = s.select(*pred), s.select(*pred)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a.cols + [a.ssup], b.cols + [b.ssup]))
        assert {f: ia[f] for f in ia if f != "pass_ms"} == {f: ib[f] for f in ib if f != "pass_ms"}
        assert s.match_sets(*pred).tobytes() == s.match_sets(*pred).tobytes()


def test_two_host_threads_on_one_object(read_set):
    k, reads, idx, s, col = read_set
    preds = (([0, 2], None, 1, None), ([0, 1, 2], None, 0, 0))
    want = [s.select(*p)[0] for p in preds]
    out, errs = [None, None], []

    def work(t):
        try:
            out[t] = [(s.select(*preds[t])[0], s.select_counts(*preds[t]), s.match_sets(*preds[t])) for _ in range(3)]
        except Exception as e:        # noqa: BLE001 -- reported below
            errs.append(e)
    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for t in range(2):
        m = s.match_sets(*preds[t])
        for bits, c, got_m in out[t]:
            assert same_bits(bits, want[t]) and c["n_selected"] == want[t].n_kmers and np.array_equal(got_m, m)


def test_refusals_name_their_cause_and_leave_everything_usable(read_set):
    k, reads, idx, s, col = read_set
    L, C = capi.lib(), capi.C
    inc, exc = s.color_mask([0, 2]), s.color_mask([1])
    before = (s.copy(), s.select([0, 2])[0], idx.search_reads([r.encode() for r in reads[:3]])[0])
    out, info, match = capi.PlainMatrixBitsC(), capi.ColorSelectInfoC(), np.zeros(s.n_sets, dtype=np.uint8)

    def pred(a=inc, b=exc, lo=1, hi=2):
        return capi.ColorPredicateC(a.ctypes.data if a is not None else None, b.ctypes.data if b is not None else None, lo, hi)

    def calls(handle, p, outputs=True):
        """the three calls' return codes and messages"""
        res = []
        for fn, args in ((L.sbwtgpu_colorsets_match_sets, (match.ctypes.data if outputs else None,)),
                         (L.sbwtgpu_colorsets_select_counts, (C.byref(info) if outputs else None,)),
                         (L.sbwtgpu_colorsets_select, (1, C.byref(out) if outputs else None, None))):
            rc = fn(handle, C.byref(p) if p is not None else None, *args)
            res.append((rc, L.sbwtgpu_last_error().decode()))
            if rc == capi.OK and fn is L.sbwtgpu_colorsets_select:
                L.sbwtgpu_free_plain_matrix(C.byref(out))
        return res

    def all_refused(res, *needles):
        for rc, msg in res:
            assert rc == capi.ERR_INVALID_ARG and all(x in msg for x in needles), (rc, msg)

    all_refused(calls(None, pred()), "NULL")
    all_refused(calls(s.handle, None), "NULL")
    all_refused(calls(s.handle, pred(a=None)), "NULL", "include")
    all_refused(calls(s.handle, pred(), outputs=False), "NULL")
    assert all(rc == capi.OK for rc, _ in calls(s.handle, pred(b=None)))                 # exclude and info may be NULL
    # a bit at or above n_colors = 3 in either mask
    high = np.array([1 << 3], dtype=np.uint64)
    all_refused(calls(s.handle, pred(a=high)), "include", "n_colors = 3")
    all_refused(calls(s.handle, pred(b=high)), "exclude", "n_colors = 3")
    refused(lambda: s.match_sets([3]), "colour 3")
    # the bounds
    all_refused(calls(s.handle, pred(lo=-1)), "min_in", "negative")
    all_refused(calls(s.handle, pred(lo=2, hi=1)), "max_in = 1", "min_in = 2")
    assert all(rc == capi.OK for rc, _ in calls(s.handle, pred(lo=5, hi=5)))             # above popcount(include): legal
    assert s.select([0, 2], None, 5)[1]["n_selected"] == 0 and not s.match_sets([0, 2], None, 5).any()
    # k outside 2 .. 64: the verdicts need no keys, the two select calls do
    rng = random.Random(65)
    long_seqs = [pw.rand_seq(rng, 200)]
    k65 = tw.make_index(long_seqs, 65)
    with built(k65, 3, [(0, long_seqs, False)]) as s65:
        assert s65.match_sets([0]).tolist() == [0, 1]
        refused(lambda: s65.select([0]), "k = 65", "2 <= k <= 64")
        refused(lambda: s65.select_counts([0]), "k = 65", "2 <= k <= 64")
    k65.close()
    # a rank-only index carries no colour-set object (create refuses it), and an object of another index is refused
    w = np.random.default_rng(1).integers(0, 2**64, size=4, dtype=np.uint64)
    ro = capi.Index.create(w, w, w, w, None, 256, k)
    refused(lambda: capi.ColorSetsBuilder.create(ro, 2), "only rank()")
    ro.close()
    # everything still answers, and the object is what it was
    after = (s.copy(), s.select([0, 2])[0], idx.search_reads([r.encode() for r in reads[:3]])[0])
    assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0])) and same_bits(before[1], after[1])
    assert np.array_equal(before[2], after[2])
    check_select(s, col, k, ([0, 2], [1], 1, None), "after the refusals")


# ---- 8. the CLI -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_world(gpu, tmp_path_factory):
    """an index file over seven sequences with three overlapping references as colours, in the three colour file kinds"""
    d = str(tmp_path_factory.mktemp("color_select_cli"))
    k = 13
    rng = random.Random(9)
    pool = [pw.rand_seq(rng, rng.randint(k + 2, 2 * k + 60)) for _ in range(7)]
    refs = [pool[:4], pool[2:6], pool[3:]]
    SBWT = tw.SBWT
    with open(d + "/all.fna", "w") as fh, open(d + "/refs.txt", "w") as lst:
        for i, s in enumerate(pool):
            fh.write(">s%d\n%s\n" % (i, s))
        for c, seqs in enumerate(refs):
            with open("%s/ref%d.fna" % (d, c), "w") as one:
                for s in seqs:
                    one.write(">r\n%s\n" % s)
            lst.write("%s/ref%d.fna\n" % (d, c))
    p = tw.run([SBWT, "build", "-i", d + "/all.fna", "-o", d + "/all.sbwt", "-k", str(k), "--temp-dir", d])
    assert p.returncode == 0, p.stderr.decode()
    for flags, name in (([], "col1"), (["--wide"], "col2"), (["--compress"], "col3")):
        p = tw.run([SBWT, "build-colors"] + flags + ["-i", d + "/all.sbwt", "-r", d + "/refs.txt", "-o", "%s/all.%s" % (d, name)])
        assert p.returncode == 0, p.stderr.decode()
    assert [open("%s/all.%s" % (d, n), "rb").read(8) for n in ("col1", "col2", "col3")] == [b"SBWTCOL1", b"SBWTCOL2", b"SBWTCOL3"]
    seqs, kmers, col = sb.colour_world({c: r for c, r in enumerate(refs)}, [], k, False, 3)
    return d, k, pool, kmers, col, [SBWT, "color-select", "-i", d + "/all.sbwt"]


def test_cli_color_select(cli_world):
    d, k, pool, kmers, col, base = cli_world
    SBWT = tw.SBWT
    # each colour file kind; the defaults are include = all, min = 1, max = |include|
    for name in ("col1", "col2", "col3"):
        out = "%s/core.%s.sbwt" % (d, name)
        p = tw.run(base + ["-c", "%s/all.%s" % (d, name), "--min", "3", "-o", out])
        assert p.returncode == 0, p.stderr.decode()
        f = hostlib.read_index_file(out)
        want, c = sb.build(col, k, [0, 1, 2], None, 3)
        assert (f.n_nodes, f.n_kmers) == (want.n_nodes, want.n_kmers) and c["n_selected"] > 0
        assert all(np.array_equal(f.cols[i], want.cols[i]) for i in range(4)) and np.array_equal(f.ssup, want.ssup)
        line = [ln for ln in (p.stdout + p.stderr).decode().splitlines() if "color-select:" in ln]
        assert len(line) == 1 and "%d of %d k-mers selected, %d colour sets matched" % (c["n_selected"], c["n_real"], c["n_sets_matched"]) in line[0]
    # the file set-op would write for the same k-mers: select everything == the union of the index with itself
    p = tw.run(base + ["-c", d + "/all.col3", "-o", d + "/every.sbwt"])
    assert p.returncode == 0, p.stderr.decode()
    p = tw.run([SBWT, "set-op", "-a", d + "/all.sbwt", "-b", d + "/all.sbwt", "--op", "union", "-o", d + "/union.sbwt"])
    assert p.returncode == 0 and open(d + "/every.sbwt", "rb").read() == open(d + "/union.sbwt", "rb").read()
    # --counts-only
    want = sb.counts(col, [0], [1, 2], 1)
    p = tw.run(base + ["-c", d + "/all.col3", "--include", "0", "--exclude", "1-2", "--counts-only"])
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout.decode().split()[-3:] == [str(want[f]) for f in COUNTS] and want["n_selected"] > 0


def test_cli_color_select_colours_of_the_result_and_refusals(cli_world):
    d, k, pool, kmers, col, base = cli_world
    SBWT = tw.SBWT
    # --colors-out, round-tripped through pseudoalign: accessory k-mers (--max 2) with their colours
    p = tw.run(base + ["-c", d + "/all.col1", "--include", "0,1-2", "--max", "2", "-o", d + "/acc.sbwt", "--colors-out", d + "/acc.colors"])
    assert p.returncode == 0, p.stderr.decode()
    assert open(d + "/acc.colors", "rb").read(8) == b"SBWTCOL3"
    sel = sb.select(col, [0, 1, 2], None, 1, 2)
    assert 0 < len(sel) < len(kmers)
    with open(d + "/q.fna", "w") as fh:
        for i, s in enumerate(pool):
            fh.write(">q%d\n%s\n" % (i, s))
    p = tw.run([SBWT, "pseudoalign", "-i", d + "/acc.sbwt", "-c", d + "/acc.colors", "-q", d + "/q.fna", "-o", d + "/q.txt", "--threshold", "0.5"])
    assert p.returncode == 0, p.stderr.decode()
    cs = [{x for x in sel if c in col[x]} for c in range(3)]
    assert open(d + "/q.txt", "rb").read() == pw.format_lines(rec[0] for rec in pb.records(cs, sel, k, pool, 1, 500_000, 0))
    # a malformed list, a colour beyond the file's, a colour file of another index, a library refusal
    for bad in ("0,,1", "2-1", "3"):
        p = tw.run(base + ["-c", d + "/all.col3", "--include", bad, "-o", d + "/x.sbwt"], 60)
        assert p.returncode != 0 and b"colour list" in p.stderr, bad
    p = tw.run(base + ["-c", d + "/acc.colors", "-o", d + "/x.sbwt"], 60)
    assert p.returncode != 0 and b"columns at k =" in p.stderr
    p = tw.run(base + ["-c", d + "/all.col3", "--min", "3", "--max", "2", "-o", d + "/x.sbwt"], 60)
    assert p.returncode != 0 and b"max_in = 2" in p.stderr
    p = tw.run([SBWT], 60)
    assert b"color-select" in p.stderr + p.stdout
