"""GPU: sbwtgpu_occurrences_* (sbwt_occurrences.hip: every reference coordinate of every column's k-mer as CSR arrays, and reads
placed on the references by diagonal voting over all of them) against the definition in tests/occurrences_brute.py.  Every
comparison is exact: both arrays on every column, and the map records field for field."""
import gzip
import random
import threading

import numpy as np
import pytest

import occurrences_brute as ob
import positions_brute as pb
import read_hits_brute as rb
import test_gpu_positions as tp                 # its helpers: World, Side, rand_seq, mutate, enc, numbered, scattered, hit_windows
import test_gpu_pseudoalign_wide as tw          # its helpers: make_index, labels_of, refused, run, tuning, SBWT
from sbwt_amd import capi, hostlib
from test_gpu_positions import reads, world     # noqa: F401  (the module's fixtures: the three references and the read sample)

pytestmark = pytest.mark.gpu

K = tp.K
T = capi.OCCURRENCES_MAP_TABLE
GUARD = 64
enc, numbered, rand_seq, mutate = tp.enc, tp.numbered, tp.rand_seq, tp.mutate


def build(idx, refs, strands, first_seq=0):
    with idx.occurrences_builder() as b:
        b.add(enc(refs), first_seq, strands)
        return b.finish()


_tables = {}


def table(side, refs, strands):
    """the brute-force occurrences of the references numbered 0, 1, ..., computed once per side and strands"""
    key = (id(side), strands)
    if key not in _tables:
        _tables[key] = ob.table(side.kmers, side.k, numbered(refs, strands))
    return _tables[key]


def check_arrays(occ, side, refs_numbered, label=None):
    """the object's arrays on every column, and its scalars, against the brute force"""
    want = ob.table(side.kmers, side.k, refs_numbered)
    off, keys = ob.arrays(want, side.labels)
    got_off, got_keys = occ.offsets(), occ.keys()
    assert got_off.dtype == np.uint64 and got_keys.dtype == np.uint64
    assert got_off.tolist() == off and got_keys.tolist() == keys, label
    info = occ.info()
    nw, nh = pb.scalars(side.kmers, side.k, refs_numbered)
    assert (info["n_columns"], info["k"], info["n_windows"], info["n_hits"]) == (side.idx.n_nodes, side.k, nw, nh), (label, info)
    assert (info["n_occurrences"], info["n_positioned"], info["max_count"]) == ob.scalars(want), (label, info)
    assert info["device_bytes"] >= 8 * (side.idx.n_nodes + 1 + len(keys))
    return want


def state(occ):
    return occ.offsets().tobytes(), occ.keys().tobytes(), occ.info()


# ---- 1. the arrays against the brute force, at every k ------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 5, 15, 31, 32, 33, 63, 64, 65])
def test_arrays_against_brute(gpu, k):
    rng = random.Random(2700 + k)
    alphabet = "ACGT" if k > 5 else "AC" if k == 2 else "ACG"
    base = rand_seq(rng, 400, alphabet)
    refs = [base + rand_seq(rng, 100, alphabet) + base[20:120], rand_seq(rng, 150, alphabet) + base[100:350] + "N" + rand_seq(rng, 90, alphabet),
            pb.revcomp(base[50:300]) + rand_seq(rng, 70, alphabet) + "acgt", "ACG"[:min(k - 1, 3)], ""]
    extra = [rand_seq(rng, 120, alphabet)]
    for rc in (False, True):
        side = tp.Side(refs + extra, k, rc)
        for strands in (1, 2):
            with side.idx.occurrences_builder() as b:
                nw, nh = b.add(enc(refs), 0, strands)
                assert nw == sum(max(len(s) - k + 1, 0) for s in refs) and nh == tp.hit_windows(side.kmers, k, refs, strands)
                with b.finish() as occ:
                    assert b.handle is None
                    want = check_arrays(occ, side, numbered(refs, strands), (k, rc, strands))
                    off, keys = occ.offsets(), occ.keys()
                    # independently of the brute force: every key spells its column's k-mer, and ascends within the column
                    for v in range(side.idx.n_nodes):
                        col = keys[int(off[v]):int(off[v + 1])].tolist()
                        assert col == sorted(set(col))
                        for f in col:
                            seq, p, t = pb.decode(f)
                            x = refs[seq][p:p + k]
                            assert len(x) == k and side.labels[v] == (pb.revcomp(x) if t else x), (k, rc, strands, v)
                    assert max(len(v) for v in want.values()) >= 2      # the planted repeat is there
                    # its first keys are the position table of the same adds, byte for byte
                    with side.idx.positions() as pos, occ.positions() as proj:
                        pos.add(enc(refs), 0, strands)
                        assert proj.first().tobytes() == pos.first().tobytes()
                        assert proj.info()["n_positioned"] == occ.info()["n_positioned"] == pos.info()["n_positioned"]
        side.idx.close()


@pytest.mark.parametrize("level", [1, 2])
def test_image_levels(world, level):
    with tw.tuning("image_level", level, 0):
        idx = tw.make_index(world.seqs, K, True)
    assert idx.image_level == level and idx.n_nodes == world.rc.idx.n_nodes
    with build(idx, world.refs, 2) as occ, build(world.rc.idx, world.refs, 2) as want:
        assert state(occ) == state(want)
    idx.close()


# ---- 2. order, chunking, threads, numbers, upload -------------------------------------------------------------------------
@pytest.mark.parametrize("rc,strands", [(False, 1), (True, 2), (False, 2), (True, 1)])
def test_order_chunking_and_threads(world, rc, strands):
    side = world.side(rc)
    with build(side.idx, world.refs, strands) as one:
        check_arrays(one, side, numbered(world.refs, strands), "one batch")
        want = state(one)
    with side.idx.occurrences_builder() as b:                        # one by one, in reverse order
        for i in reversed(range(3)):
            b.add(enc([world.refs[i]]), i, strands)
        with b.finish() as occ:
            assert state(occ) == want
    with side.idx.occurrences_builder() as b:
        with tw.tuning("occurrences_chunk_bases", 1, 0):             # every sequence a chunk of its own
            b.add(enc(world.refs), 0, strands)
        with b.finish() as occ:
            assert state(occ) == want
    with side.idx.occurrences_builder() as b:                        # two host threads on one builder
        errors = []

        def work(seqs, first_seq):
            try:
                b.add(enc(seqs), first_seq, strands)
            except Exception as e:                                   # noqa: BLE001
                errors.append(e)

        th = [threading.Thread(target=work, args=(world.refs[:2], 0)), threading.Thread(target=work, args=(world.refs[2:], 2))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors
        with b.finish() as occ:
            assert state(occ) == want
    with side.idx.occurrences_builder() as b:                        # everything twice: the arrays stay, the windows count twice
        b.add(enc(world.refs), 0, strands)
        b.add(enc(world.refs[1:]), 1, strands)
        b.add(enc(world.refs[:1]), 0, strands)
        with b.finish() as occ:
            got = state(occ)
            assert got[:2] == want[:2] and got[2]["n_windows"] == 2 * want[2]["n_windows"] and got[2]["n_hits"] == 2 * want[2]["n_hits"]
            assert got[2]["n_occurrences"] == want[2]["n_occurrences"]


def test_two_numbers_leave_both_and_an_empty_builder(world):
    side = world.fwd
    s = world.refs[1]
    with side.idx.occurrences_builder() as b:
        b.add(enc([s]), 3)
        b.add(enc([s]), 1)
        b.add(enc([s]), (1 << 30) - 1)                               # the largest number there is
        with b.finish() as occ:
            check_arrays(occ, side, [(3, s, 1), (1, s, 1), ((1 << 30) - 1, s, 1)], "three numbers")
            keys = occ.keys()
            seqs = keys >> np.uint64(32)
            assert sorted(set(seqs.tolist())) == [1, 3, (1 << 30) - 1] and len(keys) % 3 == 0
            assert np.array_equal(np.sort(keys[seqs == 1] & np.uint64(0xFFFFFFFF)), np.sort(keys[seqs == 3] & np.uint64(0xFFFFFFFF)))
    with side.idx.occurrences_builder() as b:
        with b.finish() as occ:                                       # nothing added
            assert not occ.offsets().any() and len(occ.keys()) == 0
            info = occ.info()
            assert (info["n_occurrences"], info["n_positioned"], info["max_count"], info["n_windows"]) == (0, 0, 0, 0)
            assert pb.as_tuples(occ.map_reads(enc([world.refs[0][:60], ""]))) == [(0, -1, 0, 0, 0, 60 - K + 1, 0), (0, -1, 0, 0, 0, 0, 0)]
            with occ.positions() as proj:
                assert not (proj.first() != np.uint64(capi.POS_NONE)).any()


def test_upload_maps_identically_and_refuses_damage(world, reads):
    side = world.rc
    n = side.idx.n_nodes
    with build(side.idx, world.refs, 2) as occ:
        off, keys = occ.offsets(), occ.keys()
        want = occ.map_reads(enc(reads), 2, 3)
        with capi.Occurrences.upload(side.idx, off, keys) as up:
            assert np.array_equal(up.offsets(), off) and np.array_equal(up.keys(), keys)
            a, b = up.info(), occ.info()
            assert (a["n_windows"], a["n_hits"]) == (0, 0)
            assert all(a[x] == b[x] for x in ("n_columns", "k", "n_occurrences", "n_positioned", "max_count"))
            assert np.array_equal(up.map_reads(enc(reads), 2, 3), want)
            assert up.offsets_dev() and up.keys_dev() and up.offsets_dev() != occ.offsets_dev()
        counts = np.diff(off.astype(np.int64))
        two = int(np.flatnonzero(counts >= 2)[5])                     # a column with two keys or more
        one = int(np.flatnonzero(counts >= 1)[-1])
        e2, e1 = int(off[two]), int(off[one])

        def damaged(what, column, *needles):
            o, k2 = off.copy(), keys.copy()
            what(o, k2)
            tw.refused(lambda: capi.Occurrences.upload(side.idx, o, k2), "column %d" % column, *needles)

        def set_off(i, v):
            return lambda o, k2: o.__setitem__(i, v)

        def set_key(i, v):
            return lambda o, k2: k2.__setitem__(i, v)

        damaged(set_off(0, 1), 0, "off[0]")
        assert off[two] > 0
        damaged(set_off(two + 1, int(off[two]) - 1), two, "decreases")
        damaged(set_off(n, len(keys) + 1), n - 1, "n_occ")
        damaged(set_off(n // 2, len(keys) + 7), n // 2, "decreases")   # (beyond the keys: nothing is read through it)
        damaged(set_key(e2 + 1, int(keys[e2])), two, "strictly ascending")            # equal keys
        damaged(set_key(e2, int(keys[e2 + 1]) + 1), two, "strictly ascending")          # descending
        damaged(set_key(e1, (1 << 30) << 32), one, "2^30")
        damaged(set_key(e1, 1 << 63), one, "2^30")
        # two kinds of damage: the smallest column is named
        first_col = int(np.flatnonzero(counts >= 1)[0])
        damaged(lambda o, k2: (k2.__setitem__(int(off[first_col]), 1 << 62), k2.__setitem__(e1, 1 << 62)), first_col, "2^30")
        ok = keys.copy()
        ok[-1] = (((1 << 30) - 1) << 32) | 0xFFFFFFFF               # the largest key there is, in the last column that has one
        capi.Occurrences.upload(side.idx, off, ok).close()
        with pytest.raises(ValueError):
            capi.Occurrences.upload(side.idx, off[:-1], keys)
        tw.refused(lambda: capi.Occurrences.upload(side.idx, off, keys[:-1]), "n_occ")


# ---- 3. the map against the brute force -----------------------------------------------------------------------------------
def check_map(occ, side, want_occ, batch, strands, max_occ, label=None):
    got = occ.map_reads(enc(batch), strands, max_occ)
    assert got.dtype == capi.READ_MAP_DTYPE and len(got) == len(batch)
    want = ob.records(want_occ, side.kmers, side.k, batch, strands, max_occ)
    for i, (g, x) in enumerate(zip(pb.as_tuples(got), want)):
        assert g == x, (label, i, len(batch[i]), g, x)
    return want


@pytest.mark.parametrize("rc,table_strands,strands", [(False, 1, 1), (False, 1, 2), (True, 2, 1), (True, 2, 2), (True, 1, 2)])
def test_map_against_brute(world, reads, rc, table_strands, strands):
    side = world.side(rc)
    want_occ = table(side, world.refs, table_strands)
    first = side.table(world.refs, table_strands)
    with build(side.idx, world.refs, table_strands) as occ:
        by_max = {m: check_map(occ, side, want_occ, reads, strands, m, (rc, table_strands, strands, m)) for m in (1024, 3, 2, 1)}
        want = by_max[1024]
        # the sample is what its comments say: placed reads of both orientations, overhangs, ties (more of them than the
        # projection shows: a shared stretch is one), runner-ups, reads without an anchor
        assert sum(1 for r in want if r[1] >= 0) > 30 and any(r[0] < 0 for r in want)
        assert any(r[3] == r[4] > 0 for r in want) and any(0 < r[4] < r[3] for r in want)
        assert any(r[6] == 0 and r[5] > 0 for r in want) and any(r[5] == 0 for r in want)
        proj = pb.records(first, side.kmers, side.k, reads, strands)
        assert sum(r[3] == r[4] > 0 for r in want) > sum(r[3] == r[4] > 0 for r in proj)
        assert any(r[1] > p[1] >= 0 for r, p in zip(want, proj))     # reads that leave the smallest number for the better fit
        # max_occ takes anchors away, never hits
        for m in (3, 2, 1):
            assert [r[5] for r in by_max[m]] == [r[5] for r in want]
            assert all(a[6] <= b[6] for a, b in zip(by_max[m], want))
            assert m == 3 or any(a[6] < b[6] for a, b in zip(by_max[m], want))       # (no k-mer of the world lies more than thrice)
        if strands == 2 or rc:
            assert any(r[2] == 1 for r in want) and any(r[2] == 0 and r[1] >= 0 for r in want)
        assert len(occ.map_reads([], strands)) == 0
        assert pb.as_tuples(occ.map_reads([b"", b""], strands)) == [(0, -1, 0, 0, 0, 0, 0)] * 2


def test_the_run_across_an_iteration_edge_is_what_it_says(world, reads):
    side = world.fwd
    want_occ = table(side, world.refs, 1)
    read = next(r for r in reads if len(r) == 163 and r[63:] == world.refs[0][2000:2100])
    cnt, found, anchored = ob.votes(want_occ, side.kmers, K, read)
    hits = rb.hits(side.kmers, K, read)
    assert hits[:63] == [0] * 63 and all(hits[63:]) and len(hits) == 149          # the first hit sits in lane 63 of iteration 0
    # sequence 0's stretch 2000 .. 2100 lies in the core that sequence 1 holds a mutated copy of: the winner has all 86
    assert cnt[(0, 0, 2000 - 63)] == 86 and (found, anchored) == (86, 86) and max(cnt.values()) == 86
    with build(side.idx, world.refs, 1) as occ:
        got = pb.as_tuples(occ.map_reads(enc([read])))
        assert got == [ob.record(want_occ, side.kmers, K, read)] and got[0][:4] == (1937, 0, 0, 86)


def test_the_read_of_the_last_strain_lands_on_it(gpu):
    """the CPU test's case on the device: the projection says sequence 0, the vote over all occurrences says sequence 2"""
    k = 4
    shared = "GATTACAGGC"
    strains = ["CC" + shared + "TT", "AAAAAAA", "TG" + shared + "AC"]
    idx = tw.make_index(strains, k)
    batch = enc([shared + "A", shared])
    with idx.positions() as pos, build(idx, strains, 1) as occ:
        pos.add(enc(strains), 0)
        assert pb.as_tuples(pos.map_reads(batch)) == [(2, 0, 0, 7, 1, 8, 8), (2, 0, 0, 7, 0, 7, 7)]
        assert pb.as_tuples(occ.map_reads(batch)) == [(2, 2, 0, 8, 7, 8, 8), (2, 0, 0, 7, 7, 7, 7)]
        # AAAA lies four times on sequence 1: with max_occ = 3 a read of it is found and not anchored
        assert pb.as_tuples(occ.map_reads(enc(["AAAAA"]), 1, 3)) == [(0, -1, 0, 0, 0, 2, 0)]
        assert pb.as_tuples(occ.map_reads(enc(["AAAAA"]), 1, 4)) == [(0, 1, 0, 2, 2, 2, 2)]
        assert occ.info()["max_count"] == 4
    idx.close()


def test_references_without_a_shared_kmer_map_like_the_projection(gpu, reads):
    rng = random.Random(271)
    refs = [rand_seq(rng, 3000) for _ in range(3)]
    side = tp.Side(refs, K, True)
    with build(side.idx, refs, 1) as occ, side.idx.positions() as pos:
        pos.add(enc(refs), 0, 1)
        assert occ.info()["max_count"] == 1
        batch = [mutate(rng, refs[i % 3][a:a + n], 0.02) for i, (a, n) in enumerate((rng.randrange(0, 2500), rng.randint(K, 400)) for _ in range(40))]
        batch += [pb.revcomp(r) for r in batch[:10]] + [refs[0][100:160] + refs[2][50:110], "", "ACGT"] + list(reads[:6])
        for strands in (1, 2):
            got = occ.map_reads(enc(batch), strands, 1 << 20)
            assert np.array_equal(got, pos.map_reads(enc(batch), strands)) and (got["seq"] >= 0).sum() > 30
    side.idx.close()


def test_both_adds_walk_the_same_results(gpu):
    """The frame that k_pos_add and k_occ_add share, on the smallest batch in which one wave holds forward and mirrored results
    and the last wave is partial: k = 5, references of 69 and 5 bases, two strands -- 66 windows, 132 results; the second wave
    holds forward results 64, 65 and mirrored results 0 .. 61, the third has four live lanes."""
    k, strands = 5, 2
    rng = random.Random(2801)
    a = rand_seq(rng, 69, "ACG")
    refs = [a, a[10:15]]                                    # (the one window of sequence 1 repeats a k-mer of sequence 0)
    side = tp.Side(refs, k, True)
    nums = numbered(refs, strands)
    assert sum(len(s) - k + 1 for s in refs) == 66
    want_first = pb.first_table(side.kmers, k, nums)
    want_occ = ob.table(side.kmers, k, nums)
    assert max(len(v) for v in want_occ.values()) >= 2      # k-mers repeat: the minimum and the runs of a column have work
    assert {f & 1 for v in want_occ.values() for f in v} == {0, 1}      # and both halves of the results hit
    with side.idx.positions() as pos, side.idx.occurrences_builder() as b:
        added = pos.add(enc(refs), 0, strands)
        assert added == b.add(enc(refs), 0, strands) == (66, tp.hit_windows(side.kmers, k, refs, strands))
        with b.finish() as occ, occ.positions() as proj:
            assert pos.info()["n_hits"] == occ.info()["n_hits"] == pb.scalars(side.kmers, k, nums)[1]
            assert pos.info()["n_windows"] == occ.info()["n_windows"] == 132
            assert pos.first().tolist() == pb.table_array(want_first, side.labels)
            off, keys = ob.arrays(want_occ, side.labels)
            assert occ.offsets().tolist() == off and occ.keys().tolist() == keys
            assert proj.first().tobytes() == pos.first().tobytes()
    side.idx.close()


# ---- 4. the placement table's edge -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc,strands", [(False, 1), (True, 2)])
def test_table_edge_with_a_small_capacity(world, reads, rc, strands):
    side = world.side(rc)
    want_occ = table(side, world.refs, strands)
    rng = random.Random(44)
    edge = {}
    while len(edge) < 5:                                             # reads with exactly 1 .. 5 distinct placements
        n = 1 + len(edge)
        r = tp.scattered(world, n, 24, rng)
        if ob.n_placements(want_occ, side.kmers, K, r, strands) == n:
            edge[n] = r
    batch = reads[:20] + [edge[3], edge[4], edge[5]] + reads[20:40] + [edge[5], edge[1], edge[4]] + reads[40:]
    assert [ob.n_placements(want_occ, side.kmers, K, r, strands) for r in (edge[3], edge[4], edge[5])] == [3, 4, 5]
    with build(side.idx, world.refs, strands) as occ:
        want = occ.map_reads(enc(batch), strands)                    # the compiled capacity
        for cap in (4, 3, 1, 5):
            with tw.tuning("occurrences_map_table", cap, 0):
                check_map(occ, side, want_occ, batch, strands, 1024, ("capacity", cap))
                assert np.array_equal(occ.map_reads(enc(batch), strands), want)


@pytest.fixture(scope="module")
def repeat(gpu):
    """a 20-base unit 300 times between random flanks: a read from inside has some 300 placements"""
    rng = random.Random(2720)
    unit = rand_seq(rng, 20)
    ref = rand_seq(rng, 500) + unit * 300 + rand_seq(rng, 500)
    other = rand_seq(rng, 800)
    side = tp.Side([ref, other], K, True)
    yield side, [ref, other], unit
    side.idx.close()


def test_reads_beyond_the_compiled_capacity(repeat, reads):
    side, refs, unit = repeat
    rng = random.Random(2721)
    inside = [(unit * 3)[a:a + 40] for a in (0, 7, 19)] + [pb.revcomp((unit * 3)[3:43]), mutate(rng, (unit * 3)[5:45], 0.05)]
    edge = [refs[0][480:540], refs[0][500 + 6000 - 30:500 + 6000 + 40]]          # across the repeat's two ends
    ordinary = [mutate(rng, refs[i % 2][a:a + 100], 0.01) for i, a in enumerate(rng.randrange(0, 400) for _ in range(30))]
    batch = ordinary[:10] + inside[:2] + ordinary[10:20] + edge + inside[2:] + ordinary[20:] + [inside[0]]
    for strands in (1, 2):
        want_occ = ob.table(side.kmers, K, numbered(refs, strands))
        assert max(len(v) for v in want_occ.values()) == 300
        n = [ob.n_placements(want_occ, side.kmers, K, r, strands) for r in inside]
        assert all(T < x < 2 * T for x in n[:3]), n
        assert all(ob.record(want_occ, side.kmers, K, r, strands, 16)[6] == 0 for r in inside[:3])       # too repetitive at 16
        with build(side.idx, refs, strands) as occ:
            assert occ.info()["max_count"] == 300
            want = check_map(occ, side, want_occ, batch, strands, 1024, ("beyond", strands))
            assert sum(1 for r in want if r[3] == r[4] >= 26) >= 3                 # the repeat's reads tie with their shifted selves
            check_map(occ, side, want_occ, batch, strands, 16, ("beyond, max_occ 16", strands))
            check_map(occ, side, want_occ, batch, strands, 299, ("beyond, max_occ 299", strands))
            if strands == 2:
                with tw.tuning("occurrences_map_table", 4, 0):       # the slices double several times
                    got = occ.map_reads(enc(batch), strands)
                assert pb.as_tuples(got) == want


def slice_of(placement, P=1024):
    """the second kernel's slice of a placement among P = 1024: bits 48 .. 57 of the key times the golden-ratio constant"""
    seq, o, start = placement
    key = (seq << 33) | (o << 32) | (start + (1 << 31))
    return ((key * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)) >> 48 & (P - 1)


def test_placements_that_no_slicing_separates(gpu):
    """With a capacity of one, two placements that share a slice at every P up to 1024 reach the third kernel, which counts
    placement by placement without a table."""
    rng = random.Random(2722)
    ref = rand_seq(rng, 4000)
    side = tp.Side([ref], K, False)
    by_slice = {}
    pair = None
    for start in range(100, 3800):
        s = slice_of((0, 0, start))
        if s in by_slice and abs(by_slice[s] - start) > 200:
            pair = (by_slice[s], start)
            break
        by_slice.setdefault(s, start)
    assert pair and slice_of((0, 0, pair[0])) == slice_of((0, 0, pair[1]))
    a, b = pair[0], pair[1] + 40                                      # the second piece stands 40 bases into the read
    batch = [ref[a:a + 40] + ref[b:b + 30], ref[b:b + 40] + ref[a:a + 40], ref[a:a + 50], ref[100:160] + ref[900:960] + ref[2000:2050]]
    want_occ = ob.table(side.kmers, K, numbered([ref], 1))
    cnt = ob.votes(want_occ, side.kmers, K, batch[0])[0]
    assert len(cnt) == 2 and len({slice_of(p) for p in cnt}) == 1
    with build(side.idx, [ref], 1) as occ:
        want = check_map(occ, side, want_occ, batch, 1, 1024)
        with tw.tuning("occurrences_map_table", 1, 0):
            assert pb.as_tuples(occ.map_reads(enc(batch))) == want
    side.idx.close()


# ---- 5. the three entry points, the workspace, the status word -------------------------------------------------------------
def map_dev(occ, batch, strands, max_occ=1024, lead=37):
    """sbwtgpu_occurrences_map_dev on device buffers with guard records either side: (records, workspace status)"""
    import torch
    dev = torch.device("cuda", 0)
    bases, off = capi.concat_reads(enc(batch))
    n = len(batch)
    shifted = np.concatenate([np.frombuffer(b"ACGTN" * 8, dtype=np.uint8)[:lead], bases])      # d_read_off[0] != 0
    tb, to = torch.from_numpy(shifted).to(dev), torch.from_numpy(off + lead).to(dev)
    need = capi.Occurrences.workspace_bytes(len(shifted), n, strands)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    rec = torch.full(((n + 2 * GUARD) * 4,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    occ.map_dev(tb.data_ptr(), len(shifted), to.data_ptr(), n, rec.data_ptr() + 32 * GUARD, ws.data_ptr(), need, strands, max_occ,
                st.cuda_stream)
    status = occ.index.workspace_status(ws.data_ptr(), st.cuda_stream)
    st.synchronize()
    raw = rec.cpu().numpy()
    assert (raw[:4 * GUARD] == 0x5A5A5A5A5A5A5A5A).all() and (raw[4 * (GUARD + n):] == 0x5A5A5A5A5A5A5A5A).all()
    return raw[4 * GUARD:4 * (GUARD + n)].view(capi.READ_MAP_DTYPE).copy(), status


@pytest.mark.parametrize("rc,strands", [(False, 1), (True, 2)])
def test_dev_batch_and_chunked_batch_agree(world, reads, rc, strands):
    side = world.side(rc)
    rng = random.Random(46)
    batch = reads + [tp.scattered(world, T + 8, K, rng)]
    with build(side.idx, world.refs, strands) as occ:
        want = occ.map_reads(enc(batch), strands)
        got, status = map_dev(occ, batch, strands)
        assert status == 0 and np.array_equal(got, want)
        with tw.tuning("occurrences_chunk_bases", 1, 0):             # every read a chunk of its own
            assert np.array_equal(occ.map_reads(enc(batch), strands), want)
        with tw.tuning("occurrences_chunk_bases", 3000, 0):
            assert np.array_equal(occ.map_reads(enc(batch), strands), want)
        with tw.tuning("occurrences_map_table", 2, 0):
            got, status = map_dev(occ, batch, strands, 2)
            assert status == 0 and np.array_equal(got, occ.map_reads(enc(batch), strands, 2))


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_usable(world, reads):
    import torch
    L, C = capi.lib(), capi.C
    side = world.fwd
    idx = side.idx
    batch = enc(reads[:12])
    bases, off = capi.concat_reads(batch)
    n = len(batch)
    out = np.zeros(n, dtype=capi.READ_MAP_DTYPE)
    host = (bases.ctypes.data, off.ctypes.data)
    hv = C.c_void_p()
    with idx.occurrences_builder() as b:
        bh = b.handle
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_builder_create(None, C.byref(hv))), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_builder_create(idx.handle, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_builder_add_batch(None, 0, *host, n, 1, None, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_builder_add_batch(bh, 0, bases.ctypes.data, None, n, 1, None, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_builder_add_batch(bh, 0, None, off.ctypes.data, n, 1, None, None)), "NULL")
        for strands in (0, 3, -1):
            tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_builder_add_batch(bh, 0, *host, n, strands, None, None)), "strands")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_builder_add_batch(bh, 0, *host, -1, 1, None, None)), "n_reads")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_builder_add_batch(bh, -1, *host, n, 1, None, None)), "sequence numbers")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_builder_add_batch(bh, (1 << 30) - n + 1, *host, n, 1, None, None)), "sequence numbers")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_builder_add_batch(bh, (1 << 30) + 1, *host, 0, 1, None, None)), "sequence numbers")
        with pytest.raises(capi.SbwtGpuError) as ei:
            capi._check(L.sbwtgpu_occurrences_builder_add_batch(bh, 0, bases.ctypes.data, np.array([0, 1 << 31], dtype=np.int64).ctypes.data, 1, 1, None, None))
        assert ei.value.code == capi.ERR_READ_TOO_LONG
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_builder_finish(bh, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_builder_finish(None, C.byref(hv))), "NULL")
        b.add(enc(world.refs), 0, 1)                                 # nothing of the above reached the log
        occ = b.finish()
    with occ:
        h = occ.handle
        check_arrays(occ, side, numbered(world.refs, 1), "after the refusals")
        want = state(occ)
        good = occ.map_reads(batch)
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_upload(idx.handle, None, None, 0, C.byref(hv))), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_upload(idx.handle, off.ctypes.data, None, 3, C.byref(hv))), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_upload(idx.handle, off.ctypes.data, off.ctypes.data, -1, C.byref(hv))), "n_occ")
        for strands in (0, 3, -1):
            tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_map_batch(h, *host, n, strands, 16, out.ctypes.data)), "strands")
        for bad in (0, -1, (1 << 20) + 1):
            tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_map_batch(h, *host, n, 1, bad, out.ctypes.data)), "max_occ")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_map_batch(h, bases.ctypes.data, None, n, 1, 16, out.ctypes.data)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_map_batch(h, *host, n, 1, 16, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_map_batch(h, None, off.ctypes.data, n, 1, 16, out.ctypes.data)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_map_batch(h, *host, 1 << 31, 1, 16, out.ctypes.data)), "2^31 reads")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_offsets_copy(h, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_keys_copy(h, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_offsets_dev(h, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_keys_dev(h, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_to_positions(h, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_info(None, *([None] * 8))), "NULL")
        L.sbwtgpu_occurrences_destroy(None)
        L.sbwtgpu_occurrences_builder_destroy(None)
        # the device entry point: NULL pointers, strands, n_reads, max_occ, the workspace
        dev = torch.device("cuda", 0)
        d_bases, d_off = torch.from_numpy(bases.copy()).to(dev), torch.from_numpy(off.copy()).to(dev)
        d_out = torch.zeros(n * 4, dtype=torch.int64, device=dev)
        need = capi.Occurrences.workspace_bytes(len(bases), n, 2)
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        ok = (d_bases.data_ptr(), len(bases), d_off.data_ptr(), n)
        M = L.sbwtgpu_occurrences_map_dev
        tw.refused(lambda: capi._check(M(None, *ok, 1, 16, d_out.data_ptr(), ws.data_ptr(), need, None)), "NULL")
        tw.refused(lambda: capi._check(M(h, None, len(bases), d_off.data_ptr(), n, 1, 16, d_out.data_ptr(), ws.data_ptr(), need, None)), "NULL")
        tw.refused(lambda: capi._check(M(h, d_bases.data_ptr(), len(bases), None, n, 1, 16, d_out.data_ptr(), ws.data_ptr(), need, None)), "NULL")
        tw.refused(lambda: capi._check(M(h, *ok, 1, 16, None, ws.data_ptr(), need, None)), "NULL")
        tw.refused(lambda: capi._check(M(h, *ok, 1, 16, d_out.data_ptr(), None, need, None)), "workspace")
        tw.refused(lambda: capi._check(M(h, *ok, 2, 16, d_out.data_ptr(), ws.data_ptr(), capi.Occurrences.workspace_bytes(len(bases), n, 1), None)), "workspace")
        tw.refused(lambda: capi._check(M(h, *ok, 1, 16, d_out.data_ptr(), ws.data_ptr(), capi.Occurrences.workspace_bytes(len(bases), n, 1) - 1, None)), "workspace")
        tw.refused(lambda: capi._check(M(h, *ok, 3, 16, d_out.data_ptr(), ws.data_ptr(), need, None)), "strands")
        tw.refused(lambda: capi._check(M(h, *ok, 1, 0, d_out.data_ptr(), ws.data_ptr(), need, None)), "max_occ")
        tw.refused(lambda: capi._check(M(h, *ok, 1, (1 << 20) + 1, d_out.data_ptr(), ws.data_ptr(), need, None)), "max_occ")
        tw.refused(lambda: capi._check(M(h, d_bases.data_ptr(), len(bases), d_off.data_ptr(), -1, 1, 16, d_out.data_ptr(), ws.data_ptr(), need, None)), "n_reads")
        tw.refused(lambda: capi._check(M(h, d_bases.data_ptr(), -1, d_off.data_ptr(), n, 1, 16, d_out.data_ptr(), ws.data_ptr(), need, None)), "negative")
        torch.cuda.synchronize(dev)
        for big in (1 << 30, 1 << 31):
            o = np.array([0, big], dtype=np.int64)
            with pytest.raises(capi.SbwtGpuError) as ei:
                capi._check(L.sbwtgpu_occurrences_map_batch(h, bases.ctypes.data, o.ctypes.data, 1, 2, 16, out.ctypes.data))
            assert ei.value.code == capi.ERR_READ_TOO_LONG and "bases" in ei.value.msg
        with pytest.raises(capi.SbwtGpuError) as ei:
            capi._check(M(h, d_bases.data_ptr(), 1 << 30, d_off.data_ptr(), 1, 1, 16, d_out.data_ptr(), ws.data_ptr(), need, None))
        assert ei.value.code == capi.ERR_READ_TOO_LONG
        tw.refused(lambda: capi.set_tuning("occurrences_map_table", T + 1), "occurrences_map_table")
        # any output of info may be NULL; nothing of the above changed the object
        no = C.c_int64(-1)
        capi._check(L.sbwtgpu_occurrences_info(h, None, None, None, None, C.byref(no), None, None, None))
        assert no.value == want[2]["n_occurrences"]
        assert state(occ) == want and np.array_equal(occ.map_reads(batch), good)
    # a rank-only index
    bits = np.random.default_rng(1).integers(0, 2**64, size=4, dtype=np.uint64)
    ro = capi.Index.create(bits, bits, bits, bits, None, 256, 3)
    tw.refused(ro.occurrences_builder, "only rank()")
    tw.refused(lambda: capi.Occurrences.upload(ro, np.zeros(257, np.uint64), np.zeros(0, np.uint64)), "only rank()")
    ro.close()
    assert len(idx.search_reads([world.refs[0][:100].encode()])[0]) == 100 - K + 1


def test_index_of_2_pow_31_columns_is_refused(gpu):
    L, C = capi.lib(), capi.C
    n = 1 << 31
    w = np.zeros(n // 64, dtype=np.uint64)
    big = capi.Index.create(w, w, w, w, None, n, 31, 0, 0)
    tw.refused(big.occurrences_builder, "occurrences", "2^31", "columns")
    few = np.zeros(8, dtype=np.uint64)                                # (the arrays are not looked at: the size comes first)
    h = C.c_void_p()
    tw.refused(lambda: capi._check(L.sbwtgpu_occurrences_upload(big.handle, few.ctypes.data, few.ctypes.data, 0, C.byref(h))), "occurrences", "2^31", "columns")
    assert h.value is None
    big.close()


# ---- 7. the CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_occurrences(gpu, tmp_path):
    d = str(tmp_path)
    k = 11
    rng = random.Random(2770)
    core = rand_seq(rng, 400)
    # three reference files of two, one and two sequences: the sequences are numbered 0 .. 4 in the order they are read
    files = [[core[:250] + rand_seq(rng, 80), rand_seq(rng, 120)], [core[150:] + rand_seq(rng, 60)], [rand_seq(rng, 200), core[100:200] + rand_seq(rng, 50) + core[100:160]]]
    seqs = [s for f in files for s in f]
    colours = [c for c, f in enumerate(files) for _ in f]
    extra = rand_seq(rng, 90)
    SBWT = tw.SBWT
    with open(d + "/all.fna", "w") as fh, open(d + "/refs.txt", "w") as lst:
        for i, s in enumerate(seqs + [extra]):
            fh.write(">s%d\n%s\n" % (i, s))
        for c, f in enumerate(files):
            with open("%s/ref%d.fna" % (d, c), "w") as one:
                for s in f:
                    one.write(">r\n%s\n" % s)
            lst.write("%s/ref%d.fna\n" % (d, c))
    batch = []
    for i in range(50):
        src = (seqs + [extra])[i % 6]
        a = rng.randrange(0, len(src) - 20)
        r = mutate(rng, src[a:a + rng.randint(8, 90)], 0.03, "ACGTN" if i % 6 == 0 else "ACGT")
        batch.append(pb.revcomp(r) if i % 3 == 2 else r)
    batch += [seqs[0][200:240] + seqs[3][50:90], "ACG", rand_seq(rng, 60), seqs[4][150:210], seqs[2][0:60]]
    fastq = "".join("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)) for i, r in enumerate(batch))
    with open(d + "/reads.fastq", "w") as fh:
        fh.write(fastq)
    with gzip.open(d + "/reads.fastq.gz", "wt") as fh:
        fh.write(fastq)
    for rc in (False, True):
        tag = "rc" if rc else "fwd"
        index = "%s/%s.sbwt" % (d, tag)
        p = tw.run([SBWT, "build", "-i", d + "/all.fna", "-o", index, "-k", str(k), "--temp-dir", d] + (["--add-reverse-complements"] if rc else []))
        assert p.returncode == 0, p.stderr.decode()
        kmers = set()
        for s in seqs + [extra] + ([pb.revcomp(x) for x in seqs + [extra]] if rc else []):
            kmers |= {s[i:i + k] for i in range(len(s) - k + 1) if pb.valid(s[i:i + k])}
        strands = 2 if rc else 1
        both = ["--both-strands"] if rc else []
        want_occ = ob.table(kmers, k, numbered(seqs, strands))
        assert ob.scalars(want_occ)[2] >= 3
        occfile, posfile = "%s/%s.occ" % (d, tag), "%s/%s.pos" % (d, tag)
        # with and without --positions-out, from the same adds: the same occurrence file, and the position file of the option alone
        p = tw.run([SBWT, "build-colors", "--compress"] + both + ["-i", index, "-r", d + "/refs.txt", "-o", d + "/a.colors", "--occurrences-out", occfile,
                    "--positions-out", posfile, "--batch-bases", "300"])
        assert p.returncode == 0 and b"occurrences of" in p.stderr + p.stdout, p.stderr.decode()
        p = tw.run([SBWT, "build-colors"] + both + ["-i", index, "-r", d + "/refs.txt", "-o", d + "/b.colors", "--occurrences-out", d + "/alone.occ"])
        assert p.returncode == 0, p.stderr.decode()
        assert open(d + "/alone.occ", "rb").read() == open(occfile, "rb").read()
        p = tw.run([SBWT, "build-colors", "--compress"] + both + ["-i", index, "-r", d + "/refs.txt", "-o", d + "/c.colors", "--positions-out", d + "/alone.pos"])
        assert p.returncode == 0 and open(d + "/alone.pos", "rb").read() == open(posfile, "rb").read()
        assert open(d + "/c.colors", "rb").read() == open(d + "/a.colors", "rb").read()
        off, keys, fk, col, ln = hostlib.occurrences_read(occfile)
        assert fk == k and col.tolist() == colours and ln.tolist() == [len(s) for s in seqs]
        assert sorted(keys.tolist()) == sorted(f for v in want_occ.values() for f in v) and int(off[-1]) == len(keys)
        first = hostlib.positions_read(posfile)[0]
        has = np.diff(off.astype(np.int64)) > 0
        assert np.array_equal(first[has], keys[off[:-1][has].astype(np.int64)]) and (first[~has] == np.uint64(capi.POS_NONE)).all()
        for s2 in ((1, 2) if rc else (1,)):
            prof = rb.profiles(kmers, k, batch, s2)
            for max_occ in (None, 2):
                recs = ob.records(want_occ, kmers, k, batch, s2, max_occ or 1024)
                assert sum(1 for r in recs if r[1] >= 0) > 20 and len({r[1] for r in recs}) >= 3
                want = "".join("%d %d %d %d %s\n" % (tuple(pr) + (ob.cli_columns(r),)) for pr, r in zip(prof, recs)).encode()
                for query in (("reads.fastq",) if rc else ("reads.fastq", "reads.fastq.gz")):
                    out = "%s/%s.%d.hits" % (d, tag, s2)
                    cmd = [SBWT, "read-hits", "-i", index, "-q", d + "/" + query, "-o", out, "--occurrences", occfile,
                           "--batch-bases", "400"] + (["--both-strands"] if s2 == 2 else []) + (["--max-occ", str(max_occ)] if max_occ else [])
                    p = tw.run(cmd)
                    assert p.returncode == 0, p.stderr.decode()
                    assert open(out, "rb").read() == want, (tag, s2, query, max_occ)
            assert ob.records(want_occ, kmers, k, batch, s2, 2) != ob.records(want_occ, kmers, k, batch, s2, 1024)
            # without the options: byte for byte the table of the read-hit profiles
            p = tw.run([SBWT, "read-hits", "-i", index, "-q", d + "/reads.fastq", "-o", d + "/plain.hits", "--batch-bases", "400"] +
                       (["--both-strands"] if s2 == 2 else []))
            assert p.returncode == 0 and open(d + "/plain.hits", "rb").read() == rb.format_table(prof)
    base = [SBWT, "read-hits", "-i", d + "/fwd.sbwt", "-q", d + "/reads.fastq", "-o", d + "/x.hits"]
    # the exclusive options, --max-occ's bounds and its need of --occurrences
    p = tw.run(base + ["--occurrences", d + "/fwd.occ", "--positions", d + "/fwd.pos"])
    assert p.returncode == 1 and b"cannot be combined" in p.stderr
    for bad in ("0", "1048577", "x", "-3"):
        p = tw.run(base + ["--occurrences", d + "/fwd.occ", "--max-occ", bad])
        assert p.returncode == 1 and b"--max-occ" in p.stderr, bad
    p = tw.run(base + ["--max-occ", "5"])
    assert p.returncode == 1 and b"--occurrences" in p.stderr
    # an occurrence file of another index is refused, and so is a file that is none
    p = tw.run(base + ["--occurrences", d + "/rc.occ"])
    assert p.returncode == 1 and b"columns at k" in p.stderr
    p = tw.run(base + ["--occurrences", d + "/fwd.pos"])
    assert p.returncode == 1 and b"SBWTOCC1" in p.stderr


# ---- 8. a bounded fuzz ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_fuzz(gpu, seed):
    rng = random.Random(27000 + seed)
    k = rng.choice([2, 3, 7, 12, 21, 31, 32, 40, 64])
    alphabet = "ACGT" if k > 7 else "ACG" if k > 2 else "AC"
    rc = rng.random() < 0.5
    n_refs = rng.randint(2, 5)
    refs = [rand_seq(rng, rng.randint(k, 1500 if k > 3 else 300), alphabet) for _ in range(n_refs)]
    for _ in range(rng.randint(2, 8)):                               # planted repeats, forward and reverse-complemented
        src, dst = rng.randrange(n_refs), rng.randrange(n_refs)
        if len(refs[src]) < k + 10:
            continue
        a = rng.randrange(0, len(refs[src]) - k - 5)
        piece = refs[src][a:a + rng.randint(k, 200)]
        at = rng.randrange(0, len(refs[dst]) + 1)
        refs[dst] = refs[dst][:at] + (pb.revcomp(piece) if rng.random() < 0.3 else piece) + refs[dst][at:]
    extra = rand_seq(rng, 150, alphabet)
    side = tp.Side(refs + [extra], k, rc)
    first_seq = rng.choice([0, 0, 5, (1 << 30) - n_refs])
    table_strands, strands = rng.choice([1, 2]), rng.choice([1, 2])
    refs_numbered = numbered(refs, table_strands, first_seq)
    batch = []
    for i in range(40):
        kind = rng.randrange(6)
        s = rng.choice(refs + [extra])
        a = rng.randrange(0, max(1, len(s) - k))
        r = mutate(rng, s[a:a + rng.randint(1, 300)], rng.choice([0, 0.02, 0.1]), "ACGTN" if kind == 0 else alphabet)
        if kind == 1:
            t = rng.choice(refs)
            b = rng.randrange(0, max(1, len(t) - k))
            r += t[b:b + rng.randint(k, 120)]
        if kind == 2:
            r = rand_seq(rng, rng.randint(0, 200), alphabet)
        if kind == 3:
            r = "".join(rng.choice(refs)[x:x + k] for x in (rng.randrange(0, 50) for _ in range(rng.randint(2, 30))))
        batch.append(pb.revcomp(r) if rng.random() < 0.4 else r)
    cap = rng.choice([0, 1, 2, 8])
    max_occ = rng.choice([1, 2, 5, 1024, 1 << 20])
    with side.idx.occurrences_builder() as b:
        order = list(range(n_refs))
        rng.shuffle(order)
        with tw.tuning("occurrences_chunk_bases", rng.choice([0, 1, 500]), 0):
            for i in order[: n_refs // 2]:
                b.add(enc([refs[i]]), first_seq + i, table_strands)
            rest = sorted(order[n_refs // 2:])
            runs = [[rest[0]]]
            for i in rest[1:]:
                (runs[-1].append(i) if i == runs[-1][-1] + 1 else runs.append([i]))
            for run in runs:                                         # consecutive numbers in one batch
                b.add(enc([refs[i] for i in run]), first_seq + run[0], table_strands)
        occ = b.finish()
    with occ:
        want_occ = check_arrays(occ, side, refs_numbered, ("fuzz", seed, k, rc, table_strands))
        with tw.tuning("occurrences_map_table", cap, 0):
            check_map(occ, side, want_occ, batch, strands, max_occ, ("fuzz", seed, k, rc, table_strands, strands, cap, max_occ))
        with capi.Occurrences.upload(side.idx, occ.offsets(), occ.keys()) as up:
            assert np.array_equal(up.map_reads(enc(batch), strands, max_occ), occ.map_reads(enc(batch), strands, max_occ))
    side.idx.close()
