"""GPU: sbwtgpu_positions_* (sbwt_positions.hip: the smallest reference coordinate of every column's k-mer, and reads placed on
the references by diagonal voting) against the definition in tests/positions_brute.py.  Every comparison is exact: the whole
table on every column, and the map records field for field."""
import gzip
import random
import threading

import numpy as np
import pytest

import positions_brute as pb
import read_hits_brute as rb
import test_gpu_pseudoalign_wide as tw          # its helpers: make_index, labels_of, refused, run, tuning, SBWT
from sbwt_amd import capi, hostlib

pytestmark = pytest.mark.gpu

K = 15
T = capi.POSITIONS_MAP_TABLE
GUARD = 64


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, p, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) if rng.random() < p else c for c in s)


def enc(reads):
    return [r.encode("latin-1") if isinstance(r, str) else r for r in reads]


def numbered(seqs, strands, first_seq=0):
    return [(first_seq + i, s, strands) for i, s in enumerate(seqs)]


def hit_windows(kmers, k, seqs, strands):
    n = 0
    for s in seqs:
        for i in range(len(s) - k + 1):
            x = s[i:i + k]
            n += pb.valid(x) and (x in kmers or (strands == 2 and pb.revcomp(x) in kmers))
    return n


class Side:
    """One index over the world's sequences with its labels and k-mer set"""

    def __init__(self, seqs, k, rc):
        self.idx = tw.make_index([s for s in seqs if s], k, rc)
        self.labels = tw.labels_of(self.idx)
        self.kmers = {lab for lab in self.labels if "$" not in lab}
        self.k = k
        self.tables = {}

    def table(self, refs, strands):
        """the brute-force table of the references numbered 0, 1, ..., computed once per strands"""
        if strands not in self.tables:
            self.tables[strands] = pb.first_table(self.kmers, self.k, numbered(refs, strands))
        return self.tables[strands]

    def positions(self, refs, strands):
        pos = self.idx.positions()
        pos.add(enc(refs), 0, strands)
        return pos


class World:
    """Three references of some 5 000 bases that share stretches and carry repeats, and an index over them and a stretch that
    no reference holds: forward only, and with reverse complements."""

    def __init__(self):
        rng = random.Random(2626)
        core = rand_seq(rng, 3000)
        a = core + rand_seq(rng, 2000)
        b = rand_seq(rng, 1500) + mutate(rng, core[500:2500], 0.02) + rand_seq(rng, 1000)
        c = rand_seq(rng, 2500) + a[3200:3600] + rand_seq(rng, 1200) + a[100:400]      # repeats of sequence 0 in sequence 2
        a = a + a[1000:1200] + rand_seq(rng, 300)                                        # and a repeat within sequence 0
        b = b[:700] + "N" + b[701:1400] + "acgt" + b[1404:]                              # bytes that end windows
        self.refs = [a, b, c]
        self.extra = rand_seq(rng, 600)                  # k-mers of the index without a position
        self.seqs = self.refs + [self.extra]
        self.fwd = Side(self.seqs, K, False)
        self.rc = Side(self.seqs, K, True)
        self.rng = random.Random(2627)

    def side(self, rc):
        return self.rc if rc else self.fwd

    def piece(self, n_windows, p=0.0, flip=False, src=None):
        """a read of n_windows windows drawn from a reference, with substitutions at rate p, reverse-complemented if asked"""
        rng = self.rng
        s = self.refs[rng.randrange(3) if src is None else src]
        n = n_windows + K - 1
        a = rng.randrange(0, len(s) - n)
        r = mutate(rng, s[a:a + n], p)
        return pb.revcomp(r) if flip else r


@pytest.fixture(scope="module")
def world(gpu):
    w = World()
    assert 10000 <= w.fwd.idx.n_nodes <= 40000 and w.rc.idx.n_nodes > w.fwd.idx.n_nodes
    yield w
    w.fwd.idx.close()
    w.rc.idx.close()


@pytest.fixture(scope="module")
def reads(world):
    """the sample of the map tests: every length class, clean and with substitutions, both orientations, and the special reads"""
    w, rng = world, world.rng
    out = []
    for n_windows in (1, 63, 64, 65, 127, 128, 129, 700):
        for p in (0.0, 0.01, 0.05):
            for flip in (False, True):
                out.append(w.piece(n_windows, p, flip))
    a, b, c = w.refs
    # a run that starts in the last lane of an iteration and goes on in the next: 63 windows that miss, then the reference
    # (the last of the 63 bases in front differs from the reference's, so window 62 is no window of the reference)
    out.append(rand_seq(rng, 62) + pb.COMP[a[1999]] + a[2000:2000 + 100])
    # overhang at both ends of a reference, forward and reverse-complemented
    out += [rand_seq(rng, 20) + a[:80], a[-80:] + rand_seq(rng, 20), pb.revcomp(rand_seq(rng, 20) + c[:80]), pb.revcomp(c[-80:] + rand_seq(rng, 20))]
    # ties (two placements of equal votes, in either order on the read) and chimeras
    out += [a[4100:4130] + c[300:330], c[300:330] + a[4100:4130], a[4100:4130] + pb.revcomp(c[300:330])]
    out += [a[4000:4100] + b[200:260], b[200:260] + pb.revcomp(a[4000:4100]), c[100:180] + a[4500:4560] + b[3000:3100]]
    # repeats: a stretch of sequence 2 that sequence 0 holds first, and the repeat within sequence 0
    out += [c[2480:2560], a[-520:-280], c[-320:]]
    # hits without a position, misses, short and odd reads
    out += [w.extra[100:300], w.extra[:K], rand_seq(rng, 200), "ACGT", "", "A" * (K - 1), a[3000:3000 + K], a[10:90].lower(),
            a[10:50] + "N" + a[51:120], b[650:760], b[1380:1450]]
    return out


def check_table(pos, side, refs_numbered, label=None):
    """the object's table on every column, and its scalars, against the brute force"""
    first = pb.first_table(side.kmers, side.k, refs_numbered)
    got = pos.first()
    assert got.dtype == np.uint64 and got.tolist() == pb.table_array(first, side.labels), label
    info = pos.info()
    nw, nh = pb.scalars(side.kmers, side.k, refs_numbered)
    assert (info["n_columns"], info["k"], info["n_windows"], info["n_hits"], info["n_positioned"]) == \
        (side.idx.n_nodes, side.k, nw, nh, len(first)), (label, info)
    assert info["device_bytes"] >= 8 * side.idx.n_nodes
    return first


# ---- 1. the table against the brute force, at every k -------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 5, 16, 31, 32, 33, 63, 64, 65])
def test_table_against_brute(gpu, k):
    rng = random.Random(900 + k)
    alphabet = "ACGT" if k > 5 else "AC" if k == 2 else "ACG"
    base = rand_seq(rng, 400, alphabet)
    refs = [base + rand_seq(rng, 100, alphabet), rand_seq(rng, 150, alphabet) + base[100:350] + "N" + rand_seq(rng, 90, alphabet),
            pb.revcomp(base[50:300]) + rand_seq(rng, 70, alphabet), "ACG"[:min(k - 1, 3)], ""]
    extra = [rand_seq(rng, 120, alphabet)]
    for rc in (False, True):
        side = Side(refs + extra, k, rc)
        for strands in (1, 2):
            with side.idx.positions() as pos:
                nw, nh = pos.add(enc(refs), 0, strands)
                assert nw == sum(max(len(s) - k + 1, 0) for s in refs) and nh == hit_windows(side.kmers, k, refs, strands)
                first = check_table(pos, side, numbered(refs, strands), (k, rc, strands))
                got = pos.first()
                # independently of the brute force: the reference window at the decoded position spells the column's k-mer
                n_t1 = 0
                for v in np.flatnonzero(got != np.uint64(capi.POS_NONE)).tolist():
                    seq, p, t = pb.decode(int(got[v]))
                    x = refs[seq][p:p + k]
                    assert len(x) == k and side.labels[v] == (pb.revcomp(x) if t else x), (k, rc, strands, v)
                    n_t1 += t
                # (refs[2] holds a reverse-complemented stretch of refs[0]: with two strands sequence 0 takes those columns, t = 1)
                assert n_t1 == 0 if strands == 1 else (n_t1 > 0 or k == 2), (k, rc, strands)
                # the columns with a position are the columns the colour builder marks for the same adds
                with capi.ColorSetsBuilder.create(side.idx, 1) as b:
                    b.add_reads(0, enc(refs), strands == 2)
                    with b.finish() as sets:
                        assert sets.info()["n_colored_columns"] == len(first) == pos.info()["n_positioned"]
        side.idx.close()


@pytest.mark.parametrize("level", [1, 2])
def test_image_levels(world, level):
    with tw.tuning("image_level", level, 0):
        idx = tw.make_index(world.seqs, K, True)
    assert idx.image_level == level and idx.n_nodes == world.rc.idx.n_nodes
    with idx.positions() as pos, world.rc.positions(world.refs, 2) as want:
        pos.add(enc(world.refs), 0, 2)
        assert np.array_equal(pos.first(), want.first()) and pos.info() == want.info()
    idx.close()


# ---- 2. order, chunking, threads, numbers, upload -------------------------------------------------------------------------
def state(pos):
    return pos.first().tobytes(), pos.info()


@pytest.mark.parametrize("rc,strands", [(False, 1), (True, 2)])
def test_order_and_chunking(world, rc, strands):
    side = world.side(rc)
    with side.positions(world.refs, strands) as one:
        check_table(one, side, numbered(world.refs, strands), "one batch")
        want = state(one)
        with side.idx.positions() as pos:                            # one by one, in reverse order
            for i in reversed(range(3)):
                pos.add(enc([world.refs[i]]), i, strands)
            assert state(pos) == want
            pos.reset()
            assert pos.info()["n_positioned"] == 0 and pos.info()["n_windows"] == 0
            assert not (pos.first() != np.uint64(capi.POS_NONE)).any()
            with tw.tuning("positions_chunk_bases", 1, 0):           # every sequence a chunk of its own
                pos.add(enc(world.refs), 0, strands)
            assert state(pos) == want
        with side.idx.positions() as pos:                            # two host threads on disjoint halves
            errors = []

            def work(seqs, first_seq):
                try:
                    pos.add(enc(seqs), first_seq, strands)
                except Exception as e:                               # noqa: BLE001
                    errors.append(e)

            th = [threading.Thread(target=work, args=(world.refs[:2], 0)), threading.Thread(target=work, args=(world.refs[2:], 2))]
            for t in th:
                t.start()
            for t in th:
                t.join()
            assert not errors and state(pos) == want
            first = pos.first().copy()
            pos.add(enc(world.refs), 0, strands)                     # adding everything again changes the windows counted only
            assert np.array_equal(pos.first(), first) and pos.info()["n_windows"] == 2 * want[1]["n_windows"]


def test_two_numbers_leave_the_smaller(world):
    side = world.fwd
    s = world.refs[1]
    with side.idx.positions() as pos:
        pos.add(enc([s]), 3)
        f3 = pos.first().copy()
        assert set((f3[f3 != np.uint64(capi.POS_NONE)] >> np.uint64(32)).tolist()) == {3}
        pos.add(enc([s]), 1)
        check_table(pos, side, [(3, s, 1), (1, s, 1)], "3 then 1")
        f = pos.first()
        assert set((f[f != np.uint64(capi.POS_NONE)] >> np.uint64(32)).tolist()) == {1}
        assert np.array_equal(f & np.uint64(0xFFFFFFFF), f3 & np.uint64(0xFFFFFFFF))
        pos.add(enc([s]), 3)
        assert np.array_equal(pos.first(), f)
        pos.add(enc([s]), (1 << 30) - 1)                             # the largest number there is
        assert np.array_equal(pos.first(), f)


def test_upload_maps_identically_and_refuses_damage(world, reads):
    side = world.rc
    with side.positions(world.refs, 2) as pos:
        first = pos.first()
        want = pos.map_reads(enc(reads), 2)
        with capi.Positions.upload(side.idx, first) as up:
            assert np.array_equal(up.first(), first)
            info = up.info()
            assert info["n_positioned"] == pos.info()["n_positioned"] and (info["n_windows"], info["n_hits"]) == (0, 0)
            assert np.array_equal(up.map_reads(enc(reads), 2), want)
            up.add(enc(world.refs[:1]), 0, 2)                        # an uploaded object takes adds like any other
            assert np.array_equal(up.first(), first)
        for v, value in ((0, 1 << 62), (side.idx.n_nodes - 1, (1 << 64) - 2), (side.idx.n_nodes // 2, (1 << 30) << 32)):
            bad = first.copy()
            bad[v] = value
            tw.refused(lambda: capi.Positions.upload(side.idx, bad), "first", "2^30")
        ok = first.copy()
        ok[0] = (((1 << 30) - 1) << 32) | 0xFFFFFFFF                 # the largest key there is
        capi.Positions.upload(side.idx, ok).close()
        with pytest.raises(ValueError):
            capi.Positions.upload(side.idx, first[:-1])


# ---- 3. the map against the brute force -----------------------------------------------------------------------------------
def check_map(pos, side, first, batch, strands, label=None):
    got = pos.map_reads(enc(batch), strands)
    assert got.dtype == capi.READ_MAP_DTYPE and len(got) == len(batch)
    want = pb.records(first, side.kmers, side.k, batch, strands)
    tuples = pb.as_tuples(got)
    for i, (g, x) in enumerate(zip(tuples, want)):
        assert g == x, (label, i, len(batch[i]), g, x)
    return want


@pytest.mark.parametrize("rc,table_strands,strands", [(False, 1, 1), (False, 1, 2), (True, 2, 1), (True, 2, 2), (True, 1, 2)])
def test_map_against_brute(world, reads, rc, table_strands, strands):
    side = world.side(rc)
    first = side.table(world.refs, table_strands)
    with side.positions(world.refs, table_strands) as pos:
        want = check_map(pos, side, first, reads, strands, (rc, table_strands, strands))
        # the sample is what its comments say: placed reads of both orientations, overhangs, ties, runner-ups, reads without
        # an anchor, and n_found where nothing is anchored
        assert sum(1 for r in want if r[1] >= 0) > 30 and any(r[0] < 0 for r in want)
        assert any(r[3] == r[4] > 0 for r in want) and any(0 < r[4] < r[3] for r in want)
        assert any(r[6] == 0 and r[5] > 0 for r in want) and any(r[5] == 0 for r in want)
        if strands == 2 or rc:
            assert any(r[2] == 1 for r in want) and any(r[2] == 0 and r[1] >= 0 for r in want)
        if strands == 1:
            hits = side.idx.read_hits_reads(enc(reads))
            assert [r[5] for r in want] == hits[:, 1].tolist()       # n_found is read-hits' with one strand
        # an empty batch, and a batch of empty reads
        assert len(pos.map_reads([], strands)) == 0
        assert pb.as_tuples(pos.map_reads([b"", b""], strands)) == [(0, -1, 0, 0, 0, 0, 0)] * 2


def test_the_run_across_an_iteration_edge_is_what_it_says(world, reads):
    side = world.fwd
    first = side.table(world.refs, 1)
    read = next(r for r in reads if len(r) == 163 and r[63:] == world.refs[0][2000:2100])
    cnt, found, anchored = pb.votes(first, side.kmers, K, read)
    hits = rb.hits(side.kmers, K, read)
    assert hits[:63] == [0] * 63 and all(hits[63:]) and len(hits) == 149          # the first hit sits in lane 63 of iteration 0
    assert cnt == {(0, 0, 2000 - 63): 86} and (found, anchored) == (86, 86)
    with side.positions(world.refs, 1) as pos:
        assert pb.as_tuples(pos.map_reads(enc([read]))) == [(1937, 0, 0, 86, 0, 86, 86)]


# ---- 4. the placement table's edge -----------------------------------------------------------------------------------------
def scattered(world, n_pieces, piece_len, rng):
    """a read of pieces taken from scattered offsets of the references: every piece votes for a placement of its own"""
    out = []
    for j in range(n_pieces):
        s = world.refs[j % 3]
        a = rng.randrange(0, len(s) - piece_len)
        out.append(s[a:a + piece_len])
    return "".join(out)


@pytest.mark.parametrize("rc,strands", [(False, 1), (True, 2)])
def test_table_edge_with_a_small_capacity(world, reads, rc, strands):
    side = world.side(rc)
    first = side.table(world.refs, strands)
    rng = random.Random(44)
    edge = {}
    while len(edge) < 5:                                             # reads with exactly 1 .. 5 distinct placements
        n = 1 + len(edge)
        r = scattered(world, n, 24, rng)
        if pb.n_placements(first, side.kmers, K, r, strands) == n:
            edge[n] = r
    batch = reads[:20] + [edge[3], edge[4], edge[5]] + reads[20:40] + [edge[5], edge[1], edge[4]] + reads[40:]
    assert [pb.n_placements(first, side.kmers, K, r, strands) for r in (edge[3], edge[4], edge[5])] == [3, 4, 5]
    with side.positions(world.refs, strands) as pos:
        want = pos.map_reads(enc(batch), strands)                    # the compiled capacity
        for cap in (4, 3, 1, 5):
            with tw.tuning("positions_map_table", cap, 0):
                check_map(pos, side, first, batch, strands, ("capacity", cap))
                assert np.array_equal(pos.map_reads(enc(batch), strands), want)


def test_a_read_beyond_the_compiled_capacity(world, reads):
    rng = random.Random(45)
    for rc, strands in ((False, 1), (True, 2)):
        side = world.side(rc)
        first = side.table(world.refs, strands)
        big = scattered(world, T + 8, K, rng)               # (a few pieces more than T + 1: one that falls on the N votes for nothing)
        at = scattered(world, T - 2, K, rng)
        n_big, n_at = (pb.n_placements(first, side.kmers, K, r, strands) for r in (big, at))
        assert n_big > T >= n_at > T - 16 and len(big) == (T + 8) * K, (n_big, n_at)
        # both kernels write into one output: the overflowing reads stand among ordinary ones
        batch = reads[:30] + [big] + reads[30:60] + [at, pb.revcomp(big)] + reads[60:] + [big]
        with side.positions(world.refs, strands) as pos:
            check_map(pos, side, first, batch, strands, ("beyond", rc, strands, n_big, n_at))


# ---- 5. the three entry points, the workspace, the status word -------------------------------------------------------------
def map_dev(pos, batch, strands, short_by=0, lead=37):
    """sbwtgpu_positions_map_dev on device buffers with guard records either side: (records, workspace status)"""
    import torch
    dev = torch.device("cuda", 0)
    bases, off = capi.concat_reads(enc(batch))
    n = len(batch)
    shifted = np.concatenate([np.frombuffer(b"ACGTN" * 8, dtype=np.uint8)[:lead], bases])      # d_read_off[0] != 0
    tb, to = torch.from_numpy(shifted).to(dev), torch.from_numpy(off + lead).to(dev)
    need = capi.Positions.workspace_bytes(len(shifted), n, strands)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    rec = torch.full(((n + 2 * GUARD) * 4,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    pos.map_dev(tb.data_ptr(), len(shifted), to.data_ptr(), n, rec.data_ptr() + 32 * GUARD, ws.data_ptr(), need - short_by, strands,
                st.cuda_stream)
    status = pos.index.workspace_status(ws.data_ptr(), st.cuda_stream)
    st.synchronize()
    raw = rec.cpu().numpy()
    assert (raw[:4 * GUARD] == 0x5A5A5A5A5A5A5A5A).all() and (raw[4 * (GUARD + n):] == 0x5A5A5A5A5A5A5A5A).all()
    return raw[4 * GUARD:4 * (GUARD + n)].view(capi.READ_MAP_DTYPE).copy(), status


@pytest.mark.parametrize("rc,strands", [(False, 1), (True, 2)])
def test_dev_batch_and_chunked_batch_agree(world, reads, rc, strands):
    side = world.side(rc)
    rng = random.Random(46)
    batch = reads + [scattered(world, T + 8, K, rng)]
    with side.positions(world.refs, strands) as pos:
        want = pos.map_reads(enc(batch), strands)
        got, status = map_dev(pos, batch, strands)
        assert status == 0 and np.array_equal(got, want)
        with tw.tuning("positions_chunk_bases", 1, 0):               # every read a chunk of its own
            assert np.array_equal(pos.map_reads(enc(batch), strands), want)
        with tw.tuning("positions_chunk_bases", 3000, 0):
            assert np.array_equal(pos.map_reads(enc(batch), strands), want)
        with tw.tuning("positions_map_table", 2, 0):
            got, status = map_dev(pos, batch, strands)
            assert status == 0 and np.array_equal(got, want)


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
    with side.positions(world.refs, 1) as pos:
        h = pos.handle
        want = state(pos)
        good = pos.map_reads(batch)
        host = (bases.ctypes.data, off.ctypes.data)
        hv = C.c_void_p()
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_create(None, C.byref(hv))), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_create(idx.handle, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_upload(idx.handle, None, C.byref(hv))), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_add_batch(None, 0, *host, n, 1, None, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_add_batch(h, 0, bases.ctypes.data, None, n, 1, None, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_add_batch(h, 0, None, off.ctypes.data, n, 1, None, None)), "NULL")
        for strands in (0, 3, -1):
            tw.refused(lambda: capi._check(L.sbwtgpu_positions_add_batch(h, 0, *host, n, strands, None, None)), "strands")
            tw.refused(lambda: capi._check(L.sbwtgpu_positions_map_batch(h, *host, n, strands, out.ctypes.data)), "strands")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_add_batch(h, 0, *host, -1, 1, None, None)), "n_reads")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_add_batch(h, -1, *host, n, 1, None, None)), "sequence numbers")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_add_batch(h, (1 << 30) - n + 1, *host, n, 1, None, None)), "sequence numbers")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_add_batch(h, (1 << 30) + 1, *host, 0, 1, None, None)), "sequence numbers")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_map_batch(h, bases.ctypes.data, None, n, 1, out.ctypes.data)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_map_batch(h, *host, n, 1, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_map_batch(h, None, off.ctypes.data, n, 1, out.ctypes.data)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_map_batch(h, *host, 1 << 31, 1, out.ctypes.data)), "2^31 reads")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_first_copy(h, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_first_dev(h, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_info(None, None, None, None, None, None, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_reset(None)), "NULL")
        L.sbwtgpu_positions_destroy(None)
        # the device entry point: NULL pointers, strands, n_reads, the workspace
        dev = torch.device("cuda", 0)
        d_bases, d_off = torch.from_numpy(bases.copy()).to(dev), torch.from_numpy(off.copy()).to(dev)
        d_out = torch.zeros(n * 4, dtype=torch.int64, device=dev)
        need = capi.Positions.workspace_bytes(len(bases), n, 2)
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        ok = (d_bases.data_ptr(), len(bases), d_off.data_ptr(), n)
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_map_dev(None, *ok, 1, d_out.data_ptr(), ws.data_ptr(), need, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_map_dev(h, None, len(bases), d_off.data_ptr(), n, 1, d_out.data_ptr(), ws.data_ptr(), need, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_map_dev(h, d_bases.data_ptr(), len(bases), None, n, 1, d_out.data_ptr(), ws.data_ptr(), need, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_map_dev(h, *ok, 1, None, ws.data_ptr(), need, None)), "NULL")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_map_dev(h, *ok, 1, d_out.data_ptr(), None, need, None)), "workspace")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_map_dev(h, *ok, 2, d_out.data_ptr(), ws.data_ptr(),
                                                                 capi.Positions.workspace_bytes(len(bases), n, 1), None)), "workspace")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_map_dev(h, *ok, 1, d_out.data_ptr(), ws.data_ptr(),
                                                                 capi.Positions.workspace_bytes(len(bases), n, 1) - 1, None)), "workspace")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_map_dev(h, *ok, 3, d_out.data_ptr(), ws.data_ptr(), need, None)), "strands")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_map_dev(h, d_bases.data_ptr(), len(bases), d_off.data_ptr(), -1, 1, d_out.data_ptr(),
                                                                 ws.data_ptr(), need, None)), "n_reads")
        tw.refused(lambda: capi._check(L.sbwtgpu_positions_map_dev(h, d_bases.data_ptr(), -1, d_off.data_ptr(), n, 1, d_out.data_ptr(),
                                                                 ws.data_ptr(), need, None)), "negative")
        torch.cuda.synchronize(dev)
        # a read of 2^30 bases or more in the map calls, a sequence of 2^31 in an add: from the offsets alone
        for big, code_map in ((1 << 30, capi.ERR_READ_TOO_LONG), (1 << 31, capi.ERR_READ_TOO_LONG)):
            o = np.array([0, big], dtype=np.int64)
            with pytest.raises(capi.SbwtGpuError) as ei:
                capi._check(L.sbwtgpu_positions_map_batch(h, bases.ctypes.data, o.ctypes.data, 1, 2, out.ctypes.data))
            assert ei.value.code == code_map and "bases" in ei.value.msg
        with pytest.raises(capi.SbwtGpuError) as ei:
            capi._check(L.sbwtgpu_positions_map_dev(h, d_bases.data_ptr(), 1 << 30, d_off.data_ptr(), 1, 1, d_out.data_ptr(), ws.data_ptr(), need, None))
        assert ei.value.code == capi.ERR_READ_TOO_LONG
        with pytest.raises(capi.SbwtGpuError) as ei:
            capi._check(L.sbwtgpu_positions_add_batch(h, 0, bases.ctypes.data, np.array([0, 1 << 31], dtype=np.int64).ctypes.data, 1, 1, None, None))
        assert ei.value.code == capi.ERR_READ_TOO_LONG
        tw.refused(lambda: capi.set_tuning("positions_map_table", T + 1), "positions_map_table")
        # any output of info may be NULL; nothing of the above changed the object
        np_ = C.c_int64(-1)
        capi._check(L.sbwtgpu_positions_info(h, None, None, None, None, C.byref(np_), None))
        assert np_.value == want[1]["n_positioned"]
        p = C.c_void_p()
        capi._check(L.sbwtgpu_positions_first_dev(h, C.byref(p)))
        assert p.value and pos.first_dev() == p.value
        assert state(pos) == want and np.array_equal(pos.map_reads(batch), good)
    # a rank-only index
    bits = np.random.default_rng(1).integers(0, 2**64, size=4, dtype=np.uint64)
    ro = capi.Index.create(bits, bits, bits, bits, None, 256, 3)
    tw.refused(ro.positions, "only rank()")
    tw.refused(lambda: capi.Positions.upload(ro, np.zeros(256, np.uint64)), "only rank()")
    ro.close()
    assert len(idx.search_reads([world.refs[0][:100].encode()])[0]) == 100 - K + 1


def test_index_of_2_pow_31_columns_is_refused(gpu):
    """Refused for its size before anything else, by create and by upload: any bits make an index that answers rank()."""
    L, C = capi.lib(), capi.C
    n = 1 << 31
    w = np.zeros(n // 64, dtype=np.uint64)
    big = capi.Index.create(w, w, w, w, None, n, 31, 0, 0)
    tw.refused(big.positions, "positions", "2^31", "columns")
    few = np.full(8, capi.POS_NONE, dtype=np.uint64)                  # (the table is not looked at: the size comes first)
    h = C.c_void_p()
    tw.refused(lambda: capi._check(L.sbwtgpu_positions_upload(big.handle, few.ctypes.data, C.byref(h))), "positions", "2^31", "columns")
    assert h.value is None
    big.close()


# ---- 7. the CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_positions(gpu, tmp_path):
    d = str(tmp_path)
    k = 11
    rng = random.Random(70)
    core = rand_seq(rng, 400)
    # three reference files of two, one and two sequences: the sequences are numbered 0 .. 4 in the order they are read
    files = [[core[:250] + rand_seq(rng, 80), rand_seq(rng, 120)], [core[150:] + rand_seq(rng, 60)], [rand_seq(rng, 200), core[100:200] + rand_seq(rng, 50)]]
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
    reads = []
    for i in range(50):
        src = (seqs + [extra])[i % 6]
        a = rng.randrange(0, len(src) - 20)
        r = mutate(rng, src[a:a + rng.randint(8, 90)], 0.03, "ACGTN" if i % 6 == 0 else "ACGT")
        reads.append(pb.revcomp(r) if i % 3 == 2 else r)
    reads += [seqs[0][200:240] + seqs[3][50:90], "ACG", rand_seq(rng, 60)]
    fastq = "".join("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)) for i, r in enumerate(reads))
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
        first = pb.first_table(kmers, k, numbered(seqs, strands))
        files_first = []
        modes = ((["--compress"], "sets"), (["--compress", "--stream"], "stream"), (["--wide"], "wide"), ([], "narrow"))
        for flags, name in (modes[:1] + modes[3:] if rc else modes):      # (every colour mode once, on the forward index)
            posfile = "%s/%s.%s.pos" % (d, tag, name)
            cmd = [SBWT, "build-colors"] + flags + both + ["-i", index, "-r", d + "/refs.txt", "-o", "%s/%s.%s.colors" % (d, tag, name),
                                                            "--positions-out", posfile, "--batch-bases", "300"]
            p = tw.run(cmd)
            assert p.returncode == 0, p.stderr.decode()
            f, fk, col, ln = hostlib.positions_read(posfile)
            assert fk == k and col.tolist() == colours and ln.tolist() == [len(s) for s in seqs], name
            assert sorted(f[f != np.uint64(capi.POS_NONE)].tolist()) == sorted(first.values()), name
            files_first.append(f.tobytes())
        assert len(set(files_first)) == 1                             # the colour mode does not show in the position file
        # the colour file is what it is without the option
        p = tw.run([SBWT, "build-colors", "--compress"] + both + ["-i", index, "-r", d + "/refs.txt", "-o", d + "/plain.colors"])
        assert p.returncode == 0 and open(d + "/plain.colors", "rb").read() == open("%s/%s.sets.colors" % (d, tag), "rb").read()
        for s2 in ((1, 2) if rc else (1,)):
            prof = rb.profiles(kmers, k, reads, s2)
            recs = pb.records(first, kmers, k, reads, s2)
            assert sum(1 for r in recs if r[1] >= 0) > 20 and len({r[1] for r in recs}) >= 3
            want = "".join("%d %d %d %d %s\n" % (tuple(pr) + (pb.cli_columns(r),)) for pr, r in zip(prof, recs)).encode()
            for query in (("reads.fastq",) if rc else ("reads.fastq", "reads.fastq.gz")):
                out = "%s/%s.%d.hits" % (d, tag, s2)
                cmd = [SBWT, "read-hits", "-i", index, "-q", d + "/" + query, "-o", out, "--positions", "%s/%s.sets.pos" % (d, tag),
                       "--batch-bases", "400"] + (["--both-strands"] if s2 == 2 else [])
                p = tw.run(cmd)
                assert p.returncode == 0, p.stderr.decode()
                assert open(out, "rb").read() == want, (tag, s2, query)
            # without the option: byte for byte the table of the read-hit profiles
            p = tw.run([SBWT, "read-hits", "-i", index, "-q", d + "/reads.fastq", "-o", d + "/plain.hits", "--batch-bases", "400"] +
                       (["--both-strands"] if s2 == 2 else []))
            assert p.returncode == 0 and open(d + "/plain.hits", "rb").read() == rb.format_table(prof)
    # a position file of another index is refused, and so is a file that is none
    p = tw.run([SBWT, "read-hits", "-i", d + "/fwd.sbwt", "-q", d + "/reads.fastq", "-o", d + "/x.hits", "--positions", d + "/rc.sets.pos"])
    assert p.returncode == 1 and b"columns at k" in p.stderr
    p = tw.run([SBWT, "read-hits", "-i", d + "/fwd.sbwt", "-q", d + "/reads.fastq", "-o", d + "/x.hits", "--positions", d + "/fwd.sets.colors"])
    assert p.returncode == 1 and b"SBWTPOS1" in p.stderr


# ---- 8. a bounded fuzz ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_fuzz(gpu, seed):
    rng = random.Random(7000 + seed)
    k = rng.choice([3, 7, 12, 21, 31, 32, 40])
    alphabet = "ACGT" if k > 7 else "ACG"
    rc = rng.random() < 0.5
    n_refs = rng.randint(2, 5)
    refs = [rand_seq(rng, rng.randint(k, 1500), alphabet) for _ in range(n_refs)]
    for _ in range(rng.randint(2, 8)):                               # planted repeats, forward and reverse-complemented
        src, dst = rng.randrange(n_refs), rng.randrange(n_refs)
        if len(refs[src]) < k + 10:
            continue
        a = rng.randrange(0, len(refs[src]) - k - 5)
        piece = refs[src][a:a + rng.randint(k, 200)]
        at = rng.randrange(0, len(refs[dst]) + 1)
        refs[dst] = refs[dst][:at] + (pb.revcomp(piece) if rng.random() < 0.3 else piece) + refs[dst][at:]
    extra = rand_seq(rng, 150, alphabet)
    side = Side(refs + [extra], k, rc)
    first_seq = rng.choice([0, 0, 5, (1 << 30) - n_refs])
    table_strands, strands = rng.choice([1, 2]), rng.choice([1, 2])
    refs_numbered = numbered(refs, table_strands, first_seq)
    batch = []
    for i in range(60):
        kind = rng.randrange(6)
        s = rng.choice(refs + [extra])
        a = rng.randrange(0, max(1, len(s) - k))
        r = mutate(rng, s[a:a + rng.randint(1, 400)], rng.choice([0, 0.02, 0.1]), "ACGTN" if kind == 0 else alphabet)
        if kind == 1:
            t = rng.choice(refs)
            b = rng.randrange(0, max(1, len(t) - k))
            r += t[b:b + rng.randint(k, 120)]
        if kind == 2:
            r = rand_seq(rng, rng.randint(0, 300), alphabet)
        if kind == 3:
            r = "".join(rng.choice(refs)[x:x + k] for x in (rng.randrange(0, 50) for _ in range(rng.randint(2, 30))))
        batch.append(pb.revcomp(r) if rng.random() < 0.4 else r)
    cap = rng.choice([0, 1, 2, 8])
    with side.idx.positions() as pos:
        order = list(range(n_refs))
        rng.shuffle(order)
        with tw.tuning("positions_chunk_bases", rng.choice([0, 1, 500]), 0):
            for i in order[: n_refs // 2]:
                pos.add(enc([refs[i]]), first_seq + i, table_strands)
            rest = sorted(order[n_refs // 2:])
            runs = [[rest[0]]]
            for i in rest[1:]:
                (runs[-1].append(i) if i == runs[-1][-1] + 1 else runs.append([i]))
            for run in runs:                                         # consecutive numbers in one batch
                pos.add(enc([refs[i] for i in run]), first_seq + run[0], table_strands)
        first = check_table(pos, side, refs_numbered, ("fuzz", seed, k, rc, table_strands))
        with tw.tuning("positions_map_table", cap, 0):
            check_map(pos, side, first, batch, strands, ("fuzz", seed, k, rc, table_strands, strands, cap))
    side.idx.close()
