"""GPU: sbwtgpu_pileup_* (sbwt_pileup.hip: per-base counters of a read set's alignments that live on the device across adds)
against the definition in tests/pileup_brute.py.  Every comparison is exact: every base of every sequence through counts_copy
and counts_dev, the scalars, and the calls record for record."""
import random
import threading

import numpy as np
import pytest

import align_brute as ab
import pileup_brute as pb
import verify_brute as vb
from sbwt_amd import capi, hostlib
from test_gpu_align import make_sample
from test_gpu_verify import GUARD, World, map_records, mutate, rand_seq, refused

pytestmark = pytest.mark.gpu

SHORT = (1, 63, 64, 65, 128, 70)        # packed next to each other: a sequence of 64 m bases ends on its neighbour's first slot


def records(recs, votes=None):
    """map records with (votes, votes2) set where given (map_records leaves the same junk in both)"""
    m = map_records(recs)
    if votes is not None:
        for i, (v, v2) in enumerate(votes):
            m[i]["votes"], m[i]["votes2"] = v, v2
    return m


def as_rows(arr):
    assert arr.dtype == capi.PILEUP_BASE_DTYPE
    return arr.view(np.uint32).reshape(-1, 8)


def counts_dev(pl, seq, pos, length):
    """counts_dev between guard records; the records"""
    import torch
    dev = torch.device("cuda", 0)
    buf = torch.full(((length + 2 * GUARD) * 8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    pl.counts_dev(seq, pos, length, buf.data_ptr() + 32 * GUARD, st.cuda_stream)
    st.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[:8 * GUARD] == 0x5A5A5A5A).all() and (raw[8 * (GUARD + length):] == 0x5A5A5A5A).all()
    return raw[8 * GUARD:8 * (GUARD + length)].view(capi.PILEUP_BASE_DTYPE).copy()


def check_pile(pl, brute, label=None):
    """every base of every sequence, both read-outs, and the scalars"""
    for seq in range(brute.n_seqs):
        n = len(brute.refs[seq])
        want = np.array(brute.counts(seq), dtype=np.uint32).reshape(-1, 8)
        got = pl.counts(seq)
        rows = as_rows(got)
        if not (rows == want).all():
            bad = int(np.argmax((rows != want).any(axis=1)))
            raise AssertionError((label, seq, bad, rows[bad].tolist(), want[bad].tolist()))
        assert len(got) == n and counts_dev(pl, seq, 0, n).tobytes() == got.tobytes(), (label, seq)
    info = pl.info()
    assert {k: info[k] for k in brute.info()} == brute.info(), (label, info, brute.info())
    return info


def call_tuples(calls):
    assert calls.dtype == capi.PILEUP_CALL_DTYPE
    return [tuple(int(c[f]) for f in ("pos", "seq", "allele", "ref", "depth", "count", "ref_count")) for c in calls]


def snapshot(pl, n_seqs):
    return b"".join(pl.counts(s).tobytes() for s in range(n_seqs)), {k: v for k, v in pl.info().items() if k != "device_bytes"}


@pytest.fixture(scope="module")
def world(gpu):
    w = World()
    yield w
    w.obj.close()


class ShortWorld:
    """six references of 1, 63, 64, 65, 128 and 70 bases, one N and one lower-case base among them"""

    def __init__(self):
        rng = random.Random(3030)
        self.refs = [rand_seq(rng, n) for n in SHORT]
        s = bytearray(self.refs[3])
        s[20], s[64] = ord("N"), ord("c")
        self.refs[3] = bytes(s)
        self.rng = random.Random(3031)
        self.obj = capi.RefSeqs.create()
        self.obj.add(self.refs, 0)


@pytest.fixture(scope="module")
def short(gpu):
    w = ShortWorld()
    yield w
    w.obj.close()


@pytest.fixture(scope="module")
def sample(world):
    return make_sample(world)


_ALNS = {}


def sample_alns(world, sample, band):
    """the sample's alignments from the brute force, once per band"""
    if band not in _ALNS:
        _ALNS[band] = ab.alignments(world.refs, sample[0], sample[1], band)
    return _ALNS[band]


# ---- 1. base for base ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", (0, 8, 64))
def test_the_align_sample(world, sample, band):
    reads, recs = sample
    brute = pb.Pile(world.refs)
    piled = brute.add(reads, recs, band, alns=sample_alns(world, sample, band))
    with world.obj.pileup() as pl:
        pl.add_reads(reads, map_records(recs), band)
        info = check_pile(pl, brute, band)
    assert len(reads) > 140 and 100 < sum(piled) < len(reads)          # (reads of more than 1024 bases are offered only)
    assert info["n_columns"] > 10000 and info["n_piled"] == sum(piled)
    if band == 8:
        assert info["n_clipped"] > 0 and sum(c[pb.N_INS] for c in brute.base.values()) > 3 and sum(c[pb.N_DEL] for c in brute.base.values()) > 3


@pytest.mark.parametrize("band", (0, 5))
def test_starts_beyond_either_end_of_the_short_sequences(short, band):
    w = short
    reads, recs = [], []
    for seq, ref in enumerate(w.refs):
        n = len(ref)
        for L in (1, 30, 64, 70):
            for strand in (0, 1):
                for start in (-L - band - 5, -L, -band - 1, -2, 0, (n - L) // 2, n - L, n - L + 2, n - 1, n, n + band + 5):
                    # what the reference holds there, random bases beyond its ends, a few errors
                    piece = bytes(ref[q] if 0 <= q < n else w.rng.choice(b"ACGT") for q in range(start, start + L))
                    rd = mutate(w.rng, piece, 0.03, b"ACGTN")
                    reads.append(vb.rc(rd) if strand else rd), recs.append((seq, strand, start))
        reads += [ref, ref[:max(n - 1, 1)], ref + b"A"]
        recs += [(seq, 0, 0), (seq, 0, 0), (seq, 0, 0)]
    brute = pb.Pile(w.refs)
    brute.add(reads, recs, band)
    with w.obj.pileup() as pl:
        pl.add_reads(reads, map_records(recs), band)
        info = check_pile(pl, brute, band)
    assert info["n_overhang"] > 20 and info["n_clipped"] > 20 and info["n_piled"] == len(reads)
    # reads that end at n of the sequences of 64 and 128 bases: their -1 lies on the neighbour's first slot
    assert brute.record(2, 63)[0] >= 2 and brute.record(4, 127)[0] >= 2 and brute.record(3, 0)[0] >= 1 and brute.record(5, 0)[0] >= 1


@pytest.mark.parametrize("strand", (0, 1))
def test_2049_copies_of_one_read_land_on_one_counter(world, strand):
    w = world
    ref = w.refs[0]
    piece = bytearray(ref[1000:1060] + ref[1061:1151])         # coordinate 1060 is deleted
    piece[30] = vb._COMP[piece[30]]                             # and 1030 substituted
    rd = vb.rc(bytes(piece)) if strand else bytes(piece)
    rec = (0, strand, 1000)
    v, a, runs = ab.alignment(w.refs, rd, rec, 8)
    assert v[2] == 2 and {op for _, op in runs} == {"=", "X", "D"}
    brute = pb.Pile(w.refs)
    for _ in range(2049):
        brute.add_alignment(rd, rec, pb.JUNK_VOTES, v, a, runs)
    with w.obj.pileup() as pl:
        pl.add_reads([rd] * 2049, map_records([rec] * 2049), 8)
        check_pile(pl, brute, strand)
        assert call_tuples(pl.calls(2049, 2049, 10 ** 6)) == brute.calls(2049, 2049, 10 ** 6) and len(brute.calls()) == 2
    assert brute.record(0, 1030)[0] == 2049 and max(brute.record(0, 1030)[1:5]) == 2049


def test_9000_reads(world, sample):
    """more groups of 64 than the align kernel has waves, over a megabyte of bases"""
    reads, recs = sample
    alns = sample_alns(world, sample, 8)
    short_ones = [i for i, rd in enumerate(reads) if 100 <= len(rd) <= 300]
    pick = [short_ones[i % len(short_ones)] for i in range(9000)]
    brute = pb.Pile(world.refs)
    brute.add([reads[i] for i in pick], [recs[i] for i in pick], 8, alns=[alns[i] for i in pick])
    with world.obj.pileup() as pl:
        pl.add_reads([reads[i] for i in pick], map_records([recs[i] for i in pick]), 8)
        info = check_pile(pl, brute)
    assert info["n_offered"] == info["n_piled"] == 9000


def test_pieces_in_shuffled_order_and_two_host_threads(world, sample):
    reads, recs = sample
    n = len(reads)
    with world.obj.pileup() as pl:
        pl.add_reads(reads, map_records(recs), 8)
        whole = snapshot(pl, 3)
        for pieces in (2, 7, 65):
            pl.reset()
            order = list(range(n))
            random.Random(pieces).shuffle(order)
            cuts = [n * i // pieces for i in range(pieces + 1)]
            for lo, hi in zip(cuts, cuts[1:]):
                pl.add_reads([reads[i] for i in order[lo:hi]], map_records([recs[i] for i in order[lo:hi]]), 8)
            assert snapshot(pl, 3) == whole, pieces
        pl.reset()
        errs = []

        def work(t):
            try:
                for lo in range(t, n, 16):
                    idx = range(lo, min(lo + 8, n))
                    pl.add_reads([reads[i] for i in idx], map_records([recs[i] for i in idx]), 8)
            except Exception as e:              # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=work, args=(t,)) for t in (0, 8)]
        [t.start() for t in th]
        [t.join() for t in th]
        assert not errs, errs
        assert snapshot(pl, 3) == whole


# ---- 2. the device entry points ---------------------------------------------------------------------------------------------
def on_device(reads, recs, votes=None):
    import torch
    dev = torch.device("cuda", 0)
    bases, off = capi.concat_reads(reads)
    tb = torch.from_numpy(bases).to(dev) if len(bases) else torch.zeros(1, dtype=torch.uint8, device=dev)
    to = torch.from_numpy(off).to(dev)
    tm = torch.from_numpy(records(recs, votes).view(np.int64).copy() if len(reads) else np.zeros(4, np.int64)).to(dev)
    return dev, len(bases), tb, to, tm


def add_dev_guarded(pl, reads, recs, band, **filt):
    """add_dev between guard words around its workspace; whether they are intact"""
    import torch
    dev, nb, tb, to, tm = on_device(reads, recs)
    need = capi.Pileup.workspace_bytes(nb, len(reads))
    ws = torch.full((need + 512,), 0x5A, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    pl.add_dev(tb.data_ptr(), nb, to.data_ptr(), len(reads), tm.data_ptr(), ws.data_ptr() + 256, need, band, stream=st.cuda_stream, **filt)
    st.synchronize()
    raw = ws.cpu().numpy()
    return bool((raw[:256] == 0x5A).all() and (raw[256 + need:] == 0x5A).all())


def add_aligned(obj, pl, reads, recs, band, **filt):
    """align_dev, then add_aligned_dev on its output, on one stream"""
    import torch
    dev, nb, tb, to, tm = on_device(reads, recs)
    n = len(reads)
    need = capi.RefSeqs.align_workspace_bytes(nb, n)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    ver = torch.zeros(2 * n + 2, dtype=torch.int64, device=dev)
    out = torch.zeros(2 * n + 2, dtype=torch.int64, device=dev)
    ooff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    ops = torch.zeros(2 * nb + 4, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    obj.align_dev(tb.data_ptr(), nb, to.data_ptr(), n, tm.data_ptr(), ver.data_ptr(), out.data_ptr(), ooff.data_ptr(), ops.data_ptr(), 2 * nb,
                  ws.data_ptr(), need, band, st.cuda_stream)
    pl.add_aligned_dev(tb.data_ptr(), nb, to.data_ptr(), n, tm.data_ptr(), ver.data_ptr(), out.data_ptr(), ooff.data_ptr(), ops.data_ptr(),
                       stream=st.cuda_stream, **filt)
    st.synchronize()


def test_the_three_entry_points_give_the_same_bytes(world, sample):
    reads, recs = sample
    for band in (0, 8):
        with world.obj.pileup() as a, world.obj.pileup() as b, world.obj.pileup() as c:
            a.add_reads(reads, map_records(recs), band)
            assert add_dev_guarded(b, reads, recs, band)
            add_aligned(world.obj, c, reads, recs, band)
            assert snapshot(a, 3) == snapshot(b, 3) == snapshot(c, 3)
            assert a.calls().tobytes() == b.calls().tobytes() == c.calls().tobytes()


def test_a_read_out_between_two_adds_and_reset(world, sample):
    reads, recs = sample
    alns = sample_alns(world, sample, 8)
    h = len(reads) // 2
    brute = pb.Pile(world.refs)
    with world.obj.pileup() as pl:
        pl.add_reads(reads[:h], map_records(recs[:h]), 8)
        brute.add(reads[:h], recs[:h], 8, alns=alns[:h])
        check_pile(pl, brute, "first half")
        first_calls = call_tuples(pl.calls())
        assert first_calls == brute.calls()
        pl.add_reads(reads[h:], map_records(recs[h:]), 8)      # the read-outs disturbed nothing: the same pileup goes on
        brute.add(reads[h:], recs[h:], 8, alns=alns[h:])
        check_pile(pl, brute, "both halves")
        assert call_tuples(pl.calls()) == brute.calls() != first_calls
        pl.reset()
        brute.reset()
        check_pile(pl, brute, "reset")
        assert len(pl.calls()) == 0 and pl.info()["n_offered"] == 0
        pl.add_reads(reads[:h], map_records(recs[:h]), 8)
        brute.add(reads[:h], recs[:h], 8, alns=alns[:h])
        check_pile(pl, brute, "after reset")


def test_every_filter_field(world, sample):
    reads, recs = sample
    alns = sample_alns(world, sample, 8)
    rng = random.Random(77)
    votes = [(rng.randrange(0, 12), rng.randrange(0, 12)) for _ in reads]
    votes[0], votes[1], votes[2] = (5, 5), (5, 4), (4, 5)
    with world.obj.pileup() as pl:
        for filt in ((0, 0, -1), (5, 0, -1), (6, 0, -1), (0, 1, -1), (0, 0, 0), (0, 0, 1), (0, 0, 2), (5, 1, 3), (12, 0, -1), (-1, 0, -5)):
            pl.reset()
            brute = pb.Pile(world.refs)
            piled = brute.add(reads, recs, 8, votes=votes, filt=filt, alns=alns)
            pl.add_reads(reads, records(recs, votes), 8, min_votes=filt[0], unique=bool(filt[1]), max_edit=filt[2])
            info = check_pile(pl, brute, filt)
            assert info["n_offered"] == len(reads) and info["n_piled"] == sum(piled)
        assert sum(piled) > 100
    # through the device entry points too
    with world.obj.pileup() as a, world.obj.pileup() as b:
        brute = pb.Pile(world.refs)
        brute.add(reads, recs, 8, votes=votes, filt=(5, 1, 3), alns=alns)
        a.add_reads(reads, records(recs, votes), 8, min_votes=5, unique=True, max_edit=3)
        import torch
        dev, nb, tb, to, tm = on_device(reads, recs, votes)
        need = capi.Pileup.workspace_bytes(nb, len(reads))
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        b.add_dev(tb.data_ptr(), nb, to.data_ptr(), len(reads), tm.data_ptr(), ws.data_ptr(), need, 8, min_votes=5, unique=True, max_edit=3)
        torch.cuda.synchronize(dev)
        check_pile(b, brute)
        assert snapshot(a, 3) == snapshot(b, 3)


def test_calls_at_three_threshold_sets(world):
    """eight reads over one place, three of them with a substitution, two others with a deletion, one with an insertion"""
    w = world
    ref = w.refs[0]
    base = ref[700:820]
    sub = bytearray(base)
    sub[40] = vb._COMP[sub[40]]
    dele = base[:70] + base[71:]
    ins = base[:90] + (b"A" if ref[790] != 65 else b"C") + base[90:]
    reads = [bytes(sub)] * 3 + [dele] * 2 + [ins] + [base] * 2
    recs = [(0, 0, 700)] * len(reads)
    brute = pb.Pile(w.refs)
    brute.add(reads, recs, 8)
    assert brute.record(0, 740)[0] == 8 and max(brute.record(0, 740)[1:5]) == 5
    with w.obj.pileup() as pl:
        pl.add_reads(reads, map_records(recs), 8)
        check_pile(pl, brute)
        for th in ((1, 1, 0), (8, 3, 375000), (8, 3, 375001), (8, 2, 250000), (9, 1, 0), (1, 1, 10 ** 6)):
            want = brute.calls(*th)
            assert call_tuples(pl.calls(*th)) == want, th
        assert len(brute.calls(1, 1, 0)) == 3 and [c[2] for c in brute.calls(8, 3, 375000)] == [brute.calls()[0][2]]
        assert brute.calls(8, 3, 375001) == [] and len(brute.calls(8, 2, 250000)) == 2
        assert {c[2] for c in brute.calls()} >= {pb.DEL, pb.INS}


def test_empty_and_unverified_batches(world):
    w = world
    with w.obj.pileup() as pl:
        zero = snapshot(pl, 3)
        pl.add_reads([], map_records([]), 8)
        assert add_dev_guarded(pl, [], [], 8)
        assert snapshot(pl, 3) == zero and pl.info()["n_offered"] == 0
        rd, _, _ = w.read(0, 100)
        reads = [rd, rd, rd, b"", rand_seq(w.rng, 1100)]
        recs = [(-1, 0, 5), (3, 0, 5), (0, 2, 5), (0, 0, 5), (0, 0, 5)]
        pl.add_reads(reads, map_records(recs), 8)
        info = pl.info()
        assert (info["n_offered"], info["n_piled"], info["n_columns"], info["n_clipped"], info["n_overhang"]) == (5, 0, 0, 0, 0)
        assert snapshot(pl, 3)[0] == zero[0] and len(pl.calls()) == 0
    # a pileup covers the sequences its object held when it was made
    with capi.RefSeqs.create() as o:
        o.add(w.refs[:2], 0)
        with o.pileup() as pl:
            o.add(w.refs[2:], 2)
            rd2, rec2, _ = w.read(2, 40)
            rd0, rec0, _ = w.read(0, 100)
            pl.add_reads([rd2, rd0], map_records([rec2, rec0]), 8)
            brute = pb.Pile(w.refs, 2)
            brute.add([rd2, rd0], [rec2, rec0], 8)
            info = check_pile(pl, brute)
            assert (info["n_seqs"], info["n_offered"], info["n_piled"]) == (2, 2, 1)
            refused(lambda: pl.counts(2, 0, 1), "sequence 2 of 2")


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------
def test_the_overflow_rule_and_every_other_refusal(world, sample):
    import torch
    w = world
    reads, recs = sample[0][:3], sample[1][:3]
    L = capi.lib()
    with w.obj.pileup() as pl:
        pl.add_reads(reads, map_records(recs), 8)
        before = snapshot(pl, 3)
        dev, nb, tb, to, tm = on_device(reads, recs)
        need = capi.Pileup.workspace_bytes(nb, 3)
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        f = capi.pileup_filter()
        four = [tb.data_ptr(), nb, to.data_ptr()]
        # 3 reads are in: 2^31 - 4 more would reach 2^31 - 1, one more than that is refused before anything runs
        big = (1 << 31) - 3
        rc = L.sbwtgpu_pileup_add_aligned_dev(pl.handle, *four, big, tm.data_ptr(), tm.data_ptr(), tm.data_ptr(), to.data_ptr(), tm.data_ptr(),
                                              f.ctypes.data, None)
        assert rc == capi.ERR_INVALID_ARG and b"2^31 - 1" in L.sbwtgpu_last_error() and b"offered" in L.sbwtgpu_last_error()
        rc = L.sbwtgpu_pileup_add_dev(pl.handle, *four, big, tm.data_ptr(), 8, f.ctypes.data, ws.data_ptr(), 1 << 60, None)
        assert rc == capi.ERR_INVALID_ARG and b"2^31 - 1" in L.sbwtgpu_last_error()
        assert pl.info()["n_offered"] == 3
        for n_reads, needle in ((-1, b"n_reads"), (1 << 31, b"2^31")):
            rc = L.sbwtgpu_pileup_add_dev(pl.handle, *four, n_reads, tm.data_ptr(), 8, f.ctypes.data, ws.data_ptr(), 1 << 60, None)
            assert rc == capi.ERR_INVALID_ARG and needle in L.sbwtgpu_last_error()
            rc = L.sbwtgpu_pileup_add_batch(pl.handle, tb.data_ptr(), to.data_ptr(), n_reads, tm.data_ptr(), 8, f.ctypes.data)
            assert rc == capi.ERR_INVALID_ARG and needle in L.sbwtgpu_last_error()
        bases, off = capi.concat_reads(reads)
        m = map_records(recs)
        for band in (-1, 257):
            refused(lambda: pl.add(bases, off, m, band), "band must be in 0 .. 256")
            refused(lambda: pl.add_dev(*four, 3, tm.data_ptr(), ws.data_ptr(), need, band), "band")
        bad = capi.pileup_filter(reserved=1)
        assert L.sbwtgpu_pileup_add_batch(pl.handle, bases.ctypes.data, off.ctypes.data, 3, m.ctypes.data, 8, bad.ctypes.data) == capi.ERR_INVALID_ARG
        assert b"reserved" in L.sbwtgpu_last_error()
        assert L.sbwtgpu_pileup_add_dev(pl.handle, *four, 3, tm.data_ptr(), 8, bad.ctypes.data, ws.data_ptr(), need, None) == capi.ERR_INVALID_ARG
        assert b"reserved" in L.sbwtgpu_last_error()
        for args in ((None, off.ctypes.data, 3, m.ctypes.data, 8, f.ctypes.data), (bases.ctypes.data, None, 3, m.ctypes.data, 8, f.ctypes.data),
                     (bases.ctypes.data, off.ctypes.data, 3, None, 8, f.ctypes.data), (bases.ctypes.data, off.ctypes.data, 3, m.ctypes.data, 8, None)):
            assert L.sbwtgpu_pileup_add_batch(pl.handle, *args) == capi.ERR_INVALID_ARG and b"NULL" in L.sbwtgpu_last_error()
        refused(lambda: pl.add_dev(*four, 3, tm.data_ptr(), ws.data_ptr(), need - 1), "workspace")
        refused(lambda: pl.add_dev(*four, 3, tm.data_ptr(), 0, need), "workspace")
        refused(lambda: pl.add_dev(*four, 3, tm.data_ptr(), ws.data_ptr() + 8, need), "aligned")
        refused(lambda: pl.add_dev(*four, 3, 0, ws.data_ptr(), need), "NULL")
        refused(lambda: pl.add_dev(tb.data_ptr(), nb, 0, 3, tm.data_ptr(), ws.data_ptr(), need), "NULL")
        for k in range(4):                      # d_map, d_verify, d_align, d_op_off
            ptrs = [tm.data_ptr()] * 4
            ptrs[k] = 0
            refused(lambda: pl.add_aligned_dev(*four, 3, *ptrs, tm.data_ptr()), "NULL")
        for seq, pos, n in ((3, 0, 1), (-1, 0, 1), (0, -1, 1), (0, 0, -1), (0, 0, 3001), (0, 3000, 1), (2, 69, 2), (0, 1 << 40, 1)):
            refused(lambda: pl.counts(seq, pos, n), "pileup")
            refused(lambda: pl.counts_dev(seq, pos, n, tm.data_ptr()), "pileup")
        refused(lambda: pl.counts(2, 69, 2), "outside sequence 2 of 70 bases")
        refused(lambda: pl.counts_dev(0, 0, 1, 0), "NULL")
        assert L.sbwtgpu_pileup_counts_copy(pl.handle, 0, 0, 1, None) == capi.ERR_INVALID_ARG and b"NULL" in L.sbwtgpu_last_error()
        for th, needle in (((0, 1, 0), "min_depth"), ((1, 0, 0), "min_alt"), ((1, 1, -1), "min_frac_ppm"), ((1, 1, 10 ** 6 + 1), "min_frac_ppm"),
                           ((-5, 1, 0), "min_depth")):
            refused(lambda: pl.calls(*th), needle)
        p, n = capi.C.c_void_p(), capi.C.c_int64()
        assert L.sbwtgpu_pileup_calls(pl.handle, 1, 1, 0, None, capi.C.byref(n)) == capi.ERR_INVALID_ARG and b"NULL" in L.sbwtgpu_last_error()
        assert L.sbwtgpu_pileup_calls(pl.handle, 1, 1, 0, capi.C.byref(p), None) == capi.ERR_INVALID_ARG
        torch.cuda.synchronize(dev)
        # nothing changed, and everything still works
        assert snapshot(pl, 3) == before
        brute = pb.Pile(w.refs)
        brute.add(reads, recs, 8)
        check_pile(pl, brute)
        pl.add_reads(reads, map_records(recs), 8)
        brute.add(reads, recs, 8)
        check_pile(pl, brute)
        assert len(pl.counts(0, 3000, 0)) == 0 and len(pl.counts(2, 70, 0)) == 0


# ---- 4. behind the map calls ------------------------------------------------------------------------------------------------
K = 15


def test_map_then_pile_calls_a_planted_snp(world):
    """Occurrences.map on a small index over the three references, then add on its records: a SNP carried by 20 of 20 reads is
    called, and nothing else is"""
    w = world
    rng = random.Random(15)
    bits = hostlib.build_bits(w.refs, K, False, True)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, K, bits.n_kmers, 0)
    try:
        with idx.occurrences_builder() as b:
            b.add(w.refs, 0, 1)
            occ = b.finish()
        sample_seq = bytearray(w.refs[0])
        snp = 1234
        sample_seq[snp] = vb._COMP[sample_seq[snp]]
        reads = []
        for i in range(20):
            at = snp - 140 + 7 * i
            rd = bytes(sample_seq[at:at + 150])
            reads.append(vb.rc(rd) if i % 2 else rd)
        reads += [w.refs[0][2000:2150], w.refs[0][100:250], rand_seq(rng, 150)]
        bases, off = capi.concat_reads(reads)
        placed = occ.map(bases, off, 2)
        recs = [(int(p["seq"]), int(p["strand"]), int(p["start"])) for p in placed]
        votes = [(int(p["votes"]), int(p["votes2"])) for p in placed]
        brute = pb.Pile(w.refs)
        brute.add(reads, recs, 8, votes=votes, filt=(3, 1, 5))
        with w.obj.pileup() as pl:
            pl.add(bases, off, placed, 8, min_votes=3, unique=True, max_edit=5)
            info = check_pile(pl, brute)
            calls = call_tuples(pl.calls(10, 10, 900000))
            code = pb.CODE[sample_seq[snp]]
            assert calls == [(snp, 0, code, pb.CODE[w.refs[0][snp]], 20, 20, 0)] == brute.calls(10, 10, 900000)
            assert call_tuples(pl.calls()) == calls and info["n_piled"] >= 20
        occ.close()
    finally:
        idx.close()


def test_cli_pileup_files(gpu, tmp_path):
    """read-hits --pileup-out --calls-out: the two files against the brute force's text on the placements the hits file names,
    and the hits file byte-equal to a run without the new options"""
    import test_gpu_pseudoalign_wide as tw
    d = str(tmp_path)
    k = 11
    rng = random.Random(3070)
    files = [[rand_seq(rng, 330), rand_seq(rng, 64)], [rand_seq(rng, 200)[:100] + b"N" + rand_seq(rng, 99)], [rand_seq(rng, 129), rand_seq(rng, 31)]]
    seqs = [s for f in files for s in f]
    with open(d + "/all.fna", "w") as fh, open(d + "/refs.txt", "w") as lst:
        for i, s in enumerate(seqs):
            fh.write(">s%d\n%s\n" % (i, s.decode()))
        for c, f in enumerate(files):
            with open("%s/ref%d.fna" % (d, c), "w") as one:
                for s in f:
                    one.write(">r\n%s\n" % s.decode())
            lst.write("%s/ref%d.fna\n" % (d, c))
    batch = []
    for i in range(90):
        src = seqs[i % 5]
        n = rng.randint(12, min(90, len(src)))
        a = rng.randrange(0, len(src) - n + 1)
        r = bytearray(mutate(rng, src[a:a + n], 0.03, b"ACGTN" if i % 6 == 0 else b"ACGT"))
        if i % 4 == 1 and len(r) > 30:
            del r[15:17]
        if i % 4 == 3 and len(r) > 30:
            r[20:20] = b"G"
        batch.append(vb.rc(bytes(r)) if i % 3 == 2 else bytes(r))
    twin = bytearray(seqs[0][100:220])                      # two reads with the same substitution: a call that two observations make
    twin[60] = vb._COMP[twin[60]]
    batch += [b"ACG", rand_seq(rng, 60), b"T" * 40, seqs[0][:40], seqs[4][-20:], bytes(twin), vb.rc(bytes(twin)), seqs[1]]
    with open(d + "/reads.fastq", "w") as fh:
        fh.write("".join("@r%d\n%s\n+\n%s\n" % (i, r.decode(), "I" * len(r)) for i, r in enumerate(batch)))
    SBWT, index = tw.SBWT, d + "/x.sbwt"
    p = tw.run([SBWT, "build", "-i", d + "/all.fna", "-o", index, "-k", str(k), "--temp-dir", d, "--add-reverse-complements"])
    assert p.returncode == 0, p.stderr.decode()
    p = tw.run([SBWT, "build-colors", "--both-strands", "-i", index, "-r", d + "/refs.txt", "-o", d + "/x.colors", "--occurrences-out", d + "/x.occ",
                "--positions-out", d + "/x.pos"])
    assert p.returncode == 0, p.stderr.decode()
    base = [SBWT, "read-hits", "-i", index, "-q", d + "/reads.fastq", "--both-strands", "--batch-bases", "700"]
    for option, file in (("--positions", d + "/x.pos"), ("--occurrences", d + "/x.occ")):
        for extra, filt, th, flags in (([], pb.NO_FILTER, (1, 1, 0), []), (["--cigar", "--band", "3"], (2, 1, 4), (2, 2, 250000),
                                       ["--min-votes", "2", "--unique", "--max-edit", "4", "--min-depth", "2", "--min-alt", "2", "--min-frac", "0.25"])):
            placed = base + [option, file, "--refs", d + "/refs.txt"] + extra
            p = tw.run(placed + ["-o", d + "/before.hits"])
            assert p.returncode == 0, p.stderr.decode()
            p = tw.run(placed + ["-o", d + "/with.hits", "--pileup-out", d + "/pile.tsv", "--calls-out", d + "/calls.tsv"] + flags)
            assert p.returncode == 0, p.stderr.decode()
            hits = open(d + "/with.hits", "rb").read()
            assert hits == open(d + "/before.hits", "rb").read()
            cols = [ln.split() for ln in hits.splitlines()]
            recs = [(int(f[4]), int(f[5]), int(f[6])) for f in cols]
            votes = [(int(f[7]), int(f[8])) for f in cols]
            brute = pb.Pile(seqs)
            brute.add(batch, recs, 3 if extra else 8, votes=votes, filt=filt)
            assert brute.n_piled > (10 if flags else 40) and len(brute.calls()) > 0
            assert open(d + "/pile.tsv").read() == brute.pile_tsv(), (option, extra)
            assert open(d + "/calls.tsv").read() == brute.calls_tsv(*th), (option, extra)
            assert flags or "\tN\t" in brute.pile_tsv()
            # either file alone
            p = tw.run(placed + ["-o", d + "/one.hits", "--calls-out", d + "/only.tsv"] + flags)
            assert p.returncode == 0 and open(d + "/only.tsv").read() == brute.calls_tsv(*th) and open(d + "/one.hits", "rb").read() == hits
    for bad, needle in ((["--min-frac", "1.5"], b"--min-frac must be"), (["--min-depth", "0"], b"--min-depth must be"), (["--min-alt", "0"], b"--min-alt must be")):
        p = tw.run(placed + ["-o", d + "/bad.hits", "--calls-out", d + "/bad.tsv"] + bad)
        assert p.returncode != 0 and needle in p.stderr, p.stderr


# ---- 5. fuzz ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_fuzz(gpu, seed):
    rng = random.Random(3000 + seed)
    refs = []
    for _ in range(rng.randrange(1, 6)):
        n = rng.choice((1, 2, 63, 64, 65, 127, 128, 129, 192, rng.randrange(1, 400), rng.randrange(400, 1500)))
        s = bytearray(rand_seq(rng, n))
        for _ in range(rng.randrange(0, 4)):
            s[rng.randrange(n)] = rng.choice(b"Nacgt")
        refs.append(bytes(s))
    brute = pb.Pile(refs)
    with capi.RefSeqs.create() as obj:
        obj.add(refs, 0)
        with obj.pileup() as pl:
            for _ in range(rng.randrange(1, 4)):
                reads, recs, votes = [], [], []
                for _ in range(rng.randrange(1, 120)):
                    seq = rng.randrange(len(refs))
                    ref, L = refs[seq], rng.choice((1, 20, 64, 100, 150, 257))
                    at = rng.randrange(-10, len(ref) + 5)
                    piece = bytearray(mutate(rng, ref[max(at, 0):max(at, 0) + L].ljust(L, b"A")[:L], rng.choice((0.0, 0.02, 0.2)), b"ACGTN"))
                    for _ in range(rng.randrange(0, 3)):
                        q = rng.randrange(len(piece))
                        if rng.random() < 0.5 and len(piece) > 1:
                            del piece[q]
                        else:
                            piece.insert(q, rng.choice(b"ACGT"))
                    strand = rng.randrange(2)
                    reads.append(vb.rc(bytes(piece)) if strand else bytes(piece))
                    recs.append((seq if rng.random() < 0.95 else rng.choice((-1, len(refs))), strand, at + rng.randrange(-3, 4)))
                    votes.append((rng.randrange(0, 6), rng.randrange(0, 6)))
                band = rng.choice((0, 3, 8, 20))
                filt = (rng.randrange(0, 4), rng.randrange(2), rng.choice((-1, 0, 2, 10)))
                brute.add(reads, recs, band, votes=votes, filt=filt)
                pl.add_reads(reads, records(recs, votes), band, min_votes=filt[0], unique=bool(filt[1]), max_edit=filt[2])
                check_pile(pl, brute, seed)
            for th in ((1, 1, 0), (rng.randrange(1, 4), rng.randrange(1, 3), rng.randrange(0, 10 ** 6 + 1)), (2, 1, 500000)):
                assert call_tuples(pl.calls(*th)) == brute.calls(*th), (seed, th)
