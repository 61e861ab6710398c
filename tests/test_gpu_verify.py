"""GPU: sbwtgpu_refseqs_* (sbwt_verify.hip: the reference sequences packed on the device, and mapped reads verified against them)
against the definition in tests/verify_brute.py.  Every comparison is exact: the bases the object gives back byte for byte, and
the records field for field."""
import random
import threading

import numpy as np
import pytest

import verify_brute as vb
from sbwt_amd import capi, hostlib

pytestmark = pytest.mark.gpu

GUARD = 64
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 1023, 1024, 1025)
BANDS = (0, 1, 2, 5, 8, 31, 64, 256)
JUNK = 0x5A5A5A5A


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, p, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) if rng.random() < p else c for c in s)


def map_records(recs):
    """READ_MAP_DTYPE records with (seq, strand, start) set and every other field junk: the verify calls read only those three"""
    a = np.zeros(len(recs), dtype=capi.READ_MAP_DTYPE)
    for f in ("votes", "votes2", "n_found", "n_anchored"):
        a[f] = JUNK
    for i, (seq, strand, start) in enumerate(recs):
        a[i]["seq"], a[i]["strand"], a[i]["start"] = seq, strand, start
    return a


def as_tuples(out):
    assert out.dtype == capi.READ_VERIFY_DTYPE
    return [(int(r["ref_end"]), int(r["mismatches"]), int(r["edit"])) for r in out]


def check(obj, refs, reads, recs, band, label=None):
    """the object's records for the batch against the brute force, record for record"""
    got = as_tuples(obj.verify_reads(reads, map_records(recs), band))
    want = vb.records(refs, reads, recs, band)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (label, i, len(reads[i]), recs[i], band, g, w)
    assert len(got) == len(want) == len(reads)
    return got


class World:
    """Three references: 3 000 bases, 2 999 bases with runs of N and a lower-case patch, and 70 bases."""

    def __init__(self):
        rng = random.Random(2828)
        a = rand_seq(rng, 3000)
        b = bytearray(rand_seq(rng, 2999))
        b[500:520] = b"N" * 20
        b[1500:1503] = b"NNN"
        b[2100:2104] = b"acgt"
        b[2990:2999] = b"N" * 9
        b[0:1] = b"N"
        self.refs = [a, bytes(b), rand_seq(rng, 70)]
        self.rng = random.Random(2829)
        self.obj = capi.RefSeqs.create()
        self.obj.add(self.refs, 0)

    def read(self, seq, L, p=0.0, indel=0, strand=0, shift=0, at=None):
        """(read, record, substitutions): L bases drawn from sequence seq at a random origin, with substitutions at rate p and one
        indel of |indel| bases (> 0: inserted into the read, < 0: deleted from it), reverse-complemented for strand 1; the record
        names the origin moved by shift"""
        rng, ref = self.rng, self.refs[seq]
        d = abs(indel)
        span = L - d if indel > 0 else L + d                 # the reference bases the read covers
        if at is None:
            at = rng.randrange(0, max(len(ref) - span, 0) + 1)
        piece = ref[at:at + span]
        if indel > 0 and L > d:
            q = rng.randrange(0, len(piece) + 1)
            piece = piece[:q] + rand_seq(rng, d) + piece[q:]
        elif indel < 0 and len(piece) > d:
            q = rng.randrange(0, len(piece) - d + 1)
            piece = piece[:q] + piece[q + d:]
        piece = piece[:L].ljust(L, b"A") if len(piece) != L else piece
        read = mutate(rng, piece, p)
        subs = sum(1 for x, y in zip(read, piece) if x != y)
        return (vb.rc(read) if strand else read), (seq, strand, at + shift), subs


@pytest.fixture(scope="module")
def world(gpu):
    w = World()
    yield w
    w.obj.close()


# ---- 1. the object --------------------------------------------------------------------------------------------------------
def test_get_gives_back_what_was_added(world):
    obj, refs = world.obj, world.refs
    info = obj.info()
    assert (info["n_seqs"], info["total_bases"], info["n_invalid"]) == (3, sum(map(len, refs)), vb.n_invalid(refs)) and info["n_invalid"] == 37
    assert info["device_bytes"] >= 24 * sum((len(r) + 63) // 64 for r in refs)
    assert obj.lengths().tolist() == [len(r) for r in refs]
    for s, ref in enumerate(refs):
        want = vb.stored(ref)
        assert obj.get(s) == want                                           # the whole sequence
        assert obj.get(s, len(ref) - 1, 1) == want[-1:]                      # its last base
        assert obj.get(s, len(ref), 0) == b"" and obj.get(s, 0, 0) == b""
        for pos, n in ((0, 1), (31, 2), (30, 5), (63, 2), (60, 10), (1, 64), (33, 70), (64, 1), (0, 65), (len(ref) - 40, 40)):
            if pos + n <= len(ref):                                           # slices across the 32- and 64-base word edges
                assert obj.get(s, pos, n) == want[pos:pos + n], (s, pos, n)
    rng = random.Random(1)
    small = [rand_seq(rng, n, b"ACGTNa") for n in (1, 63, 64, 65, 0, 1, 128, 129)]
    with capi.RefSeqs.create() as o:
        o.add(small)
        assert o.info()["n_invalid"] == vb.n_invalid(small) and o.lengths().tolist() == [len(s) for s in small]
        for s, ref in enumerate(small):
            assert o.get(s) == vb.stored(ref), s
            if ref:
                assert o.get(s, len(ref) - 1, 1) == vb.stored(ref)[-1:]


def test_one_by_one_and_as_one_batch(world):
    refs = world.refs + [b"", b"ACGTN", b"T" * 64]
    with capi.RefSeqs.create() as one, capi.RefSeqs.create() as batch:
        for i, r in enumerate(refs):
            one.add([r], i)
        batch.add(refs, 0)
        a, b = one.info(), batch.info()
        assert {k: a[k] for k in ("n_seqs", "total_bases", "n_invalid")} == {k: b[k] for k in ("n_seqs", "total_bases", "n_invalid")}
        assert a["n_seqs"] == len(refs) and a["n_invalid"] == vb.n_invalid(refs)
        for s, r in enumerate(refs):
            assert one.get(s) == batch.get(s) == vb.stored(r), s
        assert one.lengths().tolist() == batch.lengths().tolist() == [len(r) for r in refs]


def test_the_arrays_grow_by_doubling():
    rng = random.Random(3)
    seqs, sizes = [], []
    with capi.RefSeqs.create() as o:
        assert o.info()["n_seqs"] == 0 and o.lengths().tolist() == []
        for n_new in (300, 1500, 3000, 6000):
            new = [rand_seq(rng, rng.randint(0, 70), b"ACGTN") for _ in range(n_new)]
            o.add(new, len(seqs))
            seqs += new
            sizes.append(o.info()["device_bytes"])
            info = o.info()
            assert (info["n_seqs"], info["total_bases"], info["n_invalid"]) == (len(seqs), sum(map(len, seqs)), vb.n_invalid(seqs))
            for s in [0, 299, min(300, len(seqs) - 1), len(seqs) - 1] + [rng.randrange(len(seqs)) for _ in range(40)]:     # what was there has moved intact
                assert o.get(s) == vb.stored(seqs[s]), (n_new, s)
        assert o.lengths().tolist() == [len(s) for s in seqs]
        # 10 800 sequences of up to two units: the packed arrays and the table have each doubled at least twice since the first add
        assert sizes[0] < sizes[1] < sizes[2] < sizes[3] and sizes[3] >= 4 * sizes[0]
        # and a read still verifies on the last sequence
        last = len(seqs) - 1
        check(o, seqs, [seqs[last][:20], seqs[5]], [(last, 0, 0), (5, 0, 0)], 2)


# ---- 2. record for record ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sample(world):
    """Every length class on the two long references, clean and with 1 % and 5 % substitutions, both strands; indels of 1, 2 and 5
    bases either way; placements shifted by -3 .. 3.  One batch: the instantiation switch and the fast / slow boundary sit in
    it, lengths mixed within every wave."""
    w = world
    reads, recs = [], []
    n = 0
    for L in LENGTHS:
        for p in (0.0, 0.01, 0.05):
            for strand in (0, 1):
                rd, rec, _ = w.read(n % 2, L, p, 0, strand, shift=(n % 7) - 3 if n % 3 == 0 else 0)
                reads.append(rd), recs.append(rec)
                n += 1
    for L in (64, 65, 150, 257, 1000):
        for indel in (1, 2, 5, -1, -2, -5):
            rd, rec, _ = w.read(n % 2, L, 0.01, indel, n % 2, shift=(n % 7) - 3)
            reads.append(rd), recs.append(rec)
            n += 1
    for L in (1, 5, 40, 70, 71):                              # the short reference: reads as long as it, and longer
        rd, rec, _ = w.read(2, L, 0.02, 0, L % 2, at=0 if L >= 70 else None)
        reads.append(rd), recs.append(rec)
    order = list(range(len(reads)))
    random.Random(5).shuffle(order)
    return [reads[i] for i in order], [recs[i] for i in order]


@pytest.mark.parametrize("band", BANDS)
def test_records_of_every_length_class(world, sample, band):
    reads, recs = sample
    got = check(world.obj, world.refs, reads, recs, band)
    assert len(reads) > 130 and {len(r) for r in reads} >= set(LENGTHS)
    assert sum(1 for g in got if g[2] == 0) > 10 and sum(1 for g in got if 0 < g[2] < g[1]) > 5 and sum(1 for g in got if g[2] == -1) >= 6


def test_edit_drops_once_the_band_reaches_the_indel(world):
    """clean reads with one deletion of d bases, placed at their origin: the alignment needs d reference bases past the window of
    band 0, so edit falls to d exactly when the band reaches d, never rises, and stays below the mismatches"""
    w = world
    for d in (1, 2, 5):
        reads, recs = [], []
        for i in range(20):
            rd, rec, _ = w.read(0, 100 + i, 0.0, -d, i % 2)
            reads.append(rd), recs.append(rec)
        by_band = [check(w.obj, w.refs, reads, recs, band) for band in (0, d, 8)]
        for r0, rd_, r8 in zip(*by_band):
            assert r0[2] >= rd_[2] >= r8[2] and rd_[2] <= d and r0[1] == rd_[1] == r8[1] and rd_[2] <= r0[1]


@pytest.mark.parametrize("band", (0, 5, 64))
def test_placements_at_and_beyond_the_ends(world, band):
    w = world
    reads, recs = [], []
    for seq in (0, 1, 2):
        n = len(w.refs[seq])
        for L in (1, 30, 64, 70, 150, 257):
            for strand in (0, 1):
                rd, _, _ = w.read(seq, L, 0.01, 0, strand) if L <= n else (rand_seq(w.rng, L), None, 0)
                for start in (-L - band - 5, -L - band, -L, -1, 0, n - L, n - L + 1, n, n + band, n + band + 5):
                    reads.append(rd), recs.append((seq, strand, start))
        # the read that is its sequence's first and last bases, in place
        for L in (1, 33, min(n, 65)):
            reads += [w.refs[seq][:L], w.refs[seq][n - L:]]
            recs += [(seq, 0, 0), (seq, 0, n - L)]
    got = check(w.obj, w.refs, reads, recs, band)
    assert sum(1 for g, rd in zip(got, reads) if g[1] == len(rd)) > 50 and sum(1 for g in got if g[2] == 0) >= 6


def test_the_neighbours_in_the_packed_arrays_do_not_matter(world):
    """placements on sequence 1 that reach into the words of sequences 0 and 2: the same records from an object that holds the
    same sequence between two others"""
    w, rng = world, random.Random(7)
    mid = w.refs[1]
    n = len(mid)
    others = [rand_seq(rng, 100), mid, rand_seq(rng, 1000)]
    reads, recs = [], []
    for L in (20, 64, 150, 300):
        for start in (-L, -70, -33, -5, -1, 0, 3, n - L - 3, n - L, n - L + 1, n - 30, n - 1, n, n + 40):
            at = min(max(start, 0), n - L)
            rd = mutate(rng, mid[at:at + L], 0.02)
            strand = (start + L) % 2
            reads.append(vb.rc(rd) if strand else rd), recs.append((1, strand, start))
    with capi.RefSeqs.create() as o:
        o.add(others)
        for band in (0, 8, 64):
            a = check(w.obj, w.refs, reads, recs, band)
            b = check(o, others, reads, recs, band)
            assert a == b


def test_unverified_records_among_ordinary_reads(world):
    w = world
    reads, recs = [], []
    bad = [(-1, 0, 5), (3, 0, 5), (1 << 20, 0, 5), (-(1 << 31), 0, 5), (0, 2, 5), (0, -1, 5), (0, 1 << 30, 5), (0, 0, 1 << 40), (0, 0, -(1 << 40)),
           (1, 1, (1 << 62)), (2, 0, -(1 << 63))]
    for i in range(130):
        rd, rec, _ = w.read(i % 3, 1 + (i * 7) % 70, 0.02, 0, i % 2)
        if i % 3 == 1:
            rec = bad[(i // 3) % len(bad)]
        reads.append(rd if i % 11 else b""), recs.append(rec)
    # the largest and smallest starts that are verified
    reads += [b"ACGT", b"ACGT"]
    recs += [(0, 0, (1 << 40) - 1), (1, 1, -(1 << 40) + 1)]
    got = check(w.obj, w.refs, reads, recs, 8)
    assert sum(1 for g in got if g == vb.UNVERIFIED) >= 40 and got[-2] == ((1 << 40) - 9, 4, 4) and got[-1] == (-(1 << 40) - 7, 4, 4)


def test_small_batches(world):
    w = world
    assert len(w.obj.verify_reads([], map_records([]), 8)) == 0
    assert len(w.obj.verify(np.zeros(0, np.uint8), np.zeros(1, np.int64), map_records([]), 0)) == 0
    rd, rec, _ = w.read(0, 150, 0.01, 0, 1)
    check(w.obj, w.refs, [rd], [rec], 8)
    check(w.obj, w.refs, [b""], [(0, 0, 7)], 8)
    # 65 reads: the second wave has one lane
    reads, recs = [], []
    for i in range(65):
        rd, rec, _ = w.read(i % 2, 100 + i, 0.02, (i % 3) - 1, i % 2)
        reads.append(rd), recs.append(rec)
    check(w.obj, w.refs, reads, recs, 8)
    # a wave of long reads only: nothing for the first kernel
    reads, recs = [], []
    for i in range(70):
        rd, rec, _ = w.read(i % 2, 257 + 11 * i, 0.02, 0, i % 2)
        reads.append(rd), recs.append(rec)
    check(w.obj, w.refs, reads, recs, 3)


def test_a_batch_beyond_the_small_staging_buffer(world, sample):
    """9 000 reads, over a megabyte of bases: the call takes a device allocation of its own instead of the thread's staging
    slot.  The records of the slices, which fit the slot and are checked against the brute force elsewhere, put together."""
    reads, recs = sample
    short = [(rd, rc) for rd, rc in zip(reads, recs) if 100 <= len(rd) <= 300]
    reads = [short[i % len(short)][0] for i in range(9000)]
    m = map_records([short[i % len(short)][1] for i in range(9000)])
    bases, off = capi.concat_reads(reads)
    assert len(bases) > (1 << 20)
    whole = world.obj.verify(bases, off, m, 8)
    for lo in range(0, 9000, 1500):
        part = world.obj.verify(bases[off[lo]:off[lo + 1500]], off[lo:lo + 1501] - off[lo], m[lo:lo + 1500], 8)
        assert part.tobytes() == whole[lo:lo + 1500].tobytes(), lo
    assert as_tuples(whole[:len(short)]) == vb.records(world.refs, reads[:len(short)], [rc for _, rc in short], 8)


def test_the_fast_limit_changes_no_result(world, sample):
    """verify_fast_bases sends shorter reads to the second kernel: byte-equal records, whichever kernel wrote them"""
    reads, recs = sample
    bases, off = capi.concat_reads(reads)
    m = map_records(recs)
    base = world.obj.verify(bases, off, m, 8)
    assert as_tuples(base) == vb.records(world.refs, reads, recs, 8)
    try:
        for limit in (1, 64, 65, 128):
            capi.set_tuning("verify_fast_bases", limit)
            assert world.obj.verify(bases, off, m, 8).tobytes() == base.tobytes(), limit
    finally:
        capi.set_tuning("verify_fast_bases", 0)


def run_dev(obj, reads, recs, band, ws_extra=0):
    """verify_dev on torch buffers with guard records around d_out; (records, whether the guards are intact)"""
    import torch
    dev = torch.device("cuda", 0)
    bases, off = capi.concat_reads(reads)
    n = len(reads)
    tb = torch.from_numpy(bases).to(dev) if len(bases) else torch.zeros(1, dtype=torch.uint8, device=dev)
    to = torch.from_numpy(off).to(dev)
    tm = torch.from_numpy(map_records(recs).view(np.int64).copy() if n else np.zeros(4, np.int64)).to(dev)
    need = capi.RefSeqs.workspace_bytes(len(bases), n)
    ws = torch.zeros(need + ws_extra, dtype=torch.uint8, device=dev)
    out = torch.full(((n + 2 * GUARD) * 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    obj.verify_dev(tb.data_ptr(), len(bases), to.data_ptr(), n, tm.data_ptr(), out.data_ptr() + 16 * GUARD, ws.data_ptr(), need, band,
                   st.cuda_stream)
    st.synchronize()
    raw = out.cpu().numpy()
    intact = bool((raw[:2 * GUARD] == 0x5A5A5A5A5A5A5A5A).all() and (raw[2 * (GUARD + n):] == 0x5A5A5A5A5A5A5A5A).all())
    return raw[2 * GUARD:2 * (GUARD + n)].view(capi.READ_VERIFY_DTYPE).copy(), intact


def test_verify_dev_writes_its_records_and_nothing_else(world, sample):
    reads, recs = sample
    for band in (0, 8):
        got, intact = run_dev(world.obj, reads, recs, band)
        assert intact
        assert got.tobytes() == world.obj.verify_reads(reads, map_records(recs), band).tobytes()
    got, intact = run_dev(world.obj, reads[:65], recs[:65], 5)
    assert intact and as_tuples(got) == vb.records(world.refs, reads[:65], recs[:65], 5)
    try:
        capi.set_tuning("verify_fast_bases", 64)
        got, intact = run_dev(world.obj, reads[:65], recs[:65], 5)
        assert intact and as_tuples(got) == vb.records(world.refs, reads[:65], recs[:65], 5)
    finally:
        capi.set_tuning("verify_fast_bases", 0)
    got, intact = run_dev(world.obj, [], [], 8)
    assert intact and len(got) == 0


def refused(fn, *needles, code=capi.ERR_INVALID_ARG):
    with pytest.raises(capi.SbwtGpuError) as ei:
        fn()
    assert ei.value.code == code, ei.value
    for s in needles:
        assert s in ei.value.msg, (s, ei.value.msg)


def test_refusals_leave_everything_usable(world):
    import torch
    w, obj = world, world.obj
    rd, rec, _ = w.read(0, 100, 0.01)
    m = map_records([rec])
    bases, off = capi.concat_reads([rd])
    before = obj.info()
    refused(lambda: obj.add([b"ACGT"], 2), "first_seq is 2", "holds 3", "next number is 3")
    refused(lambda: obj.add([b"ACGT"], 4), "first_seq is 4", "3")
    refused(lambda: obj.add([b"ACGT"], -1), "first_seq is -1")
    refused(lambda: obj.add_sequences(np.zeros(4, np.uint8), np.array([0, 4, 2], np.int64), 3), "not non-decreasing")
    L = capi.lib()
    assert L.sbwtgpu_refseqs_add_batch(obj.handle, 3, None, None, 1) == capi.ERR_INVALID_ARG and b"NULL" in L.sbwtgpu_last_error()
    assert L.sbwtgpu_refseqs_add_batch(obj.handle, 3, None, off.ctypes.data, 1) == capi.ERR_INVALID_ARG and b"NULL" in L.sbwtgpu_last_error()
    assert L.sbwtgpu_refseqs_add_batch(obj.handle, 3, None, None, -1) == capi.ERR_INVALID_ARG
    assert L.sbwtgpu_refseqs_add_batch(obj.handle, 3, None, None, (1 << 30) - 2) == capi.ERR_INVALID_ARG and b"2^30" in L.sbwtgpu_last_error()
    # a sequence of 2^31 bases (its offsets say so; nothing is read before the refusal)
    big = np.array([0, 1 << 31], np.int64)
    assert L.sbwtgpu_refseqs_add_batch(obj.handle, 3, bases.ctypes.data, big.ctypes.data, 1) == capi.ERR_READ_TOO_LONG
    for band in (-1, 257, 1 << 20):
        refused(lambda: obj.verify(bases, off, m, band), "band must be in 0 .. 256")
    out = np.zeros(1, capi.READ_VERIFY_DTYPE)
    for args in ((None, off.ctypes.data, 1, m.ctypes.data, 8, out.ctypes.data), (bases.ctypes.data, None, 1, m.ctypes.data, 8, out.ctypes.data),
                 (bases.ctypes.data, off.ctypes.data, 1, None, 8, out.ctypes.data), (bases.ctypes.data, off.ctypes.data, 1, m.ctypes.data, 8, None)):
        assert L.sbwtgpu_refseqs_verify_batch(obj.handle, *args) == capi.ERR_INVALID_ARG and b"NULL" in L.sbwtgpu_last_error()
    assert L.sbwtgpu_refseqs_verify_batch(obj.handle, bases.ctypes.data, off.ctypes.data, -1, m.ctypes.data, 8, out.ctypes.data) == capi.ERR_INVALID_ARG
    assert L.sbwtgpu_refseqs_verify_batch(obj.handle, bases.ctypes.data, off.ctypes.data, 1 << 31, m.ctypes.data, 8, out.ctypes.data) == capi.ERR_INVALID_ARG
    assert b"2^31" in L.sbwtgpu_last_error()
    for seq, pos, n in ((3, 0, 1), (-1, 0, 1), (0, -1, 1), (0, 0, -1), (0, 0, 3001), (0, 3000, 1), (2, 69, 2), (0, 1 << 40, 1)):
        refused(lambda: obj.get(seq, pos, n), "refseqs")
    refused(lambda: obj.get(2, 69, 2), "outside sequence 2 of 70 bases")
    # the device entry point: its workspace, its pointers
    dev = torch.device("cuda", 0)
    tb, to = torch.from_numpy(bases).to(dev), torch.from_numpy(off).to(dev)
    tm, tout = torch.from_numpy(m.view(np.int64).copy()).to(dev), torch.zeros(2, dtype=torch.int64, device=dev)
    need = capi.RefSeqs.workspace_bytes(len(bases), 1)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    refused(lambda: obj.verify_dev(tb.data_ptr(), len(bases), to.data_ptr(), 1, tm.data_ptr(), tout.data_ptr(), ws.data_ptr(), need - 1), "workspace")
    refused(lambda: obj.verify_dev(tb.data_ptr(), len(bases), to.data_ptr(), 1, tm.data_ptr(), tout.data_ptr(), 0, need), "workspace")
    refused(lambda: obj.verify_dev(tb.data_ptr(), len(bases), to.data_ptr(), 1, tm.data_ptr(), tout.data_ptr(), ws.data_ptr() + 8, need), "aligned")
    refused(lambda: obj.verify_dev(tb.data_ptr(), len(bases), to.data_ptr(), 1, tm.data_ptr(), tout.data_ptr(), ws.data_ptr(), need, 300), "band")
    refused(lambda: obj.verify_dev(tb.data_ptr(), len(bases), to.data_ptr(), 1, 0, tout.data_ptr(), ws.data_ptr(), need), "NULL")
    refused(lambda: obj.verify_dev(tb.data_ptr(), len(bases), to.data_ptr(), 1, tm.data_ptr(), 0, ws.data_ptr(), need), "NULL")
    refused(lambda: obj.verify_dev(tb.data_ptr(), len(bases), 0, 1, tm.data_ptr(), tout.data_ptr(), ws.data_ptr(), need), "NULL")
    refused(lambda: obj.verify_dev(tb.data_ptr(), len(bases), to.data_ptr(), -1, tm.data_ptr(), tout.data_ptr(), ws.data_ptr(), need), "n_reads")
    torch.cuda.synchronize(dev)
    # nothing changed, and everything still works
    assert obj.info() == before
    check(obj, w.refs, [rd], [rec], 8)
    assert obj.get(2) == vb.stored(w.refs[2])


def test_two_host_threads_verify_on_one_object(world, sample):
    reads, recs = sample
    halves = [(reads[0::2], recs[0::2], 8), (reads[1::2], recs[1::2], 2)]
    want = [vb.records(world.refs, r, c, b) for r, c, b in halves]
    got, errs = [None, None], []

    def work(i):
        try:
            r, c, b = halves[i]
            for _ in range(4):
                got[i] = as_tuples(world.obj.verify_reads(r, map_records(c), b))
                assert got[i] == want[i]
        except Exception as e:              # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    assert got == want


# ---- 3. behind the map calls ------------------------------------------------------------------------------------------------
K = 15


def test_map_then_verify(world):
    """Occurrences.map on a small index over the three references, then verify on its records: a read without an indel placed
    at its origin has exactly its substitutions as mismatches"""
    w = world
    bits = hostlib.build_bits(w.refs, K, False, True)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, K, bits.n_kmers, 0)
    try:
        with idx.occurrences_builder() as b:
            b.add(w.refs, 0, 1)
            occ = b.finish()
        reads, truth, subs = [], [], []
        for i in range(200):
            indel = (0, 0, 0, 1, -2)[i % 5]
            # (the reads without an indel from the sequence of valid bases only: there a mismatch is a substitution)
            rd, rec, s = w.read(i % 2 if indel else 0, 150, 0.01 if i % 4 else 0.0, indel)
            reads.append(rd), truth.append(rec), subs.append(None if indel else s)
        bases, off = capi.concat_reads(reads)
        placed = occ.map(bases, off, 1)
        out = w.obj.verify(bases, off, placed, 8)
        recs = [(int(p["seq"]), int(p["strand"]), int(p["start"])) for p in placed]
        assert as_tuples(out) == vb.records(w.refs, reads, recs, 8)
        at_origin = found_indel = 0
        for o, rec, t, s in zip(out, recs, truth, subs):
            if s is not None and rec == t:
                assert (int(o["mismatches"]), int(o["edit"]) <= s) == (s, True)
                at_origin += 1
            elif s is None and rec[0] >= 0:
                found_indel += int(o["edit"]) < int(o["mismatches"])    # the diagonal is lost behind the indel, the table finds it
        # 120 reads without an indel, 80 with one (all but those whose indel sits within a few bases of an end show it)
        assert at_origin > 80 and found_indel > 60
        occ.close()
    finally:
        idx.close()


def test_cli_refs(gpu, tmp_path):
    import test_gpu_pseudoalign_wide as tw
    d = str(tmp_path)
    k = 11
    rng = random.Random(2870)
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
    for i in range(60):
        src = seqs[i % 5]
        n = rng.randint(12, min(90, len(src)))
        a = rng.randrange(0, len(src) - n + 1)
        r = bytearray(mutate(rng, src[a:a + n], 0.03, b"ACGTN" if i % 6 == 0 else b"ACGT"))
        if i % 4 == 1 and len(r) > 30:
            del r[15:17]
        if i % 4 == 3 and len(r) > 30:
            r[20:20] = b"G"
        batch.append(vb.rc(bytes(r)) if i % 3 == 2 else bytes(r))
    batch += [b"ACG", rand_seq(rng, 60), b"T" * 40, seqs[0][:40], seqs[4][-20:]]
    with open(d + "/reads.fastq", "w") as fh:
        fh.write("".join("@r%d\n%s\n+\n%s\n" % (i, r.decode(), "I" * len(r)) for i, r in enumerate(batch)))
    SBWT, index = tw.SBWT, d + "/x.sbwt"
    p = tw.run([SBWT, "build", "-i", d + "/all.fna", "-o", index, "-k", str(k), "--temp-dir", d, "--add-reverse-complements"])
    assert p.returncode == 0, p.stderr.decode()
    p = tw.run([SBWT, "build-colors", "--both-strands", "-i", index, "-r", d + "/refs.txt", "-o", d + "/x.colors", "--occurrences-out", d + "/x.occ",
                "--positions-out", d + "/x.pos"])
    assert p.returncode == 0, p.stderr.decode()
    base = [SBWT, "read-hits", "-i", index, "-q", d + "/reads.fastq", "--both-strands", "--batch-bases", "700"]
    p = tw.run(base + ["-o", d + "/plain.hits"])
    assert p.returncode == 0, p.stderr.decode()
    plain = open(d + "/plain.hits", "rb").read().splitlines()
    for option, file in (("--positions", d + "/x.pos"), ("--occurrences", d + "/x.occ")):
        p = tw.run(base + ["-o", d + "/placed.hits", option, file])
        assert p.returncode == 0, p.stderr.decode()
        placed = open(d + "/placed.hits", "rb").read().splitlines()
        assert len(placed) == len(batch) and [ln.split()[:4] for ln in placed] == [ln.split() for ln in plain]
        for band in (None, 0, 3):
            p = tw.run(base + ["-o", d + "/verified.hits", option, file, "--refs", d + "/refs.txt"] + ([] if band is None else ["--band", str(band)]))
            assert p.returncode == 0, p.stderr.decode()
            lines = open(d + "/verified.hits", "rb").read().splitlines()
            assert len(lines) == len(batch)
            n_placed = 0
            for ln, before, rd in zip(lines, placed, batch):
                f = ln.split()
                assert len(f) == 13 and b" ".join(f[:10]) == before             # the line it had, then three columns
                rec = (int(f[4]), int(f[5]), int(f[6]))
                want = vb.record(seqs, rd, rec, 8 if band is None else band)
                assert b" ".join(f[10:]) == vb.cli_columns(want).encode(), (option, band, ln, want)
                n_placed += rec[0] >= 0
            assert n_placed > 40
    # without --refs the command prints what it printed before: the table of the read-hit profiles, and the six columns alone
    assert all(len(ln.split()) == 4 for ln in plain) and all(len(ln.split()) == 10 for ln in placed)
    # a list that does not hold the placement file's sequences
    with open(d + "/short.txt", "w") as lst:
        lst.write(d + "/ref0.fna\n")
    p = tw.run(base + ["-o", d + "/y.hits", "--positions", d + "/x.pos", "--refs", d + "/short.txt"])
    assert p.returncode == 1 and b"2 sequences, the placement file lists 5" in p.stderr


# ---- 4. a bounded fuzz ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_fuzz(gpu, seed):
    rng = random.Random(28000 + seed)
    alphabet = rng.choice([b"ACGT", b"ACGT", b"AC", b"ACGTN", b"ACGTNacgt\x00"])
    refs = [rand_seq(rng, rng.randint(1, 2000), alphabet) for _ in range(rng.randint(1, 5))]
    band = rng.randint(0, 40)
    reads, recs = [], []
    for i in range(rng.randint(100, 260)):
        seq = rng.randrange(len(refs))
        ref = refs[seq]
        L = rng.randint(1, 300) if rng.random() < 0.97 else rng.randint(301, 1100)
        kind = rng.random()
        if kind < 0.7:                                           # a mutated true placement
            at = rng.randrange(0, max(len(ref) - L, 0) + 1)
            r = bytearray(mutate(rng, ref[at:at + L], rng.choice([0.0, 0.01, 0.05, 0.3]), b"ACGTN"))
            for _ in range(rng.randint(0, 2)):
                q = rng.randrange(0, len(r) + 1)
                if rng.random() < 0.5:
                    r[q:q] = rand_seq(rng, rng.randint(1, 5))
                else:
                    del r[q:q + rng.randint(1, 5)]
            strand = rng.randint(0, 1)
            rd = vb.rc(bytes(r)) if strand else bytes(r)
            rec = (seq, strand, at + rng.randint(-3, 3))
        elif kind < 0.9:                                         # a random record
            rd = rand_seq(rng, L, alphabet)
            rec = (seq, rng.randint(0, 1), rng.randint(-L - band - 10, len(ref) + band + 10))
        else:                                                    # out of range
            rd = rand_seq(rng, L % 50, alphabet)
            rec = rng.choice([(len(refs), 0, 0), (-1, 1, 3), (seq, 2, 0), (seq, -7, 1), (seq, 0, 1 << 41), ((1 << 31) - 1, 0, 0)])
        reads.append(rd), recs.append(rec)
    with capi.RefSeqs.create() as o:
        half = rng.randint(0, len(refs))
        o.add(refs[:half], 0)
        o.add(refs[half:], half)
        assert o.info()["n_invalid"] == vb.n_invalid(refs)
        for s, ref in enumerate(refs):
            assert o.get(s) == vb.stored(ref)
        limit = rng.choice([0, 0, 1, 100, 200])
        try:
            capi.set_tuning("verify_fast_bases", limit)
            check(o, refs, reads, recs, band, (seed, limit))
        finally:
            capi.set_tuning("verify_fast_bases", 0)
