"""GPU: sbwtgpu_align_* (sbwt_align.hip: the begin of a verified read's best alignment and its runs of = X I D) against the
definition in tests/align_brute.py.  Every comparison is exact: the verify records, the align records field for field, the
run offsets and every run."""
import random
import re
import threading

import numpy as np
import pytest

import align_brute as ab
import verify_brute as vb
from sbwt_amd import capi, hostlib
from test_gpu_verify import BANDS, GUARD, LENGTHS, World, map_records, mutate, rand_seq, refused

pytestmark = pytest.mark.gpu

JUNK64 = 0x5A5A5A5A5A5A5A5A


def unpack(res):
    """(verify, align, op_off, ops) as the brute force's triples: (verify record, align record, runs) per read"""
    verify, align, op_off, ops = res
    assert verify.dtype == capi.READ_VERIFY_DTYPE and align.dtype == capi.READ_ALIGN_DTYPE and ops.dtype == np.uint32
    assert len(op_off) == len(align) + 1 and op_off[0] == 0 and op_off[-1] == len(ops)
    return [((int(v["ref_end"]), int(v["mismatches"]), int(v["edit"])), (int(a["ref_begin"]), int(a["n_ops"]), int(a["n_eq"])),
             ab.decode(ops[op_off[i]:op_off[i + 1]])) for i, (v, a) in enumerate(zip(verify, align))]


def check(obj, refs, reads, recs, band, label=None, want=None):
    """the object's alignments for the batch against the brute force, read for read; -> (the call's arrays, the triples)"""
    res = obj.align_reads(reads, map_records(recs), band)
    got = unpack(res)
    want = ab.alignments(refs, reads, recs, band) if want is None else want
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (label, i, len(reads[i]), recs[i], band, g, w)
        assert g[1][1] == len(g[2]) == res[2][i + 1] - res[2][i]
    assert len(got) == len(want) == len(reads)
    return res, got


@pytest.fixture(scope="module")
def world(gpu):
    w = World()
    yield w
    w.obj.close()


def with_substitutions(w, seq, L, n_subs, strand=0):
    """(read, record): L bases of sequence seq with n_subs substitutions spread evenly, each to the base's complement"""
    ref = w.refs[seq]
    at = w.rng.randrange(600, len(ref) - L - 600)          # (sequence 1: between its N runs)
    r = bytearray(ref[at:at + L])
    for j in range(n_subs):
        q = (2 * j + 1) * L // (2 * n_subs)
        r[q] = vb._COMP[r[q]]
    return (vb.rc(bytes(r)) if strand else bytes(r)), (seq, strand, at)


def make_sample(w):
    """Every length class on the two long references, clean and with 1 % and 5 % substitutions, both strands; indels of 1, 2 and 5
    bases either way; placements shifted by -3 .. 3; reads of edit 30 .. 33, around the first kernel's limit, and one of 1024
    bases at 10 % errors.  One shuffled batch: every wave mixes band widths, lanes of edit 0 and reads for the second kernel."""
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
    for n_subs in (30, 31, 32, 33):
        for L, strand in ((250, 0), (256, 1)):
            rd, rec = with_substitutions(w, 0, L, n_subs, strand)
            reads.append(rd), recs.append(rec)
    rd, rec, _ = w.read(0, 1024, 0.10, 3, 1)
    reads.append(rd), recs.append(rec)
    order = list(range(len(reads)))
    random.Random(5).shuffle(order)
    return [reads[i] for i in order], [recs[i] for i in order]


@pytest.fixture(scope="module")
def sample(world):
    return make_sample(world)


@pytest.fixture(scope="module")
def sample8(world, sample):
    """the sample's alignments at band 8 from the brute force, computed once"""
    return ab.alignments(world.refs, sample[0], sample[1], 8)


# ---- 1. alignment for alignment ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", BANDS)
def test_alignments_of_every_length_class(world, sample, sample8, band):
    reads, recs = sample
    _, got = check(world.obj, world.refs, reads, recs, band, want=sample8 if band == 8 else None)
    assert len(reads) > 140 and {len(r) for r in reads} >= set(LENGTHS)
    edits = [g[0][2] for g in got]
    assert sum(1 for e in edits if e == 0) > 10 and sum(1 for e in edits if e == -1) >= 6
    if band == 8:
        assert {30, 31, 32, 33} <= set(edits) and max(edits) > 60                   # either side of the first kernel's limit
        assert sum(1 for g in got if any(op in "ID" for _, op in g[2])) > 20
        assert len({e for e in edits if 0 < e < 16}) >= 8                           # every band width of the first kernel


@pytest.mark.parametrize("band", (0, 5, 64))
def test_placements_at_and_beyond_the_ends(world, band):
    """starts from -L - B - 5 to n + B + 5: the band of diagonals touches column 0 and the window's right edge"""
    w = world
    reads, recs = [], []
    for seq in (0, 1, 2):
        n = len(w.refs[seq])
        for L in (1, 30, 64, 70, 150, 257):
            for strand in (0, 1):
                rd, _, _ = w.read(seq, L, 0.01, 0, strand) if L <= n else (rand_seq(w.rng, L), None, 0)
                for start in (-L - band - 5, -L - band, -L, -band - 1, -3, -1, 0, n - L, n - L + 1, n - 2, n, n + band, n + band + 5):
                    reads.append(rd), recs.append((seq, strand, start))
        for L in (1, 33, min(n, 65)):
            reads += [w.refs[seq][:L], w.refs[seq][n - L:]]
            recs += [(seq, 0, 0), (seq, 0, n - L)]
    _, got = check(w.obj, w.refs, reads, recs, band)
    assert sum(1 for g in got if g[2] and g[2][0][1] == "I") > 30 and sum(1 for g in got if g[0][2] == 0) >= 6
    assert sum(1 for g in got if g[1][0] < 0) >= 3 or band == 0


def test_the_neighbours_in_the_packed_arrays_do_not_matter(world):
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
            a, _ = check(w.obj, w.refs, reads, recs, band)
            b = o.align_reads(reads, map_records(recs), band)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_the_fast_limit_changes_no_result(world, sample, sample8):
    """align_fast_edit sends reads of smaller edit to the second kernel: byte-equal output, whichever kernel wrote it"""
    reads, recs = sample
    base, _ = check(world.obj, world.refs, reads, recs, 8, want=sample8)
    try:
        for limit in (1, 2, 7):
            capi.set_tuning("align_fast_edit", limit)
            got = world.obj.align_reads(reads, map_records(recs), 8)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(base, got)), limit
    finally:
        capi.set_tuning("align_fast_edit", 0)


# ---- 2. the device entry point ------------------------------------------------------------------------------------------------
def run_dev(obj, reads, recs, band, ops_cap):
    """align_dev on torch buffers with guards around d_out and d_op_off and behind d_ops[ops_cap];
    (verify, align, op_off, the ops_cap stored runs, whether the guards are intact)"""
    import torch
    dev = torch.device("cuda", 0)
    bases, off = capi.concat_reads(reads)
    n = len(reads)
    tb = torch.from_numpy(bases).to(dev) if len(bases) else torch.zeros(1, dtype=torch.uint8, device=dev)
    to = torch.from_numpy(off).to(dev)
    tm = torch.from_numpy(map_records(recs).view(np.int64).copy() if n else np.zeros(4, np.int64)).to(dev)
    need = capi.RefSeqs.align_workspace_bytes(len(bases), n)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    ver = torch.full(((n + 2 * GUARD) * 2,), JUNK64, dtype=torch.int64, device=dev)
    out = torch.full(((n + 2 * GUARD) * 2,), JUNK64, dtype=torch.int64, device=dev)
    ooff = torch.full((n + 1 + 2 * GUARD,), JUNK64, dtype=torch.int64, device=dev)
    ops = torch.full((ops_cap + 2 * GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    obj.align_dev(tb.data_ptr(), len(bases), to.data_ptr(), n, tm.data_ptr(), ver.data_ptr() + 16 * GUARD, out.data_ptr() + 16 * GUARD,
                  ooff.data_ptr() + 8 * GUARD, ops.data_ptr() + 4 * GUARD, ops_cap, ws.data_ptr(), need, band, st.cuda_stream)
    st.synchronize()
    rv, ro, rf, rp = ver.cpu().numpy(), out.cpu().numpy(), ooff.cpu().numpy(), ops.cpu().numpy()
    intact = True
    for raw, lo, hi, junk in ((rv, 2 * GUARD, 2 * (GUARD + n), JUNK64), (ro, 2 * GUARD, 2 * (GUARD + n), JUNK64),
                              (rf, GUARD, GUARD + n + 1, JUNK64), (rp, GUARD, GUARD + ops_cap, 0x5A5A5A5A)):
        intact = intact and bool((raw[:lo] == junk).all() and (raw[hi:] == junk).all())
    return (rv[2 * GUARD:2 * (GUARD + n)].view(capi.READ_VERIFY_DTYPE).copy(), ro[2 * GUARD:2 * (GUARD + n)].view(capi.READ_ALIGN_DTYPE).copy(),
            rf[GUARD:GUARD + n + 1].copy(), rp[GUARD:GUARD + ops_cap].view(np.uint32).copy(), intact)


def test_align_dev_against_align_batch_and_verify_dev(world, sample):
    from test_gpu_verify import run_dev as verify_dev
    reads, recs = sample
    for band in (0, 8):
        v, a, off, ops = world.obj.align_reads(reads, map_records(recs), band)
        total = int(off[-1])
        dv, da, doff, dops, intact = run_dev(world.obj, reads, recs, band, total)
        assert intact
        assert (dv.tobytes(), da.tobytes(), doff.tobytes(), dops.tobytes()) == (v.tobytes(), a.tobytes(), off.tobytes(), ops.tobytes())
        only, intact = verify_dev(world.obj, reads, recs, band)
        assert intact and only.tobytes() == dv.tobytes()                # d_verify_out is what verify_dev writes


def test_ops_cap_bounds_what_is_stored(world, sample):
    reads, recs = sample
    v, a, off, ops = world.obj.align_reads(reads, map_records(recs), 8)
    total = int(off[-1])
    assert total > 500
    for cap in (0, total - 1, total, total + 7, 3):
        dv, da, doff, dops, intact = run_dev(world.obj, reads, recs, 8, cap)
        assert intact, cap                                              # nothing at or beyond d_ops[ops_cap]
        assert (dv.tobytes(), da.tobytes(), doff.tobytes()) == (v.tobytes(), a.tobytes(), off.tobytes()), cap
        assert doff[-1] == total                                        # the true total, whatever was stored
        m = min(cap, total)
        assert dops[:m].tobytes() == ops[:m].tobytes(), cap
        assert (dops[m:] == 0x5A5A5A5A).all()
    dv, da, doff, dops, intact = run_dev(world.obj, [], [], 8, 4)
    assert intact and len(dv) == len(da) == 0 and doff.tolist() == [0] and (dops == 0x5A5A5A5A).all()


def test_small_batches(world):
    w = world
    v, a, off, ops = w.obj.align_reads([], map_records([]), 8)
    assert len(v) == len(a) == len(ops) == 0 and off.tolist() == [0]
    rd, rec, _ = w.read(0, 150, 0.01, 0, 1)
    check(w.obj, w.refs, [rd], [rec], 8)
    _, got = check(w.obj, w.refs, [b""], [(0, 0, 7)], 8)
    assert got == [((-1, 0, 0), (-1, 0, 0), [])]
    _, got = check(w.obj, w.refs, [b"", b"ACGT", b""], [(0, 0, 7), (9, 0, 0), (1, 1, -2)], 3)       # no runs at all
    assert [g[1] for g in got] == [(4, 0, 0), (0, 0, 0), (-5, 0, 0)]
    # 65 reads: the second wave has one lane
    reads, recs = [], []
    for i in range(65):
        rd, rec, _ = w.read(i % 2, 100 + i, 0.02, (i % 3) - 1, i % 2)
        reads.append(rd), recs.append(rec)
    check(w.obj, w.refs, reads, recs, 8)
    # a wave of reads for the second kernel only: longer than the first kernel's rows, or of more than 31 edits
    reads, recs = [], []
    for i in range(70):
        rd, rec, _ = w.read(i % 2, 257 + 11 * i, 0.02, 0, i % 2) if i % 2 else w.read(i % 2, 100 + i, 0.5, 0, i % 2)
        reads.append(rd), recs.append(rec)
    _, got = check(w.obj, w.refs, reads, recs, 3)
    assert all(g[0][2] > 31 or len(rd) > 256 for g, rd in zip(got, reads))


def test_a_batch_beyond_the_small_staging_buffer(world, sample, sample8):
    """9 000 reads, over a megabyte of bases: more groups of 64 than the first kernel has waves.  The output of the slices put
    together, and the first of them against the brute force."""
    reads, recs = sample
    short = [i for i, rd in enumerate(reads) if 100 <= len(rd) <= 300]
    pick = [short[i % len(short)] for i in range(9000)]
    many = [reads[i] for i in pick]
    m = map_records([recs[i] for i in pick])
    bases, off = capi.concat_reads(many)
    assert len(bases) > (1 << 20)
    whole = world.obj.align(bases, off, m, 8)
    assert unpack(whole)[:len(short)] == [sample8[i] for i in short]
    for lo in range(0, 9000, 3000):
        part = world.obj.align(bases[off[lo]:off[lo + 3000]], off[lo:lo + 3001] - off[lo], m[lo:lo + 3000], 8)
        assert part[0].tobytes() == whole[0][lo:lo + 3000].tobytes() and part[1].tobytes() == whole[1][lo:lo + 3000].tobytes()
        assert (part[2] + whole[2][lo]).tobytes() == whole[2][lo:lo + 3001].tobytes()
        assert part[3].tobytes() == whole[3][whole[2][lo]:whole[2][lo + 3000]].tobytes()


def test_refusals_leave_everything_usable(world):
    import ctypes as C
    import torch
    w, obj = world, world.obj
    rd, rec, _ = w.read(0, 100, 0.01)
    m = map_records([rec])
    bases, off = capi.concat_reads([rd])
    before = obj.info()
    for band in (-1, 257, 1 << 20):
        refused(lambda: obj.align(bases, off, m, band), "band must be in 0 .. 256")
    L = capi.lib()
    ver, out, ooff = np.zeros(1, capi.READ_VERIFY_DTYPE), np.zeros(1, capi.READ_ALIGN_DTYPE), np.zeros(2, np.int64)
    p, n = C.c_void_p(), C.c_int64()
    good = [bases.ctypes.data, off.ctypes.data, 1, m.ctypes.data, 8, ver.ctypes.data, out.ctypes.data, ooff.ctypes.data, C.byref(p), C.byref(n)]
    for hole in (0, 1, 3, 5, 6, 7, 8, 9):
        args = list(good)
        args[hole] = None
        assert L.sbwtgpu_align_batch(obj.handle, *args) == capi.ERR_INVALID_ARG and b"NULL" in L.sbwtgpu_last_error(), hole
    args = list(good)
    args[2] = -1
    assert L.sbwtgpu_align_batch(obj.handle, *args) == capi.ERR_INVALID_ARG and b"n_reads" in L.sbwtgpu_last_error()
    args[2] = 1 << 31
    assert L.sbwtgpu_align_batch(obj.handle, *args) == capi.ERR_INVALID_ARG and b"2^31" in L.sbwtgpu_last_error()
    # the device entry point: its workspace, its pointers, ops_cap
    dev = torch.device("cuda", 0)
    tb, to = torch.from_numpy(bases).to(dev), torch.from_numpy(off).to(dev)
    tm = torch.from_numpy(m.view(np.int64).copy()).to(dev)
    tv, tout, toff = (torch.zeros(2, dtype=torch.int64, device=dev) for _ in range(3))
    tops = torch.zeros(64, dtype=torch.int32, device=dev)
    need = capi.RefSeqs.align_workspace_bytes(len(bases), 1)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)

    def call(**kw):
        a = dict(d_bases=tb.data_ptr(), total_bases=len(bases), d_read_off=to.data_ptr(), n_reads=1, d_map=tm.data_ptr(),
                 d_verify_out=tv.data_ptr(), d_out=tout.data_ptr(), d_op_off=toff.data_ptr(), d_ops=tops.data_ptr(), ops_cap=64,
                 d_ws=ws.data_ptr(), ws_bytes=need, band=8)
        a.update(kw)
        return lambda: obj.align_dev(**a)

    refused(call(ws_bytes=need - 1), "workspace")
    refused(call(d_ws=0), "workspace")
    refused(call(d_ws=ws.data_ptr() + 8), "aligned")
    refused(call(band=300), "band")
    refused(call(ops_cap=-1), "ops_cap")
    refused(call(n_reads=-1), "n_reads")
    for name in ("d_map", "d_read_off", "d_verify_out", "d_out", "d_op_off", "d_ops"):
        refused(call(**{name: 0}), "NULL")
    call(d_ops=0, ops_cap=0)()                                          # no room for runs needs no d_ops
    torch.cuda.synchronize(dev)
    assert int(toff.cpu()[1]) >= 1
    # nothing changed, and everything still works
    assert obj.info() == before
    check(obj, w.refs, [rd], [rec], 8)


def test_two_host_threads_align_on_one_object(world, sample):
    reads, recs = sample
    halves = [(reads[0::2], recs[0::2], 8), (reads[1::2], recs[1::2], 2)]
    want = [ab.alignments(world.refs, r, c, b) for r, c, b in halves]
    got, errs = [None, None], []

    def work(i):
        try:
            r, c, b = halves[i]
            for _ in range(4):
                got[i] = unpack(world.obj.align_reads(r, map_records(c), b))
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


def test_map_then_align(world):
    """Occurrences.map on a small index over the three references, then align on its records: a read without an indel placed at
    its origin begins there and has one run per boundary between matches and substitutions"""
    w = world
    bits = hostlib.build_bits(w.refs, K, False, True)
    idx = capi.Index.create(bits.cols[0], bits.cols[1], bits.cols[2], bits.cols[3], bits.ssup, bits.n_nodes, K, bits.n_kmers, 0)
    try:
        with idx.occurrences_builder() as b:
            b.add(w.refs, 0, 1)
            occ = b.finish()
        reads, truth, planted = [], [], []
        for i in range(200):
            indel = (0, 0, 0, 1, -2)[i % 5]
            rd, rec, _ = w.read(i % 2 if indel else 0, 150, 0.01 if i % 4 else 0.0, indel)
            reads.append(rd), truth.append(rec), planted.append(indel)
        bases, off = capi.concat_reads(reads)
        placed = occ.map(bases, off, 1)
        recs = [(int(p["seq"]), int(p["strand"]), int(p["start"])) for p in placed]
        got = unpack(w.obj.align(bases, off, placed, 8))
        assert got == ab.alignments(w.refs, reads, recs, 8)
        at_origin = found_indel = 0
        for (v, a, runs), rec, t, indel, rd in zip(got, recs, truth, planted, reads):
            if indel == 0 and rec == t:
                # the runs of the diagonal: = where the read has the reference's base, X where it does not
                ref = w.refs[0][t[2]:t[2] + len(rd)]
                assert a[0] == t[2] and runs == ab.merge(["=" if x == y else "X" for x, y in zip(reversed(rd), reversed(ref))])
                assert a[1] == len(runs) and v[2] == v[1] == sum(n for n, op in runs if op == "X")
                at_origin += 1
            elif indel and rec[0] >= 0:
                found_indel += (abs(indel), "I" if indel > 0 else "D") in runs
        assert at_origin > 80 and found_indel > 50
        occ.close()
    finally:
        idx.close()


def test_cli_cigar(gpu, tmp_path):
    import test_gpu_pseudoalign_wide as tw
    d = str(tmp_path)
    k = 11
    rng = random.Random(2970)
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
    batch += [b"ACG", rand_seq(rng, 60), b"T" * 40, seqs[0][:40], seqs[4][-20:], seqs[0][100:180] + seqs[0][182:252]]
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
        for band in (None, 3):
            extra = [option, file, "--refs", d + "/refs.txt"] + ([] if band is None else ["--band", str(band)])
            p = tw.run(base + ["-o", d + "/verified.hits"] + extra)
            assert p.returncode == 0, p.stderr.decode()
            verified = open(d + "/verified.hits", "rb").read().splitlines()
            p = tw.run(base + ["-o", d + "/aligned.hits"] + extra + ["--cigar"])
            assert p.returncode == 0, p.stderr.decode()
            lines = open(d + "/aligned.hits", "rb").read().splitlines()
            assert len(lines) == len(verified) == len(batch)
            n_runs = 0
            for ln, before, rd in zip(lines, verified, batch):
                f = ln.split()
                assert len(f) == 15 and b" ".join(f[:13]) == before             # the line without --cigar, then two columns
                rec = (int(f[4]), int(f[5]), int(f[6]))
                v, a, runs = ab.alignment(seqs, rd, rec, 8 if band is None else band)
                assert b" ".join(f[10:]) == ab.cli_columns(v, a, runs).encode(), (option, band, ln, v, a, runs)
                n_runs += len(runs) > 0
            assert n_runs > 40 and sum(1 for ln in lines if ln.endswith(b" 0 *")) >= 1
            if band is None:                                                    # the read with 2 reference bases missing
                f = lines[-1].split()
                assert f[4:7] == [b"0", b"0", b"100"] and f[11:14] == [b"2", b"252", b"100"] and re.fullmatch(rb"\d+=2D\d+=", f[14]), lines[-1]


# ---- 4. a bounded fuzz ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_fuzz(gpu, seed):
    rng = random.Random(29000 + seed)
    alphabet = rng.choice([b"ACGT", b"ACGT", b"AC", b"ACGTN", b"ACGTNacgt\x00"])
    refs = [rand_seq(rng, rng.randint(1, 2000), alphabet) for _ in range(rng.randint(1, 5))]
    band = rng.randint(0, 40)
    reads, recs = [], []
    for i in range(rng.randint(100, 200)):
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
        limit = rng.choice([0, 0, 1, 3, 12])
        try:
            capi.set_tuning("align_fast_edit", limit)
            _, got = check(o, refs, reads, recs, band, (seed, limit))
        finally:
            capi.set_tuning("align_fast_edit", 0)
        for (v, a, runs), rd, rec in zip(got, reads, recs):
            if runs:                                             # the runs replayed over the reference give back the read
                assert ab.replay(refs[rec[0]], vb.orient(rd, rec[1]), a[0], runs) == v[0]
