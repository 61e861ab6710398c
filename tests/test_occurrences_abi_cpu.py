"""CPU: the occurrence layer's surface without a device -- the header declares the names and the libraries export them, NULL
handles are refused before anything touches a GPU, the workspace arithmetic, the tuning keys and the bounds of max_occ, the
two subcommands name their new options, and the occurrence file: its bytes, its round trip and every refusal."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from sbwt_amd import capi, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")
NAMES = ["sbwtgpu_occurrences_builder_create", "sbwtgpu_occurrences_builder_add_batch", "sbwtgpu_occurrences_builder_finish",
         "sbwtgpu_occurrences_builder_destroy", "sbwtgpu_occurrences_upload", "sbwtgpu_occurrences_destroy", "sbwtgpu_occurrences_info",
         "sbwtgpu_occurrences_offsets_copy", "sbwtgpu_occurrences_keys_copy", "sbwtgpu_occurrences_offsets_dev",
         "sbwtgpu_occurrences_keys_dev", "sbwtgpu_occurrences_to_positions", "sbwtgpu_occurrences_map_workspace_bytes",
         "sbwtgpu_occurrences_map_dev", "sbwtgpu_occurrences_map_batch"]


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_the_header_declares_the_names_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", header("sbwtgpu.h"), flags=re.S)
    declared = sorted(set(re.findall(r"\b(sbwtgpu_occurrences_\w+)\s*\(", text)))
    assert declared == sorted(NAMES)
    L = capi.lib()
    for n in NAMES:
        assert hasattr(L, n) and n in capi.EXPORTED_SYMBOLS, n
    assert "typedef struct sbwtgpu_occurrences sbwtgpu_occurrences;" in text
    assert "typedef struct sbwtgpu_occurrences_builder sbwtgpu_occurrences_builder;" in text
    m = re.search(r"#define\s+SBWTGPU_OCCURRENCES_MAP_TABLE\s+(\d+)\b", text)
    assert m and int(m.group(1)) == capi.OCCURRENCES_MAP_TABLE >= 256
    assert re.search(r"#define\s+SBWTGPU_OCCURRENCES_MAX_OCC\s+\(1 << 20\)", text) and capi.OCCURRENCES_MAX_OCC == 1 << 20
    # the definitions stand in the header
    full = header("sbwtgpu.h")
    for phrase in ("off[0] = 0, non-decreasing and off[n] = N", "strictly\n *     ascending", "occ[off[v]] == first[v]",
                   "A palindromic window with two strands leaves both keys", "ONE VOTE FOR EACH of its c occurrences",
                   "a hit votes at most once per placement", "n_anchored is the hits that voted, not the number of votes cast",
                   "THEY ARE SERIALISED", "bytes per logged hit", "{0, -1, 0, 0, 0, n_found, 0}"):
        assert phrase in full, phrase
    for n in ("sbwthost_occurrences_write", "sbwthost_occurrences_read"):
        assert hasattr(hostlib.lib(), n) and n in hostlib.EXPORTED_SYMBOLS and n in header("sbwthost.h")


def refused(rc, *needles):
    assert rc == capi.ERR_INVALID_ARG
    msg = capi.lib().sbwtgpu_last_error().decode()
    for s in needles:
        assert s in msg, (s, msg)


def test_null_handles_are_refused_without_a_device():
    L = capi.lib()
    h = C.c_void_p()
    off = np.zeros(2, dtype=np.int64)
    out = np.zeros(1, dtype=capi.READ_MAP_DTYPE)
    refused(L.sbwtgpu_occurrences_builder_create(None, C.byref(h)), "occurrences", "NULL")
    refused(L.sbwtgpu_occurrences_builder_add_batch(None, 0, None, off.ctypes.data, 1, 1, None, None), "occurrences", "NULL")
    refused(L.sbwtgpu_occurrences_builder_finish(None, C.byref(h)), "occurrences", "NULL")
    refused(L.sbwtgpu_occurrences_builder_finish(None, None), "occurrences", "NULL")
    refused(L.sbwtgpu_occurrences_upload(None, off.ctypes.data, off.ctypes.data, 0, C.byref(h)), "occurrences", "NULL")
    refused(L.sbwtgpu_occurrences_info(None, None, None, None, None, None, None, None, None), "occurrences", "NULL")
    refused(L.sbwtgpu_occurrences_offsets_copy(None, off.ctypes.data), "occurrences", "NULL")
    refused(L.sbwtgpu_occurrences_keys_copy(None, off.ctypes.data), "occurrences", "NULL")
    refused(L.sbwtgpu_occurrences_offsets_dev(None, C.byref(h)), "occurrences", "NULL")
    refused(L.sbwtgpu_occurrences_keys_dev(None, C.byref(h)), "occurrences", "NULL")
    refused(L.sbwtgpu_occurrences_to_positions(None, C.byref(h)), "occurrences", "NULL")
    refused(L.sbwtgpu_occurrences_map_batch(None, None, off.ctypes.data, 1, 1, 16, out.ctypes.data), "occurrences", "NULL")
    refused(L.sbwtgpu_occurrences_map_dev(None, None, 0, None, 0, 1, 16, None, None, 0, None), "occurrences", "NULL")
    L.sbwtgpu_occurrences_destroy(None)
    L.sbwtgpu_occurrences_builder_destroy(None)
    assert h.value is None


def test_workspace_bytes_and_the_tuning_keys():
    W = capi.Occurrences.workspace_bytes
    prev = -1
    for nb, nr in ((0, 0), (0, 1), (100, 1), (100, 7), (1 << 20, 1000), (1 << 24, 1 << 17), (1 << 28, 1 << 21)):
        for strands in (1, 2):
            w = W(nb, nr, strands)
            # the search and its results in front, the map header and 4 bytes per read behind them
            assert w % 256 == 0 and w >= capi.pseudoalign_workspace_bytes(nb, nr, strands == 2) + 256 + 4 * nr
        assert W(nb, nr, 1) >= prev and W(nb, nr, 2) >= W(nb, nr, 1)
        prev = W(nb, nr, 1)
    assert W(-5, -5, 1) == W(0, 0, 1)
    T = capi.OCCURRENCES_MAP_TABLE
    for v in (0, 1, 4, T):
        capi.set_tuning("occurrences_map_table", v)
    capi.set_tuning("occurrences_map_table", 0)
    for v in (-1, T + 1):
        with pytest.raises(capi.SbwtGpuError) as ei:
            capi.set_tuning("occurrences_map_table", v)
        assert ei.value.code == capi.ERR_INVALID_ARG and "occurrences_map_table" in ei.value.msg
    capi.set_tuning("occurrences_chunk_bases", 1)
    capi.set_tuning("occurrences_chunk_bases", 0)


def test_the_subcommands_name_their_new_options():
    p = subprocess.run([SBWT, "build-colors", "--help"], capture_output=True, timeout=60)
    assert b"--occurrences-out" in p.stderr and b"occurrence file" in p.stderr and b"--positions-out" in p.stderr
    p = subprocess.run([SBWT, "read-hits", "--help"], capture_output=True, timeout=60)
    assert b"--occurrences" in p.stderr and b"--max-occ" in p.stderr and b"seq strand start votes votes2 n_anchored" in p.stderr
    assert b"default is 1024" in p.stderr and b"Cannot be combined with --positions" in p.stderr


def key(seq, pos, t=0):
    return (seq << 32) | (pos << 1) | t


def test_occurrence_file_bytes_round_trip_and_refusals(tmp_path):
    path = str(tmp_path / "x.occ")
    k = 5
    off = np.array([0, 0, 2, 2, 5, 6], dtype=np.uint64)                 # five columns
    occ = np.array([key(0, 3), key(2, 0, 1), key(0, 0), key(0, 0, 1), key(1, 2), key(2, 95)], dtype=np.uint64)
    col, ln = [0, 0, 4], [20, 7, 100]
    hostlib.occurrences_write(path, off, occ, k, col, ln)
    raw = open(path, "rb").read()
    body = 40 + 3 * 16
    assert raw[:8] == b"SBWTOCC1" and len(raw) == body + 6 * 8 + 6 * 8
    assert np.frombuffer(raw[8:40], dtype=np.int64).tolist() == [5, 5, 3, 6]             # n_columns, k, n_seqs, n_occ
    assert np.frombuffer(raw[40:body], dtype=np.int32).reshape(3, 4)[:, :2].tolist() == [[0, 0], [0, 0], [4, 0]]
    assert np.frombuffer(raw[40:body], dtype=np.int64).reshape(3, 2)[:, 1].tolist() == ln
    assert np.array_equal(np.frombuffer(raw[body:body + 48], dtype=np.uint64), off)
    assert np.array_equal(np.frombuffer(raw[body + 48:], dtype=np.uint64), occ)
    got = hostlib.occurrences_read(path)
    assert np.array_equal(got[0], off) and np.array_equal(got[1], occ) and got[2] == k and got[3].tolist() == col and got[4].tolist() == ln
    # an empty table: columns without an occurrence, and no column at all
    hostlib.occurrences_write(path, np.zeros(4, np.uint64), np.zeros(0, np.uint64), 7, [], [])
    got = hostlib.occurrences_read(path)
    assert got[0].tolist() == [0, 0, 0, 0] and len(got[1]) == 0 and got[2] == 7 and len(got[3]) == 0
    assert len(open(path, "rb").read()) == 40 + 4 * 8
    hostlib.occurrences_write(path, np.zeros(1, np.uint64), np.zeros(0, np.uint64), 7, [1], [9])
    got = hostlib.occurrences_read(path)
    assert got[0].tolist() == [0] and len(got[1]) == 0 and got[3].tolist() == [1] and got[4].tolist() == [9]

    def damaged(data, needle):
        open(path, "wb").write(bytes(data))
        with pytest.raises(RuntimeError, match=needle):
            hostlib.occurrences_read(path)

    # truncation, trailing bytes, another magic
    damaged(raw[:-3], "truncated")
    damaged(raw[:5], "truncated")
    damaged(raw[:30], "truncated")
    damaged(raw + b"\0", "after its table")
    damaged(b"SBWTPOS1" + raw[8:], "SBWTOCC1")

    def with_word(at, value):
        bad = bytearray(raw)
        bad[at:at + 8] = int(value).to_bytes(8, "little")
        return bad

    # non-monotone offsets (off[2] = 3 > off[3] = 2), a first offset that is not 0, a last one that is not n_occ
    damaged(with_word(body + 2 * 8, 3), "not monotone at column 2")
    damaged(with_word(body, 1), "off.0. is not 0")
    damaged(with_word(body + 5 * 8, 5), "is not n_occ")
    # unsorted keys within a column: equal, and descending
    damaged(with_word(body + 48 + 3 * 8, key(0, 0)), "column 3 are not sorted")
    damaged(with_word(body + 48 + 1 * 8, key(0, 1)), "column 1 are not sorted")
    # a key on a sequence that is not listed, and one whose window ends beyond its sequence
    damaged(with_word(body + 48 + 5 * 8, key(3, 0)), "sequence 3")
    damaged(with_word(body + 48 + 5 * 8, key(2, 96)), "beyond its length 100")
    damaged(with_word(body + 48 + 4 * 8, key(1, 3)), "offset 3 of sequence 1, beyond its length 7")
    # the writer refuses the same
    with pytest.raises(RuntimeError, match="sequence 2"):
        hostlib.occurrences_write(path, off, occ, k, col[:2], ln[:2])
    with pytest.raises(RuntimeError, match="not monotone"):
        hostlib.occurrences_write(path, np.array([0, 2, 1, 2, 5, 6], np.uint64), occ, k, col, ln)
    with pytest.raises(RuntimeError, match="not sorted"):
        hostlib.occurrences_write(path, off, occ[[1, 0, 2, 3, 4, 5]], k, col, ln)
    with pytest.raises(RuntimeError, match="is not n_occ"):
        hostlib.occurrences_write(path, off, occ[:5], k, col, ln)


def test_max_occ_bounds():
    """1 .. 2^20; anything else is refused, before the object is looked at"""
    L = capi.lib()
    off = np.zeros(2, dtype=np.int64)
    out = np.zeros(1, dtype=capi.READ_MAP_DTYPE)
    for bad in (0, -1, (1 << 20) + 1, 1 << 30):
        refused(L.sbwtgpu_occurrences_map_batch(None, None, off.ctypes.data, 1, 1, bad, out.ctypes.data), "max_occ", "1 .. 1048576")
        refused(L.sbwtgpu_occurrences_map_dev(None, None, 0, None, 0, 1, bad, None, None, 0, None), "max_occ", "1 .. 1048576")
    for good in (1, 1024, 1 << 20):
        refused(L.sbwtgpu_occurrences_map_batch(None, None, off.ctypes.data, 1, 1, good, out.ctypes.data), "NULL")
    import inspect
    assert inspect.signature(capi.Occurrences.map).parameters["max_occ"].default == 1024
