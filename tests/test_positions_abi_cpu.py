"""CPU: the position layer's surface without a device -- the header declares the names and the libraries export them, NULL
handles are refused before anything touches a GPU, the record is 32 bytes, the two subcommands name their new options, and
the position file round-trips through the host library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from sbwt_amd import capi, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")
NAMES = ["sbwtgpu_positions_create", "sbwtgpu_positions_upload", "sbwtgpu_positions_reset", "sbwtgpu_positions_destroy",
         "sbwtgpu_positions_add_batch", "sbwtgpu_positions_info", "sbwtgpu_positions_first_copy", "sbwtgpu_positions_first_dev",
         "sbwtgpu_positions_map_workspace_bytes", "sbwtgpu_positions_map_dev", "sbwtgpu_positions_map_batch"]


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_the_header_declares_the_names_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", header("sbwtgpu.h"), flags=re.S)
    declared = sorted(set(re.findall(r"\b(sbwtgpu_positions_\w+)\s*\(", text)))
    assert declared == sorted(NAMES)
    L = capi.lib()
    for n in NAMES:
        assert hasattr(L, n) and n in capi.EXPORTED_SYMBOLS, n
    assert "typedef struct sbwtgpu_positions sbwtgpu_positions;" in text
    assert re.search(r"#define\s+SBWTGPU_POSITIONS_MAP_TABLE\s+256\b", text) and capi.POSITIONS_MAP_TABLE == 256
    # the definitions stand in the header: the key, the vote and the record's empty form
    full = header("sbwtgpu.h")
    for phrase in ("(seq << 32) | (pos << 1) | 0", "o = s XOR t", "start = pos - (W - 1 - i) if o = 1", "{0, -1, 0, 0, 0, n_found, 0}",
                   "not an enumeration of all"):
        assert phrase in full, phrase
    for n in ("sbwthost_positions_write", "sbwthost_positions_read"):
        assert hasattr(hostlib.lib(), n) and n in hostlib.EXPORTED_SYMBOLS and n in header("sbwthost.h")


def test_the_record_is_32_bytes():
    class ReadMap(C.Structure):
        _fields_ = [("start", C.c_int64), ("seq", C.c_int32), ("strand", C.c_int32), ("votes", C.c_int32), ("votes2", C.c_int32),
                    ("n_found", C.c_int32), ("n_anchored", C.c_int32)]

    assert C.sizeof(ReadMap) == 32 == capi.READ_MAP_DTYPE.itemsize
    assert [capi.READ_MAP_DTYPE.fields[n][1] for n, _ in ReadMap._fields_] == [getattr(ReadMap, n).offset for n, _ in ReadMap._fields_]
    m = re.search(r"typedef struct \{([^}]*)\} sbwtgpu_read_map;", header("sbwtgpu.h"))
    assert m and re.findall(r"(int\d+_t) (\w+);", m.group(1)) == [
        ("int64_t", "start"), ("int32_t", "seq"), ("int32_t", "strand"), ("int32_t", "votes"), ("int32_t", "votes2"),
        ("int32_t", "n_found"), ("int32_t", "n_anchored")]


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
    refused(L.sbwtgpu_positions_create(None, C.byref(h)), "positions", "NULL")
    refused(L.sbwtgpu_positions_upload(None, off.ctypes.data, C.byref(h)), "positions", "NULL")
    refused(L.sbwtgpu_positions_reset(None), "positions", "NULL")
    refused(L.sbwtgpu_positions_add_batch(None, 0, None, off.ctypes.data, 1, 1, None, None), "positions", "NULL")
    refused(L.sbwtgpu_positions_info(None, None, None, None, None, None, None), "positions", "NULL")
    refused(L.sbwtgpu_positions_first_copy(None, off.ctypes.data), "positions", "NULL")
    refused(L.sbwtgpu_positions_first_dev(None, C.byref(h)), "positions", "NULL")
    refused(L.sbwtgpu_positions_map_batch(None, None, off.ctypes.data, 1, 1, out.ctypes.data), "positions", "NULL")
    refused(L.sbwtgpu_positions_map_dev(None, None, 0, None, 0, 1, None, None, 0, None), "positions", "NULL")
    L.sbwtgpu_positions_destroy(None)
    assert h.value is None


def test_workspace_bytes_and_the_tuning_keys():
    W = capi.Positions.workspace_bytes
    prev = -1
    for nb, nr in ((0, 0), (0, 1), (100, 1), (100, 7), (1 << 20, 1000), (1 << 24, 1 << 17), (1 << 28, 1 << 21)):
        for strands in (1, 2):
            w = W(nb, nr, strands)
            # the search and its results in front, the map header and 4 bytes per read behind them
            assert w % 256 == 0 and w >= capi.pseudoalign_workspace_bytes(nb, nr, strands == 2) + 256 + 4 * nr
        assert W(nb, nr, 1) >= prev and W(nb, nr, 2) >= W(nb, nr, 1)
        prev = W(nb, nr, 1)
    assert W(-5, -5, 1) == W(0, 0, 1)
    for v in (0, 1, 4, 256):
        capi.set_tuning("positions_map_table", v)
    capi.set_tuning("positions_map_table", 0)
    for v in (-1, 257):
        with pytest.raises(capi.SbwtGpuError) as ei:
            capi.set_tuning("positions_map_table", v)
        assert ei.value.code == capi.ERR_INVALID_ARG and "positions_map_table" in ei.value.msg
    capi.set_tuning("positions_chunk_bases", 1)
    capi.set_tuning("positions_chunk_bases", 0)


def test_the_subcommands_name_their_new_options():
    p = subprocess.run([SBWT, "build-colors", "--help"], capture_output=True, timeout=60)
    assert b"--positions-out" in p.stderr and b"position file" in p.stderr
    p = subprocess.run([SBWT, "read-hits", "--help"], capture_output=True, timeout=60)
    assert b"--positions" in p.stderr and b"seq strand start votes votes2 n_anchored" in p.stderr


def test_position_file_round_trip_and_refusals(tmp_path):
    path = str(tmp_path / "x.pos")
    none = np.uint64(capi.POS_NONE)
    first = np.array([none, (1 << 32) | 7, 0, (2 << 32) | (5 << 1), none], dtype=np.uint64)
    hostlib.positions_write(path, first, 31, [0, 0, 4], [100, 7, 1 << 33])
    raw = open(path, "rb").read()
    assert raw[:8] == b"SBWTPOS1" and len(raw) == 32 + 3 * 16 + 5 * 8
    assert np.frombuffer(raw[8:32], dtype=np.int64).tolist() == [5, 31, 3]
    assert np.frombuffer(raw[32:80], dtype=np.int32).reshape(3, 4)[:, :2].tolist() == [[0, 0], [0, 0], [4, 0]]
    assert np.frombuffer(raw[32:80], dtype=np.int64).reshape(3, 2)[:, 1].tolist() == [100, 7, 1 << 33]
    assert np.array_equal(np.frombuffer(raw[80:], dtype=np.uint64), first)
    got = hostlib.positions_read(path)
    assert np.array_equal(got[0], first) and got[1] == 31 and got[2].tolist() == [0, 0, 4] and got[3].tolist() == [100, 7, 1 << 33]
    # an empty table
    hostlib.positions_write(path, np.zeros(0, np.uint64), 5, [], [])
    got = hostlib.positions_read(path)
    assert len(got[0]) == 0 and got[1] == 5 and len(got[2]) == 0
    # refusals: a position on a sequence that is not listed; truncation, trailing bytes, another magic
    with pytest.raises(RuntimeError, match="sequence 2"):
        hostlib.positions_write(path, first, 31, [0, 0], [100, 7])
    for damaged, needle in ((raw[:-3], "truncated"), (raw + b"\0", "after its table"), (b"SBWTCOL1" + raw[8:], "SBWTPOS1"), (raw[:5], "truncated")):
        open(path, "wb").write(damaged)
        with pytest.raises(RuntimeError, match=needle):
            hostlib.positions_read(path)
    bad = bytearray(raw)
    bad[80 + 8 + 4] = 3                     # column 1 now lies on sequence 3 of 3
    open(path, "wb").write(bytes(bad))
    with pytest.raises(RuntimeError, match="sequence 3"):
        hostlib.positions_read(path)
