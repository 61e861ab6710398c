"""CPU: the verification layer's surface without a device -- the header declares the names and the library exports them, the
16-byte record and its dtype, NULL handles are refused before anything touches a GPU, create without a device says so, the
workspace arithmetic, the tuning key's bounds, and read-hits names its new options and refuses their misuse."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from sbwt_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")
NAMES = ["sbwtgpu_refseqs_create", "sbwtgpu_refseqs_destroy", "sbwtgpu_refseqs_add_batch", "sbwtgpu_refseqs_info",
         "sbwtgpu_refseqs_lengths_copy", "sbwtgpu_refseqs_get", "sbwtgpu_refseqs_verify_workspace_bytes", "sbwtgpu_refseqs_verify_dev",
         "sbwtgpu_refseqs_verify_batch"]


def header():
    return open(os.path.join(ROOT, "include", "sbwtgpu.h")).read()


def test_the_header_declares_the_names_and_the_library_exports_them():
    full = header()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert sorted(set(re.findall(r"\b(sbwtgpu_refseqs_\w+)\s*\(", text))) == sorted(NAMES)
    L = capi.lib()
    for n in NAMES:
        assert hasattr(L, n) and n in capi.EXPORTED_SYMBOLS, n
    assert "typedef struct sbwtgpu_refseqs sbwtgpu_refseqs;" in text
    assert "typedef struct { int64_t ref_end; int32_t mismatches; int32_t edit; } sbwtgpu_read_verify;" in text
    m = re.search(r"#define\s+SBWTGPU_VERIFY_MAX_BAND\s+(\d+)\b", text)
    assert m and int(m.group(1)) == capi.VERIFY_MAX_BAND == 256
    m = re.search(r"#define\s+SBWTGPU_VERIFY_MAX_READ\s+(\d+)\b", text)
    assert m and int(m.group(1)) == capi.VERIFY_MAX_READ == 1024
    # the definitions stand in the header, under their heading
    for phrase in ("reference sequences and verification", "matches nothing, not even itself", "2 bits per base, 32 bases per uint64",
                   "One validity bit per base, 64 per uint64", "no two sequences share a word", "0.375 bytes per base",
                   "MUST NOT RUN CONCURRENTLY WITH AN ADD", "an invalid byte stays invalid",
                   "D[0][t] = 0 for t = 0 ... L + 2B, D[i][0] = i, and edit = min_t D[L][t]", "The empty substring is included",
                   "smallest exclusive end coordinate start - B + t", "The path is not band-limited", "The unverified record is {0, -1, -1}",
                   "|start| >= 2^40", "L = 0 gives {start - B, 0, 0}", "edit <= mismatches for every B", "edit is non-increasing in B",
                   "never synchronises and never allocates", "ONE LANE", "verify_fast_bases", "SBWTGPU_ERR_READ_TOO_LONG"):
        assert phrase in full, phrase


def test_the_record_is_16_bytes():
    d = capi.READ_VERIFY_DTYPE
    assert d.itemsize == 16 and d.names == ("ref_end", "mismatches", "edit")
    assert [d.fields[n][1] for n in d.names] == [0, 8, 12]
    assert [d.fields[n][0] for n in d.names] == [np.dtype(np.int64), np.dtype(np.int32), np.dtype(np.int32)]
    assert capi.READ_MAP_DTYPE.itemsize == 32 and capi.READ_MAP_DTYPE.fields["start"][1] == 0


def refused(rc, *needles):
    assert rc == capi.ERR_INVALID_ARG
    msg = capi.lib().sbwtgpu_last_error().decode()
    for s in needles:
        assert s in msg, (s, msg)


def test_null_handles_are_refused_without_a_device():
    L = capi.lib()
    off = np.zeros(2, dtype=np.int64)
    rec = np.zeros(1, dtype=capi.READ_MAP_DTYPE)
    out = np.zeros(1, dtype=capi.READ_VERIFY_DTYPE)
    refused(L.sbwtgpu_refseqs_create(0, None), "refseqs", "NULL")
    refused(L.sbwtgpu_refseqs_add_batch(None, 0, None, off.ctypes.data, 1), "refseqs", "NULL")
    refused(L.sbwtgpu_refseqs_info(None, None, None, None, None), "refseqs", "NULL")
    refused(L.sbwtgpu_refseqs_lengths_copy(None, off.ctypes.data), "refseqs", "NULL")
    refused(L.sbwtgpu_refseqs_get(None, 0, 0, 1, off.ctypes.data), "refseqs", "NULL")
    refused(L.sbwtgpu_refseqs_verify_batch(None, None, off.ctypes.data, 1, rec.ctypes.data, 8, out.ctypes.data), "refseqs", "NULL")
    refused(L.sbwtgpu_refseqs_verify_dev(None, None, 0, None, 0, None, 8, None, None, 0, None), "refseqs", "NULL")
    L.sbwtgpu_refseqs_destroy(None)


def test_create_without_a_device_says_so():
    # with a device this is a no-op: tests/test_gpu_verify.py creates objects there
    if capi.device_count() > 0:
        return
    with pytest.raises(capi.SbwtGpuError) as ei:
        capi.RefSeqs.create()
    assert ei.value.code == capi.ERR_NO_DEVICE


def test_workspace_bytes_and_the_tuning_key():
    W = capi.RefSeqs.workspace_bytes
    sizes = [(0, 0), (0, 1), (100, 1), (100, 7), (1 << 20, 1000), (1 << 24, 1 << 17), (1 << 28, 1 << 21), (1 << 35, (1 << 31) - 1)]
    for nb, nr in sizes:
        w = W(nb, nr)
        assert w % 256 == 0 and w >= 256 + 4 * nr             # the header and 4 bytes per read
        for nb2, nr2 in sizes:                                  # non-decreasing in both arguments
            if nb2 >= nb and nr2 >= nr:
                assert W(nb2, nr2) >= w
    assert W(-5, -5) == W(0, 0)
    for v in (0, 1, 64, 65, 128, 256):
        capi.set_tuning("verify_fast_bases", v)
    capi.set_tuning("verify_fast_bases", 0)
    for v in (-1, 257, 1 << 20):
        with pytest.raises(capi.SbwtGpuError) as ei:
            capi.set_tuning("verify_fast_bases", v)
        assert ei.value.code == capi.ERR_INVALID_ARG and "verify_fast_bases" in ei.value.msg


def test_read_hits_names_its_new_options():
    p = subprocess.run([SBWT, "read-hits", "--help"], capture_output=True, timeout=60)
    for needle in (b"--refs", b"--band", b"mismatches edit ref_end", b"build-colors -r", b"The default is 8", b"0 .. 256",
                   b"With --positions or --occurrences", b"With --refs", b"-1 -1 0"):
        assert needle in p.stderr, needle


def test_read_hits_refuses_refs_and_band_by_name(tmp_path):
    """the refusals that need no device: they come before the index is loaded"""
    idx, q, refs = tmp_path / "x.sbwt", tmp_path / "q.fna", tmp_path / "refs.txt"
    idx.write_bytes(b"not an index")
    q.write_text(">r\nACGT\n")
    refs.write_text(str(q) + "\n")
    base = [SBWT, "read-hits", "-i", str(idx), "-q", str(q), "-o", str(tmp_path / "out.txt")]

    def fails(extra, *needles):
        p = subprocess.run(base + extra, capture_output=True, timeout=60)
        assert p.returncode != 0
        for s in needles:
            assert s in p.stderr, (s, p.stderr)

    fails(["--refs", str(refs)], b"--refs needs --positions or --occurrences")
    fails(["--band", "4"], b"--band needs --refs")
    fails(["--band", "4", "--positions", str(idx)], b"--band needs --refs")
    for bad in ("-1", "257", "x", "3x"):
        fails(["--positions", str(idx), "--refs", str(refs), "--band=" + bad], b"--band must be a number in 0 .. 256")
    fails(["--positions", str(idx), "--refs", str(tmp_path / "none.txt")], b"none.txt")
