"""CPU: the alignment layer's surface without a device -- the header declares the names and the library exports them, the
16-byte record and its dtype, the definitions stand in the header, NULL handles are refused before anything touches a GPU, the
workspace arithmetic, the tuning key's bounds, cigar_string, and read-hits names --cigar and refuses its misuse."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from sbwt_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")
NAMES = ["sbwtgpu_align_workspace_bytes", "sbwtgpu_align_dev", "sbwtgpu_align_batch"]


def header():
    return open(os.path.join(ROOT, "include", "sbwtgpu.h")).read()


def test_the_header_declares_the_names_and_the_library_exports_them():
    full = header()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert sorted(set(re.findall(r"\b(sbwtgpu_align_\w+)\s*\(", text))) == sorted(NAMES)
    L = capi.lib()
    for n in NAMES:
        assert hasattr(L, n) and n in capi.EXPORTED_SYMBOLS, n
    assert "typedef struct { int64_t ref_begin; int32_t n_ops; int32_t n_eq; } sbwtgpu_read_align;" in text
    assert re.search(r"int\s+sbwtgpu_align_dev\(const sbwtgpu_refseqs \*r, const char \*d_bases, int64_t total_bases, const int64_t \*d_read_off, "
                     r"int64_t n_reads,\s+const sbwtgpu_read_map \*d_map, int band, sbwtgpu_read_verify \*d_verify_out, sbwtgpu_read_align \*d_out,"
                     r"\s+int64_t \*d_op_off\s+, uint32_t \*d_ops, int64_t ops_cap,\s+void \*d_workspace, int64_t workspace_bytes, void \*stream\);", text)
    assert re.search(r"int\s+sbwtgpu_align_batch\(const sbwtgpu_refseqs \*r, const char \*bases, const int64_t \*read_off, int64_t n_reads, "
                     r"const sbwtgpu_read_map \*map,\s+int band, sbwtgpu_read_verify \*verify_out, sbwtgpu_read_align \*out, int64_t \*op_off, "
                     r"uint32_t \*\*ops_out, int64_t \*n_ops\);", text)


def test_the_definitions_stand_in_the_header():
    full = header()
    at = full.index("alignment of mapped reads (DESIGN.md section 29)")
    assert at > full.index("reference sequences and verification (DESIGN.md section 28)")
    sec = " ".join(full[at:].replace(" * ", " ").replace(" *\n", "\n").split())
    for phrase in ("Column t >= 1 of D stands for reference coordinate start - B + t - 1", "Let tE = ref_end - (start - B)",
                   "walking back from (i, t) = (L, tE) until i = 0", "take the FIRST step that applies",
                   "Applies if t > 0 and D[i-1][t-1] + c == D[i][t]", "Emit = when c = 0 and X when c = 1", "Applies if D[i-1][t] + 1 == D[i][t]",
                   "read base r[i-1] faces nothing", "Otherwise t > 0 and D[i][t-1] + 1 == D[i][t]", "a reference coordinate faces nothing",
                   "When i = 0, ref_begin = start - B + t", "reversed into read order, and equal neighbours are merged into runs",
                   "length << 4 | code, with I = 1, D = 2, = = 7, X = 8", "It can only be X or D", "ref_begin may be negative",
                   "sbwtgpu_read_align is 16 bytes: int64 ref_begin; int32 n_ops; int32 n_eq", "gives {0, 0, 0} and no runs",
                   "L = 0 gives {start - B, 0, 0}", "n_ops = 0 holds in no other case", "#= + #X + #I = L", "#= + #X + #D = ref_end - ref_begin",
                   "#X + #I + #D = edit", "The first and the last run are never D", "tE is the smallest minimiser", "n_ops <= 2 edit + 1",
                   "No two neighbouring runs have the same code", "edit = 0 gives the single run L= and ref_begin = ref_end - L",
                   "ref_begin >= start - B", "(rc(read), 1 - strand) gives the same alignment as (read, strand)",
                   "The alignment does not depend on neighbouring sequences", "The band lemma", "|d - (tE - L)| <= edit",
                   "takes exactly the same steps as the walk over the full table", "lies on an optimal path to (L, tE)",
                   "has at most edit indels, so it cannot leave the band", "has a banded value at least as large, so it fails there too",
                   "2 edit + 1 cells per row, not the window", "exactly what sbwtgpu_refseqs_verify_dev writes for the same input",
                   "d_op_off[n_reads] always receives the true total", "nothing is written at or beyond d_ops[ops_cap]",
                   "never synchronises and never allocates", "device scan", "ONE LANE", "align_fast_edit", "sbwtgpu_free_host",
                   "must not run during an add", "ops_cap < 0"):
        assert phrase in sec, phrase
    # what the verify section says is still not built
    ver = " ".join(full[full.index("reference sequences and verification (DESIGN.md section 28)"):at].replace(" * ", " ").split())
    assert "Not built: the runner-up's verification" in ver and "a reference file format" in ver and "SAM/PAF files, clipping of overhangs" in ver
    assert "a reverse pass" not in ver


def test_the_record_is_16_bytes():
    d = capi.READ_ALIGN_DTYPE
    assert d.itemsize == 16 and d.names == ("ref_begin", "n_ops", "n_eq")
    assert [d.fields[n][1] for n in d.names] == [0, 8, 12]
    assert [d.fields[n][0] for n in d.names] == [np.dtype(np.int64), np.dtype(np.int32), np.dtype(np.int32)]


def test_cigar_string():
    assert capi.cigar_string(np.array([(57 << 4) | 7, (1 << 4) | 8, (92 << 4) | 7], np.uint32)) == "57=1X92="
    assert capi.cigar_string([(80 << 4) | 7, (2 << 4) | 2, (70 << 4) | 7]) == "80=2D70="
    assert capi.cigar_string([(3 << 4) | 1]) == "3I"
    assert capi.cigar_string(np.zeros(0, np.uint32)) == "*" and capi.cigar_string([]) == "*"


def refused(rc, *needles):
    assert rc == capi.ERR_INVALID_ARG
    msg = capi.lib().sbwtgpu_last_error().decode()
    for s in needles:
        assert s in msg, (s, msg)


def test_null_handles_are_refused_without_a_device():
    L = capi.lib()
    off = np.zeros(2, dtype=np.int64)
    rec = np.zeros(1, dtype=capi.READ_MAP_DTYPE)
    ver = np.zeros(1, dtype=capi.READ_VERIFY_DTYPE)
    out = np.zeros(1, dtype=capi.READ_ALIGN_DTYPE)
    p, n = C.c_void_p(), C.c_int64()
    refused(L.sbwtgpu_align_batch(None, None, off.ctypes.data, 1, rec.ctypes.data, 8, ver.ctypes.data, out.ctypes.data, off.ctypes.data,
                                  C.byref(p), C.byref(n)), "refseqs", "NULL")
    refused(L.sbwtgpu_align_dev(None, None, 0, None, 0, None, 8, None, None, None, None, 0, None, 0, None), "refseqs", "NULL")


def test_workspace_bytes_and_the_tuning_key():
    W, V = capi.RefSeqs.align_workspace_bytes, capi.RefSeqs.workspace_bytes
    sizes = [(0, 0), (0, 1), (100, 1), (100, 7), (100, 64), (100, 65), (1 << 20, 1000), (1 << 24, 1 << 17), (1 << 28, 1 << 21),
             (1 << 35, (1 << 31) - 1)]
    for nb, nr in sizes:
        w = W(nb, nr)
        assert w % 256 == 0 and w >= V(nb, nr) + 256 + 12 * nr      # the verify workspace first, a header, 12 bytes per read
        for nb2, nr2 in sizes:                                      # non-decreasing in both arguments
            if nb2 >= nb and nr2 >= nr:
                assert W(nb2, nr2) >= w
    assert W(-5, -5) == W(0, 0)
    # the waves' scratch is a fixed grid's: it stops growing, and nothing grows with the bases
    assert W(1 << 35, 1000) == W(0, 1000)
    for nr in (1 << 17, 1 << 21, 1 << 30):
        assert W(0, nr) - V(0, nr) - 12 * nr < 300 << 20
    for v in (0, 1, 2, 7, 30, 31):
        capi.set_tuning("align_fast_edit", v)
    capi.set_tuning("align_fast_edit", 0)
    for v in (-1, 32, 64, 1 << 20):
        with pytest.raises(capi.SbwtGpuError) as ei:
            capi.set_tuning("align_fast_edit", v)
        assert ei.value.code == capi.ERR_INVALID_ARG and "align_fast_edit" in ei.value.msg


def test_read_hits_names_cigar():
    p = subprocess.run([SBWT, "read-hits", "--help"], capture_output=True, timeout=60)
    for needle in (b"--cigar", b"With --refs", b"ref_begin cigar", b"= X I D", b"0 *", b"mismatches edit ref_end"):
        assert needle in p.stderr, needle


def test_read_hits_refuses_cigar_without_refs(tmp_path):
    """the refusals that need no device: they come before the index is loaded"""
    idx, q = tmp_path / "x.sbwt", tmp_path / "q.fna"
    idx.write_bytes(b"not an index")
    q.write_text(">r\nACGT\n")
    base = [SBWT, "read-hits", "-i", str(idx), "-q", str(q), "-o", str(tmp_path / "out.txt")]
    for extra in (["--cigar"], ["--cigar", "--positions", str(idx)], ["--cigar", "--occurrences", str(idx)]):
        p = subprocess.run(base + extra, capture_output=True, timeout=60)
        assert p.returncode != 0 and b"--cigar needs --refs" in p.stderr, p.stderr
    p = subprocess.run(base + ["--cigar", "--band", "3"], capture_output=True, timeout=60)
    assert p.returncode != 0 and (b"--band needs --refs" in p.stderr or b"--cigar needs --refs" in p.stderr)
