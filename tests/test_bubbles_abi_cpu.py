"""CPU: include/sbwtgpu.h declares the sbwtgpu_bubbles_* calls and the record, capi.EXPORTED_SYMBOLS lists them, the library
exports them, and NULL handles are refused before any device is touched."""
import os
import re

from sbwt_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sbwtgpu_bubbles_create", "sbwtgpu_bubbles_info", "sbwtgpu_bubbles_dev", "sbwtgpu_bubbles_copy",
         "sbwtgpu_bubbles_in_degrees_copy", "sbwtgpu_bubbles_stats", "sbwtgpu_bubbles_destroy"]


def test_the_header_declares_and_the_library_exports_the_bubble_calls():
    text = open(os.path.join(ROOT, "include", "sbwtgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(sbwtgpu_bubbles_\w+)\s*\(", text)) == set(NAMES)
    assert "typedef struct sbwtgpu_bubbles sbwtgpu_bubbles;" in text
    assert re.search(r"#define SBWTGPU_BUBBLE_OTHER 0u\s+#define SBWTGPU_BUBBLE_SNP\s+1u", text)
    assert re.search(r"typedef struct \{ uint32_t source, branch\[2\], sink, n_kmers\[2\], kind, reserved\s*; \} sbwtgpu_bubble;", text)
    assert set(NAMES) <= set(capi.EXPORTED_SYMBOLS)
    L = capi.lib()
    for n in NAMES:
        assert hasattr(L, n), n
    for m in ("bubbles", "in_degrees"):
        assert callable(getattr(capi.Unitigs, m)), m
    for m in ("info", "records", "branch_colors", "dev_ptrs", "stats", "close", "__enter__", "__exit__"):
        assert callable(getattr(capi.Bubbles, m)), m


def test_the_record_is_32_bytes_with_the_abi_field_names():
    assert capi.BUBBLE.itemsize == 32
    assert capi.BUBBLE.names == ("source", "branch", "sink", "n_kmers", "kind", "reserved")
    assert [capi.BUBBLE.fields[n][1] for n in capi.BUBBLE.names] == [0, 4, 12, 16, 24, 28]
    assert (capi.BUBBLE_OTHER, capi.BUBBLE_SNP) == (0, 1)


def test_null_handles_are_refused_without_a_device():
    L = capi.lib()
    assert L.sbwtgpu_bubbles_create(None, None, None) == capi.ERR_INVALID_ARG and b"NULL" in L.sbwtgpu_last_error()
    assert L.sbwtgpu_bubbles_info(None, None, None, None, None) == capi.ERR_INVALID_ARG and b"NULL" in L.sbwtgpu_last_error()
    assert L.sbwtgpu_bubbles_dev(None, None, None, None) == capi.ERR_INVALID_ARG
    assert L.sbwtgpu_bubbles_copy(None, None, None, None) == capi.ERR_INVALID_ARG
    assert L.sbwtgpu_bubbles_in_degrees_copy(None, None) == capi.ERR_INVALID_ARG
    assert L.sbwtgpu_bubbles_stats(None, None) == capi.ERR_INVALID_ARG
    L.sbwtgpu_bubbles_destroy(None)
