"""CPU: include/sbwtgpu.h declares the sbwtgpu_screen_* calls, capi.EXPORTED_SYMBOLS lists them, the library exports them, and
the workspace size is a pure function that behaves (no device)."""
import os
import re

from sbwt_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sbwtgpu_screen_create", "sbwtgpu_screen_reset", "sbwtgpu_screen_destroy", "sbwtgpu_screen_workspace_bytes",
         "sbwtgpu_screen_add_dev", "sbwtgpu_screen_add_batch", "sbwtgpu_screen_info", "sbwtgpu_screen_sets", "sbwtgpu_screen_colors",
         "sbwtgpu_screen_seen_dev", "sbwtgpu_screen_seen_copy"]


def test_the_header_declares_and_the_library_exports_the_screen_calls():
    text = open(os.path.join(ROOT, "include", "sbwtgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sbwtgpu_screen_\w+)\s*\(", text))
    assert declared == set(NAMES)
    assert "typedef struct sbwtgpu_screen sbwtgpu_screen;" in text
    assert set(NAMES) <= set(capi.EXPORTED_SYMBOLS)
    L = capi.lib()
    for n in NAMES:
        assert hasattr(L, n), n
    assert hasattr(capi.ColorSets, "screen")
    for m in ("add", "add_dev", "info", "sets", "colors", "seen", "reset", "close"):
        assert callable(getattr(capi.Screen, m)), m


def test_the_workspace_size_is_monotone_and_holds_the_search_workspace():
    bases = [0, 1, 29, 30, 1000, 1 << 20, (1 << 25) + 1, 1 << 30, 3 << 30]
    reads = [0, 1, 7, 1000, 1 << 20, (1 << 31) - 1]
    for strands in (1, 2):
        grid = [[capi.screen_workspace_bytes(b, r, strands) for r in reads] for b in bases]
        for i, row in enumerate(grid):
            assert row == sorted(row), (strands, bases[i])
            assert all(x % 256 == 0 and x >= capi.search_workspace_bytes(bases[i]) for x in row)
        for j in range(len(reads)):
            col = [row[j] for row in grid]
            assert col == sorted(col), (strands, reads[j])
    assert capi.screen_workspace_bytes(10**6, 10**4, 2) > capi.screen_workspace_bytes(10**6, 10**4, 1)
    assert capi.screen_workspace_bytes(-5, -5, 1) == capi.screen_workspace_bytes(0, 0, 1)


def test_null_handles_are_refused_without_a_device():
    L = capi.lib()
    assert L.sbwtgpu_screen_create(None, None) == capi.ERR_INVALID_ARG and b"NULL" in L.sbwtgpu_last_error()
    assert L.sbwtgpu_screen_info(None, None, None, None, None, None) == capi.ERR_INVALID_ARG and b"NULL" in L.sbwtgpu_last_error()
    assert L.sbwtgpu_screen_add_batch(None, None, None, 0, 1) == capi.ERR_INVALID_ARG
    assert L.sbwtgpu_screen_seen_dev(None, None) == capi.ERR_INVALID_ARG
    L.sbwtgpu_screen_destroy(None)
