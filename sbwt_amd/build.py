"""Build driver: compiles every native piece IN-TREE (the .so files travel to the GPU box with the
snapshot; they are git-ignored).

  sbwt_amd/lib/libsbwtgpu.so   HIP kernels + C ABI (include/sbwtgpu.h), hipcc --offload-arch=gfx950
  sbwt_amd/lib/libsbwtgpu_mega12.so  the same sources with -DSBWT_MEGA_SHIFT=12: a TEST build whose mega blocks hold 4096
                               columns, so that a 250 k-column index spans 60 of them (tests/test_gpu_mega_small.py)
  sbwt_amd/lib/libsbwthost.so  GPU-free host helpers (include/sbwthost.h), g++
  sbwt_amd/bin/sbwt            the `sbwt search|build` CLI (C++ host mirror), g++ linked to libsbwtgpu.so
  oracle/liboracle.so          the CPU oracle (test infrastructure), gcc

Usage: python -m sbwt_amd.build [--force]
"""
from __future__ import annotations

import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sbwt_amd", "csrc")
HOST = os.path.join(CSRC, "host")
LIB = os.path.join(ROOT, "sbwt_amd", "lib")
BIN = os.path.join(ROOT, "sbwt_amd", "bin")
INC = os.path.join(ROOT, "include")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXX = os.environ.get("CXX", "g++")


def _newer(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd):
    print("+", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def _glob(d, exts):
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(exts)]


GPU_SRCS = [os.path.join(CSRC, f) for f in ("sbwt_search.hip", "sbwt_search_fused.hip", "sbwt_api_kernels.hip", "sbwt_derived.hip", "sbwt_build.hip", "sbwt_sort.hip",
                                              "sbwt_format.hip", "sbwt_ms.hip", "sbwt_unitigs.hip", "sbwt_setops.hip", "sbwt_readhits.hip", "sbwt_walks.hip", "sbwt_colors.hip", "sbwt_colorsets.hip", "sbwt_colormerge.hip", "sbwt_colormatrix.hip", "sbwt_colorselect.hip", "sbwt_screen.hip", "sbwt_bubbles.hip", "sbwt_genotype.hip", "sbwt_positions.hip", "sbwt_occurrences.hip", "sbwt_verify.hip", "sbwt_align.hip", "sbwt_pileup.hip", "sbwtgpu_capi.cpp", "sbwtgpu_capi_reads.cpp", "sbwtgpu_capi_colors.cpp", "sbwtgpu_capi_placement.cpp", "sbwtgpu_capi_verify.cpp", "sbwtgpu_capi_align.cpp", "sbwtgpu_capi_pileup.cpp")]
GPU_DEPS = GPU_SRCS + [os.path.join(CSRC, f) for f in ("sbwt_device.h", "sbwt_kernels_common.h", "sbwt_scan.h", "sbwt_ms.h", "sbwt_unitigs.h", "sbwt_colwalk.h", "sbwt_setops.h", "sbwt_readhits.h", "sbwt_walks.h", "sbwt_colors.h", "sbwt_colorsets.h", "sbwt_colormerge.h", "sbwt_colormatrix.h", "sbwt_colorselect.h", "sbwt_screen.h", "sbwt_bubbles.h", "sbwt_genotype.h", "sbwt_positions.h", "sbwt_posmap.h", "sbwt_occurrences.h", "sbwt_verify.h", "sbwt_verify_text.h", "sbwt_align.h", "sbwt_pileup.h", "sbwt_search_fused_loop.inc", "sbwtgpu_internal.h", "sbwt_read_chunks.h")] + \
    [os.path.join(INC, "sbwtgpu.h")]
MEGA_TEST_SHIFT = 12
MEGA_TEST_LIB = os.path.join(LIB, "libsbwtgpu_mega%d.so" % MEGA_TEST_SHIFT)


def _hipcc_cmd(out, defines=()):
    return [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared"] + list(defines) + ["-o", out] + GPU_SRCS + ["-ldl"]


def build_gpu(force=False) -> str:
    os.makedirs(LIB, exist_ok=True)
    out = os.path.join(LIB, "libsbwtgpu.so")
    if force or _newer(out, GPU_DEPS):
        _run(_hipcc_cmd(out))
    return out


def start_gpu_mega_test(force=False):
    """Starts the compiler for the test library when it is missing or older than a source (the rule of build_gpu) and returns
    the process, or None: build_all lets it run beside the product library's compiler (two hipcc jobs in all)."""
    os.makedirs(LIB, exist_ok=True)
    if not (force or _newer(MEGA_TEST_LIB, GPU_DEPS)):
        return None
    cmd = _hipcc_cmd(MEGA_TEST_LIB, ["-DSBWT_MEGA_SHIFT=%d" % MEGA_TEST_SHIFT])
    print("+", " ".join(cmd), flush=True)
    return subprocess.Popen(cmd)


def finish_gpu_mega_test(proc) -> str:
    if proc is not None and proc.wait() != 0:
        raise subprocess.CalledProcessError(proc.returncode, proc.args)
    return MEGA_TEST_LIB


def build_gpu_mega_test(force=False) -> str:
    """libsbwtgpu_mega12.so: libsbwtgpu.so's sources with mega blocks of 2^12 columns instead of 2^31 (sbwt_device.h).  Test
    infrastructure: loaded only through SBWTGPU_LIB, by the worker of tests/test_gpu_mega_small.py."""
    return finish_gpu_mega_test(start_gpu_mega_test(force))


def build_host(force=False) -> str:
    os.makedirs(LIB, exist_ok=True)
    out = os.path.join(LIB, "libsbwthost.so")
    src = os.path.join(HOST, "host_capi.cpp")
    deps = [src, os.path.join(INC, "sbwthost.h")] + _glob(HOST, (".hh",))
    if force or _newer(out, deps):
        _run([CXX, "-O3", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wall", "-o", out, src, "-lz"])
    return out


def build_cli(force=False) -> str:
    os.makedirs(BIN, exist_ok=True)
    out = os.path.join(BIN, "sbwt")
    src = os.path.join(HOST, "sbwt_cli.cpp")
    deps = [src, os.path.join(INC, "sbwtgpu.h"), os.path.join(INC, "sbwthost.h"), os.path.join(LIB, "libsbwtgpu.so"),
            os.path.join(LIB, "libsbwthost.so")] + _glob(HOST, (".hh",))
    if force or _newer(out, deps):
        _run([CXX, "-O3", "-std=c++17", "-pthread", "-Wall", "-o", out, src, "-L" + LIB, "-lsbwtgpu", "-lsbwthost", "-lz",
              "-Wl,-rpath,$ORIGIN/../lib", "-Wl,-rpath,/opt/rocm/lib"])
    return out


def build_oracle(force=False) -> str:
    d = os.path.join(ROOT, "oracle")
    if force:
        subprocess.call(["make", "-C", d, "clean"], stdout=subprocess.DEVNULL)
    _run(["make", "-C", d, "liboracle.so"])
    return os.path.join(d, "liboracle.so")


def build_all(force=False):
    mega = start_gpu_mega_test(force)
    try:
        built = [build_gpu(force), build_host(force), build_cli(force), build_oracle(force)]
    except BaseException:
        if mega is not None:
            mega.kill()
            mega.wait()
        raise
    return built + [finish_gpu_mega_test(mega)]


if __name__ == "__main__":
    build_all("--force" in sys.argv)
    print("build ok")
