"""CPU: the test build of the GPU library with small mega blocks (sbwt_amd/build.py, tests/test_gpu_mega_small.py) is built
beside the product library, exports the whole C ABI and says in its version string which build it is; the product library's
version string stays as it was."""
import os
import subprocess
import sys

from sbwt_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = ("import sys; sys.path.insert(0, %r); from sbwt_amd import capi; L = capi.lib(); "
         "[getattr(L, s) for s in capi.EXPORTED_SYMBOLS]; print(capi.LIB_PATH); print(L.sbwtgpu_version().decode())" % ROOT)


def version_in_child(lib_path):
    """(path loaded, version string) of a fresh process: capi binds one library per process, named by SBWTGPU_LIB."""
    env = {key: val for key, val in os.environ.items() if key != "SBWTGPU_LIB"}
    if lib_path:
        env["SBWTGPU_LIB"] = lib_path
    p = subprocess.run([sys.executable, "-c", PROBE], env=env, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    path, version = p.stdout.decode().splitlines()[-2:]
    return path, version


def test_test_build_exists_exports_the_abi_and_names_itself():
    lib = build.MEGA_TEST_LIB
    assert os.path.basename(lib) == "libsbwtgpu_mega12.so"
    assert os.path.exists(lib), "%s is missing: build it with `python -m sbwt_amd.build`" % lib
    path, version = version_in_child(lib)
    assert path == lib and version.endswith(" mega_shift=%d" % build.MEGA_TEST_SHIFT), (path, version)


def test_product_build_carries_no_marker():
    path, version = version_in_child(None)
    assert path == os.path.join(ROOT, "sbwt_amd", "lib", "libsbwtgpu.so")
    assert version == "sbwtgpu 0.1 (gfx950)"
    assert capi.lib().sbwtgpu_version().decode() == version
