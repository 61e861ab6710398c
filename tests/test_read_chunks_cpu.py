"""CPU: the chunk rule of the chunked host-buffer calls (sbwt_amd/csrc/sbwt_read_chunks.h), checked by a stand-alone program
under the address and undefined-behaviour sanitizers: tests/cpp/test_read_chunks.cpp.  No GPU and no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_chunk_rule_matches_the_loop_it_replaced(tmp_path):
    exe = str(tmp_path / "test_read_chunks")
    src = os.path.join(ROOT, "tests", "cpp", "test_read_chunks.cpp")
    p = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                        "-Werror", "-o", exe, src], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "cases ok" in p.stdout and not p.stderr, p.stdout + p.stderr
