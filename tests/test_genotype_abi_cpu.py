"""CPU: include/sbwtgpu.h declares the sbwtgpu_genotype type and its ten calls, capi.EXPORTED_SYMBOLS lists them, the library
exports them, NULL handles are refused before any device is touched, and `sbwt bubbles` knows the genotype options."""
import os
import re
import subprocess

from sbwt_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")
NAMES = ["sbwtgpu_genotype_create", "sbwtgpu_genotype_reset", "sbwtgpu_genotype_destroy", "sbwtgpu_genotype_workspace_bytes",
         "sbwtgpu_genotype_add_dev", "sbwtgpu_genotype_add_batch", "sbwtgpu_genotype_info", "sbwtgpu_genotype_branches",
         "sbwtgpu_genotype_kmer_hits_copy", "sbwtgpu_genotype_calls"]


def test_the_header_declares_and_the_library_exports_the_genotype_calls():
    text = open(os.path.join(ROOT, "include", "sbwtgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(sbwtgpu_genotype_\w+)\s*\(", text)) == set(NAMES)
    assert "typedef struct sbwtgpu_genotype sbwtgpu_genotype;" in text                # the eleventh name
    assert set(NAMES) <= set(capi.EXPORTED_SYMBOLS)
    L = capi.lib()
    for n in NAMES:
        assert hasattr(L, n), n
    assert callable(capi.Unitigs.genotype) and callable(capi.genotype_workspace_bytes)
    for m in ("add", "add_reads", "add_dev", "reset", "info", "branches", "kmer_hits", "calls", "close", "__enter__", "__exit__"):
        assert callable(getattr(capi.Genotype, m)), m


def test_the_workspace_is_the_strand_search_workspace():
    for s in (1, 2):
        sizes = [capi.genotype_workspace_bytes(b, r, s) for b in (0, 1, 1000, 10**6) for r in (0, 1, 1000)]
        assert all(x > 0 for x in sizes)
        assert sizes == [capi.screen_workspace_bytes(b, r, s) for b in (0, 1, 1000, 10**6) for r in (0, 1, 1000)]
    assert capi.genotype_workspace_bytes(10**6, 1000, 2) > capi.genotype_workspace_bytes(10**6, 1000, 1) >= capi.search_workspace_bytes(10**6)


def test_null_handles_are_refused_without_a_device():
    L = capi.lib()
    assert L.sbwtgpu_genotype_create(None, None, None, None) == capi.ERR_INVALID_ARG and b"NULL" in L.sbwtgpu_last_error()
    assert L.sbwtgpu_genotype_reset(None) == capi.ERR_INVALID_ARG and b"NULL" in L.sbwtgpu_last_error()
    assert L.sbwtgpu_genotype_add_dev(None, None, 0, None, 0, 1, None, 0, None) == capi.ERR_INVALID_ARG
    assert L.sbwtgpu_genotype_add_batch(None, None, None, 0, 1) == capi.ERR_INVALID_ARG
    assert L.sbwtgpu_genotype_info(None, None, None, None, None, None, None) == capi.ERR_INVALID_ARG
    assert L.sbwtgpu_genotype_branches(None, None, None, None) == capi.ERR_INVALID_ARG
    assert L.sbwtgpu_genotype_kmer_hits_copy(None, None, None) == capi.ERR_INVALID_ARG
    assert L.sbwtgpu_genotype_calls(None, 1_000_000, 1, None, None, None, None) == capi.ERR_INVALID_ARG and b"NULL" in L.sbwtgpu_last_error()
    L.sbwtgpu_genotype_destroy(None)
    assert L.sbwtgpu_set_tuning(b"genotype_chunk_bases", 0) == capi.OK


def run(*args):
    build.build_all(force=False)
    return subprocess.run([SBWT] + list(args), capture_output=True, timeout=60)


def test_bubbles_help_names_the_genotype_options():
    p = run("bubbles", "--help")
    assert p.returncode == 1
    for opt in (b"--query-file", b"--both-strands", b"--min-breadth", b"--min-depth", b"--refs-out"):
        assert opt in p.stderr, opt


def test_genotype_options_without_a_query_are_a_usage_error(tmp_path):
    out = str(tmp_path / "b.tsv")
    for extra in (["--both-strands"], ["--min-breadth", "0.5"], ["--min-depth", "2"], ["--refs-out", str(tmp_path / "r.tsv")]):
        p = run("bubbles", "-i", "no-such-index", "-o", out, *extra)
        assert p.returncode == 1 and b"Error: " + extra[0].encode() + b" needs a query file (-q)" in p.stderr, p.stderr
    assert not os.path.exists(out)
    p = run("bubbles", "-i", "no-such-index", "-o", out, "-q", "reads.fna", "--refs-out", str(tmp_path / "r.tsv"))
    assert p.returncode == 1 and b"--refs-out needs a colour file (-c)" in p.stderr
    for bad in ("0", "1.5", "x", "0.1234567"):
        p = run("bubbles", "-i", "no-such-index", "-o", out, "-q", "reads.fna", "--min-breadth", bad)
        assert p.returncode == 1 and b"--min-breadth must be a decimal number in (0, 1]" in p.stderr, bad
    p = run("bubbles", "-i", "no-such-index", "-o", out, "-q", "reads.fna", "--min-depth", "-1")
    assert p.returncode == 1 and b"--min-depth must be a non-negative integer" in p.stderr
