"""CPU: the frame every `sbwt` subcommand shares -- the list of commands, the usage text of each, how a bad option and an
unknown command are reported.  No GPU is opened before any of these texts, so the whole file runs in a second or two."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBWT = os.path.join(ROOT, "sbwt_amd", "bin", "sbwt")

# the order `sbwt` lists its commands in
COMMANDS = ["build", "search", "matching-statistics", "dump-unitigs", "thread", "bubbles", "set-op", "read-hits", "build-colors",
            "compress-colors", "merge-colors", "color-matrix", "color-select", "screen", "pseudoalign"]
# the option that names the (first) index, for the commands that have no --index-file
INDEX_OPTION = {"build": b"--in-file", "set-op": b"--index-a", "merge-colors": b"--index-u"}


def run(*args):
    return subprocess.run([SBWT] + list(args), capture_output=True, timeout=60)


def listed_commands():
    p = run()
    assert p.returncode == 0 and b"Available commands" in p.stderr, p.stderr
    return re.findall(r"^   \S+ (\S+)$", p.stderr.decode(), flags=re.M)


def pytest_generate_tests(metafunc):
    if "cmd" in metafunc.fixturenames:
        from sbwt_amd import build
        build.build_all(force=False)                 # (the names come from the binary itself: it has to be there)
        metafunc.parametrize("cmd", listed_commands())


def test_the_command_list_has_its_fifteen_names_in_order():
    got = listed_commands()
    assert len(got) == 15 and got == COMMANDS
    # README.md names them as `sbwt search|build|...`: the same names
    with open(os.path.join(ROOT, "README.md"), encoding="utf-8") as f:
        readme = re.search(r"`sbwt ([a-z|-]+\|[a-z|-]+)`", f.read())
    assert readme and sorted(readme.group(1).split("|")) == sorted(got)
    # and the header comment of the source has one entry per command, in that order
    with open(os.path.join(ROOT, "sbwt_amd", "csrc", "host", "sbwt_cli.cpp"), encoding="utf-8") as f:
        header = f.read().split("#include", 1)[0]
    assert re.findall(r"^//   sbwt ([a-z-]+) ", header, flags=re.M) == got


def test_no_arguments_print_the_usage_text(cmd):
    p = run(cmd)
    assert p.returncode == 1 and p.stdout == b""
    assert b"Usage:" in p.stderr and b"--help" in p.stderr
    assert INDEX_OPTION.get(cmd, b"--index-file") in p.stderr
    assert run(cmd, "--help").stderr.split(b"\n", 1)[1] == p.stderr.split(b"\n", 1)[1]      # (the first line carries the time)


def test_an_unknown_option_is_reported_without_the_usage_text(cmd):
    p = run(cmd, "--no-such-option")
    assert p.returncode == 1
    assert "Error: Option ‘no-such-option’ does not exist".encode() in p.stderr
    assert b"Usage:" not in p.stderr


def test_an_unknown_command_is_refused():
    p = run("frobnicate")
    assert p.returncode == 1 and b"Runtime error: Invalid command: frobnicate" in p.stderr
