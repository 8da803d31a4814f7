"""LtmBlock (csrc/ltm_block.h), the resident blocks a rule keeps beside its eigenvalue planes, checked without a device:
tests/c/ltm_block_main.cpp supplies dev_alloc / dev_free itself (malloc / free, a table of live blocks, an allocation that
fails on demand) and exits 0 only if every check held, no block is live at the end and no unknown or repeated free was seen."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "autobzcore.jl_amd", "csrc")


def _build_and_run(tmp_path, name, extra):
    """g++ -std=c++17 -Wall -Wextra -Werror on the stand-alone program: the headers need nothing of HIP."""
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", *extra, os.path.join(ROOT, "tests", "c", "ltm_block_main.cpp"),
           "-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ltm_block: ok" in run.stdout
    return run


def test_ltm_block_tiles_replaces_and_drops(tmp_path):
    _build_and_run(tmp_path, "ltm_block_main", [])


def test_ltm_block_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same program, stand-alone, with ASan (leaks included) and UBSan: any report aborts it with a non-zero status."""
    run = _build_and_run(tmp_path, "ltm_block_main_san",
                         ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr


def _includes(header):
    with open(os.path.join(CSRC, header)) as f:
        return [ln.strip() for ln in f if ln.lstrip().startswith("#include")]


def test_ltm_block_headers_include_nothing_of_hip():
    assert _includes("plane_view.h") == ["#include <cstdint>"]
    assert _includes("ltm_block.h") == ['#include "dev_buf.h"', '#include "plane_view.h"']
    # ... and the internal header takes PlaneView and the block type from them, not from a definition of its own
    internal = _includes("abz_internal.h")
    assert '#include "plane_view.h"' in internal and '#include "ltm_block.h"' in internal
    with open(os.path.join(CSRC, "abz_internal.h")) as f:
        assert "struct PlaneView {" not in f.read()
