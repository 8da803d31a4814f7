"""DevBuf (csrc/dev_buf.h), the owner of every device block, checked without a device: tests/c/devbuf_main.cpp supplies
dev_alloc / dev_free itself (malloc / free, a table of live blocks, an allocation that fails on demand) and exits 0 only if
every check held, no block is live at the end and no unknown or repeated free was seen."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_devbuf_program(tmp_path):
    """g++ -std=c++17 -Wall -Wextra -Werror on the stand-alone program: the header needs nothing of HIP."""
    exe = tmp_path / "devbuf_main"
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", os.path.join(ROOT, "tests", "c", "devbuf_main.cpp"),
           "-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def test_devbuf_owns_moves_and_frees_on_every_exit(tmp_path):
    exe = _build_devbuf_program(tmp_path)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "devbuf: ok" in run.stdout


def test_dev_buf_header_includes_nothing_of_hip():
    with open(os.path.join(ROOT, "autobzcore.jl_amd", "csrc", "dev_buf.h")) as f:
        includes = [ln.strip() for ln in f if ln.lstrip().startswith("#include")]
    assert includes == ["#include <cstddef>"], includes
