"""eval_route (csrc/eval_route.h), the one place that decides which instance of the grid Fourier-eval kernel runs, on what
launch grid and with how much LDS, checked without a device: tests/c/eval_route_main.cpp holds a table of shapes with the
routes recorded from the launch code before the decisions were gathered in that header, and exits 0 only if every field of
every route matches."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, *extra):
    """g++ -std=c++17 -Wall -Wextra -Werror on the stand-alone program: the header needs nothing of HIP."""
    exe = tmp_path / "eval_route_main"
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", *extra, os.path.join(ROOT, "tests", "c", "eval_route_main.cpp"),
           "-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def test_eval_route_matches_the_recorded_routes(tmp_path):
    run = subprocess.run([str(_build(tmp_path))], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "eval_route: ok" in run.stdout


def test_eval_route_header_includes_nothing_of_hip():
    with open(os.path.join(ROOT, "autobzcore.jl_amd", "csrc", "eval_route.h")) as f:
        includes = [ln.strip() for ln in f if ln.lstrip().startswith("#include")]
    assert includes and all(inc.startswith("#include <") and "hip" not in inc for inc in includes), includes
