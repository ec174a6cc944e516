"""CPU: the range arithmetic of the grid search's window rows (gradslam_amd/csrc/gs_lanewin.hpp: exact range -> covered chunks,
flattened candidate index -> (row, offset)) checked exhaustively by a stand-alone host program, tests/lanewin_check.cpp, built
with the address and undefined-behaviour sanitizers.  The header has no HIP dependency: the kernel and this program compile
the same functions."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gradslam_amd", "csrc")


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        path = shutil.which(name) if name else None
        if path:
            return path
    return None


def test_lanewin_ranges_exhaustive(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++ / g++ / clang++) on this machine")
    exe = str(tmp_path / "lanewin_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(HERE, "lanewin_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "cases passed" in run.stdout
