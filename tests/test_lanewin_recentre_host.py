"""CPU: the index helpers of the grid search's re-centred second window (gradslam_amd/csrc/gs_lanewin.hpp: recentred_row, the row
ranges of a window of radius 1 to 3 around the pixel a point projects to; element7, the flattened candidate index over its up
to seven rows) checked exhaustively against naive enumerations on small grids, borders and corners included, by a stand-alone
host program, tests/lanewin_recentre_check.cpp, built with the address and undefined-behaviour sanitizers.  The header has no
HIP dependency: the kernel and this program compile the same functions."""
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


def test_recentred_window_rows_exhaustive(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++ / g++ / clang++) on this machine")
    exe = str(tmp_path / "lanewin_recentre_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(HERE, "lanewin_recentre_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "cases passed" in run.stdout
