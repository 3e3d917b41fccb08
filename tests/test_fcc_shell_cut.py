"""Host: the cut of a 13-point pair's shell into bricks (pffdtd_amd/csrc/pf_fcc_shell_cut.h, what air_variant 42 builds its tables with) has no
device in it.  tests/fcc_shell_cut_check.cpp drives it as a program of its own, built with the host compiler under the address and
undefined-behaviour sanitizers: three folded box rooms and one with a pillar through the shell, wall depths 3 and 7, one and two steps per
launch, the fp32 and fp64 LDS bounds -- every shell cell owned by exactly one brick, no box cell owned, extended boxes inside the interior,
LDS bytes and node counts within their bounds, every node's info word and list entry in place, every boundary node a brick's or the rest
list's, and the refusals (a source two cells from the shell, a node on the ABC shell, no brick size that fits) with their messages."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_the_shell_cut_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "fcc_shell_cut_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "pffdtd_amd" / "csrc"), str(ROOT / "tests" / "fcc_shell_cut_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
