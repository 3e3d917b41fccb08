"""No GPU: the lane maps of the staged column-strip bodies (pffdtd_amd/csrc/pf_strip_map.h) against the per-lane rules, on the CPU.

The staged bodies of k_wall2 move a tile's planes through LDS so that consecutive lanes reach consecutive 16 bytes of one row; the header
holds all of the index arithmetic -- element -> (row, vector), a row's source row, a row's store predicate, the places in the LDS tile --
and has no device in it.  tests/strip_map_check.cpp drives it as a program of its own, built with the host compiler under the address and
undefined-behaviour sanitizers (as test_host.py builds slab_cut_check.cpp), for 20-cell fp32 pencils on both sides of the grid, tiles that
start before the grid, end beyond the owned range and beyond the grid; it names every violated condition on stderr."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_the_strip_maps_reorder_and_nothing_else(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "strip_map_check"
    subprocess.run([cxx, "-std=c++17", "-O0", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "include"), "-I", str(ROOT / "pffdtd_amd" / "csrc"), str(ROOT / "tests" / "strip_map_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    assert "tiles checked" in r.stdout and not r.stdout.startswith("0 "), r.stdout
