"""Host: a region of the field cut to the slabs of a chain (pffdtd_amd/csrc/pf_region_cut.h, what pf_multi_get_region hands every slab) has no
device in it.  tests/region_cut_check.cpp drives it as a program of its own, built with the host compiler under the address and
undefined-behaviour sanitizers: 1 to 5 slabs, cut along x and along file z, even and random cuts, random regions with strides 1 to 4 --
regions that miss slabs and regions of thickness 1 on the planes beside every cut among them -- : the slabs' parts tile the region exactly
once and land where the same slicing of the global array puts them; regions that are not well-formed or leave the grid are refused with a
message that names the field.  The parsers of the command line's regions (pffdtd_amd/fields.py) are host code too."""
import os
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_the_region_cut_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "region_cut_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "pffdtd_amd" / "csrc"), "-I", str(ROOT / "include"), str(ROOT / "tests" / "region_cut_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]


def test_the_command_line_regions():
    from pffdtd_amd import fields
    N = (40, 36, 44)
    assert fields.parse_planes("x=3,z=-1,x=39", N) == [((3, 0, 0), (4, 36, 44), (1, 1, 1)), ((0, 0, 43), (40, 36, 44), (1, 1, 1)), ((39, 0, 0), (40, 36, 44), (1, 1, 1))]
    assert fields.parse_box("3:29:1,1:27:2,2:25:3", N) == ((3, 1, 2), (29, 27, 25), (1, 2, 3))
    assert fields.parse_box(":,4:9,:44:5", N) == ((0, 4, 0), (40, 9, 44), (1, 1, 5))
    for bad in ("w=1", "x", "x=40", "y=-37", ""):
        with pytest.raises(ValueError):
            fields.parse_planes(bad, N)
    for bad in ("1:2,3:4", "5:5,0:3,0:3", "0:41,0:3,0:3", "0:4:0,0:3,0:3", "3,0:3,0:3"):
        with pytest.raises(ValueError):
            fields.parse_box(bad, N)


def test_the_launcher_refuses_the_field_arguments(tmp_path):
    """one process per GPU (WORLD_SIZE > 1): refused before anything is loaded, as the checkpoint arguments are"""
    r = subprocess.run([sys.executable, "-m", "pffdtd_amd.fdtd_main", "--field-planes", "x=3", "--field-every", "4"], cwd=tmp_path,
                       env={**os.environ, "PYTHONPATH": str(ROOT), "WORLD_SIZE": "2"}, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--field-planes" in r.stderr and "WORLD_SIZE" in r.stderr, (r.stdout[-500:], r.stderr[-500:])
    r = subprocess.run([sys.executable, "-m", "pffdtd_amd.fdtd_main", "--field-planes", "x=3"], cwd=tmp_path,
                       env={**os.environ, "PYTHONPATH": str(ROOT)}, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--field-every" in r.stderr  # (a region without a period, caught by the parser)
