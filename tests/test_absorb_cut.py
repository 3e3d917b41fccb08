"""CPU: the chain's merge of the wall absorption maps (csrc/pf_absorb_cut.h) as a stand-alone program under the host compiler's sanitizers."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_the_chains_absorption_merge_under_sanitizers(tmp_path):
    """csrc/pf_absorb_cut.h -- how pf_multi_absorb_get / _set move the slabs' node rows and add their bins -- has no device in it:
    tests/absorb_cut_check.cpp drives it over pf_slab_cut.h's slabs (G = 1, 2, 3, both cut axes) as a program of its own, built with the host
    compiler under the address and undefined-behaviour sanitizers: the node rows go through the slabs and back unchanged, and every ABC node and
    every source is counted by exactly one slab, the owner of its plane.  It names every violated condition on stderr."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "absorb_cut_check"
    subprocess.run([cxx, "-std=c++17", "-O0", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "include"), "-I", str(ROOT / "pffdtd_amd" / "csrc"), str(ROOT / "tests" / "absorb_cut_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
