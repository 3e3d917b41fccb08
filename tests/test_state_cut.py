"""CPU: the chain's cut of the canonical state (csrc/pf_state_cut.h) as a stand-alone program under the host compiler's sanitizers."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_the_chains_state_cut_under_sanitizers(tmp_path):
    """csrc/pf_state_cut.h -- how pf_multi_save_state / _load_state cut the scene's state to the slabs and put it together again -- has no
    device in it: tests/state_cut_check.cpp drives it over pf_slab_cut.h's slabs on a small unsorted scene with duplicate lossy entries
    (G = 1, 2, 3, 5, both axes, fp32 and fp64) as a program of its own, built with the host compiler under the address and
    undefined-behaviour sanitizers; it names every violated condition on stderr."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "state_cut_check"
    subprocess.run([cxx, "-std=c++17", "-O0", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "include"), "-I", str(ROOT / "pffdtd_amd" / "csrc"), str(ROOT / "tests" / "state_cut_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
