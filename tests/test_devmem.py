"""CPU: the engine's owner of device allocations (csrc/pf_devmem.h) as a stand-alone program under the host compiler's sanitizers."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_the_engines_device_memory_owner_under_sanitizers(tmp_path):
    """csrc/pf_devmem.h -- the list of what an engine allocated on the device and the one function that frees it -- has no device in it:
    the free function is handed in.  tests/devmem_check.cpp drives it with a counting fake over malloc'ed blocks (every block freed exactly
    once by release, by the destructor or by both; null, foreign and already released pointers refused; the caller's pointer nulled; one
    address taken again after its release; "adopt two of a pool of six, release the rest" with two foreign members) as a program of its own,
    built with the host compiler under the address and undefined-behaviour sanitizers; it names every violated condition on stderr."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "devmem_check"
    subprocess.run([cxx, "-std=c++17", "-O0", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "pffdtd_amd" / "csrc"), str(ROOT / "tests" / "devmem_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
