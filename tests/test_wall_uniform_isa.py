"""No GPU: the march loops of the uniform-branch-count wall kernels in cross-compiled gfx950 ISA (tools/wall_loop_isa.py), against the counts
committed for the guarded form of the same kernels (profiles/wall_loop_isa_new.txt).

The guarded form spends, per evaluation of fd_regs, a compare and three selects per branch on `m < M` (about 102 v_cndmask and 33 v_cmp_lt_i32
per march loop), a twelfth branch for eleven, and twelve packed multiplications by two: about 216 instructions per march loop in all.  The
uniform form must have dropped them: at most 15 selects, no integer compare, at least 150 instructions fewer (the margin covers scheduling
noise), no scratch, no more registers.  And every other instantiation must still be the same machine code (`code`: a hash of the kernel's
instructions)."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.skipif(not Path("/opt/rocm/bin/hipcc").exists(), reason="no hipcc to cross-compile with")


def parse(text):
    """{kernel name: {"res": {VGPR, AGPR, scratch, code}, "bodies": [{column: count}]}}; defaulted trailing template arguments dropped"""
    out, cur, cols = {}, None, None
    for line in text.splitlines():
        m = re.match(r"^(k_wall2<.*>)\s*$", line)
        if m:
            name = re.sub(r", 0, false>$", ">", m.group(1))
            cur = out[name] = {"res": {}, "bodies": []}
            continue
        if cur is None:
            continue
        m = re.match(r"^\s+VGPR (\d+)\s+AGPR (\d+)\s+SGPR \d+\s+scratch (\d+) B\s+instructions \d+\s+code (\w+)", line)
        if m:
            cur["res"] = {"VGPR": int(m.group(1)), "AGPR": int(m.group(2)), "scratch": int(m.group(3)), "code": m.group(4)}
        elif line.split()[:1] == ["body"]:
            cols = line.split()
        elif line.strip() and cols:
            cur["bodies"].append(dict(zip(cols, map(int, line.split()))))
    return out


@pytest.fixture(scope="module")
def isa():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "wall_loop_isa.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return parse(r.stdout), parse((ROOT / "profiles" / "wall_loop_isa_new.txt").read_text())


KINDS = [("float, 10, false, true, true, 12, false, 3, 6, 1", 4), ("float, 20, true, true, true, 12, false, 3, 16, 1", 2)]


@pytest.mark.parametrize("mb", [11, 12])
@pytest.mark.parametrize("args, nbody", KINDS, ids=["xy", "strips"])
def test_uniform_loops_lost_the_guards(isa, args, nbody, mb):
    new, parent = isa
    k, p = new[f"k_wall2<{args}, {mb}, false>"], parent[f"k_wall2<{args}>"]
    assert len(k["bodies"]) == nbody == len(p["bodies"])
    for b, pb in zip(k["bodies"], p["bodies"]):
        print(args, mb, "body", b["body"], "total", b["total"], "parent", pb["total"], "v_cndmask", b["v_cndmask"], "v_cmp_lt_i32", b["v_cmp_lt_i32"])
        assert b["v_cndmask"] <= 15, b
        assert b["v_cmp_lt_i32"] == 0, b
        assert b["total"] <= pb["total"] - 150, (b, pb)
    assert k["res"]["scratch"] == 0, k["res"]
    assert k["res"]["VGPR"] + k["res"]["AGPR"] <= p["res"]["VGPR"] + p["res"]["AGPR"], (k["res"], p["res"])


def test_other_instantiations_are_the_same_machine_code(isa):
    new, parent = isa
    assert len(parent) == 6
    for name, p in parent.items():
        assert new[name]["res"]["code"] == p["res"]["code"], name
