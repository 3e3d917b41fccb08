#!/usr/bin/env python3
"""The march loops of the three-step wall kernels (pf_wall.h: k_wall2<..., NS = 3, GD>) in gfx950 ISA, counted by instruction class.

Cross-compiles a small translation unit that instantiates the kernels (no GPU needed) and prints, per kernel, registers and scratch and,
per body (one march loop each: x / y regions four -- mode x side --, column strips two), the instructions between the loop's header and
its back edge.  The count is STATIC: out-of-line paths inside the loop count whether a step runs them or not.  Where the header has them, the
uniform-branch-count bodies (UB = 11, 12, and 4 with the count as a wave-uniform bound) are listed after the guarded ones; the columns after
`s_cmp` count what those bodies are about: vector compares (the integer `m < M` guards apart), packed multiplications, LDS accesses by width.

  tools/wall_loop_isa.py [--csrc DIR] [--keep FILE.s]

--csrc: the directory holding pf_wall.h (default: pffdtd_amd/csrc), e.g. an older checkout's, to compare.  `code` is a hash of a kernel's
instructions with the labels taken out: equal hashes = the same machine code.
"""
import argparse
import hashlib
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
ap = argparse.ArgumentParser()
ap.add_argument("--csrc", default=str(ROOT / "pffdtd_amd" / "csrc"))
ap.add_argument("--keep", default="")
args = ap.parse_args()
csrc = Path(args.csrc)
header = (csrc / "pf_wall.h").read_text()
profiles = "int PR" in header  # (wall profiles: a trailing template parameter)
uniform = "int UB" in header   # (uniform branch counts: two more)
per_lane = "bool PL" in header # (the strips' uniform bodies are staged through LDS; PL = true: their per-lane form)

# (Real, DP, VEC, FAST, NODES, MC, SG, NS, GD[, PR[, UB, USK]])
kernels = []
for dp, vec, gd in ((10, "false", 6), (20, "true", 16)):
    kernels.append(f"float, {dp}, {vec}, true, true, 12, false, 3, {gd}")
    if profiles:
        kernels.append(f"float, {dp}, {vec}, true, true, 12, false, 3, {gd}, 1")
        kernels.append(f"float, {dp}, {vec}, true, true, 4, false, 3, {gd}, 2")
    if uniform:
        kernels.append(f"float, {dp}, {vec}, true, true, 12, false, 3, {gd}, 1, 11, false")
        kernels.append(f"float, {dp}, {vec}, true, true, 12, false, 3, {gd}, 1, 12, false")
        kernels.append(f"float, {dp}, {vec}, true, true, 4, false, 3, {gd}, 1, 4, true")
    if per_lane and vec == "true":
        kernels.append(f"float, {dp}, {vec}, true, true, 12, false, 3, {gd}, 1, 11, false, true")
        kernels.append(f"float, {dp}, {vec}, true, true, 12, false, 3, {gd}, 1, 12, false, true")
        kernels.append(f"float, {dp}, {vec}, true, true, 4, false, 3, {gd}, 1, 4, true, true")
src = '#include "pf_wall.h"\n' + "".join(f"template __global__ void pf::k_wall2<{k}>(pf::WallParams<float>, float, float);\n" for k in kernels)

with tempfile.TemporaryDirectory() as d:
    unit, asm = Path(d) / "wall_isa.hip", Path(args.keep) if args.keep else Path(d) / "wall_isa.s"
    unit.write_text(src)
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-value", "--cuda-device-only", "-S",
           "-I", str(ROOT / "include"), "-I", str(csrc), str(unit), "-o", str(asm)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr[-3000:])
    text = asm.read_text().splitlines()

CLASSES = ("total", "VALU", "SALU", "VMEM", "DS", "v_mov", "accvgpr", "v_cndmask", "s_cselect", "s_cmp", "v_cmp", "v_cmp_lt_i32", "v_pk_mul_f32", "ds_b128", "ds_b64", "ds_read2")


def classify(op):
    c = []
    if op.startswith("v_"):
        c.append("VALU")
        if op.startswith("v_accvgpr"):
            c.append("accvgpr")
        elif op.startswith(("v_mov_b", "v_pk_mov")):
            c.append("v_mov")
        elif op.startswith("v_cndmask"):
            c.append("v_cndmask")
        elif op.startswith("v_cmp"):
            c.append("v_cmp")
            if op.startswith("v_cmp_lt_i32"):
                c.append("v_cmp_lt_i32")
        elif op.startswith("v_pk_mul_f32"):
            c.append("v_pk_mul_f32")
    elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        c.append("VMEM")
    elif op.startswith("ds_"):
        c.append("DS")
        if op.startswith(("ds_read_b128", "ds_write_b128")):
            c.append("ds_b128")
        elif op.startswith(("ds_read_b64", "ds_write_b64")):
            c.append("ds_b64")
        elif op.startswith(("ds_read2", "ds_write2")):
            c.append("ds_read2")
    elif op.startswith("s_") and not op.startswith(("s_waitcnt", "s_nop", "s_branch", "s_cbranch", "s_load", "s_barrier", "s_endpgm", "s_sleep", "s_setprio")):
        c.append("SALU")
        if op.startswith("s_cselect"):
            c.append("s_cselect")
        elif op.startswith(("s_cmp", "s_bitcmp")):
            c.append("s_cmp")
    return c


# cut the assembly into functions: "<name>:" ... ".end_amdhsa_kernel" / the resource comments that follow
funcs, cur = {}, None
for line in text:
    m = re.match(r"^(_Z\w+):", line)
    if m and "k_wall2" in m.group(1):
        cur = m.group(1)
        funcs[cur] = {"lines": [], "res": {}}
        continue
    if cur is None:
        continue
    m = re.match(r"^\s*; (NumVgprs|NumAgprs|TotalNumSgprs|ScratchSize|Occupancy): (\d+)", line)
    if m:
        funcs[cur]["res"][m.group(1)] = int(m.group(2))
        if m.group(1) == "Occupancy":
            cur = None
        continue
    funcs[cur]["lines"].append(line)

names = subprocess.run(["c++filt"] + list(funcs), capture_output=True, text=True, stdin=subprocess.DEVNULL).stdout.splitlines()
print("march loop of k_wall2<float, DP, VEC, FAST, NODES, MC, SG, NS, GD" + (", PR" if profiles else "") + (", UB, USK" if uniform else "") + ("[, PL = true]" if per_lane else "") + ">, static instruction counts per body")
for (mangled, f), name in zip(funcs.items(), names):
    name = re.sub(r"\(.*", "", name).replace("void pf::", "")
    if per_lane:  # (the last argument is printed where it is set only: the other kernels keep the names they had)
        name = re.sub(r", false>$", ">", name)
    # instructions in order, labels remembered by the index of the instruction that follows them
    ins, labels = [], {}
    for line in f["lines"]:
        s = line.split(";")[0].strip()
        if not s or s.startswith("."):
            m = re.match(r"^(\.LBB\w+):", s)
            if m:
                labels[m.group(1)] = len(ins)
            continue
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        ins.append(s.split(None, 1))
    code = hashlib.sha1("\n".join(" ".join(re.sub(r"\.LBB\w+", "L", t) for t in i) for i in ins).encode()).hexdigest()[:12]
    res = f["res"]
    print(f"\n{name}\n  VGPR {res.get('NumVgprs', 0)}  AGPR {res.get('NumAgprs', 0)}  SGPR {res.get('TotalNumSgprs', 0)}  scratch {res.get('ScratchSize', 0)} B  "
          f"instructions {len(ins)}  code {code}")
    loops = []
    for i, t in enumerate(ins):
        if t[0].startswith(("s_cbranch", "s_branch")) and len(t) > 1 and t[1] in labels and labels[t[1]] <= i:
            loops.append((labels[t[1]], i))
    # A march loop has several back edges (its out-of-line paths jump back into it): overlapping spans are one loop, from the first
    # header to the last back edge.  (The copy of the coefficients to LDS is a short loop of its own.)
    outer = []
    for b, e in sorted(loops):
        if outer and b <= outer[-1][1]:
            outer[-1][1] = max(outer[-1][1], e)
        else:
            outer.append([b, e])
    outer = [l for l in outer if l[1] - l[0] > 300]
    print("  " + " ".join(f"{c:>{max(9, len(c))}}" for c in ("body",) + CLASSES))
    for n, (b, e) in enumerate(sorted(outer)):
        cnt = dict.fromkeys(CLASSES, 0)
        for t in ins[b:e + 1]:
            cnt["total"] += 1
            for c in classify(t[0]):
                cnt[c] += 1
        print("  " + " ".join(f"{v:>{max(9, len(c))}}" for c, v in zip(("body",) + CLASSES, [n] + [cnt[c] for c in CLASSES])))
