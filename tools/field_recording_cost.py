#!/usr/bin/env python3
"""What a decimating recorder costs per sample, and which slot group S of its fold and which depth of its ring are fastest: pf_engine_decim_add
against a band accumulator on the same region and against the engine's own steps.

  tools/field_recording_cost.py --build                      (where hipcc is: the library once per S, beside the product)
  tools/field_recording_cost.py [--size 512] [--reps 7] [--out profiles/field_recording.txt]
  tools/field_recording_cost.py --axes [--size 512] [--reps 7] [--out profiles/field_vector_recording.txt]

S is a compile-time constant of csrc/pf_vdecim.h, so the library is built once per candidate S in {1, 4, 8} (tools/_decim_cost/, kept out of the
history; S = 4 is the product library as built) and every S is measured in a process of its own, started under a time limit of its own; the first
that fails ends the measurement.  In each process, on a shoebox size^3, fp32 (synth.shoebox), once stored in file order and once with the x and z
axes exchanged:
  * a size^2 z plane and a 64^3 box; factor 8 with 97 taps (P = 13) and with the verified 80 dB design for fpass = 1400 Hz at Ts = 1 / 25000
    (recordings.decimation_filter: 779 taps, P = 98); 2 shared sections (the integrator + low-cut of order 4);
  * ms per sample at depths 1, 4, 8 and 16: wall time around 16 adds that end in a device synchronise, over 16, after a warm-up of the same 16; the
    median of --reps repetitions in which the depths and a band accumulator of 6 octave bands (pf_bandacc, its default depth) ALTERNATE;
  * beside them the same engine's wall time per single step (run(n, 1)) without any recorder call in between.
No threshold is fixed in advance.  Recorded at the end: the (S, depth) with the smallest sum of medians over the plane cases, which PF_DECIM_SLOTS
and PF_DECIM_DEFAULT_DEPTH (csrc/pf_vdecim.h) are to equal.  Needs a GPU; there is no fallback.

--axes measures the VECTOR decimating recorders instead (pf_engine_vdecim_add, csrc/pf_vdecim.h), with the product library alone, in one process
under one time limit: the same engine, filters and method; the regions keep one cell clear of the faces (the plane is the (size - 2)^2 interior of
the z plane), as a difference needs; per region and filter the scalar recorder (the vector recorder's code with the one component 0, entered through
pf_engine_decim_*), the vector recorder with comp = [0] and the one with the 4
components 0, 1, 2, 3 (the sections directional.gradient_sections gives: 3 per component), each at depths 1, 4, 8 and 16, all twelve ALTERNATING.
Recorded at the end: the depth with the smallest sum of the 4-component medians over the plane cases, which PF_VDECIM_DEFAULT_DEPTH
(csrc/pf_vdecim.h) is to equal.
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

BATCH = 16
DEPTHS = (1, 4, 8, 16)
SLOTS = (1, 4, 8)
PRODUCT_S = 4
VARIANTS = ROOT / "tools" / "_decim_cost"


def variant(s):
    return ROOT / "pffdtd_amd" / "libpffdtd_hip.so" if s == PRODUCT_S else VARIANTS / f"libpffdtd_hip_S{s}.so"


def build():
    from pffdtd_amd import build as b
    VARIANTS.mkdir(exist_ok=True)
    b.build_hip()
    for s in SLOTS:
        if s != PRODUCT_S:
            b.build_hip(extra_flags=[f"-DPF_DECIM_SLOTS_N={s}"], out=variant(s))


def child(a):
    """one S: prints the report's lines, then one JSON line of the plane cases' sums per depth"""
    from pffdtd_amd import engine
    engine.lib_path = lambda: variant(a.child)  # (before the first call loads the library)
    from checkpoint_cost import timed
    from pffdtd_amd import decay, recordings, sim_data, synth
    import numpy as np
    if engine.device_count() < 1:
        raise SystemExit("no HIP device visible: nothing can be measured here")
    n = a.size
    sd = sim_data.SimData.from_sim(synth.shoebox(n, n, n, Nt=16 + a.reps + 8, Nm=1, Mb=3), "single", build_mask=False)
    sd.scale_input()
    Ts = 1.0 / 25000.0
    pre = decay.pre_sections(Ts, True, 10.0, 4)
    bands = decay.band_sections(Ts, [125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0], 3)
    long_taps, info = recordings.decimation_filter(Ts, 8, 1400.0, 80.0)
    short_taps = np.ascontiguousarray(long_taps[(long_taps.size - 97) // 2:(long_taps.size + 97) // 2])
    filters = [("97 taps, P = 13", short_taps), (f"{long_taps.size} taps, P = {info['slots']}", long_taps)]
    assert pre.shape == (2, 6) and short_taps.size == 97
    h, b0 = n // 2, n // 2 - 32
    shapes = [(f"{n}^2 z plane", ([0, 0, h], [n, n, h + 1])), ("64^3 box", ([b0] * 3, [b0 + 64] * 3))]
    cap = 2 * BATCH * (a.reps + 1) // 8  # never full: nothing is read
    plane_sum = {d: 0.0 for d in DEPTHS}
    for name, layout in (("file order", engine.PF_LAYOUT_FILE), ("exchanged axes", engine.PF_LAYOUT_EXCHANGED)):
        eng = engine.HipEngine(sd, layout=layout)
        assert eng.layout()[2] == (layout == engine.PF_LAYOUT_EXCHANGED)
        eng.run(0, 16)
        eng.sync()
        step = 16
        t1 = []
        for _ in range(a.reps):  # the engine alone: no recorder exists yet
            t1.append(timed(lambda: (eng.run(step, 1), eng.sync()))[0] * 1e3)
            step += 1
        print(f"S = {a.child}, {name}: the engine alone: a single step {statistics.median(t1):.3f} ms (min {min(t1):.3f})", flush=True)
        for label, (lo, hi) in shapes:
            for fname, taps in filters:
                recs = {d: eng.decimating_recorder(lo, hi, pre_sos=pre, taps=taps, factor=8, cap=cap, depth=d) for d in DEPTHS}
                recs["band"] = eng.band_accumulator(lo, hi, pre_sos=pre, band_sos=bands, nbin=40)
                batches = {k: 0 for k in recs}

                def batch(k):
                    for _ in range(BATCH):
                        if k == "band":
                            recs[k].add(batches[k] % 40)
                        else:
                            recs[k].add()
                    eng.sync()
                    batches[k] += 1

                ms = {k: [] for k in recs}
                for k in recs:
                    batch(k)  # warm-up: the code objects of this depth's fold
                for _ in range(a.reps):
                    for k in recs:
                        ms[k].append(timed(lambda: batch(k))[0] * 1e3 / BATCH)
                med = {k: statistics.median(ms[k]) for k in recs}
                for k in recs:
                    what = f"depth {k:2d}" if k != "band" else "pf_bandacc, 6 bands"
                    print(f"  S = {a.child}  {label:13s} {fname:20s} {what:20s}: {med[k]:8.4f} ms per sample (min {min(ms[k]):.4f}, max {max(ms[k]):.4f})   "
                          f"{100 * med[k] / statistics.median(t1):5.1f} % of a single step", flush=True)
                    if "plane" in label and k != "band":
                        plane_sum[k] += med[k]
                for r in recs.values():
                    assert r.count == BATCH * (a.reps + 1)
                    r.close()
        eng.close()
    print("RESULT " + json.dumps({str(d): plane_sum[d] for d in DEPTHS}), flush=True)


def child_axes(a):
    """the vector recorders beside the scalar one: prints the report's lines, then one JSON line of the 4-component plane sums per depth"""
    from checkpoint_cost import timed
    from pffdtd_amd import decay, directional, engine, recordings, sim_data, synth
    import numpy as np
    if engine.device_count() < 1:
        raise SystemExit("no HIP device visible: nothing can be measured here")
    n = a.size
    sd = sim_data.SimData.from_sim(synth.shoebox(n, n, n, Nt=16 + a.reps + 8, Nm=1, Mb=3), "single", build_mask=False)
    sd.scale_input()
    Ts = 1.0 / 25000.0
    pre = decay.pre_sections(Ts, True, 10.0, 4)
    omni, grad = directional.gradient_sections(Ts, 343.0 * Ts * np.sqrt(3.0), 343.0, True, 10.0, 4)
    pre4 = np.stack([omni, grad, grad, grad])
    long_taps, info = recordings.decimation_filter(Ts, 8, 1400.0, 80.0)
    short_taps = np.ascontiguousarray(long_taps[(long_taps.size - 97) // 2:(long_taps.size + 97) // 2])
    filters = [("97 taps, P = 13", short_taps), (f"{long_taps.size} taps, P = {info['slots']}", long_taps)]
    h, b0 = n // 2, n // 2 - 32
    shapes = [(f"{n - 2}^2 z plane", ([1, 1, h], [n - 1, n - 1, h + 1])), ("64^3 box", ([b0] * 3, [b0 + 64] * 3))]
    cap = 2 * BATCH * (a.reps + 1) // 8  # never full: nothing is read
    kinds = [("scalar", None), ("comp [0]", (0,)), ("4 components", (0, 1, 2, 3))]
    plane_sum = {d: 0.0 for d in DEPTHS}
    for name, layout in (("file order", engine.PF_LAYOUT_FILE), ("exchanged axes", engine.PF_LAYOUT_EXCHANGED)):
        eng = engine.HipEngine(sd, layout=layout)
        assert eng.layout()[2] == (layout == engine.PF_LAYOUT_EXCHANGED)
        eng.run(0, 16)
        eng.sync()
        step = 16
        t1 = []
        for _ in range(a.reps):  # the engine alone: no recorder exists yet
            t1.append(timed(lambda: (eng.run(step, 1), eng.sync()))[0] * 1e3)
            step += 1
        print(f"{name}: the engine alone: a single step {statistics.median(t1):.3f} ms (min {min(t1):.3f})", flush=True)
        for label, (lo, hi) in shapes:
            for fname, taps in filters:
                recs = {}
                for kname, comp in kinds:
                    for d in DEPTHS:
                        if comp is None:
                            recs[(kname, d)] = eng.decimating_recorder(lo, hi, pre_sos=pre, taps=taps, factor=8, cap=cap, depth=d)
                        else:
                            recs[(kname, d)] = eng.vector_decimating_recorder(lo, hi, comp=comp, pre_sos=pre4[:len(comp)], taps=taps, factor=8, cap=cap, depth=d)

                def batch(k):
                    for _ in range(BATCH):
                        recs[k].add()
                    eng.sync()

                ms = {k: [] for k in recs}
                for k in recs:
                    batch(k)  # warm-up: the code objects of this depth's fold
                for _ in range(a.reps):
                    for k in recs:
                        ms[k].append(timed(lambda: batch(k))[0] * 1e3 / BATCH)
                med = {k: statistics.median(ms[k]) for k in recs}
                for k in recs:
                    print(f"  {label:13s} {fname:20s} {k[0]:13s} depth {k[1]:2d}: {med[k]:8.4f} ms per sample (min {min(ms[k]):.4f}, max {max(ms[k]):.4f})   "
                          f"{100 * med[k] / statistics.median(t1):5.1f} % of a single step", flush=True)
                    if "plane" in label and k[0] == "4 components":
                        plane_sum[k[1]] += med[k]
                for r in recs.values():
                    assert r.count == BATCH * (a.reps + 1)
                    r.close()
        eng.close()
    print("RESULT " + json.dumps({str(d): plane_sum[d] for d in DEPTHS}), flush=True)


def main_axes(a):
    out = a.out if a.out else str(ROOT / "profiles" / "field_vector_recording.txt")
    lines = [f"vector decimating recorders: shoebox {a.size}^3 fp32, factor 8, ms per sample (wall time of {BATCH} adds and a synchronise, over {BATCH}), median of "
             f"{a.reps} alternating repetitions; scalar: 2 shared sections; vector: 3 sections per component; one process"]
    print(lines[0], flush=True)
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, __file__, "--child-axes", "--size", str(a.size), "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    sums = None
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            sums = {int(k): v for k, v in json.loads(line[7:]).items()}
        else:
            print(line, flush=True)
            lines.append(line)
    if r.returncode != 0 or sums is None:
        print(r.stderr[-3000:], file=sys.stderr)
        raise SystemExit(f"--axes: the measurement ended with status {r.returncode}; stopped")
    lines.append("4 components: sum of the plane cases' medians per depth: " + ", ".join(f"{d}: {sums[d]:.4f} ms" for d in DEPTHS))
    lines.append(f"->  the default depth these measurements justify for PF_VDECIM_DEFAULT_DEPTH: {min(DEPTHS, key=lambda d: sums[d])}")
    print("\n".join(lines[-2:]), flush=True)
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="", help="the report (default: profiles/field_recording.txt; with --axes profiles/field_vector_recording.txt)")
    ap.add_argument("--axes", action="store_true", help="measure the vector decimating recorders beside the scalar one (the product library alone)")
    ap.add_argument("--child-axes", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--limit", type=int, default=240, metavar="SECONDS", help="the time limit of each S's process")
    a = ap.parse_args()
    if a.build:
        return build()
    if a.child:
        return child(a)
    if a.child_axes:
        return child_axes(a)
    if a.axes:
        return main_axes(a)
    a.out = a.out if a.out else str(ROOT / "profiles" / "field_recording.txt")
    missing = [str(variant(s)) for s in SLOTS if not variant(s).exists()]
    if missing:
        raise SystemExit(f"not built: {', '.join(missing)} (tools/field_recording_cost.py --build)")
    lines = [f"decimating recorders: shoebox {a.size}^3 fp32, factor 8, 2 shared sections, ms per sample (wall time of {BATCH} adds and a synchronise, over {BATCH}), "
             f"median of {a.reps} alternating repetitions; one process per S"]
    print(lines[0], flush=True)
    sums = {}
    for s in SLOTS:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, __file__, "--child", str(s), "--size", str(a.size), "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                sums[s] = {int(k): v for k, v in json.loads(line[7:]).items()}
            else:
                print(line, flush=True)
                lines.append(line)
        if r.returncode != 0 or s not in sums:  # the first failure ends the measurement: nothing more is started on the device
            print(r.stderr[-3000:], file=sys.stderr)
            raise SystemExit(f"S = {s}: the measurement ended with status {r.returncode}; stopped")
    for s in SLOTS:
        lines.append(f"S = {s}: sum of the plane cases' medians per depth: " + ", ".join(f"{d}: {sums[s][d]:.4f} ms" for d in DEPTHS))
    best = min(((s, d) for s in SLOTS for d in DEPTHS), key=lambda sd_: sums[sd_[0]][sd_[1]])
    lines.append(f"->  the S and the default depth these measurements justify: S = {best[0]}, depth {best[1]}")
    print("\n".join(lines[-len(SLOTS) - 1:]), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
