#!/usr/bin/env python3
"""What a checkpoint costs: pf_engine_save_state / pf_engine_load_state against the calls that moved the fields before them.

  tools/checkpoint_cost.py [--size 1024] [--mb 11] [--reps 3] [--out profiles/checkpoint_cost.txt]

On the headline grid as bench.py builds it (shoebox size^3, 7-point fp32, Mb = 11 walls), in one process:
  * save_state and load_state, wall time around calls that end in a device synchronise, the median of --reps alternating repetitions;
  * the two pf_engine_get_grid / two pf_engine_set_grid calls that were the only way to move the fields before (unchanged by the
    checkpoint work: the parent's cost), alternating with them;
  * on a second engine that stores the axes exchanged: device memory in use (hipMemGetInfo) before, DURING (sampled by a second thread
    while the call runs) and after a save -- what the call adds is its staging buffer and the node arrays' device copy, not a grid.
Expected, to be recorded rather than trusted: save / load at most 1.25 x the corresponding pair (the node state adds about 7 % to the
bytes).  A larger ratio means the staging serialises copies and kernels.  Needs a GPU; there is no fallback.
"""
import argparse
import ctypes
import statistics
import sys
import threading
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402  (build_scene: the headline grid exactly as the benchmark builds it)
from pffdtd_amd import engine  # noqa: E402


def mem_used():
    try:  # the HIP runtime this process already uses (engine.lib() loaded it)
        hip = ctypes.CDLL(None)
        hip.hipMemGetInfo
    except (OSError, AttributeError):
        hip = ctypes.CDLL("libamdhip64.so")
    fr, tot = ctypes.c_size_t(), ctypes.c_size_t()
    if hip.hipMemGetInfo(ctypes.byref(fr), ctypes.byref(tot)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return tot.value - fr.value


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--mb", type=int, default=11)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "checkpoint_cost.txt"))
    a = ap.parse_args()
    if engine.device_count() < 1:
        raise SystemExit("no HIP device visible: nothing can be measured here")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = a.size
    sd = bench.build_scene(n, 64, "single", False, True, a.mb)
    field_b, node_b = 2 * sd.Npts * 4, sd.Nbl * 26 * 4
    say(f"checkpoint cost: shoebox {n}^3, 7-point fp32, Mb = {a.mb}: {sd.Nbl} frequency-dependent nodes; fields {field_b / 2**30:.2f} GiB, "
        f"node state {node_b / 2**30:.3f} GiB ({100.0 * node_b / field_b:.1f} % of the fields)")
    eng = engine.HipEngine(sd)
    eng.run(0, 12)
    tm = eng.timing()
    say(f"engine: interior path {({0: 'lean single steps', 1: 'barrier-free single steps', 2: 'blocked passes'}).get(tm['air_path'], 'other')}, "
        f"wall regions {sum(tm['wall_blocks']) > 0}, bricks {tm['wall_bricks']}, exchanged axes {eng.layout()[2]}")
    st = eng.save_state()  # (warm-up: the host arrays' pages, the kernels' code objects)
    eng.load_state(st)
    g = [eng.get_grid(0), eng.get_grid(1)]
    t = {"save_state": [], "get_grid x2": [], "load_state": [], "set_grid x2": []}
    for _ in range(a.reps):  # alternating: other people's work shares the host
        t["get_grid x2"].append(timed(lambda: [eng.get_grid(0), eng.get_grid(1)])[0])
        t["save_state"].append(timed(eng.save_state)[0])
        t["set_grid x2"].append(timed(lambda: [eng.set_grid(0, g[0]), eng.set_grid(1, g[1])])[0])
        t["load_state"].append(timed(lambda: eng.load_state(st))[0])
    med = {k: statistics.median(v) for k, v in t.items()}
    for k, v in t.items():
        say(f"  {k:12s} median {med[k]:7.3f} s  (runs: {', '.join(f'{x:.3f}' for x in v)})  {((field_b + (node_b if 'state' in k else 0)) / med[k]) / 1e9:6.2f} GB/s")
    for x, y in (("save_state", "get_grid x2"), ("load_state", "set_grid x2")):
        r = med[x] / med[y]
        say(f"  {x} / {y} = {r:.3f}  (expected at most 1.25: {'within' if r <= 1.25 else 'ABOVE -- the staging serialises copies and kernels'})")
    # (the state survived all of that: the run goes on and the engine still answers)
    eng.run(12, 4)
    eng.close()
    del g, st

    ex = engine.HipEngine(sd, layout=engine.PF_LAYOUT_EXCHANGED)
    ex.run(0, 4)
    before = mem_used()
    peak, stop = [before], threading.Event()

    def sample():
        while not stop.is_set():
            peak.append(mem_used())
            time.sleep(0.01)

    th = threading.Thread(target=sample)
    th.start()
    dt, st = timed(ex.save_state)
    stop.set()
    th.join()
    after = mem_used()
    stage_b = min(32, sd.Nx) * sd.Ny * sd.Nz * 4
    say(f"exchanged-axes engine, save_state {dt:.3f} s: device memory in use before {before / 2**20:.0f} MiB, peak during {max(peak) / 2**20:.0f} MiB "
        f"({len(peak)} samples), after {after / 2**20:.0f} MiB; rise {(max(peak) - before) / 2**20:.0f} MiB = staging buffer {stage_b / 2**20:.0f} MiB "
        f"+ node arrays {node_b / 2**20:.0f} MiB (one grid: {sd.Npts * 4 / 2**20:.0f} MiB)")
    dt, _ = timed(lambda: ex.get_grid(1))
    say(f"  (pf_engine_get_grid on the same engine allocates a whole grid for its {dt:.3f} s)")
    ex.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
