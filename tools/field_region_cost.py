#!/usr/bin/env python3
"""What a field region costs: pf_engine_get_region against pf_engine_get_grid plus slicing, the only way to a plane before it.

  tools/field_region_cost.py [--size 512] [--reps 7] [--out profiles/field_regions.txt]

On a shoebox size^3, fp32 (synth.shoebox), once stored in file order and once with the x and z axes exchanged, in one process:
  * an x plane, a y plane, a z plane and a 64^3 box through get_region: wall time around calls that end in a device synchronise, after a
    warm-up call per shape, the median of --reps repetitions ALTERNATING with
  * the same data through get_grid(1) and numpy slicing -- pf_engine_get_grid is not touched by the region work, so this is the parent
    commit's path, measured in the same process on the same engine;
  * the whole grid as one region against get_grid;
  * device memory in use (hipMemGetInfo) before and DURING the whole-grid region and get_grid (sampled by a second thread while the call
    runs): what get_region adds is its staging buffer, at most 32 MiB (PF_REGION_STAGE_BYTES), never a grid.
Condition, to be recorded rather than trusted: no case slower than get_grid plus slicing, no call above the staging cap.
Needs a GPU; there is no fallback.
"""
import argparse
import statistics
import sys
import threading
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from checkpoint_cost import mem_used, timed  # noqa: E402
from pffdtd_amd import engine, sim_data, synth  # noqa: E402

STAGE_CAP = 32 << 20


def peak_during(f):
    """-> (seconds, rise of the device memory in use while f runs, samples)"""
    before = mem_used()
    peak, stop = [before], threading.Event()

    def sample():
        while not stop.is_set():
            peak.append(mem_used())
            time.sleep(0.002)

    th = threading.Thread(target=sample)
    th.start()
    dt, _ = timed(f)
    stop.set()
    th.join()
    return dt, max(peak) - before, len(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "field_regions.txt"))
    a = ap.parse_args()
    if engine.device_count() < 1:
        raise SystemExit("no HIP device visible: nothing can be measured here")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = a.size
    sd = sim_data.SimData.from_sim(synth.shoebox(n, n, n, Nt=16, Nm=1, Mb=3), "single", build_mask=False)
    sd.scale_input()
    h, b0 = n // 2, n // 2 - 32
    shapes = [("x plane", ([h, 0, 0], [h + 1, n, n], [1, 1, 1])), ("y plane", ([0, h, 0], [n, h + 1, n], [1, 1, 1])),
              ("z plane", ([0, 0, h], [n, n, h + 1], [1, 1, 1])), ("64^3 box", ([b0] * 3, [b0 + 64] * 3, [1, 1, 1])),
              ("whole grid", ([0, 0, 0], [n, n, n], [1, 1, 1]))]
    say(f"field regions: shoebox {n}^3 fp32 ({sd.Npts * 4 / 2**20:.0f} MiB per grid), median of {a.reps} alternating repetitions, ms")
    worst = 0.0
    for name, layout in (("file order", engine.PF_LAYOUT_FILE), ("exchanged axes", engine.PF_LAYOUT_EXCHANGED)):
        eng = engine.HipEngine(sd, layout=layout)
        eng.run(0, 8)
        assert eng.layout()[2] == (layout == engine.PF_LAYOUT_EXCHANGED)
        say(f"{name}:")
        for label, (lo, hi, st) in shapes:
            sl = tuple(slice(lo[k], hi[k], st[k]) for k in range(3))
            new = lambda: eng.get_region(1, lo, hi, st)
            old = lambda: np.ascontiguousarray(eng.get_grid(1)[sl])
            assert np.array_equal(new(), old())  # (warm-up of both, and the same cells)
            reps = a.reps if label != "whole grid" else max(3, a.reps // 2)
            t_new, t_old = [], []
            for _ in range(reps):
                t_old.append(timed(old)[0] * 1e3)
                t_new.append(timed(new)[0] * 1e3)
            m_new, m_old = statistics.median(t_new), statistics.median(t_old)
            worst = max(worst, m_new / m_old)
            nbytes = int(np.prod([hi[k] - lo[k] for k in range(3)])) * 4
            say(f"  {label:10s} {nbytes / 2**20:8.2f} MiB  get_region {m_new:9.3f} (min {min(t_new):.3f}, max {max(t_new):.3f})   "
                f"get_grid + slicing {m_old:9.3f} (min {min(t_old):.3f}, max {max(t_old):.3f})   ratio {m_new / m_old:.4f}")
        lo, hi, st = shapes[-1][1]
        dt, rise, ns = peak_during(lambda: eng.get_region(1, lo, hi, st))
        say(f"  device memory while the whole-grid region runs ({dt * 1e3:.0f} ms, {ns} samples): +{rise / 2**20:.1f} MiB "
            f"(cap {STAGE_CAP / 2**20:.0f} MiB: {'within' if rise <= STAGE_CAP else 'ABOVE'})")
        dt, rise, ns = peak_during(lambda: eng.get_grid(1))
        say(f"  device memory while get_grid runs ({dt * 1e3:.0f} ms, {ns} samples): +{rise / 2**20:.1f} MiB")
        eng.run(8, 4)  # (the engine still steps)
        eng.close()
    say(f"largest get_region / (get_grid + slicing): {worst:.4f}  ({'no case slower' if worst <= 1.0 else 'A CASE IS SLOWER'})")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
