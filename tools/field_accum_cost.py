#!/usr/bin/env python3
"""What a field accumulator costs per sample, and which depth of its ring is faster: pf_engine_accum_add against the engine's own steps.

  tools/field_accum_cost.py [--size 512] [--reps 7] [--out profiles/field_spectra.txt]

On a shoebox size^3, fp32 (synth.shoebox), once stored in file order and once with the x and z axes exchanged, in one process:
  * a z plane and an x plane with 32 frequencies (64 channels) and a 64^3 box with 8 frequencies (16 channels);
  * ms per sample at depth 1, at depth 8 and at the library's default (depth 0): wall time around 16 adds that end in a device synchronise
    (16 is a multiple of every depth measured, so every timing holds whole folds), over 16, after a warm-up of the same 16; the median of --reps
    repetitions in which the depths ALTERNATE;
  * beside them the same engine's wall time per single step (run(n, 1)) and per run of three steps (run(n, 3): a triple where the engine steps in
    triples) without any accumulator call in between -- the parent commit's behaviour, what the cost is read against;
  * the bytes per sample counted from the formulas of csrc/pf_accum.h -- depth 1: cells * (16 nchan + sizeof(Real)), depth T: cells *
    (16 nchan / T + 2 sizeof(Real)) -- and the TB/s they give over the measured time (a whole-call rate: launches, the weights' copy and the host
    synchronisation of every add are inside it; it is not a kernel's share of the memory bandwidth).
No threshold is fixed in advance.  The one condition, recorded at the end: PF_ACCUM_DEFAULT_DEPTH is the faster of the measured depths on the plane
cases.  Needs a GPU; there is no fallback.
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from checkpoint_cost import timed  # noqa: E402
from pffdtd_amd import engine, sim_data, synth  # noqa: E402

BATCH = 16


def sample_bytes(cells, nchan, depth, real_bytes):
    return cells * (16 * nchan + real_bytes) if depth == 1 else cells * (16 * nchan / depth + 2 * real_bytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "field_spectra.txt"))
    a = ap.parse_args()
    if engine.device_count() < 1:
        raise SystemExit("no HIP device visible: nothing can be measured here")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = a.size
    nt = 16 + 4 * a.reps + 8
    sd = sim_data.SimData.from_sim(synth.shoebox(n, n, n, Nt=nt, Nm=1, Mb=3), "single", build_mask=False)
    sd.scale_input()
    h, b0 = n // 2, n // 2 - 32
    shapes = [("z plane", ([0, 0, h], [n, n, h + 1]), 64), ("x plane", ([h, 0, 0], [h + 1, n, n]), 64), ("64^3 box", ([b0] * 3, [b0 + 64] * 3), 16)]
    depths = (1, 8, 0)  # 0: the library's default
    say(f"field accumulators: shoebox {n}^3 fp32, ms per sample (wall time of {BATCH} adds and a synchronise, over {BATCH}), median of {a.reps} alternating repetitions")
    plane_wins = {1: 0, 8: 0}
    for name, layout in (("file order", engine.PF_LAYOUT_FILE), ("exchanged axes", engine.PF_LAYOUT_EXCHANGED)):
        eng = engine.HipEngine(sd, layout=layout)
        assert eng.layout()[2] == (layout == engine.PF_LAYOUT_EXCHANGED)
        eng.run(0, 16)
        eng.sync()
        step = 16
        t1, t3 = [], []
        for _ in range(a.reps):  # the engine alone: no accumulator exists yet
            t1.append(timed(lambda: (eng.run(step, 1), eng.sync()))[0] * 1e3)
            step += 1
            t3.append(timed(lambda: (eng.run(step, 3), eng.sync()))[0] * 1e3)
            step += 3
        say(f"{name}: the engine alone: a single step {statistics.median(t1):.3f} ms (min {min(t1):.3f}), a run of three {statistics.median(t3):.3f} ms (min {min(t3):.3f})")
        for label, (lo, hi), nchan in shapes:
            cells = int(np.prod([hi[k] - lo[k] for k in range(3)]))
            w = np.cos(np.arange(nchan) * 0.37)
            accs = {d: eng.accumulator(lo, hi, nchan=nchan, depth=d) for d in depths}

            def batch(acc):
                for _ in range(BATCH):
                    acc.add(w)
                eng.sync()

            ms = {d: [] for d in depths}
            for d in depths:
                batch(accs[d])  # warm-up: the code objects of this depth's fold
            for _ in range(a.reps):
                for d in depths:
                    ms[d].append(timed(lambda: batch(accs[d]))[0] * 1e3 / BATCH)
            med = {d: statistics.median(ms[d]) for d in depths}
            for d in depths:
                dd = d if d else 8  # (bytes of the default: PF_ACCUM_DEFAULT_DEPTH, csrc/pf_accum.h)
                by = sample_bytes(cells, nchan, dd, 4)
                say(f"  {label:9s} {nchan:3d} channels, {'default depth' if d == 0 else f'depth {d:2d}     '}: {med[d]:8.4f} ms per sample (min {min(ms[d]):.4f}, max {max(ms[d]):.4f})   "
                    f"{by / 2**20:8.2f} MiB per sample{'' if d else ' at depth 8'}   {by / (med[d] * 1e-3) / 1e12:6.3f} TB/s   "
                    f"{100 * med[d] / statistics.median(t1):5.1f} % of a single step")
            if "plane" in label:
                plane_wins[1 if med[1] <= med[8] else 8] += 1
            for acc in accs.values():
                assert acc.count == BATCH * (a.reps + 1)
                acc.close()
        eng.close()
    best = 8 if plane_wins[8] > plane_wins[1] else 1
    say(f"plane cases in which depth 8 is faster than depth 1: {plane_wins[8]} of {plane_wins[1] + plane_wins[8]}  ->  the default depth these measurements justify: {best}")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
