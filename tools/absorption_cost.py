#!/usr/bin/env python3
"""What the wall absorption maps cost per step: time per single step with and without the observer (pf_engine_absorb_add before every step), and
the wall kernel's bytes per node.

  tools/absorption_cost.py [--size 1024] [--fcc-size 512] [--batch 12] [--reps 7] [--out profiles/absorption_cost.txt]

Two grids, each in a process of its own under a time limit of its own (the first that fails ends the measurement): the headline shoebox size^3,
fp32, Mb = 11 (synth.shoebox as bench.py builds it), and a folded-FCC grid fcc_size x (2 fcc_size - 2) x fcc_size before folding.  In each, on one
engine with its default options, after a warm-up of one batch of each kind:
  * plain:    `batch` calls run(n, 1), then a device synchronise;
  * observed: `batch` times run(n, 1) then add(n + 1, bin), then the same synchronise (the add is enqueued, never waited for); the priming add is
    taken before the clock starts, so every timed add accounts a step;
the two ALTERNATE for --reps repetitions, wall time per batch over `batch`; reported: the medians, the minima and the ratio of the medians.
No threshold is fixed in advance; the number to beat is the plain single step of the same process.  The bytes per node are counted from the
kernel's accesses (csrc/pf_absorb.h), not measured.  Needs a GPU; there is no fallback.
"""
import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def child(a):
    from pffdtd_amd import absorption, engine, sim_data, synth
    if engine.device_count() < 1:
        raise SystemExit("no HIP device visible: nothing can be measured here")
    n, nt = a.size, (2 * a.reps + 3) * a.batch + 1
    if a.child == "fcc":
        sim = synth.shoebox(n, 2 * (n - 1), n, Nt=nt, fcc=True, Nm=1, Mb=11)
        sim = synth.fold_fcc(sim) or sim
        name = f"folded FCC {n} x {2 * (n - 1)} x {n} before folding"
    else:
        sim = synth.shoebox(n, n, n, Nt=nt, Nm=1, Mb=11)
        name = f"shoebox {n}^3"
    sd = sim_data.SimData.from_sim(sim, "single", build_mask=False)
    sd.scale_input()
    eng = engine.HipEngine(sd)
    obs = eng.absorption(*absorption.scales(sd), nbin=4)
    step = [0]

    def batch(observed):
        if observed:  # (the plain batch before left a gap: prime again, outside the timed region -- every timed sample accounts a step)
            obs.set(None, 0)
            obs.add(step[0], 0)
            eng.sync()
        t0 = time.perf_counter()
        for _ in range(a.batch):
            eng.run(step[0], 1)
            step[0] += 1
            if observed:
                obs.add(step[0], step[0] % 4)
        eng.sync()
        return (time.perf_counter() - t0) * 1e3 / a.batch

    batch(False)
    batch(True)
    ms = {False: [], True: []}
    for _ in range(a.reps):
        ms[False].append(batch(False))
        ms[True].append(batch(True))
    med = {k: statistics.median(v) for k, v in ms.items()}
    real = 4
    per_node = 3 * 11 * real + 16 + real + 1
    print(f"{name}, fp32, Mb = 11: Nbl = {sd.Nbl} frequency-dependent nodes, Nba = {sd.Nba} ABC nodes, {sd.Ns} source nodes")
    print(f"  single step, plain:    median {med[False]:.4f} ms (min {min(ms[False]):.4f}) over {a.reps} batches of {a.batch}")
    print(f"  single step, observed: median {med[True]:.4f} ms (min {min(ms[True]):.4f}), alternating with the plain batches")
    print(f"  overhead: observed / plain = {med[True] / med[False]:.4f} ({med[True] - med[False]:+.4f} ms per step)")
    print(f"  wall kernel: {per_node} B per node counted (vh1, prev read, prev written: 3 x 11 x {real}; node_sum read + written: 16; ssaf {real}; material 1) = "
          f"{per_node * sd.Nbl / 1e6:.1f} MB per sample")
    eng.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=1024)
    p.add_argument("--fcc-size", type=int, default=512)
    p.add_argument("--batch", type=int, default=12)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--out", default=str(ROOT / "profiles" / "absorption_cost.txt"))
    p.add_argument("--limit", type=int, default=420, help="seconds per process")
    p.add_argument("--child", default="")
    a = p.parse_args()
    if a.child:
        return child(a)
    lines = [f"tools/absorption_cost.py --size {a.size} --fcc-size {a.fcc_size} --batch {a.batch} --reps {a.reps}",
             "wall time per step around batches of run(n, 1) that end in a device synchronise; plain and observed batches alternate; one process per grid"]
    for kind, size in (("cart", a.size), ("fcc", a.fcc_size)):
        r = subprocess.run([sys.executable, __file__, "--child", kind, "--size", str(size), "--batch", str(a.batch), "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=a.limit)
        if r.returncode != 0:
            print(r.stdout + r.stderr[-3000:])
            raise SystemExit(f"the {kind} measurement failed (exit status {r.returncode}): nothing more is started")
        lines += r.stdout.rstrip().split("\n")
    text = "\n".join(lines) + "\n"
    Path(a.out).parent.mkdir(exist_ok=True)
    Path(a.out).write_text(text)
    print(text, end="")


if __name__ == "__main__":
    main()
