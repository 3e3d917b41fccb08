#!/usr/bin/env python3
"""What a vector band accumulator costs per sample, which depth of its ring is fastest, and what it costs beside a band accumulator on the same
region and bands: pf_engine_vband_add against pf_engine_bandacc_add and the engine's own steps.

  tools/field_directional_cost.py [--size 512] [--reps 7] [--out profiles/field_directional.txt]
  tools/field_directional_cost.py --fcc [--size 512] [--reps 7] [--out profiles/field_directional_fcc.txt]

On a shoebox size^3, fp32 (synth.shoebox), once stored in file order and once with the x and z axes exchanged, in one process:
  * a z plane of (size - 2)^2 cells (one cell clear of the x and y faces, as the difference components need) and a 64^3 box, 6 octave bands of 3
    sections each and 3 sections per component (what pffdtd_amd/directional.py builds for order 3 and the integrator + low-cut of order 4), 40 time
    bins, the bin changing every 16 samples;
  * omni + the difference along y (2 components, 4 products) and omni + all three axes (4 components, 10 products);
  * ms per sample at depths 1, 2, 4 and 8: wall time around 16 adds that end in a device synchronise (16 is a multiple of every depth measured, so
    every timing holds whole folds), over 16, after a warm-up of the same 16; the median of --reps repetitions in which the depths ALTERNATE;
  * in the same alternation the EXISTING band accumulator (its default depth) on the same region and bands, and beside them the engine's wall
    time per single step (run(n, 1)) without any accumulator call in between.
--fcc: the same measurement on a FOLDED FCC shoebox, size x (size / 2 + 1) x size stored, with the lattice differences (comp 4 / 5 / 6, one
k_region_lat launch per sample for all of them) in the differences' place: the plane and the box one cell clear of ALL faces, omni + y and
omni + x, y, z, the gradient sections with span = 8.
No threshold is fixed in advance: the figures are written down, not gated.  Recorded at the end: the depth with the smallest sum of medians over
the plane cases, which PF_VBAND_DEFAULT_DEPTH (csrc/pf_vband.h) is to equal.  Needs a GPU; there is no fallback.
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
from pffdtd_amd import decay, directional, engine, sim_data, synth  # noqa: E402

BATCH = 16
DEPTHS = (1, 2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--fcc", action="store_true", help="a folded FCC grid and the lattice differences")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    a.out = a.out or str(ROOT / "profiles" / ("field_directional_fcc.txt" if a.fcc else "field_directional.txt"))
    if engine.device_count() < 1:
        raise SystemExit("no HIP device visible: nothing can be measured here")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = a.size
    sim = synth.shoebox(n, n, n, Nt=16 + a.reps + 8, fcc=a.fcc, Nm=1, Mb=3)
    if a.fcc:
        synth.sort_sim(synth.fold_fcc(sim))
    sd = sim_data.SimData.from_sim(sim, "single", build_mask=False)
    sd.scale_input()
    ny = int(sd.Ny)  # (folded: size / 2 + 1 stored rows)
    Ts = 1.0 / 25500.0
    c = 343.0
    omni, grad = directional.gradient_sections(Ts, c * Ts * (1.0 if a.fcc else 3.0 ** 0.5), c, True, 10.0, 4, span=directional.LATTICE_SPAN if a.fcc else 2)
    bands = decay.band_sections(Ts, [125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0], 3)
    assert omni.shape == (3, 6) and bands.shape == (6, 3, 6)
    h, b0 = n // 2, n // 2 - 32
    by = min(b0, ny - 65)
    shapes = [(f"{n - 2} x {ny - 2} z plane" if a.fcc else f"{n - 2}^2 z plane", ([1, 1, h], [n - 1, ny - 1, h + 1])), ("64^3 box", ([b0, by, b0], [b0 + 64, by + 64, b0 + 64]))]
    comps = [("omni + y", (0, 5)), ("omni + x, y, z", (0, 4, 5, 6))] if a.fcc else [("omni + y", (0, 2)), ("omni + x, y, z", (0, 1, 2, 3))]
    nbin = 40
    say(f"vector band accumulators: {f'folded FCC shoebox {n} x {ny} x {n} stored, lattice differences,' if a.fcc else f'shoebox {n}^3'} fp32, 6 bands x 3 sections + 3 per component, ms per sample (wall time of {BATCH} adds and a synchronise, over {BATCH}), "
        f"median of {a.reps} alternating repetitions; 'bandacc': the band accumulator (one component, its square; 3 shared sections, default depth) on the same region and bands")
    plane_sum = {d: 0.0 for d in DEPTHS}
    for name, layout in (("file order", engine.PF_LAYOUT_FILE), ("exchanged axes", engine.PF_LAYOUT_EXCHANGED)):
        eng = engine.HipEngine(sd, layout=layout)
        assert eng.layout()[2] == (layout == engine.PF_LAYOUT_EXCHANGED)
        eng.run(0, 16)
        eng.sync()
        step = 16
        t1 = []
        for _ in range(a.reps):  # the engine alone: no accumulator exists yet
            t1.append(timed(lambda: (eng.run(step, 1), eng.sync()))[0] * 1e3)
            step += 1
        say(f"{name}: the engine alone: a single step {statistics.median(t1):.3f} ms (min {min(t1):.3f})")
        for label, (lo, hi) in shapes:
            for cname, comp in comps:
                pre = np.stack([omni] + [grad] * (len(comp) - 1))
                prod = directional.products(len(comp) - 1)
                accs = {d: eng.vector_band_accumulator(lo, hi, comp=comp, pre_sos=pre, band_sos=bands, prod=prod, nbin=nbin, depth=d) for d in DEPTHS}
                accs["bandacc"] = eng.band_accumulator(lo, hi, pre_sos=omni, band_sos=bands, nbin=nbin)
                keys = list(DEPTHS) + ["bandacc"]
                batches = {k: 0 for k in keys}

                def batch(k):
                    for _ in range(BATCH):
                        accs[k].add(batches[k] % nbin)
                    eng.sync()
                    batches[k] += 1

                ms = {k: [] for k in keys}
                for k in keys:
                    batch(k)  # warm-up: the code objects of this depth's fold
                for _ in range(a.reps):
                    for k in keys:
                        ms[k].append(timed(lambda: batch(k))[0] * 1e3 / BATCH)
                med = {k: statistics.median(ms[k]) for k in keys}
                for k in keys:
                    tag = f"depth {k:2d}" if k != "bandacc" else "bandacc "
                    say(f"  {label:13s} {cname:15s} {tag}: {med[k]:8.4f} ms per sample (min {min(ms[k]):.4f}, max {max(ms[k]):.4f})   {100 * med[k] / statistics.median(t1):5.1f} % of a single step"
                        + (f"   {med[k] / med['bandacc']:5.2f} x bandacc" if k != "bandacc" else ""))
                    if "plane" in label and k != "bandacc":
                        plane_sum[k] += med[k]
                for acc in accs.values():
                    assert acc.count == BATCH * (a.reps + 1)
                    acc.close()
        eng.close()
    best = min(DEPTHS, key=lambda d: plane_sum[d])
    say("sum of the plane cases' medians per depth: " + ", ".join(f"{d}: {plane_sum[d]:.4f} ms" for d in DEPTHS) + f"  ->  the default depth these measurements justify: {best}")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
