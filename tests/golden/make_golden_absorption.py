#!/usr/bin/env python3
"""Golden vectors of the wall absorption maps: the reference PYTHON engine's per-step loss terms (python/fdtd/sim_fdtd.py:615-620), split the way
pffdtd_amd's absorption output splits them, for the scenes of energy_cases.py.  The reference is run by make_golden_energy.run_reference behind
that module's shims (this container only); its run_steps is wrapped to read, after every step, the state it leaves; the input row is the
reference's own E_in series.  Nothing of the reference is copied: the fixtures hold the scene's digest + outputs,
  wall_nodes [Nt, Nbl]   V_fac * 0.25 * h / l * ssaf_i * sum_m ((vh0 + vh1)^2 * E)_{i,m} per step, rows in the order of bnl_ixyz
  materials  [Nt, Nm]    the same summed per material
  open_boundary [Nt]     0.5 * V_fac * h / l * sum (2^-Q * Q) * (u^{n+1} - u^{n-1})^2 over the ABC nodes
  input [Nt]             0.5 * V_fac * h / l2 * sum (u^{n+1} - u^{n-1}) * in_sigs[:, n] over the sources
"""
from pathlib import Path

import numpy as np

import make_golden_energy as mge  # (sets up the shims and sys.path)
from make_golden import digest
from energy_cases import ENERGY_CASES

HERE = Path(__file__).resolve().parent


def run_split(sim):
    """-> (the split per step, E_lost, E_in).  The input row is the reference's own series, np.diff(E_in); the wall and ABC rows are computed here from
    the state the reference leaves after each step (e.vh0 / e.vh1: the branch currents before / after it, e.u1 = u^{n+1}, e.u2ba = u^{n-1} at the ABC
    nodes), and main() holds their sum to np.diff(E_lost)."""
    rec = {"wall_nodes": [], "materials": [], "open_boundary": []}
    plain = mge.SimEngine.run_steps

    def spy(e, n, nsteps):
        plain(e, n, nsteps)
        unit = (2.0 if e.fcc else 1.0) * e.h / e.l  # V_fac h / l
        current = e.vh0 + e.vh1
        wall = (0.25 * unit) * e.ssaf_bnl * np.einsum("im,im,im->i", current, current, e.E_bnl)
        rec["wall_nodes"].append(wall)
        rec["materials"].append(np.array([wall[e.mat_bnl == k].sum() for k in range(e.Nm)]))
        q = np.asarray(e.Q_bna, dtype=np.float64)
        rise = e.u1.reshape(-1)[e.bna_ixyz] - e.u2ba
        rec["open_boundary"].append((0.5 * unit) * np.dot(q * np.exp2(-q), rise * rise))

    mge.SimEngine.run_steps = spy
    try:
        _, _, El, Ei = mge.run_reference(sim)
    finally:
        mge.SimEngine.run_steps = plain
    out = {k: np.array(v) for k, v in rec.items()}
    out["input"] = np.diff(Ei)
    return out, El, Ei


def main():
    from pffdtd_amd import synth
    for name, kw in ENERGY_CASES.items():
        sim = synth.shoebox(**kw)
        rec, El, Ei = run_split(sim)
        lost = rec["materials"].sum(1) + rec["open_boundary"]
        out = HERE / f"absorption_{name}.npz"
        np.savez_compressed(out, digest=np.array(digest(sim)), **rec)
        print(f"{out.name}: Nbl {rec['wall_nodes'].shape[1]}  max|lost - diff(E_lost)| {np.abs(lost - np.diff(El)).max():.3e} of {np.diff(El).max():.3e}"
              f"  {out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
