"""GPU: the wall absorption maps from the command line (fdtd_main --absorption [--absorption-bin-ms] [--absorption-first], pffdtd_amd/absorption.py) on a
written folder of the cart_lossy scene of the energy fixtures (fp64: the scene's input is not differentiated).

  * the file's arrays are the reference Python engine's (tests/golden/absorption_cart_lossy.npz) after the infac^2 rule -- the command line scales
    the input by 1 / infac, the file multiplies the sums by infac^2 -- to 1e-9 of each series' peak, the tolerance of tests/test_hip_energy.py;
  * a chain of two slabs (--devices 0,0: the suite's boxes may hold one GPU, and --gpus 2 is the same chain on devices 0, 1) gives the same nodes bit
    for bit and the same bins within the bounds of tests/test_hip_absorb.py;
  * a run stopped mid-bin at a checkpoint and resumed gives the file of the run in one piece, byte for byte.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

from pffdtd_amd import absorption, engine, h5io, sim_data, synth
from test_hip_absorb import EPS, _host_terms, _observe, _run
from test_hip_checkpoint import _cli

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
from energy_cases import ENERGY_CASES  # noqa: E402

DOUBLE = ("--precision", "double")


def _folder(d):
    synth.write_folder(synth.shoebox(**ENERGY_CASES["cart_lossy"]), d)
    return d


def _one_step_bins(d):
    sd = sim_data.SimData.from_folder(d, "double", build_mask=False)
    return sd, ("--absorption", "--absorption-bin-ms", f"{sd.Ts * 1e3:.12g}")


@pytest.fixture(scope="module")
def whole(tmp_path_factory):
    d = _folder(tmp_path_factory.mktemp("absorb_whole"))
    sd, args = _one_step_bins(d)
    r = _cli(d, *DOUBLE, *args)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"--field wall absorption of {sd.Nt} steps, 2 materials, bins of 1 steps" in r.stdout and "PF_MULTI_NO_PAIRS" not in r.stdout, r.stdout[-1500:]
    return d


def test_the_file_is_the_references_split(whole):
    g = np.load(GOLDEN / "absorption_cart_lossy.npz")
    sd = sim_data.SimData.from_folder(whole, "double", build_mask=False)
    f = absorption.read(whole / "sim_absorption.h5", raw=True)
    assert list(f["sampling"]) == [0, 1, sd.Nt] and f["bin_seconds"] == sd.Ts and f["Nm"] == 2
    assert np.array_equal(f["bnl_ixyz"], sd.bnl_ixyz) and np.array_equal(f["mat_bnl"], sd.mat_bnl)
    infac = sd.scale_input()
    assert infac != 1.0 and np.array_equal(f["materials"], f["raw_materials"] * (infac * infac))
    for key, ref in (("materials", g["materials"]), ("open_boundary", g["open_boundary"]), ("input", g["input"]), ("nodes", g["wall_nodes"].sum(0))):
        err, scale = np.abs(f[key] - ref).max(), max(np.abs(ref).max(), 1e-300)
        print(f"{key}: max |difference| {err:.3e}, peak {scale:.3e}")
        assert f[key].shape == ref.shape and err <= 1e-9 * scale, key
    p = absorption.parameters(f["materials"], f["open_boundary"], f["input"])
    assert np.all(p["remaining"] >= -1e-9 * f["input"].sum()) and (f["materials"].sum(0) > 0).all()
    ix, iy, iz, e = absorption.node_map(f, sd.Ny, sd.Nz)
    assert e.size == sd.Nbl and np.array_equal((ix * sd.Ny + iy) * sd.Nz + iz, sd.bnl_ixyz)


def test_a_chain_of_two_slabs_gives_the_same_file_contents(whole, tmp_path):
    d = _folder(tmp_path)
    sd, args = _one_step_bins(d)
    r = _cli(d, *DOUBLE, "--devices", "0,0", *args)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--field absorption: the chain is created with PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES" in r.stdout, r.stdout[:1500]
    one, two = absorption.read(whole / "sim_absorption.h5", raw=True), absorption.read(d / "sim_absorption.h5", raw=True)
    assert two["raw_nodes"].tobytes() == one["raw_nodes"].tobytes() and two["nodes"].tobytes() == one["nodes"].tobytes()
    assert np.all(np.abs(two["raw_materials"] - one["raw_materials"]) <= sd.Nbl * EPS * one["raw_materials"])
    assert np.all(np.abs(two["raw_open_boundary"] - one["raw_open_boundary"]) <= sd.Nba * EPS * one["raw_open_boundary"])
    # the input row's bound needs the sum of |terms| per step: restated from an engine's saved states, with the command line's scaled input
    sd.scale_input()
    eng = engine.HipEngine(sd)
    a = _observe(eng, sd, sd.Nt)
    states = {}
    _run(eng, a, 0, sd.Nt, lambda s: s, between=lambda n: states.__setitem__(n, eng.save_state()))
    eng.close()
    scales = absorption.scales(sd)
    in_abs = np.array([np.abs(_host_terms(sd, scales, states[s], states[s + 1], s)[2]).sum() for s in range(sd.Nt)])
    assert np.all(np.abs(two["raw_input"] - one["raw_input"]) <= sd.Ns * EPS * in_abs)
    assert h5io.read(d / "sim_outs.h5", "u_out").tobytes() == h5io.read(whole / "sim_outs.h5", "u_out").tobytes()


def test_stopped_and_resumed_gives_the_file_of_the_run_in_one_piece(tmp_path):
    one, parts = _folder(tmp_path / "one"), _folder(tmp_path / "parts")
    args = ("--absorption", "--absorption-bin-ms", "1.0", "--absorption-first", "3")
    sd = sim_data.SimData.from_folder(one, "double", build_mask=False)
    per_bin = int(round(1e-3 / sd.Ts))
    stop = 3 + per_bin + per_bin // 2  # inside the second bin
    assert per_bin >= 2 and stop + per_bin < sd.Nt  # (a bin boundary lies in the second part)
    r = _cli(one, *DOUBLE, *args)
    assert r.returncode == 0, r.stderr[-2000:]
    r = _cli(parts, *DOUBLE, *args, "--stop-after", str(stop), "--checkpoint", "ck.h5")
    assert r.returncode == 0 and not (parts / "sim_outs.h5").exists(), r.stderr[-2000:]
    f = absorption.read(parts / "sim_absorption.h5")
    assert list(f["sampling"]) == [3, per_bin, stop - 3] and not f["materials"][2:].any() and f["materials"][1].any()
    r = _cli(parts, *DOUBLE, *args, "--resume", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert (parts / "sim_absorption.h5").read_bytes() == (one / "sim_absorption.h5").read_bytes()
    assert h5io.read(parts / "sim_outs.h5", "u_out").tobytes() == h5io.read(one / "sim_outs.h5", "u_out").tobytes()
    assert list(absorption.read(one / "sim_absorption.h5")["sampling"]) == [3, per_bin, sd.Nt - 3]
    # another bin width than the file's: refused by the field's name
    r = _cli(parts, *DOUBLE, "--absorption", "--absorption-bin-ms", "2.0", "--absorption-first", "3", "--resume", "ck.h5")
    assert r.returncode != 0 and "bin_steps" in r.stderr, r.stderr[-1500:]
