"""GPU: energy decay maps from the command line (fdtd_main --decay-planes / --decay-box / --decay-bands, pffdtd_amd/decay.py).

r*_E is infac^2 times the numpy fold -- the contract's three lines per section, squares into the step's bin -- of the frames a second run records
at every step (--field-every 1) over the same regions; a run stopped at a checkpoint and resumed gives the file and the sim_outs.h5 of the run in
one piece, on one device and on a chain of two slabs; without the arguments no file appears.  Every comparison is np.array_equal (or bytes)."""
import numpy as np
import pytest

import cases
from pffdtd_amd import decay, fields, h5io, synth
from test_hip_checkpoint import STOP
from test_hip_region import _cli, _oracle_frames

pytestmark = pytest.mark.gpu
PLANES, BOX, BANDS = "x=13,z=21", "3:26:1,1:20:2,2:22:3", "500,1000"
ARGS = ("--decay-planes", PLANES, "--decay-box", BOX, "--decay-bands", BANDS, "--decay-bin-ms", "1", "--decay-first", "2")


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("regions", "bands", "sampling", "pre_sos", "band_sos")) and a["Ts"] == b["Ts"] and \
        all(x.tobytes() == y.tobytes() for k in ("E", "sums", "state") for x, y in zip(a[k], b[k]))


@pytest.fixture(scope="module")
def whole(tmp_path_factory):
    """the run in one piece on one device, with the decay arguments"""
    d = tmp_path_factory.mktemp("whole")
    synth.write_folder(synth.sort_sim(cases.make_sim("cart_mb11")), d)
    r = _cli(d, *ARGS)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--field decay of 78 samples in 2 bands" in r.stdout and "PF_MULTI_NO_PAIRS" not in r.stdout, r.stdout[-1500:]
    return d


def test_the_file_is_infac_squared_times_the_fold_of_every_frame(whole, tmp_path):
    plain, frames_dir = tmp_path / "plain", tmp_path / "frames"
    for d in (plain, frames_dir):
        d.mkdir()
        synth.write_folder(synth.sort_sim(cases.make_sim("cart_mb11")), d)
    _, ref_out, infac, N = _oracle_frames(plain, set())
    r = _cli(plain)
    assert r.returncode == 0, r.stderr[-2000:]
    assert not (plain / "sim_decay.h5").exists() and "decay" not in r.stdout  # without the arguments: no file, no word
    assert np.array_equal(h5io.read(plain / "sim_outs.h5", "u_out"), ref_out)
    assert h5io.read(whole / "sim_outs.h5", "u_out").tobytes() == h5io.read(plain / "sim_outs.h5", "u_out").tobytes()
    r = _cli(frames_dir, "--field-planes", PLANES, "--field-box", BOX, "--field-every", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    regions, steps, frames = fields.read(frames_dir / "sim_fields.h5")
    f = decay.read(whole / "sim_decay.h5", raw=True)
    specs = fields.parse_planes(PLANES, N) + [fields.parse_box(BOX, N)]
    Nt, first = 80, 2
    Ts = float(h5io.read(whole / "sim_consts.h5", "Ts"))
    bin_steps = int(round(1e-3 / Ts))
    assert steps == list(range(Nt)) and np.array_equal(f["regions"], regions) and [tuple(r) for r in regions] == [lo + hi + st for lo, hi, st in specs]
    assert np.array_equal(f["bands"], [500.0, 1000.0]) and list(f["sampling"]) == [first, bin_steps, Nt - first] and f["Ts"] == Ts
    assert 1 <= bin_steps < Nt - first  # (more than one bin)
    pre, bands = decay.pre_sections(Ts, True, 10.0, 4), decay.band_sections(Ts, [500.0, 1000.0], 3)
    assert np.array_equal(f["pre_sos"], pre) and np.array_equal(f["band_sos"], bands) and pre.shape == (2, 6) and bands.shape == (2, 3, 6)
    nbin = -(-(Nt - first) // bin_steps)

    def section(k, s, x):
        y = k[0] * x + s[0]
        s[0] = (k[1] * x - k[4] * y) + s[1]
        s[1] = k[2] * x - k[5] * y
        return y

    for i in range(len(specs)):
        cells = frames[(i, 0)].shape
        E, state = np.zeros((2, nbin) + cells), np.zeros((2 + 2 * 3, 2) + cells)
        for n in range(first, Nt):
            u = (frames[(i, n)] / infac).astype(np.float32)  # a frame is double(cell) * infac: the division rounds back onto the cell's fp32 value
            assert np.array_equal(u.astype(np.float64) * infac, frames[(i, n)])
            x = u.astype(np.float64)
            for q in range(2):
                x = section(pre[q], state[q], x)
            for b in range(2):
                y = x
                for s in range(3):
                    y = section(bands[b, s], state[2 + 3 * b + s], y)
                k = (n - first) // bin_steps
                E[b, k] = E[b, k] + y * y
        assert np.array_equal(f["sums"][i], E) and np.array_equal(f["state"][i], state), i
        assert np.array_equal(f["E"][i], E * (infac * infac)) and f["E"][i].shape == (2, nbin) + cells
    assert sum(f["E"][i].max() > 0 for i in range(len(specs))) >= 2  # (not zeros against zeros; the ghost plane z = 21 may stay 0)


@pytest.mark.parametrize("devices", [(), ("--devices", "0,0")], ids=["one_device", "two_slabs"])
def test_stopped_and_resumed_equals_the_run_in_one_piece(whole, tmp_path, devices):
    synth.write_folder(synth.sort_sim(cases.make_sim("cart_mb11")), tmp_path)
    r = _cli(tmp_path, *devices, *ARGS, "--stop-after", str(STOP), "--checkpoint", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert ("PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES" in r.stdout) == bool(devices), r.stdout[:1500]
    assert decay.read(tmp_path / "sim_decay.h5")["sampling"][2] == STOP - 2 and not (tmp_path / "sim_outs.h5").exists()
    r = _cli(tmp_path, *devices, *ARGS, "--resume", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert h5io.read(tmp_path / "sim_outs.h5", "u_out").tobytes() == h5io.read(whole / "sim_outs.h5", "u_out").tobytes()
    assert _same(decay.read(whole / "sim_decay.h5", raw=True), decay.read(tmp_path / "sim_decay.h5", raw=True))
    # other bands than the file's: refused by the field's name
    r = _cli(tmp_path, *devices, "--decay-planes", PLANES, "--decay-box", BOX, "--decay-bands", "500", "--decay-bin-ms", "1", "--decay-first", "2", "--resume", "ck.h5")
    assert r.returncode != 0 and "bands" in r.stderr, r.stderr[-1500:]
