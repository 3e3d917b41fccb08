"""GPU: directional band maps from the command line (fdtd_main --dir-planes / --dir-box / --dir-bands / --dir-axes, pffdtd_amd/directional.py).

r*_S is infac^2 times VFold (tests/test_hip_vband.py: the contract's lines in numpy) of the frames a second run records at every step
(--field-every 1) over the regions widened by one cell along the chosen axes; a run stopped at a checkpoint and resumed gives the file and the
sim_outs.h5 of the run in one piece, on one device and on a chain of two slabs (whose cut the difference along x crosses); without the arguments
no file appears.  Every comparison is np.array_equal (or bytes)."""
import numpy as np
import pytest

import cases
from pffdtd_amd import decay, directional, fields, h5io, synth
from test_hip_checkpoint import STOP
from test_hip_region import _cli, _oracle_frames
from test_hip_vband import VFold, _components, _widened

pytestmark = pytest.mark.gpu
BOXES = ("1:25:1,10:11:1,1:21:1", "3:25:1,1:19:2,2:21:3")  # (cart_mb11 is 26 x 20 x 22) the plane y = 10 clear of the x and z faces, and a strided box
WIDE = ("0:26:1,9:12:1,1:21:1", "2:26:1,0:19:1,2:21:3")    # ... widened by one cell along y and x, stride 1 there
BANDS, AXES = "500,1000", "y,x"
ARGS = ("--dir-box", BOXES[0], "--dir-box", BOXES[1], "--dir-bands", BANDS, "--dir-axes", AXES, "--dir-bin-ms", "1", "--dir-first", "2")


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("regions", "bands", "axes", "sampling", "pre_sos", "band_sos", "prod")) and a["Ts"] == b["Ts"] and \
        all(x.tobytes() == y.tobytes() for k in ("S", "sums", "state") for x, y in zip(a[k], b[k]))


@pytest.fixture(scope="module")
def whole(tmp_path_factory):
    """the run in one piece on one device, with the directional arguments"""
    d = tmp_path_factory.mktemp("whole")
    synth.write_folder(synth.sort_sim(cases.make_sim("cart_mb11")), d)
    r = _cli(d, *ARGS)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--field directional maps of 78 samples in 2 bands along y,x" in r.stdout and "PF_MULTI_NO_PAIRS" not in r.stdout, r.stdout[-1500:]
    return d


def test_the_file_is_infac_squared_times_the_fold_of_every_frame(whole, tmp_path):
    plain, frames_dir = tmp_path / "plain", tmp_path / "frames"
    for d in (plain, frames_dir):
        d.mkdir()
        synth.write_folder(synth.sort_sim(cases.make_sim("cart_mb11")), d)
    _, ref_out, infac, N = _oracle_frames(plain, set())
    r = _cli(plain)
    assert r.returncode == 0, r.stderr[-2000:]
    assert not (plain / "sim_directional.h5").exists() and "directional" not in r.stdout  # without the arguments: no file, no word
    assert np.array_equal(h5io.read(plain / "sim_outs.h5", "u_out"), ref_out)
    assert h5io.read(whole / "sim_outs.h5", "u_out").tobytes() == h5io.read(plain / "sim_outs.h5", "u_out").tobytes()
    r = _cli(frames_dir, "--field-box", WIDE[0], "--field-box", WIDE[1], "--field-every", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    _, steps, frames = fields.read(frames_dir / "sim_fields.h5")
    f = directional.read(whole / "sim_directional.h5", raw=True)
    specs = [fields.parse_box(b, N) for b in BOXES]
    comp = (0, 2, 1)
    for s, w in zip(specs, WIDE):
        assert tuple(tuple(v) for v in _widened(s, comp)) == tuple(tuple(v) for v in fields.parse_box(w, N))
    Nt, first = 80, 2
    Ts = float(h5io.read(whole / "sim_consts.h5", "Ts"))
    h, c = float(h5io.read(whole / "sim_consts.h5", "h")), float(h5io.read(whole / "sim_consts.h5", "c"))
    bin_steps = int(round(1e-3 / Ts))
    assert steps == list(range(Nt)) and [tuple(r) for r in f["regions"]] == [lo + hi + st for lo, hi, st in specs]
    assert np.array_equal(f["bands"], [500.0, 1000.0]) and list(f["axes"]) == [2, 1] and list(f["sampling"]) == [first, bin_steps, Nt - first] and f["Ts"] == Ts
    assert 1 <= bin_steps < Nt - first  # (more than one bin)
    omni, grad = directional.gradient_sections(Ts, h, c, True, 10.0, 4)
    pre, bands, prod = np.stack([omni, grad, grad]), decay.band_sections(Ts, [500.0, 1000.0], 3), directional.products(2)
    assert np.array_equal(f["pre_sos"], pre) and np.array_equal(f["band_sos"], bands) and np.array_equal(f["prod"], prod) and pre.shape == (3, 3, 6)
    nbin = -(-(Nt - first) // bin_steps)
    for i, spec in enumerate(specs):
        cells = tuple(-(-(spec[1][a] - spec[0][a]) // spec[2][a]) for a in range(3))
        want = VFold(3, pre, bands, prod, nbin, cells)
        for n in range(first, Nt):
            u = (frames[(i, n)] / infac).astype(np.float32)  # a frame is double(cell) * infac: the division rounds back onto the cell's fp32 value
            assert np.array_equal(u.astype(np.float64) * infac, frames[(i, n)])
            want.add(_components(u, spec, comp), (n - first) // bin_steps)
        assert np.array_equal(f["sums"][i], want.S) and np.array_equal(f["state"][i], want.state), i
        assert np.array_equal(f["S"][i], want.S * (infac * infac)) and f["S"][i].shape == (7, 2, nbin) + cells
        assert f["S"][i][0].max() > 0 and f["S"][i][1].max() > 0 and f["S"][i][2].min() < 0  # (not zeros against zeros; a plain product takes both signs)
    out = directional.parameters(f["S"][0], f["prod"], bin_steps * Ts)
    assert out["LF"].shape == (2, 2) + f["S"][0].shape[3:] and np.nanmax(out["LF"]) > 0


@pytest.mark.parametrize("devices", [(), ("--devices", "0,0")], ids=["one_device", "two_slabs"])
def test_stopped_and_resumed_equals_the_run_in_one_piece(whole, tmp_path, devices):
    synth.write_folder(synth.sort_sim(cases.make_sim("cart_mb11")), tmp_path)
    r = _cli(tmp_path, *devices, *ARGS, "--stop-after", str(STOP), "--checkpoint", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert ("PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES" in r.stdout) == bool(devices), r.stdout[:1500]
    assert directional.read(tmp_path / "sim_directional.h5")["sampling"][2] == STOP - 2 and not (tmp_path / "sim_outs.h5").exists()
    r = _cli(tmp_path, *devices, *ARGS, "--resume", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert h5io.read(tmp_path / "sim_outs.h5", "u_out").tobytes() == h5io.read(whole / "sim_outs.h5", "u_out").tobytes()
    assert _same(directional.read(whole / "sim_directional.h5", raw=True), directional.read(tmp_path / "sim_directional.h5", raw=True))
    # other axes than the file's: refused by the field's name; a whole plane along a chosen axis: refused by the axis's name
    r = _cli(tmp_path, *devices, *[v if v != AXES else "y" for v in ARGS], "--resume", "ck.h5")
    assert r.returncode != 0 and "axes" in r.stderr, r.stderr[-1500:]
    r = _cli(tmp_path, *devices, "--dir-planes", "x=13", "--dir-bands", BANDS, "--dir-axes", "y")
    assert r.returncode != 0 and "along file y" in r.stderr, r.stderr[-1500:]
