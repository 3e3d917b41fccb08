"""GPU: directional band maps of a folded FCC folder from the command line (fdtd_main --dir-stencil lattice, pffdtd_amd/directional.py).

r*_sums is VFold (tests/test_hip_vband.py: the contract's lines in numpy) of the lattice differences (tests/test_hip_vband_fcc.py: their numpy
restatement) of the frames a second run records at every step (--field-every 1) over the regions widened by one cell on all three axes -- where
such a frame holds the fold row Ny - 1, with that row replaced by its row Ny - 2, which is what the contract puts there at an add and what a run
that takes no sample still carries from two steps before (tests/test_hip_vband_fcc.py pins the row itself, on the engine's own frames) --; r*_S is
infac^2 times that with the room's sign in the mirrored cells, r*_iy every cell's physical row; a run stopped at a checkpoint and resumed gives the
file and the sim_outs.h5 of the run in one piece, on one device and on a chain of two slabs; the wrong stencil for the folder is refused by the
flag's name.  Every comparison is np.array_equal (or bytes)."""
import numpy as np
import pytest

import cases
from pffdtd_amd import decay, directional, fields, h5io, sim_data, synth
from test_hip_checkpoint import STOP
from test_hip_region import _cli
from test_hip_vband import VFold
from test_hip_vband_fcc import _components, _wide

pytestmark = pytest.mark.gpu
SCENE = "fcc2_outside"  # 30 x 17 x 26 stored (a room of 32 rows), 60 steps
# the plane y = 8 clear of the faces, a strided box, and a box whose last row y = 15 = Ny - 2 reads the fold row
BOXES = ("1:29:1,8:9:1,1:25:1", "3:27:1,1:15:2,2:24:3", "3:27:2,13:16:1,2:24:3")
WIDE = ("0:30:1,7:10:1,0:26:1", "2:28:1,0:15:1,1:25:1", "2:27:1,12:17:1,1:25:1")  # ... widened by one cell on every axis, stride 1
BANDS, AXES = "500,1000", "y,x"
ARGS = ("--dir-box", BOXES[0], "--dir-box", BOXES[1], "--dir-box", BOXES[2], "--dir-bands", BANDS, "--dir-axes", AXES, "--dir-stencil", "lattice", "--dir-bin-ms", "1",
        "--dir-first", "2")


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("regions", "bands", "axes", "sampling", "pre_sos", "band_sos", "prod")) and a["Ts"] == b["Ts"] and \
        a["stencil"] == b["stencil"] and a["fcc_flag"] == b["fcc_flag"] and all(x.tobytes() == y.tobytes() for k in ("S", "sums", "state", "iy") for x, y in zip(a[k], b[k]))


@pytest.fixture(scope="module")
def whole(tmp_path_factory):
    """the run in one piece on one device, with the directional arguments"""
    d = tmp_path_factory.mktemp("whole")
    synth.write_folder(cases.make_sim(SCENE), d)
    r = _cli(d, *ARGS)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--field directional maps of 58 samples in 2 bands along y,x" in r.stdout and "PF_MULTI_NO_PAIRS" not in r.stdout, r.stdout[-1500:]
    return d


def test_the_file_is_the_fold_of_every_frame_in_room_coordinates(whole, tmp_path):
    synth.write_folder(cases.make_sim(SCENE), tmp_path)
    r = _cli(tmp_path, *[a for w in WIDE for a in ("--field-box", w)], "--field-every", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    assert h5io.read(whole / "sim_outs.h5", "u_out").tobytes() == h5io.read(tmp_path / "sim_outs.h5", "u_out").tobytes()  # the maps change nothing
    _, steps, frames = fields.read(tmp_path / "sim_fields.h5")
    f = directional.read(whole / "sim_directional.h5", raw=True)
    N = tuple(int(h5io.read(whole / "vox_out.h5", k)) for k in ("Nx", "Ny", "Nz"))
    assert N == (30, 17, 26) and int(h5io.read(whole / "sim_consts.h5", "fcc_flag")) == 2
    specs = [fields.parse_box(b, N) for b in BOXES]
    for s, w in zip(specs, WIDE):
        assert tuple(tuple(v) for v in _wide(s)) == tuple(tuple(v) for v in fields.parse_box(w, N))
    Nt, first = 60, 2
    Ts = float(h5io.read(whole / "sim_consts.h5", "Ts"))
    h, c = float(h5io.read(whole / "sim_consts.h5", "h")), float(h5io.read(whole / "sim_consts.h5", "c"))
    sd = sim_data.SimData.from_folder(whole, "single")
    sd.scale_input()
    infac = float(sd.infac)
    bin_steps = int(round(1e-3 / Ts))
    assert steps == list(range(Nt)) and [tuple(r) for r in f["regions"]] == [lo + hi + st for lo, hi, st in specs]
    assert f["stencil"] == "lattice" and f["fcc_flag"] == 2 and list(f["axes"]) == [2, 1] and list(f["sampling"]) == [first, bin_steps, Nt - first] and f["Ts"] == Ts
    assert 1 <= bin_steps < Nt - first  # (more than one bin)
    omni, grad = directional.gradient_sections(Ts, h, c, True, 10.0, 4, span=8)
    pre, bands, prod = np.stack([omni, grad, grad]), decay.band_sections(Ts, [500.0, 1000.0], 3), directional.products(2)
    assert np.array_equal(f["pre_sos"], pre) and np.array_equal(f["band_sos"], bands) and np.array_equal(f["prod"], prod)
    comp = (0, 5, 4)
    nbin = -(-(Nt - first) // bin_steps)
    signed = stale = 0
    for i, spec in enumerate(specs):
        cells = tuple(-(-(spec[1][a] - spec[0][a]) // spec[2][a]) for a in range(3))
        want = VFold(3, pre, bands, prod, nbin, cells)
        for n in range(first, Nt):
            u = (frames[(i, n)] / infac).astype(np.float32)  # a frame is double(cell) * infac: the division rounds back onto the cell's fp32 value
            assert np.array_equal(u.astype(np.float64) * infac, frames[(i, n)])
            if _wide(spec)[1][1] == N[1]:  # the frame's last row is the fold row: the copy of row Ny - 2 of the same field
                stale += int(np.count_nonzero(u[:, -1, :] != u[:, -2, :]))
                u[:, -1, :] = u[:, -2, :]
            want.add(_components(u, spec, comp), (n - first) // bin_steps)
        assert np.array_equal(f["sums"][i], want.S) and np.array_equal(f["state"][i], want.state), i
        _, iy, _, upper = directional.fold_coordinates(spec, N[1])
        assert np.array_equal(f["iy"][i], iy) and upper.any() and not upper.all()
        S = want.S * (infac * infac)
        S[2][..., upper] = -S[2][..., upper]  # (0, y) plain: the stored +y of a mirrored cell is the room's -y
        assert np.array_equal(f["S"][i], S) and f["S"][i].shape == (7, 2, nbin) + cells
        assert f["S"][i][0].max() > 0 and f["S"][i][1].max() > 0 and f["S"][i][2].min() < 0 and f["S"][i][5].min() < 0
        signed += int(np.count_nonzero(f["S"][i][2][..., upper]))
    assert signed > 0
    print(f"cells of the fold row that a run without samples carried from an earlier step: {stale}")
    # (7 steps of this coarse scene are 1.019 ms, outside the 1 % within which parameters takes a bin for a whole fraction of 5 ms: the nominal bin)
    out = directional.parameters(f["S"][0], f["prod"], 1e-3)
    assert out["LF"].shape == (2, 2) + f["S"][0].shape[3:] and np.nanmax(out["LF"]) > 0


@pytest.mark.parametrize("devices", [(), ("--devices", "0,0")], ids=["one_device", "two_slabs"])
def test_stopped_and_resumed_equals_the_run_in_one_piece(whole, tmp_path, devices):
    synth.write_folder(cases.make_sim(SCENE), tmp_path)
    r = _cli(tmp_path, *devices, *ARGS, "--stop-after", str(STOP), "--checkpoint", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert ("PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES" in r.stdout) == bool(devices), r.stdout[:1500]
    assert directional.read(tmp_path / "sim_directional.h5")["sampling"][2] == STOP - 2 and not (tmp_path / "sim_outs.h5").exists()
    r = _cli(tmp_path, *devices, *ARGS, "--resume", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert h5io.read(tmp_path / "sim_outs.h5", "u_out").tobytes() == h5io.read(whole / "sim_outs.h5", "u_out").tobytes()
    assert _same(directional.read(whole / "sim_directional.h5", raw=True), directional.read(tmp_path / "sim_directional.h5", raw=True))
    # a region on a face: refused by the axis's name, whichever axis the gradient is along
    r = _cli(tmp_path, *devices, "--dir-planes", "x=13", "--dir-bands", BANDS, "--dir-axes", "x", "--dir-stencil", "lattice")
    assert r.returncode != 0 and "along file y" in r.stderr and "lattice" in r.stderr, r.stderr[-1500:]


def test_the_two_refusals_of_the_flag(tmp_path):
    fcc, cart = tmp_path / "fcc", tmp_path / "cart"
    synth.write_folder(cases.make_sim(SCENE), fcc)
    synth.write_folder(synth.sort_sim(cases.make_sim("cart_mb11")), cart)
    r = _cli(cart, "--dir-box", "1:25:1,10:11:1,1:21:1", "--dir-bands", BANDS, "--dir-stencil", "lattice")
    assert r.returncode != 0 and "--dir-stencil lattice" in r.stderr and "fcc_flag" in r.stderr, r.stderr[-1500:]
    for extra in ((), ("--dir-stencil", "axis")):  # the default is axis: refused as before, and the message points to the flag
        r = _cli(fcc, "--dir-box", BOXES[0], "--dir-bands", BANDS, *extra)
        assert r.returncode != 0 and "fcc_flag" in r.stderr and "--dir-stencil lattice" in r.stderr, r.stderr[-1500:]
    assert not (fcc / "sim_directional.h5").exists() and not (cart / "sim_directional.h5").exists()
    r = _cli(cart, "--dir-stencil", "lattice")
    assert r.returncode != 0 and "--dir-stencil" in r.stderr, r.stderr[-1500:]  # the flag alone names no region
