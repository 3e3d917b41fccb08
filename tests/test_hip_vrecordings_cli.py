"""GPU: B-format field recordings from the command line (fdtd_main --rec-planes / --rec-box ... --rec-axes x,y,z [--rec-stencil], pffdtd_amd/recordings.py).

The file's frames are infac times one `Decim` per channel (tests/test_recordings_host.py) over `_components` (tests/test_hip_vband.py) of the frames
a second run records at every step (--field-every 1) over the widened regions, rounded to the file's float32; W is also `Decim` over the oracle's row of
a receiver in the cell; a second run gives the same file; a run stopped at a checkpoint and resumed gives the file of the run in one piece, on one
device and on a chain of two slabs; without --rec-axes the file is the scalar recorder's.  A folded FCC folder with --rec-stencil lattice --rec-axes y:
the y channel is +-infac times `Decim` over the lattice difference (tests/test_hip_vband_fcc.py) with the room's sign in the mirrored cells, r*_iy every
cell's physical row, acc and state raw; stopped and resumed likewise.  Every comparison is np.array_equal (or bytes)."""
import numpy as np
import pytest

import cases
import oracle
import test_hip_vband as cart
import test_hip_vband_fcc as lat
from pffdtd_amd import directional, fields, h5io, recordings, sim_data, synth
from test_hip_checkpoint import STOP
from test_hip_region import _cli
from test_recordings_host import Decim

pytestmark = pytest.mark.gpu
BOXES = ["3:25:1,1:19:2,2:21:3", "13:14:1,1:19:1,1:21:1"]  # a strided box and an x plane, one cell clear of every face
FACTOR, FPASS, ATTEN, FIRST = 3, 1200.0, 40.0, 2  # Ts = 84 us: the new Nyquist frequency is 1983 Hz
COMMON = ("--rec-factor", str(FACTOR), "--rec-fpass", str(FPASS), "--rec-atten", str(ATTEN), "--rec-first", str(FIRST))
COMP = (0, 1, 2, 3)


def _args(boxes, axes="x,y,z"):
    return tuple(v for b in boxes for v in ("--rec-box", b)) + COMMON + (("--rec-axes", axes) if axes else ())


def _same_files(a, b):
    names = h5io.list_datasets(a)
    return names == h5io.list_datasets(b) and all(np.asarray(h5io.read(a, n)).tobytes() == np.asarray(h5io.read(b, n)).tobytes() for n in names)


def _folder(d):
    synth.write_folder(synth.sort_sim(cases.make_sim("cart_mb11")), d)
    return d


@pytest.fixture(scope="module")
def whole(tmp_path_factory):
    """the run in one piece on one device, with --rec-axes x,y,z"""
    d = _folder(tmp_path_factory.mktemp("vwhole"))
    r = _cli(d, *_args(BOXES))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--field recording of 78 samples, 26 frames at every 3th step" in r.stdout and "channels W X Y Z (axis differences)" in r.stdout, r.stdout[-1500:]
    assert "PF_MULTI_NO_PAIRS" not in r.stdout
    return d


def test_the_file_is_infac_times_the_filter_per_channel(whole, tmp_path):
    again, frames_dir, scalar = _folder(tmp_path / "again"), _folder(tmp_path / "frames"), _folder(tmp_path / "scalar")
    path = whole / "sim_recordings.h5"
    r = _cli(again, *_args(BOXES))
    assert r.returncode == 0 and _same_files(path, again / "sim_recordings.h5"), r.stderr[-2000:]  # a second run: the same file
    sd = sim_data.SimData.from_folder(whole, "single")
    N, Nt, Ts, infac = (sd.Nx, sd.Ny, sd.Nz), sd.Nt, float(sd.Ts), None
    specs = [fields.parse_box(b, N) for b in BOXES]
    wide = [cart._widened(s, COMP) for s in specs]
    r = _cli(frames_dir, *[v for lo, hi, st in wide for v in ("--field-box", ",".join(f"{lo[a]}:{hi[a]}:{st[a]}" for a in range(3)))], "--field-every", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    regions, steps, frames = fields.read(frames_dir / "sim_fields.h5")
    assert steps == list(range(Nt)) and [tuple(r) for r in regions] == [tuple(lo) + tuple(hi) + tuple(st) for lo, hi, st in wide]
    sd.scale_input()
    infac = sd.infac
    f = recordings.read_file(path, raw=True)
    taps, info = recordings.decimation_filter(Ts, FACTOR, FPASS, ATTEN)
    nf = -(-(Nt - FIRST) // FACTOR)
    omni, grad = directional.gradient_sections(Ts, float(sd.h), float(sd.c), True, 10.0, 4)
    assert list(f["sampling"]) == [FIRST, FACTOR, Nt - FIRST, nf] and np.array_equal(f["taps"], taps) and f["axes"].tolist() == [1, 2, 3] and f["stencil"] == "axis"
    assert f["fcc_flag"] == 0 and np.array_equal(f["pre_sos"], np.stack([omni, grad, grad, grad])) and list(f["blocks"]) == [0]
    for i, spec in enumerate(specs):
        cells = tuple(len(range(spec[0][a], spec[1][a], spec[2][a])) for a in range(3))
        ds = [Decim(f["pre_sos"][k], taps, FACTOR, cells) for k in range(4)]
        for n in range(FIRST, Nt):
            u = (frames[(i, n)] / infac).astype(np.float32)  # a frame is double(cell) * infac: the division rounds back onto the cell's fp32 value
            assert np.array_equal(u.astype(np.float64) * infac, frames[(i, n)])
            for d, x in zip(ds, cart._components(u, spec, COMP)):
                d.add(x)
        got = recordings.read(path, i)[0]
        want = np.stack([np.array(d.frames) for d in ds], axis=1)
        assert got.dtype == np.float32 and got.shape == (nf, 4) + cells and np.array_equal(got, (want * infac).astype(np.float32)), i
        assert np.array_equal(f["acc"][i], np.stack([d.acc for d in ds])) and np.array_equal(f["state"][i], np.stack([d.state for d in ds])), i
        assert all(np.abs(got[:, k]).max() > 0 for k in range(4)), i
    # without --rec-axes: the scalar recorder's file, with today's datasets; its frames are W (the omni channel's extra section is the identity)
    r = _cli(scalar, *_args(BOXES, axes=""))
    assert r.returncode == 0 and "channels" not in r.stdout, r.stderr[-2000:]
    sf = recordings.read_file(scalar / "sim_recordings.h5", raw=True)
    names = h5io.list_datasets(scalar / "sim_recordings.h5")
    assert sf["axes"] is None and sorted(names) == sorted(["regions", "Ts", "sampling", "taps", "pre_sos", "npre", "frame_bytes", "design", "blocks", "nblocks"] +
                                                          [f"r{i:03d}_{s}" for i in range(2) for s in ("f0000000", "acc", "state")])
    assert np.array_equal(sf["pre_sos"], omni[:-1]) and sf["acc"][0].ndim == 4
    for i in range(2):
        assert np.array_equal(recordings.read(scalar / "sim_recordings.h5", i)[0], recordings.read(path, i)[0][:, 0])
        assert np.array_equal(sf["acc"][i], f["acc"][i][0]) and np.array_equal(sf["state"][i], f["state"][i][0, :-1])


def test_w_is_the_filter_over_a_receivers_row(tmp_path):
    d = _folder(tmp_path)
    sd = sim_data.SimData.from_folder(d, "single")
    sd.scale_input()
    N = (sd.Nx, sd.Ny, sd.Nz)
    cellsof = [(int(v) // (N[1] * N[2]), int(v) // N[2] % N[1], int(v) % N[2]) for v in sd.out_ixyz]
    rows = [(row, c) for row, c in enumerate(cellsof) if all(1 <= c[a] <= N[a] - 2 for a in range(3))]
    assert rows
    row, c = rows[0]
    r = _cli(d, *_args([",".join(f"{c[a]}:{c[a] + 1}:1" for a in range(3))]), "--rec-dtype", "f8")
    assert r.returncode == 0, r.stderr[-2000:]
    oracle.run_sim(sd)  # (raw rows: u^n of the receivers' cells)
    f = recordings.read_file(d / "sim_recordings.h5")
    w = Decim(f["pre_sos"][0], f["taps"], FACTOR, (1, 1, 1))
    for n in range(FIRST, sd.Nt):
        w.add(sd.u_out[row, n].reshape(1, 1, 1))
    got = recordings.read(d / "sim_recordings.h5", 0)[0]
    assert got.dtype == np.float64 and np.array_equal(got[:, 0], np.array(w.frames) * sd.infac) and np.abs(got[:, 0]).max() > 0


@pytest.mark.parametrize("devices", [(), ("--devices", "0,0")], ids=["one_device", "two_slabs"])
def test_stopped_and_resumed_equals_the_run_in_one_piece(whole, tmp_path, devices):
    _folder(tmp_path)
    args = _args(BOXES)
    r = _cli(tmp_path, *devices, *args, "--stop-after", str(STOP), "--checkpoint", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert ("PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES" in r.stdout) == bool(devices), r.stdout[:1500]
    path = tmp_path / "sim_recordings.h5"
    assert list(recordings.read_file(path)["sampling"]) == [FIRST, FACTOR, STOP - FIRST, -(-(STOP - FIRST) // FACTOR)] and not (tmp_path / "sim_outs.h5").exists()
    r = _cli(tmp_path, *devices, *args, "--resume", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert h5io.read(tmp_path / "sim_outs.h5", "u_out").tobytes() == h5io.read(whole / "sim_outs.h5", "u_out").tobytes()
    assert _same_files(whole / "sim_recordings.h5", path)
    # other axes than the file's, and the scalar recorder: refused by the field's name
    for axes in ("x,y", ""):
        r = _cli(tmp_path, *devices, *_args(BOXES, axes=axes), "--resume", "ck.h5")
        assert r.returncode != 0 and ": axes: " in r.stderr, r.stderr[-1500:]
    # --rec-axes without a region, a lattice stencil on a Cartesian folder, a region on a face along a recorded axis
    r = _cli(tmp_path, "--rec-axes", "x")
    assert r.returncode != 0 and "need --rec-planes or --rec-box" in r.stderr, r.stderr[-1500:]
    r = _cli(tmp_path, *args, "--rec-stencil", "lattice")
    assert r.returncode != 0 and "--rec-stencil lattice" in r.stderr and "FCC grids only" in r.stderr, r.stderr[-1500:]
    r = _cli(tmp_path, "--rec-planes", "z=21", *COMMON, "--rec-axes", "y")
    assert r.returncode != 0 and "along file y" in r.stderr, r.stderr[-1500:]


# ---- a folded FCC folder: --rec-stencil lattice --rec-axes y -----------------------------------------------------------------------------------------
FCC_SCENE = "fcc2_outside"  # 30 x 17 x 26 stored (a room of 32 rows), 60 steps
# the plane y = 8 clear of the faces, a strided box, and a box whose last row y = 15 = Ny - 2 reads the fold row (tests/test_hip_directional_fcc_cli.py)
FCC_BOXES = ("1:29:1,8:9:1,1:25:1", "3:27:1,1:15:2,2:24:3", "3:27:2,13:16:1,2:24:3")
FCC_WIDE = ("0:30:1,7:10:1,0:26:1", "2:28:1,0:15:1,1:25:1", "2:27:1,12:17:1,1:25:1")  # ... widened by one cell on every axis, stride 1


def _fcc_args(folder):
    """the recording arguments for the folder's Ts: flat up to 0.6 of the new Nyquist frequency"""
    Ts = float(h5io.read(folder / "sim_consts.h5", "Ts"))
    fpass = round(0.6 / (2 * FACTOR * Ts))
    return tuple(v for b in FCC_BOXES for v in ("--rec-box", b)) + ("--rec-factor", str(FACTOR), "--rec-fpass", str(fpass), "--rec-atten", str(ATTEN), "--rec-first", str(FIRST),
                                                                       "--rec-axes", "y", "--rec-stencil", "lattice", "--rec-dtype", "f8"), float(fpass)


@pytest.fixture(scope="module")
def fcc_whole(tmp_path_factory):
    d = tmp_path_factory.mktemp("vfcc")
    synth.write_folder(cases.make_sim(FCC_SCENE), d)
    r = _cli(d, *_fcc_args(d)[0])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--field recording of 58 samples, 20 frames at every 3th step" in r.stdout and "channels W Y (lattice differences)" in r.stdout, r.stdout[-1500:]
    return d


def test_a_folded_folder_gives_the_rooms_sign_and_raw_state(fcc_whole, tmp_path):
    synth.write_folder(cases.make_sim(FCC_SCENE), tmp_path)
    r = _cli(tmp_path, *[a for w in FCC_WIDE for a in ("--field-box", w)], "--field-every", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    assert h5io.read(fcc_whole / "sim_outs.h5", "u_out").tobytes() == h5io.read(tmp_path / "sim_outs.h5", "u_out").tobytes()  # recording changes nothing
    _, steps, frames = fields.read(tmp_path / "sim_fields.h5")
    path = fcc_whole / "sim_recordings.h5"
    f = recordings.read_file(path, raw=True)
    sd = sim_data.SimData.from_folder(fcc_whole, "single")
    sd.scale_input()
    N, Nt, Ts, infac = (sd.Nx, sd.Ny, sd.Nz), sd.Nt, float(sd.Ts), float(sd.infac)
    assert N == (30, 17, 26) and int(sd.fcc_flag) == 2 and steps == list(range(Nt))
    specs = [fields.parse_box(b, N) for b in FCC_BOXES]
    for s, w in zip(specs, FCC_WIDE):
        assert tuple(tuple(v) for v in lat._wide(s)) == tuple(tuple(v) for v in fields.parse_box(w, N))
    taps, _ = recordings.decimation_filter(Ts, FACTOR, _fcc_args(fcc_whole)[1], ATTEN)
    omni, grad = directional.gradient_sections(Ts, float(sd.h), float(sd.c), True, 10.0, 4, span=8)
    nf = -(-(Nt - FIRST) // FACTOR)
    assert f["stencil"] == "lattice" and f["fcc_flag"] == 2 and f["axes"].tolist() == [2] and list(f["sampling"]) == [FIRST, FACTOR, Nt - FIRST, nf]
    assert np.array_equal(f["taps"], taps) and np.array_equal(f["pre_sos"], np.stack([omni, grad])) and [tuple(r) for r in f["regions"]] == [lo + hi + st for lo, hi, st in specs]
    signed = 0
    for i, spec in enumerate(specs):
        cells = tuple(-(-(spec[1][a] - spec[0][a]) // spec[2][a]) for a in range(3))
        ds = [Decim(omni, taps, FACTOR, cells), Decim(grad, taps, FACTOR, cells)]
        for n in range(FIRST, Nt):
            u = (frames[(i, n)] / infac).astype(np.float32)  # a frame is double(cell) * infac: the division rounds back onto the cell's fp32 value
            assert np.array_equal(u.astype(np.float64) * infac, frames[(i, n)])
            if lat._wide(spec)[1][1] == N[1]:  # the frame's last row is the fold row: the copy of row Ny - 2 of the same field, which an add writes first
                u[:, -1, :] = u[:, -2, :]
            for d, x in zip(ds, lat._components(u, spec, (0, 5))):
                d.add(x)
        _, iy, _, upper = directional.fold_coordinates(spec, N[1])
        assert np.array_equal(f["iy"][i], iy) and upper.any() and not upper.all()
        got = recordings.read(path, i)[0]
        w, y = np.array(ds[0].frames) * infac, np.array(ds[1].frames) * infac
        assert got.dtype == np.float64 and got.shape == (nf, 2) + cells
        assert np.array_equal(got[:, 0], w) and np.array_equal(got[:, 1], np.where(upper, -y, y)), i  # the stored +y of a mirrored cell is the room's -y
        assert np.array_equal(f["acc"][i], np.stack([d.acc for d in ds])) and np.array_equal(f["state"][i], np.stack([d.state for d in ds])), i  # raw: storage form
        assert np.abs(got[:, 0]).max() > 0 and np.abs(got[:, 1]).max() > 0, i
        signed += int(np.count_nonzero(got[:, 1][..., upper]))
    assert signed > 0


@pytest.mark.parametrize("devices", [(), ("--devices", "0,0")], ids=["one_device", "two_slabs"])
def test_a_folded_folder_stopped_and_resumed(fcc_whole, tmp_path, devices):
    synth.write_folder(cases.make_sim(FCC_SCENE), tmp_path)
    args = _fcc_args(tmp_path)[0]
    r = _cli(tmp_path, *devices, *args, "--stop-after", str(STOP), "--checkpoint", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert list(recordings.read_file(tmp_path / "sim_recordings.h5")["sampling"])[2] == STOP - FIRST and not (tmp_path / "sim_outs.h5").exists()
    r = _cli(tmp_path, *devices, *args, "--resume", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert h5io.read(tmp_path / "sim_outs.h5", "u_out").tobytes() == h5io.read(fcc_whole / "sim_outs.h5", "u_out").tobytes()
    assert _same_files(fcc_whole / "sim_recordings.h5", tmp_path / "sim_recordings.h5")
    # the axis stencil on an FCC folder, and another stencil than the file's: refused by name
    r = _cli(tmp_path, *devices, *[v for v in args if v not in ("--rec-stencil", "lattice")])
    assert r.returncode != 0 and "fcc_flag" in r.stderr and "--rec-stencil lattice" in r.stderr, r.stderr[-1500:]
