"""GPU: decimated field recordings from the command line (fdtd_main --rec-planes / --rec-box / --rec-factor / --rec-fpass, pffdtd_amd/recordings.py).

The file's frames are infac times `Decim` (tests/test_recordings_host.py: the contract's lines in numpy) over the frames a second run records at
every step (--field-every 1) over the same regions, rounded to the file's float32; a run stopped at a checkpoint and resumed gives the file and
the sim_outs.h5 of the run in one piece, on one device and on a chain of two slabs; without the arguments no file appears.  Every comparison is
np.array_equal (or bytes)."""
import numpy as np
import pytest

import cases
from pffdtd_amd import decay, fields, h5io, recordings, synth
from test_hip_checkpoint import STOP
from test_hip_region import _cli, _oracle_frames
from test_recordings_host import Decim

pytestmark = pytest.mark.gpu
PLANES, BOX = "x=13,z=21", "3:26:1,1:20:2,2:22:3"
FACTOR, FPASS, ATTEN, FIRST = 3, 1200.0, 40.0, 2  # Ts = 84 us: the new Nyquist frequency is 1983 Hz
ARGS = ("--rec-planes", PLANES, "--rec-box", BOX, "--rec-factor", str(FACTOR), "--rec-fpass", str(FPASS), "--rec-atten", str(ATTEN), "--rec-first", str(FIRST))


def _same(a, b, n):
    fa, fb = recordings.read_file(a, raw=True), recordings.read_file(b, raw=True)
    return all(np.array_equal(fa[k], fb[k]) for k in ("regions", "sampling", "taps", "pre_sos", "design", "blocks")) and fa["Ts"] == fb["Ts"] and \
        all(x.tobytes() == y.tobytes() for k in ("acc", "state") for x, y in zip(fa[k], fb[k])) and \
        all(recordings.read(a, i)[0].tobytes() == recordings.read(b, i)[0].tobytes() for i in range(n))


@pytest.fixture(scope="module")
def whole(tmp_path_factory):
    """the run in one piece on one device, with the recording arguments"""
    d = tmp_path_factory.mktemp("whole")
    synth.write_folder(synth.sort_sim(cases.make_sim("cart_mb11")), d)
    r = _cli(d, *ARGS)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--field recording of 78 samples, 26 frames at every 3th step" in r.stdout and "PF_MULTI_NO_PAIRS" not in r.stdout, r.stdout[-1500:]
    return d


def test_the_file_is_infac_times_the_filter_over_every_frame(whole, tmp_path):
    plain, frames_dir = tmp_path / "plain", tmp_path / "frames"
    for d in (plain, frames_dir):
        d.mkdir()
        synth.write_folder(synth.sort_sim(cases.make_sim("cart_mb11")), d)
    _, ref_out, infac, N = _oracle_frames(plain, set())
    r = _cli(plain)
    assert r.returncode == 0, r.stderr[-2000:]
    assert not (plain / "sim_recordings.h5").exists() and "recording" not in r.stdout  # without the arguments: no file, no word
    assert np.array_equal(h5io.read(plain / "sim_outs.h5", "u_out"), ref_out)
    assert h5io.read(whole / "sim_outs.h5", "u_out").tobytes() == h5io.read(plain / "sim_outs.h5", "u_out").tobytes()
    r = _cli(frames_dir, "--field-planes", PLANES, "--field-box", BOX, "--field-every", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    regions, steps, frames = fields.read(frames_dir / "sim_fields.h5")
    path = whole / "sim_recordings.h5"
    f = recordings.read_file(path, raw=True)
    specs = fields.parse_planes(PLANES, N) + [fields.parse_box(BOX, N)]
    Nt = 80
    Ts = float(h5io.read(whole / "sim_consts.h5", "Ts"))
    assert steps == list(range(Nt)) and np.array_equal(f["regions"], regions) and [tuple(r) for r in regions] == [lo + hi + st for lo, hi, st in specs]
    taps, info = recordings.decimation_filter(Ts, FACTOR, FPASS, ATTEN)
    nf = -(-(Nt - FIRST) // FACTOR)
    assert list(f["sampling"]) == [FIRST, FACTOR, Nt - FIRST, nf] and f["Ts"] == Ts and np.array_equal(f["taps"], taps) and list(f["blocks"]) == [0]
    assert list(f["design"]) == [FPASS, ATTEN, info["stop_db"], info["ripple_db"], (taps.size - 1) / 2] and info["stop_db"] <= -ATTEN
    pre = decay.pre_sections(Ts, True, 10.0, 4)
    assert np.array_equal(f["pre_sos"], pre) and pre.shape == (2, 6)
    live = 0
    for i in range(len(specs)):
        d = Decim(pre, taps, FACTOR, frames[(i, 0)].shape)
        for n in range(FIRST, Nt):
            u = (frames[(i, n)] / infac).astype(np.float32)  # a frame is double(cell) * infac: the division rounds back onto the cell's fp32 value
            assert np.array_equal(u.astype(np.float64) * infac, frames[(i, n)])
            d.add(u)
        got, fs_out, t0 = recordings.read(path, i)
        assert got.dtype == np.float32 and got.shape == (nf,) + frames[(i, 0)].shape and fs_out == 1.0 / (FACTOR * Ts) and t0 == (FIRST - (taps.size - 1) / 2) * Ts
        assert np.array_equal(got, (np.array(d.frames) * infac).astype(np.float32)), i
        assert np.array_equal(f["acc"][i], d.acc) and np.array_equal(f["state"][i], d.state), i
        live += np.abs(got).max() > 0
    assert live >= 2  # (not zeros against zeros; the ghost plane z = 21 may stay 0)


@pytest.mark.parametrize("devices", [(), ("--devices", "0,0")], ids=["one_device", "two_slabs"])
def test_stopped_and_resumed_equals_the_run_in_one_piece(whole, tmp_path, devices):
    synth.write_folder(synth.sort_sim(cases.make_sim("cart_mb11")), tmp_path)
    r = _cli(tmp_path, *devices, *ARGS, "--stop-after", str(STOP), "--checkpoint", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert ("PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES" in r.stdout) == bool(devices), r.stdout[:1500]
    path = tmp_path / "sim_recordings.h5"
    assert list(recordings.read_file(path)["sampling"]) == [FIRST, FACTOR, STOP - FIRST, -(-(STOP - FIRST) // FACTOR)] and not (tmp_path / "sim_outs.h5").exists()
    r = _cli(tmp_path, *devices, *ARGS, "--resume", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert h5io.read(tmp_path / "sim_outs.h5", "u_out").tobytes() == h5io.read(whole / "sim_outs.h5", "u_out").tobytes()
    assert _same(whole / "sim_recordings.h5", path, 3)
    # another low-pass than the file's: refused by the field's name
    r = _cli(tmp_path, *devices, "--rec-planes", PLANES, "--rec-box", BOX, "--rec-factor", str(FACTOR), "--rec-fpass", "1000", "--rec-atten", str(ATTEN), "--rec-first", str(FIRST),
             "--resume", "ck.h5")
    assert r.returncode != 0 and "taps" in r.stderr, r.stderr[-1500:]
    # a region without --rec-factor, --rec-factor without a region: refused both ways round
    for args in (("--rec-planes", PLANES), ("--rec-factor", "3", "--rec-fpass", "1200")):
        r = _cli(tmp_path, *args)
        assert r.returncode != 0 and "--rec-planes / --rec-box need --rec-factor and --rec-fpass" in r.stderr, r.stderr[-1500:]
