"""GPU: field spectra from the command line (fdtd_main --spectrum-planes / --spectrum-box / --spectrum-freqs, pffdtd_amd/spectra.py).

The file is infac times the numpy fold of the frames a second run records at every step (--field-every 1) over the same regions; a run stopped and
resumed gives the file and the sim_outs.h5 of the run in one piece; a chain gives the file of one device; without the arguments nothing changes.
Every comparison is np.array_equal (or the files' bytes)."""
import numpy as np
import pytest

import cases
from pffdtd_amd import fields, h5io, spectra, synth
from test_hip_checkpoint import STOP
from test_hip_region import _cli, _oracle_frames

pytestmark = pytest.mark.gpu
PLANES, BOX, FREQS = "x=13,z=21", "3:26:1,1:20:2,2:22:3", "400,1500,2750.5"
ARGS = ("--spectrum-planes", PLANES, "--spectrum-box", BOX, "--spectrum-freqs", FREQS)


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("regions", "freqs", "sampling")) and a["Ts"] == b["Ts"] and a["window"] == b["window"] and \
        all(x.tobytes() == y.tobytes() for k in ("re", "im") for x, y in zip(a[k], b[k]))


@pytest.fixture(scope="module")
def whole(tmp_path_factory):
    """the run in one piece on one device, with the spectrum arguments"""
    d = tmp_path_factory.mktemp("whole")
    synth.write_folder(synth.sort_sim(cases.make_sim("cart_mb11")), d)
    r = _cli(d, *ARGS)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--field spectrum of 80 samples at 3 frequencies" in r.stdout and "PF_MULTI_NO_PAIRS" not in r.stdout, r.stdout[-1500:]
    return d


def test_the_file_is_infac_times_the_fold_of_every_frame(whole, tmp_path):
    plain, frames_dir = tmp_path / "plain", tmp_path / "frames"
    for d in (plain, frames_dir):
        d.mkdir()
        synth.write_folder(synth.sort_sim(cases.make_sim("cart_mb11")), d)
    _, ref_out, infac, N = _oracle_frames(plain, set())
    r = _cli(plain)
    assert r.returncode == 0, r.stderr[-2000:]
    assert not (plain / "sim_spectra.h5").exists() and "spectrum" not in r.stdout  # without the arguments: no file, no word
    assert np.array_equal(h5io.read(plain / "sim_outs.h5", "u_out"), ref_out)
    assert h5io.read(whole / "sim_outs.h5", "u_out").tobytes() == h5io.read(plain / "sim_outs.h5", "u_out").tobytes()
    r = _cli(frames_dir, "--field-planes", PLANES, "--field-box", BOX, "--field-every", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    regions, steps, frames = fields.read(frames_dir / "sim_fields.h5")
    f = spectra.read(whole / "sim_spectra.h5")
    specs = fields.parse_planes(PLANES, N) + [fields.parse_box(BOX, N)]
    Nt = 80
    assert steps == list(range(Nt)) and np.array_equal(f["regions"], regions) and [tuple(r) for r in regions] == [lo + hi + st for lo, hi, st in specs]
    assert np.array_equal(f["freqs"], [400.0, 1500.0, 2750.5]) and list(f["sampling"]) == [0, 1, Nt] and f["window"] == 0
    assert f["Ts"] == float(h5io.read(whole / "sim_consts.h5", "Ts"))
    host = spectra.FieldSpectrum("unused.h5", type("S", (), {"Ts": f["Ts"], "Nt": Nt, "infac": infac})(), specs, f["freqs"])
    for i in range(len(specs)):
        acc = np.zeros((6,) + frames[(i, 0)].shape)
        for n in range(Nt):
            u = (frames[(i, n)] / infac).astype(np.float32)  # a frame is double(cell) * infac: the division rounds back onto the cell's fp32 value
            assert np.array_equal(u.astype(np.float64) * infac, frames[(i, n)])
            w = host.weights(n)
            for m in range(6):
                acc[m] += w[m] * u.astype(np.float64)
        assert np.array_equal(f["re"][i], acc[0::2] * infac) and np.array_equal(f["im"][i], acc[1::2] * infac), i
        assert f["re"][i].shape == (3,) + frames[(i, 0)].shape
    assert sum(np.abs(f["re"][i]).max() > 0 and np.abs(f["im"][i]).max() > 0 for i in range(len(specs))) >= 2  # (not zeros against zeros; the ghost plane z = 21 may stay 0)


def test_stopped_and_resumed_equals_the_run_in_one_piece(whole, tmp_path):
    synth.write_folder(synth.sort_sim(cases.make_sim("cart_mb11")), tmp_path)
    r = _cli(tmp_path, *ARGS, "--stop-after", str(STOP), "--checkpoint", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert list(spectra.read(tmp_path / "sim_spectra.h5")["sampling"]) == [0, 1, STOP] and not (tmp_path / "sim_outs.h5").exists()
    r = _cli(tmp_path, *ARGS, "--resume", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert h5io.read(tmp_path / "sim_outs.h5", "u_out").tobytes() == h5io.read(whole / "sim_outs.h5", "u_out").tobytes()
    assert _same(spectra.read(whole / "sim_spectra.h5"), spectra.read(tmp_path / "sim_spectra.h5"))
    # other frequencies than the file's: refused by the field's name
    r = _cli(tmp_path, "--spectrum-planes", PLANES, "--spectrum-box", BOX, "--spectrum-freqs", "400,1500", "--resume", "ck.h5")
    assert r.returncode != 0 and "freqs" in r.stderr, r.stderr[-1500:]


def test_a_chain_gives_the_file_of_one_device(whole, tmp_path):
    synth.write_folder(synth.sort_sim(cases.make_sim("cart_mb11")), tmp_path)
    r = _cli(tmp_path, "--devices", "0,0", *ARGS)  # (--gpus 2 on one device)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--2 slabs on devices [0, 0]" in r.stdout and "PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES" in r.stdout, r.stdout[:1500]
    assert h5io.read(tmp_path / "sim_outs.h5", "u_out").tobytes() == h5io.read(whole / "sim_outs.h5", "u_out").tobytes()
    assert _same(spectra.read(whole / "sim_spectra.h5"), spectra.read(tmp_path / "sim_spectra.h5"))
