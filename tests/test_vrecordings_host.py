"""CPU: the host side of the B-format field recordings (pffdtd_amd/recordings.py with `axes`): a plane wave through per-component `Decim`s
(tests/test_recordings_host.py) with directional.gradient_sections gives X / W = cos(theta) and Y / W = sin(theta) within the documented error
terms, on the central difference and on the lattice difference of an FCC checkerboard; virtual_microphone; the file with and without `axes`, the
folded grid's negation and iy, stop and resume, and every refusal -- with a vector recorder object that folds in numpy, no device."""
import functools
import types

import numpy as np
import pytest

from pffdtd_amd import directional, h5io, recordings
from test_recordings_host import KW, Decim
from test_recordings_host import REGIONS as SCALAR_REGIONS
from test_recordings_host import FakeEngine as ScalarEngine
from test_recordings_host import _run
from test_recordings_host import _sd as _scalar_sd

TS = 1.0 / 25500.0
C, H = 343.0, 343.0 * TS * np.sqrt(3.0)  # the Cartesian scheme's stability limit: h = c Ts sqrt 3
N = (5, 6, 7)
REGIONS = [((1, 1, 3), (4, 5, 4), (1, 1, 1)), ((1, 1, 1), (4, 5, 6), (2, 2, 3))]  # one cell clear of all six faces
# the + offsets of the lattice differences (include/pffdtd_hip.h), in the order of the 12-point stencil
LAT_OFFS = {4: [(1, 1, 0), (1, 0, 1), (1, -1, 0), (1, 0, -1)], 5: [(1, 1, 0), (0, 1, 1), (-1, 1, 0), (0, 1, -1)], 6: [(0, 1, 1), (1, 0, 1), (0, -1, 1), (-1, 0, 1)]}
AXIS_OFFS = {1: (1, 0, 0), 2: (0, 1, 0), 3: (0, 0, 1)}


def _component(at, k):
    """component k of the contract from at(offset) -> the field at the cells shifted by `offset`, in the contract's association"""
    if k == 0:
        return at((0, 0, 0))
    if k <= 3:
        o = AXIS_OFFS[k]
        return at(o) - at(tuple(-v for v in o))
    d = [at(o) - at(tuple(-v for v in o)) for o in LAT_OFFS[k]]
    return (d[0] + d[1]) + (d[2] + d[3])


# ---- the physics: a plane wave in the x-y plane ------------------------------------------------------------------------------------------------------
F0, LOWCUT, ORDER, FACTOR, FPASS, ATTEN = 1000.0, 20.0, 2, 4, 2000.0, 40.0
ANGLES = np.deg2rad([0.0, 30.0, 60.0, 90.0, 135.0, 180.0, 250.0])
NSAMP, TAIL = 6000, 300  # samples, and the frames of the fit: the sections' slowest pole, 0.707 * 2 pi 20 Hz, has decayed by e^-19 at sample 5000


@functools.lru_cache(maxsize=None)
def _plane_wave(stencil):
    """-> (frames [F, 3, nangle] (W, X, Y) of a tone F0 travelling along ANGLES, one angle per 'cell'; the times of the frames; the design's info)"""
    span = directional.LATTICE_SPAN if stencil == "lattice" else 2
    omni, grad = directional.gradient_sections(TS, H, C, False, LOWCUT, ORDER, span=span)
    taps, info = recordings.decimation_filter(TS, FACTOR, FPASS, ATTEN)
    comp = (0, 4, 5) if stencil == "lattice" else (0, 1, 2)
    ds = [Decim(omni, taps, FACTOR, ANGLES.shape), Decim(grad, taps, FACTOR, ANGLES.shape), Decim(grad, taps, FACTOR, ANGLES.shape)]
    w = 2 * np.pi * F0
    kx, ky = np.cos(ANGLES), np.sin(ANGLES)
    for n in range(NSAMP):
        def at(o):  # p = sin(w (t - r . k / c)) at the node o (in cells) beside the centre: a node of the checkerboard where o is a lattice offset
            return np.sin(w * (n * TS - H * (o[0] * kx + o[1] * ky) / C))
        for d, k in zip(ds, comp):
            d.add(_component(at, k))
    frames = np.stack([np.array(d.frames) for d in ds], axis=1)
    t = (np.arange(frames.shape[0]) * FACTOR - info["delay"]) * TS  # frame m is the filtered signal at sample m D - delay
    return frames, t, info


def _bound(info):
    """the documented error terms (pffdtd_amd/directional.py) and the design's passband ripple as a relative deviation"""
    w = 2 * np.pi * F0
    return (w * H / C) ** 2 / 6 + (w * TS) ** 2 / 12 + (LOWCUT / F0) ** 2 / 2 + (10.0 ** (info["ripple_db"] / 20.0) - 1.0)


def _tone(y, t):
    """complex amplitudes of the tone F0 in the last TAIL frames of y [F, ...], and the largest residual of the fit: a pure tone, the transient gone"""
    w = 2 * np.pi * F0
    basis = np.stack([np.sin(w * t[-TAIL:]), np.cos(w * t[-TAIL:])], axis=1)
    tail = y[-TAIL:].reshape(TAIL, -1)
    coef = np.linalg.lstsq(basis, tail, rcond=None)[0]
    return (coef[0] + 1j * coef[1]).reshape(y.shape[1:]), np.abs(basis @ coef - tail).max()


@pytest.mark.parametrize("stencil", ["axis", "lattice"])
def test_a_plane_wave_gives_cosine_and_sine(stencil):
    """X / W = cos(theta) and Y / W = sin(theta): the real part of the ratio of the complex amplitudes, within
        (omega h / c)^2 / 6 + (omega Ts)^2 / 12 + (lowcut / f)^2 / 2 + the design's ripple.
    The lattice difference of a wave along (c, s, 0) is 2 [sin(x (c + s)) + sin(x (c - s)) + 2 sin(x c)] = 8 sin(x c) (1 + cos(x s)) / 2, x = omega h / c:
    against 8 x c it misses by at most x^2 (c^3 / 6 + c s^2 / 4) = x^2 (c / 4 - c^3 / 12) <= x^2 / 6, the central difference's own term."""
    frames, t, info = _plane_wave(stencil)
    bound = _bound(info)
    amp, res = _tone(frames, t)
    assert frames.shape[0] == NSAMP // FACTOR and res <= 1e-6, res
    assert np.all(np.abs(np.abs(amp[0]) - 1.0) <= 10.0 ** (info["ripple_db"] / 20.0) - 1.0 + (LOWCUT / F0) ** 4)  # W: the tone itself (2nd-order low-cut: 1 - r^4 / 2)
    for ch, want in ((1, np.cos(ANGLES)), (2, np.sin(ANGLES))):
        ratio = amp[ch] / amp[0]
        signed = ratio.real  # (the part of X in phase with W)
        print(f"{stencil} channel {ch}: ratio {np.round(signed, 6).tolist()}, want {np.round(want, 6).tolist()}, bound {bound:.3e}")
        assert np.all(np.abs(signed - want) <= bound), (stencil, ch, np.abs(signed - want).max(), bound)
        assert np.all(np.abs(ratio.imag) <= LOWCUT / F0 + bound)  # (the first-order high-pass turns the phase by about lowcut / f)


@pytest.mark.parametrize("stencil", ["axis", "lattice"])
def test_virtual_microphone(stencil):
    frames, t, info = _plane_wave(stencil)
    bound = _bound(info)
    w_amp = np.abs(_tone(frames[:, 0], t)[0])
    for i, th in enumerate(ANGLES):
        d = np.array([np.cos(th), np.sin(th), 0.0])
        one = frames[:, :, i]
        along = np.abs(_tone(recordings.virtual_microphone(one, [1, 2], d), t)[0])
        against = np.abs(_tone(recordings.virtual_microphone(one, [1, 2], -d), t)[0])
        assert abs(along - w_amp[i]) <= bound and against <= bound, (stencil, th, along, against, bound)
    one = frames[:, :, 1]
    assert np.array_equal(recordings.virtual_microphone(one, [1, 2], [1, 0, 0], pattern=1.0), one[:, 0])  # omni
    assert np.array_equal(recordings.virtual_microphone(one, [1, 2], [0, 1, 0], pattern=0.0), one[:, 2])  # a figure-of-eight along y
    assert np.array_equal(recordings.virtual_microphone(one[:, [0, 2]], [2], [0, -1, 0], pattern=0.0), -one[:, 2])
    with pytest.raises(ValueError, match="virtual_microphone: direction: .* along file z, but axis 3 was not recorded"):
        recordings.virtual_microphone(one, [1, 2], [0.6, 0.0, 0.8])
    with pytest.raises(ValueError, match="virtual_microphone: direction: .* unit vector"):
        recordings.virtual_microphone(one, [1, 2], [1.0, 1.0, 0.0])
    with pytest.raises(ValueError, match="virtual_microphone: frames: "):
        recordings.virtual_microphone(one, [1], [1.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="virtual_microphone: pattern: "):
        recordings.virtual_microphone(one, [1, 2], [1.0, 0.0, 0.0], pattern=1.5)


# ---- the file: a vector recorder object that folds in numpy, no device -----------------------------------------------------------------------------
def _sd(Nt=144, Ts=TS, infac=0.37, diff=True, h=H, fcc_flag=0):
    return types.SimpleNamespace(Nt=Nt, Ts=Ts, infac=infac, Nx=N[0], Ny=N[1], Nz=N[2], diff=diff, h=h, c=C, fcc_flag=fcc_flag)


class FakeVRecorder:
    """engine.VectorDecimatingRecorder in numpy: one Decim per component"""

    def __init__(self, lo, hi, st, comp, pre, taps, factor, cap, field):
        self.cells = tuple(-(-(hi[a] - lo[a]) // st[a]) for a in range(3))
        self.lo, self.hi, self.st, self.comp, self.ncomp = lo, hi, st, tuple(int(c) for c in comp), len(comp)
        pre = np.asarray(pre).reshape(self.ncomp, -1, 6)
        self.d, self.cap, self.rd, self.field = [Decim(pre[k], taps, factor, self.cells) for k in range(self.ncomp)], cap, 0, field

    count = property(lambda self: self.d[0].count)
    pending = property(lambda self: len(self.d[0].frames) - self.rd)

    def add(self):
        assert not (self.count % self.d[0].D == 0 and self.pending == self.cap), "the device would refuse: cap frames wait"
        u = self.field()

        def at(o):
            return u[tuple(slice(self.lo[a] + o[a], self.hi[a] + o[a], self.st[a]) for a in range(3))]
        for d, k in zip(self.d, self.comp):
            x = _component(at, k)
            assert x.dtype == u.dtype
            d.add(x)

    def read(self, max_frames=None):
        n = self.pending if max_frames is None else min(max_frames, self.pending)
        out = np.stack([np.array(d.frames[self.rd:self.rd + n]).reshape((n,) + self.cells) for d in self.d], axis=1)
        first, self.rd = self.rd, self.rd + n
        return first, out

    def get_state(self):
        return np.stack([d.acc for d in self.d]), np.stack([d.state for d in self.d])

    def set_state(self, acc, state, count):
        for k, d in enumerate(self.d):
            d.acc = np.zeros_like(d.acc) if acc is None else np.array(acc, dtype=np.float64).reshape((self.ncomp,) + d.acc.shape)[k]
            d.state = np.zeros_like(d.state) if state is None else np.array(state, dtype=np.float64).reshape((self.ncomp,) + d.state.shape)[k]
            d.count = count
            d.frames = [None] * -(-count // d.D)
        self.rd = len(self.d[0].frames)

    def close(self):
        pass


class FakeEngine:
    """u^n = a seeded random field per step; the scalar recorder is test_recordings_host's"""

    def __init__(self):
        self.n = 0

    def field(self):
        return np.random.default_rng(3000 + self.n).standard_normal(N).astype(np.float32)

    def decimating_recorder(self, lo, hi, stride=(1, 1, 1), pre_sos=None, taps=None, factor=1, cap=0, depth=0):
        from test_recordings_host import FakeRecorder
        return FakeRecorder(lo, hi, stride, pre_sos, taps, factor, cap, self.field)

    def vector_decimating_recorder(self, lo, hi, stride=(1, 1, 1), comp=(0,), pre_sos=None, taps=None, factor=1, cap=0, depth=0):
        return FakeVRecorder(lo, hi, stride, comp, pre_sos, taps, factor, cap, self.field)


# what a file without `axes` holds: written down here, not derived from the code (KW: first 3, factor 4, cap 5; 144 steps -> 36 frames, P = ceil(ntap / 4))
def _scalar_file_datasets(ntap, cells):
    P = -(-ntap // 4)
    want = {"regions": (2, 9), "Ts": (), "sampling": (4,), "taps": (ntap,), "pre_sos": (2, 6), "npre": (), "frame_bytes": (), "design": (5,), "blocks": (8,), "nblocks": ()}
    for i, c in enumerate(cells):
        for m0 in range(0, 36, 5):
            want[f"r{i:03d}_f{m0:07d}"] = (min(5, 36 - m0),) + c
        want[f"r{i:03d}_acc"] = (P,) + c
        want[f"r{i:03d}_state"] = (2, 2) + c
    return want


def _shapes(path):
    return {name: tuple(np.shape(h5io.read(path, name))) for name in h5io.list_datasets(path)}


def test_a_file_without_axes_is_todays(tmp_path):
    sd = _scalar_sd()
    fr = recordings.FieldRecording(tmp_path / "scalar.h5", sd, SCALAR_REGIONS, **KW)
    assert fr.axes is None and fr.comp is None and fr.pre_sos.shape == (2, 6)
    _run(fr, ScalarEngine(), 0, sd.Nt)
    fr.write()
    assert type(fr.recs[0]).__name__ == "FakeRecorder"  # the scalar recorder is what runs
    assert _shapes(tmp_path / "scalar.h5") == _scalar_file_datasets(fr.taps.size, [(4, 5, 1), (2, 3, 2)])
    f = recordings.read_file(tmp_path / "scalar.h5")
    assert f["axes"] is None and f["stencil"] == "axis" and f["fcc_flag"] == 0 and "iy" not in f
    frames = recordings.read(tmp_path / "scalar.h5", 1)[0]
    assert frames.shape == (36, 2, 3, 2) and frames.dtype == np.float32
    # ... and the same values as axes=None given by name
    again = recordings.FieldRecording(tmp_path / "again.h5", sd, SCALAR_REGIONS, axes=None, stencil="axis", **KW)
    _run(again, ScalarEngine(), 0, sd.Nt)
    again.write()
    for name in h5io.list_datasets(tmp_path / "scalar.h5"):
        assert np.array_equal(h5io.read(tmp_path / "scalar.h5", name), h5io.read(tmp_path / "again.h5", name)), name


def test_vector_file_and_resume(tmp_path):
    sd = _sd()
    axes = [2, 1, 3]
    whole = recordings.FieldRecording(tmp_path / "whole.h5", sd, REGIONS, axes=axes, **KW)
    omni, grad = directional.gradient_sections(TS, H, C, True, 10.0, 4)
    assert whole.comp.tolist() == [0, 2, 1, 3] and np.array_equal(whole.pre_sos, np.stack([omni, grad, grad, grad])) and whole.pre_sos.shape == (4, 3, 6)
    eng = FakeEngine()
    _run(whole, eng, 0, sd.Nt)
    whole.write()
    w = recordings.read_file(tmp_path / "whole.h5", raw=True)
    nf = -(-(sd.Nt - 3) // 4)
    P = -(-whole.taps.size // 4)
    assert list(w["sampling"]) == [3, 4, sd.Nt - 3, nf] and w["axes"].tolist() == axes and w["stencil"] == "axis" and w["fcc_flag"] == 0 and "iy" not in w
    assert np.array_equal(w["pre_sos"], whole.pre_sos) and np.array_equal(w["taps"], whole.taps) and list(w["blocks"]) == list(range(0, nf, 5))
    shapes = _shapes(tmp_path / "whole.h5")
    extra = set(shapes) - set(_scalar_file_datasets(whole.taps.size, [r.cells for r in whole.recs]))
    assert extra == {"axes", "stencil", "fcc_flag"} and shapes["pre_sos"] == (4, 3, 6) and shapes["axes"] == (3,)
    for i, r in enumerate(whole.recs):
        assert shapes[f"r{i:03d}_f0000000"] == (5, 4) + r.cells and shapes[f"r{i:03d}_acc"] == (4, P) + r.cells and shapes[f"r{i:03d}_state"] == (4, 3, 2) + r.cells
        frames, fs_out, t0 = recordings.read(tmp_path / "whole.h5", i)
        ref = FakeVRecorder(*REGIONS[i], whole.comp, whole.pre_sos, whole.taps, 4, nf, eng.field)
        for n in range(3, sd.Nt):
            eng.n = n
            ref.add()
        want = ref.read()[1]
        assert frames.dtype == np.float32 and frames.shape == (nf, 4) + r.cells
        assert np.array_equal(frames, (want * 0.37).astype(np.float32)) and all(np.abs(frames[:, k]).max() > 0 for k in range(4))
        assert fs_out == 1.0 / (4 * TS) and t0 == (3 - (whole.taps.size - 1) / 2) * TS
        assert np.array_equal(w["acc"][i], ref.get_state()[0]) and np.array_equal(w["state"][i], ref.get_state()[1])
    # a run stopped at step 54 (inside a block, inside an output) and resumed gives the blocks of the uninterrupted run
    path = tmp_path / "rec.h5"
    a = recordings.FieldRecording(path, sd, REGIONS, axes=axes, **KW)
    _run(a, FakeEngine(), 0, 54)
    a.write()
    assert list(recordings.read_file(path)["sampling"]) == [3, 4, 51, 13] and list(recordings.read_file(path)["blocks"]) == [0, 5, 10]
    stopped = path.read_bytes()
    b = recordings.FieldRecording(path, sd, REGIONS, axes=axes, resume_at=54, **KW)
    assert b.count == 51
    eng = FakeEngine()
    b.attach(eng)
    _run(b, eng, 54, sd.Nt)
    b.write()
    assert _shapes(path) == shapes
    for name in shapes:
        assert np.array_equal(h5io.read(path, name), h5io.read(tmp_path / "whole.h5", name)), name
    # every refusal of a resume names its field
    path.write_bytes(stopped)  # (the file of step 54 again)
    other = [REGIONS[0], ((1, 1, 1), (4, 5, 6), (2, 2, 2))]
    kv = dict(axes=axes, **KW)
    for field, args, k2 in (("regions", (sd, other), kv), ("taps", (sd, REGIONS), {**kv, "fpass_hz": 1500.0}), ("taps", (sd, REGIONS), {**kv, "atten_db": 50.0}),
                            ("pre_sos", (sd, REGIONS), {**kv, "lowcut_hz": 20.0}), ("pre_sos", (_sd(h=H * 1.01), REGIONS), kv), ("Ts", (_sd(Ts=TS * 1.01), REGIONS), kv),
                            ("first", (sd, REGIONS), {**kv, "first": 2}), ("factor", (sd, REGIONS), {**kv, "factor": 5}), ("blocks", (sd, REGIONS), {**kv, "cap": 4}),
                            ("axes", (sd, REGIONS), {**kv, "axes": [2, 1]}), ("axes", (sd, REGIONS), {**kv, "axes": [1, 2, 3]}), ("axes", (sd, REGIONS), {**kv, "axes": None}),
                            ("dtype", (sd, REGIONS), {**kv, "dtype": "f8"})):
        with pytest.raises(ValueError, match=f": {field}: "):
            recordings.FieldRecording(path, *args, resume_at=54, **k2)
    with pytest.raises(ValueError, match=": count: "):
        recordings.FieldRecording(path, sd, REGIONS, resume_at=55, **kv)
    # a scalar file is no file of a vector run, and the stencil is compared
    scalar = tmp_path / "scalar.h5"
    s = recordings.FieldRecording(scalar, sd, REGIONS, **KW)
    _run(s, FakeEngine(), 0, 54)
    s.write()
    with pytest.raises(ValueError, match=": axes: "):
        recordings.FieldRecording(scalar, sd, REGIONS, axes=axes, resume_at=54, **KW)
    lat = tmp_path / "lattice.h5"
    fsd = _sd(fcc_flag=1)
    c = recordings.FieldRecording(lat, fsd, REGIONS, axes=axes, stencil="lattice", **KW)
    _run(c, FakeEngine(), 0, 54)
    c.write()
    assert recordings.read_file(lat)["stencil"] == "lattice" and recordings.read_file(lat)["fcc_flag"] == 1 and c.comp.tolist() == [0, 5, 4, 6]
    recordings.FieldRecording(lat, fsd, REGIONS, axes=axes, stencil="lattice", resume_at=54, **KW)
    lat.write_bytes(stopped)  # (an axis file under the lattice run's name)
    with pytest.raises(ValueError, match=": stencil: "):
        recordings.FieldRecording(lat, fsd, REGIONS, axes=axes, stencil="lattice", resume_at=54, **KW)


def test_a_folded_grid_negates_y_in_the_odd_cells(tmp_path):
    sd = _sd(fcc_flag=2, Nt=40)
    path = tmp_path / "folded.h5"
    fr = recordings.FieldRecording(path, sd, REGIONS, axes=[2, 3], stencil="lattice", dtype="f8", **KW)
    assert fr.comp.tolist() == [0, 5, 6] and np.array_equal(fr.pre_sos[1], directional.gradient_sections(TS, H, C, True, 10.0, 4, span=8)[1])
    eng = FakeEngine()
    _run(fr, eng, 0, sd.Nt)
    fr.write()
    f = recordings.read_file(path, raw=True)
    assert f["fcc_flag"] == 2 and f["stencil"] == "lattice" and len(f["iy"]) == 2
    for i, r in enumerate(REGIONS):
        ix, iy, iz, upper = directional.fold_coordinates(r, sd.Ny)
        assert np.array_equal(f["iy"][i], iy) and f["iy"][i].dtype == np.int64 and upper.any() and not upper.all()
        ref = FakeVRecorder(*r, fr.comp, fr.pre_sos, fr.taps, 4, 99, eng.field)
        for n in range(3, sd.Nt):
            eng.n = n
            ref.add()
        raw = ref.read()[1] * 0.37
        frames = recordings.read(path, i)[0]
        sign = np.where(upper, -1.0, 1.0)
        assert np.array_equal(frames[:, 0], raw[:, 0]) and np.array_equal(frames[:, 2], raw[:, 2])  # W and z as stored
        assert np.array_equal(frames[:, 1], raw[:, 1] * sign) and np.abs(frames[:, 1][..., upper]).max() > 0  # y: negated in the odd cells, exactly
        assert np.array_equal(f["acc"][i], ref.get_state()[0]) and np.array_equal(f["state"][i], ref.get_state()[1])  # raw, in storage form


def test_refusals_of_a_vector_recording(tmp_path):
    sd = _sd()
    for field, args, kw in (("axes", (sd, REGIONS), dict(axes=[])), ("axes", (sd, REGIONS), dict(axes=[1, 1])), ("axes", (sd, REGIONS), dict(axes=[4])),
                            ("axes", (sd, REGIONS), dict(axes=[1, 2, 3, 1])), ("stencil", (sd, REGIONS), dict(axes=[1], stencil="box")),
                            ("stencil", (sd, REGIONS), dict(stencil="lattice")), ("fcc_flag", (_sd(fcc_flag=1), REGIONS), dict(axes=[1])),
                            ("fcc_flag", (_sd(fcc_flag=2), REGIONS), dict(axes=[2], stencil="axis")), ('stencil="lattice"', (sd, REGIONS), dict(axes=[1], stencil="lattice")),
                            ("lowcut_hz", (sd, REGIONS), dict(axes=[1], lowcut_hz=0.0)), ("lowcut_order", (sd, REGIONS), dict(axes=[1], lowcut_order=16)),
                            ("h, c", (types.SimpleNamespace(Nt=10, Ts=TS, infac=1.0, Nx=5, Ny=6, Nz=7, diff=True), REGIONS), dict(axes=[1]))):
        with pytest.raises(ValueError, match=field):
            recordings.FieldRecording(tmp_path / "no.h5", *args, **{**KW, **kw})
    assert not (tmp_path / "no.h5").exists()


def test_arguments_are_refused_both_ways_round():
    import argparse

    def parse(*argv):
        p = argparse.ArgumentParser()
        recordings.add_arguments(p)
        a = p.parse_args(list(argv))
        recordings.check_arguments(p, a)
        return a

    base = ("--rec-planes", "x=3", "--rec-factor", "8", "--rec-fpass", "1400")
    a = parse(*base)
    assert a.rec and a.rec_axes == "" and a.rec_stencil == "axis"
    a = parse(*base, "--rec-axes", "y,x", "--rec-stencil", "lattice")
    assert a.rec and a.rec_axes == "y,x" and a.rec_stencil == "lattice" and directional.parse_axes(a.rec_axes) == [2, 1]
    for argv in (("--rec-axes", "x"), ("--rec-stencil", "lattice"), (*base, "--rec-stencil", "lattice"), (*base, "--rec-axes", "w"), (*base, "--rec-axes", "x,x"),
                 (*base, "--rec-stencil", "box")):
        with pytest.raises(SystemExit):
            parse(*argv)
