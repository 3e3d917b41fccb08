"""CPU: the host side of the directional band maps (pffdtd_amd/directional.py): the gradient's sections against their definition and against a plane
wave, LF / LFC / intensity of hand-made sums, the file and the refusals of a resume -- with a vector band accumulator object that folds in numpy,
no device."""
import types

import numpy as np
import pytest
from scipy.signal import butter, sosfreqz

from pffdtd_amd import decay, directional

TS = 1.0 / 25500.0
C, H = 343.0, 343.0 * TS * np.sqrt(3.0)  # the Cartesian scheme's stability limit: h = c Ts sqrt 3
N = (5, 6, 7)
REGIONS = [((1, 1, 3), (4, 5, 4), (1, 1, 1)), ((1, 1, 1), (4, 5, 6), (2, 2, 3))]


def _sd(Nt=40, Ts=TS, infac=0.37, diff=True, h=H, fcc_flag=0):
    return types.SimpleNamespace(Nt=Nt, Ts=Ts, infac=infac, Nx=N[0], Ny=N[1], Nz=N[2], diff=diff, h=h, c=C, fcc_flag=fcc_flag)


def _section(k, s, x):
    """the contract's three lines; k: a scipy row, s: [2, ...] state, changed in place"""
    y = k[0] * x + s[0]
    s[0] = (k[1] * x - k[4] * y) + s[1]
    s[1] = k[2] * x - k[5] * y
    return y


class FakeVBand:
    """engine.VectorBandAccumulator in numpy: the contract's lines"""

    def __init__(self, lo, hi, st, comp, pre, bands, prod, nbin, field):
        cells = tuple(-(-(hi[a] - lo[a]) // st[a]) for a in range(3))
        self.lo, self.hi, self.st, self.comp, self.field = lo, hi, st, [int(c) for c in comp], field
        self.pre, self.bands, self.prod = np.asarray(pre), np.asarray(bands), [tuple(int(v) for v in p) for p in prod]
        self.shape = (len(self.prod), self.bands.shape[0], nbin) + cells
        self.state_shape = (len(self.comp), self.pre.shape[1] + self.bands.shape[0] * self.bands.shape[1], 2) + cells
        self.S, self.state, self.count = np.zeros(self.shape), np.zeros(self.state_shape), 0

    def _sl(self, axis, shift):
        return tuple(slice(self.lo[a] + (shift if a == axis else 0), self.hi[a] + (shift if a == axis else 0), self.st[a]) for a in range(3))

    def add(self, bin):
        u = self.field()
        npre, nsec = self.pre.shape[1], self.bands.shape[1]
        xs = []
        for c, k in enumerate(self.comp):
            x = (u[self._sl(-1, 0)] if k == 0 else u[self._sl(k - 1, 1)] - u[self._sl(k - 1, -1)]).astype(np.float64)
            for q in range(npre):
                x = _section(self.pre[c, q], self.state[c, q], x)
            xs.append(x)
        for b in range(self.bands.shape[0]):
            ys = []
            for c, x in enumerate(xs):
                for s in range(nsec):
                    x = _section(self.bands[b, s], self.state[c, npre + b * nsec + s], x)
                ys.append(x)
            if bin >= 0:
                for p, (i, j, mode) in enumerate(self.prod):
                    self.S[p, b, bin] = self.S[p, b, bin] + (np.fabs(ys[i] * ys[j]) if mode else ys[i] * ys[j])
        self.count += 1

    def get(self):
        return self.S.copy(), self.state.copy()

    def set(self, sums, state, count):
        self.S = np.zeros(self.shape) if sums is None else np.array(sums, dtype=np.float64).reshape(self.shape)
        self.state = np.zeros(self.state_shape) if state is None else np.array(state, dtype=np.float64).reshape(self.state_shape)
        self.count = count

    def close(self):
        pass


class FakeEngine:
    """u^n = a seeded random field per step"""

    def __init__(self):
        self.n = 0

    def field(self):
        return np.random.default_rng(2000 + self.n).standard_normal(N).astype(np.float32)

    def vector_band_accumulator(self, lo, hi, stride=(1, 1, 1), comp=(0,), pre_sos=None, band_sos=None, prod=((0, 0, 0),), nbin=1, depth=0):
        return FakeVBand(lo, hi, stride, comp, pre_sos, band_sos, prod, nbin, self.field)


def test_gradient_sections_against_their_definition():
    for diff in (True, False):
        omni, grad = directional.gradient_sections(TS, H, C, diff, 10.0, 4)
        pre = decay.pre_sections(TS, diff, 10.0, 4)
        assert omni.shape == grad.shape == (len(pre) + 1, 6)
        assert np.array_equal(omni[:-1], pre) and np.array_equal(grad[:-1], pre) and np.array_equal(omni[-1], [1, 0, 0, 1, 0, 0])
        b, a = butter(1, 2 * TS * 10.0, btype="high")
        g = -(C / (2 * H)) * (TS / 2) * b[0]
        assert np.array_equal(grad[-1], [g, g, 0.0, 1.0, a[1], 0.0]) and g < 0 and 0 < -a[1] < 1
        # the section is the bilinear integrator times the first-order high-pass, the pole at 1 cancelled: compare the responses away from 0 Hz
        w = 2 * np.pi * np.array([20.0, 100.0, 1000.0, 5000.0]) * TS
        z = np.exp(-1j * w)
        want = -(C / (2 * H)) * (TS / 2) * (1 + z) / (1 - z) * (b[0] + b[1] * z) / (1 + a[1] * z)
        _, got = sosfreqz(grad[-1:], worN=w)
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))
    with pytest.raises(ValueError, match="lowcut_hz"):
        directional.gradient_sections(TS, H, C, False, 0.0, 4)
    assert directional.parse_axes("y") == [2] and directional.parse_axes(" y, x ,z") == [2, 1, 3]
    for bad in ("", "w", "x,x", "x,y,z,x"):
        with pytest.raises(ValueError, match="dir-axes"):
            directional.parse_axes(bad)
    assert np.array_equal(directional.products(2), [(0, 0, 0), (1, 1, 0), (0, 1, 0), (0, 1, 1), (2, 2, 0), (0, 2, 0), (0, 2, 1)])


@pytest.mark.parametrize("f", [125.0, 1000.0])
@pytest.mark.parametrize("deg", [0.0, 60.0, 90.0, 180.0])
def test_a_plane_wave_gives_the_cosine(f, deg):
    """A tone of frequency f as a plane wave at angle theta to the axis, sampled at three cells, through the last gradient section by the contract's
    lines.  After the transient (pole radius a: a^n < 1e-9 of the amplitude) the output is a tone whose amplitude against the pressure's is
    |G(e^{j omega})| * 2 sin(omega h cos(theta) / c) to 1e-6 relative, and that value lies within
        (omega h / c)^2 / 6 + (omega Ts)^2 / 12 + (f_lowcut / f)^2 / 2
    of cos(theta).  Each term bounds one factor of  model / cos(theta) = [sin(x cos) / (x cos)] * [y cot y] * |HP|,  x = omega h / c, y = omega Ts / 2:
    the sinc of the central difference, sin(u) / u >= 1 - u^2 / 6; the bilinear integrator, y cot y = 1 - y^2 / 3 - y^4 / 45 - ... (the y^4 term,
    below 6e-6 here, is covered by the cross terms the sum of the three bounds leaves out, above 3e-8 at 125 Hz and 1e-4 at 1 kHz); the first-order
    high-pass, 1 / sqrt(1 + r^2) >= 1 - r^2 / 2 with r = tan(pi f_lowcut Ts) / tan(pi f Ts) <= f_lowcut / f."""
    lowcut = 10.0
    theta = np.deg2rad(deg)
    cos_t = np.cos(theta) if deg != 90.0 else 0.0
    _, grad = directional.gradient_sections(TS, H, C, True, lowcut, 4)
    last = grad[-1]
    radius = last[4] * -1.0
    nwait = int(np.ceil(np.log(1e-9 * 1e-3) / np.log(radius)))  # the transient's start is below 1e3 amplitudes (|g| (1 + a) / (1 - a) * 2)
    w = 2 * np.pi * f
    n = np.arange(nwait + 4096)
    t = n * TS
    delay = H * cos_t / C
    lo_, mid, hi_ = np.sin(w * (t + delay)), np.sin(w * t), np.sin(w * (t - delay))  # the cells at -h, 0, +h along the axis
    d = hi_ - lo_
    b0, b1, b2, a1, a2 = (float(last[i]) for i in (0, 1, 2, 4, 5))
    s1 = s2 = 0.0
    y = np.empty_like(d)
    for i, x in enumerate(d.tolist()):  # the contract's three lines on Python floats: the same doubles, the same association
        v = b0 * x + s1
        s1 = (b1 * x - a1 * v) + s2
        s2 = b2 * x - a2 * v
        y[i] = v
    tail = slice(nwait, None)
    basis = np.stack([np.sin(w * t[tail]), np.cos(w * t[tail])], axis=1)
    coef, res, _, _ = np.linalg.lstsq(basis, y[tail], rcond=None)
    amp = np.hypot(*coef)
    assert np.abs(basis @ coef - y[tail]).max() <= 1e-9 * max(amp, 1.0)  # a pure tone: the transient is gone
    _, G = sosfreqz(last[None], worN=[w * TS])
    model = np.abs(G[0]) * 2 * np.sin(w * H * cos_t / C)  # signed with cos(theta)
    bound = (w * H / C) ** 2 / 6 + (w * TS) ** 2 / 12 + (lowcut / f) ** 2 / 2
    print(f"f {f:g} Hz, theta {deg:g}: amplitude {amp:.9f}, model {model:.9f}, cos {cos_t:.9f}, bound {bound:.3e}")
    if deg == 90.0:
        assert amp <= 1e-9 and model == 0.0
        return
    assert abs(amp - abs(model)) <= 1e-6 * abs(model)
    assert abs(model - cos_t) <= bound
    # the sign: in phase with the pressure for theta < 90 degrees, in antiphase beyond (the in-phase coefficient carries it)
    assert np.sign(coef[0]) == np.sign(cos_t) and abs(coef[0]) > 0.9 * amp


def test_lf_and_lfc_of_hand_made_sums():
    prod = directional.products(2)
    nbin, cells = 24, (1, 1, 2)
    S = np.zeros((7, 1, nbin) + cells)
    # cell 0: onset at bin 2, 5 ms bins: omni energy 1 per bin over 20 bins; lateral (component 1) 0.25 per bin, |p p_1| 0.5, component 2 nothing
    S[0, 0, 2:22, 0, 0, 0] = 1.0
    S[1, 0, 2:22, 0, 0, 0] = 0.25
    S[2, 0, 2:22, 0, 0, 0] = -0.5
    S[3, 0, 2:22, 0, 0, 0] = 0.5
    # cell 1: silent
    out = directional.parameters(S, prod, 0.005)
    assert out["LF"].shape == out["LFC"].shape == (2, 1) + cells and out["intensity"].shape == (2, 1, nbin) + cells
    assert out["onset"][0, 0, 0, 0] == 2
    # 5 .. 80 ms = bins 1 .. 15 after the onset (15 bins), 0 .. 80 ms = 16 bins
    assert out["LF"][0, 0, 0, 0, 0] == 0.25 * 15 / 16 and out["LFC"][0, 0, 0, 0, 0] == 0.5 * 15 / 16
    assert out["LF"][1, 0, 0, 0, 0] == 0.0 and out["LFC"][1, 0, 0, 0, 0] == 0.0
    assert np.isnan(out["LF"][0, 0, 0, 0, 1])
    assert np.array_equal(out["intensity"][0], S[2]) and out["intensity_total"][0, 0, 0, 0, 0] == -10.0 and not out["intensity_total"][1].any()
    # 1 ms bins: the same cell, every 5 ms bin spread over five
    S1 = np.repeat(S, 5, axis=2) / 5.0
    out1 = directional.parameters(S1, prod, 0.001)
    assert abs(out1["LF"][0, 0, 0, 0, 0] - 0.25 * 75 / 80) < 1e-12 and out1["onset"][0, 0, 0, 0] == 10
    # the refusals
    # a bin is a whole number of steps: 128 steps of 1 / 25500 s are 5.0196 ms, the nominal 5 ms bin -- the same limits; 2 % off is no such bin
    near = directional.parameters(S, prod, 128 * TS)
    assert np.array_equal(near["LF"], out["LF"], equal_nan=True) and np.array_equal(near["LFC"], out["LFC"], equal_nan=True)
    for bs in (0.004, 0.003, 0.0075, 0.0051, 0.0049):
        with pytest.raises(ValueError, match="bin_seconds"):
            directional.parameters(S, prod, bs)
    with pytest.raises(ValueError, match="S: shape"):
        directional.parameters(S[:6], prod, 0.005)
    with pytest.raises(ValueError, match="prod: no row"):
        directional.parameters(S[1:], prod[1:], 0.005)
    with pytest.raises(ValueError, match="prod: no row"):
        directional.parameters(S[:6], prod[:6], 0.005)


def _run(fd, eng, n0, n1):
    for n in range(n0, n1):
        eng.n = n
        if fd.due(n):
            fd.take(eng, n)


def test_refusals_of_field_directional():
    sd = _sd()
    kw = dict(bands_hz=[500.0], axes=[2], bin_ms=0.4)
    for field, args, k2 in (("axes", (sd, REGIONS), {**kw, "axes": []}), ("axes", (sd, REGIONS), {**kw, "axes": [2, 2]}), ("axes", (sd, REGIONS), {**kw, "axes": [4]}),
                            ("bands", (sd, REGIONS), {**kw, "bands_hz": [500.0] * 17}), ("bands", (sd, REGIONS), {**kw, "bands_hz": [10000.0]}),
                            ("bin_ms", (sd, REGIONS), {**kw, "bin_ms": 0.01}), ("lowcut_hz", (sd, REGIONS), {**kw, "lowcut_hz": 0.0}),
                            ("fcc_flag", (_sd(fcc_flag=1), REGIONS), kw), ("at least one region", (sd, []), kw), ("lowcut_order", (sd, REGIONS), {**kw, "lowcut_order": 16})):
        with pytest.raises(ValueError, match=field):
            directional.FieldDirectional("unused.h5", *args, **k2)
    fd = directional.FieldDirectional("unused.h5", _sd(Nt=1000), REGIONS, [125.0], [2, 1], 5.0, first=7)
    assert fd.bin_steps == 128 and fd.nbin == -(-(1000 - 7) // 128) and fd.comp.tolist() == [0, 2, 1] and fd.pre_sos.shape == (3, 3, 6) and fd.prod.shape == (7, 3)
    assert [fd.bin_of(n) for n in (7, 134, 135, 999)] == [0, 0, 1, 7] and not fd.due(6) and fd.due(7) and not fd.due(1000) and fd.next_step(0) == 7
    with pytest.raises(ValueError, match="no sample is due"):
        fd.take(FakeEngine(), 3)


def test_file_and_resume(tmp_path):
    sd = _sd(Nt=40)
    kw = dict(bands_hz=[500.0, 1000.0], axes=[2, 3], bin_ms=0.4, first=3)
    path = tmp_path / "dir.h5"
    whole = directional.FieldDirectional(tmp_path / "whole.h5", sd, REGIONS, **kw)
    assert whole.bin_steps == 10
    _run(whole, FakeEngine(), 0, 40)
    whole.write()
    w = directional.read(tmp_path / "whole.h5", raw=True)
    assert list(w["sampling"]) == [3, 10, 37] and np.array_equal(w["regions"], whole.table) and np.array_equal(w["bands"], [500.0, 1000.0]) and list(w["axes"]) == [2, 3]
    assert np.array_equal(w["pre_sos"], whole.pre_sos) and np.array_equal(w["band_sos"], whole.band_sos) and np.array_equal(w["prod"], whole.prod) and w["Ts"] == TS
    for i in range(2):
        assert w["S"][i].shape == (7, 2, 4) + whole.accs[i].shape[3:] and np.array_equal(w["S"][i], w["sums"][i] * (0.37 * 0.37)) and w["S"][i].max() > 0
        assert w["S"][i][2].min() < 0 and w["S"][i][3].min() >= 0  # a plain product takes both signs, an absolute one does not
    # a run stopped at step 17 and resumed
    a = directional.FieldDirectional(path, sd, REGIONS, **kw)
    _run(a, FakeEngine(), 0, 17)
    a.write()
    assert not (tmp_path / "dir.h5.tmp").exists()
    b = directional.FieldDirectional(path, sd, REGIONS, resume_at=17, **kw)
    assert b.count == 14
    eng = FakeEngine()
    b.attach(eng)
    _run(b, eng, 17, 40)
    b.write()
    r = directional.read(path, raw=True)
    for key in ("S", "sums", "state"):
        for i in range(2):
            assert np.array_equal(r[key][i], w[key][i]), (key, i)
    assert list(r["sampling"]) == [3, 10, 37]
    # every refusal names its field
    a.write()  # (the file of step 17 again)
    other = [REGIONS[0], ((1, 1, 1), (4, 5, 6), (2, 2, 2))]
    for field, args, k2 in (("regions", (sd, other), kw), ("bands", (sd, REGIONS), {**kw, "bands_hz": [500.0, 2000.0]}), ("axes", (sd, REGIONS), {**kw, "axes": [3, 2]}),
                            ("pre_sos", (sd, REGIONS), {**kw, "lowcut_hz": 20.0}), ("pre_sos", (_sd(h=H * 1.01), REGIONS), kw),
                            ("band_sos", (sd, REGIONS), {**kw, "order": 4}), ("Ts", (_sd(Ts=TS * 1.5), REGIONS), {**kw, "bin_ms": 0.6}),
                            ("first", (sd, REGIONS), {**kw, "first": 2}), ("bin_steps", (sd, REGIONS), {**kw, "bin_ms": 0.5})):
        with pytest.raises(ValueError, match=f": {field}: "):
            directional.FieldDirectional(path, *args, resume_at=17, **k2)
    with pytest.raises(ValueError, match=": count: "):
        directional.FieldDirectional(path, sd, REGIONS, resume_at=18, **kw)
    with pytest.raises(ValueError, match="no directional file"):
        directional.FieldDirectional(tmp_path / "missing.h5", sd, REGIONS, resume_at=17, **kw)
