"""CPU: the host side of the energy decay maps (pffdtd_amd/decay.py): the band filters' edges, the bin of a step, the command line's bands, the
file and the refusals of a resume -- with a band accumulator object that folds in numpy, no device -- and decay.parameters on synthetic decays."""
import types

import numpy as np
import pytest
from scipy.signal import sosfreqz

from pffdtd_amd import decay

TS = 1.0 / 25500.0
REGIONS = [((0, 0, 3), (4, 5, 4), (1, 1, 1)), ((1, 0, 0), (4, 5, 6), (2, 2, 3))]


def _sd(Nt=40, Ts=TS, infac=0.37, diff=True):
    return types.SimpleNamespace(Nt=Nt, Ts=Ts, infac=infac, Nx=4, Ny=5, Nz=6, diff=diff)


class FakeBand:
    """engine.BandAccumulator in numpy: the contract's three lines"""

    def __init__(self, lo, hi, st, pre, bands, nbin, field):
        cells = tuple(-(-(hi[a] - lo[a]) // st[a]) for a in range(3))
        self.sl = tuple(slice(lo[a], hi[a], st[a]) for a in range(3))
        self.pre, self.bands, self.field = np.asarray(pre).reshape(-1, 6), np.asarray(bands), field
        self.shape = (self.bands.shape[0], nbin) + cells
        self.state_shape = (len(self.pre) + self.bands.shape[0] * self.bands.shape[1], 2) + cells
        self.E, self.state, self.count = np.zeros(self.shape), np.zeros(self.state_shape), 0

    def _section(self, k, q, x):
        s = self.state[q]
        y = k[0] * x + s[0]
        s[0] = (k[1] * x - k[4] * y) + s[1]
        s[1] = k[2] * x - k[5] * y
        return y

    def add(self, bin):
        x = self.field()[self.sl].astype(np.float64)
        for q, k in enumerate(self.pre):
            x = self._section(k, q, x)
        for b in range(self.bands.shape[0]):
            y = x
            for s in range(self.bands.shape[1]):
                y = self._section(self.bands[b, s], len(self.pre) + b * self.bands.shape[1] + s, y)
            if bin >= 0:
                self.E[b, bin] = self.E[b, bin] + y * y
        self.count += 1

    def get(self):
        return self.E.copy(), self.state.copy()

    def set(self, sums, state, count):
        self.E = np.zeros(self.shape) if sums is None else np.array(sums, dtype=np.float64).reshape(self.shape)
        self.state = np.zeros(self.state_shape) if state is None else np.array(state, dtype=np.float64).reshape(self.state_shape)
        self.count = count

    def close(self):
        pass


class FakeEngine:
    """u^n = a seeded random field per step"""

    def __init__(self):
        self.n = 0

    def field(self):
        return np.random.default_rng(1000 + self.n).standard_normal((4, 5, 6)).astype(np.float32)

    def band_accumulator(self, lo, hi, stride=(1, 1, 1), pre_sos=None, band_sos=None, nbin=1, depth=0):
        return FakeBand(lo, hi, stride, pre_sos, band_sos, nbin, self.field)


def test_band_edges_hold_half_the_power():
    """Butterworth through the prewarped bilinear map is exact at its edges: |H|^2 = 1/2 at fc / sqrt 2 and fc * sqrt 2"""
    fcs = [63.0, 125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0]
    for order in (3, 4):
        sos = decay.band_sections(TS, fcs, order)
        assert sos.shape == (len(fcs), order, 6) and np.all(sos[:, :, 3] == 1.0)
        for fc, s in zip(fcs, sos):
            edges = np.array([fc / np.sqrt(2.0), fc * np.sqrt(2.0)])
            _, h = sosfreqz(s, worN=2.0 * np.pi * edges * TS)
            p = np.abs(h) ** 2
            print(f"order {order}, {fc:g} Hz: |H|^2 at the edges {p[0]:.12f} {p[1]:.12f}")
            assert np.all(np.abs(p - 0.5) <= 1e-9), (order, fc, p)
    with pytest.raises(ValueError, match="8000 Hz band"):
        decay.band_sections(1.0 / 22000.0, [1000.0, 8000.0], 3)  # 8000 * sqrt 2 > 11000
    with pytest.raises(ValueError, match="bands"):
        decay.FieldDecay("unused.h5", _sd(), REGIONS, [10000.0], 5.0)


def test_pre_sections_are_those_of_process_outputs():
    from scipy.signal import bilinear_zpk, butter, zpk2sos
    z, p, k = butter(4, 10.0 * 2 * np.pi, btype="high", analog=True, output="zpk")
    want = zpk2sos(*bilinear_zpk(z[1:], p, k, 1 / TS))
    assert np.array_equal(decay.pre_sections(TS, True, 10.0, 4), want) and want.shape == (2, 6)
    assert np.array_equal(decay.pre_sections(TS, False, 10.0, 4), butter(4, 2 * TS * 10.0, btype="high", output="sos"))
    assert decay.pre_sections(TS, False, 0.0, 4).shape == (0, 6)
    with pytest.raises(ValueError, match="lowcut_hz"):
        decay.pre_sections(TS, True, 0.0, 4)


def test_bins_and_sample_steps():
    sd = _sd(Nt=1000)
    fd = decay.FieldDecay("unused.h5", sd, REGIONS, [125.0, 250.0], 5.0, first=7)
    assert fd.bin_steps == round(5e-3 / TS) == 128  # 127.5 rounds to the even neighbour
    assert fd.nbin == -(-(1000 - 7) // 128)
    assert [fd.bin_of(n) for n in (7, 8, 134, 135, 262, 263, 999)] == [0, 0, 0, 1, 1, 2, 7] and fd.bin_of(999) == fd.nbin - 1
    assert [fd.samples_below(n) for n in (0, 7, 8, 100)] == [0, 0, 1, 93]
    assert not fd.due(6) and fd.due(7) and fd.due(999) and not fd.due(1000)
    assert fd.next_step(0) == 7 and fd.next_step(7) == 7 and fd.next_step(8) == 8
    with pytest.raises(ValueError, match="no sample is due"):
        fd.take(FakeEngine(), 3)
    with pytest.raises(ValueError, match="bin_ms"):
        decay.FieldDecay("unused.h5", sd, REGIONS, [125.0], 0.01)
    with pytest.raises(ValueError, match="bands"):
        decay.FieldDecay("unused.h5", sd, REGIONS, [125.0] * 17, 5.0)


def test_parse_bands():
    assert np.array_equal(decay.parse_bands("125,250,500"), [125.0, 250.0, 500.0])
    assert np.array_equal(decay.parse_bands(" 63 "), [63.0])
    for bad in ("", "a,b", "-5", "0", "125,nan"):
        with pytest.raises(ValueError, match="decay-bands"):
            decay.parse_bands(bad)


def _run(fd, eng, n0, n1):
    for n in range(n0, n1):
        eng.n = n
        if fd.due(n):
            fd.take(eng, n)


def test_file_and_resume(tmp_path):
    sd = _sd(Nt=40)
    kw = dict(bands_hz=[500.0, 1000.0], bin_ms=0.4, first=3)
    path = tmp_path / "decay.h5"
    whole = decay.FieldDecay(tmp_path / "whole.h5", sd, REGIONS, **kw)
    assert whole.bin_steps == 10
    _run(whole, FakeEngine(), 0, 40)
    whole.write()
    w = decay.read(tmp_path / "whole.h5", raw=True)
    assert list(w["sampling"]) == [3, 10, 37] and np.array_equal(w["regions"], whole.table) and np.array_equal(w["bands"], [500.0, 1000.0])
    assert np.array_equal(w["pre_sos"], whole.pre_sos) and np.array_equal(w["band_sos"], whole.band_sos) and w["Ts"] == TS
    for i in range(2):
        assert w["E"][i].shape == (2, 4) + whole.accs[i].shape[2:] and np.array_equal(w["E"][i], w["sums"][i] * (0.37 * 0.37)) and w["E"][i].max() > 0
    # a run stopped at step 17 and resumed
    a = decay.FieldDecay(path, sd, REGIONS, **kw)
    _run(a, FakeEngine(), 0, 17)
    a.write()
    assert not (tmp_path / "decay.h5.tmp").exists()
    b = decay.FieldDecay(path, sd, REGIONS, resume_at=17, **kw)
    assert b.count == 14
    eng = FakeEngine()
    b.attach(eng)
    _run(b, eng, 17, 40)
    b.write()
    r = decay.read(path, raw=True)
    for key in ("E", "sums", "state"):
        for i in range(2):
            assert np.array_equal(r[key][i], w[key][i]), (key, i)
    assert list(r["sampling"]) == [3, 10, 37]
    # every refusal names its field
    a.write()  # (the file of step 17 again)
    other = [REGIONS[0], ((0, 0, 0), (4, 5, 6), (2, 2, 3))]
    for field, args, k2 in (("regions", (sd, other), kw), ("bands", (sd, REGIONS), {**kw, "bands_hz": [500.0, 2000.0]}), ("pre_sos", (sd, REGIONS), {**kw, "lowcut_hz": 20.0}),
                            ("band_sos", (sd, REGIONS), {**kw, "order": 4}), ("Ts", (_sd(Ts=TS * 1.5), REGIONS), {**kw, "bin_ms": 0.6}),
                            ("first", (sd, REGIONS), {**kw, "first": 2}), ("bin_steps", (sd, REGIONS), {**kw, "bin_ms": 0.5})):
        with pytest.raises(ValueError, match=f": {field}: "):
            decay.FieldDecay(path, *args, resume_at=17, **k2)
    with pytest.raises(ValueError, match=": count: "):
        decay.FieldDecay(path, sd, REGIONS, resume_at=18, **kw)
    with pytest.raises(ValueError, match="no decay file"):
        decay.FieldDecay(tmp_path / "missing.h5", sd, REGIONS, resume_at=17, **kw)


def test_parameters_of_an_exponential_decay():
    """E_k = exp(-13.8 t_k / T) carried to -100 dB: the EDC's slope in dB is exactly -10 * 13.8 / (T ln 10) per second up to the tail's truncation,
    whose error at -35 dB is below 1e-6 dB: T20 and T30 within 1e-4, EDT (three bins of 0 .. -10 dB fewer than T30 has) within 1e-3"""
    dt = 5e-3
    for T in (0.4, 1.3):
        nbin = int(np.ceil(100.0 / (10.0 * 13.8 / (T * np.log(10.0))) / dt)) + 1
        t = np.arange(nbin) * dt
        E = np.exp(-13.8 * t / T)
        assert 10 * np.log10(E[-1]) <= -100.0
        E4 = np.stack([E, 3.0 * E]).reshape(2, nbin, 1, 1, 1) * np.ones((1, 1, 1, 2, 3))
        p = decay.parameters(E4, dt)
        want = T * 6.0 * np.log(10.0) / 13.8  # the time of 60 dB at that slope
        assert p["T20"].shape == (2, 1, 2, 3) and p["edc"].shape == E4.shape
        print(f"T {T}: EDT {p['EDT'][0, 0, 0, 0]:.8f} T20 {p['T20'][0, 0, 0, 0]:.8f} T30 {p['T30'][0, 0, 0, 0]:.8f}, expected {want:.8f}")
        assert np.allclose(p["T20"], want, rtol=1e-4, atol=0) and np.allclose(p["T30"], want, rtol=1e-4, atol=0)
        assert np.allclose(p["EDT"], want, rtol=1e-3, atol=0)
        assert np.array_equal(p["edc"][:, 0], E4.sum(axis=1)) or np.allclose(p["edc"][:, 0], E4.sum(axis=1), rtol=1e-13)
    silent = decay.parameters(np.zeros((3, 1, 1, 1)), dt)
    assert np.isnan(silent["T30"]).all()


def test_a_delayed_onset_moves_the_split():
    """C80 splits 80 ms after the onset: a decay delayed by d bins splits d bins later, so C80, C50 and D50 do not change"""
    dt, T, nbin = 5e-3, 0.8, 400
    E = np.exp(-13.8 * np.arange(nbin) * dt / T)
    base = decay.parameters(E.reshape(nbin, 1, 1, 1), dt)
    k80 = round(0.08 / dt)
    want = 10 * np.log10(E[:k80].sum() / E[k80:].sum())
    assert abs(base["C80"][0, 0, 0] - want) <= 1e-12
    for d in (1, 7, 30):
        delayed = np.concatenate([np.full(d, 1e-9), E[:nbin - d]])  # a noise floor 90 dB down before the onset: not the onset
        p = decay.parameters(delayed.reshape(nbin, 1, 1, 1), dt)
        early, late = delayed[d:d + k80].sum(), delayed[d + k80:].sum()
        assert abs(p["C80"][0, 0, 0] - 10 * np.log10(early / late)) <= 1e-12, d
        # a split that had stayed at bin k80 would count d bins of the decay's start as late energy
        wrong = 10 * np.log10(delayed[:k80].sum() / delayed[k80:].sum())
        assert abs(p["C80"][0, 0, 0] - wrong) > 0.05, d
        assert abs(p["C80"][0, 0, 0] - base["C80"][0, 0, 0]) < 0.01 and abs(p["D50"][0, 0, 0] - base["D50"][0, 0, 0]) < 1e-3
