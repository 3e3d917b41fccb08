"""CPU: the host side of field spectra (pffdtd_amd/spectra.py): frequencies of the command line, the weights of a sample, the sample steps, the
file and the refusals of a resume -- with an accumulator object that folds in numpy, no device."""
import types

import numpy as np
import pytest

from pffdtd_amd import spectra

TS = 1.0 / 48000.0
REGIONS = [((0, 0, 3), (4, 5, 4), (1, 1, 1)), ((1, 0, 0), (4, 5, 6), (2, 2, 3))]


def _sd(Nt=40, Ts=TS, infac=0.37):
    return types.SimpleNamespace(Nt=Nt, Ts=Ts, infac=infac, Nx=4, Ny=5, Nz=6)


class FakeAcc:
    def __init__(self, lo, hi, st, nchan):
        self.shape = (nchan,) + tuple(-(-(hi[a] - lo[a]) // st[a]) for a in range(3))
        self.sl = tuple(slice(lo[a], hi[a], st[a]) for a in range(3))
        self.acc, self.count, self.field = np.zeros(self.shape), 0, None

    def add(self, w):
        u = self.field()[self.sl].astype(np.float64)
        for m in range(self.shape[0]):
            self.acc[m] += w[m] * u
        self.count += 1

    def get(self):
        return self.acc.copy()

    def set(self, a, count):
        self.acc = np.zeros(self.shape) if a is None else np.array(a, dtype=np.float64).reshape(self.shape)
        self.count = count

    def close(self):
        pass


class FakeEngine:
    """u^n = a seeded random field per step"""

    def __init__(self):
        self.n = 0

    def field(self):
        return np.random.default_rng(1000 + self.n).standard_normal((4, 5, 6)).astype(np.float32)

    def accumulator(self, lo, hi, stride=(1, 1, 1), nchan=1, depth=0):
        a = FakeAcc(lo, hi, stride, nchan)
        a.field = self.field
        return a


def test_parse_freqs():
    assert np.array_equal(spectra.parse_freqs("63,125,250"), [63.0, 125.0, 250.0])
    assert np.array_equal(spectra.parse_freqs(" 31.5 "), [31.5])
    assert np.array_equal(spectra.parse_freqs("100:200:5"), np.linspace(100.0, 200.0, 5))  # linear, both ends
    assert np.array_equal(spectra.parse_freqs("50:50:1"), [50.0])
    for bad in ("", "a,b", "1:2", "1:2:0", "-5", "1:2:x"):
        with pytest.raises(ValueError, match="spectrum-freqs"):
            spectra.parse_freqs(bad)


def test_weights():
    sd = _sd(Nt=2000)
    fs = spectra.FieldSpectrum("unused.h5", sd, REGIONS, [0.0, 1.0 / (4.0 * TS)])
    want = [(1, 0), (0, -1), (-1, 0), (0, 1)]
    for n in list(range(8)) + [996, 997, 998, 999, 1000]:
        w = fs.weights(n)
        assert w.shape == (4,) and w.dtype == np.float64
        assert w[0] == 1.0 and w[1] == 0.0  # f = 0: exactly (1, -0.0 or 0.0)
        # phi = 2 pi ((f Ts n) mod 1): f Ts is 1/4 to within an ulp, so phi is off by at most 2 pi * n * 2^-53 < 1e-12 for n <= 1000
        assert abs(w[2] - want[n % 4][0]) <= 1e-12 and abs(w[3] - want[n % 4][1]) <= 1e-12, (n, w)
    f = 1234.5
    w = spectra.FieldSpectrum("unused.h5", sd, REGIONS, [f]).weights(77)
    phi = 2.0 * np.pi * ((f * TS * 77) % 1.0)
    assert w[0] == np.cos(phi) and w[1] == -np.sin(phi)


def test_hann_window_and_nyquist():
    sd = _sd(Nt=41)
    fs = spectra.FieldSpectrum("unused.h5", sd, REGIONS, [0.0], every=4, first=3, window="hann")
    steps = list(range(3, 41, 4))
    assert fs.nsamples == len(steps) == 10
    g = [fs.weights(n)[0] for n in steps]
    assert g[0] == 0.0 and g[-1] == 0.0 and all(0 < v <= 1 for v in g[1:-1])  # the end points
    assert np.allclose(g, 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(10) / 9), rtol=0, atol=1e-14)
    assert abs(g[4] - g[5]) < 1e-14 and abs(g[1] - g[8]) < 1e-14  # symmetric
    assert all(fs.weights(n)[1] == 0.0 for n in steps)
    with pytest.raises(ValueError, match="window"):
        spectra.FieldSpectrum("unused.h5", sd, REGIONS, [0.0], window="hamming")
    # f >= 1 / (2 every Ts) is refused: such samples cannot tell it from its alias
    nyq = 1.0 / (2.0 * TS)
    spectra.FieldSpectrum("unused.h5", sd, REGIONS, [np.nextafter(nyq, 0)])
    for every, f in ((1, nyq), (1, 2 * nyq), (2, nyq / 2), (3, 9000.0)):
        with pytest.raises(ValueError, match="freqs"):
            spectra.FieldSpectrum("unused.h5", sd, REGIONS, [100.0, f], every=every)
    with pytest.raises(ValueError, match="freqs"):
        spectra.FieldSpectrum("unused.h5", sd, REGIONS, [-1.0])
    with pytest.raises(ValueError):
        spectra.FieldSpectrum("unused.h5", sd, [], [10.0])
    with pytest.raises(ValueError):
        spectra.FieldSpectrum("unused.h5", sd, REGIONS, [10.0], every=0)


def test_next_step_and_due():
    sd = _sd(Nt=20)
    fs = spectra.FieldSpectrum("unused.h5", sd, REGIONS, [100.0], every=6, first=2)
    assert [fs.next_step(n) for n in (0, 2, 3, 8, 9, 14, 15, 20, 21)] == [2, 2, 8, 8, 14, 14, 20, 20, 26]
    assert [n for n in range(30) if fs.due(n)] == [2, 8, 14]  # (20 is not below Nt)
    assert [fs.samples_below(n) for n in (0, 2, 3, 8, 9, 20)] == [0, 0, 1, 1, 2, 3]
    one = spectra.FieldSpectrum("unused.h5", sd, REGIONS, [100.0])
    assert all(one.due(n) and one.next_step(n) == n for n in range(20)) and not one.due(20)
    with pytest.raises(ValueError, match="no sample is due"):
        fs.take(FakeEngine(), 3)


def _run(fs, eng, n0, n1):
    for n in range(n0, n1):
        eng.n = n
        if fs.due(n):
            assert fs.take(eng, n) == n


def test_file_round_trip_and_resume(tmp_path):
    sd = _sd()
    freqs = [63.0, 125.0, 250.0]
    kw = dict(every=3, first=4, window="hann")
    path = tmp_path / "sim_spectra.h5"
    eng = FakeEngine()
    fs = spectra.FieldSpectrum(path, sd, REGIONS, freqs, **kw)
    _run(fs, eng, 0, sd.Nt)
    fs.write()
    assert not (tmp_path / "sim_spectra.h5.tmp").exists()  # moved into place
    f = spectra.read(path)
    assert np.array_equal(f["regions"], [lo + hi + st for lo, hi, st in REGIONS]) and np.array_equal(f["freqs"], freqs) and f["Ts"] == TS
    assert list(f["sampling"]) == [4, 3, 12] and f["window"] == 1
    for i, (lo, hi, st) in enumerate(REGIONS):
        acc = np.zeros((6,) + fs.accs[i].shape[1:])
        for n in range(4, sd.Nt, 3):
            eng.n = n
            w = fs.weights(n)
            u = eng.field()[tuple(slice(lo[a], hi[a], st[a]) for a in range(3))].astype(np.float64)
            for m in range(6):
                acc[m] += w[m] * u
        assert f["re"][i].shape == (3,) + acc.shape[1:] and f["re"][i].dtype == np.float64
        assert np.array_equal(f["re"][i], acc[0::2] * sd.infac) and np.array_equal(f["im"][i], acc[1::2] * sd.infac)  # a single multiplication
        assert np.abs(f["im"][i]).max() > 0
    # stopped before step 19 and resumed there: the file of the run in one piece
    part = tmp_path / "part.h5"
    a = spectra.FieldSpectrum(part, sd, REGIONS, freqs, **kw)
    _run(a, eng, 0, 19)
    a.write()
    assert list(spectra.read(part)["sampling"]) == [4, 3, 5]
    b = spectra.FieldSpectrum(part, sd, REGIONS, freqs, resume_at=19, **kw)
    assert b.count == 5
    _run(b, FakeEngine(), 19, sd.Nt)
    b.write()
    g = spectra.read(part)
    assert list(g["sampling"]) == [4, 3, 12]
    assert all(np.array_equal(x, y) for k in ("re", "im") for x, y in zip(f[k], g[k]))
    # refusals, by the field's name
    a = spectra.FieldSpectrum(part, sd, REGIONS, freqs, **kw)
    _run(a, eng, 0, 19)
    a.write()
    other = [REGIONS[0], ((0, 0, 0), (4, 5, 6), (2, 2, 3))]
    for field, args, kws in (("regions", (other, freqs), kw), ("freqs", (REGIONS, [63.0, 125.0, 251.0]), kw), ("first", (REGIONS, freqs), {**kw, "first": 1}),
                             ("every", (REGIONS, freqs), {**kw, "every": 2}), ("window", (REGIONS, freqs), {**kw, "window": None})):
        with pytest.raises(ValueError, match=field):
            spectra.FieldSpectrum(part, sd, *args, resume_at=19, **kws)
    for at in (16, 20, 40):  # 5 samples lie below the steps 17 .. 19 only
        with pytest.raises(ValueError, match="count"):
            spectra.FieldSpectrum(part, sd, REGIONS, freqs, resume_at=at, **kw)
    spectra.FieldSpectrum(part, sd, REGIONS, freqs, resume_at=17, **kw)
    with pytest.raises(ValueError, match="Ts"):
        spectra.FieldSpectrum(part, _sd(Ts=TS * 0.5), REGIONS, freqs, resume_at=19, **kw)
    with pytest.raises(ValueError, match="no spectra file"):
        spectra.FieldSpectrum(tmp_path / "none.h5", sd, REGIONS, freqs, resume_at=19, **kw)


def test_a_chain_inside_a_pass_is_told_how_to_be_created():
    from pffdtd_amd.engine import PfError

    class Busy(FakeEngine):
        def accumulator(self, *a, **k):
            acc = super().accumulator(*a, **k)

            def add(w):
                e = PfError("pffdtd_hip error 4: inside a pair")
                e.code = 4
                raise e
            acc.add = add
            return acc

    fs = spectra.FieldSpectrum("unused.h5", _sd(), REGIONS, [100.0])
    with pytest.raises(PfError, match=r"create the chain with PF_MULTI_NO_PAIRS \| PF_MULTI_NO_TRIPLES") as ei:
        fs.take(Busy(), 0)
    assert ei.value.code == 4
