"""CPU: the host side of the decimated field recordings (pffdtd_amd/recordings.py): the numpy reference `Decim` of a decimating recorder -- the
contract's lines of include/pffdtd_hip.h, which every device comparison of tests/test_hip_decim.py is np.array_equal against -- held to
scipy.signal.upfirdn and to the filter's frequency response; the verified filter design and its refusals; the file, the blocks and the refusals of
a resume, with a recorder object that folds in numpy, no device."""
import types

import numpy as np
import pytest
from scipy.signal import freqz, upfirdn

from pffdtd_amd import recordings

TS = 1.0 / 25000.0
REGIONS = [((0, 0, 3), (4, 5, 4), (1, 1, 1)), ((1, 0, 0), (4, 5, 6), (2, 2, 3))]
PAIRS = [(1, 1), (1, 3), (7, 3), (5, 4), (128, 1), (33, 16), (4096, 64)]  # (ntap, D) of the device tests


class Decim:
    """the reference: a numpy loop over time, vectorised over cells, written with the contract's lines"""

    def __init__(self, pre, taps, D, cells):
        self.pre = np.asarray([] if pre is None else pre, dtype=np.float64).reshape(-1, 6)
        self.h, self.D = np.asarray(taps, dtype=np.float64).reshape(-1), int(D)
        self.ntap = self.h.size
        self.P = -(-self.ntap // self.D)
        self.acc = np.zeros((self.P,) + tuple(cells))
        self.state = np.zeros((len(self.pre), 2) + tuple(cells))
        self.count, self.frames = 0, []  # frames[m]

    def _section(self, k, q, x):
        s = self.state[q]
        y = k[0] * x + s[0]
        s[0] = (k[1] * x - k[4] * y) + s[1]
        s[1] = k[2] * x - k[5] * y
        return y

    def add(self, u):
        x = np.asarray(u).astype(np.float64)
        for q, k in enumerate(self.pre):
            x = self._section(k, q, x)
        n, D, P = self.count, self.D, self.P
        q = -(-n // D)
        for p in range(P):
            m = q + ((p - q) % P)
            k = m * D - n  # the output slot p carries, and the tap this sample meets in it
            if k < self.ntap:
                self.acc[p] = self.acc[p] + self.h[k] * x
                if k == 0:
                    assert m == len(self.frames)
                    self.frames.append(self.acc[p].copy())
                    self.acc[p] = 0.0
        self.count += 1


def test_decim_is_upfirdn():
    """the same sum in another order: |difference| <= ntap * 2^-52 * sum|h| * max|x|"""
    rng = np.random.default_rng(5)
    for ntap, D in PAIRS:
        n = max(3 * ntap // 2, 40) if ntap < 4096 else 4500
        h, x = rng.uniform(-1, 1, ntap), rng.standard_normal((n, 2, 1, 3))
        d = Decim(None, h, D, (2, 1, 3))
        for v in x:
            d.add(v)
        nf = -(-n // D)
        assert len(d.frames) == nf and d.count == n and d.P * D >= ntap
        want = upfirdn(h, x, down=D, axis=0)[:nf]
        err = np.abs(np.array(d.frames) - want).max()
        bound = ntap * 2.0 ** -52 * np.abs(h).sum() * np.abs(x).max()
        print(f"ntap {ntap} D {D}: {nf} frames, max difference {err:.3e}, bound {bound:.3e}")
        assert err <= bound and np.abs(want).max() > 0
    d = Decim(None, [0.5], 1, (1, 1, 1))  # (1, 1): the frames are the samples times the tap
    for v in (3.0, -0.0, 1e-310):
        d.add(np.full((1, 1, 1), v))
    assert [f[0, 0, 0] for f in d.frames] == [1.5, 0.0, 0.5e-310]


@pytest.mark.parametrize("factor,fpass,atten", [(8, 1400.0, 80.0), (6, 1400.0, 100.0)])
def test_the_design_is_verified(factor, fpass, atten):
    h, info = recordings.decimation_filter(TS, factor, fpass, atten)
    f, H = freqz(h, worN=1 << 14, fs=1.0 / TS)  # the design's own grid
    nyq_new = 1.0 / (2 * factor * TS)
    stop_db = 20 * np.log10(np.abs(H[f >= nyq_new]).max())
    print(f"D {factor}, {atten} dB: {h.size} taps, P {info['slots']}, stopband {stop_db:.3f} dB, ripple {info['ripple_db']:.2e} dB")
    assert stop_db <= -atten and info["stop_db"] == stop_db
    assert h.size % 2 == 1 and np.array_equal(h, h[::-1]) and info["delay"] == (h.size - 1) / 2  # linear phase
    assert info["slots"] == -(-h.size // factor) <= 128
    assert info["ripple_db"] == np.abs(20 * np.log10(np.abs(H[f <= fpass]))).max() < 0.01
    if (factor, atten) == (8, 80.0):
        assert h.size == 779 and info["slots"] == 98


def test_the_design_refuses_by_name():
    for kw, word in ((dict(factor=1), "factor"), (dict(fpass_hz=1562.5), "fpass_hz"), (dict(fpass_hz=0.0), "fpass_hz"), (dict(atten_db=0.0), "atten_db")):
        with pytest.raises(ValueError, match=f"decimation_filter: {word}: "):
            recordings.decimation_filter(**{**dict(Ts=TS, factor=8, fpass_hz=1400.0, atten_db=80.0), **kw})
    with pytest.raises(ValueError, match="P: .* smaller factor"):
        recordings.decimation_filter(TS, 8, 1540.0, 80.0)  # a transition band of 22.5 Hz: thousands of taps


def test_sinusoids_come_out_at_the_response():
    """an FIR has no transient beyond its length: after ntap samples a sinusoid's frames are |H(f)| times a sinusoid.  To 1e-12 relative to the
    INPUT's amplitude 1: the rounding of the sum is bounded by ntap * 2^-53 * sum|h| * max|x| (about 1e-13 here) and does not shrink with |H|"""
    h, _ = recordings.decimation_filter(TS, 8, 1400.0, 80.0)
    for f0 in (700.0, 1300.0, 2500.0, 9000.0):  # two in the passband, two in the stopband
        n = np.arange(h.size + 8 * 40)
        d = Decim(None, h, 8, (2,))
        for v in np.stack([np.cos(2 * np.pi * f0 * TS * n), np.sin(2 * np.pi * f0 * TS * n)], axis=1):
            d.add(v)
        y = np.array(d.frames)[-(-h.size // 8):]  # the frames whose taps all met samples
        amp = np.hypot(y[:, 0], y[:, 1])  # (cos, sin through the same filter: the quadrature pair's modulus is the amplitude)
        H = np.abs(freqz(h, worN=[f0], fs=1.0 / TS)[1][0])
        print(f"{f0:g} Hz: |H| {H:.6e}, amplitude {amp.min():.6e} .. {amp.max():.6e}")
        assert y.shape[0] >= 30 and np.abs(amp - H).max() <= 1e-12
        assert (H > 0.999) == (f0 <= 1400.0) and (H < 1e-4) == (f0 > 1562.5)


# ---- the file: a recorder object that folds in numpy, no device -----------------------------------------------------------------------------------
def _sd(Nt=144, Ts=TS, infac=0.37, diff=True):
    return types.SimpleNamespace(Nt=Nt, Ts=Ts, infac=infac, Nx=4, Ny=5, Nz=6, diff=diff)


class FakeRecorder:
    """engine.DecimatingRecorder in numpy"""

    def __init__(self, lo, hi, st, pre, taps, factor, cap, field):
        self.cells = tuple(-(-(hi[a] - lo[a]) // st[a]) for a in range(3))
        self.sl = tuple(slice(lo[a], hi[a], st[a]) for a in range(3))
        self.d, self.cap, self.rd, self.field = Decim(pre, taps, factor, self.cells), cap, 0, field

    count = property(lambda self: self.d.count)
    pending = property(lambda self: len(self.d.frames) - self.rd)

    def add(self):
        assert not (self.d.count % self.d.D == 0 and self.pending == self.cap), "the device would refuse: cap frames wait"
        self.d.add(self.field()[self.sl])

    def read(self, max_frames=None):
        n = self.pending if max_frames is None else min(max_frames, self.pending)
        first, out = self.rd, np.array(self.d.frames[self.rd:self.rd + n]).reshape((n,) + self.cells)
        self.rd += n
        return first, out

    def get_state(self):
        return self.d.acc.copy(), self.d.state.copy()

    def set_state(self, acc, state, count):
        self.d.acc = np.zeros_like(self.d.acc) if acc is None else np.array(acc, dtype=np.float64).reshape(self.d.acc.shape)
        self.d.state = np.zeros_like(self.d.state) if state is None else np.array(state, dtype=np.float64).reshape(self.d.state.shape)
        self.d.count = count
        self.d.frames = [None] * -(-count // self.d.D)
        self.rd = len(self.d.frames)

    def close(self):
        pass


class FakeEngine:
    """u^n = a seeded random field per step"""

    def __init__(self):
        self.n = 0

    def field(self):
        return np.random.default_rng(1000 + self.n).standard_normal((4, 5, 6)).astype(np.float32)

    def decimating_recorder(self, lo, hi, stride=(1, 1, 1), pre_sos=None, taps=None, factor=1, cap=0, depth=0):
        return FakeRecorder(lo, hi, stride, pre_sos, taps, factor, cap, self.field)


def _run(fr, eng, n0, n1):
    for n in range(n0, n1):
        eng.n = n
        if fr.due(n):
            fr.take(eng, n)


KW = dict(factor=4, fpass_hz=2000.0, atten_db=40.0, first=3, cap=5)


def test_file_and_resume(tmp_path):
    sd = _sd()
    whole = recordings.FieldRecording(tmp_path / "whole.h5", sd, REGIONS, **KW)
    assert whole.taps.size % 2 == 1 and whole.pre_sos.shape == (2, 6)
    eng = FakeEngine()
    _run(whole, eng, 0, sd.Nt)
    whole.write()
    w = recordings.read_file(tmp_path / "whole.h5", raw=True)
    nf = -(-(sd.Nt - 3) // 4)
    assert list(w["sampling"]) == [3, 4, sd.Nt - 3, nf] and np.array_equal(w["regions"], whole.table) and w["Ts"] == TS
    assert np.array_equal(w["taps"], whole.taps) and np.array_equal(w["pre_sos"], whole.pre_sos)
    assert list(w["design"]) == [2000.0, 40.0, whole.info["stop_db"], whole.info["ripple_db"], (whole.taps.size - 1) / 2]
    assert list(w["blocks"]) == list(range(0, nf, 5)) and nf % 5 != 0  # (the last block is not full)
    for i in range(2):
        frames, fs_out, t0 = recordings.read(tmp_path / "whole.h5", i)
        d = Decim(whole.pre_sos, whole.taps, 4, whole.recs[i].cells)
        for n in range(3, sd.Nt):
            eng.n = n
            d.add(eng.field()[whole.recs[i].sl])
        assert frames.dtype == np.float32 and frames.shape == (nf,) + whole.recs[i].cells
        assert np.array_equal(frames, (np.array(d.frames) * 0.37).astype(np.float32)) and np.abs(frames).max() > 0
        assert fs_out == 1.0 / (4 * TS) and t0 == (3 - (whole.taps.size - 1) / 2) * TS
        assert np.array_equal(w["acc"][i], d.acc) and np.array_equal(w["state"][i], d.state)
    # a run stopped at step 54 (inside a block, inside an output) and resumed
    path = tmp_path / "rec.h5"
    a = recordings.FieldRecording(path, sd, REGIONS, **KW)
    _run(a, FakeEngine(), 0, 54)
    a.write()
    assert not (tmp_path / "rec.h5.tmp").exists() and list(recordings.read_file(path)["sampling"]) == [3, 4, 51, 13]
    assert list(recordings.read_file(path)["blocks"]) == [0, 5, 10]
    stopped = path.read_bytes()
    b = recordings.FieldRecording(path, sd, REGIONS, resume_at=54, **KW)
    assert b.count == 51
    eng = FakeEngine()
    b.attach(eng)
    _run(b, eng, 54, sd.Nt)
    b.write()
    r = recordings.read_file(path, raw=True)
    for key in ("sampling", "blocks", "taps", "pre_sos", "design"):
        assert np.array_equal(r[key], w[key]), key
    for i in range(2):
        assert recordings.read(path, i)[0].tobytes() == recordings.read(tmp_path / "whole.h5", i)[0].tobytes()
        assert np.array_equal(r["acc"][i], w["acc"][i]) and np.array_equal(r["state"][i], w["state"][i])
    # float64 frames on request
    c = recordings.FieldRecording(tmp_path / "f8.h5", sd, REGIONS[:1], dtype="f8", **KW)
    _run(c, FakeEngine(), 0, 30)
    c.write()
    f8 = recordings.read(tmp_path / "f8.h5", 0)[0]
    assert f8.dtype == np.float64 and f8.shape[0] == 7 and np.array_equal(f8.astype(np.float32), recordings.read(tmp_path / "whole.h5", 0)[0][:7])
    # every refusal names its field
    path.write_bytes(stopped)  # (the file of step 54 again)
    other = [REGIONS[0], ((0, 0, 0), (4, 5, 6), (2, 2, 3))]
    for field, args, k2 in (("regions", (sd, other), KW), ("taps", (sd, REGIONS), {**KW, "fpass_hz": 1500.0}), ("taps", (sd, REGIONS), {**KW, "atten_db": 50.0}),
                            ("pre_sos", (sd, REGIONS), {**KW, "lowcut_hz": 20.0}), ("Ts", (_sd(Ts=TS * 1.01), REGIONS), KW), ("first", (sd, REGIONS), {**KW, "first": 2}),
                            ("factor", (sd, REGIONS), {**KW, "factor": 5}), ("blocks", (sd, REGIONS), {**KW, "cap": 4})):
        with pytest.raises(ValueError, match=f": {field}: "):
            recordings.FieldRecording(path, *args, resume_at=54, **k2)
    with pytest.raises(ValueError, match=": count: "):
        recordings.FieldRecording(path, sd, REGIONS, resume_at=55, **KW)
    with pytest.raises(ValueError, match="no recording file"):
        recordings.FieldRecording(tmp_path / "missing.h5", sd, REGIONS, resume_at=54, **KW)
    with pytest.raises(ValueError, match="dtype"):
        recordings.FieldRecording(path, sd, REGIONS, **{**KW, "dtype": "f2"})
    with pytest.raises(ValueError, match="no sample is due"):
        recordings.FieldRecording(tmp_path / "unused.h5", sd, REGIONS, **KW).take(FakeEngine(), 2)


def test_arguments_are_refused_both_ways_round():
    import argparse

    def parse(*argv):
        p = argparse.ArgumentParser()
        recordings.add_arguments(p)
        a = p.parse_args(list(argv))
        recordings.check_arguments(p, a)
        return a

    assert not parse().rec
    a = parse("--rec-planes", "x=3", "--rec-factor", "8", "--rec-fpass", "1400")
    assert a.rec and (a.rec_atten, a.rec_first, a.rec_dtype, a.rec_file) == (80.0, 0, "f4", "")
    for argv in (("--rec-planes", "x=3"), ("--rec-planes", "x=3", "--rec-factor", "8"), ("--rec-factor", "8", "--rec-fpass", "1400"), ("--rec-first", "4"),
                 ("--rec-dtype", "f8"), ("--rec-file", "a.h5"), ("--rec-box", "0:4:1,0:4:1,0:4:1", "--rec-factor", "8", "--rec-fpass", "1400", "--rec-first", "-1")):
        with pytest.raises(SystemExit):
            parse(*argv)
