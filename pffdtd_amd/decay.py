"""Octave-band energy decay maps: per band, the filtered and squared pressure of every cell of a plane or a box, summed into time bins on the
device as the run goes, in one HDF5 file -- what EDT, T20 / T30, C50 / C80, D50 and strength of every seat are functions of.

    fd = FieldDecay(path, sd, regions, bands_hz, bin_ms, first=0, order=3, lowcut_hz=10, lowcut_order=4)     regions: [(lo, hi, stride)], FILE x, y, z
    fd.take(obj, n)                              obj: a HipEngine or HipMulti that has taken the steps 0 .. n-1; n >= first: every such step is a sample
    fd.write()
    decay.parameters(E, bin_seconds)             host numpy: EDC, EDT, T20, T30, C50, C80, D50 per band and cell

A sum of raw u^2 would mean nothing: the grid carries the DIFFERENTIATED response (comms_out's diff), so the samples first run through what
ProcessOutputs.initial_process (process_outputs.py) applies to the receivers -- the integrator + low-cut, by the same scipy calls; the plain
high-pass where diff is not set; nothing for lowcut_hz = 0 without diff -- as the shared sections `pre_sos` of one band accumulator per region
(engine.BandAccumulator, pf_engine_bandacc_*).  The bands are butter(order, [fc / sqrt 2, fc * sqrt 2], 'band') at Fs = 1 / Ts: their power is
exactly one half at both edges (the prewarped bilinear map); a band whose upper edge reaches 1 / (2 Ts) is refused by name.

Every step from `first` on is a sample -- there is no `every`: a recursive filter over skipped samples is another filter.  The bin of step n is
(n - first) // bin_steps with bin_steps = round(bin_ms * 1e-3 / Ts).  A chain answers only while no slab is inside a pair or triple, and a
sample is never shifted: a chain that is sampled is created with PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES.

The file (write(): written to a temporary name and moved into place with os.replace) holds
    regions  int64 [R, 9]      bands  float64 [B]      Ts  float64      sampling  int64 [3] = first, bin_steps, count (samples so far)
    pre_sos  float64 [npre, 6]      band_sos  float64 [B, nsec, 6]      (scipy's rows)
    r{i:03d}_E      float64 [B, nbin, c0, c1, c2] of region i: sums * infac^2 (the square of the factor SimData.rescale_output applies to u_out)
    r{i:03d}_sums   the raw sums, and  r{i:03d}_state  float64 [npre + B * nsec, 2, c0, c1, c2]  the filters' state: what a resumed run continues from
With resume_at (the step a resumed run continues at) the file must match in regions, bands, pre_sos, band_sos, Ts, first and bin_steps, and its
count must be the number of sample steps below resume_at; otherwise it is refused with the field's name.
The command line's --decay-bands is parsed here: host code, no device.
"""
import os

import numpy as np
from scipy.signal import bilinear_zpk, butter, zpk2sos

from . import h5io
from .engine import PfError


def parse_bands(spec):
    """'125,250,500' -> those centre frequencies in Hz"""
    try:
        f = np.array([float(s) for s in spec.split(",") if s.strip()], dtype=np.float64)
    except ValueError:
        raise ValueError(f"--decay-bands: '{spec}' is not f1,f2,...")
    if f.size == 0 or not np.all(np.isfinite(f)) or np.any(f <= 0):
        raise ValueError(f"--decay-bands: '{spec}' names no band, or one that is not positive")
    return f


def pre_sections(Ts, diff, lowcut_hz, lowcut_order):
    """the sections of ProcessOutputs.initial_process(fcut=lowcut_hz, N_order=lowcut_order): float64 [npre, 6]"""
    if lowcut_hz > 0:
        if diff:
            z, p, k = butter(lowcut_order, lowcut_hz * 2 * np.pi, btype="high", analog=True, output="zpk")
            zd, pd, kd = bilinear_zpk(z[1:], p, k, 1 / Ts)  # one zero removed = integrator
            return np.ascontiguousarray(zpk2sos(zd, pd, kd), dtype=np.float64)
        return np.ascontiguousarray(butter(lowcut_order, 2 * Ts * lowcut_hz, btype="high", output="sos"), dtype=np.float64)
    if diff:
        raise ValueError("FieldDecay: lowcut_hz: the scene's input is differentiated (diff): its integrator needs the low-cut, lowcut_hz > 0")
    return np.zeros((0, 6))


def band_sections(Ts, bands_hz, order):
    """butter(order, [fc / sqrt 2, fc * sqrt 2], 'band') at Fs = 1 / Ts: float64 [B, order, 6]"""
    nyq = 1.0 / (2.0 * Ts)
    out = []
    for fc in bands_hz:
        lo, hi = fc / np.sqrt(2.0), fc * np.sqrt(2.0)
        if hi >= nyq:
            raise ValueError(f"FieldDecay: bands: the {fc:g} Hz band's upper edge {hi:g} Hz reaches 1 / (2 Ts) = {nyq:g} Hz")
        out.append(butter(order, [lo / nyq, hi / nyq], btype="band", output="sos"))
    return np.ascontiguousarray(np.stack(out), dtype=np.float64)


class FieldDecay:
    def __init__(self, path, sd, regions, bands_hz, bin_ms, first=0, order=3, lowcut_hz=10.0, lowcut_order=4, resume_at=None):
        self.path, self.sd = os.fspath(path), sd
        self.regions = [tuple(tuple(int(v) for v in t) for t in r) for r in regions]
        self.bands = np.ascontiguousarray(bands_hz, dtype=np.float64).reshape(-1)
        self.first, self.Ts = int(first), float(sd.Ts)
        self.bin_steps = int(round(float(bin_ms) * 1e-3 / self.Ts))
        if self.first < 0 or not self.regions or self.bands.size == 0 or int(order) < 1:
            raise ValueError("FieldDecay: at least one region and one band, first >= 0, order >= 1")
        if self.bands.size > 16 or int(order) > 8:
            raise ValueError(f"FieldDecay: bands: {self.bands.size} bands of order {order}, a band accumulator holds 16 of 8 sections")
        if self.bin_steps < 1:
            raise ValueError(f"FieldDecay: bin_ms: {bin_ms} ms is less than half a step of {self.Ts * 1e3:g} ms")
        self.pre_sos = pre_sections(self.Ts, bool(getattr(sd, "diff", False)), float(lowcut_hz), int(lowcut_order))
        self.band_sos = band_sections(self.Ts, self.bands, int(order))
        self.nbin = max(1, -(-(sd.Nt - self.first) // self.bin_steps))
        self.table = np.array([lo + hi + st for lo, hi, st in self.regions], dtype=np.int64).reshape(-1, 9)
        self.accs, self._restore = None, None
        if resume_at is not None:
            self._restore = self._read_matching(int(resume_at))

    # ---- the sample steps ----
    def next_step(self, n):
        """the first step >= n at which a sample is due (it may lie at or past Nt: no sample then)"""
        return max(n, self.first)

    def due(self, n):
        return self.first <= n < self.sd.Nt

    def samples_below(self, n):
        """how many sample steps lie below step n"""
        return max(0, n - self.first)

    def bin_of(self, n):
        return (n - self.first) // self.bin_steps

    # ---- the sums ----
    def attach(self, obj):
        """one band accumulator per region on obj (a HipEngine or a HipMulti); a resumed run's sums and filter state go into them"""
        if self.accs is not None:
            return
        self.accs = [obj.band_accumulator(lo, hi, st, pre_sos=self.pre_sos, band_sos=self.band_sos, nbin=self.nbin) for lo, hi, st in self.regions]
        if self._restore is not None:
            count, sums, state = self._restore
            for a, e, s in zip(self.accs, sums, state):
                a.set(e, s, count)
            self._restore = None

    @property
    def count(self):
        if self.accs is None:
            return self._restore[0] if self._restore is not None else 0
        return self.accs[0].count

    def take(self, obj, n):
        """the sample of step n (due(n)) -- never of another step"""
        if not self.due(n):
            raise ValueError(f"FieldDecay.take: no sample is due at step {n} (first {self.first}, Nt {self.sd.Nt})")
        self.attach(obj)
        try:
            for a in self.accs:
                a.add(self.bin_of(n))
        except PfError as e:
            if e.code != 4:  # (PF_ERR_STATE: a slab inside a pair or triple; no slab took the sample)
                raise
            err = PfError(f"field decay: step {n} cannot be sampled, a slab is inside a blocked pass there, and a sample is never shifted: "
                          f"create the chain with PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES ({e})")
            err.code = 4
            raise err
        return n

    def write(self):
        """the file as it stands: every region's sums and filter state so far"""
        if self.accs is None:
            raise ValueError("FieldDecay.write: no accumulators yet (attach or take first)")
        tmp = self.path + ".tmp"
        h5io.write(tmp, "regions", self.table, append=False)
        h5io.write(tmp, "bands", self.bands)
        h5io.write(tmp, "Ts", np.float64(self.Ts))
        h5io.write(tmp, "sampling", np.array([self.first, self.bin_steps, self.count], dtype=np.int64))
        h5io.write(tmp, "pre_sos", self.pre_sos if self.pre_sos.size else np.zeros((1, 6)))  # (no shared section: one row of zeros)
        h5io.write(tmp, "npre", np.int64(self.pre_sos.shape[0]))
        h5io.write(tmp, "band_sos", self.band_sos)
        for i, a in enumerate(self.accs):
            e, s = a.get()
            h5io.write(tmp, f"r{i:03d}_sums", e)
            h5io.write(tmp, f"r{i:03d}_state", s)
            h5io.write(tmp, f"r{i:03d}_E", e * (self.sd.infac * self.sd.infac))
        os.replace(tmp, self.path)

    def close(self):
        for a in self.accs or []:
            a.close()
        self.accs = None

    def _read_matching(self, resume_at):
        """(count, [raw sums per region], [filter state per region]) of the file a resumed run continues, or ValueError naming the field that differs"""
        if not os.path.exists(self.path):
            raise ValueError(f"{self.path}: no decay file to resume from")
        f = read(self.path, raw=True)
        if not np.array_equal(f["regions"], self.table):
            raise ValueError(f"{self.path}: regions: the file holds the sums of other regions")
        if not np.array_equal(f["bands"], self.bands):
            raise ValueError(f"{self.path}: bands: the file holds the sums of other bands")
        if f["Ts"] != self.Ts:
            raise ValueError(f"{self.path}: Ts: {f['Ts']!r} in the file, {self.Ts!r} in the scene")
        first, bin_steps, count = (int(v) for v in f["sampling"])
        if first != self.first:
            raise ValueError(f"{self.path}: first: {first} in the file, {self.first} asked for")
        if bin_steps != self.bin_steps:
            raise ValueError(f"{self.path}: bin_steps: {bin_steps} in the file, {self.bin_steps} asked for")
        if not np.array_equal(f["pre_sos"], self.pre_sos):
            raise ValueError(f"{self.path}: pre_sos: the file's sums went through other shared sections (low-cut, integrator)")
        if not np.array_equal(f["band_sos"], self.band_sos):
            raise ValueError(f"{self.path}: band_sos: the file's sums went through other band filters (order)")
        if count != self.samples_below(resume_at):
            raise ValueError(f"{self.path}: count: the file holds {count} samples, {self.samples_below(resume_at)} sample steps lie below step {resume_at}")
        return count, f["sums"], f["state"]


def read(path, raw=False):
    """-> dict(regions [R, 9], bands [B], Ts, sampling [first, bin_steps, count], pre_sos [npre, 6], band_sos [B, nsec, 6], E: per region float64
    [B, nbin, c0, c1, c2]; raw: also sums and state, unscaled) of a file FieldDecay wrote"""
    regions = np.asarray(h5io.read(path, "regions", h5io.I64)).reshape(-1, 9)
    npre = int(h5io.read(path, "npre", h5io.I64))
    out = {"regions": regions, "bands": np.asarray(h5io.read(path, "bands", h5io.F64)).reshape(-1), "Ts": float(h5io.read(path, "Ts", h5io.F64)),
           "sampling": np.asarray(h5io.read(path, "sampling", h5io.I64)).reshape(3),
           "pre_sos": np.asarray(h5io.read(path, "pre_sos", h5io.F64)).reshape(-1, 6)[:npre], "band_sos": np.asarray(h5io.read(path, "band_sos", h5io.F64))}
    for key in ("E",) + (("sums", "state") if raw else ()):
        out[key] = [np.asarray(h5io.read(path, f"r{i:03d}_{key}", h5io.F64)) for i in range(len(regions))]
    return out


def _decay_time(edc_db, t, hi, lo):
    """least squares on the EDC in dB between `hi` and `lo` dB -> the time of 60 dB at that slope, per column (nan where fewer than 2 points)"""
    nb = edc_db.shape[0]
    flat = edc_db.reshape(nb, -1)
    out = np.full(flat.shape[1], np.nan)
    for j in range(flat.shape[1]):
        y = flat[:, j]
        if not np.isfinite(y[0]):
            continue
        sel = (y <= hi) & (y >= lo) & np.isfinite(y)
        below = np.nonzero(y < lo)[0]  # (the EDC falls monotonically; stop at the first crossing)
        if below.size:
            sel[below[0]:] = False
        if np.count_nonzero(sel) < 2:
            continue
        slope = np.polyfit(t[sel], y[sel], 1)[0]
        if slope < 0:
            out[j] = -60.0 / slope
    return out.reshape(edc_db.shape[1:])


def parameters(E, bin_seconds):
    """E: float64 [..., nbin, c0, c1, c2] -- a region's r*_E, or one band of it --, bin_seconds = bin_steps * Ts.  -> dict of
        edc   [..., nbin, cells]   Schroeder's backward integration: edc[k] = sum of E[k:]
        EDT, T20, T30  [..., cells]   seconds: least squares on 10 log10(edc / edc[0]) at the bins' start times over 0 .. -10, -5 .. -25, -5 .. -35 dB,
                       extrapolated to 60 dB (nan where the range holds fewer than two bins, or the cell is silent)
        C50, C80  dB,  D50  a fraction: early against late (all) energy, split 50 / 80 ms after the onset
    The onset of a cell is its first bin within 20 dB of its largest bin; the split lies a whole number of bins after it, round(0.05 / bin_seconds)
    or round(0.08 / bin_seconds): the time resolution of C50, C80 and D50 is ONE BIN (5 ms bins place the 50 ms split exactly, the onset within 5 ms)."""
    E = np.asarray(E, dtype=np.float64)
    lead = E.shape[:-4]
    nbin = E.shape[-4]
    cells = E.shape[-3:]
    e = np.moveaxis(E.reshape((-1, nbin) + cells), 1, 0).reshape(nbin, -1)  # [nbin, columns]
    edc = np.cumsum(e[::-1], axis=0)[::-1]
    t = np.arange(nbin) * float(bin_seconds)
    with np.errstate(divide="ignore", invalid="ignore"):
        db = 10.0 * np.log10(edc / edc[0])
    out = {"edc": np.moveaxis(edc.reshape((nbin,) + lead + cells), 0, len(lead))}
    for name, hi, lo in (("EDT", 0.0, -10.0), ("T20", -5.0, -25.0), ("T30", -5.0, -35.0)):
        out[name] = _decay_time(db, t, hi, lo).reshape(lead + cells)
    peak = e.max(axis=0)
    onset = np.argmax(e >= peak * 1e-2, axis=0)  # the first bin within 20 dB of the largest
    csum = np.concatenate([np.zeros((1, e.shape[1])), np.cumsum(e, axis=0)])  # csum[k] = sum of e[:k]
    total = csum[-1]
    cols = np.arange(e.shape[1])
    for name, ms in (("50", 0.05), ("80", 0.08)):
        split = np.minimum(onset + int(round(ms / float(bin_seconds))), nbin)
        early = csum[split, cols] - csum[onset, cols]
        late = total - csum[split, cols]
        with np.errstate(divide="ignore", invalid="ignore"):
            out["C" + name] = (10.0 * np.log10(early / late)).reshape(lead + cells)
            if name == "50":
                out["D50"] = (early / (early + late)).reshape(lead + cells)
    return out
