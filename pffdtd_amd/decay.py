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
(n - first) // bin_steps with bin_steps = round(bin_ms * 1e-3 / Ts).  FieldDecay is a field_output.FieldOutput: a sample is never shifted, a chain
that is sampled is created with PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES, and take, write and the rules of a resume are described there.

The file holds
    regions  int64 [R, 9]      bands  float64 [B]      Ts  float64      sampling  int64 [3] = first, bin_steps, count (samples so far)
    pre_sos  float64 [npre, 6]      band_sos  float64 [B, nsec, 6]      (scipy's rows)
    r{i:03d}_E      float64 [B, nbin, c0, c1, c2] of region i: sums * infac^2 (the square of the factor SimData.rescale_output applies to u_out)
    r{i:03d}_sums   the raw sums, and  r{i:03d}_state  float64 [npre + B * nsec, 2, c0, c1, c2]  the filters' state: what a resumed run continues from
With resume_at (the step a resumed run continues at) the file must match in regions, bands, pre_sos, band_sos, Ts, first and bin_steps, and its
count must be the number of sample steps below resume_at; otherwise it is refused with the field's name.
The command line's --decay-bands is parsed here: host code, no device.
"""
import numpy as np
from scipy.signal import bilinear_zpk, butter, zpk2sos

from . import h5io
from .field_output import FieldOutput


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


class BandOutput(FieldOutput):
    """what the decay maps and the directional maps share: octave bands, time bins, a sum and a filter state per region.  A kind sets `sections`
    and `holder` (the words of the pre_sos refusal, the observer's name) and writes its scaled sums (`_write_scaled`)."""
    holds, observers_noun = "sums", "accumulators"
    accs = property(lambda self: self.observers)

    def _bands_and_bins(self, bands_hz, bin_ms, order):
        """bands, bin_steps, nbin and their refusals"""
        who = type(self).__name__
        self.bands = np.ascontiguousarray(bands_hz, dtype=np.float64).reshape(-1)
        self.bin_steps = int(round(float(bin_ms) * 1e-3 / self.Ts))
        if self.first < 0 or not self.regions or self.bands.size == 0 or int(order) < 1:
            raise ValueError(f"{who}: at least one region and one band, first >= 0, order >= 1")
        if self.bands.size > 16 or int(order) > 8:
            raise ValueError(f"{who}: bands: {self.bands.size} bands of order {order}, a {self.holder} holds 16 of 8 sections")
        if self.bin_steps < 1:
            raise ValueError(f"{who}: bin_ms: {bin_ms} ms is less than half a step of {self.Ts * 1e3:g} ms")
        self.nbin = max(1, -(-(self.sd.Nt - self.first) // self.bin_steps))

    def bin_of(self, n):
        return (n - self.first) // self.bin_steps

    def _sample(self, n):
        return (self.bin_of(n),)

    def _restore_observer(self, a, i, count, sums, state):
        a.set(sums[i], state[i], count)

    def _write_region(self, path, i, a):
        e, s = a.get()
        h5io.write(path, f"r{i:03d}_sums", e)
        h5io.write(path, f"r{i:03d}_state", s)
        self._write_scaled(path, i, e * (self.sd.infac * self.sd.infac))

    def _band_checks(self, f):
        """the rows of `_checks` from Ts on"""
        return [*self._same_clock(f), self._asked("bin_steps", f["sampling"][1], self.bin_steps),
                ("pre_sos", np.array_equal(f["pre_sos"], self.pre_sos), f"the file's sums went through other {self.sections}"),
                ("band_sos", np.array_equal(f["band_sos"], self.band_sos), "the file's sums went through other band filters (order)")]

    def _saved(self, f, count):
        return count, f["sums"], f["state"]


class FieldDecay(BandOutput):
    label, noun, holder, sections = "field decay", "decay", "band accumulator", "shared sections (low-cut, integrator)"

    def __init__(self, path, sd, regions, bands_hz, bin_ms, first=0, order=3, lowcut_hz=10.0, lowcut_order=4, resume_at=None):
        super().__init__(path, sd, regions, first)
        self._bands_and_bins(bands_hz, bin_ms, order)
        self.pre_sos = pre_sections(self.Ts, bool(getattr(sd, "diff", False)), float(lowcut_hz), int(lowcut_order))
        self.band_sos = band_sections(self.Ts, self.bands, int(order))
        self._resume(resume_at)

    def _observer(self, obj, lo, hi, st):
        return obj.band_accumulator(lo, hi, st, pre_sos=self.pre_sos, band_sos=self.band_sos, nbin=self.nbin)

    def _write_head(self, path, append):
        h5io.write(path, "regions", self.table, append=append)
        h5io.write(path, "bands", self.bands)
        h5io.write(path, "Ts", np.float64(self.Ts))
        h5io.write(path, "sampling", np.array([self.first, self.bin_steps, self.count], dtype=np.int64))
        h5io.write(path, "pre_sos", self.pre_sos if self.pre_sos.size else np.zeros((1, 6)))  # (no shared section: one row of zeros)
        h5io.write(path, "npre", np.int64(self.pre_sos.shape[0]))
        h5io.write(path, "band_sos", self.band_sos)

    def _write_scaled(self, path, i, E):
        h5io.write(path, f"r{i:03d}_E", E)

    def _read_file(self):
        return read(self.path, raw=True)

    def _checks(self, f):
        return [self._other(f, "bands"), *self._band_checks(f)]


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


def add_arguments(p):
    """the --decay-* arguments of the command line"""
    p.add_argument("--decay-planes", action="append", default=[], metavar="x=I,y=J,z=K", help="sum the band-filtered, squared field of these planes into time bins on the device (the syntax of --field-planes)")
    p.add_argument("--decay-box", action="append", default=[], metavar="x0:x1:sx,y0:y1:sy,z0:z1:sz", help="... of this strided box")
    p.add_argument("--decay-bands", default="", metavar="F1,F2,...", help="... in the octave bands around these centre frequencies in Hz")
    p.add_argument("--decay-bin-ms", type=float, default=5.0, metavar="MS", help="... in time bins of MS milliseconds (default 5)")
    p.add_argument("--decay-first", type=int, default=0, metavar="N", help="... at every step from N on (default 0)")
    p.add_argument("--decay-file", default="", metavar="FILE", help="... into this HDF5 file (default: sim_decay.h5 in the data folder)")


def check_arguments(p, a):
    """a.decay: are decay maps asked for?  Regions without --decay-bands, and any --decay-* without a region, are refused"""
    a.decay = bool(a.decay_planes or a.decay_box)
    if a.decay != bool(a.decay_bands) or a.decay_bin_ms <= 0 or a.decay_first < 0:
        p.error("--decay-planes / --decay-box need --decay-bands (and the other way round); --decay-bin-ms: positive, --decay-first: not negative")
    if (a.decay_first or a.decay_file or a.decay_bin_ms != 5.0) and not a.decay:
        p.error("--decay-bin-ms / --decay-first / --decay-file need --decay-planes or --decay-box")
