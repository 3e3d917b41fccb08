"""Field spectra: the DFT of every cell of a plane or a box at chosen frequencies, summed on the device as the run goes, in one HDF5 file.

    fs = FieldSpectrum(path, sd, regions, freqs, every=1, first=0, window=None)     regions: [(lo, hi, stride)] in FILE coordinates x, y, z
    fs.take(obj, n)                                     obj: a HipEngine or HipMulti that has taken the steps 0 .. n-1; n: a sample step
    fs.write()

Field frames (fields.py) go through the host and are taken every K steps; a spectrum needs EVERY sample of every cell.  It is kept where the
field is: one accumulator per region (engine.Accumulator, pf_engine_accum_*: acc[m] += w[m] * double(u^n) on the device) with the channels
2k, 2k + 1 = the real and imaginary part at freqs[k],
    w[2k] = g(n) cos(phi),  w[2k + 1] = -g(n) sin(phi),   phi = 2 pi ((freqs[k] * Ts * n) mod 1.0)  in double,
g = 1, or a Hann window over the sample steps (window="hann": 0 at the first and at the last sample step below Nt).  The sample of step n is
u^n, the field the receivers of step n sample: at a receiver's cell the sums are the same sums over that receiver's row of u_out.

Samples are due at the steps first, first + every, ... below Nt.  every > 1 means samples every `every` steps: the sampling rate is
1 / (every * Ts), and whatever the field holds above 1 / (2 * every * Ts) ALIASES into the sums.  The grid carries energy up to its own
Nyquist frequency 1 / (2 Ts) unless the source is band-limited, so choose `every` for the source's band, not for the frequencies asked for;
frequencies at or above 1 / (2 * every * Ts) are refused.  What every > 1 buys: a single domain that steps in triples keeps them with
every = 3 and runs of three steps between the samples (an accumulator answers between runs, never inside a pass).  A chain answers only
while no slab is inside a pair or triple and `take` NEVER shifts the step -- a DFT over unevenly spaced samples is not the DFT the file
promises --: a chain that is sampled is created with PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES.

FieldSpectrum is a field_output.FieldOutput: the schedule, the accumulators of the regions, take, write and the rules of a resume are described there.
The file holds
    regions   int64 [R, 9]     lo, hi, stride of every region
    freqs     float64 [K]      Ts   float64      sampling  int64 [3] = first, every, count (samples summed so far)      window  int64 (0 none, 1 hann)
    r{i:03d}_re, r{i:03d}_im   float64 [K, c0, c1, c2] of region i: acc * sd.infac, a single multiplication (the factor SimData.rescale_output
                               applies to u_out)
With resume_at (the step a resumed run continues at) the file must hold the sums of the same regions, freqs, first, every and window, and
its count must be the number of sample steps below resume_at; otherwise it is refused with the field's name.  The file keeps the raw sums
beside the scaled ones (r{i:03d}_acc float64 [2K, c0, c1, c2]: a division by infac would not give them back bit for bit); they are set into
the new accumulators and the run goes on to the sums of a run in one piece.
The command line's --spectrum-freqs is parsed here: host code, no device.
"""
import numpy as np

from . import h5io
from .field_output import FieldOutput

WINDOWS = {None: 0, "none": 0, "hann": 1}


def parse_freqs(spec):
    """'63,125,250' -> those; 'lo:hi:n' -> n frequencies from lo to hi, linearly spaced, both included"""
    spec = spec.strip()
    try:
        if ":" in spec:
            lo, hi, n = spec.split(":")
            if int(n) < 1:
                raise ValueError
            f = np.linspace(float(lo), float(hi), int(n))
        else:
            f = np.array([float(s) for s in spec.split(",") if s.strip()], dtype=np.float64)
    except ValueError:
        raise ValueError(f"--spectrum-freqs: '{spec}' is neither f1,f2,... nor lo:hi:n")
    if f.size == 0 or not np.all(np.isfinite(f)) or np.any(f < 0):
        raise ValueError(f"--spectrum-freqs: '{spec}' names no frequency, or a negative one")
    return f


class FieldSpectrum(FieldOutput):
    label, noun, holds, observers_noun = "field spectrum", "spectra", "sums", "accumulators"
    accs = property(lambda self: self.observers)

    def __init__(self, path, sd, regions, freqs, every=1, first=0, window=None, resume_at=None):
        super().__init__(path, sd, regions, first)
        self.freqs = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        self.every = int(every)
        if window not in WINDOWS:
            raise ValueError(f"FieldSpectrum: window = {window!r} is neither None nor 'hann'")
        self.window = WINDOWS[window]
        if self.every < 1 or self.first < 0 or not self.regions or self.freqs.size == 0:
            raise ValueError("FieldSpectrum: at least one region and one frequency, every >= 1, first >= 0")
        if 2 * self.freqs.size > 256:
            raise ValueError(f"FieldSpectrum: freqs: {self.freqs.size} frequencies, an accumulator holds 128 (256 channels)")
        nyq = 1.0 / (2.0 * self.every * self.Ts)
        if np.any(self.freqs < 0) or np.any(self.freqs >= nyq):
            raise ValueError(f"FieldSpectrum: freqs: every frequency must lie in [0, 1 / (2 * every * Ts)) = [0, {nyq:g}) Hz: samples every {self.every} "
                             f"step(s) cannot tell {float(self.freqs.max()):g} Hz from its alias")
        self.nsamples = self.samples_below(sd.Nt)  # of the whole run: the Hann window's length
        self._resume(resume_at)

    def weights(self, n):
        """float64 [2K]: g(n) cos(phi_k), -g(n) sin(phi_k) of step n, phi_k = 2 pi ((freqs[k] * Ts * n) mod 1.0)"""
        g = 1.0
        if self.window == 1 and self.nsamples > 1:
            k = (n - self.first) // self.every
            g = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.mod(k / (self.nsamples - 1), 1.0))
        phi = 2.0 * np.pi * np.mod(self.freqs * self.Ts * n, 1.0)
        w = np.empty(2 * self.freqs.size, dtype=np.float64)
        w[0::2] = g * np.cos(phi)
        w[1::2] = -(g * np.sin(phi))
        return w

    # ---- what FieldOutput asks of a kind ----
    def _observer(self, obj, lo, hi, st):
        return obj.accumulator(lo, hi, st, nchan=2 * self.freqs.size)

    def _restore_observer(self, a, i, count, sums):
        a.set(sums[i], count)

    def _due_rule(self):
        return f"first {self.first}, every {self.every}"

    def _sample(self, n):
        return (self.weights(n),)

    def _write_head(self, path, append):
        h5io.write(path, "regions", self.table, append=append)
        h5io.write(path, "freqs", self.freqs)
        h5io.write(path, "Ts", np.float64(self.Ts))
        h5io.write(path, "sampling", np.array([self.first, self.every, self.count], dtype=np.int64))
        h5io.write(path, "window", np.int64(self.window))

    def _write_region(self, path, i, a):
        acc = a.get()
        h5io.write(path, f"r{i:03d}_acc", acc)
        h5io.write(path, f"r{i:03d}_re", acc[0::2] * self.sd.infac)
        h5io.write(path, f"r{i:03d}_im", acc[1::2] * self.sd.infac)

    def _read_file(self):
        return read(self.path, raw=True)

    def _checks(self, f):
        return [self._other(f, "freqs", "frequencies"), *self._same_clock(f), self._asked("every", f["sampling"][1], self.every),
                self._asked("window", f["window"], self.window, " (0 none, 1 hann)")]

    def _saved(self, f, count):
        return count, f["acc"]


def read(path, raw=False):
    """-> dict(regions [R, 9], freqs [K], Ts, sampling [first, every, count], window, re / im: per region float64 [K, c0, c1, c2];
    raw: also acc, the unscaled sums [2K, c0, c1, c2]) of a file FieldSpectrum wrote"""
    regions = np.asarray(h5io.read(path, "regions", h5io.I64)).reshape(-1, 9)
    out = {"regions": regions, "freqs": np.asarray(h5io.read(path, "freqs", h5io.F64)).reshape(-1), "Ts": float(h5io.read(path, "Ts", h5io.F64)),
           "sampling": np.asarray(h5io.read(path, "sampling", h5io.I64)).reshape(3), "window": int(h5io.read(path, "window", h5io.I64))}
    for key in ("re", "im") + (("acc",) if raw else ()):
        out[key] = [np.asarray(h5io.read(path, f"r{i:03d}_{key}", h5io.F64)) for i in range(len(regions))]
    return out


def add_arguments(p):
    """the --spectrum-* arguments of the command line"""
    p.add_argument("--spectrum-planes", action="append", default=[], metavar="x=I,y=J,z=K", help="sum the DFT of these planes of the field on the device (the syntax of --field-planes)")
    p.add_argument("--spectrum-box", action="append", default=[], metavar="x0:x1:sx,y0:y1:sy,z0:z1:sz", help="... of this strided box")
    p.add_argument("--spectrum-freqs", default="", metavar="F1,F2,... | LO:HI:N", help="... at these frequencies in Hz (LO:HI:N: N of them, linearly spaced)")
    p.add_argument("--spectrum-every", type=int, default=1, metavar="K", help="... sampling every K steps (default 1; content above 1 / (2 K Ts) aliases)")
    p.add_argument("--spectrum-first", type=int, default=0, metavar="N", help="... from step N on (default 0)")
    p.add_argument("--spectrum-window", default=None, choices=["hann"], help="... under a window over the sample steps (default: none)")
    p.add_argument("--spectrum-file", default="", metavar="FILE", help="... into this HDF5 file (default: sim_spectra.h5 in the data folder)")


def check_arguments(p, a):
    """a.spectrum: is a spectrum asked for?  Regions without --spectrum-freqs, and any --spectrum-* without a region, are refused"""
    a.spectrum = bool(a.spectrum_planes or a.spectrum_box)
    if a.spectrum != bool(a.spectrum_freqs) or a.spectrum_every < 1 or a.spectrum_first < 0:
        p.error("--spectrum-planes / --spectrum-box need --spectrum-freqs (and the other way round); --spectrum-every >= 1, --spectrum-first: not negative")
    if (a.spectrum_first or a.spectrum_file or a.spectrum_window or a.spectrum_every != 1) and not a.spectrum:
        p.error("--spectrum-every / --spectrum-first / --spectrum-window / --spectrum-file need --spectrum-planes or --spectrum-box")
