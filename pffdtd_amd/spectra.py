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

The file (write(): written to a temporary name and moved into place with os.replace, so a reader never sees half of it) holds
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
import os

import numpy as np

from . import h5io
from .engine import PfError

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


class FieldSpectrum:
    def __init__(self, path, sd, regions, freqs, every=1, first=0, window=None, resume_at=None):
        self.path, self.sd = os.fspath(path), sd
        self.regions = [tuple(tuple(int(v) for v in t) for t in r) for r in regions]
        self.freqs = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        self.every, self.first = int(every), int(first)
        if window not in WINDOWS:
            raise ValueError(f"FieldSpectrum: window = {window!r} is neither None nor 'hann'")
        self.window = WINDOWS[window]
        if self.every < 1 or self.first < 0 or not self.regions or self.freqs.size == 0:
            raise ValueError("FieldSpectrum: at least one region and one frequency, every >= 1, first >= 0")
        if 2 * self.freqs.size > 256:
            raise ValueError(f"FieldSpectrum: freqs: {self.freqs.size} frequencies, an accumulator holds 128 (256 channels)")
        self.Ts = float(sd.Ts)
        nyq = 1.0 / (2.0 * self.every * self.Ts)
        if np.any(self.freqs < 0) or np.any(self.freqs >= nyq):
            raise ValueError(f"FieldSpectrum: freqs: every frequency must lie in [0, 1 / (2 * every * Ts)) = [0, {nyq:g}) Hz: samples every {self.every} "
                             f"step(s) cannot tell {float(self.freqs.max()):g} Hz from its alias")
        self.nsamples = self.samples_below(sd.Nt)  # of the whole run: the Hann window's length
        self.table = np.array([lo + hi + st for lo, hi, st in self.regions], dtype=np.int64).reshape(-1, 9)
        self.accs, self._restore = None, None
        if resume_at is not None:
            self._restore = self._read_matching(int(resume_at))

    # ---- the sample steps ----
    def next_step(self, n):
        """the first step >= n at which a sample is due (it may lie at or past Nt: no sample then)"""
        return self.first if n <= self.first else self.first + -(-(n - self.first) // self.every) * self.every

    def due(self, n):
        return n < self.sd.Nt and self.next_step(n) == n

    def samples_below(self, n):
        """how many sample steps lie below step n"""
        return 0 if n <= self.first else -(-(n - self.first) // self.every)

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

    # ---- the sums ----
    def attach(self, obj):
        """one accumulator per region on obj (a HipEngine or a HipMulti); a resumed run's sums go into them"""
        if self.accs is not None:
            return
        self.accs = [obj.accumulator(lo, hi, st, nchan=2 * self.freqs.size) for lo, hi, st in self.regions]
        if self._restore is not None:
            count, sums = self._restore
            for a, s in zip(self.accs, sums):
                a.set(s, count)
            self._restore = None

    @property
    def count(self):
        if self.accs is None:
            return self._restore[0] if self._restore is not None else 0
        return self.accs[0].count

    def take(self, obj, n):
        """the sample of step n (due(n)) -- never of another step"""
        if not self.due(n):
            raise ValueError(f"FieldSpectrum.take: no sample is due at step {n} (first {self.first}, every {self.every}, Nt {self.sd.Nt})")
        self.attach(obj)
        w = self.weights(n)
        try:
            for a in self.accs:
                a.add(w)
        except PfError as e:
            if e.code != 4:  # (PF_ERR_STATE: a slab inside a pair or triple; no slab took the sample)
                raise
            err = PfError(f"field spectrum: step {n} cannot be sampled, a slab is inside a blocked pass there, and a sample is never shifted: "
                          f"create the chain with PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES ({e})")
            err.code = 4
            raise err
        return n

    def write(self):
        """the file as it stands: every region's sums so far"""
        if self.accs is None:
            raise ValueError("FieldSpectrum.write: no accumulators yet (attach or take first)")
        tmp = self.path + ".tmp"
        h5io.write(tmp, "regions", self.table, append=False)
        h5io.write(tmp, "freqs", self.freqs)
        h5io.write(tmp, "Ts", np.float64(self.Ts))
        h5io.write(tmp, "sampling", np.array([self.first, self.every, self.count], dtype=np.int64))
        h5io.write(tmp, "window", np.int64(self.window))
        for i, a in enumerate(self.accs):
            acc = a.get()
            h5io.write(tmp, f"r{i:03d}_acc", acc)
            h5io.write(tmp, f"r{i:03d}_re", acc[0::2] * self.sd.infac)
            h5io.write(tmp, f"r{i:03d}_im", acc[1::2] * self.sd.infac)
        os.replace(tmp, self.path)

    def close(self):
        for a in self.accs or []:
            a.close()
        self.accs = None

    def _read_matching(self, resume_at):
        """(count, [raw sums per region]) of the file a resumed run continues, or ValueError naming the field that differs"""
        if not os.path.exists(self.path):
            raise ValueError(f"{self.path}: no spectra file to resume from")
        f = read(self.path, raw=True)
        if not np.array_equal(f["regions"], self.table):
            raise ValueError(f"{self.path}: regions: the file holds the sums of other regions")
        if not np.array_equal(f["freqs"], self.freqs):
            raise ValueError(f"{self.path}: freqs: the file holds the sums of other frequencies")
        if f["Ts"] != self.Ts:
            raise ValueError(f"{self.path}: Ts: {f['Ts']!r} in the file, {self.Ts!r} in the scene")
        first, every, count = (int(v) for v in f["sampling"])
        if first != self.first:
            raise ValueError(f"{self.path}: first: {first} in the file, {self.first} asked for")
        if every != self.every:
            raise ValueError(f"{self.path}: every: {every} in the file, {self.every} asked for")
        if f["window"] != self.window:
            raise ValueError(f"{self.path}: window: {f['window']} in the file, {self.window} asked for (0 none, 1 hann)")
        if count != self.samples_below(resume_at):
            raise ValueError(f"{self.path}: count: the file holds {count} samples, {self.samples_below(resume_at)} sample steps lie below step {resume_at}")
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
