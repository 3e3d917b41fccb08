"""Wall absorption maps: which surface takes the energy out of the room -- the energy every step loses per frequency-dependent wall node, per
material and per time bin, with the loss at the open boundary (the ABC shell) and the energy the sources put in, summed on the device as the run
goes, in one HDF5 file.  The one output that reads the WALLS: it has no regions.

    wa = WallAbsorption(path, sd, bin_ms=5.0, first=0)
    wa.take(obj, n)          obj: a HipEngine or HipMulti that stands before step n (it has taken the steps 0 .. n-1); every n from `first` on
    wa.settle(obj, n)        before a write: the step before n is accounted too (take(obj, n) unless it was taken)
    wa.write()
    absorption.read(path), absorption.parameters(f), absorption.node_map(f)             host numpy

The terms are the reference Python engine's E_lost and E_in (python/fdtd/sim_fdtd.py:615-620), so over a run
    materials.sum() + open_boundary.sum() = E_lost[-1]        input.sum() = E_in[-1]
and the room's remaining energy is cumsum(input) - cumsum(losses).  engine.Absorption (pf_engine_absorb_*) keeps the sums; `scales` gives it the
reference's factors from sd: V_fac (2 on FCC grids, else 1), h, l, l2 and the materials' E = DEF[:, 1].  The sample before step n closes step
n - 1: it needs the branch currents of two consecutive samples, so every step from `first` on is sampled -- there is no `every` -- and the first
sample of a run (or of a resumed run) only primes.  Step s goes to bin (s - first) // bin_steps, bin_steps = round(bin_ms * 1e-3 / Ts).

BROADBAND: the loss is quadratic in the branch currents, so the sums cannot be split into bands afterwards.  Octave-band absorption needs a
band-limited source (one run per band) or per-node filters in front of the square; neither is here.

WallAbsorption is a field_output.FieldOutput without regions: a sample is never shifted, a chain that is sampled is created with
PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES, and write and the rules of a resume are described there.  The file holds
    Ts, bin_seconds  float64      sampling  int64 [3] = first, bin_steps, count (steps accounted)      Nm  int64
    bnl_ixyz  int64 [Nbl]   mat_bnl  int64 [Nbl]     the frequency-dependent nodes (file index x * Ny * Nz + y * Nz + z) and their materials
    materials  float64 [nbin, Nm]   open_boundary  float64 [nbin]   input  float64 [nbin]   nodes  float64 [Nbl]
        in the units of the reference Python engine on the same folder: the sums * infac^2 (the C path's scale_input divides the input by infac)
    raw_materials, raw_open_boundary, raw_input, raw_nodes      the sums as the device holds them: what a resumed run continues from
With resume_at the file must match in Ts, first, bin_steps, Nm, bnl_ixyz and mat_bnl, and its count must be the steps from `first` below resume_at.
On one domain the resumed file equals the file of a run in one piece byte for byte; a chain of slabs resumes its node sums bit for bit and its bins to
rounding (Nbl * 2^-52 relative): the file keeps the scene's bins, and the slabs then add the same terms in another order (csrc/pf_absorb_cut.h).
"""
import numpy as np

from . import h5io
from .engine import PF_MMB
from .field_output import FieldOutput

KEYS = ("materials", "open_boundary", "input", "nodes")


def _write(path, name, data, append=True):
    """without HDF5's modification times: the file's bytes depend on its contents alone, so a resumed run's file IS the file of the run in one piece"""
    h5io.write(path, name, data, append=append, times=False)


def scales(sd):
    """-> (E float64 [Nm, 12], wall_scale, abc_scale, in_scale) of engine.Absorption for scene sd (sim_fdtd.py:615-620)"""
    if getattr(sd, "h", None) is None:
        raise ValueError("WallAbsorption: the scene's constants hold no grid spacing h")
    V = 2.0 if sd.fcc_flag > 0 else 1.0
    E = np.zeros((max(sd.Nm, 1), PF_MMB), dtype=np.float64)
    for k, d in enumerate(sd.DEF):
        E[k, :d.shape[0]] = d[:, 1]
    return E[:sd.Nm], V * 0.25 * sd.h / sd.l, 0.5 * V * sd.h / sd.l, 0.5 * V * sd.h / sd.l2


class WallAbsorption(FieldOutput):
    label, noun, holds, observers_noun = "wall absorption", "absorption", "sums", "absorption maps"

    def __init__(self, path, sd, bin_ms=5.0, first=0, resume_at=None):
        super().__init__(path, sd, [], first)
        self.bin_steps = int(round(float(bin_ms) * 1e-3 / self.Ts))
        if self.first < 0:
            raise ValueError("WallAbsorption: first >= 0")
        if self.bin_steps < 1:
            raise ValueError(f"WallAbsorption: bin_ms: {bin_ms} ms is less than half a step of {self.Ts * 1e3:g} ms")
        self.nbin = max(1, -(-(sd.Nt - self.first) // self.bin_steps))
        self.Nm = np.int64(sd.Nm)
        self.bnl_ixyz = np.ascontiguousarray(sd.bnl_ixyz, dtype=np.int64)
        self.mat_bnl = np.ascontiguousarray(sd.mat_bnl, dtype=np.int64)
        self._scales = scales(sd)
        self._taken = None  # the n of the last sample
        self._resume(resume_at)

    def bin_of(self, step):
        """the time bin of step `step` >= first"""
        return (step - self.first) // self.bin_steps

    # ---- the one observer ----
    def _observers(self, obj):
        return [obj.absorption(*self._scales, nbin=self.nbin)]

    def _restore_observer(self, a, i, count, sums):
        a.set(sums, count)

    def _sample(self, n):
        return n, self.bin_of(max(n - 1, self.first))  # (the sample before step n closes step n - 1; a priming sample's bin is not used)

    def take(self, obj, n):
        if self._taken == n:  # (settle took it)
            return n
        super().take(obj, n)
        self._taken = n
        return n

    def settle(self, obj, n):
        """the engine stands before step n: the step before it is accounted too, as a write needs it (a sample at n = Nt, or where a run stops, closes the
        last step; the run that goes on from a checkpoint takes the sample of n again, which then only primes)"""
        if self._taken == n or n <= self.first:
            return
        self.attach(obj)
        for o in self.observers:
            o.add(*self._sample(n))
        self._taken = n

    # ---- the file ----
    def _write_head(self, path, append):
        _write(path, "Ts", np.float64(self.Ts), append=append)
        _write(path, "bin_seconds", np.float64(self.bin_steps * self.Ts))
        _write(path, "sampling", np.array([self.first, self.bin_steps, self.count], dtype=np.int64))
        _write(path, "Nm", np.int64(self.Nm))
        if self.bnl_ixyz.size:
            _write(path, "bnl_ixyz", self.bnl_ixyz)
            _write(path, "mat_bnl", self.mat_bnl)

    def _write_region(self, path, i, a):
        s = a.get()
        k2 = self.sd.infac * self.sd.infac
        for key in KEYS:
            if s[key].size:
                _write(path, "raw_" + key, s[key])
                _write(path, key, s[key] * k2)

    def _read_file(self):
        f = read(self.path, raw=True)
        f["regions"] = self.table  # (no regions: nothing to compare)
        return f

    def _checks(self, f):
        return [*self._same_clock(f), self._asked("bin_steps", f["sampling"][1], self.bin_steps), self._asked("Nm", f["Nm"], int(self.Nm)),
                self._other(f, "bnl_ixyz", "wall nodes"), self._other(f, "mat_bnl", "materials")]

    def _saved(self, f, count):
        return count, {k: f["raw_" + k] for k in KEYS}


def read(path, raw=False):
    """-> dict(Ts, bin_seconds, sampling [first, bin_steps, count], Nm, bnl_ixyz [Nbl], mat_bnl [Nbl], materials [nbin, Nm], open_boundary [nbin],
    input [nbin], nodes [Nbl]; raw: also raw_*, the unscaled sums) of a file WallAbsorption wrote"""
    out = {"Ts": float(h5io.read(path, "Ts", h5io.F64)), "bin_seconds": float(h5io.read(path, "bin_seconds", h5io.F64)),
           "sampling": np.asarray(h5io.read(path, "sampling", h5io.I64)).reshape(3), "Nm": int(h5io.read(path, "Nm", h5io.I64))}
    have = h5io.exists(path, "bnl_ixyz")
    for key in ("bnl_ixyz", "mat_bnl"):
        out[key] = np.asarray(h5io.read(path, key, h5io.I64)).reshape(-1) if have else np.zeros(0, dtype=np.int64)
    nbin = np.asarray(h5io.read(path, "open_boundary", h5io.F64)).size
    shape = {"materials": (nbin, out["Nm"]), "open_boundary": (nbin,), "input": (nbin,), "nodes": (out["bnl_ixyz"].size,)}
    for pre in ("",) + (("raw_",) if raw else ()):
        for key in KEYS:
            out[pre + key] = (np.asarray(h5io.read(path, pre + key, h5io.F64)).reshape(shape[key]) if int(np.prod(shape[key])) else np.zeros(shape[key]))
    return out


def parameters(materials, open_boundary, input):
    """materials [nbin, Nm], open_boundary [nbin], input [nbin] of a file -> dict of
        absorbed   [nbin, Nm + 1]   cumulative energy absorbed by each material and (last column) the open boundary, up to the end of each bin
        share      [nbin, Nm + 1]   absorbed / the energy injected up to then (nan before any energy went in)
        remaining  [nbin]           the room's energy at the end of each bin: cumsum(input) - cumsum(all losses)"""
    losses = np.concatenate([np.asarray(materials, dtype=np.float64).reshape(len(open_boundary), -1), np.asarray(open_boundary, dtype=np.float64)[:, None]], axis=1)
    absorbed = np.cumsum(losses, axis=0)
    injected = np.cumsum(np.asarray(input, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(injected[:, None] != 0, absorbed / injected[:, None], np.nan)
    return {"absorbed": absorbed, "share": share, "remaining": injected - absorbed.sum(axis=1)}


def node_map(f, Ny, Nz):
    """f: read(path); Ny, Nz: the grid's -> (ix, iy, iz, energy), one entry per frequency-dependent node: the energy it absorbed over the run"""
    ii = np.asarray(f["bnl_ixyz"], dtype=np.int64)
    return ii // (Ny * Nz), (ii // Nz) % Ny, ii % Nz, np.asarray(f["nodes"], dtype=np.float64)


def add_arguments(p):
    """the --absorption* arguments of the command line"""
    p.add_argument("--absorption", action="store_true", help="sum the energy every step loses per wall node, per material and at the open boundary, and the sources' input, on the device "
                                                            "into sim_absorption.h5 in the data folder")
    p.add_argument("--absorption-bin-ms", type=float, default=5.0, metavar="MS", help="... in time bins of MS milliseconds (default 5)")
    p.add_argument("--absorption-first", type=int, default=0, metavar="N", help="... from step N on (default 0)")


def check_arguments(p, a):
    """a.absorption: asked for?  The other two without it are refused"""
    if a.absorption_bin_ms <= 0 or a.absorption_first < 0:
        p.error("--absorption-bin-ms: positive, --absorption-first: not negative")
    if (a.absorption_first or a.absorption_bin_ms != 5.0) and not a.absorption:
        p.error("--absorption-bin-ms / --absorption-first need --absorption")
