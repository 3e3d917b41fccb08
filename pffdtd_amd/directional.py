"""Directional band maps: per octave band, the lateral energy fraction (LF, LFC of ISO 3382-1) and the sound intensity of every cell of a plane
or a box, from products of the band-filtered pressure and the band-filtered pressure GRADIENT along file axes, summed into time bins on the device
as the run goes, in one HDF5 file.

    fd = FieldDirectional(path, sd, regions, bands_hz, axes, bin_ms, first=0, order=3, lowcut_hz=10, lowcut_order=4, stencil="axis")
                                                 regions: [(lo, hi, stride)], FILE x, y, z
    fd.take(obj, n)                              obj: a HipEngine or HipMulti that has taken the steps 0 .. n-1; n >= first: every such step is a sample
    fd.write()
    directional.parameters(S, prod, bin_seconds) host numpy: LF, LFC per band, cell and axis; the intensity vector per bin and over the run

The components of one vector band accumulator per region (engine.VectorBandAccumulator, pf_engine_vband_*) are the cell itself (omni) and the
central difference d_a = u[c + e_a] - u[c - e_a] along each chosen axis.  The omni component runs through decay.pre_sections -- what
ProcessOutputs.initial_process applies to the receivers -- and one identity section; a difference runs through the same sections and then through
ONE first-order section that turns it into the pressure a figure-of-eight microphone along +a would give:  p_a = rho c v_a = -c * integral of
dp/dx_a dt,  dp/dx_a ~ d_a / 2h.  The integral is the bilinear integrator (Ts / 2)(1 + z^-1) / (1 - z^-1); its pole at 1 is cancelled analytically
against the zero of butter(1, 2 Ts lowcut_hz, 'high') = k (1 - z^-1) / (1 - a z^-1), which leaves
    g * [1, 1, 0, 1, -a, 0],     g = -(c / 2h)(Ts / 2) k
(gradient_sections).  A plane wave along +a then gives p_a = cos(theta) p, up to the sinc of the central difference, (omega h / c)^2 / 6, the
bilinear integrator, (omega Ts)^2 / 12, and the first-order high-pass, (lowcut_hz / f)^2 / 2 (tests/test_directional_host.py).
The products, per chosen axis a (component k): (0, 0) -- once --, (k, k), (0, k) plain and (0, k) absolute.

Every step from `first` on is a sample, and a sample is never shifted, exactly as decay.FieldDecay; a chain that is sampled is created with
PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES.  These difference components exist on Cartesian grids only (fcc_flag 0), and a region keeps one cell clear
of both faces along every chosen axis: the engine refuses anything else by name.

FCC grids (fcc_flag 1, the checkerboard, and 2, the checkerboard folded along y) take stencil="lattice": an axis neighbour at +-1 is no node of the
lattice, but eight of a node's twelve neighbours sit at +-1 along any axis a, in four opposite pairs, and the sum of the four pair differences is
    L_a = sum over the pairs of u[c + o] - u[c - o] = 8 h du/da + O(h^3)
(components 4 / 5 / 6 of the vector band accumulator; the offsets and the association: include/pffdtd_hip.h).  The same sections with span = 8 in
g's place of 2 turn it into p_a; `axes` stays 1 .. 3.  A region keeps one cell clear of ALL six faces.  The device works in STORED coordinates.  On a
folded grid of Ny stored rows the cell (ix, j, iz) holds the node of physical row j where ix + j + iz is even and of physical row 2 (Ny - 1) - 1 - j
where it is odd (the upper half of the room, mirrored; row Ny - 1 is the fold's ghost, a copy of row Ny - 2): fold_coordinates.  There the stored
+y is the room's -y, so the file's S has every product with an odd number of y factors and mode 0 negated in the odd cells -- exact -- and the file
carries each cell's physical row; the raw sums and the filter state stay in storage form, which is what a resumed run continues bit for bit.  The
axes are the folder's file axes: a rotation sim_setup applied before it wrote the folder is not undone (the folder does not record it).

The file (write(): written to a temporary name and moved into place with os.replace) holds
    regions  int64 [R, 9]    bands  float64 [B]    axes  int64 [A] (1 / 2 / 3 = x / y / z)    Ts  float64    sampling  int64 [3] = first, bin_steps, count
    pre_sos  float64 [1 + A, npre, 6]      band_sos  float64 [B, nsec, 6]      prod  int64 [1 + 3 A, 3]
    r{i:03d}_S      float64 [nprod, B, nbin, c0, c1, c2] of region i: sums * infac^2
    r{i:03d}_sums   the raw sums, and  r{i:03d}_state  float64 [1 + A, npre + B * nsec, 2, c0, c1, c2]: what a resumed run continues from
    stencil  int64 (0: axis, 1: lattice; read() gives the name)    fcc_flag  int64
    r{i:03d}_iy     int64 [c0, c1, c2], folded grids (fcc_flag 2) only: the physical y index of every cell of region i
With resume_at the file must match in regions, bands, axes, stencil, Ts, first, bin_steps, pre_sos, band_sos and prod, and its count must be the number of
sample steps below resume_at; otherwise it is refused with the field's name.
"""
import os

import numpy as np
from scipy.signal import butter

from . import h5io
from .decay import band_sections, pre_sections
from .engine import PfError

IDENTITY = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])


def parse_axes(spec):
    """'y' or 'y,x,z' -> the components 1 / 2 / 3 of those file axes, in the order given"""
    names = [s.strip().lower() for s in spec.split(",") if s.strip()]
    if not names or any(s not in ("x", "y", "z") for s in names) or len(set(names)) != len(names):
        raise ValueError(f"--dir-axes: '{spec}' is not one to three different axes out of x, y, z")
    return [1 + "xyz".index(s) for s in names]


STENCILS = ("axis", "lattice")
LATTICE_SPAN = 8  # L_a = 8 h du/da + O(h^3)


def fold_coordinates(region, Ny_folded):
    """region (lo, hi, stride) of a FOLDED grid (fcc_flag 2) with Ny_folded stored rows -> (ix, iy_phys, iz, upper), int64 / bool arrays of the
    region's shape [c0, c1, c2]: the stored x and z of every cell, the PHYSICAL row of the node it holds -- j where ix + j + iz is even,
    2 (Ny_folded - 1) - 1 - j where it is odd (synth.fold_fcc mirrors the rows iy >= Ny / 2 of a room of Ny = 2 (Ny_folded - 1) rows onto
    Ny - 1 - iy) -- and whether that node is of the mirrored upper half.  Cells of the fold's ghost row j = Ny_folded - 1 hold no node of their
    own: iy_phys = -1 there."""
    lo, hi, st = region
    ax = [np.arange(int(lo[a]), int(hi[a]), int(st[a]), dtype=np.int64) for a in range(3)]
    ix, j, iz = np.meshgrid(*ax, indexing="ij")
    upper = ((ix + j + iz) & 1) == 1
    iy = np.where(upper, 2 * (int(Ny_folded) - 1) - 1 - j, j)
    iy = np.where(j == int(Ny_folded) - 1, -1, iy)
    return ix, iy, iz, upper


def gradient_sections(Ts, h, c, diff, lowcut_hz, lowcut_order, span=2):
    """-> (omni [npre, 6], gradient [npre, 6]): decay.pre_sections(Ts, diff, lowcut_hz, lowcut_order) followed by an identity section for the cell
    itself, and by g * [1, 1, 0, 1, -a, 0], g = -(c / (span h))(Ts / 2) k, for a difference that spans `span` cells: 2, the central difference;
    8, the lattice difference of an FCC grid (see the module's text)"""
    if not lowcut_hz > 0:
        raise ValueError("FieldDirectional: lowcut_hz: the gradient's integrator needs the low-cut, lowcut_hz > 0")
    pre = pre_sections(Ts, diff, lowcut_hz, lowcut_order)
    b, a = butter(1, 2.0 * Ts * lowcut_hz, btype="high")  # k (1 - z^-1) / (1 - a z^-1)
    k, pole = float(b[0]), -float(a[1])
    g = -(c / (float(span) * h)) * (Ts / 2.0) * k
    last = np.array([g, g, 0.0, 1.0, -pole, 0.0])
    return (np.ascontiguousarray(np.vstack([pre, IDENTITY[None]]), dtype=np.float64), np.ascontiguousarray(np.vstack([pre, last[None]]), dtype=np.float64))


def products(naxes):
    """int64 [1 + 3 naxes, 3]: (0, 0, 0), then per axis component k = 1 .. naxes: (k, k, 0), (0, k, 0), (0, k, 1)"""
    rows = [(0, 0, 0)]
    for k in range(1, naxes + 1):
        rows += [(k, k, 0), (0, k, 0), (0, k, 1)]
    return np.array(rows, dtype=np.int64)


class FieldDirectional:
    def __init__(self, path, sd, regions, bands_hz, axes, bin_ms, first=0, order=3, lowcut_hz=10.0, lowcut_order=4, resume_at=None, stencil="axis"):
        self.path, self.sd = os.fspath(path), sd
        self.stencil, self.fcc_flag = stencil, int(getattr(sd, "fcc_flag", 0))
        self.regions = [tuple(tuple(int(v) for v in t) for t in r) for r in regions]
        self.bands = np.ascontiguousarray(bands_hz, dtype=np.float64).reshape(-1)
        self.axes = np.ascontiguousarray(axes, dtype=np.int64).reshape(-1)
        self.first, self.Ts = int(first), float(sd.Ts)
        self.bin_steps = int(round(float(bin_ms) * 1e-3 / self.Ts))
        if self.first < 0 or not self.regions or self.bands.size == 0 or int(order) < 1:
            raise ValueError("FieldDirectional: at least one region and one band, first >= 0, order >= 1")
        if self.axes.size < 1 or self.axes.size > 3 or np.any(self.axes < 1) or np.any(self.axes > 3) or len(set(self.axes.tolist())) != self.axes.size:
            raise ValueError(f"FieldDirectional: axes: {self.axes.tolist()} is not one to three different axes out of 1, 2, 3 (x, y, z)")
        if self.bands.size > 16 or int(order) > 8:
            raise ValueError(f"FieldDirectional: bands: {self.bands.size} bands of order {order}, a vector band accumulator holds 16 of 8 sections")
        if self.bin_steps < 1:
            raise ValueError(f"FieldDirectional: bin_ms: {bin_ms} ms is less than half a step of {self.Ts * 1e3:g} ms")
        if stencil not in STENCILS:
            raise ValueError(f"FieldDirectional: stencil: {stencil!r} is neither \"axis\" nor \"lattice\"")
        if stencil == "axis" and self.fcc_flag != 0:
            raise ValueError("FieldDirectional: fcc_flag: the central difference along an axis exists on Cartesian grids only (fcc_flag 0); an FCC grid takes "
                             "stencil=\"lattice\", the difference over the lattice's own neighbours")
        if stencil == "lattice" and self.fcc_flag == 0:
            raise ValueError("FieldDirectional: stencil=\"lattice\": the lattice difference exists on FCC grids only (fcc_flag 1 or 2); a Cartesian grid takes "
                             "stencil=\"axis\"")
        if getattr(sd, "h", None) is None or getattr(sd, "c", None) is None:
            raise ValueError("FieldDirectional: h, c: the scene's constants hold no grid spacing or speed of sound (sim_consts.h5: h, c)")
        omni, grad = gradient_sections(self.Ts, float(sd.h), float(sd.c), bool(getattr(sd, "diff", False)), float(lowcut_hz), int(lowcut_order),
                                       span=LATTICE_SPAN if stencil == "lattice" else 2)
        if omni.shape[0] > 8:
            raise ValueError(f"FieldDirectional: lowcut_order: {omni.shape[0]} sections per component, a vector band accumulator holds 8")
        self.pre_sos = np.ascontiguousarray(np.stack([omni] + [grad] * self.axes.size))
        self.band_sos = band_sections(self.Ts, self.bands, int(order))
        self.comp = np.concatenate([[0], self.axes + (3 if stencil == "lattice" else 0)]).astype(np.int64)
        self.prod = products(self.axes.size)
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
        """one vector band accumulator per region on obj (a HipEngine or a HipMulti); a resumed run's sums and filter state go into them"""
        if self.accs is not None:
            return
        self.accs = [obj.vector_band_accumulator(lo, hi, st, comp=self.comp, pre_sos=self.pre_sos, band_sos=self.band_sos, prod=self.prod, nbin=self.nbin)
                     for lo, hi, st in self.regions]
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
            raise ValueError(f"FieldDirectional.take: no sample is due at step {n} (first {self.first}, Nt {self.sd.Nt})")
        self.attach(obj)
        try:
            for a in self.accs:
                a.add(self.bin_of(n))
        except PfError as e:
            if e.code != 4:  # (PF_ERR_STATE: a slab inside a pair or triple; no slab took the sample)
                raise
            err = PfError(f"directional maps: step {n} cannot be sampled, a slab is inside a blocked pass there, and a sample is never shifted: "
                          f"create the chain with PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES ({e})")
            err.code = 4
            raise err
        return n

    def write(self):
        """the file as it stands: every region's sums and filter state so far"""
        if self.accs is None:
            raise ValueError("FieldDirectional.write: no accumulators yet (attach or take first)")
        tmp = self.path + ".tmp"
        h5io.write(tmp, "regions", self.table, append=False)
        h5io.write(tmp, "bands", self.bands)
        h5io.write(tmp, "axes", self.axes)
        h5io.write(tmp, "Ts", np.float64(self.Ts))
        h5io.write(tmp, "sampling", np.array([self.first, self.bin_steps, self.count], dtype=np.int64))
        h5io.write(tmp, "pre_sos", self.pre_sos)
        h5io.write(tmp, "band_sos", self.band_sos)
        h5io.write(tmp, "prod", self.prod)
        h5io.write(tmp, "stencil", np.int64(STENCILS.index(self.stencil)))
        h5io.write(tmp, "fcc_flag", np.int64(self.fcc_flag))
        # the products whose sign follows the room's y: an odd number of y factors, mode 0 (folded grids: the stored +y of an odd cell is the room's -y)
        ycomp = [k for k, c in enumerate(self.comp.tolist()) if c in (2, 5)]
        flip = [p for p, (i, j, mode) in enumerate(self.prod.tolist()) if mode == 0 and ((i in ycomp) != (j in ycomp))]
        for i, a in enumerate(self.accs):
            e, s = a.get()
            h5io.write(tmp, f"r{i:03d}_sums", e)
            h5io.write(tmp, f"r{i:03d}_state", s)
            S = e * (self.sd.infac * self.sd.infac)
            if self.fcc_flag == 2:
                _, iy, _, upper = fold_coordinates(self.regions[i], self.sd.Ny)
                h5io.write(tmp, f"r{i:03d}_iy", np.ascontiguousarray(iy, dtype=np.int64))
                for p in flip:
                    S[p][..., upper] = -S[p][..., upper]
            h5io.write(tmp, f"r{i:03d}_S", S)
        os.replace(tmp, self.path)

    def close(self):
        for a in self.accs or []:
            a.close()
        self.accs = None

    def _read_matching(self, resume_at):
        """(count, [raw sums per region], [filter state per region]) of the file a resumed run continues, or ValueError naming the field that differs"""
        if not os.path.exists(self.path):
            raise ValueError(f"{self.path}: no directional file to resume from")
        f = read(self.path, raw=True)
        for name, mine in (("regions", self.table), ("bands", self.bands), ("axes", self.axes)):
            if not np.array_equal(f[name], mine):
                raise ValueError(f"{self.path}: {name}: the file holds the sums of other {name}")
        if f["stencil"] != self.stencil:
            raise ValueError(f"{self.path}: stencil: the file holds the sums of stencil=\"{f['stencil']}\", \"{self.stencil}\" is asked for")
        if f["Ts"] != self.Ts:
            raise ValueError(f"{self.path}: Ts: {f['Ts']!r} in the file, {self.Ts!r} in the scene")
        first, bin_steps, count = (int(v) for v in f["sampling"])
        if first != self.first:
            raise ValueError(f"{self.path}: first: {first} in the file, {self.first} asked for")
        if bin_steps != self.bin_steps:
            raise ValueError(f"{self.path}: bin_steps: {bin_steps} in the file, {self.bin_steps} asked for")
        if not np.array_equal(f["pre_sos"], self.pre_sos):
            raise ValueError(f"{self.path}: pre_sos: the file's sums went through other sections per component (low-cut, integrator, grid spacing)")
        if not np.array_equal(f["band_sos"], self.band_sos):
            raise ValueError(f"{self.path}: band_sos: the file's sums went through other band filters (order)")
        if not np.array_equal(f["prod"], self.prod):
            raise ValueError(f"{self.path}: prod: the file holds the sums of other products")
        if count != self.samples_below(resume_at):
            raise ValueError(f"{self.path}: count: the file holds {count} samples, {self.samples_below(resume_at)} sample steps lie below step {resume_at}")
        return count, f["sums"], f["state"]


def read(path, raw=False):
    """-> dict(regions [R, 9], bands [B], axes [A], Ts, sampling [first, bin_steps, count], pre_sos [1 + A, npre, 6], band_sos [B, nsec, 6], prod
    [nprod, 3], stencil "axis" / "lattice", fcc_flag (a file from before they were written: "axis", 0), S: per region float64 [nprod, B, nbin, c0, c1,
    c2]; fcc_flag 2: iy, per region int64 [c0, c1, c2]; raw: also sums and state, unscaled) of a file FieldDirectional wrote"""
    regions = np.asarray(h5io.read(path, "regions", h5io.I64)).reshape(-1, 9)
    axes = np.asarray(h5io.read(path, "axes", h5io.I64)).reshape(-1)
    pre = np.asarray(h5io.read(path, "pre_sos", h5io.F64))
    out = {"regions": regions, "bands": np.asarray(h5io.read(path, "bands", h5io.F64)).reshape(-1), "axes": axes, "Ts": float(h5io.read(path, "Ts", h5io.F64)),
           "sampling": np.asarray(h5io.read(path, "sampling", h5io.I64)).reshape(3), "pre_sos": pre.reshape(1 + axes.size, -1, 6),
           "band_sos": np.asarray(h5io.read(path, "band_sos", h5io.F64)), "prod": np.asarray(h5io.read(path, "prod", h5io.I64)).reshape(-1, 3)}
    out["stencil"] = STENCILS[int(h5io.read(path, "stencil", h5io.I64))] if h5io.exists(path, "stencil") else "axis"
    out["fcc_flag"] = int(h5io.read(path, "fcc_flag", h5io.I64)) if h5io.exists(path, "fcc_flag") else 0
    for key in ("S",) + (("sums", "state") if raw else ()):
        out[key] = [np.asarray(h5io.read(path, f"r{i:03d}_{key}", h5io.F64)) for i in range(len(regions))]
    if out["fcc_flag"] == 2:
        out["iy"] = [np.asarray(h5io.read(path, f"r{i:03d}_iy", h5io.I64)) for i in range(len(regions))]
    return out


def _limit_bins(bin_seconds):
    """-> (k5, k80): the 5 ms and 80 ms limits in whole bins.  A file's bin is a whole number of steps, bin_steps = round(bin_ms 1e-3 / Ts), so
    bin_steps * Ts misses the nominal bin_ms by up to half a step: 0.4 % for 5 ms bins at 25.5 kHz, below 1 % for any bin of 50 steps or more.
    Hence: 5 ms must be k5 bins to within 1 % (k5 >= 1), the nominal bin is then 5 ms / k5, and 80 ms is 16 k5 of them."""
    k = 0.005 / float(bin_seconds)
    k5 = int(round(k))
    if k5 < 1 or abs(k - k5) > 0.01 * k5:
        raise ValueError(f"directional.parameters: bin_seconds: the 5 ms limit is {k:g} bins of {bin_seconds * 1e3:g} ms, not a whole number of bins (to within 1 %, the "
                         f"rounding of a bin to whole steps): use bins of 5 ms, 2.5 ms, 1 ms, ...")
    return k5, 16 * k5


def parameters(S, prod, bin_seconds):
    """S: float64 [nprod, B, nbin, c0, c1, c2] -- a region's r*_S --, prod [nprod, 3] as the file holds it, bin_seconds = bin_steps * Ts.  -> dict of
        onset            [B, cells]          a cell's first bin within 20 dB of its largest omni bin: the onset decay.parameters uses
        LF, LFC          [A, B, cells]       sum of p_a^2 (LFC: of |p_a p|) over 5 .. 80 ms after the onset / sum of p^2 over 0 .. 80 ms (nan: a silent cell)
        intensity        [A, B, nbin, cells] the per-bin vector sum of p * p_a: where the energy flows
        intensity_total  [A, B, cells]       ... summed over the run
    per axis in the order of the file's `axes`.  The limits at 5 ms and 80 ms must be whole bins (ValueError otherwise): 5 ms bins, or 2.5, 1, ... --
    whole to within the 1 % by which bin_steps * Ts misses the nominal bin (_limit_bins)."""
    S = np.asarray(S, dtype=np.float64)
    prod = np.asarray(prod, dtype=np.int64).reshape(-1, 3)
    if S.ndim != 6 or S.shape[0] != prod.shape[0]:
        raise ValueError(f"directional.parameters: S: shape {S.shape} is not [nprod = {prod.shape[0]}, B, nbin, c0, c1, c2]")
    k5, k80 = _limit_bins(bin_seconds)
    rows = {tuple(int(v) for v in p): i for i, p in enumerate(prod)}
    if (0, 0, 0) not in rows:
        raise ValueError("directional.parameters: prod: no row (0, 0, 0), the omni energy")
    comps = sorted({int(p[1]) for p in prod if p[1] != 0})
    for k in comps:
        for need in ((k, k, 0), (0, k, 0), (0, k, 1)):
            if need not in rows:
                raise ValueError(f"directional.parameters: prod: no row {need} for component {k}")
    nb, nbin, cells = S.shape[1], S.shape[2], S.shape[3:]

    def cols(p):  # [nbin, columns]
        return np.moveaxis(S[rows[p]], 1, 0).reshape(nbin, -1)

    e = cols((0, 0, 0))
    peak = e.max(axis=0)
    onset = np.argmax(e >= peak * 1e-2, axis=0)
    col = np.arange(e.shape[1])

    def window(x, k0, k1):  # sum of x over the bins [onset + k0, onset + k1) of every column
        cs = np.concatenate([np.zeros((1, x.shape[1])), np.cumsum(x, axis=0)])
        return cs[np.minimum(onset + k1, nbin), col] - cs[np.minimum(onset + k0, nbin), col]

    omni = window(e, 0, k80)
    out = {"onset": onset.reshape((nb,) + cells), "LF": [], "LFC": [], "intensity": [], "intensity_total": []}
    for k in comps:
        with np.errstate(divide="ignore", invalid="ignore"):
            out["LF"].append((window(cols((k, k, 0)), k5, k80) / omni).reshape((nb,) + cells))
            out["LFC"].append((window(cols((0, k, 1)), k5, k80) / omni).reshape((nb,) + cells))
        out["intensity"].append(S[rows[(0, k, 0)]])
        out["intensity_total"].append(S[rows[(0, k, 0)]].sum(axis=1))
    for name in ("LF", "LFC", "intensity", "intensity_total"):
        out[name] = np.stack(out[name]) if comps else np.zeros((0,))
    return out
