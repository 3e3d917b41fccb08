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

Every step from `first` on is a sample, exactly as decay.FieldDecay (both are decay.BandOutput, a field_output.FieldOutput: the schedule, take, write
and the rules of a resume are described there).  These difference components exist on Cartesian grids only (fcc_flag 0), and a region keeps one cell clear
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

The file holds
    regions  int64 [R, 9]    bands  float64 [B]    axes  int64 [A] (1 / 2 / 3 = x / y / z)    Ts  float64    sampling  int64 [3] = first, bin_steps, count
    pre_sos  float64 [1 + A, npre, 6]      band_sos  float64 [B, nsec, 6]      prod  int64 [1 + 3 A, 3]
    r{i:03d}_S      float64 [nprod, B, nbin, c0, c1, c2] of region i: sums * infac^2
    r{i:03d}_sums   the raw sums, and  r{i:03d}_state  float64 [1 + A, npre + B * nsec, 2, c0, c1, c2]: what a resumed run continues from
    stencil  int64 (0: axis, 1: lattice; read() gives the name)    fcc_flag  int64
    r{i:03d}_iy     int64 [c0, c1, c2], folded grids (fcc_flag 2) only: the physical y index of every cell of region i
With resume_at the file must match in regions, bands, axes, stencil, Ts, first, bin_steps, pre_sos, band_sos and prod, and its count must be the number of
sample steps below resume_at; otherwise it is refused with the field's name.
"""
import numpy as np
from scipy.signal import butter

from . import h5io
from .decay import BandOutput, band_sections, pre_sections

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


def vector_setup(who, holder, sd, axes, stencil, lowcut_hz, lowcut_order):
    """-> (axes int64 [A], pre_sos [1 + A, npre, 6]: the omni sections, then the gradient's per axis, comp int64 [1 + A]: the cell and the difference
    `stencil` names per axis) for the scene sd, or ValueError in the name of the class `who`, whose observer is "a `holder`" """
    axes = np.ascontiguousarray(axes, dtype=np.int64).reshape(-1)
    fcc_flag = int(getattr(sd, "fcc_flag", 0))
    if axes.size < 1 or axes.size > 3 or np.any(axes < 1) or np.any(axes > 3) or len(set(axes.tolist())) != axes.size:
        raise ValueError(f"{who}: axes: {axes.tolist()} is not one to three different axes out of 1, 2, 3 (x, y, z)")
    if stencil not in STENCILS:
        raise ValueError(f"{who}: stencil: {stencil!r} is neither \"axis\" nor \"lattice\"")
    if stencil == "axis" and fcc_flag != 0:
        raise ValueError(f"{who}: fcc_flag: the central difference along an axis exists on Cartesian grids only (fcc_flag 0); an FCC grid takes "
                         "stencil=\"lattice\", the difference over the lattice's own neighbours")
    if stencil == "lattice" and fcc_flag == 0:
        raise ValueError(f"{who}: stencil=\"lattice\": the lattice difference exists on FCC grids only (fcc_flag 1 or 2); a Cartesian grid takes "
                         "stencil=\"axis\"")
    if getattr(sd, "h", None) is None or getattr(sd, "c", None) is None:
        raise ValueError(f"{who}: h, c: the scene's constants hold no grid spacing or speed of sound (sim_consts.h5: h, c)")
    omni, grad = gradient_sections(float(sd.Ts), float(sd.h), float(sd.c), bool(getattr(sd, "diff", False)), float(lowcut_hz), int(lowcut_order),
                                   span=LATTICE_SPAN if stencil == "lattice" else 2)
    if omni.shape[0] > 8:
        raise ValueError(f"{who}: lowcut_order: {omni.shape[0]} sections per component, a {holder} holds 8")
    return axes, np.ascontiguousarray(np.stack([omni] + [grad] * axes.size)), np.concatenate([[0], axes + (3 if stencil == "lattice" else 0)]).astype(np.int64)


def y_components(comp):
    """the positions in the component list `comp` of the differences along y (2: axis, 5: lattice).  On a folded grid (fcc_flag 2) the stored +y
    of an odd cell (fold_coordinates: upper) is the room's -y: what is odd in these components is negated there -- exact"""
    return [k for k, c in enumerate(np.asarray(comp).tolist()) if c in (2, 5)]


def products(naxes):
    """int64 [1 + 3 naxes, 3]: (0, 0, 0), then per axis component k = 1 .. naxes: (k, k, 0), (0, k, 0), (0, k, 1)"""
    rows = [(0, 0, 0)]
    for k in range(1, naxes + 1):
        rows += [(k, k, 0), (0, k, 0), (0, k, 1)]
    return np.array(rows, dtype=np.int64)


class FieldDirectional(BandOutput):
    label, noun, holder, sections = "directional maps", "directional", "vector band accumulator", "sections per component (low-cut, integrator, grid spacing)"

    def __init__(self, path, sd, regions, bands_hz, axes, bin_ms, first=0, order=3, lowcut_hz=10.0, lowcut_order=4, resume_at=None, stencil="axis"):
        super().__init__(path, sd, regions, first)
        self.stencil, self.fcc_flag = stencil, int(getattr(sd, "fcc_flag", 0))
        self._bands_and_bins(bands_hz, bin_ms, order)
        self.axes, self.pre_sos, self.comp = vector_setup("FieldDirectional", self.holder, sd, axes, stencil, lowcut_hz, lowcut_order)
        self.band_sos = band_sections(self.Ts, self.bands, int(order))
        self.prod = products(self.axes.size)
        self._resume(resume_at)

    def _observer(self, obj, lo, hi, st):
        return obj.vector_band_accumulator(lo, hi, st, comp=self.comp, pre_sos=self.pre_sos, band_sos=self.band_sos, prod=self.prod, nbin=self.nbin)

    def _write_head(self, path, append):
        h5io.write(path, "regions", self.table, append=append)
        h5io.write(path, "bands", self.bands)
        h5io.write(path, "axes", self.axes)
        h5io.write(path, "Ts", np.float64(self.Ts))
        h5io.write(path, "sampling", np.array([self.first, self.bin_steps, self.count], dtype=np.int64))
        h5io.write(path, "pre_sos", self.pre_sos)
        h5io.write(path, "band_sos", self.band_sos)
        h5io.write(path, "prod", self.prod)
        h5io.write(path, "stencil", np.int64(STENCILS.index(self.stencil)))
        h5io.write(path, "fcc_flag", np.int64(self.fcc_flag))

    def _write_scaled(self, path, i, S):
        if self.fcc_flag == 2:
            _, iy, _, upper = fold_coordinates(self.regions[i], self.sd.Ny)
            h5io.write(path, f"r{i:03d}_iy", np.ascontiguousarray(iy, dtype=np.int64))
            ycomp = y_components(self.comp)
            for p, (i0, i1, mode) in enumerate(self.prod.tolist()):  # the products whose sign follows the room's y: an odd number of y factors, mode 0
                if mode == 0 and ((i0 in ycomp) != (i1 in ycomp)):
                    S[p][..., upper] = -S[p][..., upper]
        h5io.write(path, f"r{i:03d}_S", S)

    def _read_file(self):
        return read(self.path, raw=True)

    def _checks(self, f):
        return [self._other(f, "bands"), self._other(f, "axes"),
                ("stencil", f["stencil"] == self.stencil, f"the file holds the sums of stencil=\"{f['stencil']}\", \"{self.stencil}\" is asked for"),
                *self._band_checks(f), self._other(f, "prod", "products")]


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


def add_arguments(p):
    """the --dir-* arguments of the command line"""
    p.add_argument("--dir-planes", action="append", default=[], metavar="x=I,y=J,z=K", help="sum band-filtered products of the pressure and its gradient on these planes into time bins on the device (the syntax of --field-planes)")
    p.add_argument("--dir-box", action="append", default=[], metavar="x0:x1:sx,y0:y1:sy,z0:z1:sz", help="... of this strided box")
    p.add_argument("--dir-bands", default="", metavar="F1,F2,...", help="... in the octave bands around these centre frequencies in Hz")
    p.add_argument("--dir-axes", default="", metavar="y[,x,z]", help="... with the gradient along these file axes (default y)")
    p.add_argument("--dir-stencil", default="", choices=["", "axis", "lattice"], metavar="axis|lattice", help="... as the central difference along the axis (axis, the default: Cartesian grids) or the FCC lattice's difference (lattice: FCC folders)")
    p.add_argument("--dir-bin-ms", type=float, default=5.0, metavar="MS", help="... in time bins of MS milliseconds (default 5)")
    p.add_argument("--dir-first", type=int, default=0, metavar="N", help="... at every step from N on (default 0)")
    p.add_argument("--dir-file", default="", metavar="FILE", help="... into this HDF5 file (default: sim_directional.h5 in the data folder)")


def check_arguments(p, a):
    """a.directional: are directional maps asked for?  Regions without --dir-bands, and any --dir-* without a region, are refused; the defaults of
    --dir-stencil (axis) and --dir-axes (y) are filled in"""
    a.directional = bool(a.dir_planes or a.dir_box)
    if a.directional != bool(a.dir_bands) or a.dir_bin_ms <= 0 or a.dir_first < 0:
        p.error("--dir-planes / --dir-box need --dir-bands (and the other way round); --dir-bin-ms: positive, --dir-first: not negative")
    if (a.dir_first or a.dir_file or a.dir_axes or a.dir_stencil or a.dir_bin_ms != 5.0) and not a.directional:
        p.error("--dir-axes / --dir-stencil / --dir-bin-ms / --dir-first / --dir-file need --dir-planes or --dir-box")
    a.dir_stencil = a.dir_stencil or "axis"
    if a.directional and not a.dir_axes:
        a.dir_axes = "y"
