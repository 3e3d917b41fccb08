"""Field frames: planes and boxes of the field recorded as a run goes, in one HDF5 file.

    fw = FieldWriter(path, sd, regions, every, first=0)      regions: [(lo, hi, stride)] in FILE coordinates x, y, z
    n = fw.take(obj, n)                                      obj: a HipEngine or HipMulti that has taken the steps 0 .. n-1

Frames are due at the steps first, first + every, ... below Nt (field_output.Schedule).  The frame of step n is u^n -- get_region(1, ...) after run(0, n) --, the
field the receivers of step n sample: at a receiver's cell it equals that receiver's sample n.  The file holds
    regions           int64 [R, 9]   lo, hi, stride of every region
    steps             int64 [F]      the steps of the frames so far, rewritten after each frame
    r{i:03d}_n{step:07d}   float64, shape counts of region i: double(cell) * sd.infac, the expression SimData.rescale_output applies to u_out
and is written as the run goes (h5io.write(..., append=True)): a run that is stopped keeps the frames it took.  A chain whose slabs step
in blocked pairs or triples answers get_region between passes only (PfError.code == 4 inside one): `take` then advances single steps, at
most five, takes the frame at the first step that allows it and records that step -- what fdtd_main does for a checkpoint.
The regions of the command line (--field-planes, --field-box) are parsed here too: host code, no device.
"""
import os

import numpy as np

from . import h5io
from .engine import PfError
from .field_output import Schedule, normalise_regions

MAX_SHIFT = 5  # steps a frame may be taken late (a triple ends within two steps, a pair within one; slabs need not agree)


def parse_planes(spec, N):
    """'x=I,y=J,z=K' (any subset, an axis may repeat; a negative index counts from the end) -> [(lo, hi, stride)], whole planes of a grid of N cells"""
    out = []
    for item in filter(None, (s.strip() for s in spec.split(","))):
        ax, eq, val = item.partition("=")
        if ax not in ("x", "y", "z") or not eq:
            raise ValueError(f"--field-planes: '{item}' is not x=I, y=J or z=K")
        a, k = "xyz".index(ax), int(val)
        k += N[a] if k < 0 else 0
        if not 0 <= k < N[a]:
            raise ValueError(f"--field-planes: {item} is outside the grid (N{ax} = {N[a]})")
        lo, hi = [0, 0, 0], [int(v) for v in N]
        lo[a], hi[a] = k, k + 1
        out.append((tuple(lo), tuple(hi), (1, 1, 1)))
    if not out:
        raise ValueError("--field-planes: no plane given")
    return out


def parse_box(spec, N):
    """'x0:x1:sx,y0:y1:sy,z0:z1:sz' -> (lo, hi, stride); an empty start is 0, an empty end N, a missing stride 1"""
    parts = [s.strip() for s in spec.split(",")]
    if len(parts) != 3:
        raise ValueError(f"--field-box: '{spec}' is not x0:x1:sx,y0:y1:sy,z0:z1:sz")
    lo, hi, st = [], [], []
    for a, part in enumerate(parts):
        f = part.split(":")
        if len(f) not in (2, 3):
            raise ValueError(f"--field-box: '{part}' is not start:end or start:end:stride")
        lo.append(int(f[0]) if f[0] else 0)
        hi.append(int(f[1]) if f[1] else int(N[a]))
        st.append(int(f[2]) if len(f) == 3 and f[2] else 1)
        if not (0 <= lo[a] < hi[a] <= N[a] and st[a] >= 1):
            raise ValueError(f"--field-box: '{part}' is not a range inside [0, {N[a]}) with a stride >= 1")
    return tuple(lo), tuple(hi), tuple(st)


class FieldWriter(Schedule):
    def __init__(self, path, sd, regions, every, first=0, resume_at=None):
        """resume_at: the step a resumed run continues at -- an existing file is appended to and keeps its frames of the steps before it"""
        self.path, self.sd = os.fspath(path), sd
        self.regions, table = normalise_regions(regions)
        self.every, self.first = int(every), int(first)
        if self.every < 1 or self.first < 0 or not self.regions:
            raise ValueError("FieldWriter: at least one region, every >= 1, first >= 0")
        self.steps = []
        if resume_at is not None and os.path.exists(self.path):
            if not np.array_equal(np.asarray(h5io.read(self.path, "regions", h5io.I64)).reshape(-1, 9), table):
                raise ValueError(f"{self.path}: holds the frames of other regions")
            self.steps = [int(s) for s in np.asarray(h5io.read(self.path, "steps", h5io.I64)).reshape(-1) if s < resume_at]
        else:
            h5io.write(self.path, "regions", table, append=False)
        h5io.write(self.path, "steps", np.array(self.steps, dtype=np.int64))

    def take(self, obj, n):
        """the frame of step n -- or, where a slab is inside a blocked pass there, of the first step after it at which none is; -> that step"""
        shift = 0
        while True:
            try:
                frames = [obj.get_region(1, lo, hi, st) for lo, hi, st in self.regions]
                break
            except PfError as e:
                if e.code != 4 or n >= self.sd.Nt or shift >= MAX_SHIFT:  # (PF_ERR_STATE: inside a pass)
                    raise
            obj.run(n, 1)
            n += 1
            shift += 1
        for i, f in enumerate(frames):
            h5io.write(self.path, f"r{i:03d}_n{n:07d}", f.astype(np.float64) * self.sd.infac)
        self.steps = [s for s in self.steps if s != n] + [n]
        h5io.write(self.path, "steps", np.array(self.steps, dtype=np.int64))
        return n


def read(path):
    """-> (regions [R, 9], steps [F], {(i, step): frame}) of a file FieldWriter wrote"""
    regions = np.asarray(h5io.read(path, "regions", h5io.I64)).reshape(-1, 9)
    steps = [int(s) for s in np.asarray(h5io.read(path, "steps", h5io.I64)).reshape(-1)]
    return regions, steps, {(i, n): h5io.read(path, f"r{i:03d}_n{n:07d}", h5io.F64) for i in range(len(regions)) for n in steps}
