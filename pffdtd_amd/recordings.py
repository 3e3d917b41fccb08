"""Decimated field recordings: the impulse response of every cell of a plane or a box, low-pass filtered by a linear-phase FIR and kept at every
D-th step on the device as the run goes, in one HDF5 file -- what can be listened to, and what every other map of a seat is a function of.

    h, info = decimation_filter(Ts, factor, fpass_hz, atten_db=80)        a verified Kaiser design: nothing at or above the new Nyquist frequency
    fr = FieldRecording(path, sd, regions, factor, fpass_hz, atten_db=80, first=0, lowcut_hz=10, lowcut_order=4, dtype="f4")
    fr.take(obj, n)                              obj: a HipEngine or HipMulti that has taken the steps 0 .. n-1; n >= first: every such step is a sample
    fr.write()                                   what is complete so far, and the state a resumed run continues from
    frames, Fs_out, t0 = read(path, i)           region i: float [F, c0, c1, c2] at Fs_out = 1 / (factor Ts); frame m belongs to the time t0 + m / Fs_out
    FieldRecording(..., axes=[1, 2, 3], stencil="axis")                   B-format: W and one figure-of-eight channel per file axis, frames [F, 1 + A, c0, c1, c2]
    virtual_microphone(frames, axes, direction, pattern=0.5)             host numpy: a first-order microphone pointed anywhere, at every cell

A receiver per cell at the grid's rate is ten times or more oversampled against fmax; raw frames every D steps (fields.FieldWriter) fold everything
above the new Nyquist frequency into the band of interest.  Here every step is a sample: it runs through what ProcessOutputs.initial_process applies
to the receivers (decay.pre_sections: the integrator + low-cut as shared sections) and through the FIR, of which every factor-th output is kept
(engine.DecimatingRecorder, pf_engine_decim_*).  After the host-side low-pass and resampling that remain, a cell's frames are what ProcessOutputs
gives for a receiver in that cell, delayed by the FIR's (ntap - 1) / 2 samples: t0 = (first - delay) Ts.

Every step from `first` on is a sample (FieldRecording is a field_output.FieldOutput: the schedule, take and the rules of a resume are described
there).  Up to `cap` frames wait on the device; take() drains them into the file when they are `cap`.

The file holds
    regions  int64 [R, 9]      Ts  float64      sampling  int64 [4] = first, factor, count (samples so far), frames (complete so far)
    taps  float64 [ntap]      pre_sos  float64 [npre, 6]  (scipy's rows)      design  float64 [5] = fpass, atten, stop_db, ripple_db, delay
    frame_bytes  int64 = 4 or 8: the frames' dtype
    blocks  int64 [B]   the first frame of each block (multiples of cap; the last one may not be full yet), rewritten after each drain
    r{i:03d}_f{m0:07d}   [nf, c0, c1, c2] in `dtype`: the frames m0 .. m0 + nf - 1 of region i times infac (the factor SimData.rescale_output applies
                         to u_out), appended as drained
    r{i:03d}_acc  float64 [P, c0, c1, c2]   and   r{i:03d}_state  float64 [npre, 2, c0, c1, c2]: the outputs in flight and the sections' state, raw
write() drains, copies the file to a temporary name, puts sampling, blocks, acc and state there and moves it into place with os.replace.
With `axes` (1 .. 3 file axes, directional.parse_axes) one engine.VectorDecimatingRecorder per region (pf_engine_vdecim_*) keeps the cell and one
difference per axis -- the central difference, or with stencil="lattice" the lattice difference of an FCC grid -- through the sections
directional.gradient_sections gives, stacked as FieldDirectional stacks them (omni, then the gradient per axis): channel 0 is W, the pressure, channel
1 + a the pressure of a figure-of-eight microphone along file axis axes[a].  The stencil and fcc_flag rules are FieldDirectional's.  Such a file
additionally holds axes int64 [A], stencil int64, fcc_flag int64; pre_sos is [1 + A, npre, 6], a block [nf, 1 + A, c0, c1, c2], acc [1 + A, P, ...] and
state [1 + A, npre, 2, ...].  On a folded grid (fcc_flag 2) the file's frames of a y channel are negated in the odd cells -- exact, as directional.py
negates its odd-y products -- and r{i:03d}_iy int64 [c0, c1, c2] holds every cell's physical row; acc and state stay raw, in storage form.  Without
`axes` the file has exactly the datasets above and the scalar recorder runs.
With resume_at (the step a resumed run continues at) the file must match in regions, axes, stencil, Ts, first, factor, taps and pre_sos, and its count must be
the number of sample steps below resume_at; otherwise it is refused with the field's name.  Blocks at or beyond ceil(count / factor) are dropped.
"""
import os
import shutil

import numpy as np
from scipy.signal import firwin, freqz, kaiserord

from . import h5io
from .decay import pre_sections
from .directional import STENCILS, fold_coordinates, parse_axes, vector_setup, y_components
from .field_output import FieldOutput

MAX_SLOTS = 128  # P = ceil(ntap / factor): the outputs a recorder holds in flight (include/pffdtd_hip.h)
DTYPES = {"f4": np.float32, "f8": np.float64}


def decimation_filter(Ts, factor, fpass_hz, atten_db=80.0):
    """-> (h float64 [ntap], info): a linear-phase low-pass of odd length for decimation by `factor` at Fs = 1 / Ts, flat up to fpass_hz, at or below
    -atten_db at and above the new Nyquist frequency 1 / (2 factor Ts).  kaiserord and firwin, cutoff midway; the design is verified on 2^14 points
    of freqz and grows by two taps until it holds.  info: stop_db (the measured stopband maximum), ripple_db (the largest passband deviation up to
    fpass), delay = (ntap - 1) / 2 samples, and fpass, atten, factor, slots."""
    factor, fpass_hz, atten_db, Ts = int(factor), float(fpass_hz), float(atten_db), float(Ts)
    if factor < 2:
        raise ValueError(f"decimation_filter: factor: {factor} < 2, nothing to decimate")
    fs, nyq_new = 1.0 / Ts, 1.0 / (2.0 * factor * Ts)
    if not 0 < fpass_hz < nyq_new:
        raise ValueError(f"decimation_filter: fpass_hz: {fpass_hz:g} Hz is not below the new Nyquist frequency 1 / (2 factor Ts) = {nyq_new:g} Hz (and above 0)")
    if not atten_db > 0:
        raise ValueError(f"decimation_filter: atten_db: {atten_db:g} dB is not positive")
    ntap, beta = kaiserord(atten_db, (nyq_new - fpass_hz) / (0.5 * fs))
    ntap += 1 - ntap % 2
    while True:
        if -(-ntap // factor) > MAX_SLOTS:
            raise ValueError(f"decimation_filter: P: {ntap} taps at factor {factor} keep {-(-ntap // factor)} outputs in flight, a recorder holds {MAX_SLOTS}: "
                             f"take a smaller factor (a wider transition band up to its Nyquist frequency), or a lower fpass_hz or atten_db")
        h = firwin(ntap, 0.5 * (fpass_hz + nyq_new), window=("kaiser", beta), fs=fs)
        f, H = freqz(h, worN=1 << 14, fs=fs)
        mag = np.abs(H)
        stop = mag[f >= nyq_new].max()
        if stop <= 10.0 ** (-atten_db / 20.0):
            break
        ntap += 2
    ripple = np.abs(20.0 * np.log10(mag[f <= fpass_hz])).max()
    info = {"stop_db": float(20.0 * np.log10(stop)), "ripple_db": float(ripple), "delay": (ntap - 1) / 2.0, "fpass": fpass_hz, "atten": atten_db, "factor": factor,
            "slots": -(-ntap // factor)}
    return np.ascontiguousarray(h, dtype=np.float64), info


class FieldRecording(FieldOutput):
    label, noun, holds, observers_noun = "field recording", "recording", "frames", "recorders"
    recs = property(lambda self: self.observers)

    def __init__(self, path, sd, regions, factor, fpass_hz, atten_db=80.0, first=0, lowcut_hz=10.0, lowcut_order=4, dtype="f4", resume_at=None, cap=32, axes=None,
                 stencil="axis"):
        super().__init__(path, sd, regions, first)
        self.cap = int(cap)
        if self.first < 0 or not self.regions or self.cap < 1:
            raise ValueError("FieldRecording: at least one region, first >= 0, cap >= 1")
        if dtype not in DTYPES:
            raise ValueError(f"FieldRecording: dtype: '{dtype}' is not f4 or f8")
        self.dtype = DTYPES[dtype]
        self.taps, self.info = decimation_filter(self.Ts, factor, fpass_hz, atten_db)
        self.factor = int(factor)
        self.axes, self.stencil, self.fcc_flag, self.comp = None, stencil, int(getattr(sd, "fcc_flag", 0)), None
        if stencil not in STENCILS:
            raise ValueError(f"FieldRecording: stencil: {stencil!r} is neither \"axis\" nor \"lattice\"")
        if axes is None:
            if stencil != "axis":
                raise ValueError("FieldRecording: stencil: stencil=\"lattice\" chooses the difference of the channels `axes` asks for; without axes the pressure alone is recorded")
            self.pre_sos = pre_sections(self.Ts, bool(getattr(sd, "diff", False)), float(lowcut_hz), int(lowcut_order))
        else:  # W and one figure-of-eight channel per file axis: the components, and the sections per component as FieldDirectional stacks them
            self.axes, self.pre_sos, self.comp = vector_setup("FieldRecording", "vector decimating recorder", sd, axes, stencil, lowcut_hz, lowcut_order)
        self.blocks, self._part, self._part0 = [], [], 0
        self._resume(resume_at)

    # ---- the recorders ----
    def _frame_cells(self, r):
        """the shape of one frame of a recorder: its cells, with the channels in front where `axes` asks for them"""
        return r.cells if self.axes is None else (1 + self.axes.size,) + r.cells

    def _as_filed(self, i, fr):
        """frames as the file stores them: times infac, in `dtype`; on a folded grid a y channel negated in the odd cells (the stored +y of such a
        cell is the room's -y: exact)"""
        fr = fr * self.sd.infac
        if self.axes is not None and self.fcc_flag == 2:
            upper = fold_coordinates(self.regions[i], self.sd.Ny)[3]
            for k in y_components(self.comp):
                fr[:, k][..., upper] = -fr[:, k][..., upper]
        return fr.astype(self.dtype)

    def _observer(self, obj, lo, hi, st):
        if self.axes is None:
            return obj.decimating_recorder(lo, hi, st, pre_sos=self.pre_sos, taps=self.taps, factor=self.factor, cap=self.cap)
        return obj.vector_decimating_recorder(lo, hi, st, comp=self.comp, pre_sos=self.pre_sos, taps=self.taps, factor=self.factor, cap=self.cap)

    def _restore_observer(self, r, i, count, acc, state, nfull, part):
        r.set_state(acc[i], state[i], count)

    def attach(self, obj):
        """one decimating recorder per region on obj (a HipEngine or a HipMulti); a resumed run's outputs in flight and filter state go into them.
        A new run starts the file; a resumed one keeps the blocks below its first frame."""
        if self.recs is not None:
            return
        resumed = self._restore
        super().attach(obj)
        self._part = [np.zeros((0,) + self._frame_cells(r), dtype=self.dtype) for r in self.recs]  # the frames of the block that is not full yet, as the file stores them
        self._part0 = 0  # ... and its first frame
        if resumed is None:
            self._write_head(self.path, append=False)
            return
        nfull, part = resumed[3:]
        self.blocks, self._part0 = [k * self.cap for k in range(nfull)], nfull * self.cap
        if part is not None:
            self._part = [p.astype(self.dtype) for p in part]
        self._write_blocks(self.path, last=True)

    @property
    def frames(self):
        """frames complete so far"""
        return -(-self.count // self.factor)

    def _before_sample(self):
        """the frames on the device go to the file first when they are `cap`"""
        if self.recs[0].pending == self.cap:
            self.drain()

    def _sample(self, n):
        return ()

    def drain(self):
        """the complete frames of every region from the device; whole blocks of `cap` frames go to the file.  Blocks start at multiples of `cap`
        whenever they are drained, so a run stopped and resumed writes the blocks of the run in one piece."""
        for i, r in enumerate(self.recs):
            _, fr = r.read()
            if fr.shape[0]:
                self._part[i] = np.concatenate([self._part[i], self._as_filed(i, fr)])
        full = False
        while self._part[0].shape[0] >= self.cap:
            for i in range(len(self.recs)):
                h5io.write(self.path, f"r{i:03d}_f{self._part0:07d}", self._part[i][:self.cap])
                self._part[i] = self._part[i][self.cap:]
            self.blocks.append(self._part0)
            self._part0 += self.cap
            full = True
        if full:
            self._write_blocks(self.path)

    def _write_blocks(self, path, last=False):
        """last: the block that is not full yet is in the file too"""
        blocks = self.blocks + ([self._part0] if last and self._part[0].shape[0] else [])
        h5io.write(path, "blocks", np.array(blocks if blocks else [-1], dtype=np.int64))  # (no block yet: one row of -1)
        h5io.write(path, "nblocks", np.int64(len(blocks)))

    def _write_head(self, path, append=True):
        h5io.write(path, "regions", self.table, append=append)
        h5io.write(path, "Ts", np.float64(self.Ts))
        h5io.write(path, "sampling", np.array([self.first, self.factor, self.count, self.frames], dtype=np.int64))
        h5io.write(path, "taps", self.taps)
        h5io.write(path, "pre_sos", self.pre_sos if self.pre_sos.size else np.zeros((1, 6)))  # (no section: one row of zeros)
        h5io.write(path, "npre", np.int64(self.pre_sos.shape[-2]))
        if self.axes is not None:
            h5io.write(path, "axes", self.axes)
            h5io.write(path, "stencil", np.int64(STENCILS.index(self.stencil)))
            h5io.write(path, "fcc_flag", np.int64(self.fcc_flag))
            if self.fcc_flag == 2:
                for i, r in enumerate(self.regions):
                    h5io.write(path, f"r{i:03d}_iy", np.ascontiguousarray(fold_coordinates(r, self.sd.Ny)[1], dtype=np.int64))
        h5io.write(path, "frame_bytes", np.int64(np.dtype(self.dtype).itemsize))
        h5io.write(path, "design", np.array([self.info[k] for k in ("fpass", "atten", "stop_db", "ripple_db", "delay")], dtype=np.float64))
        self._write_blocks(path)

    def _write_region(self, path, i, r):
        if self._part[i].shape[0]:
            h5io.write(path, f"r{i:03d}_f{self._part0:07d}", self._part[i])
        acc, state = r.get_state()
        h5io.write(path, f"r{i:03d}_acc", acc)
        if state.size:
            h5io.write(path, f"r{i:03d}_state", state)

    def write(self):
        """the file as it stands: every complete frame, and the outputs in flight and filter state a resumed run continues from.  The blocks are in
        the file already: it is copied, not written anew"""
        self._attached("write")
        self.drain()
        tmp = self.path + ".tmp"
        shutil.copyfile(self.path, tmp)
        self._write_head(tmp)
        self._write_blocks(tmp, last=True)
        for i, r in enumerate(self.recs):
            self._write_region(tmp, i, r)
        os.replace(tmp, self.path)

    # ---- the file of a resumed run ----
    def _read_file(self):
        return read_file(self.path, raw=True)

    def _checks(self, f):
        theirs, mine = h5io._CODE_TO_NP[f["frame_code"]], self.dtype
        return [("axes", (f["axes"] is None) == (self.axes is None) and (self.axes is None or np.array_equal(f["axes"], self.axes)),
                 f"the file holds the channels of axes {None if f['axes'] is None else f['axes'].tolist()}, {None if self.axes is None else self.axes.tolist()} asked for"),
                ("stencil", f["stencil"] == self.stencil, f"the file holds the frames of stencil=\"{f['stencil']}\", \"{self.stencil}\" is asked for"),
                *self._same_clock(f), self._asked("factor", f["sampling"][1], self.factor),
                ("taps", np.array_equal(f["taps"], self.taps), "the file's frames went through another low-pass (fpass, atten)"),
                ("dtype", theirs == mine, f"the file's frames are {np.dtype(theirs).name}, {np.dtype(mine).name} asked for"),
                ("pre_sos", np.array_equal(f["pre_sos"], self.pre_sos), "the file's frames went through other sections (low-cut, integrator, grid spacing)")]

    def _saved(self, f, count):
        """(count, [acc per region], [state per region], the number of full blocks, [the frames of the block not full yet per region] or None)"""
        done = -(-count // self.factor)  # frames complete at the resumed step; blocks at or beyond it are a later run's
        nfull, have = done // self.cap, [int(b) for b in f["blocks"] if b < done]
        if have != [k * self.cap for k in range(-(-done // self.cap))]:
            raise ValueError(f"{self.path}: blocks: the file's blocks {have} are not those of {done} frames in blocks of cap = {self.cap}")
        part = None
        if done > nfull * self.cap:
            part = [np.asarray(h5io.read(self.path, f"r{i:03d}_f{nfull * self.cap:07d}", f["frame_code"]))[:done - nfull * self.cap] for i in range(len(self.regions))]
            if any(p.shape[0] != done - nfull * self.cap for p in part):
                raise ValueError(f"{self.path}: blocks: the block at frame {nfull * self.cap} holds fewer than {done - nfull * self.cap} frames")
        return count, f["acc"], f["state"], nfull, part


def read_file(path, raw=False):
    """-> dict(regions [R, 9], Ts, sampling [first, factor, count, frames], taps, pre_sos [npre, 6], design [5], blocks [B], axes None, stencil "axis",
    fcc_flag 0; raw: also acc and state per region, state None without sections) of a file FieldRecording wrote.  A file written with `axes`: axes
    int64 [A], stencil "axis" / "lattice", fcc_flag, pre_sos [1 + A, npre, 6], and -- fcc_flag 2 -- iy, per region int64 [c0, c1, c2]"""
    regions = np.asarray(h5io.read(path, "regions", h5io.I64)).reshape(-1, 9)
    npre, nblocks = int(h5io.read(path, "npre", h5io.I64)), int(h5io.read(path, "nblocks", h5io.I64))
    axes = np.asarray(h5io.read(path, "axes", h5io.I64)).reshape(-1) if h5io.exists(path, "axes") else None
    pre = np.asarray(h5io.read(path, "pre_sos", h5io.F64))
    out = {"regions": regions, "Ts": float(h5io.read(path, "Ts", h5io.F64)), "sampling": np.asarray(h5io.read(path, "sampling", h5io.I64)).reshape(4),
           "taps": np.asarray(h5io.read(path, "taps", h5io.F64)).reshape(-1), "pre_sos": pre.reshape(-1, 6)[:npre] if axes is None else pre.reshape(1 + axes.size, -1, 6),
           "axes": axes, "stencil": STENCILS[int(h5io.read(path, "stencil", h5io.I64))] if axes is not None else "axis",
           "fcc_flag": int(h5io.read(path, "fcc_flag", h5io.I64)) if axes is not None else 0,
           "design": np.asarray(h5io.read(path, "design", h5io.F64)).reshape(5), "blocks": np.asarray(h5io.read(path, "blocks", h5io.I64)).reshape(-1)[:nblocks],
           "frame_code": h5io.F32 if int(h5io.read(path, "frame_bytes", h5io.I64)) == 4 else h5io.F64}
    if raw:
        out["acc"] = [np.asarray(h5io.read(path, f"r{i:03d}_acc", h5io.F64)) for i in range(len(regions))]
        out["state"] = [np.asarray(h5io.read(path, f"r{i:03d}_state", h5io.F64)) if npre else None for i in range(len(regions))]
    if out["fcc_flag"] == 2:
        out["iy"] = [np.asarray(h5io.read(path, f"r{i:03d}_iy", h5io.I64)) for i in range(len(regions))]
    return out


def read(path, i):
    """-> (frames [F, c0, c1, c2] of region i -- [F, 1 + A, c0, c1, c2] of a file written with `axes`: W, then the figure-of-eight channel per axis --,
    the blocks concatenated; Fs_out = 1 / (factor Ts); t0 = (first - delay) Ts, the time of frame 0)"""
    f = read_file(path)
    first, factor = int(f["sampling"][0]), int(f["sampling"][1])
    parts = [np.asarray(h5io.read(path, f"r{i:03d}_f{int(m0):07d}", f["frame_code"])) for m0 in f["blocks"]]
    at = int(f["blocks"][0]) if parts else 0
    for m0, p in zip(f["blocks"], parts):
        if int(m0) != at:
            raise ValueError(f"{path}: blocks: block {int(m0)} of region {i} does not follow frame {at - 1}")
        at += p.shape[0]
    counts = tuple(int(-(-(hi - lo) // st)) for lo, hi, st in zip(f["regions"][i, 0:3], f["regions"][i, 3:6], f["regions"][i, 6:9]))
    if f["axes"] is not None:
        counts = (1 + f["axes"].size,) + counts
    frames = np.concatenate(parts) if parts else np.zeros((0,) + counts, dtype=h5io._CODE_TO_NP[f["frame_code"]])
    return frames, 1.0 / (factor * f["Ts"]), (first - f["design"][4]) * f["Ts"]


def virtual_microphone(frames, axes, direction, pattern=0.5):
    """frames [F, 1 + A, ...] as read() gives them for a file written with `axes` (1 / 2 / 3 = file x / y / z, in the file's order), direction: a unit
    vector in file axes -> [F, ...]: pattern * W + (1 - pattern) * sum_a d_a V_a, the signal of a first-order microphone pointed along `direction`
    at every cell.  pattern 1: omni, 0.5: cardioid, 0: figure-of-eight.  A direction with a component along an axis that was not recorded is refused
    by name."""
    frames = np.asarray(frames)
    axes = [int(a) for a in np.asarray(axes).reshape(-1)]
    d = np.asarray(direction, dtype=np.float64).reshape(-1)
    if frames.ndim < 2 or frames.shape[1] != 1 + len(axes):
        raise ValueError(f"virtual_microphone: frames: shape {frames.shape} is not [F, 1 + {len(axes)}, ...] for axes {axes}")
    if d.size != 3 or not np.isfinite(d).all() or abs(float(np.sqrt((d * d).sum())) - 1.0) > 1e-9:
        raise ValueError(f"virtual_microphone: direction: {d.tolist()} is not a unit vector (x, y, z) in file axes")
    if not 0.0 <= float(pattern) <= 1.0:
        raise ValueError(f"virtual_microphone: pattern: {pattern} outside 0 (figure-of-eight) .. 1 (omni)")
    for a in (1, 2, 3):
        if a not in axes and d[a - 1] != 0.0:
            raise ValueError(f"virtual_microphone: direction: a component {d[a - 1]:g} along file {'xyz'[a - 1]}, but axis {a} was not recorded (axes {axes})")
    out = float(pattern) * frames[:, 0].astype(np.float64)
    for k, a in enumerate(axes):
        out = out + (1.0 - float(pattern)) * d[a - 1] * frames[:, 1 + k]
    return out


def add_arguments(p):
    """the --rec-* arguments of the command line"""
    p.add_argument("--rec-planes", action="append", default=[], metavar="x=I,y=J,z=K", help="record the low-pass filtered, decimated field of these planes on the device (the syntax of --field-planes)")
    p.add_argument("--rec-box", action="append", default=[], metavar="x0:x1:sx,y0:y1:sy,z0:z1:sz", help="... of this strided box")
    p.add_argument("--rec-factor", type=int, default=0, metavar="D", help="... keeping every D-th output of the low-pass (2 .. 64)")
    p.add_argument("--rec-fpass", type=float, default=0.0, metavar="HZ", help="... which is flat up to HZ, below the new Nyquist frequency 1 / (2 D Ts)")
    p.add_argument("--rec-atten", type=float, default=80.0, metavar="DB", help="... and DB decibels down from that frequency on (default 80)")
    p.add_argument("--rec-first", type=int, default=0, metavar="N", help="... at every step from N on (default 0)")
    p.add_argument("--rec-dtype", choices=sorted(DTYPES), default="f4", help="... stored as float32 (f4, the default) or float64 (f8)")
    p.add_argument("--rec-file", default="", metavar="FILE", help="... into this HDF5 file (default: sim_recordings.h5 in the data folder)")
    p.add_argument("--rec-axes", default="", metavar="x,y,z", help="... as a B-format impulse response: W and a figure-of-eight channel along each of these file axes (one to three)")
    p.add_argument("--rec-stencil", choices=STENCILS, default="axis", help="... from the central difference along the axis (Cartesian grids, the default) or the lattice difference (FCC grids)")


def check_arguments(p, a):
    """a.rec: are recordings asked for?  --rec-* without a region, and a region without --rec-factor / --rec-fpass, are refused both ways round"""
    a.rec = bool(a.rec_planes or a.rec_box)
    if a.rec != bool(a.rec_factor) or a.rec != bool(a.rec_fpass) or a.rec_first < 0 or a.rec_atten <= 0:
        p.error("--rec-planes / --rec-box need --rec-factor and --rec-fpass (and the other way round); --rec-atten: positive, --rec-first: not negative")
    if (a.rec_first or a.rec_file or a.rec_atten != 80.0 or a.rec_dtype != "f4" or a.rec_axes or a.rec_stencil != "axis") and not a.rec:
        p.error("--rec-atten / --rec-first / --rec-dtype / --rec-file / --rec-axes / --rec-stencil need --rec-planes or --rec-box")
    if a.rec_stencil != "axis" and not a.rec_axes:
        p.error("--rec-stencil chooses the difference of the channels --rec-axes asks for: it needs --rec-axes")
    if a.rec_axes:
        try:
            parse_axes(a.rec_axes)
        except ValueError as e:
            p.error(str(e).replace("--dir-axes", "--rec-axes"))
