"""Drop-in for the reference binaries `fdtd_main_{cpu,gpu}_{single,double}.x` (c_cuda/fdtd_main.c:35-59).

    cd <sim_data folder> && python -m pffdtd_amd.fdtd_main --precision single [--gpus N]

Same flow: load_sim_data -> scale_input -> run_sim -> rescale_output -> write_outputs -> print_last_samples,
reading the four input .h5 files from the current directory and writing sim_outs.h5 there.

`--gpus N` is the counterpart of the reference GPU binary driving every visible device from one process
(gpu_engine.h:680-690, 993-1145): ONE process, the C library's chain object (pf_multi_*, csrc/pf_multi.hip: the grid cut
into Z-slabs like gpu_engine.h:516-662, one host thread per slab, ghost planes by peer copies or native RCCL on the edge
stream) on devices 0 .. N-1 -- round 4: the one N > 1 driver of the product.  `--devices 0,1,2,3` names the chain
explicitly; a device id may repeat (several slabs on one GPU).  Unlike the reference (gpu_engine.h:688) the lists need
not be sorted: the slabs are cut by plane tests and every engine sorts its own lists.

Under an external launcher (`python -m torch.distributed.run --nproc-per-node N -m pffdtd_amd.fdtd_main ...`: one process
per GPU, WORLD_SIZE set) each rank cuts its own slab (`pffdtd_amd/slab.py`), steps it with the split-phase engine and
exchanges over RCCL through torch.distributed; rank 0 gathers the receiver rows and writes `sim_outs.h5`.

`--progress [K]` prints the reference's progress fields (fdtd_common.h:106-190: T / I / TPW / IPW / TA / IA / TB / IB Mvox/s
and the air share, "I" = over the last K steps, default 200) as one plain line per report -- the reference redraws six
lines per STEP, which would cost a device synchronisation per step here.

Checkpoint and resume (no counterpart in the reference, whose run_steps is re-entrant in memory only): `--checkpoint FILE` names a
checkpoint file (pffdtd_amd/checkpoint.py), written every `--checkpoint-every K` steps and when `--stop-after N` ends the run after
its first N steps (steps 0 .. N-1; exit status 0, no sim_outs.h5); `--resume FILE` continues from such a file and produces the
sim_outs.h5 of a run in one piece, bit for bit.  A chain whose slabs step in blocked pairs or triples can only be saved between
passes: the checkpoint is then taken up to five steps later, at the first step every slab's pass has ended (the file records its step).
One process with one device or a chain of them; the one-process-per-GPU launcher refuses these arguments.

Field frames (the data behind the reference's `--plot`, without the plotting): `--field-planes x=I,y=J,z=K` (any subset, an axis may
repeat) and `--field-box x0:x1:sx,y0:y1:sy,z0:z1:sz` name regions of the grid in FILE coordinates, `--field-every K` records them at the
steps `--field-first N` (default 0), N + K, ... into `--field-file FILE` (default sim_fields.h5 beside sim_outs.h5; pffdtd_amd/fields.py
describes the file).  The run is cut at the frame steps exactly as at checkpoint steps, and a chain inside a blocked pass takes the frame
up to five steps later, recording where.  With `--resume` the file is appended to and the frames before the resumed step are kept.
Same processes as the checkpoint arguments; without these arguments nothing about a run changes.

Field spectra (pffdtd_amd/spectra.py): `--spectrum-planes` / `--spectrum-box` (the syntax of the field arguments) name regions whose cells' DFT at
`--spectrum-freqs 63,125,250` (or `lo:hi:n`, linearly spaced) is summed ON THE DEVICE over the steps `--spectrum-first N` (default 0), N + K, ...
(`--spectrum-every K`, default 1: every step), optionally under `--spectrum-window hann`, and written to `--spectrum-file FILE` (default
sim_spectra.h5 beside sim_outs.h5) at every checkpoint and at the end.  The run is cut at the sample steps exactly as at frame and checkpoint
steps; a sample is never taken at another step than its own, so a chain is created with PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES (one line says
so).  `--resume` restores the sums from the file.  Same processes as the checkpoint arguments; without these arguments nothing about a run changes.

Energy decay maps (pffdtd_amd/decay.py): `--decay-planes` / `--decay-box` (the syntax of the field arguments) name regions whose cells' pressure is
filtered into the octave bands `--decay-bands 125,250,500` (centre frequencies in Hz), squared and summed ON THE DEVICE into time bins of
`--decay-bin-ms 5` milliseconds, at EVERY step from `--decay-first N` (default 0) on, and written to `--decay-file FILE` (default sim_decay.h5
beside sim_outs.h5) at every checkpoint and at the end.  The run is cut at every step from N on; a chain is created with
PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES (one line says so).  `--resume` restores sums and filter state from the file.  Same processes as the
checkpoint arguments; without these arguments nothing about a run changes.  (`--energy` is not a name of these: it stays the diagnostic's.)

Directional band maps (pffdtd_amd/directional.py): `--dir-planes` / `--dir-box` (the syntax of the field arguments; one cell clear of the faces along
every chosen axis) name regions whose cells' pressure and pressure gradient along `--dir-axes y[,x,z]` (file axes; default y) are filtered into the
octave bands `--dir-bands 125,250,500`, multiplied and summed ON THE DEVICE into time bins of `--dir-bin-ms 5` milliseconds, at EVERY step from
`--dir-first N` (default 0) on, and written to `--dir-file FILE` (default sim_directional.h5 beside sim_outs.h5) at every checkpoint and at the end:
what the lateral energy fractions LF, LFC and the intensity maps are functions of (directional.parameters).  `--dir-stencil axis` (default) is the
central difference along the axis, on Cartesian grids only; `--dir-stencil lattice` is the FCC lattice's own difference over the eight neighbours at
+-1 along the axis, on FCC folders only (fcc_flag 1 / 2; regions one cell clear of ALL faces; on a folded grid the file carries every cell's
physical y index and S has the room's sign).  The wrong stencil for the folder's grid is refused by name.  Everything else as the decay arguments: the run is cut at every step from N on, a chain is created with PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES (one line says
so), `--resume` restores sums and filter state from the file, and without these arguments nothing about a run changes.

Decimated field recordings (pffdtd_amd/recordings.py): `--rec-planes` / `--rec-box` (the syntax of the field arguments) name regions whose cells'
pressure is low-pass filtered ON THE DEVICE at EVERY step from `--rec-first N` (default 0) on by a verified linear-phase FIR -- flat up to
`--rec-fpass HZ`, `--rec-atten 80` dB down from the new Nyquist frequency on -- and kept at every `--rec-factor D`-th step: the impulse response of
every cell at the rate 1 / (D Ts), not aliased, in `--rec-dtype f4|f8`, appended to `--rec-file FILE` (default sim_recordings.h5 beside sim_outs.h5)
as the run goes and completed at every checkpoint and at the end.  Everything else as the decay arguments: the run is cut at every step from N on,
a chain is created with PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES (one line says so), `--resume` restores the outputs in flight and the filter state
from the file, and without these arguments nothing about a run changes.  `--rec-axes x,y,z` (one to three file axes) records the B-format impulse
response instead: channel 0 is W, the pressure, and one channel per axis is the pressure of a figure-of-eight microphone along it, from the
difference `--rec-stencil axis|lattice` names (the rules of `--dir-stencil`; regions one cell clear of the faces the difference reads); frames are
[F, 1 + A, c0, c1, c2], and recordings.virtual_microphone points a first-order microphone anywhere at every cell.  Without `--rec-axes` the file is
the pressure's, as before.

Wall absorption maps (pffdtd_amd/absorption.py): `--absorption` sums ON THE DEVICE, at EVERY step from `--absorption-first N` (default 0) on, the energy the
step loses per frequency-dependent wall node, per material and at the open boundary, and the energy the sources put in, into time bins of
`--absorption-bin-ms 5` milliseconds, and writes them to sim_absorption.h5 beside sim_outs.h5 at every checkpoint and at the end: which surface takes
the energy out of the room.  It names no regions -- it reads the walls -- and is broadband.  Everything else as the decay arguments: the run is cut at
every step from N on, a chain is created with PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES (one line says so), `--resume` restores the sums from the file and,
on one domain, gives the file of a run in one piece byte for byte (a chain of slabs: the node sums bit for bit, the bins to rounding -- the file keeps
the scene's bins, not each slab's), and without these arguments nothing about a run changes.
"""
import argparse
import os
import time
from pathlib import Path
from types import ModuleType
from typing import Callable, NamedTuple

from . import checkpoint, engine, fields, sim_data, spectra
from . import absorption as absorb_mod
from . import decay as decay_mod
from . import directional as dir_mod
from . import recordings as rec_mod


def _summary(sd, tm, el):
    t_air = tm["air_ms_total"] * 1e-3
    t_rest = max(tm["step_ms_total"] * 1e-3 - t_air, 0.0)
    # the reference's three summary lines (cpu_engine.h:355-357 / gpu_engine.h:1251-1253), HIP-event timed
    print(f"Air update: {t_air:.6f}s, {sd.Npts * sd.Nt / 1e6 / max(t_air, 1e-12):.2f} Mvox/s")
    print(f"Boundary loop: {t_rest:.6f}s, {sd.Nb * sd.Nt / 1e6 / max(t_rest, 1e-12):.2f} Mvox/s")
    print(f"Combined (total): {el:.6f}s, {sd.Npts * sd.Nt / 1e6 / el:.2f} Mvox/s")


def _finish(sd, data_dir):
    sd.rescale_output()
    sd.write_outputs(data_dir)
    print("wrote output dataset")
    sd.print_last_samples(5)
    print(f"--Date and time: {time.ctime()}")


def _progress(sd, n, nt, t_all, t_chunk, k, air_all, air_chunk, bn_all, bn_chunk, workers):
    """one report in the reference's vocabulary (fdtd_common.h:106-190)"""
    def hms(sec):
        sec = int(sec)
        return f"{sec // 3600:02d}:{sec % 3600 // 60:02d}:{sec % 60:02d}"
    mv = lambda cells, t: 1e-6 * cells / max(t, 1e-12)
    print(f"Running [{100.0 * n / nt:.1f}%] [{hms(t_all)}<{hms(t_all * nt / max(n, 1))}] "
          f"T: {mv(sd.Npts * n, t_all):06.1f} - I: {mv(sd.Npts * k, t_chunk):06.1f} | "
          f"TPW: {mv(sd.Npts * n, t_all) / workers:06.1f} - IPW: {mv(sd.Npts * k, t_chunk) / workers:06.1f} | "
          f"TA: {mv(sd.Npts * n, air_all):06.1f} - IA: {mv(sd.Npts * k, air_chunk):06.1f} | "
          f"TB: {mv(sd.Nb * n, bn_all):06.1f} - IB: {mv(sd.Nb * k, bn_chunk):06.1f} | "
          f"T: {100.0 * air_all / max(t_all, 1e-12):02.1f}% - I: {100.0 * air_chunk / max(t_chunk, 1e-12):02.1f}%", flush=True)


def _save_checkpoint(a, sd, m, n):
    """the checkpoint at step n -- or, where a slab is inside a blocked pass there, at the first step after it at which none is; -> that step"""
    while True:
        try:
            state = m.save_state()
            break
        except engine.PfError as e:
            if e.code != 4 or n >= sd.Nt:  # (PF_ERR_STATE: inside a pass)
                raise
        m.run(n, 1)
        n += 1
    checkpoint.write(a.checkpoint, sd, n, state)
    print(f"--checkpoint at step {n} of {sd.Nt}: {a.checkpoint}", flush=True)
    return n


def _run_chain(a, sd, m):
    """all Nt steps of a chain object, in one go or in chunks with progress reports; returns (seconds, timing of the busiest slab).
    With --resume / --checkpoint / --stop-after: from the resumed step, to the step the run stops after (a.stopped_at: less than Nt then)."""
    live = range(m.nslabs)
    if a.resume or a.checkpoint or a.field_every or any(getattr(a, kind.flag, False) for kind in KINDS):
        return _run_chain_checkpointed(a, sd, m)
    t0 = time.perf_counter()
    if not a.progress:
        m.run(0, sd.Nt)
        el = time.perf_counter() - t0
        tms = [m.slab(g)["engine"].timing() for g in live]
        return el, {"air_ms_total": max(t["air_ms_total"] for t in tms), "step_ms_total": max(t["step_ms_total"] for t in tms)}
    air_all = step_all = 0.0
    n = 0
    while n < sd.Nt:
        k = min(a.progress, sd.Nt - n)
        tc = time.perf_counter()
        m.run(n, k)
        now = time.perf_counter()
        n += k
        tms = [m.slab(g)["engine"].timing(reset=True) for g in live]
        air = max(t["air_ms_total"] for t in tms) * 1e-3
        step = max(t["step_ms_total"] for t in tms) * 1e-3
        if step <= 0:
            step = now - tc  # (slab engines time their interior launches only)
        air_all += air
        step_all += step
        _progress(sd, n, sd.Nt, now - t0, now - tc, k, air_all, air, max(step_all - air_all, 1e-12), max(step - air, 1e-12), m.nslabs)
    return time.perf_counter() - t0, {"air_ms_total": air_all * 1e3, "step_ms_total": step_all * 1e3}


def _field_writer(a, sd, resume_at):
    """the FieldWriter of --field-planes / --field-box (None without them)"""
    if not a.field_every:
        return None
    N = (sd.Nx, sd.Ny, sd.Nz)
    try:
        regions = [r for spec in a.field_planes for r in fields.parse_planes(spec, N)] + [fields.parse_box(spec, N) for spec in a.field_box]
        path = a.field_file if a.field_file else Path(a.data_dir) / "sim_fields.h5"
        return fields.FieldWriter(path, sd, regions, a.field_every, a.field_first, resume_at=resume_at)
    except ValueError as e:
        raise SystemExit(str(e))


class _Kind(NamedTuple):
    """one kind of field output that is summed or filtered on the device, as the command line sees it"""
    name: str  # in the lines of standard output: "--field <name> ..."
    prefix: str  # of its arguments: --<prefix>-planes, --<prefix>-box, --<prefix>-file
    flag: str  # a.<flag>, set by its module's check_arguments: is it asked for?
    module: ModuleType  # add_arguments, check_arguments
    file: str  # the default file name, beside sim_outs.h5
    build: Callable  # (a, sd, regions, path, resume_at) -> the output
    reword: tuple  # (old, new) applied to a ValueError's text after "--field-" has become "--<prefix>-"
    attach_names_regions: bool  # a PfError of attach is a refusal of the regions: it exits as "--<prefix>-planes / --<prefix>-box: ..."
    sampled: str  # why its chain takes single steps (_chain_flags)
    done: Callable  # the output -> the end-of-run line between "--field " and ": <path>"
    asked_by: str = ""  # the arguments that ask for it, in refusals (default: --<prefix>-planes / --<prefix>-box)

    def names(self):
        return self.asked_by or f"--{self.prefix}-planes / --{self.prefix}-box"


def _stencil_words(prefix):
    return (('stencil="lattice"', f"--{prefix}-stencil lattice"), ('stencil="axis"', f"--{prefix}-stencil axis"))


KINDS = (  # in the order they are built, sampled within a step, written and reported
    _Kind("spectrum", "spectrum", "spectrum", spectra, "sim_spectra.h5",
          lambda a, sd, regions, path, resume_at: spectra.FieldSpectrum(path, sd, regions, spectra.parse_freqs(a.spectrum_freqs), a.spectrum_every, a.spectrum_first,
                                                                        a.spectrum_window, resume_at=resume_at),
          (), False, "every sample step can be sampled", lambda o: f"spectrum of {o.count} samples at {o.freqs.size} frequencies"),
    _Kind("decay", "decay", "decay", decay_mod, "sim_decay.h5",
          lambda a, sd, regions, path, resume_at: decay_mod.FieldDecay(path, sd, regions, decay_mod.parse_bands(a.decay_bands), a.decay_bin_ms, a.decay_first, resume_at=resume_at),
          (), False, "every step is sampled", lambda o: f"decay of {o.count} samples in {o.bands.size} bands, bins of {o.bin_steps} steps"),
    _Kind("directional", "dir", "directional", dir_mod, "sim_directional.h5",
          lambda a, sd, regions, path, resume_at: dir_mod.FieldDirectional(path, sd, regions, decay_mod.parse_bands(a.dir_bands), dir_mod.parse_axes(a.dir_axes), a.dir_bin_ms,
                                                                           a.dir_first, resume_at=resume_at, stencil=a.dir_stencil),
          (("--decay-", "--dir-"),) + _stencil_words("dir"), True, "every step is sampled",  # (attach: a region on a face along a chosen axis, an FCC grid: the engine names it)
          lambda o: f"directional maps of {o.count} samples in {o.bands.size} bands along {','.join('xyz'[k - 1] for k in o.axes)}"
                    f"{' (lattice differences)' if o.stencil == 'lattice' else ''}, bins of {o.bin_steps} steps"),
    _Kind("recording", "rec", "rec", rec_mod, "sim_recordings.h5",
          lambda a, sd, regions, path, resume_at: rec_mod.FieldRecording(path, sd, regions, a.rec_factor, a.rec_fpass, a.rec_atten, a.rec_first, dtype=a.rec_dtype, resume_at=resume_at,
                                                                         axes=dir_mod.parse_axes(a.rec_axes) if a.rec_axes else None, stencil=a.rec_stencil),
          (("--dir-", "--rec-"),) + _stencil_words("rec"), True, "every step is sampled",  # (attach: a factor or a tap count the engine refuses, a region on a face along a recorded axis)
          lambda o: f"recording of {o.count} samples, {o.frames} frames at every {o.factor}th step through {o.taps.size} taps"
                    + ("" if o.axes is None else f", channels W {' '.join('XYZ'[k - 1] for k in o.axes.tolist())} ({o.stencil} differences)")),
    _Kind("absorption", "absorption", "absorption", absorb_mod, "sim_absorption.h5",  # (no regions: it reads the walls)
          lambda a, sd, regions, path, resume_at: absorb_mod.WallAbsorption(path, sd, a.absorption_bin_ms, a.absorption_first, resume_at=resume_at),
          (), False, "every step is sampled", lambda o: f"wall absorption of {o.count} steps, {int(o.Nm)} materials, bins of {o.bin_steps} steps", "--absorption"),
)


def _field_output(kind, a, sd, m, resume_at):
    """the output of `kind` on chain m, attached; a resumed run's state is restored from its file"""
    N = (sd.Nx, sd.Ny, sd.Nz)
    try:
        regions = ([r for spec in getattr(a, kind.prefix + "_planes", ()) for r in fields.parse_planes(spec, N)]
                   + [fields.parse_box(spec, N) for spec in getattr(a, kind.prefix + "_box", ())])
        path = getattr(a, kind.prefix + "_file", "") or Path(a.data_dir) / kind.file
        out = kind.build(a, sd, regions, path, resume_at)
    except ValueError as e:
        text = str(e).replace("--field-", f"--{kind.prefix}-")
        for old, new in kind.reword:
            text = text.replace(old, new)
        raise SystemExit(text)
    try:
        out.attach(m)
    except engine.PfError as e:
        if not kind.attach_names_regions:
            raise
        raise SystemExit(f"{kind.names()}: {e}")
    return out


def _chain_flags(a, nslabs):
    """multi_flags of the chain: sampled by a field output of KINDS, no slab steps in pairs or triples (a sample is never shifted, and no slab
    answers inside a pass)"""
    asked = [kind for kind in KINDS if getattr(a, kind.flag, False)]
    if not asked or nslabs < 2:
        return 0
    for kind in reversed(asked):
        print(f"--field {kind.name}: the chain is created with PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES (its slabs take single steps: {kind.sampled})")
    return engine.PF_MULTI_NO_PAIRS | engine.PF_MULTI_NO_TRIPLES


def _run_chain_checkpointed(a, sd, m):
    """the run cut at checkpoint steps, at frame steps (--field-every) and at the sample steps of every field output of KINDS"""
    live = range(m.nslabs)
    n = 0
    if a.resume:
        try:
            n, state, u_out = checkpoint.read(a.resume, sd)
        except (checkpoint.CheckpointMismatch, KeyError, IOError) as e:
            raise SystemExit(f"cannot resume: {e}")
        sd.u_out[...] = u_out  # (in place: the library writes into this array)
        m.load_state(state)
        print(f"--resumed at step {n} of {sd.Nt}: {a.resume}", flush=True)
    fw = _field_writer(a, sd, n if a.resume else None)
    outs = [(kind, _field_output(kind, a, sd, m, n if a.resume else None)) for kind in KINDS if getattr(a, kind.flag, False)]
    cuts = ([fw] if fw else []) + [out for _, out in outs]  # the run is cut at the next step of each of these
    end = sd.Nt if a.stop_after is None else min(max(a.stop_after, n), sd.Nt)
    every = a.checkpoint_every if a.checkpoint else 0
    t0 = time.perf_counter()
    air_all = step_all = 0.0
    if fw and fw.due(n) and n < end:  # (the frame of the first step: before any step of this run)
        n = fw.take(m, n)
        print(f"--field frame at step {n} of {sd.Nt}: {fw.path}", flush=True)
    for _, out in outs:  # (a step's sample belongs to the run that takes the step: a stopped run leaves the sample of its last step to the resumed one)
        if out.due(n) and n < end:
            out.take(m, n)
    while n < end:
        k = end - n
        if a.progress:
            k = min(k, a.progress)
        if every:
            k = min(k, every - n % every)
        for out in cuts:
            k = min(k, out.next_step(n + 1) - n)
        tc = time.perf_counter()
        m.run(n, k)
        n += k
        save = a.checkpoint and n < sd.Nt and ((every and n % every == 0) or n == end)
        if fw and fw.due(n):
            n = fw.take(m, n)
            print(f"--field frame at step {n} of {sd.Nt}: {fw.path}", flush=True)
            end = max(end, n)
        if save:
            n = _save_checkpoint(a, sd, m, n)
            end = max(end, n)
            for _, out in outs:
                out.settle(m, n)
                out.write()  # (the output of the sample steps below n: what --resume of this checkpoint continues)
        for _, out in outs:
            if out.due(n) and n < end:
                out.take(m, n)
        now = time.perf_counter()
        tms = [m.slab(g)["engine"].timing(reset=True) for g in live]
        air = max(t["air_ms_total"] for t in tms) * 1e-3
        step = max(t["step_ms_total"] for t in tms) * 1e-3
        if step <= 0:
            step = now - tc
        air_all += air
        step_all += step
        if a.progress:
            _progress(sd, n, sd.Nt, now - t0, now - tc, k, air_all, air, max(step_all - air_all, 1e-12), max(step - air, 1e-12), m.nslabs)
    a.stopped_at = n
    for kind, out in outs:
        out.settle(m, n)
        out.write()
        print(f"--field {kind.done(out)}: {out.path}", flush=True)
        out.close()
    return time.perf_counter() - t0, {"air_ms_total": air_all * 1e3, "step_ms_total": step_all * 1e3}


def _stopped_early(a, sd):
    """--stop-after ended the run before Nt: the checkpoint is the result, no sim_outs.h5"""
    n = getattr(a, "stopped_at", sd.Nt)
    if n >= sd.Nt:
        return False
    print(f"--stopped after {n} of {sd.Nt} steps; continue with --resume {a.checkpoint}")
    print(f"--Date and time: {time.ctime()}")
    return True


def run_single(a):
    """One device.  Rooms (scenes the library stores with the x and z axes exchanged) run as TWO slabs on it, like pf_run_sim:
    the halves' kernels overlap (CTK church 313 against 288 Gvox/s); box rooms as one domain."""
    print(f"--Date and time: {time.ctime()}")
    sd = sim_data.SimData.from_folder(Path(a.data_dir), a.precision, build_mask=False)
    sd.scale_input()
    from .dist import scene_prefers_exchanged_axes
    two = sd.Nz >= 64 and scene_prefers_exchanged_axes(sd)  # (`--devices 0` = one domain on device 0)
    m = engine.HipMulti(sd, [a.gpu] * (2 if two else 1), multi_flags=_chain_flags(a, 2 if two else 1), timing=1)
    if two:
        print(f"--2 slabs on device {a.gpu}, cut along file z: {[(m.slab(g)['x0'], m.slab(g)['x1']) for g in range(2)]}")
    # sub-timers: the busier slab's HIP-event sums (two slabs run side by side on the device)
    el, tm = _run_chain(a, sd, m)
    if tm["step_ms_total"] <= 0:  # (slab engines time their interior launches only)
        tm["step_ms_total"] = el * 1e3
    m.close()
    if _stopped_early(a, sd):
        return
    _summary(sd, tm, el)
    _finish(sd, a.data_dir)


def run_devices(a, devices):
    """`--gpus N` / `--devices`: the C library's chain object in this process (what pf_run_sim_devices does inside)"""
    print(f"--Date and time: {time.ctime()}")
    sd = sim_data.SimData.from_folder(Path(a.data_dir), a.precision, build_mask=False)
    sd.scale_input()
    try:  # (the library checks the slab count against the axis it actually cuts -- file x, or file z for rooms; gpu_engine.h:682)
        m = engine.HipMulti(sd, devices, multi_flags=_chain_flags(a, len(devices)), timing=1, verify_exchange=2)
    except engine.PfError as e:
        raise SystemExit(f"cannot run on {len(devices)} slabs: {e}")
    info = m.info()
    spans = [(m.slab(g)["x0"], m.slab(g)["x1"]) for g in range(m.nslabs)]
    print(f"--{len(devices)} slabs on devices {devices}, cut along file {'z' if info['cut_along_z'] else 'x'}: planes {spans}, ghost planes by {info['transport_name']}")
    el, tm = _run_chain(a, sd, m)
    if tm["step_ms_total"] <= 0:
        tm["step_ms_total"] = el * 1e3
    info = m.info()
    m.close()
    if info["exchange_verified"] is False:
        raise SystemExit("slab exchange self-check failed: a ghost plane does not hold what the neighbour sent")
    if _stopped_early(a, sd):
        return
    _summary(sd, tm, el)
    _finish(sd, a.data_dir)


def run_rank(a, world):
    """One rank of a `--gpus N` run (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from torch.distributed.run)."""
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # RCCL intra-node transport on this driver (dmabuf IPC)
    import torch
    import torch.distributed as dist
    from . import dist as pdist
    rank, local_rank = int(os.environ["RANK"]), int(os.environ.get("LOCAL_RANK", "0"))
    # debug only: PFFDTD_BACKEND=gloo runs every rank on GPU 0 with host-staged planes (one-GPU boxes)
    backend = os.environ.get("PFFDTD_BACKEND", "nccl")
    if backend == "gloo":
        local_rank = a.gpu
    if engine.device_count() <= local_rank:
        raise SystemExit(f"rank {rank}: no GPU {local_rank} (the HIP engine has no CPU fallback)")
    torch.cuda.set_device(local_rank)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if backend == "gloo":
        dist.init_process_group("gloo")
    else:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    try:
        if rank == 0:
            print(f"--Date and time: {time.ctime()}")
        sd = sim_data.SimData.from_folder(Path(a.data_dir), a.precision, build_mask=False)
        if world >= sd.Nx:
            raise SystemExit(f"need ngpus < Nx (got {world}, Nx={sd.Nx})")  # gpu_engine.h:682
        sd.scale_input()
        runner, loc, info = pdist.make_hip_runner(sd, rank, world, local_rank, None, timing=True)
        if rank == 0:
            az = bool(getattr(info, "along_z", False))
            print(f"--{world} GPUs, slabs of {[x1 - x0 for x0, x1 in pdist.slab_mod.partition_weighted(sd, world, az, getattr(info, 'wall_scale', 1.0))]} planes"
                  + (" cut along file z (engines store the x and z axes exchanged)" if az else " along x"))
        dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        runner.run(0, sd.Nt)
        runner.finish()
        dist.barrier()
        el = time.perf_counter() - t0
        tm = runner.st.eng.timing()
        pdist.gather_outputs(sd, loc, info)
        runner.close_comm()
        runner.st.close()
        if rank == 0:
            _summary(sd, tm, el)  # air / boundary split: rank 0's slab; the total: the whole job
            _finish(sd, a.data_dir)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--precision", default="single", choices=["single", "double"])
    p.add_argument("--data_dir", default=".", help="folder with the input .h5 files (the reference uses the CWD)")
    p.add_argument("--gpu", type=int, default=0, help="device of a single-GPU run")
    p.add_argument("--gpus", type=int, default=1, help="number of GPUs: Z-slabs on devices 0 .. N-1, driven from this one process")
    p.add_argument("--devices", default="", help="comma-separated device chain instead of 0 .. N-1, e.g. 0,1,2,3 (ids may repeat)")
    p.add_argument("--progress", type=int, nargs="?", const=200, default=0, metavar="K",
                   help="report the reference's progress fields (fdtd_common.h:106-190) every K steps (default 200)")
    p.add_argument("--checkpoint", default="", metavar="FILE", help="checkpoint file to write (--checkpoint-every, --stop-after)")
    p.add_argument("--checkpoint-every", type=int, default=0, metavar="K", help="write the checkpoint every K steps")
    p.add_argument("--stop-after", type=int, default=None, metavar="N",
                   help="take the first N steps (0 .. N-1), write the checkpoint and exit with status 0, without sim_outs.h5")
    p.add_argument("--resume", default="", metavar="FILE", help="continue from this checkpoint file")
    p.add_argument("--field-planes", action="append", default=[], metavar="x=I,y=J,z=K", help="record these planes of the field (FILE coordinates; any subset, an axis may repeat)")
    p.add_argument("--field-box", action="append", default=[], metavar="x0:x1:sx,y0:y1:sy,z0:z1:sz", help="record this strided box of the field")
    p.add_argument("--field-every", type=int, default=0, metavar="K", help="record the field regions every K steps")
    p.add_argument("--field-first", type=int, default=0, metavar="N", help="... from step N on (default 0)")
    p.add_argument("--field-file", default="", metavar="FILE", help="... into this HDF5 file (default: sim_fields.h5 in the data folder)")
    for kind in KINDS:
        kind.module.add_arguments(p)
    a = p.parse_args()
    for kind in reversed(KINDS):  # (p.error exits at the first refusal: recordings first, as ever)
        kind.module.check_arguments(p, a)
    if bool(a.field_planes or a.field_box) != bool(a.field_every) or a.field_every < 0 or a.field_first < 0:
        p.error("--field-planes / --field-box need --field-every K >= 1 (and the other way round); --field-first: not negative")
    if (a.field_first or a.field_file) and not a.field_every:
        p.error("--field-first / --field-file need --field-planes or --field-box")
    if (a.checkpoint_every or a.stop_after is not None) and not a.checkpoint:
        p.error("--checkpoint-every / --stop-after need --checkpoint FILE")
    if a.checkpoint_every < 0 or (a.stop_after is not None and a.stop_after < 0):
        p.error("--checkpoint-every / --stop-after: not negative")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    fixed = [("--checkpoint / --resume", a.checkpoint or a.resume), ("--field-planes / --field-box", a.field_every)]
    for names, asked in fixed + [(kind.names(), getattr(a, kind.flag, False)) for kind in KINDS]:
        if world > 1 and asked and not a.devices:
            raise SystemExit(f"{names}: not under a one-process-per-GPU launcher (WORLD_SIZE > 1); run one process with --gpus N or --devices")
    if a.devices:
        return run_devices(a, [int(v) for v in a.devices.split(",")])
    if world > 1:
        if a.gpus not in (1, world):
            raise SystemExit(f"--gpus {a.gpus} != WORLD_SIZE {world}")
        return run_rank(a, world)
    if a.gpus > 1:
        ndev = engine.device_count()
        if ndev < a.gpus:
            raise SystemExit(f"--gpus {a.gpus}: only {ndev} device(s) visible (name a chain with repeats by --devices for virtual slabs)")
        return run_devices(a, list(range(a.gpus)))
    run_single(a)


if __name__ == "__main__":
    main()
