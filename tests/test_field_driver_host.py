"""CPU: the run loop of the field outputs (fdtd_main._run_chain_checkpointed) with all four device-side kinds and field frames at once, on a chain
object that folds in numpy -- the observers of the kinds' own host tests behind the five factory methods, every call logged -- and a checkpoint file
kept in memory: each kind is sampled at exactly its due steps, no run crosses one, the files of a checkpoint follow its state, the takes of a step
come in the order of the kinds, a run stopped and resumed writes the files of the run in one piece, the lines of standard output carry the counts the
arguments give, and a resume with another argument is refused by the field's name."""
import argparse
import types
from collections import Counter

import numpy as np
import pytest

from pffdtd_amd import fdtd_main, h5io, recordings
from test_decay_host import FakeBand
from test_directional_host import FakeVBand
from test_recordings_host import FakeRecorder
from test_spectra_host import FakeAcc
from test_vrecordings_host import FakeVRecorder

N, NT, TS = (4, 5, 6), 40, 1.0 / 25500.0
KINDS = ("spectrum", "decay", "directional", "recording")  # the order of the takes within a step
FILES = {"frames": "sim_fields.h5", "spectrum": "sim_spectra.h5", "decay": "sim_decay.h5", "directional": "sim_directional.h5", "recording": "sim_recordings.h5"}
FIRST, EVERY = {"frames": 0, "spectrum": 2, "decay": 3, "directional": 1, "recording": 0}, {"frames": 7, "spectrum": 3}
CHECKPOINT_EVERY, STOP, FACTOR, FPASS, ATTEN = 10, 17, 4, 2000.0, 40.0
# two regions per kind, a plane and a strided box; the differences of the directional maps (and of --rec-axes) keep one cell clear of the faces
ARGS = dict(field_planes=["z=3"], field_box=["1:4:2,0:5:2,0:6:3"], field_every=EVERY["frames"], field_first=FIRST["frames"],
            spectrum_planes=["x=1"], spectrum_box=["1:4:2,0:5:2,0:6:3"], spectrum_freqs="63,125,250", spectrum_every=EVERY["spectrum"], spectrum_first=FIRST["spectrum"],
            decay_planes=["y=2"], decay_box=["0:4:1,1:5:2,0:6:3"], decay_bands="500,1000", decay_bin_ms=0.4, decay_first=FIRST["decay"],
            dir_box=["1:3:1,1:4:1,3:4:1", "1:3:1,1:4:2,1:5:3"], dir_bands="500,1000", dir_axes="y", dir_bin_ms=0.4, dir_first=FIRST["directional"],
            rec_box=["1:3:1,1:4:1,2:3:1", "1:3:1,1:4:2,1:5:3"], rec_factor=FACTOR, rec_fpass=FPASS, rec_atten=ATTEN, rec_first=FIRST["recording"],
            checkpoint="ck.h5", checkpoint_every=CHECKPOINT_EVERY)
ALONE = {"frames": ("field_",), "spectrum": ("spectrum_",), "decay": ("decay_",), "directional": ("dir_",), "recording": ("rec_",)}


def due_steps(kind, end=NT):
    return list(range(FIRST[kind], end, EVERY.get(kind, 1)))


def arguments(data_dir, only=None, **over):
    """what main() hands the run loop: argparse's defaults, ARGS (`only`: of these kinds and the checkpoint alone), `over` on top"""
    a = dict(data_dir=str(data_dir), progress=0, checkpoint="", checkpoint_every=0, stop_after=None, resume="",
             field_planes=[], field_box=[], field_every=0, field_first=0, field_file="",
             spectrum_planes=[], spectrum_box=[], spectrum_freqs="", spectrum_every=1, spectrum_first=0, spectrum_window=None, spectrum_file="",
             decay_planes=[], decay_box=[], decay_bands="", decay_bin_ms=5.0, decay_first=0, decay_file="",
             dir_planes=[], dir_box=[], dir_bands="", dir_axes="", dir_stencil="axis", dir_bin_ms=5.0, dir_first=0, dir_file="",
             rec_planes=[], rec_box=[], rec_factor=0, rec_fpass=0.0, rec_atten=80.0, rec_first=0, rec_dtype="f4", rec_file="", rec_axes="", rec_stencil="axis")
    keep = None if only is None else tuple(p for k in only for p in ALONE[k]) + ("checkpoint",)
    a.update({k: v for k, v in ARGS.items() if keep is None or k.startswith(keep)})
    a.update(over)
    a = argparse.Namespace(**a)
    a.spectrum, a.decay = bool(a.spectrum_planes or a.spectrum_box), bool(a.decay_planes or a.decay_box)
    a.directional, a.rec = bool(a.dir_planes or a.dir_box), bool(a.rec_planes or a.rec_box)
    return a


def scene():
    return types.SimpleNamespace(Nt=NT, Ts=TS, infac=0.37, Nx=N[0], Ny=N[1], Nz=N[2], diff=True, h=343.0 * TS * np.sqrt(3.0), c=343.0, fcc_flag=0, u_out=np.zeros((2, NT)))


def _logged(cls, kind, getter, chain):
    """the observer class `cls` with every add logged as a take and every `getter` call -- what a write() of the kind begins with -- as a write"""
    def add(self, *args):
        chain.log.append(("take", kind, chain.n))
        return cls.add(self, *args)

    def get(self):
        chain.log.append(("write", kind, chain.n))
        return getattr(cls, getter)(self)
    return type(cls.__name__, (cls,), {"add": add, getter: get})


class FakeChain:
    """a chain of one slab that has taken the steps 0 .. n-1: u^n is a seeded random field per step; `log` holds every call in order"""
    nslabs = 1

    def __init__(self):
        self.n, self.log = 0, []
        self._acc, self._band, self._vband = _logged(FakeAcc, "spectrum", "get", self), _logged(FakeBand, "decay", "get", self), _logged(FakeVBand, "directional", "get", self)
        self._rec, self._vrec = _logged(FakeRecorder, "recording", "get_state", self), _logged(FakeVRecorder, "recording", "get_state", self)

    def field(self):
        return np.random.default_rng(1000 + self.n).standard_normal(N).astype(np.float32)

    def run(self, n, k):
        assert n == self.n and k >= 1 and n + k <= NT, (n, k, self.n)
        self.log.append(("run", n, k))
        self.n = n + k

    def slab(self, g):
        return {"engine": types.SimpleNamespace(timing=lambda reset=False: {"air_ms_total": 0.0, "step_ms_total": 0.0})}

    def save_state(self):
        self.log.append(("save_state", self.n))
        return {"n": self.n}

    def load_state(self, state):
        self.log.append(("load_state", state["n"]))
        self.n = state["n"]

    def get_region(self, which, lo, hi, stride=(1, 1, 1)):
        assert which == 1
        self.log.append(("take", "frames", self.n))
        return self.field()[tuple(slice(lo[a], hi[a], stride[a]) for a in range(3))]

    def accumulator(self, lo, hi, stride=(1, 1, 1), nchan=1, depth=0):
        a = self._acc(lo, hi, stride, nchan)
        a.field = self.field
        return a

    def band_accumulator(self, lo, hi, stride=(1, 1, 1), pre_sos=None, band_sos=None, nbin=1, depth=0):
        return self._band(lo, hi, stride, pre_sos, band_sos, nbin, self.field)

    def vector_band_accumulator(self, lo, hi, stride=(1, 1, 1), comp=(0,), pre_sos=None, band_sos=None, prod=((0, 0, 0),), nbin=1, depth=0):
        return self._vband(lo, hi, stride, comp, pre_sos, band_sos, prod, nbin, self.field)

    def decimating_recorder(self, lo, hi, stride=(1, 1, 1), pre_sos=None, taps=None, factor=1, cap=0, depth=0):
        return self._rec(lo, hi, stride, pre_sos, taps, factor, cap, self.field)

    def vector_decimating_recorder(self, lo, hi, stride=(1, 1, 1), comp=(0,), pre_sos=None, taps=None, factor=1, cap=0, depth=0):
        return self._vrec(lo, hi, stride, comp, pre_sos, taps, factor, cap, self.field)


@pytest.fixture
def checkpoints(monkeypatch):
    """checkpoint.read / checkpoint.write as fdtd_main calls them, on a dict: {file name: (step, state, u_out)}"""
    store = {}

    def write(path, sd, n, state):
        store[str(path)] = (n, state, sd.u_out.copy())

    def read(path, sd):
        if str(path) not in store:
            raise IOError(f"{path}: no such checkpoint")
        return store[str(path)]
    monkeypatch.setattr(fdtd_main.checkpoint, "write", write)
    monkeypatch.setattr(fdtd_main.checkpoint, "read", read)
    return store


def drive(a):
    """one call of the run loop on a new chain -> its log"""
    m = FakeChain()
    fdtd_main._run_chain_checkpointed(a, scene(), m)
    return m.log


def taken(log, kind):
    """the steps at which `kind` was sampled, one entry per region, in the order of the log"""
    return [e[2] for e in log if e[0] == "take" and e[1] == kind]


def datasets(path):
    return {name: np.asarray(h5io.read(path, name)) for name in h5io.list_datasets(path)}


def test_every_kind_is_sampled_at_its_due_steps_and_no_run_crosses_one(tmp_path, checkpoints, capsys):
    a = arguments(tmp_path)
    log = drive(a)
    assert a.stopped_at == NT
    takes = [e for e in log if e[0] == "take"]
    for kind in FILES:
        steps = taken(log, kind)
        assert steps == sorted(steps) and Counter(steps) == Counter({n: 2 for n in due_steps(kind)}), kind  # once each: one add per region
    # no run crosses a due step of any kind, or a checkpoint step
    cuts = set(range(0, NT, CHECKPOINT_EVERY)).union(*(due_steps(kind) for kind in FILES))
    runs = [e for e in log if e[0] == "run"]
    assert sum(k for _, _, k in runs) == NT and all(not any(n < s < n + k for s in cuts) for _, n, k in runs), runs
    assert all(k == 1 for _, n, k in runs if n >= 1)  # (the directional maps sample every step from 1 on)
    # at a checkpoint step the four files follow the state: what --resume of that checkpoint continues
    saves = [i for i, e in enumerate(log) if e[0] == "save_state"]
    assert [log[i][1] for i in saves] == list(range(CHECKPOINT_EVERY, NT, CHECKPOINT_EVERY)) and sorted(checkpoints) == ["ck.h5"]
    for i in saves:
        assert log[i + 1:i + 9] == [("write", kind, log[i][1]) for kind in KINDS for _ in range(2)], log[i:i + 9]
    # within one step the takes come in the order of the kinds (the frame before them: its take may move the step)
    for n in range(NT):
        order = [k for _, k, at in takes if at == n]
        assert order == [k for k in ("frames",) + KINDS for _ in range(2) if n in due_steps(k)], (n, order)
    # the lines of standard output, with the counts the arguments give
    out = capsys.readouterr().out
    ntap = recordings.decimation_filter(TS, FACTOR, FPASS, ATTEN)[0].size
    lines = [f"--field spectrum of {len(due_steps('spectrum'))} samples at 3 frequencies: {tmp_path / FILES['spectrum']}",
             f"--field decay of {NT - FIRST['decay']} samples in 2 bands, bins of 10 steps: {tmp_path / FILES['decay']}",
             f"--field directional maps of {NT - FIRST['directional']} samples in 2 bands along y, bins of 10 steps: {tmp_path / FILES['directional']}",
             f"--field recording of {NT} samples, {NT // FACTOR} frames at every {FACTOR}th step through {ntap} taps: {tmp_path / FILES['recording']}"]
    assert (len(due_steps("spectrum")), round(0.4e-3 / TS)) == (13, 10)
    assert [s for s in out.splitlines() if s.startswith("--field ") and "frame at step" not in s] == lines, out
    assert [s for s in out.splitlines() if "frame at step" in s] == [f"--field frame at step {n} of {NT}: {tmp_path / FILES['frames']}" for n in due_steps("frames")]
    assert [s for s in out.splitlines() if s.startswith("--checkpoint")] == [f"--checkpoint at step {n} of {NT}: ck.h5" for n in (10, 20, 30)]


@pytest.mark.parametrize("rec_axes", ["", "x,y"], ids=["pressure", "b_format"])
def test_stopped_and_resumed_writes_the_files_of_the_run_in_one_piece(tmp_path, checkpoints, rec_axes):
    whole, part = tmp_path / "whole", tmp_path / "part"
    whole.mkdir(), part.mkdir()
    drive(arguments(whole, rec_axes=rec_axes))
    a = arguments(part, rec_axes=rec_axes, stop_after=STOP)
    log = drive(a)
    assert a.stopped_at == STOP and checkpoints["ck.h5"][0] == STOP and [e[1] for e in log if e[0] == "save_state"] == [10, STOP]
    for kind in FILES:  # a step's sample belongs to the run that takes the step
        assert sorted(set(taken(log, kind))) == due_steps(kind, STOP), kind
    log = drive(arguments(part, rec_axes=rec_axes, resume="ck.h5"))
    assert log[0] == ("load_state", STOP)
    for kind in FILES:
        assert sorted(set(taken(log, kind))) == [n for n in due_steps(kind) if n >= STOP], kind
    for kind, name in FILES.items():
        want, got = datasets(whole / name), datasets(part / name)
        assert list(got) == list(want) and len(want) > 4, kind
        for key in want:
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (kind, key)
    frames = recordings.read(part / FILES["recording"], 0)[0]
    assert frames.shape[:-3] == ((NT // FACTOR, 3) if rec_axes else (NT // FACTOR,)) and np.abs(frames).max() > 0


@pytest.mark.parametrize("field, over", [("freqs", {"spectrum_freqs": "63,125,251"}), ("bands", {"decay_bands": "500,2000"}), ("axes", {"dir_axes": "x"}),
                                         ("factor", {"rec_factor": 3})])
def test_a_resume_with_another_argument_is_refused_by_the_fields_name(tmp_path, checkpoints, field, over):
    drive(arguments(tmp_path, stop_after=STOP))
    with pytest.raises(SystemExit, match=f": {field}: "):
        drive(arguments(tmp_path, resume="ck.h5", **over))
