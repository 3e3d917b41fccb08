"""GPU: the region observers in the order the drivers use -- add(), then run(n, 1), with NOTHING between -- on slab chains.

The other observer tests read the field right after (or before) every add: get_region begins with a synchronisation and ends in a blocking copy, so
there the sample's kernels (k_region_cut / k_region_lat on the main stream) have drained before the next step is enqueued.  fdtd_main.py never
does that.  A slab whose ghost shell lives in memory (every FCC grid) starts its next step with the ghost flips on its EDGE stream, and they rewrite
the shell of u^n, the grid the pending sample reads: the face cells of a region with lo = 0 or hi = N, and the neighbours of a lattice difference
at index 1 or N - 2.  Between two runs that shell is two steps old, and the contract (pf_engine_observe.inc) pins the sample to it -- "exactly as
get_region(1, ...) gives it at the same moment".  So a sample that is not ordered before the next step's flips may read a fresh shell instead.

Every test runs twice.  The reference run is the pinned order: add, get_region(1, ...) of the cells the sample reads, run(n, 1), at ring depth 1;
the host references are folded from its frames in numpy, in double precision, in call order (VFold for the band kinds, the recorders' and the
accumulator's own restatements).  The run under test is a fresh chain on a fresh scene: add, run(n, 1), no call into the chain between, one read
at the end.  Every comparison is np.array_equal over every cell, face cells and their neighbours included (no mask), and the receivers are the
oracle's.  Each region's reference frames are shown to hold face cells that are non-zero and differ between steps n and n - 2: else a stale shell
and a fresh one would be equal and the test would prove nothing.

What discriminates: the *_outside scenes (live faces all round) and the large case.  fcc2_lossy's room fills its grid, so of its faces only the fold
row is live, and a vector kind's sample writes that row itself: its cases pin u_out, the depths and single precision in driver order, but a sample
that lost the race would still pass them -- nobody should rely on them for the ordering.  The same holds for the observers of the paired chain
(section d), whose scene is a room of that sort: that test pins that a chain really inside 13-point pairs (steps_per_pass == 2, every second add
refused) takes its samples in driver order and keeps its receivers, which is the form of step_begin that starts with launch_flips on the edge
stream.  The small scenes never pair or triple (a pair's box needs 16 planes and 24 rows, a default slab 96 planes): their "default_flags" cases
run the same single steps as "no_passes" with the chain's default flags, and assert so.  No chain of this file steps in triples.

No Cartesian case: the engines a Cartesian chain makes keep a virtual ghost shell (lean / barrier-free kernels; the `kind` parameters v25 / v40 of
tests/test_hip_vband.py name single engines of that sort too), whose steps write no shell; no test of this suite runs a chain with the unfused
kernel sequence, and this file adds no engine and chain combination of its own.

(This file sorts behind tests/test_hip_autotune.py: see tests/test_hip_spectra_engines.py for why its chains of three slabs must.)
"""
import numpy as np
import pytest

import cases
import oracle
from pffdtd_amd import engine, sim_data, synth
from test_hip_accum import _fold, _w5
from test_hip_bandacc import BANDS, PRE
from test_hip_decim import _frames
from test_hip_region import PAIRS_KW
from test_hip_vband import VFold
from test_hip_vband_fcc import CHAINS, NO_PASSES, _components, _wide
from test_hip_vdecim import PRE4, TAPS, VRef
from test_recordings_host import Decim

pytestmark = pytest.mark.gpu

FCC4 = (0, 4, 5, 6)  # u, L_x, L_y, L_z
PROD5 = [(0, 0, 0), (1, 1, 0), (0, 2, 0), (0, 3, 1), (1, 3, 0)]
NTAP, FACTOR = 7, 3  # the recorders' FIR: a frame every third sample
NBIN, PER_BIN = 4, 3
VECTOR, SCALAR = ("vband", "vrec"), ("band", "rec", "acc")


# ---- the five kinds: the device observer, its host fold, what both return ------------------------------------------------------------------------------
def _cells(r):
    return tuple(len(range(r[0][a], r[1][a], r[2][a])) for a in range(3))


def _read_region(kind, r):
    """the cells a sample reads: a vector kind's lattice differences reach one cell further along all three axes"""
    return _wide(r) if kind in VECTOR else r


def _create(obj, kind, r, depth, bands=BANDS, prod=PROD5, pre=True, nbin=NBIN):
    if kind == "vband":
        return obj.vector_band_accumulator(*r, comp=FCC4, pre_sos=np.stack([PRE] * 4) if pre else None, band_sos=bands, prod=prod, nbin=nbin, depth=depth)
    if kind == "vrec":
        return obj.vector_decimating_recorder(*r, comp=FCC4, pre_sos=PRE4, taps=TAPS[NTAP], factor=FACTOR, depth=depth)
    if kind == "band":
        return obj.band_accumulator(*r, pre_sos=PRE, band_sos=bands, nbin=nbin, depth=depth)
    if kind == "rec":
        return obj.decimating_recorder(*r, pre_sos=PRE, taps=TAPS[NTAP], factor=FACTOR, depth=depth)
    return obj.accumulator(*r, nchan=5, depth=depth)


def _bin(k, nbin):
    return min(k // PER_BIN, nbin - 1)


def _add(o, kind, k, n):
    """sample k of the run, taken at step n"""
    if kind in ("vband", "band"):
        o.add(_bin(k, o.nbin))
    elif kind in ("vrec", "rec"):
        o.add()
    else:
        o.add(_w5(n))


def _read(o, kind):
    if kind in ("vband", "band"):
        return list(o.get())
    if kind in ("vrec", "rec"):
        first, frames = o.read()
        assert first == 0
        return [frames] + list(o.get_state())
    return [o.get()]


NAMES = {"vband": ("sums", "state"), "band": ("sums", "state"), "vrec": ("frames", "acc", "state"), "rec": ("frames", "acc", "state"), "acc": ("sums",)}


class Host:
    """the reference of one observer: its kind's numpy restatement, fed the frames of the synchronised run"""

    def __init__(self, kind, r, bands=BANDS, prod=PROD5, pre=True, nbin=NBIN):
        self.kind, self.r, self.nbin, c = kind, r, nbin, _cells(r)
        if kind == "vband":
            self.h = VFold(4, np.stack([PRE] * 4) if pre else np.zeros((4, 0, 6)), bands, prod, nbin, c)
        elif kind == "band":  # the vector kind with the one component 0 and its square
            self.h = VFold(1, PRE[None], bands, [(0, 0, 0)], nbin, c)
        elif kind == "vrec":
            self.h = VRef(PRE4, TAPS[NTAP], FACTOR, 4, c)
        elif kind == "rec":
            self.h = Decim(PRE, TAPS[NTAP], FACTOR, c)
        else:
            self.h = np.zeros((5,) + c)

    def add(self, frame, k, n):
        """frame: get_region(1, *_read_region(kind, r)) of the moment of the add"""
        if self.kind == "vband":
            self.h.add(_components(frame, self.r, FCC4), _bin(k, self.nbin))
        elif self.kind == "band":
            self.h.add([frame], _bin(k, self.nbin))
        elif self.kind == "vrec":
            self.h.add(_components(frame, self.r, FCC4))
        elif self.kind == "rec":
            self.h.add(frame)
        else:
            _fold(self.h, _w5(n), frame)

    def arrays(self):
        if self.kind == "vband":
            return [self.h.S, self.h.state]
        if self.kind == "band":
            return [self.h.S[0], self.h.state[0]]
        if self.kind == "vrec":
            return [self.h.frames(_cells(self.r)), self.h.acc, self.h.state]
        if self.kind == "rec":
            return [_frames(self.h, _cells(self.r)), self.h.acc, self.h.state]
        return [self.h]


def _face_mask(w, N):
    """over the cells of the region w: which of them lie on a face of the grid"""
    m = np.zeros(_cells(w), dtype=bool)
    for a in range(3):
        idx = np.arange(w[0][a], w[1][a], w[2][a])
        sel = [None, None, None]
        sel[a] = slice(None)
        m |= ((idx == 0) | (idx == N[a] - 1))[tuple(sel)]
    return m


def _where(got, want, r, N):
    """for a failure's message: how many cells of the region differ, how many of those neither lie on a face nor beside one, the first few"""
    d = got != want
    while d.ndim > 3:
        d = d.any(axis=0)
    at = np.argwhere(d) * np.array(r[2]) + np.array(r[0])
    near = ((at <= 1) | (at >= np.array(N) - 2)).any(axis=1)
    return {"cells": int(len(at)), "away_from_faces": int(np.count_nonzero(~near)), "first": at[:6].tolist()}


ORACLE = {}  # (name, prec, overrides) -> the oracle's receivers: computed once, never changed


def _oracle_out(name, prec, **override):
    key = (name, prec, repr(sorted(override.items())))
    if key not in ORACLE:
        sd = cases.make_sd(name, prec, **override)
        oracle.run_sim(sd)
        assert np.abs(sd.u_out).max() > 0
        ORACLE[key] = sd.u_out.copy()
    return ORACLE[key]


def _chain(kind, sd, flags):
    devices, cut = CHAINS[kind]
    return engine.HipMulti(sd, devices, multi_flags=cut | flags, verify_exchange=2)


def _run(sd, obj, specs, steps, depth, synchronised, **kw):
    """steps [n0, n1) with a sample of every observer before each step a chain takes one at; -> (what every observer returns, the steps taken,
    the hosts fed by this run's frames and per observer the face cells of those frames -- both only in the synchronised order)"""
    obs = [_create(obj, kind, r, depth, **kw) for kind, r in specs]
    hosts = [Host(kind, r, **kw) for kind, r in specs] if synchronised else None
    N = (sd.Nx, sd.Ny, sd.Nz)
    masks = [_face_mask(_read_region(kind, r), N) for kind, r in specs]
    faces = [dict() for _ in specs]
    taken = []
    obj.run(0, steps[0])
    for n in range(*steps):
        k = len(taken)
        order = [(k + j) % len(specs) for j in range(len(specs))]  # the add right before the run is another observer's at every sample
        refused = False
        for j, i in enumerate(order):
            kind, r = specs[i]
            try:
                _add(obs[i], kind, k, n)
            except engine.PfError as e:  # a slab inside a pair or triple: no observer takes this step (all or nothing, nothing has changed)
                assert j == 0 and e.code == 4 and "PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES" in str(e), str(e)
                refused = True
                break
            if synchronised:
                frame = obj.get_region(1, *_read_region(kind, r))  # the same moment: the operands of this add
                hosts[i].add(frame, k, n)
                faces[i][n] = frame[masks[i]].copy()
        if not refused:
            taken.append(n)
        obj.run(n, 1)  # (in the order under test: nothing has entered the chain since the last add)
    got = [_read(o, kind) for o, (kind, r) in zip(obs, specs)]
    obj.run(steps[1], sd.Nt - steps[1])
    return got, taken, hosts, faces


def _assert_live(faces, taken, which, label):
    """the face cells of the frames the reference was folded from are non-zero and differ from those two steps earlier: of the observers `which`"""
    pairs = [n for n in taken if n - 2 in taken]
    assert len(pairs) >= 2 and len(which) >= 1, (label, taken, which)
    for i in which:
        f = faces[i]
        assert all(f[n].size for n in taken), (label, i)
        for n in pairs:
            assert f[n].any() and not np.array_equal(f[n], f[n - 2]), (label, "face cells not live", i, n)


def _assert_equal(got, want, specs, N, label):
    for (kind, r), g, w in zip(specs, got, want):
        assert len(g) == len(w) == len(NAMES[kind])
        for name, x, y in zip(NAMES[kind], g, w):
            assert x.dtype == np.float64 and x.shape == y.shape, (label, kind, r, name, x.shape, y.shape)
            assert np.array_equal(x, y), (label, kind, r, name, _where(x, y, r, N))


# ---- a, c. the small scenes: every kind, every depth, single steps under both flag sets ---------------------------------------------------------------------------------
def _specs(N):
    inner = ([1, 1, 1], [N[0] - 1, N[1] - 1, N[2] - 1], [1, 1, 1])
    whole = ([0, 0, 0], list(N), [1, 1, 1])
    specs = []
    for kinds, base in ((VECTOR, inner), (SCALAR, whole)):
        regions = []
        for a in range(3):  # the planes at index 1 and N - 2: a lattice difference there reads a face; a scalar kind's plane runs from face to face
            for i in (1, N[a] - 2):
                lo, hi = list(base[0]), list(base[1])
                lo[a], hi[a] = i, i + 1
                regions.append((lo, hi, [1, 1, 1]))
        regions.append(base)  # the whole interior; a scalar kind: the whole grid, all six faces in it
        specs += [(kind, r) for kind in kinds for r in regions]
    return specs


# the source stands at (3, 3, 3) of the *_outside scenes: a cell per step, the far faces at step 29, their two-step-old copies in the shell at 31
FIRST = {"fcc2_outside": 32, "fcc1_outside": 32, "fcc2_lossy": 24}


@pytest.mark.parametrize("passes", ["no_passes", "default_flags"])
@pytest.mark.parametrize("kind", ["chain2", "chain3", "chain2z"])
@pytest.mark.parametrize("name,prec", [("fcc2_outside", "double"), ("fcc1_outside", "double"), ("fcc2_lossy", "single")])
def test_add_then_run_equals_the_fold_of_the_synchronised_twin(name, prec, kind, passes):
    flags = NO_PASSES if passes == "no_passes" else 0
    steps = (FIRST[name], FIRST[name] + 10)
    want_out = _oracle_out(name, prec)
    sd = cases.make_sd(name, prec)
    N = (sd.Nx, sd.Ny, sd.Nz)
    specs = _specs(N)
    assert len(specs) == 7 * 5
    label = (name, kind, passes)
    # the reference run: the order the other tests pin, at depth 1
    obj = _chain(kind, sd, flags)
    assert obj.nslabs == len(CHAINS[kind][0])
    assert all(obj.slab(g)["steps_per_pass"] == 0 for g in range(obj.nslabs))  # (these scenes are too small for a pass: single steps whatever the flags)
    got, taken, hosts, faces = _run(sd, obj, specs, steps, 1, True)
    obj.close()
    assert taken == list(range(*steps)), (label, taken)
    want = [h.arrays() for h in hosts]
    # fcc2_lossy's room fills its grid: nothing but zeros ever stands in the three planes behind each wall, so of its faces only the fold row (y = Ny - 1,
    # the other half of the room) is live, away from the walls: only the observers that read that row there can tell one shell from another -- the
    # vector kinds' plane y = Ny - 2 and whole interior, the scalar kinds' whole grid
    def reads_live_faces(k, r):
        lo, hi, _ = _read_region(k, r)
        return name != "fcc2_lossy" or (hi[1] == N[1] and hi[0] - lo[0] > 3 and hi[2] - lo[2] > 3)

    live = [i for i, (k, r) in enumerate(specs) if reads_live_faces(k, r)]
    assert len(live) == (len(specs) if name != "fcc2_lossy" else 2 * 2 + 3), (label, live)
    _assert_live(faces, taken, live, label)
    _assert_equal(got, want, specs, N, label + ("synchronised",))
    assert all(np.isfinite(a).all() for w in want for a in w) and all(np.abs(want[i][0]).max() > 0 for i in live)
    assert np.array_equal(sd.u_out, want_out), label
    # the runs under test: add, run, nothing between; the default depth, 3, and 1
    base = None
    for depth in (1, 0, 3):
        sd = cases.make_sd(name, prec)
        obj = _chain(kind, sd, flags)
        got, took, _, _ = _run(sd, obj, specs, steps, depth, False)
        obj.close()
        assert took == taken, (label, depth, took, taken)
        _assert_equal(got, want, specs, N, label + ("depth", depth))
        assert np.array_equal(sd.u_out, want_out) and np.abs(sd.u_out).max() > 0, (label, depth, "u_out")
        if base is None:
            base = got
        else:  # the depth of the ring changes no bit in driver order either
            _assert_equal(got, base, specs, N, label + ("depth", depth, "against depth 1"))


# ---- b. a window wide enough to lose the race in ---------------------------------------------------------------------------------------------------------
BIG = dict(Nx=352, Ny=352, Nz=352, Nt=14, rcv=[[4, 4, 4], [2, 5, 3], [4, 3, 5]])  # stored 352 x 177 x 352, receivers the wave reaches in 14 steps; the figures behind the choice: profiles/observer_ordering.txt


def test_a_long_sample_is_ordered_before_the_next_step():
    """one vector band accumulator over the whole interior of a 352-cube, two slabs, ring depth 2: the sample's kernels run for many times the host's
    gap between add returning and the next step's first launch (profiles/observer_ordering.txt), so flips that are not ordered behind the sample
    land while most of its planes are still unread"""
    name, prec, kind, steps = "fcc2_outside", "double", "chain2", (6, 12)
    want_out = _oracle_out(name, prec, **BIG)
    kw = dict(bands=np.array([[[0.25, 0.5, 0.25, 1.0, -0.2, 0.1]]]), prod=[(0, 2, 0)], pre=False, nbin=1)  # one band of one section, one product, one bin
    sd = cases.make_sd(name, prec, **BIG)
    N = (sd.Nx, sd.Ny, sd.Nz)
    specs = [("vband", ([1, 1, 1], [N[0] - 1, N[1] - 1, N[2] - 1], [1, 1, 1]))]
    obj = _chain(kind, sd, NO_PASSES)
    got, taken, hosts, faces = _run(sd, obj, specs, steps, 1, True, **kw)
    obj.close()
    assert taken == list(range(*steps))
    want = [h.arrays() for h in hosts]
    _assert_live(faces, taken, [0], "big")  # (beside the source corner: the low faces)
    _assert_equal(got, want, specs, N, ("big", "synchronised"))
    assert np.abs(want[0][0]).max() > 0 and np.isfinite(want[0][0]).all()
    assert np.array_equal(sd.u_out, want_out)
    sd = cases.make_sd(name, prec, **BIG)
    obj = _chain(kind, sd, NO_PASSES)
    got, took, _, _ = _run(sd, obj, specs, steps, 2, False, **kw)
    obj.close()
    assert took == taken
    _assert_equal(got, want, specs, N, ("big", "add then run"))
    assert np.array_equal(sd.u_out, want_out) and np.abs(sd.u_out).max() > 0


# ---- d. a chain that really steps in pairs: every second add refused, the others in driver order ---------------------------------------------------------
def _pairs_scene():
    return synth.sort_sim(synth.fold_fcc(synth.shoebox(**PAIRS_KW, fcc=True)))  # 100 x 36 x 276 stored: the scene of test_a_chain_inside_a_pair_takes_no_sample


def _pairs_sd(mask):
    sd = sim_data.SimData.from_sim(_pairs_scene(), "single", build_mask=mask)
    sd.scale_input()
    return sd


def test_a_paired_chain_takes_its_samples_in_driver_order():
    """two slabs in blocked 13-point pairs (their first half begins with launch_flips on the edge stream), stepped one step at a time: the adds at odd
    steps are refused, those at even steps are followed at once by the pair's first half"""
    flags = engine.PF_MULTI_FORCE_PAIRS | engine.PF_MULTI_NO_TRIPLES
    steps = (8, 20)  # the source stands 5 rows from the fold row: live from step 6 on
    key = ("pairs", "single")
    if key not in ORACLE:
        ref = _pairs_sd(True)
        oracle.run_sim(ref)
        ORACLE[key] = ref.u_out.copy()
    want_out = ORACLE[key]
    assert np.abs(want_out).max() > 0

    def chain(sd):
        m = engine.HipMulti(sd, [0, 0], multi_flags=flags, air_variant=40, verify_exchange=2)
        assert m.slab(0)["steps_per_pass"] == 2 and m.slab(1)["steps_per_pass"] == 2, (m.slab(0), m.slab(1))
        return m

    sd = _pairs_sd(False)
    N = (sd.Nx, sd.Ny, sd.Nz)
    inner = ([1, 1, 1], [N[0] - 1, N[1] - 1, N[2] - 1], [1, 1, 1])
    fold = ([1, N[1] - 2, 1], [N[0] - 1, N[1] - 1, N[2] - 1], [1, 1, 1])  # the plane beside the fold row
    whole = ([0, 0, 0], list(N), [1, 1, 1])
    specs = [(k, r) for k in VECTOR for r in (fold, inner)] + [(k, whole) for k in SCALAR]
    obj = chain(sd)
    got, taken, hosts, faces = _run(sd, obj, specs, steps, 1, True)
    obj.close()
    assert taken == list(range(steps[0], steps[1], 2)) and len(taken) >= 4, taken  # (the adds at the odd steps were refused: a pair was in flight)
    want = [h.arrays() for h in hosts]
    _assert_live(faces, taken, list(range(len(specs))), "pairs")
    _assert_equal(got, want, specs, N, ("pairs", "synchronised"))
    assert all(np.isfinite(a).all() for w in want for a in w) and all(np.abs(w[0]).max() > 0 for w in want)
    assert np.array_equal(sd.u_out, want_out)
    for depth in (0, 3):
        sd = _pairs_sd(False)
        obj = chain(sd)
        got, took, _, _ = _run(sd, obj, specs, steps, depth, False)
        obj.close()
        assert took == taken, (depth, took)
        _assert_equal(got, want, specs, N, ("pairs", "depth", depth))
        assert np.array_equal(sd.u_out, want_out), ("pairs", depth, "u_out")
