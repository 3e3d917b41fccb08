"""GPU: vector decimating recorders (pf_engine_vdecim_* / pf_multi_vdecim_*, kernels k_region_diff / k_region_lat / k_vband_pre / k_vdecim_fold): per
cell of a region up to four components of the field -- the cell, or a difference -- run through their own second-order sections and each through a
FIR whose every D-th output is kept as a frame [ncomp][cells], on the device.

The bar: frames, the outputs in flight and the sections' state are bit for bit those of one `Decim` per component (tests/test_recordings_host.py)
over `_components(frame, r, comp)` of tests/test_hip_vband.py / tests/test_hip_vband_fcc.py, the frame being what get_region(1, ...) gives for the
widened region at the same moment -- in every cell -- and over the oracle's fields inside; neither the depth of the ring nor the frame capacity
changes a bit; asking changes nothing: the run continues to the oracle's receivers.  Every comparison is np.array_equal.  (This file sorts behind
tests/test_hip_autotune.py: see tests/test_hip_spectra_engines.py for why its chains of three slabs must.)
"""
import ctypes

import numpy as np
import pytest
from scipy.signal import butter

import cases
import oracle
import test_hip_vband as cart
import test_hip_vband_fcc as fcc
from pffdtd_amd import engine, sim_data, synth
from test_hip_accum import KERNEL_N, KERNEL_REGIONS
from test_hip_region import PAIRS_KW, _regions, _slices
from test_hip_spectra_engines import SAMPLES
from test_hip_spectra_engines import sampled  # noqa: F401  (the module-scoped fixture: the scene, its oracle trajectory, the five makers)
from test_recordings_host import PAIRS, Decim

pytestmark = pytest.mark.gpu

# one section per component, each with coefficients of its own
PRE4 = np.stack([butter(2, wc, "high", output="sos") for wc in (0.02, 0.05, 0.08, 0.11)])
TAPS = {ntap: np.random.default_rng(97 + ntap).uniform(-1.0, 1.0, ntap) for ntap, _ in PAIRS}
assert PRE4.shape == (4, 1, 6)
CART4, FCC4 = (0, 1, 2, 3), (0, 4, 5, 6)


class VRef:
    """the reference: one Decim per component"""

    def __init__(self, pre, taps, D, ncomp, cells):
        pre = np.asarray([] if pre is None else pre, dtype=np.float64).reshape(ncomp, -1, 6)
        self.d = [Decim(pre[k], taps, D, cells) for k in range(ncomp)]

    def add(self, comps):
        assert len(comps) == len(self.d)
        for d, u in zip(self.d, comps):
            d.add(u)

    count = property(lambda self: self.d[0].count)
    acc = property(lambda self: np.stack([d.acc for d in self.d]))
    state = property(lambda self: np.stack([d.state for d in self.d]))

    def frames(self, cells):
        """[F, ncomp, c0, c1, c2]"""
        n = len(self.d[0].frames)
        return np.stack([np.array(d.frames).reshape((n,) + tuple(cells)) for d in self.d], axis=1)


def _same(rec, ref, label, got=None):
    """what is left on the device (after the frames in `got`: [(first, frames)] of earlier reads) against the reference"""
    got = list(got or [])
    got.append(rec.read())
    at = 0
    for first, fr in got:
        assert first == at and fr.dtype == np.float64 and fr.shape[1:] == (rec.ncomp,) + rec.cells, (label, first, at)
        at += fr.shape[0]
    frames, want = np.concatenate([fr for _, fr in got]), ref.frames(rec.cells)
    assert frames.shape == want.shape, (label, frames.shape, want.shape)
    assert np.array_equal(frames, want), (label, "frames", int(np.count_nonzero(frames != want)))
    acc, state = rec.get_state()
    assert acc.shape == ref.acc.shape and state.shape == ref.state.shape, label
    assert np.array_equal(acc, ref.acc), (label, "acc", int(np.count_nonzero(acc != ref.acc)))
    assert np.array_equal(state, ref.state), (label, "state", int(np.count_nonzero(state != ref.state)))
    assert rec.count == ref.count and rec.pending == 0, label
    return frames


# ---- 1. the four small scenes: frames, the oracle, and the run goes on --------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec", [("cart_outside", "double"), ("cart_mb11", "single"), ("fcc2_outside", "double"), ("fcc1_outside", "double")])
def test_frames_and_state_equal_the_fold_of_frames_and_of_the_oracle(name, prec):
    nsteps = 23
    ref_sd = cases.make_sd(name, prec)
    ref = oracle.Engine(ref_sd)
    ref_u = {}
    for n in range(nsteps):
        ref_u[n] = ref.grid(1).copy()
        ref.step(n)
    sd = cases.make_sd(name, prec)
    N = (sd.Nx, sd.Ny, sd.Nz)
    lattice = int(sd.fcc_flag) != 0
    if lattice:
        comp, regions, mod, margin = FCC4, fcc._scene_regions(N), fcc, 3
        wide = fcc._wide
    else:
        comp, mod, margin = CART4, cart, 2
        regions = [r for r in _regions(N) if cart._clear(r, N)]
        regions.append(([2, 1, 2], [N[0] - 1, N[1] - 1, N[2] - 1], [2, 1, 3]))  # a strided box around the source
        for a in range(3):  # the planes at index 1 and N - 2: the widened region holds a face cell, which forces the ghost shell
            for k in (1, N[a] - 2):
                lo, hi = [1, 1, 1], [N[0] - 1, N[1] - 1, N[2] - 1]
                lo[a], hi[a] = k, k + 1
                regions.append((lo, hi, [1, 1, 1]))

        def wide(r):
            return cart._widened(r, comp)
    assert len(regions) >= 7
    eng = engine.HipEngine(sd)
    cfg = [(7, 3), (5, 4)]  # (5, 4): P = 2 slots of 8 samples for 5 taps -- idle slots
    recs = {(c, i): eng.vector_decimating_recorder(*r, comp=comp, pre_sos=PRE4, taps=TAPS[c[0]], factor=c[1]) for c in cfg for i, r in enumerate(regions)}
    want = {k: VRef(PRE4, TAPS[k[0][0]], k[0][1], 4, a.cells) for k, a in recs.items()}
    want_ref = {k: VRef(PRE4, TAPS[k[0][0]], k[0][1], 4, a.cells) for k, a in recs.items()}
    assert recs[((5, 4), 0)].slots == 2 and recs[((7, 3), 0)].slots == 3 and recs[((7, 3), 0)].comp == comp and recs[((7, 3), 0)].ncomp == 4
    for n in range(nsteps):  # every step is a sample
        for i, r in enumerate(regions):
            for c in cfg:
                recs[(c, i)].add()
            comps = mod._components(eng.get_region(1, *wide(r)), r, comp)  # the same moment: the operands of these adds (a fold row written by them included)
            comps_ref = mod._of_grid(ref_u[n], r, comp)
            for c in cfg:
                want[(c, i)].add(comps)
                want_ref[(c, i)].add(comps_ref)
        eng.run(n, 1)
    inner = np.zeros(N, dtype=bool)
    inner[margin:-margin, margin:-margin, margin:-margin] = True  # the cell and all the neighbours it reads lie inside
    live4 = 0
    for (c, i), a in recs.items():
        r = regions[i]
        frames = _same(a, want[(c, i)], (name, c, r))
        assert frames.shape[0] == -(-nsteps // c[1])
        acc, state = a.get_state()
        sel = inner[_slices(r)]
        w = want_ref[(c, i)]
        assert np.array_equal(frames[..., sel], w.frames(a.cells)[..., sel]) and np.array_equal(acc[..., sel], w.acc[..., sel]) and \
            np.array_equal(state[..., sel], w.state[..., sel]), (name, "oracle", c, r)
        live4 += all(np.abs(frames[:, k]).max() > 0 for k in range(4))
    assert live4 >= len(cfg)  # (23 steps: the wave has reached a region, in every component)
    eng.run(nsteps, sd.Nt - nsteps)  # nothing a later step reads has changed
    for n in range(nsteps, ref_sd.Nt):
        ref.step(n)
    assert np.array_equal(sd.u_out, ref_sd.u_out) and np.abs(ref_sd.u_out).max() > 0
    eng.close()
    ref.close()


# ---- 2. the kernel alone: fields with a denormal, a -0.0 and a large value -------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [engine.PF_LAYOUT_FILE, engine.PF_LAYOUT_EXCHANGED], ids=["file_order", "exchanged"])
@pytest.mark.parametrize("prec", ["single", "double"])
def test_nine_samples_are_the_exact_filter(prec, layout):
    sd = sim_data.SimData.from_sim(synth.shoebox(*KERNEL_N, Nt=4, Nm=1, Mb=3), prec, build_mask=False)
    sd.scale_input()
    dt = np.float32 if prec == "single" else np.float64
    rng = np.random.default_rng(103)
    state = engine._state_arrays(sd)[0]
    state["u_prev"] = rng.standard_normal(KERNEL_N).astype(dt)
    fields = []
    for k in range(9):
        u = rng.standard_normal(KERNEL_N).astype(dt)
        u[5, 5, 5 + k % 2] = dt(1e-40) if prec == "single" else dt(1e-310)  # a denormal of the field's format
        u[5, 5, 6 - k % 2] = dt(-0.0)
        u[5, 5, 9] = dt(2.0 ** 60) if prec == "single" else dt(2.0 ** 500)  # (|taps| <= 1 and the sections below never amplify: everything stays finite)
        assert u[5, 5, 5 + k % 2] != 0 and abs(u[5, 5, 5 + k % 2]) < np.finfo(dt).tiny
        fields.append(u)
    # sections whose gain stays below 1: |b|, |a| <= 0.3 (no inf - inf, so no NaN reaches array_equal)
    pre8 = np.concatenate([rng.uniform(-0.3, 0.3, (4, 8, 3)), np.ones((4, 8, 1)), rng.uniform(-0.3, 0.3, (4, 8, 2))], axis=2)
    comps = {1: (0,), 2: (3, 0), 3: (1, 0, 2), 4: (2, 0, 3, 1)}
    eng = engine.HipEngine(sd, layout=layout)
    assert eng.layout()[2] == (layout == engine.PF_LAYOUT_EXCHANGED)
    recs, want = [], []
    for ntap, D in PAIRS:
        for npre in (0, 8):
            for ncomp in (1, 2, 3, 4):
                for r in KERNEL_REGIONS:
                    a = eng.vector_decimating_recorder(*r, comp=comps[ncomp], pre_sos=pre8[:ncomp, :npre], taps=TAPS[ntap], factor=D, cap=9)
                    assert (a.ncomp, a.npre, a.ntap, a.factor, a.slots) == (ncomp, npre, ntap, D, -(-ntap // D)) and a.count == 0 and a.pending == 0
                    assert not a.get_state()[0].any()
                    recs.append(a)
                    want.append((VRef(pre8[:ncomp, :npre], TAPS[ntap], D, ncomp, a.cells), r, comps[ncomp], (ntap, D, npre, ncomp)))
    assert {a.slots for a in recs} >= {1, 2, 3, 64, 128}
    for k in range(9):
        state["u_cur"] = fields[k]
        eng.load_state(state)
        for a, (w, r, comp, _) in zip(recs, want):
            a.add()
            w.add(cart._of_grid(fields[k], r, comp))
    for a, (w, r, comp, c) in zip(recs, want):
        assert np.isfinite(w.acc).all() and np.isfinite(w.state).all() and np.isfinite(w.frames(a.cells)).all()
        assert a.pending == -(-9 // c[1])
        frames = _same(a, w, (prec, c, r))
        if c[:2] == (4096, 64):  # one frame completes; the rest is pinned through get_state (above): 64 outputs in flight
            assert frames.shape[0] == 1 and a.slots == 64
        if c[:3] == (1, 1, 0):  # one tap, every sample kept: the frames are tap * double(component) exactly
            u = np.stack([np.stack(cart._of_grid(f, r, comp)) for f in fields]).astype(np.float64)
            assert np.array_equal(frames, TAPS[1][0] * u)
    eng.close()


# ---- 3. the cell alone is a decimating recorder ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cart_mb11", "fcc2_outside"])
def test_the_cell_alone_is_a_decimating_recorder(name):
    sd = cases.make_sd(name, "single")
    N = (sd.Nx, sd.Ny, sd.Nz)
    eng = engine.HipEngine(sd)
    regions = [([3, 1, 2], [min(26, N[0]), min(20, N[1]), min(22, N[2])], [1, 2, 3]), ([0, 0, 11], [N[0], N[1], 12], [1, 1, 1])]  # (the plane holds face cells)
    pairs = [(eng.vector_decimating_recorder(*r, comp=(0,), pre_sos=PRE4[:1], taps=TAPS[7], factor=3, cap=8, depth=3),
              eng.decimating_recorder(*r, pre_sos=PRE4[0], taps=TAPS[7], factor=3, cap=8, depth=4)) for r in regions]
    for n in range(20):
        for v, s in pairs:
            v.add()
            s.add()
        eng.run(n, 1)
    for v, s in pairs:
        (fv, frv), (fs, frs), (av, sv), (as_, ss) = v.read(), s.read(), v.get_state(), s.get_state()
        assert fv == fs == 0 and frv.shape == (7, 1) + s.cells and av.shape == (1,) + as_.shape and sv.shape == (1,) + ss.shape
        assert np.array_equal(frv[:, 0], frs) and np.array_equal(av[0], as_) and np.array_equal(sv[0], ss) and v.count == s.count == 20
    assert any(np.abs(s.get_state()[0]).max() > 0 for _, s in pairs)
    eng.close()


# ---- 4. neither the depth of the ring nor the frame capacity changes a bit -----------------------------------------------------------------------------
def test_depth_and_cap_change_no_bit():
    sd = cases.make_sd("cart_mb11", "single")
    N = (sd.Nx, sd.Ny, sd.Nz)
    regions = [([3, 1, 2], [25, 19, 21], [1, 2, 3]), ([1, 1, 11], [N[0] - 1, N[1] - 1, 12], [1, 1, 1])]
    comp = (0, 2, 3)
    eng = engine.HipEngine(sd)
    keys = [(d, cap, i) for d in (1, 5, 16) for cap in (1, 2, 7) for i in range(len(regions))]
    recs = {k: eng.vector_decimating_recorder(*regions[k[2]], comp=comp, pre_sos=PRE4[:3], taps=TAPS[7], factor=3, cap=k[1], depth=k[0]) for k in keys}
    want = [VRef(PRE4[:3], TAPS[7], 3, 3, recs[(1, 1, i)].cells) for i in range(len(regions))]
    got = {k: [] for k in keys}
    refused = {k: [] for k in keys}
    eng.run(0, 20)
    for s in range(17):
        n = 20 + s
        for k, a in recs.items():
            try:
                a.add()
            except engine.PfError as e:  # cap frames wait: nothing has changed; a read of one frame makes room
                assert e.code == 4 and "cap" in str(e) and "pf_engine_vdecim_add" in str(e) and s % 3 == 0, (k, s, str(e))
                refused[k].append(s)
                w = want[k[2]]
                assert a.count == s == w.count and a.pending == k[1]
                acc, state = a.get_state()  # (folds the ring: a sample the refused add had cut into it would show here)
                assert np.array_equal(acc, w.acc) and np.array_equal(state, w.state), (k, s)
                first, fr = a.read(1)
                assert fr.shape[0] == 1 and np.array_equal(fr[0], w.frames(a.cells)[first]) and a.pending == k[1] - 1, (k, s)
                got[k].append((first, fr))
                a.add()  # reading, then adding, goes on to the same bits
        for i, r in enumerate(regions):
            want[i].add(cart._components(eng.get_region(1, *cart._widened(r, comp)), r, comp))
        if s == 9:  # a read of one frame in between, samples pending in the deeper rings
            for k, a in recs.items():
                if a.pending:
                    got[k].append(a.read(1))
                    assert got[k][-1][1].shape[0] == 1
        eng.run(n, 1)
    for k, a in recs.items():
        _same(a, want[k[2]], k, got[k])
        assert (len(refused[k]) > 0) == (k[1] < 7), (k, refused[k])  # six frames in 17 samples: cap 7 never fills
    assert refused[(5, 1, 0)] == [3, 6, 9, 15] and refused[(16, 2, 1)] == [6, 9, 15]
    assert all(np.abs(w.frames(recs[(1, 1, i)].cells)).max() > 0 for i, w in enumerate(want))
    assert any(all(np.abs(w.frames(recs[(1, 1, i)].cells)[:, k]).max() > 0 for k in range(3)) for i, w in enumerate(want))
    eng.close()


# ---- 5. engines that share no kernel, layout or decomposition --------------------------------------------------------------------------------------
SHARED = {}


@pytest.mark.parametrize("kind", ["v25", "v40", "exchanged", "chain3", "chain2z"])
def test_frames_of_every_engine_and_chain(sampled, kind):  # noqa: F811
    N = sampled.n
    regions = [(r, (0, 1, 3)) for r in cart._cut_regions(N)]  # boxes across every cut of both chains
    for ck, a in (("chain3", 0), ("chain2z", 2)):  # the planes on both sides of every cut, the difference along the cut axis: its neighbour lies in the other slab
        for x in cart._chain_cuts(sampled, ck):
            for k in (x - 1, x):
                lo, hi = [1, 1, 1], [N[0] - 1, N[1] - 1, N[2] - 1]
                lo[a], hi[a] = k, k + 1
                regions.append(((lo, hi, [1, 1, 1]), (0, a + 1)))
    assert len(regions) == 2 + 2 * 2 + 2
    obj, sd = sampled.make(kind)
    if isinstance(obj, engine.HipMulti):
        assert obj.info()["cut_along_z"] == (kind == "chain2z") and all(obj.slab(g)["steps_per_pass"] == 0 for g in range(obj.nslabs))
    elif kind == "v40":
        assert obj.timing()["tb_steps_per_pass"] == 3
    elif kind == "exchanged":
        assert obj.layout()[2]
    obj.load_state(sampled.start)
    recs = [obj.vector_decimating_recorder(*r, comp=c, pre_sos=PRE4[:len(c)], taps=TAPS[7], factor=3, cap=2, depth=4) for r, c in regions]
    want = [VRef(PRE4[:len(c)], TAPS[7], 3, len(c), a.cells) for (r, c), a in zip(regions, recs)]
    want_ref = [VRef(PRE4[:len(c)], TAPS[7], 3, len(c), a.cells) for (r, c), a in zip(regions, recs)]
    got = [[] for _ in recs]
    for n in SAMPLES:  # (v40 steps in triples: run(n, 3) between the samples)
        for i, (r, c) in enumerate(regions):
            want[i].add(cart._components(obj.get_region(1, *cart._widened(r, c)), r, c))
            if recs[i].pending == 2:  # (a chain reads through its slabs' parts: the frames land in the region's cells)
                got[i].append(recs[i].read(1))
            recs[i].add()
            want_ref[i].add(cart._of_grid(sampled.ref_u[n], r, c))
        obj.run(n, 3)
    inner = np.zeros(N, dtype=bool)
    inner[2:-2, 2:-2, 2:-2] = True
    res = []
    for i, (r, c) in enumerate(regions):
        frames = _same(recs[i], want[i], (kind, sampled.prec, r), got[i])
        acc, state = recs[i].get_state()
        sel = inner[_slices(r)]
        w = want_ref[i]
        assert np.array_equal(frames[..., sel], w.frames(recs[i].cells)[..., sel]) and np.array_equal(acc[..., sel], w.acc[..., sel]) and \
            np.array_equal(state[..., sel], w.state[..., sel]) and np.abs(frames).max() > 0, (kind, "oracle", r)
        res.append((frames, acc, state))
    first = SHARED.setdefault(sampled.prec, (kind, res))  # all five give the same arrays
    for (f, a, s), (f0, a0, s0) in zip(res, first[1]):
        assert np.array_equal(f, f0) and np.array_equal(a, a0) and np.array_equal(s, s0), (kind, first[0])
    out, after = sd.u_out.copy(), obj.save_state()
    obj.close()
    sampled.check_end(out, after, f"{kind} after vector decimating recorders")


@pytest.mark.parametrize("one_thread", [False, True], ids=["slab_threads", "one_thread"])
def test_a_chain_inside_a_pair_takes_no_sample(one_thread):
    sd = sim_data.SimData.from_sim(synth.shoebox(**PAIRS_KW), "single", build_mask=False)
    sd.scale_input()
    flags = engine.PF_MULTI_FORCE_PAIRS | engine.PF_MULTI_NO_TRIPLES | (engine.PF_MULTI_ONE_THREAD if one_thread else 0)
    m = engine.HipMulti(sd, [0, 0], multi_flags=flags, air_variant=40, verify_exchange=2)
    assert m.slab(0)["steps_per_pass"] == 2 and m.slab(1)["steps_per_pass"] == 2
    r = ([1, 1, 1], [sd.Nx - 1, sd.Ny - 1, sd.Nz - 1], [3, 1, 5])  # both slabs hold cells of it
    comp = (0, 1)
    rec = m.vector_decimating_recorder(*r, comp=comp, pre_sos=PRE4[:2], taps=TAPS[5], factor=4, cap=1, depth=4)
    want = VRef(PRE4[:2], TAPS[5], 4, 2, rec.cells)
    taken, refused, full, got = [], [], [], []
    for n in range(12):
        try:
            rec.add()
        except engine.PfError as e:
            assert e.code == 4, str(e)
            if "PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES" in str(e):
                refused.append(n)
            else:  # the chain's own arithmetic, before any slab samples: cap frames wait
                assert "cap" in str(e) and "pf_multi_vdecim_add" in str(e), str(e)
                full.append(n)
                got.append(rec.read())
                rec.add()
        if n not in refused:
            taken.append(n)
            want.add(cart._components(m.get_region(1, *cart._widened(r, comp)), r, comp))
            acc, state = rec.get_state()  # (whatever a refused add before it had done would show here)
            assert np.array_equal(acc, want.acc) and np.array_equal(state, want.state), n
        assert rec.count == len(taken) and rec.pending == len(want.d[0].frames) - sum(f.shape[0] for _, f in got)
        m.run(n, 1)
    assert taken == list(range(0, 12, 2)) and refused == list(range(1, 12, 2)) and full == [8], (taken, refused, full)  # (samples 0 and 4 complete frames 0 and 1)
    frames = _same(rec, want, "end", got)
    assert np.abs(frames[:, 0]).max() > 0 and np.abs(frames[:, 1]).max() > 0
    m.run(12, sd.Nt - 12)
    ref = sim_data.SimData.from_sim(synth.shoebox(**PAIRS_KW), "single")
    ref.scale_input()
    oracle.run_sim(ref)
    assert np.array_equal(sd.u_out, ref.u_out)
    m.close()


# ---- 6. continue from the saved outputs in flight and filter state ------------------------------------------------------------------------------------
def test_a_resumed_recorder_continues_bit_for_bit():
    r = ([3, 1, 2], [25, 19, 21], [1, 2, 3])
    kw = dict(comp=CART4, pre_sos=PRE4, taps=TAPS[33], factor=16, cap=2, depth=4)

    def run(eng, rec, n0, n1):
        for n in range(n0, n1):
            rec.add()
            eng.run(n, 1)

    sd = cases.make_sd("cart_mb11", "single")
    eng = engine.HipEngine(sd)
    rec = eng.vector_decimating_recorder(*r, **{**kw, "cap": 3})
    run(eng, rec, 0, 40)
    whole = (rec.read(), rec.get_state())
    assert whole[0][0] == 0 and whole[0][1].shape[:2] == (3, 4)  # the samples 0, 16 and 32 complete a frame each
    eng.close()
    sd = cases.make_sd("cart_mb11", "single")
    eng = engine.HipEngine(sd)
    rec = eng.vector_decimating_recorder(*r, **kw)
    run(eng, rec, 0, 21)  # sample 20: inside the outputs 2 (tap 12 next) and 3
    (first, early), (acc, fstate), count, state = rec.read(), rec.get_state(), rec.count, eng.save_state()
    eng.close()  # (destroys the recorder with it)
    assert count == 21 and first == 0 and early.shape[0] == 2 and np.abs(fstate).max() > 0 and np.abs(acc).max() > 0
    results = []
    for restore in (True, False):
        sd = cases.make_sd("cart_mb11", "single")
        eng = engine.HipEngine(sd)
        eng.load_state(state)
        rec = eng.vector_decimating_recorder(*r, **kw)
        rec.add()  # a pending sample and a complete frame: set_state drops both
        assert rec.pending == 1
        rec.set_state(acc if restore else None, fstate, count)
        assert rec.count == 21 and rec.pending == 0
        run(eng, rec, 21, 40)
        results.append((rec.read(), rec.get_state()))
        assert rec.count == 40
        eng.close()
    (first, late), (acc1, st1) = results[0]
    assert first == 2 and np.array_equal(np.concatenate([early, late]), whole[0][1]) and np.array_equal(acc1, whole[1][0]) and np.array_equal(st1, whole[1][1])
    assert not np.array_equal(results[1][0][1], late)  # the control: with the outputs in flight zeroed at set_state a frame differs


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_field_and_leave_the_engine_running():
    sd = cases.make_sd("cart_mb11", "single")
    other_sd = cases.make_sd("cart_mb11", "single")
    eng, other = engine.HipEngine(sd), engine.HipEngine(other_sd)
    N = [sd.Nx, sd.Ny, sd.Nz]
    lo1, hi1 = [1, 1, 1], [N[0] - 1, N[1] - 1, N[2] - 1]
    ok = dict(comp=(0, 2), pre_sos=PRE4[:2], taps=TAPS[7], factor=3, cap=4)
    bad = TAPS[7].copy()
    bad[4] = np.inf
    nan_pre = PRE4[:2].copy()
    nan_pre[1, 0, 2] = np.nan
    for kw, field in ((dict(pre_sos=np.repeat(PRE4[:2], 9, axis=1)), "npre"), (dict(taps=[]), "ntap"), (dict(taps=np.ones(4097), factor=64), "ntap"), (dict(factor=0), "factor"),
                      (dict(factor=65), "factor"), (dict(taps=np.ones(129), factor=1), "P = "), (dict(taps=np.ones(4096), factor=31), "P = "), (dict(cap=-1), "cap"),
                      (dict(depth=17), "depth"), (dict(depth=-1), "depth"), (dict(taps=bad), "taps[4]"), (dict(pre_sos=nan_pre), "pre_sos[1][0][2]"),
                      (dict(comp=(0, 7)), "comp[1]"), (dict(comp=(0, -1)), "comp[1]"), (dict(comp=(2, 2)), "repeated"), (dict(comp=(0, 1, 2, 3, 0), pre_sos=None), "ncomp"),
                      (dict(comp=(), pre_sos=None), "ncomp")):
        with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
            eng.vector_decimating_recorder(lo1, hi1, **{**ok, **kw})
        assert ei.value.code == 1 and field in str(ei.value) and "pf_engine_vdecim_create" in str(ei.value), str(ei.value)
    for k in (4, 5, 6):  # a lattice difference on a Cartesian grid, by the component's name
        with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
            eng.vector_decimating_recorder(lo1, hi1, **{**ok, "comp": (0, k)})
        assert "comp[1]" in str(ei.value) and "fcc_flag" in str(ei.value), str(ei.value)
    for a, name in enumerate("xyz"):  # the one-cell rule along the difference axis, by the axis's name; the other axes may touch the faces
        for side in (0, 1):
            l, h = list(lo1), list(hi1)
            if side == 0:
                l[a] = 0
            else:
                h[a] = N[a]
            with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
                eng.vector_decimating_recorder(l, h, **{**ok, "comp": (0, a + 1)})
            assert f"along file {name}" in str(ei.value) and f"lo[{a}]" in str(ei.value), str(ei.value)
            eng.vector_decimating_recorder(l, h, **{**ok, "comp": (0, 1 + (a + 1) % 3)}).close()
    with pytest.raises(engine.PfError, match="a0"):
        eng.vector_decimating_recorder(lo1, hi1, **{**ok, "pre_sos": PRE4[:2] * 2.0})
    with pytest.raises(engine.PfError, match="ncomp = 2"):
        eng.vector_decimating_recorder(lo1, hi1, **{**ok, "pre_sos": PRE4[:3]})
    for lo, hi, st, field in (([0, 0, 0], [N[0], N[1] + 1, N[2]], [1, 1, 1], "hi[1]"), ([0, 0, 0], N, [1, 0, 1], "stride[1]"), ([-1, 0, 0], N, [1, 1, 1], "lo[0]")):
        with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
            eng.vector_decimating_recorder(lo, hi, st, **ok)
        assert field in str(ei.value), str(ei.value)
    # an FCC grid: the axis differences are refused and say where to go; the lattice ones keep clear of all six faces
    fsd = cases.make_sd("fcc2_outside", "single")
    feng = engine.HipEngine(fsd)
    fhi = [fsd.Nx - 1, fsd.Ny - 1, fsd.Nz - 1]
    for a in (1, 2, 3):
        with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
            feng.vector_decimating_recorder(lo1, fhi, **{**ok, "comp": (0, a)})
        assert "comp" in str(ei.value) and "fcc_flag" in str(ei.value) and "4 / 5 / 6" in str(ei.value), str(ei.value)
    with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
        feng.vector_decimating_recorder([1, 0, 0], fhi, **{**ok, "comp": (0, 4)})
    assert "along file y" in str(ei.value) and "lattice" in str(ei.value)
    feng.vector_decimating_recorder(lo1, fhi, **{**ok, "comp": (0, 5)}).close()
    feng.close()
    L = engine.lib()
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    r = engine.PfRegion((ctypes.c_int64 * 3)(*lo1), (ctypes.c_int64 * 3)(*hi1), (ctypes.c_int64 * 3)(1, 1, 1))
    h, one, c0 = vp(), np.ones(1), np.zeros(1, dtype=np.int32)
    tp, cp = one.ctypes.data_as(vp), c0.ctypes.data_as(vp)
    assert L.pf_engine_vdecim_create(eng._h, None, 1, cp, 0, None, 1, tp, 1, 1, 0, ctypes.byref(h)) == 1 and b"null pf_region" in L.pf_last_error()
    assert L.pf_engine_vdecim_create(eng._h, ctypes.byref(r), 1, cp, 0, None, 1, tp, 1, 1, 0, None) == 1 and b"null out" in L.pf_last_error()
    assert L.pf_engine_vdecim_create(None, ctypes.byref(r), 1, cp, 0, None, 1, tp, 1, 1, 0, ctypes.byref(h)) == 1 and b"null engine" in L.pf_last_error()
    assert L.pf_engine_vdecim_create(eng._h, ctypes.byref(r), 1, None, 0, None, 1, tp, 1, 1, 0, ctypes.byref(h)) == 1 and b"null comp" in L.pf_last_error()
    assert L.pf_engine_vdecim_create(eng._h, ctypes.byref(r), 1, cp, 1, None, 1, tp, 1, 1, 0, ctypes.byref(h)) == 1 and b"null pre_sos" in L.pf_last_error()
    assert L.pf_engine_vdecim_create(eng._h, ctypes.byref(r), 1, cp, 0, None, 1, None, 1, 1, 0, ctypes.byref(h)) == 1 and b"null taps" in L.pf_last_error()
    assert L.pf_engine_vdecim_create(eng._h, ctypes.byref(r), 1, cp, 0, None, 1, tp, 1, 0, 0, ctypes.byref(h)) == 1 and b"cap" in L.pf_last_error()
    assert L.pf_multi_vdecim_create(None, ctypes.byref(r), 1, cp, 0, None, 1, tp, 1, 1, 0, ctypes.byref(h)) == 1
    rec = eng.vector_decimating_recorder(lo1, hi1, comp=(0, 3), taps=[1.0], factor=1, cap=2)
    assert (rec.npre, rec.ntap, rec.slots, rec.ncomp, rec.comp) == (0, 1, 1, 2, (0, 3)) and rec.state_shape[:2] == (2, 0)
    buf = np.empty((2, 2) + rec.cells)
    bp = buf.ctypes.data_as(vp)
    first, nread = i64(), i64()
    fb, nb = ctypes.byref(first), ctypes.byref(nread)
    assert L.pf_engine_vdecim_add(eng._h, None) == 1 and b"null pf_vdecim" in L.pf_last_error()
    assert L.pf_engine_vdecim_read(eng._h, rec._a, bp, -1, fb, nb) == 1 and b"max_frames" in L.pf_last_error()
    assert L.pf_engine_vdecim_read(eng._h, rec._a, None, 1, fb, nb) == 1 and b"null frames" in L.pf_last_error()
    assert L.pf_engine_vdecim_read(eng._h, rec._a, bp, 1, None, nb) == 1 and b"null first" in L.pf_last_error()
    assert L.pf_engine_vdecim_read(eng._h, rec._a, bp, 1, fb, None) == 1 and b"null nread" in L.pf_last_error()
    assert L.pf_engine_vdecim_read(eng._h, None, bp, 1, fb, nb) == 1 and b"null pf_vdecim" in L.pf_last_error()
    assert L.pf_engine_vdecim_get_state(eng._h, rec._a, None, None) == 1 and b"null acc" in L.pf_last_error()
    assert L.pf_engine_vdecim_get_state(eng._h, None, bp, None) == 1 and b"null pf_vdecim" in L.pf_last_error()
    assert L.pf_engine_vdecim_set_state(eng._h, None, None, None, 0) == 1 and b"null pf_vdecim" in L.pf_last_error()
    assert L.pf_engine_vdecim_set_state(eng._h, rec._a, None, None, -1) == 1 and b"count" in L.pf_last_error()
    assert L.pf_engine_vdecim_destroy(eng._h, None) == 1 and L.pf_vdecim_count(None) < 0 and L.pf_vdecim_pending(None) < 0
    for call in (lambda: L.pf_engine_vdecim_add(other._h, rec._a), lambda: L.pf_engine_vdecim_read(other._h, rec._a, bp, 1, fb, nb),
                 lambda: L.pf_engine_vdecim_get_state(other._h, rec._a, bp, None), lambda: L.pf_engine_vdecim_set_state(other._h, rec._a, None, None, 0),
                 lambda: L.pf_engine_vdecim_destroy(other._h, rec._a)):
        assert call() == 1 and b"another engine" in L.pf_last_error()
    assert rec.count == 0 and rec.pending == 0
    # split-phase steps: refused inside one, valid between them
    steps = 5
    for n in range(steps):
        eng.step_begin(n)
        if n == 2:
            for f in (rec.add, rec.read, rec.get_state, lambda: rec.set_state(None, None, 0)):
                with pytest.raises(engine.PfError, match="pffdtd_hip error 4") as ei:
                    f()
                assert ei.value.code == 4
        eng.step_end(n)
    assert rec.count == 0
    r2 = (lo1, hi1, [1, 1, 1])
    u = np.stack(cart._components(eng.get_region(1, *cart._widened(r2, (0, 3))), r2, (0, 3))).astype(np.float64)
    rec.add()
    rec.add()
    with pytest.raises(engine.PfError, match="pffdtd_hip error 4") as ei:  # cap = 2 frames wait
        rec.add()
    assert "cap" in str(ei.value) and rec.count == 2 and rec.pending == 2
    first, fr = rec.read(0)
    assert first == 0 and fr.shape[0] == 0 and rec.pending == 2
    first, fr = rec.read()
    assert first == 0 and np.array_equal(fr, np.stack([u, u])) and np.abs(fr[:, 1]).max() > 0 and rec.pending == 0
    rec.set_state(None, None, 7)  # the next frame to complete is ceil(7 / 1)
    rec.add()
    assert rec.read()[0] == 7 and rec.count == 8
    # a chain names the axis against the scene's faces; a one-rank cost model has no field of the scene
    m = engine.HipMulti(cases.make_sd("cart_mb11", "single"), [0, 0], multi_flags=engine.PF_MULTI_NO_PAIRS | engine.PF_MULTI_NO_TRIPLES)
    with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
        m.vector_decimating_recorder([1, 1, 0], hi1, **{**ok, "comp": (0, 3)})
    assert "along file z" in str(ei.value) and "pf_multi_vdecim_create" in str(ei.value)
    m.vector_decimating_recorder(lo1, hi1, **ok).close()
    m.close()
    m = engine.HipMulti(cases.make_sd("cart_mb11", "single"), [0, 0], only_slab=1)
    with pytest.raises(engine.PfError, match="pffdtd_hip error 4") as ei:
        m.vector_decimating_recorder(lo1, hi1, **ok)
    assert ei.value.code == 4 and "only_slab" in str(ei.value)
    m.close()
    # the engine still runs to the oracle's receivers
    eng.run(steps, sd.Nt - steps)
    ref = cases.make_sd("cart_mb11", "single")
    oracle.run_sim(ref)
    assert np.array_equal(sd.u_out, ref.u_out) and np.abs(ref.u_out).max() > 0
    eng.close()
    other.close()
