"""GPU: decimating recorders (pf_engine_decim_* / pf_multi_decim_*, the vector recorder's kernels k_vband_pre / k_vdecim_fold with one component):
per cell of a region every sample u^n runs through shared second-order sections and a FIR whose every D-th output is kept as a frame, on the device.

The bar: frames, the outputs in flight and the sections' state are bit for bit those of `Decim` (tests/test_recordings_host.py: a numpy loop over
time, vectorised over cells, written with the contract's lines -- the FIR in arrival order, product and sum each rounded to double once) over the
frames get_region(1, ...) gives at the same moments -- in every cell, ghost cells and the folded row included -- and over the oracle's fields
inside; neither the depth of the ring nor the frame capacity changes a bit; asking changes nothing: the run continues to the oracle's receivers
and fields.  Every comparison is np.array_equal.  (This file sorts behind tests/test_hip_autotune.py: see tests/test_hip_spectra_engines.py for
why its chains of three slabs must.)
"""
import ctypes

import numpy as np
import pytest
from scipy.signal import butter

import cases
import oracle
from pffdtd_amd import engine, sim_data, synth
from test_hip_accum import KERNEL_N, KERNEL_REGIONS, _inner
from test_hip_region import PAIRS_KW, _regions, _slices
from test_hip_spectra_engines import SAMPLES, _chain_regions
from test_hip_spectra_engines import sampled  # noqa: F401  (the module-scoped fixture: the scene, its oracle trajectory, the five makers)
from test_recordings_host import PAIRS, Decim

pytestmark = pytest.mark.gpu

PRE = butter(2, 0.02, "high", output="sos")  # npre = 1
TAPS = {ntap: np.random.default_rng(97 + ntap).uniform(-1.0, 1.0, ntap) for ntap, _ in PAIRS}
assert PRE.shape == (1, 6)


def _frames(ref, cells):
    return np.array(ref.frames).reshape((len(ref.frames),) + tuple(cells))


def _same(rec, ref, label, got=None):
    """what is left on the device (after the frames in `got`: [(first, frames)] of earlier reads) against the reference"""
    got = list(got or [])
    got.append(rec.read())
    at = 0
    for first, fr in got:
        assert first == at and fr.dtype == np.float64 and fr.shape[1:] == rec.cells, (label, first, at)
        at += fr.shape[0]
    frames, want = np.concatenate([fr for _, fr in got]), _frames(ref, rec.cells)
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
    regions = _regions(N)
    eng = engine.HipEngine(sd)
    inner = _inner(N)
    cfg = [(7, 3), (5, 4)]  # (5, 4): P = 2 slots of 8 samples for 5 taps -- idle slots
    recs = {(c, i): eng.decimating_recorder(*r, pre_sos=PRE, taps=TAPS[c[0]], factor=c[1]) for c in cfg for i, r in enumerate(regions)}
    want = {k: Decim(PRE, TAPS[k[0][0]], k[0][1], a.cells) for k, a in recs.items()}
    want_ref = {k: Decim(PRE, TAPS[k[0][0]], k[0][1], a.cells) for k, a in recs.items()}
    assert recs[((5, 4), 0)].slots == 2 and recs[((7, 3), 0)].slots == 3
    for n in range(nsteps):  # every step is a sample
        for i, r in enumerate(regions):
            frame = eng.get_region(1, *r)  # before add: the same moment
            for c in cfg:
                recs[(c, i)].add()
                want[(c, i)].add(frame)
                want_ref[(c, i)].add(ref_u[n][_slices(r)])
        eng.run(n, 1)
    live = 0
    for (c, i), a in recs.items():
        r = regions[i]
        frames = _same(a, want[(c, i)], (name, c, r))
        assert frames.shape[0] == -(-nsteps // c[1])
        acc, state = a.get_state()
        sel = inner[_slices(r)]
        assert np.array_equal(frames[:, sel], _frames(want_ref[(c, i)], a.cells)[:, sel]) and np.array_equal(acc[:, sel], want_ref[(c, i)].acc[:, sel]) and \
            np.array_equal(state[:, :, sel], want_ref[(c, i)].state[:, :, sel]), (name, "oracle", c, r)
        live += np.abs(frames).max() > 0
    assert live >= len(cfg) * 3
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
    rng = np.random.default_rng(101)
    state = engine._state_arrays(sd)[0]
    state["u_prev"] = rng.standard_normal(KERNEL_N).astype(dt)
    fields = []
    for k in range(9):
        u = rng.standard_normal(KERNEL_N).astype(dt)
        u[5, 5, 5 + k % 2] = dt(1e-40) if prec == "single" else dt(1e-310)  # a denormal of the field's format
        u[5, 5, 6 - k % 2] = dt(-0.0)
        u[5, 5, 7] = dt(2.0 ** 60) if prec == "single" else dt(2.0 ** 500)  # (|taps| <= 1 and the sections below never amplify: everything stays finite)
        assert u[5, 5, 5 + k % 2] != 0 and abs(u[5, 5, 5 + k % 2]) < np.finfo(dt).tiny
        fields.append(u)
    # sections whose gain stays below 1: |b|, |a| <= 0.3 (no inf - inf, so no NaN reaches array_equal)
    pre8 = np.concatenate([rng.uniform(-0.3, 0.3, (8, 3)), np.ones((8, 1)), rng.uniform(-0.3, 0.3, (8, 2))], axis=1)
    eng = engine.HipEngine(sd, layout=layout)
    assert eng.layout()[2] == (layout == engine.PF_LAYOUT_EXCHANGED)
    recs, want = [], []
    for ntap, D in PAIRS:
        for npre in (0, 8):
            for r in KERNEL_REGIONS:
                a = eng.decimating_recorder(*r, pre_sos=pre8[:npre], taps=TAPS[ntap], factor=D, cap=9)
                assert (a.npre, a.ntap, a.factor, a.slots) == (npre, ntap, D, -(-ntap // D)) and a.count == 0 and a.pending == 0 and not a.get_state()[0].any()
                recs.append(a)
                want.append((Decim(pre8[:npre], TAPS[ntap], D, a.cells), r, (ntap, D, npre)))
    assert {a.slots for a in recs} >= {1, 2, 3, 64, 128}
    for k in range(9):
        state["u_cur"] = fields[k]
        eng.load_state(state)
        for a, (w, r, _) in zip(recs, want):
            a.add()
            w.add(fields[k][_slices(r)])
    for a, (w, r, c) in zip(recs, want):
        assert np.isfinite(w.acc).all() and np.isfinite(w.state).all() and np.isfinite(np.array(w.frames)).all()
        assert a.pending == -(-9 // c[1])
        frames = _same(a, w, (prec, c, r))
        if c[:2] == (4096, 64):  # one frame completes; the rest is pinned through get_state (above): 64 outputs in flight
            assert frames.shape[0] == 1 and a.slots == 64
        if c == (1, 1, 0):  # one tap, every sample kept: the frames are tap * double(u) exactly -- the denormal survives the conversion
            u = np.stack([f[_slices(r)] for f in fields]).astype(np.float64)
            assert np.array_equal(frames, TAPS[1][0] * u)
            assert frames[0, 5 - r[0][0], 0, 5 - r[0][2]] == TAPS[1][0] * float(fields[0][5, 5, 5]) != 0
    eng.close()


def test_one_unit_tap_gives_the_field_itself():
    """(ntap, D) = (1, 1) with h = [1]: the frames are double(u) exactly"""
    sd = cases.make_sd("cart_mb11", "single")
    N = (sd.Nx, sd.Ny, sd.Nz)
    eng = engine.HipEngine(sd)
    rec = eng.decimating_recorder([0, 0, 0], N, taps=[1.0], factor=1, cap=4, depth=3)
    eng.run(0, 20)
    us = []
    for n in range(20, 24):
        us.append(eng.get_region(1, [0, 0, 0], N).astype(np.float64))
        rec.add()
        eng.run(n, 1)
    first, frames = rec.read()
    assert first == 0 and np.array_equal(frames, np.stack(us)) and np.abs(frames).max() > 0 and not rec.get_state()[0].any()
    eng.close()


# ---- 3. neither the depth of the ring nor the frame capacity changes a bit -----------------------------------------------------------------------------
def test_depth_and_cap_change_no_bit():
    sd = cases.make_sd("cart_mb11", "single")
    N = (sd.Nx, sd.Ny, sd.Nz)
    regions = [([3, 1, 2], [26, 20, 22], [1, 2, 3]), ([0, 0, 11], [N[0], N[1], 12], [1, 1, 1])]
    eng = engine.HipEngine(sd)
    keys = [(d, cap, i) for d in (1, 5, 16) for cap in (1, 2, 7) for i in range(len(regions))]
    recs = {k: eng.decimating_recorder(*regions[k[2]], pre_sos=PRE, taps=TAPS[7], factor=3, cap=k[1], depth=k[0]) for k in keys}
    want = [Decim(PRE, TAPS[7], 3, recs[(1, 1, i)].cells) for i in range(len(regions))]
    got = {k: [] for k in keys}
    refused = {k: [] for k in keys}
    eng.run(0, 20)
    for s in range(17):
        n = 20 + s
        for k, a in recs.items():
            try:
                a.add()
            except engine.PfError as e:  # cap frames wait: nothing has changed; a read of one frame makes room
                assert e.code == 4 and "cap" in str(e) and s % 3 == 0, (k, s, str(e))
                refused[k].append(s)
                w = want[k[2]]
                assert a.count == s == w.count and a.pending == k[1]
                acc, state = a.get_state()
                assert np.array_equal(acc, w.acc) and np.array_equal(state, w.state), (k, s)
                first, fr = a.read(1)
                assert fr.shape[0] == 1 and np.array_equal(fr[0], w.frames[first]) and a.pending == k[1] - 1, (k, s)
                got[k].append((first, fr))
                a.add()  # reading, then adding, goes on to the same bits
        for i, r in enumerate(regions):
            want[i].add(eng.get_region(1, *r))
        if s == 9:  # a read of one frame in between, samples pending in the deeper rings
            for k, a in recs.items():
                if a.pending:
                    got[k].append(a.read(1))
                    assert got[k][-1][1].shape[0] == 1
        eng.run(n, 1)
    for k, a in recs.items():
        _same(a, want[k[2]], k, got[k])
        assert (len(refused[k]) > 0) == (k[1] < 7), (k, refused[k])  # six frames in 17 samples: cap 7 never fills
    assert refused[(5, 1, 0)] == [3, 6, 9, 15] and refused[(16, 2, 1)] == [6, 9, 15] and all(np.abs(np.array(w.frames)).max() > 0 for w in want)
    eng.close()


# ---- 4. engines that share no kernel, layout or decomposition --------------------------------------------------------------------------------------
_five = {}


@pytest.mark.parametrize("kind", ["v25", "v40", "exchanged", "chain3", "chain2z"])
def test_frames_of_every_engine_and_chain(sampled, kind):  # noqa: F811
    obj, sd = sampled.make(kind)
    N = sampled.n
    if isinstance(obj, engine.HipMulti):
        assert obj.info()["cut_along_z"] == (kind == "chain2z") and all(obj.slab(g)["steps_per_pass"] == 0 for g in range(obj.nslabs))
    elif kind == "v40":
        assert obj.timing()["tb_steps_per_pass"] == 3
    elif kind == "exchanged":
        assert obj.layout()[2]
    obj.load_state(sampled.start)
    regions = _chain_regions(obj, N, kind)
    recs = [obj.decimating_recorder(*r, pre_sos=PRE, taps=TAPS[7], factor=3, cap=2, depth=4) for r in regions]
    want = [Decim(PRE, TAPS[7], 3, a.cells) for a in recs]
    want_ref = [Decim(PRE, TAPS[7], 3, a.cells) for a in recs]
    got = [[] for _ in recs]
    for k, n in enumerate(SAMPLES):  # (v40 steps in triples: run(n, 3) between the samples)
        for i, r in enumerate(regions):
            want[i].add(obj.get_region(1, *r))
            if recs[i].pending == 2:  # (a chain reads through its slabs' parts: the frames land in the region's cells)
                got[i].append(recs[i].read(1))
            recs[i].add()
            want_ref[i].add(sampled.ref_u[n][_slices(r)])
        obj.run(n, 3)
    inner = _inner(N)
    for i, r in enumerate(regions):
        frames = _same(recs[i], want[i], (kind, sampled.prec, r), got[i])
        acc, state = recs[i].get_state()
        sel = inner[_slices(r)]
        assert np.array_equal(frames[:, sel], _frames(want_ref[i], recs[i].cells)[:, sel]) and np.array_equal(acc[:, sel], want_ref[i].acc[:, sel]) and \
            np.array_equal(state[:, :, sel], want_ref[i].state[:, :, sel]) and np.abs(frames).max() > 0, (kind, "oracle", r)
        if i < 3:  # the regions every kind shares: all five give the same arrays
            first = _five.setdefault((sampled.prec, i), (kind, frames, acc, state))
            assert all(np.array_equal(x, y) for x, y in zip(first[1:], (frames, acc, state))), (kind, first[0], r)
    out, after = sd.u_out.copy(), obj.save_state()
    obj.close()
    sampled.check_end(out, after, f"{kind} after decimating recorders")


# ---- 5. a chain inside a pair takes no sample -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_thread", [False, True], ids=["slab_threads", "one_thread"])
def test_a_chain_inside_a_pair_takes_no_sample(one_thread):
    sd = sim_data.SimData.from_sim(synth.shoebox(**PAIRS_KW), "single", build_mask=False)
    sd.scale_input()
    flags = engine.PF_MULTI_FORCE_PAIRS | engine.PF_MULTI_NO_TRIPLES | (engine.PF_MULTI_ONE_THREAD if one_thread else 0)
    m = engine.HipMulti(sd, [0, 0], multi_flags=flags, air_variant=40, verify_exchange=2)
    assert m.slab(0)["steps_per_pass"] == 2 and m.slab(1)["steps_per_pass"] == 2
    r = ([1, 1, 1], [sd.Nx - 1, sd.Ny - 1, sd.Nz - 1], [3, 1, 5])  # both slabs hold cells of it
    rec = m.decimating_recorder(*r, pre_sos=PRE, taps=TAPS[5], factor=4, cap=1, depth=4)
    want = Decim(PRE, TAPS[5], 4, rec.cells)
    taken, refused, full, got = [], [], [], []
    for n in range(12):
        try:
            rec.add()
        except engine.PfError as e:
            assert e.code == 4, str(e)
            if "PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES" in str(e):
                refused.append(n)
            else:  # the chain's own arithmetic, before any slab samples: cap frames wait
                assert "cap" in str(e) and "pf_multi_decim_add" in str(e), str(e)
                full.append(n)
                got.append(rec.read())
                rec.add()
        if n not in refused:
            taken.append(n)
            want.add(m.get_region(1, *r))
            acc, state = rec.get_state()  # (whatever a refused add before it had done would show here)
            assert np.array_equal(acc, want.acc) and np.array_equal(state, want.state), n
        assert rec.count == len(taken) and rec.pending == len(want.frames) - sum(f.shape[0] for _, f in got)
        m.run(n, 1)
    assert taken == list(range(0, 12, 2)) and refused == list(range(1, 12, 2)) and full == [8], (taken, refused, full)  # (samples 0 and 4 complete frames 0 and 1)
    _same(rec, want, "end", got)
    assert np.abs(np.array(want.frames)).max() > 0
    m.run(12, sd.Nt - 12)
    ref = sim_data.SimData.from_sim(synth.shoebox(**PAIRS_KW), "single")
    ref.scale_input()
    oracle.run_sim(ref)
    assert np.array_equal(sd.u_out, ref.u_out)
    m.close()


# ---- 6. frames equal receivers -------------------------------------------------------------------------------------------------------------------------
def test_frames_equal_receivers():
    sd = cases.make_sd("cart_outside", "double")
    rcv = [(24, 22, 20), (2, 23, 3), (12, 12, 12)]
    rows = [[int(v) for v in sd.out_ixyz].index((x * sd.Ny + y) * sd.Nz + z) for x, y, z in rcv]
    eng = engine.HipEngine(sd)
    recs = [eng.decimating_recorder([x, y, z], [x + 1, y + 1, z + 1], pre_sos=PRE, taps=TAPS[7], factor=3, cap=-(-sd.Nt // 3)) for x, y, z in rcv]
    for n in range(sd.Nt):
        for a in recs:
            a.add()
        eng.run(n, 1)
    ref = cases.make_sd("cart_outside", "double")
    oracle.run_sim(ref)
    assert np.array_equal(sd.u_out, ref.u_out)
    live = 0
    for row, a in zip(rows, recs):
        want = Decim(PRE, TAPS[7], 3, (1, 1, 1))
        for n in range(sd.Nt):
            want.add(sd.u_out[row, n].reshape(1, 1, 1))  # the raw row: u^n of the receiver's cell
        live += np.abs(_same(a, want, row)).max() > 0
    assert live >= 2  # (the receiver inside the closed box hears nothing: the source stands outside)
    eng.close()


# ---- 7. continue from the saved outputs in flight and filter state ------------------------------------------------------------------------------------
def test_a_resumed_recorder_continues_bit_for_bit():
    r = ([3, 1, 2], [26, 20, 22], [1, 2, 3])
    kw = dict(pre_sos=PRE, taps=TAPS[33], factor=16, cap=2, depth=4)

    def run(eng, rec, n0, n1):
        for n in range(n0, n1):
            rec.add()
            eng.run(n, 1)

    sd = cases.make_sd("cart_mb11", "single")
    eng = engine.HipEngine(sd)
    rec = eng.decimating_recorder(*r, **{**kw, "cap": 3})
    run(eng, rec, 0, 40)
    whole = (rec.read(), rec.get_state())
    assert whole[0][0] == 0 and whole[0][1].shape[0] == 3  # the samples 0, 16 and 32 complete a frame each
    eng.close()
    sd = cases.make_sd("cart_mb11", "single")
    eng = engine.HipEngine(sd)
    rec = eng.decimating_recorder(*r, **kw)
    run(eng, rec, 0, 21)  # sample 20: inside the outputs 2 (tap 12 next) and 3
    (first, early), (acc, fstate), count, state = rec.read(), rec.get_state(), rec.count, eng.save_state()
    eng.close()  # (destroys the recorder with it)
    assert count == 21 and first == 0 and early.shape[0] == 2 and np.abs(fstate).max() > 0 and np.count_nonzero(np.abs(acc).reshape(3, -1).max(axis=1)) == 2
    results = []
    for restore in (True, False):
        sd = cases.make_sd("cart_mb11", "single")
        eng = engine.HipEngine(sd)
        eng.load_state(state)
        rec = eng.decimating_recorder(*r, **kw)
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


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_field_and_leave_the_engine_running():
    sd = cases.make_sd("cart_mb11", "single")
    other_sd = cases.make_sd("cart_mb11", "single")
    eng, other = engine.HipEngine(sd), engine.HipEngine(other_sd)
    N = [sd.Nx, sd.Ny, sd.Nz]
    ok = dict(pre_sos=PRE, taps=TAPS[7], factor=3, cap=4)
    bad = TAPS[7].copy()
    bad[4] = np.inf
    for kw, field in ((dict(pre_sos=np.repeat(PRE, 9, axis=0)), "npre"), (dict(taps=[]), "ntap"), (dict(taps=np.ones(4097), factor=64), "ntap"), (dict(factor=0), "factor"),
                      (dict(factor=65), "factor"), (dict(taps=np.ones(129), factor=1), "P = "), (dict(taps=np.ones(4096), factor=31), "P = "), (dict(cap=-1), "cap"),
                      (dict(depth=17), "depth"), (dict(depth=-1), "depth"), (dict(taps=bad), "taps[4]"), (dict(pre_sos=PRE * np.array([1, 1, np.nan, 1, 1, 1])), "pre_sos[0][2]")):
        with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
            eng.decimating_recorder([0, 0, 0], N, **{**ok, **kw})
        assert ei.value.code == 1 and field in str(ei.value), str(ei.value)
    with pytest.raises(engine.PfError, match="a0"):
        eng.decimating_recorder([0, 0, 0], N, **{**ok, "pre_sos": PRE * 2.0})
    for lo, hi, st, field in (([0, 0, 0], [N[0], N[1] + 1, N[2]], [1, 1, 1], "hi[1]"), ([0, 0, 0], N, [1, 0, 1], "stride[1]"), ([-1, 0, 0], N, [1, 1, 1], "lo[0]")):
        with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
            eng.decimating_recorder(lo, hi, st, **ok)
        assert field in str(ei.value), str(ei.value)
    L = engine.lib()
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    r = engine.PfRegion((ctypes.c_int64 * 3)(0, 0, 0), (ctypes.c_int64 * 3)(*N), (ctypes.c_int64 * 3)(1, 1, 1))
    h, one = vp(), np.ones(1)
    tp = one.ctypes.data_as(vp)
    assert L.pf_engine_decim_create(eng._h, None, 0, None, 1, tp, 1, 1, 0, ctypes.byref(h)) == 1 and b"null pf_region" in L.pf_last_error()
    assert L.pf_engine_decim_create(eng._h, ctypes.byref(r), 0, None, 1, tp, 1, 1, 0, None) == 1 and b"null out" in L.pf_last_error()
    assert L.pf_engine_decim_create(None, ctypes.byref(r), 0, None, 1, tp, 1, 1, 0, ctypes.byref(h)) == 1 and b"null engine" in L.pf_last_error()
    assert L.pf_engine_decim_create(eng._h, ctypes.byref(r), 1, None, 1, tp, 1, 1, 0, ctypes.byref(h)) == 1 and b"null pre_sos" in L.pf_last_error()
    assert L.pf_engine_decim_create(eng._h, ctypes.byref(r), 0, None, 1, None, 1, 1, 0, ctypes.byref(h)) == 1 and b"null taps" in L.pf_last_error()
    assert L.pf_engine_decim_create(eng._h, ctypes.byref(r), 0, None, 1, tp, 1, 0, 0, ctypes.byref(h)) == 1 and b"cap" in L.pf_last_error()
    assert L.pf_multi_decim_create(None, ctypes.byref(r), 0, None, 1, tp, 1, 1, 0, ctypes.byref(h)) == 1
    rec = eng.decimating_recorder([0, 0, 0], N, taps=[1.0], factor=1, cap=2)
    assert (rec.npre, rec.ntap, rec.slots) == (0, 1, 1) and rec.state_shape[0] == 0
    buf = np.empty((2,) + rec.cells)
    bp = buf.ctypes.data_as(vp)
    first, nread = i64(), i64()
    fb, nb = ctypes.byref(first), ctypes.byref(nread)
    assert L.pf_engine_decim_add(eng._h, None) == 1 and b"null pf_decim" in L.pf_last_error()
    assert L.pf_engine_decim_read(eng._h, rec._a, bp, -1, fb, nb) == 1 and b"max_frames" in L.pf_last_error()
    assert L.pf_engine_decim_read(eng._h, rec._a, None, 1, fb, nb) == 1 and b"null frames" in L.pf_last_error()
    assert L.pf_engine_decim_read(eng._h, rec._a, bp, 1, None, nb) == 1 and b"null first" in L.pf_last_error()
    assert L.pf_engine_decim_read(eng._h, rec._a, bp, 1, fb, None) == 1 and b"null nread" in L.pf_last_error()
    assert L.pf_engine_decim_read(eng._h, None, bp, 1, fb, nb) == 1 and b"null pf_decim" in L.pf_last_error()
    assert L.pf_engine_decim_get_state(eng._h, rec._a, None, None) == 1 and b"null acc" in L.pf_last_error()
    assert L.pf_engine_decim_get_state(eng._h, None, bp, None) == 1 and b"null pf_decim" in L.pf_last_error()
    assert L.pf_engine_decim_set_state(eng._h, None, None, None, 0) == 1 and b"null pf_decim" in L.pf_last_error()
    assert L.pf_engine_decim_set_state(eng._h, rec._a, None, None, -1) == 1 and b"count" in L.pf_last_error()
    assert L.pf_engine_decim_destroy(eng._h, None) == 1 and L.pf_decim_count(None) < 0 and L.pf_decim_pending(None) < 0
    for call in (lambda: L.pf_engine_decim_add(other._h, rec._a), lambda: L.pf_engine_decim_read(other._h, rec._a, bp, 1, fb, nb),
                 lambda: L.pf_engine_decim_get_state(other._h, rec._a, bp, None), lambda: L.pf_engine_decim_set_state(other._h, rec._a, None, None, 0),
                 lambda: L.pf_engine_decim_destroy(other._h, rec._a)):
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
    u = eng.get_region(1, [0, 0, 0], N).astype(np.float64)
    rec.add()
    rec.add()
    with pytest.raises(engine.PfError, match="pffdtd_hip error 4") as ei:  # cap = 2 frames wait
        rec.add()
    assert "cap" in str(ei.value) and rec.count == 2 and rec.pending == 2
    first, fr = rec.read(0)
    assert first == 0 and fr.shape[0] == 0 and rec.pending == 2
    first, fr = rec.read()
    assert first == 0 and np.array_equal(fr, np.stack([u, u])) and fr.max() > 0 and rec.pending == 0
    rec.set_state(None, None, 7)  # the next frame to complete is ceil(7 / 1)
    rec.add()
    assert rec.read()[0] == 7 and rec.count == 8
    # a one-rank cost model has no field of the scene
    m = engine.HipMulti(cases.make_sd("cart_mb11", "single"), [0, 0], only_slab=1)
    with pytest.raises(engine.PfError, match="pffdtd_hip error 4") as ei:
        m.decimating_recorder([0, 0, 0], N, **ok)
    assert ei.value.code == 4 and "only_slab" in str(ei.value)
    m.close()
    # the engine with the energy diagnostic answers
    sd2 = cases.make_sd("cart_mb11", "double")
    en = engine.HipEngine(sd2, energy=True)
    en.energy_cfg(sd2.h, sd2.c, sd2.Ts, sd2.DEF)
    en.run_energy(0, 9, np.zeros(sd2.Nt), np.zeros(sd2.Nt + 1), np.zeros(sd2.Nt + 1))
    a2 = en.decimating_recorder([3, 1, 2], [26, 20, 22], [1, 2, 3], taps=[1.0], factor=1, cap=1)
    a2.add()
    g = en.get_grid(1)[3:26:1, 1:20:2, 2:22:3]
    assert np.array_equal(a2.read()[1][0], g) and g.any()
    en.close()
    # the engine still runs to the oracle's receivers
    eng.run(steps, sd.Nt - steps)
    ref = cases.make_sd("cart_mb11", "single")
    oracle.run_sim(ref)
    assert np.array_equal(sd.u_out, ref.u_out) and np.abs(ref.u_out).max() > 0
    eng.close()
    other.close()
