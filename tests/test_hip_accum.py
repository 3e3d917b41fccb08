"""GPU: field accumulators (pf_engine_accum_* / pf_multi_accum_*, kernel k_accum_fold): running sums acc[m] += w[m] * double(u^n) of a region, on the device.

The bar: the sums are bit for bit the numpy fold `acc += w * u.astype(float64)` of the frames get_region(1, ...) gives at the same moments -- in every
cell, ghost cells and the folded row included -- and of the oracle's fields inside; the depth of the ring changes no bit; asking changes nothing: the
run continues to the oracle's receivers and fields.  Every comparison is np.array_equal.
"""
import ctypes

import numpy as np
import pytest

import cases
import oracle
from pffdtd_amd import engine, sim_data, synth
from test_hip_region import PAIRS_KW, _regions, _slices

pytestmark = pytest.mark.gpu
F1, F2 = 0.0371, 0.2113  # cycles per step of the two test frequencies


def _w5(n):
    """cos and -sin at two frequencies, and one channel with w = 1"""
    p1, p2 = 2 * np.pi * ((F1 * n) % 1.0), 2 * np.pi * ((F2 * n) % 1.0)
    return np.array([np.cos(p1), -np.sin(p1), np.cos(p2), -np.sin(p2), 1.0])


def _fold(acc, w, u):
    """one sample, as the issue states it: one multiplication and one addition per channel, both rounded to double"""
    u = u.astype(np.float64)
    for m in range(len(w)):
        acc[m] += w[m] * u


def _inner(N):
    inner = np.zeros(N, dtype=bool)
    inner[1:-1, 1:-1, 1:-1] = True
    return inner


# ---- 1. the four small scenes: frames, the oracle, and the run goes on ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec", [("cart_outside", "double"), ("cart_mb11", "single"), ("fcc2_outside", "double"), ("fcc1_outside", "double")])
def test_sums_equal_the_fold_of_frames_and_of_the_oracle(name, prec):
    nsteps = 23
    ref_sd = cases.make_sd(name, prec)
    ref = oracle.Engine(ref_sd)
    ref_u = {}
    for n in range(nsteps):
        ref_u[n] = ref.grid(1).copy()
        ref.step(n)
    for every in (1, 3):  # one engine samples every step from 2 on, a second every third step with run(n, 3)
        sd = cases.make_sd(name, prec)
        N = (sd.Nx, sd.Ny, sd.Nz)
        regions = _regions(N)
        eng = engine.HipEngine(sd)
        accs = [eng.accumulator(*r, nchan=5) for r in regions]
        want = [np.zeros(a.shape) for a in accs]
        want_ref = [np.zeros(a.shape) for a in accs]
        eng.run(0, 2)
        n, taken = 2, 0
        while n < nsteps:
            w = _w5(n)
            for i, r in enumerate(regions):
                frame = eng.get_region(1, *r)  # before add: the same moment
                accs[i].add(w)
                _fold(want[i], w, frame)
                _fold(want_ref[i], w, ref_u[n][_slices(r)])
            taken += 1
            k = min(every, nsteps - n)
            eng.run(n, k)
            n += k
        inner = _inner(N)
        for i, r in enumerate(regions):
            got = accs[i].get()
            assert got.dtype == np.float64 and got.shape == (5,) + want[i].shape[1:] and accs[i].count == taken
            assert np.array_equal(got, want[i]), (name, every, r, int(np.count_nonzero(got != want[i])))
            sel = inner[_slices(r)]
            assert np.array_equal(got[:, sel], want_ref[i][:, sel]), (name, every, "oracle", r)
        assert max(np.abs(x).max() for x in want) > 0
        # nothing a later step reads has changed
        eng.run(nsteps, sd.Nt - nsteps)
        if every == 1:
            for n in range(nsteps, ref_sd.Nt):
                ref.step(n)
        assert np.array_equal(sd.u_out, ref_sd.u_out) and np.abs(ref_sd.u_out).max() > 0
        for a in accs:
            a.close()
        eng.close()
    ref.close()


# ---- 2. the kernel alone: one sample of a field with a denormal, a -0.0 and a huge value --------------------------------------------------------
KERNEL_N = (264, 12, 70)
KERNEL_REGIONS = [([5, 5, 5], [6, 6, 6], [1, 1, 1]), ([5, 5, 5], [6, 6, 7], [1, 1, 1]), ([5, 5, 3], [6, 6, 66], [1, 1, 1]), ([5, 5, 2], [6, 6, 67], [1, 1, 1]),
                  ([3, 5, 5], [260, 6, 8], [1, 1, 1])]  # 1, 2, 63, 65 and 257 x 1 x 3 cells: odd counts (the tail guard, the rows' alignment)


@pytest.mark.parametrize("layout", [engine.PF_LAYOUT_FILE, engine.PF_LAYOUT_EXCHANGED], ids=["file_order", "exchanged"])
@pytest.mark.parametrize("prec", ["single", "double"])
def test_one_sample_is_the_exact_product(prec, layout):
    sd = sim_data.SimData.from_sim(synth.shoebox(*KERNEL_N, Nt=4, Nm=1, Mb=3), prec, build_mask=False)
    sd.scale_input()
    dt = np.float32 if prec == "single" else np.float64
    rng = np.random.default_rng(79)
    state = engine._state_arrays(sd)[0]
    state["u_prev"] = rng.standard_normal(KERNEL_N).astype(dt)
    u = rng.standard_normal(KERNEL_N).astype(dt)
    u[5, 5, 5] = dt(1e-40) if prec == "single" else dt(1e-310)  # a denormal of the field's format
    u[5, 5, 6] = dt(-0.0)
    u[5, 5, 7] = np.finfo(dt).max * dt(2.0 ** -4)
    assert u[5, 5, 5] != 0 and abs(u[5, 5, 5]) < np.finfo(dt).tiny
    state["u_cur"] = u
    eng = engine.HipEngine(sd, layout=layout)
    assert eng.layout()[2] == (layout == engine.PF_LAYOUT_EXCHANGED)
    eng.load_state(state)
    for nchan in (1, 2, 256):
        w = rng.standard_normal(nchan)
        for r in KERNEL_REGIONS:
            acc = eng.accumulator(*r, nchan=nchan)
            assert acc.count == 0 and not acc.get().any()
            acc.add(w)  # at step 0, without any run
            got = acc.get()
            want = w[:, None, None, None] * u[_slices(r)].astype(np.float64)[None]
            assert got.shape == want.shape and np.array_equal(got, want), (prec, nchan, r)
            assert got[0, 5 - r[0][0], 0, 5 - r[0][2]] == w[0] * float(u[5, 5, 5]) != 0  # the denormal survived the conversion
            assert acc.count == 1
            acc.close()
    eng.close()


# ---- 3. the depth of the ring changes no bit ------------------------------------------------------------------------------------------------------------
def test_depth_changes_no_bit():
    sd = cases.make_sd("cart_mb11", "single")
    N = (sd.Nx, sd.Ny, sd.Nz)
    regions = [([3, 1, 2], [26, 20, 22], [1, 2, 3]), ([0, 0, 11], [N[0], N[1], 12], [1, 1, 1])]
    eng = engine.HipEngine(sd)
    depths = (1, 4, 16)
    accs = {(d, i): eng.accumulator(*r, nchan=5, depth=d) for d in depths for i, r in enumerate(regions)}
    want = [np.zeros(accs[(1, i)].shape) for i in range(len(regions))]
    eng.run(0, 20)
    for s in range(11):
        n = 20 + s
        w = _w5(n)
        for i, r in enumerate(regions):
            _fold(want[i], w, eng.get_region(1, *r))
        for a in accs.values():
            a.add(w)
        if s == 5:  # after the sixth sample: two pending at depth 4, six at depth 16
            for (d, i), a in accs.items():
                assert a.count == 6 and np.array_equal(a.get(), want[i]), (d, i, "mid-run")
        eng.run(n, 1)
    for (d, i), a in accs.items():
        assert a.count == 11 and np.array_equal(a.get(), want[i]), (d, i)
    assert all(np.abs(x).max() > 0 for x in want)
    for a, b in ((1, 4), (1, 16), (4, 16)):
        for i in range(len(regions)):
            assert np.array_equal(accs[(a, i)].get(), accs[(b, i)].get())
    eng.close()


# ---- 4. engines that share no kernel, layout or decomposition: tests/test_hip_spectra_engines.py (that file says why); here the chain that refuses ----
@pytest.mark.parametrize("one_thread", [False, True], ids=["slab_threads", "one_thread"])
def test_a_chain_inside_a_pair_takes_no_sample(one_thread):
    """slabs in blocked pairs, stepped one step at a time: inside a pair the add is refused as a whole -- PF_ERR_STATE, no slab's sums or count
    change, the chain stays usable --, between pairs it is taken; the sums are the fold of exactly the samples that were taken"""
    sd = sim_data.SimData.from_sim(synth.shoebox(**PAIRS_KW), "single", build_mask=False)
    sd.scale_input()
    flags = engine.PF_MULTI_FORCE_PAIRS | engine.PF_MULTI_NO_TRIPLES | (engine.PF_MULTI_ONE_THREAD if one_thread else 0)
    m = engine.HipMulti(sd, [0, 0], multi_flags=flags, air_variant=40, verify_exchange=2)
    assert m.slab(0)["steps_per_pass"] == 2 and m.slab(1)["steps_per_pass"] == 2
    r = ([1, 1, 1], [sd.Nx - 1, sd.Ny - 1, sd.Nz - 1], [3, 1, 5])  # both slabs hold cells of it
    acc = m.accumulator(*r, nchan=5, depth=4)
    want = np.zeros(acc.shape)
    taken, refused = [], []
    for n in range(12):
        w = _w5(n)
        try:
            acc.add(w)
        except engine.PfError as e:
            assert e.code == 4 and "PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES" in str(e), str(e)
            refused.append(n)
        else:
            taken.append(n)
            _fold(want, w, m.get_region(1, *r))
            assert np.array_equal(acc.get(), want), n  # (whatever a refused add before it had done would show here)
        assert acc.count == len(taken)
        m.run(n, 1)
    assert taken == list(range(0, 12, 2)) and refused == list(range(1, 12, 2)), (taken, refused)
    assert np.array_equal(acc.get(), want) and np.abs(want).max() > 0
    m.run(12, sd.Nt - 12)
    ref = sim_data.SimData.from_sim(synth.shoebox(**PAIRS_KW), "single")
    ref.scale_input()
    oracle.run_sim(ref)
    assert np.array_equal(sd.u_out, ref.u_out)
    m.close()


# ---- 5. sums equal receivers ---------------------------------------------------------------------------------------------------------------------------
def test_sums_equal_receivers():
    sd = cases.make_sd("cart_outside", "double")
    rcv = [(24, 22, 20), (2, 23, 3), (12, 12, 12)]
    rows = [[int(v) for v in sd.out_ixyz].index((x * sd.Ny + y) * sd.Nz + z) for x, y, z in rcv]
    eng = engine.HipEngine(sd)
    accs = [eng.accumulator([x, y, z], [x + 1, y + 1, z + 1], nchan=2) for x, y, z in rcv]
    ws = []
    for n in range(sd.Nt):
        ws.append(_w5(n)[2:4])
        for a in accs:
            a.add(ws[-1])
        eng.run(n, 1)
    sums = [a.get().reshape(2) for a in accs]
    eng.close()
    ref = cases.make_sd("cart_outside", "double")
    oracle.run_sim(ref)
    assert np.array_equal(sd.u_out, ref.u_out)
    live = 0
    for row, s in zip(rows, sums):
        want = np.zeros(2)
        for n in range(sd.Nt):
            want += ws[n] * sd.u_out[row, n]  # the raw row: double(u^n) of the receiver's cell
        assert np.array_equal(s, want), (row, s, want)
        live += np.abs(want).min() > 0
    assert live >= 2  # (the receiver inside the closed box hears nothing: the source stands outside)


# ---- 6. continue from saved sums --------------------------------------------------------------------------------------------------------------------
def test_a_resumed_run_continues_the_sums():
    r = ([3, 1, 2], [26, 20, 22], [1, 2, 3])

    def run(eng, acc, n0, n1):
        for n in range(n0, n1):
            acc.add(_w5(n))
            eng.run(n, 1)

    sd = cases.make_sd("cart_mb11", "single")
    eng = engine.HipEngine(sd)
    acc = eng.accumulator(*r, nchan=5, depth=4)
    run(eng, acc, 0, 20)
    whole = acc.get()
    eng.close()
    sd = cases.make_sd("cart_mb11", "single")
    eng = engine.HipEngine(sd)
    acc = eng.accumulator(*r, nchan=5, depth=4)
    run(eng, acc, 0, 9)
    sums, count, state = acc.get(), acc.count, eng.save_state()
    eng.close()  # (destroys the accumulator with it)
    assert count == 9
    results = []
    for restore in (True, False):
        sd = cases.make_sd("cart_mb11", "single")
        eng = engine.HipEngine(sd)
        eng.load_state(state)
        acc = eng.accumulator(*r, nchan=5, depth=4)
        acc.add(_w5(3))  # a pending sample: set drops it
        acc.set(sums if restore else None, count if restore else 0)
        assert acc.count == (9 if restore else 0)
        run(eng, acc, 9, 20)
        results.append((acc.get(), acc.count))
        eng.close()
    assert np.array_equal(results[0][0], whole) and results[0][1] == 20
    assert not np.array_equal(results[1][0], whole) and results[1][1] == 11  # the control: without the saved sums a value changes


# ---- 7. a region larger than one launch's grid or one 32 MiB piece ----------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [engine.PF_LAYOUT_FILE, engine.PF_LAYOUT_EXCHANGED], ids=["file_order", "exchanged"])
def test_the_whole_grid_of_a_large_scene(layout):
    n = (132, 182, 182)
    sd = sim_data.SimData.from_sim(synth.shoebox(*n, Nt=4, Nm=1, Mb=3), "double", build_mask=False)
    sd.scale_input()
    eng = engine.HipEngine(sd, layout=layout)
    assert eng.layout()[2] == (layout == engine.PF_LAYOUT_EXCHANGED)
    rng = np.random.default_rng(83)
    eng.set_grid(1, rng.standard_normal(n) * 1e-2)
    assert n[0] * n[1] * n[2] * 8 > 32 << 20
    r = ([0, 0, 0], list(n), [1, 1, 1])
    acc = eng.accumulator(*r, nchan=2, depth=2)
    want = np.zeros(acc.shape)
    for s in range(3):
        w = _w5(s)[2:4]
        _fold(want, w, eng.get_region(1, *r))
        acc.add(w)
        eng.run(s, 1)
    got = acc.get()
    assert np.array_equal(got, want) and np.abs(want).max() > 0
    eng.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_field_and_leave_the_engine_running():
    sd = cases.make_sd("cart_mb11", "single")
    other_sd = cases.make_sd("cart_mb11", "single")
    eng, other = engine.HipEngine(sd), engine.HipEngine(other_sd)
    N = [sd.Nx, sd.Ny, sd.Nz]
    for kw, field in ((dict(nchan=0), "nchan"), (dict(nchan=257), "nchan"), (dict(depth=17), "depth"), (dict(depth=-1), "depth")):
        with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
            eng.accumulator([0, 0, 0], N, **{"nchan": 1, **kw})
        assert ei.value.code == 1 and field in str(ei.value), str(ei.value)
    for lo, hi, st, field in (([0, 0, 0], [N[0], N[1] + 1, N[2]], [1, 1, 1], "hi[1]"), ([0, 0, 0], N, [1, 0, 1], "stride[1]"), ([-1, 0, 0], N, [1, 1, 1], "lo[0]")):
        with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
            eng.accumulator(lo, hi, st)
        assert field in str(ei.value), str(ei.value)
    L = engine.lib()
    vp = ctypes.c_void_p
    r = engine.PfRegion((ctypes.c_int64 * 3)(0, 0, 0), (ctypes.c_int64 * 3)(*N), (ctypes.c_int64 * 3)(1, 1, 1))
    h = vp()
    assert L.pf_engine_accum_create(eng._h, None, 1, 0, ctypes.byref(h)) == 1 and b"null pf_region" in L.pf_last_error()
    assert L.pf_engine_accum_create(eng._h, ctypes.byref(r), 1, 0, None) == 1 and b"null out" in L.pf_last_error()
    assert L.pf_engine_accum_create(None, ctypes.byref(r), 1, 0, ctypes.byref(h)) == 1 and b"null engine" in L.pf_last_error()
    assert L.pf_multi_accum_create(None, ctypes.byref(r), 1, 0, ctypes.byref(h)) == 1
    acc = eng.accumulator([0, 0, 0], N, nchan=2)
    w = np.array([1.0, 2.0])
    buf = np.empty(acc.shape)
    wp, bp = w.ctypes.data_as(vp), buf.ctypes.data_as(vp)
    assert L.pf_engine_accum_add(eng._h, acc._a, None) == 1 and b"null weights" in L.pf_last_error()
    assert L.pf_engine_accum_add(eng._h, None, wp) == 1 and b"null pf_accum" in L.pf_last_error()
    assert L.pf_engine_accum_get(eng._h, acc._a, None) == 1 and b"null host" in L.pf_last_error()
    assert L.pf_engine_accum_get(eng._h, None, bp) == 1 and b"null pf_accum" in L.pf_last_error()
    assert L.pf_engine_accum_set(eng._h, None, None, 0) == 1 and b"null pf_accum" in L.pf_last_error()
    assert L.pf_engine_accum_set(eng._h, acc._a, None, -1) == 1 and b"count" in L.pf_last_error()
    assert L.pf_engine_accum_destroy(eng._h, None) == 1 and L.pf_accum_count(None) < 0
    # a handle from another engine
    for call in (lambda: L.pf_engine_accum_add(other._h, acc._a, wp), lambda: L.pf_engine_accum_get(other._h, acc._a, bp),
                 lambda: L.pf_engine_accum_set(other._h, acc._a, None, 0), lambda: L.pf_engine_accum_destroy(other._h, acc._a)):
        assert call() == 1 and b"another engine" in L.pf_last_error()
    assert acc.count == 0
    # split-phase steps: refused inside one, valid between them
    steps = 5
    for n in range(steps):
        eng.step_begin(n)
        if n == 2:
            for f in (lambda: acc.add(w), acc.get, lambda: acc.set(None, 0)):
                with pytest.raises(engine.PfError, match="pffdtd_hip error 4") as ei:
                    f()
                assert ei.value.code == 4
        eng.step_end(n)
    assert acc.count == 0
    acc.add(w)
    assert np.array_equal(acc.get(), w[:, None, None, None] * eng.get_region(1, [0, 0, 0], N).astype(np.float64)[None]) and acc.count == 1
    # a one-rank cost model has no field of the scene
    m = engine.HipMulti(cases.make_sd("cart_mb11", "single"), [0, 0], only_slab=1)
    with pytest.raises(engine.PfError, match="pffdtd_hip error 4") as ei:
        m.accumulator([0, 0, 0], N)
    assert ei.value.code == 4 and "only_slab" in str(ei.value)
    m.close()
    # the engine with the energy diagnostic answers
    sd2 = cases.make_sd("cart_mb11", "double")
    en = engine.HipEngine(sd2, energy=True)
    en.energy_cfg(sd2.h, sd2.c, sd2.Ts, sd2.DEF)
    en.run_energy(0, 9, np.zeros(sd2.Nt), np.zeros(sd2.Nt + 1), np.zeros(sd2.Nt + 1))
    a2 = en.accumulator([3, 1, 2], [26, 20, 22], [1, 2, 3], nchan=1)
    a2.add([0.5])
    assert np.array_equal(a2.get()[0], 0.5 * en.get_grid(1)[3:26:1, 1:20:2, 2:22:3]) and a2.get().any()
    en.close()
    # the engine still runs to the oracle's receivers
    eng.run(steps, sd.Nt - steps)
    ref = cases.make_sd("cart_mb11", "single")
    oracle.run_sim(ref)
    assert np.array_equal(sd.u_out, ref.u_out) and np.abs(ref.u_out).max() > 0
    eng.close()
    other.close()
