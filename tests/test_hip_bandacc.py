"""GPU: band accumulators (pf_engine_bandacc_* / pf_multi_bandacc_*, kernels k_band_pre / k_band_fold): per cell of a region u^n runs through
shared second-order sections and then through each band's sections, is squared and summed into time bins, on the device.

The bar: sums and filter state are bit for bit those of a numpy loop over time, vectorised over cells, written with the contract's three lines
    y = b0*x + s1;   s1 = (b1*x - a1*y) + s2;   s2 = b2*x - a2*y
(every operation rounded to double once) over the frames get_region(1, ...) gives at the same moments -- in every cell, ghost cells and the folded
row included -- and over the oracle's fields inside; the depth of the ring changes no bit; asking changes nothing: the run continues to the
oracle's receivers and fields.  Every comparison is np.array_equal.  (This file sorts behind tests/test_hip_autotune.py: see
tests/test_hip_spectra_engines.py for why its chains of three slabs must.)
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

pytestmark = pytest.mark.gpu

PRE = butter(2, 0.02, "high", output="sos")  # npre = 1
BANDS = np.stack([butter(2, [lo, 2 * lo], "band", output="sos") for lo in (0.05, 0.1, 0.2)])  # 3 bands x 2 sections, normalised edges 0.05 .. 0.4
assert PRE.shape == (1, 6) and BANDS.shape == (3, 2, 6)


class Fold:
    """the reference: a numpy loop over time, vectorised over cells, the contract's association"""

    def __init__(self, pre, bands, nbin, cells):
        self.pre = np.asarray(pre, dtype=np.float64).reshape(-1, 6)
        self.bands = np.asarray(bands, dtype=np.float64)
        self.nband, self.nsec = self.bands.shape[0], self.bands.shape[1]
        self.E = np.zeros((self.nband, nbin) + tuple(cells))
        self.state = np.zeros((len(self.pre) + self.nband * self.nsec, 2) + tuple(cells))

    def _section(self, k, q, x):
        s = self.state[q]
        y = k[0] * x + s[0]
        s[0] = (k[1] * x - k[4] * y) + s[1]
        s[1] = k[2] * x - k[5] * y
        return y

    def add(self, u, bin):
        x = u.astype(np.float64)
        for q, k in enumerate(self.pre):
            x = self._section(k, q, x)
        for b in range(self.nband):
            y = x
            for s in range(self.nsec):
                y = self._section(self.bands[b, s], len(self.pre) + b * self.nsec + s, y)
            if bin >= 0:
                self.E[b, bin] = self.E[b, bin] + y * y


def _same(acc, ref, label, count=None):
    e, s = acc.get()
    assert e.dtype == np.float64 and e.shape == ref.E.shape and s.shape == ref.state.shape, label
    assert np.array_equal(e, ref.E), (label, "sums", int(np.count_nonzero(e != ref.E)))
    assert np.array_equal(s, ref.state), (label, "state", int(np.count_nonzero(s != ref.state)))
    if count is not None:
        assert acc.count == count, label


# ---- 1. the four small scenes: frames, the oracle, and the run goes on --------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec", [("cart_outside", "double"), ("cart_mb11", "single"), ("fcc2_outside", "double"), ("fcc1_outside", "double")])
def test_sums_and_state_equal_the_fold_of_frames_and_of_the_oracle(name, prec):
    nsteps, step_bin = 23, 4
    ref_sd = cases.make_sd(name, prec)
    ref = oracle.Engine(ref_sd)
    ref_u = {}
    for n in range(nsteps):
        ref_u[n] = ref.grid(1).copy()
        ref.step(n)
    sd = cases.make_sd(name, prec)
    N = (sd.Nx, sd.Ny, sd.Nz)
    regions = _regions(N)
    nbin = -(-(nsteps - 4) // step_bin)
    eng = engine.HipEngine(sd)
    accs = [eng.band_accumulator(*r, pre_sos=PRE, band_sos=BANDS, nbin=nbin) for r in regions]
    want = [Fold(PRE, BANDS, nbin, a.shape[2:]) for a in accs]
    want_ref = [Fold(PRE, BANDS, nbin, a.shape[2:]) for a in accs]
    eng.run(0, 2)
    for n in range(2, nsteps):  # every step from 2; the first two samples only run the filters
        bin = -1 if n < 4 else (n - 4) // step_bin
        for i, r in enumerate(regions):
            frame = eng.get_region(1, *r)  # before add: the same moment
            accs[i].add(bin)
            want[i].add(frame, bin)
            want_ref[i].add(ref_u[n][_slices(r)], bin)
        eng.run(n, 1)
    inner = _inner(N)
    for i, r in enumerate(regions):
        _same(accs[i], want[i], (name, r), count=nsteps - 2)
        e, s = accs[i].get()
        sel = inner[_slices(r)]
        assert np.array_equal(e[:, :, sel], want_ref[i].E[:, :, sel]) and np.array_equal(s[:, :, sel], want_ref[i].state[:, :, sel]), (name, "oracle", r)
    assert max(w.E.max() for w in want) > 0 and all(np.isfinite(w.E).all() for w in want)
    eng.run(nsteps, sd.Nt - nsteps)  # nothing a later step reads has changed
    for n in range(nsteps, ref_sd.Nt):
        ref.step(n)
    assert np.array_equal(sd.u_out, ref_sd.u_out) and np.abs(ref_sd.u_out).max() > 0
    eng.close()
    ref.close()


# ---- 2. the kernel alone: fields with a denormal, a -0.0 and a large value -------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [engine.PF_LAYOUT_FILE, engine.PF_LAYOUT_EXCHANGED], ids=["file_order", "exchanged"])
@pytest.mark.parametrize("prec", ["single", "double"])
def test_three_samples_are_the_exact_cascade(prec, layout):
    sd = sim_data.SimData.from_sim(synth.shoebox(*KERNEL_N, Nt=4, Nm=1, Mb=3), prec, build_mask=False)
    sd.scale_input()
    dt = np.float32 if prec == "single" else np.float64
    rng = np.random.default_rng(89)
    state = engine._state_arrays(sd)[0]
    state["u_prev"] = rng.standard_normal(KERNEL_N).astype(dt)
    fields = []
    for k in range(3):
        u = rng.standard_normal(KERNEL_N).astype(dt)
        u[5, 5, 5 + k % 2] = dt(1e-40) if prec == "single" else dt(1e-310)  # a denormal of the field's format
        u[5, 5, 6 - k % 2] = dt(-0.0)
        u[5, 5, 7] = dt(2.0 ** 60) if prec == "single" else dt(2.0 ** 500)  # (its square is finite in double; the sections below never amplify)
        assert u[5, 5, 5 + k % 2] != 0 and abs(u[5, 5, 5 + k % 2]) < np.finfo(dt).tiny
        fields.append(u)
    # sections whose gain stays below 1 over three samples: |b|, |a| <= 0.3 (no inf - inf, so no NaN reaches array_equal)
    pre8 = np.concatenate([rng.uniform(-0.3, 0.3, (8, 3)), np.ones((8, 1)), rng.uniform(-0.3, 0.3, (8, 2))], axis=1)
    band16 = np.concatenate([rng.uniform(-0.3, 0.3, (16, 8, 3)), np.ones((16, 8, 1)), rng.uniform(-0.3, 0.3, (16, 8, 2))], axis=2)
    eng = engine.HipEngine(sd, layout=layout)
    assert eng.layout()[2] == (layout == engine.PF_LAYOUT_EXCHANGED)
    cfg = [(nband, nsec, npre) for nband in (1, 16) for nsec in (0, 1, 8) for npre in (0, 8)]
    accs, want = [], []
    for nband, nsec, npre in cfg:
        for r in KERNEL_REGIONS:
            pre, bands = pre8[:npre], band16[:nband, :nsec]
            a = eng.band_accumulator(*r, pre_sos=pre, band_sos=bands, nbin=2)
            assert (a.npre, a.nband, a.nsec) == (npre, nband, nsec) and a.count == 0 and not a.get()[0].any()
            accs.append(a)
            want.append((Fold(pre, bands, 2, a.shape[2:]), r, (nband, nsec, npre)))
    for k, bin in enumerate((0, 1, 1)):  # a bin change inside the fold, then two samples of one bin
        state["u_cur"] = fields[k]
        eng.load_state(state)
        for a, (w, r, _) in zip(accs, want):
            a.add(bin)
            w.add(fields[k][_slices(r)], bin)
    for a, (w, r, c) in zip(accs, want):
        assert np.isfinite(w.E).all() and np.isfinite(w.state).all()
        _same(a, w, (prec, c, r), count=3)
        if c[1] == 0 and c[2] == 0:  # plain squares: the denormal survived the conversion
            d = a.get()[0][0, 0, 5 - r[0][0], 0, 5 - r[0][2]]
            assert d == float(fields[0][5, 5, 5]) ** 2 and (d != 0 or prec == "double")  # (1e-310 ** 2 underflows in any arithmetic)
    eng.close()


# ---- 3. the depth of the ring changes no bit ------------------------------------------------------------------------------------------------------------
def test_depth_changes_no_bit():
    sd = cases.make_sd("cart_mb11", "single")
    N = (sd.Nx, sd.Ny, sd.Nz)
    regions = [([3, 1, 2], [26, 20, 22], [1, 2, 3]), ([0, 0, 11], [N[0], N[1], 12], [1, 1, 1])]
    eng = engine.HipEngine(sd)
    depths = (1, 5, 16)
    accs = {(d, i): eng.band_accumulator(*r, pre_sos=PRE, band_sos=BANDS, nbin=4, depth=d) for d in depths for i, r in enumerate(regions)}
    want = [Fold(PRE, BANDS, 4, accs[(1, i)].shape[2:]) for i in range(len(regions))]
    eng.run(0, 20)
    for s in range(11):
        n = 20 + s
        bin = s // 3  # bins of 3 steps: they change inside the folds of depth 5 and 16
        for i, r in enumerate(regions):
            want[i].add(eng.get_region(1, *r), bin)
        for a in accs.values():
            a.add(bin)
        if s == 6:  # after the seventh sample: two pending at depth 5, seven at depth 16
            for (d, i), a in accs.items():
                _same(a, want[i], (d, i, "mid-run"), count=7)
        eng.run(n, 1)
    for (d, i), a in accs.items():
        _same(a, want[i], (d, i), count=11)
    assert all(w.E.max() > 0 for w in want)
    eng.close()


# ---- 4. engines that share no kernel, layout or decomposition --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["v25", "v40", "exchanged", "chain3", "chain2z"])
def test_sums_of_every_engine_and_chain(sampled, kind):  # noqa: F811
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
    accs = [obj.band_accumulator(*r, pre_sos=PRE, band_sos=BANDS, nbin=3) for r in regions]
    want = [Fold(PRE, BANDS, 3, a.shape[2:]) for a in accs]
    want_ref = [Fold(PRE, BANDS, 3, a.shape[2:]) for a in accs]
    for k, n in enumerate(SAMPLES):  # (v40 steps in triples: run(n, 3) between the samples)
        bin = k // 2
        for i, r in enumerate(regions):
            want[i].add(obj.get_region(1, *r), bin)
            accs[i].add(bin)
            want_ref[i].add(sampled.ref_u[n][_slices(r)], bin)
        obj.run(n, 3)
    inner = _inner(N)
    for i, r in enumerate(regions):
        _same(accs[i], want[i], (kind, sampled.prec, r), count=len(SAMPLES))
        e, s = accs[i].get()
        sel = inner[_slices(r)]
        assert np.array_equal(e[:, :, sel], want_ref[i].E[:, :, sel]) and np.array_equal(s[:, :, sel], want_ref[i].state[:, :, sel]) and e.max() > 0, (kind, "oracle", r)
    out, after = sd.u_out.copy(), obj.save_state()
    obj.close()
    sampled.check_end(out, after, f"{kind} after band accumulators")


# ---- 5. a chain inside a pair takes no sample -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_thread", [False, True], ids=["slab_threads", "one_thread"])
def test_a_chain_inside_a_pair_takes_no_sample(one_thread):
    sd = sim_data.SimData.from_sim(synth.shoebox(**PAIRS_KW), "single", build_mask=False)
    sd.scale_input()
    flags = engine.PF_MULTI_FORCE_PAIRS | engine.PF_MULTI_NO_TRIPLES | (engine.PF_MULTI_ONE_THREAD if one_thread else 0)
    m = engine.HipMulti(sd, [0, 0], multi_flags=flags, air_variant=40, verify_exchange=2)
    assert m.slab(0)["steps_per_pass"] == 2 and m.slab(1)["steps_per_pass"] == 2
    r = ([1, 1, 1], [sd.Nx - 1, sd.Ny - 1, sd.Nz - 1], [3, 1, 5])  # both slabs hold cells of it
    acc = m.band_accumulator(*r, pre_sos=PRE, band_sos=BANDS, nbin=3, depth=4)
    want = Fold(PRE, BANDS, 3, acc.shape[2:])
    taken, refused = [], []
    for n in range(12):
        try:
            acc.add(n // 4)
        except engine.PfError as e:
            assert e.code == 4 and "PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES" in str(e), str(e)
            refused.append(n)
        else:
            taken.append(n)
            want.add(m.get_region(1, *r), n // 4)
            _same(acc, want, n)  # (whatever a refused add before it had done would show here)
        assert acc.count == len(taken)
        m.run(n, 1)
    assert taken == list(range(0, 12, 2)) and refused == list(range(1, 12, 2)), (taken, refused)
    _same(acc, want, "end")
    assert want.E.max() > 0
    m.run(12, sd.Nt - 12)
    ref = sim_data.SimData.from_sim(synth.shoebox(**PAIRS_KW), "single")
    ref.scale_input()
    oracle.run_sim(ref)
    assert np.array_equal(sd.u_out, ref.u_out)
    m.close()


# ---- 6. sums equal receivers ---------------------------------------------------------------------------------------------------------------------------
def test_sums_equal_receivers():
    sd = cases.make_sd("cart_outside", "double")
    rcv = [(24, 22, 20), (2, 23, 3), (12, 12, 12)]
    rows = [[int(v) for v in sd.out_ixyz].index((x * sd.Ny + y) * sd.Nz + z) for x, y, z in rcv]
    step_bin = 8
    nbin = -(-sd.Nt // step_bin)
    eng = engine.HipEngine(sd)
    accs = [eng.band_accumulator([x, y, z], [x + 1, y + 1, z + 1], pre_sos=PRE, band_sos=BANDS, nbin=nbin) for x, y, z in rcv]
    for n in range(sd.Nt):
        for a in accs:
            a.add(n // step_bin)
        eng.run(n, 1)
    got = [a.get() for a in accs]
    eng.close()
    ref = cases.make_sd("cart_outside", "double")
    oracle.run_sim(ref)
    assert np.array_equal(sd.u_out, ref.u_out)
    live = 0
    for row, (e, s) in zip(rows, got):
        want = Fold(PRE, BANDS, nbin, (1, 1, 1))
        for n in range(sd.Nt):
            want.add(sd.u_out[row, n].reshape(1, 1, 1), n // step_bin)  # the raw row: u^n of the receiver's cell
        assert np.array_equal(e, want.E) and np.array_equal(s, want.state), row
        live += want.E.max() > 0
    assert live >= 2  # (the receiver inside the closed box hears nothing: the source stands outside)


# ---- 7. continue from saved sums and filter state ----------------------------------------------------------------------------------------------------
def test_a_resumed_run_continues_sums_and_state():
    r = ([3, 1, 2], [26, 20, 22], [1, 2, 3])
    kw = dict(pre_sos=PRE, band_sos=BANDS, nbin=5, depth=4)

    def run(eng, acc, n0, n1):
        for n in range(n0, n1):
            acc.add(n // 4)
            eng.run(n, 1)

    sd = cases.make_sd("cart_mb11", "single")
    eng = engine.HipEngine(sd)
    acc = eng.band_accumulator(*r, **kw)
    run(eng, acc, 0, 20)
    whole = acc.get()
    eng.close()
    sd = cases.make_sd("cart_mb11", "single")
    eng = engine.HipEngine(sd)
    acc = eng.band_accumulator(*r, **kw)
    run(eng, acc, 0, 9)
    (sums, fstate), count, state = acc.get(), acc.count, eng.save_state()
    eng.close()  # (destroys the accumulator with it)
    assert count == 9 and np.abs(fstate).max() > 0
    results = []
    for restore in (True, False):
        sd = cases.make_sd("cart_mb11", "single")
        eng = engine.HipEngine(sd)
        eng.load_state(state)
        acc = eng.band_accumulator(*r, **kw)
        acc.add(0)  # a pending sample: set drops it
        acc.set(sums, fstate if restore else None, count)
        assert acc.count == 9
        run(eng, acc, 9, 20)
        results.append(acc.get())
        assert acc.count == 20
        eng.close()
    assert np.array_equal(results[0][0], whole[0]) and np.array_equal(results[0][1], whole[1])
    assert not np.array_equal(results[1][0], whole[0])  # the control: with the filter state zeroed at set a sum differs


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_field_and_leave_the_engine_running():
    sd = cases.make_sd("cart_mb11", "single")
    other_sd = cases.make_sd("cart_mb11", "single")
    eng, other = engine.HipEngine(sd), engine.HipEngine(other_sd)
    N = [sd.Nx, sd.Ny, sd.Nz]
    ok = dict(pre_sos=PRE, band_sos=BANDS, nbin=2)
    nine = np.repeat(PRE, 9, axis=0)
    bad = BANDS.copy()
    bad[1, 0, 4] = np.inf
    for kw, field in ((dict(band_sos=np.zeros((0, 2, 6))), "nband"), (dict(band_sos=np.repeat(BANDS, 6, axis=0)[:17]), "nband"), (dict(pre_sos=nine), "npre"),
                      (dict(band_sos=np.repeat(BANDS, 5, axis=1)[:, :9]), "nsec"), (dict(nbin=0), "nbin"), (dict(depth=17), "depth"), (dict(depth=-1), "depth"),
                      (dict(band_sos=bad), "band_sos[1][0][3]"), (dict(pre_sos=PRE * np.array([1, 1, np.nan, 1, 1, 1])), "pre_sos[0][2]")):
        with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
            eng.band_accumulator([0, 0, 0], N, **{**ok, **kw})
        assert ei.value.code == 1 and field in str(ei.value), str(ei.value)
    with pytest.raises(engine.PfError, match="a0"):
        eng.band_accumulator([0, 0, 0], N, **{**ok, "pre_sos": PRE * 2.0})
    for lo, hi, st, field in (([0, 0, 0], [N[0], N[1] + 1, N[2]], [1, 1, 1], "hi[1]"), ([0, 0, 0], N, [1, 0, 1], "stride[1]"), ([-1, 0, 0], N, [1, 1, 1], "lo[0]")):
        with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
            eng.band_accumulator(lo, hi, st, **ok)
        assert field in str(ei.value), str(ei.value)
    L = engine.lib()
    vp = ctypes.c_void_p
    r = engine.PfRegion((ctypes.c_int64 * 3)(0, 0, 0), (ctypes.c_int64 * 3)(*N), (ctypes.c_int64 * 3)(1, 1, 1))
    h = vp()
    sq = (None, 0, None)  # plain squares: no sections at all
    assert L.pf_engine_bandacc_create(eng._h, None, 0, None, 1, 0, None, 1, 0, ctypes.byref(h)) == 1 and b"null pf_region" in L.pf_last_error()
    assert L.pf_engine_bandacc_create(eng._h, ctypes.byref(r), 0, None, 1, 0, None, 1, 0, None) == 1 and b"null out" in L.pf_last_error()
    assert L.pf_engine_bandacc_create(None, ctypes.byref(r), 0, None, 1, 0, None, 1, 0, ctypes.byref(h)) == 1 and b"null engine" in L.pf_last_error()
    assert L.pf_engine_bandacc_create(eng._h, ctypes.byref(r), 1, None, 1, 0, None, 1, 0, ctypes.byref(h)) == 1 and b"null pre_sos" in L.pf_last_error()
    assert L.pf_engine_bandacc_create(eng._h, ctypes.byref(r), 0, None, 1, 1, None, 1, 0, ctypes.byref(h)) == 1 and b"null band_sos" in L.pf_last_error()
    assert L.pf_multi_bandacc_create(None, ctypes.byref(r), 0, None, 1, 0, None, 1, 0, ctypes.byref(h)) == 1
    acc = eng.band_accumulator([0, 0, 0], N, band_sos=np.zeros((2, 0, 6)), nbin=2)
    assert (acc.npre, acc.nband, acc.nsec) == (0, 2, 0) and acc.state_shape[0] == 0
    buf = np.empty(acc.shape)
    bp = buf.ctypes.data_as(vp)
    for bin in (-2, 2):
        assert L.pf_engine_bandacc_add(eng._h, acc._a, bin) == 1 and b"bin" in L.pf_last_error()
    assert L.pf_engine_bandacc_add(eng._h, None, 0) == 1 and b"null pf_bandacc" in L.pf_last_error()
    assert L.pf_engine_bandacc_get(eng._h, acc._a, None, None) == 1 and b"null sums" in L.pf_last_error()
    assert L.pf_engine_bandacc_get(eng._h, None, bp, None) == 1 and b"null pf_bandacc" in L.pf_last_error()
    assert L.pf_engine_bandacc_set(eng._h, None, None, None, 0) == 1 and b"null pf_bandacc" in L.pf_last_error()
    assert L.pf_engine_bandacc_set(eng._h, acc._a, None, None, -1) == 1 and b"count" in L.pf_last_error()
    assert L.pf_engine_bandacc_destroy(eng._h, None) == 1 and L.pf_bandacc_count(None) < 0
    for call in (lambda: L.pf_engine_bandacc_add(other._h, acc._a, 0), lambda: L.pf_engine_bandacc_get(other._h, acc._a, bp, None),
                 lambda: L.pf_engine_bandacc_set(other._h, acc._a, None, None, 0), lambda: L.pf_engine_bandacc_destroy(other._h, acc._a)):
        assert call() == 1 and b"another engine" in L.pf_last_error()
    assert acc.count == 0
    # split-phase steps: refused inside one, valid between them
    steps = 5
    for n in range(steps):
        eng.step_begin(n)
        if n == 2:
            for f in (lambda: acc.add(0), acc.get, lambda: acc.set(None, None, 0)):
                with pytest.raises(engine.PfError, match="pffdtd_hip error 4") as ei:
                    f()
                assert ei.value.code == 4
        eng.step_end(n)
    assert acc.count == 0
    acc.add(1)
    u = eng.get_region(1, [0, 0, 0], N).astype(np.float64)
    e, s = acc.get()
    assert np.array_equal(e[:, 1], np.stack([u * u, u * u])) and not e[:, 0].any() and acc.count == 1 and e.max() > 0 and s.size == 0
    # a one-rank cost model has no field of the scene
    m = engine.HipMulti(cases.make_sd("cart_mb11", "single"), [0, 0], only_slab=1)
    with pytest.raises(engine.PfError, match="pffdtd_hip error 4") as ei:
        m.band_accumulator([0, 0, 0], N, **ok)
    assert ei.value.code == 4 and "only_slab" in str(ei.value)
    m.close()
    # the engine with the energy diagnostic answers
    sd2 = cases.make_sd("cart_mb11", "double")
    en = engine.HipEngine(sd2, energy=True)
    en.energy_cfg(sd2.h, sd2.c, sd2.Ts, sd2.DEF)
    en.run_energy(0, 9, np.zeros(sd2.Nt), np.zeros(sd2.Nt + 1), np.zeros(sd2.Nt + 1))
    a2 = en.band_accumulator([3, 1, 2], [26, 20, 22], [1, 2, 3], band_sos=np.zeros((1, 0, 6)), nbin=1)
    a2.add(0)
    g = en.get_grid(1)[3:26:1, 1:20:2, 2:22:3]
    assert np.array_equal(a2.get()[0][0, 0], g * g) and a2.get()[0].any()
    en.close()
    # the engine still runs to the oracle's receivers
    eng.run(steps, sd.Nt - steps)
    ref = cases.make_sd("cart_mb11", "single")
    oracle.run_sim(ref)
    assert np.array_equal(sd.u_out, ref.u_out) and np.abs(ref.u_out).max() > 0
    eng.close()
    other.close()


# ---- 9. the scalar kind is the vector kind with one component ---------------------------------------------------------------------------------------------
PRE2 = np.concatenate([PRE, butter(2, 0.03, "high", output="sos")])  # npre = 2
assert PRE2.shape == (2, 6)


@pytest.mark.parametrize("owner", ["engine", "chain2"])
@pytest.mark.parametrize("name,prec", [("cart_mb11", "single"), ("fcc2_outside", "double")])
def test_the_scalar_kind_is_the_vector_kind_with_one_component(name, prec, owner):
    """A band_accumulator and a vector_band_accumulator(comp=(0,), prod=((0, 0, 0),)) of the same owner, sections and depth 8 return the same bits
    after 20 samples (the bin changes every 3 samples, one sample goes to bin -1), for npre 0 and 2, over 5 x 3 x 7 = 105 cells (an odd count: the
    padding cell of the last double2) and over more than one block of 512 cells: 24 x 18 x 20 = 8640 cells on cart_mb11; fcc2_outside is folded to
    30 x 17 x 26, where 18 cells along y do not exist, so its large region is 28 x 15 x 24 = 10080 cells."""
    sd = cases.make_sd(name, prec)
    N = (sd.Nx, sd.Ny, sd.Nz)
    if owner == "engine":
        obj = engine.HipEngine(sd)
    else:
        obj = engine.HipMulti(sd, [0, 0], multi_flags=engine.PF_MULTI_NO_PAIRS | engine.PF_MULTI_NO_TRIPLES)
        assert obj.info()["nslabs"] == 2
    x0 = N[0] // 2 - 2  # (around the middle plane: both slabs of the chain hold cells of it)
    small = ([x0, 2, 3], [x0 + 5, 5, 10])
    large, large_cells = (([1, 1, 1], [25, 19, 21]), 8640) if name == "cart_mb11" else (([1, 1, 1], [29, 16, 25]), 10080)
    pairs = []
    for npre in (0, 2):
        for r, cells in ((small, 105), (large, large_cells)):
            kw = dict(band_sos=BANDS, nbin=7, depth=8)
            s = obj.band_accumulator(*r, pre_sos=PRE2[:npre] if npre else None, **kw)
            v = obj.vector_band_accumulator(*r, comp=(0,), pre_sos=PRE2[None, :npre] if npre else None, prod=((0, 0, 0),), **kw)
            assert (s.npre, v.npre) == (npre, npre) and (v.ncomp, v.nprod) == (1, 1)
            assert int(np.prod(s.shape[2:])) == cells
            assert v.shape == (1,) + s.shape and v.state_shape == (1,) + s.state_shape
            pairs.append((npre, r, s, v))
    obj.run(0, 12)  # (the wave has reached both regions)
    for k in range(20):
        bin = -1 if k == 10 else k // 3
        for _, _, s, v in pairs:
            s.add(bin)
            v.add(bin)
        obj.run(12 + k, 1)
    for npre, r, s, v in pairs:
        (es, ss), (ev, sv) = s.get(), v.get()
        assert s.count == 20 and v.count == 20
        assert np.array_equal(ev.reshape(es.shape), es), (npre, r, "sums", int(np.count_nonzero(ev.reshape(es.shape) != es)))
        assert np.array_equal(sv.reshape(ss.shape), ss), (npre, r, "state", int(np.count_nonzero(sv.reshape(ss.shape) != ss)))
        assert es[:, 6].max() > 0 and np.abs(ss).max() > 0 and np.isfinite(es).all()
    obj.close()
