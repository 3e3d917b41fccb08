"""GPU: vector band accumulators (pf_engine_vband_* / pf_multi_vband_*, kernels k_region_diff / k_vband_pre / k_vband_fold): per cell of a region up
to four components -- the cell of u^n or its central difference along a file axis, one subtraction in the field's own precision -- run through
second-order sections, and products of two filtered components are summed into time bins, on the device.

The bar: sums and filter state are bit for bit those of VFold, a numpy loop over time, vectorised over cells, written with the contract's lines
    d_a = u[c + e_a] - u[c - e_a]   (the field's dtype);   y = b0*x + s1;   s1 = (b1*x - a1*y) + s2;   s2 = b2*x - a2*y;   S = S + y_i * y_j  (or + |y_i * y_j|)
over the frames get_region(1, ...) gives for the region widened by one cell at the same moments, and over the oracle's fields inside; the depth of the
ring and the greedy pieces of a fold change no bit; asking changes nothing.  Every comparison is np.array_equal.  (This file sorts behind
tests/test_hip_autotune.py: see tests/test_hip_spectra_engines.py for why its chains of three slabs must.)
"""
import ctypes

import numpy as np
import pytest

import cases
import oracle
from pffdtd_amd import engine, sim_data, synth
from test_hip_accum import KERNEL_N, KERNEL_REGIONS
from test_hip_bandacc import BANDS, PRE, Fold
from test_hip_region import PAIRS_KW, _regions, _slices
from test_hip_spectra_engines import SAMPLES
from test_hip_spectra_engines import sampled  # noqa: F401  (the module-scoped fixture: the scene, its oracle trajectory, the five makers)

pytestmark = pytest.mark.gpu

COMP4 = (0, 1, 2, 3)  # u, d_x, d_y, d_z
PROD5 = [(0, 0, 0), (2, 2, 0), (0, 2, 0), (0, 2, 1), (1, 3, 0)]


def _widened(r, comp):
    """the region of the cells actually read: one cell more on both sides along every difference axis, stride 1 there unless the region's is 1 or 2"""
    lo, hi, st = [list(v) for v in r]
    for a in comp:
        if a:
            last = lo[a - 1] + (hi[a - 1] - lo[a - 1] - 1) // st[a - 1] * st[a - 1]
            lo[a - 1], hi[a - 1], st[a - 1] = lo[a - 1] - 1, last + 2, 1
    return lo, hi, st


def _components(frame, r, comp):
    """frame: the field over _widened(r, comp) -> the components over r, each in the field's dtype (one subtraction)"""
    st = r[2]
    base = []
    for a in range(3):
        if (a + 1) in comp:
            n = (frame.shape[a] - 3) // st[a] + 1
            base.append((1, n, st[a]))
        else:
            base.append((0, frame.shape[a], 1))
    out = []
    for k in comp:
        def sl(shift):
            return tuple(slice(b0 + (shift if a == k - 1 else 0), b0 + (shift if a == k - 1 else 0) + (n - 1) * s + 1, s) for a, (b0, n, s) in enumerate(base))
        out.append(frame[sl(0)] if k == 0 else frame[sl(1)] - frame[sl(-1)])
        assert out[-1].dtype == frame.dtype
    return out


def _of_grid(u, r, comp):
    """the components over r from a whole grid in file order"""
    w = _widened(r, comp)
    return _components(u[_slices(w)], r, comp)


class VFold:
    """the reference: a numpy loop over time, vectorised over cells, the contract's association"""

    def __init__(self, ncomp, pre, bands, prod, nbin, cells):
        self.pre = np.asarray(pre, dtype=np.float64).reshape(ncomp, -1, 6)
        self.bands = np.asarray(bands, dtype=np.float64)
        self.nband, self.nsec, self.npre = self.bands.shape[0], self.bands.shape[1], self.pre.shape[1]
        self.prod = [tuple(int(v) for v in p) for p in prod]
        self.S = np.zeros((len(self.prod), self.nband, nbin) + tuple(cells))
        self.state = np.zeros((ncomp, self.npre + self.nband * self.nsec, 2) + tuple(cells))

    def _section(self, k, s, x):
        y = k[0] * x + s[0]
        s[0] = (k[1] * x - k[4] * y) + s[1]
        s[1] = k[2] * x - k[5] * y
        return y

    def add(self, comps, bin):
        xs = []
        for c, u in enumerate(comps):
            x = u.astype(np.float64)
            for q in range(self.npre):
                x = self._section(self.pre[c, q], self.state[c, q], x)
            xs.append(x)
        for b in range(self.nband):
            ys = []
            for c, x in enumerate(xs):
                y = x
                for s in range(self.nsec):
                    y = self._section(self.bands[b, s], self.state[c, self.npre + b * self.nsec + s], y)
                ys.append(y)
            if bin >= 0:
                for p, (i, j, mode) in enumerate(self.prod):
                    self.S[p, b, bin] = self.S[p, b, bin] + (np.fabs(ys[i] * ys[j]) if mode else ys[i] * ys[j])


def _same(acc, ref, label, count=None):
    e, s = acc.get()
    assert e.dtype == np.float64 and e.shape == ref.S.shape and s.shape == ref.state.shape, label
    assert np.array_equal(e, ref.S), (label, "sums", int(np.count_nonzero(e != ref.S)))
    assert np.array_equal(s, ref.state), (label, "state", int(np.count_nonzero(s != ref.state)))
    if count is not None:
        assert acc.count == count, label


def _clear(r, N, comp=COMP4):
    """does the region keep one cell clear of both faces along the difference axes?"""
    lo, hi, st = r
    for a in comp:
        if a:
            last = lo[a - 1] + (hi[a - 1] - lo[a - 1] - 1) // st[a - 1] * st[a - 1]
            if lo[a - 1] < 1 or last > N[a - 1] - 2:
                return False
    return True


def _pre_per(comp, pre=PRE):
    return np.stack([pre] * len(comp))


# ---- 1. the small scenes: frames, the oracle, and the run goes on ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec", [("cart_outside", "double"), ("cart_mb11", "single")])
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
    regions = [r for r in _regions(N) if _clear(r, N)]
    regions.append(([2, 1, 2], [N[0] - 1, N[1] - 1, N[2] - 1], [2, 1, 3]))  # a strided box around the source, clear of the faces on every scene
    for a in range(3):  # the planes at index 1 and N - 2: the widened region holds a face cell, which forces the ghost shell
        for k in (1, N[a] - 2):
            lo, hi = [1, 1, 1], [N[0] - 1, N[1] - 1, N[2] - 1]
            lo[a], hi[a] = k, k + 1
            regions.append((lo, hi, [1, 1, 1]))
    assert len(regions) >= 7
    nbin = -(-(nsteps - 4) // step_bin)
    eng = engine.HipEngine(sd)
    pre = _pre_per(COMP4)
    accs = [eng.vector_band_accumulator(*r, comp=COMP4, pre_sos=pre, band_sos=BANDS, prod=PROD5, nbin=nbin) for r in regions]
    want = [VFold(4, pre, BANDS, PROD5, nbin, a.shape[3:]) for a in accs]
    want_ref = [VFold(4, pre, BANDS, PROD5, nbin, a.shape[3:]) for a in accs]
    eng.run(0, 2)
    for n in range(2, nsteps):  # every step from 2; the first two samples only run the filters
        bin = -1 if n < 4 else (n - 4) // step_bin
        for i, r in enumerate(regions):
            frame = eng.get_region(1, *_widened(r, COMP4))  # before add: the same moment
            accs[i].add(bin)
            want[i].add(_components(frame, r, COMP4), bin)
            want_ref[i].add(_of_grid(ref_u[n], r, COMP4), bin)
        eng.run(n, 1)
    wide_inner = np.zeros(N, dtype=bool)
    wide_inner[2:-2, 2:-2, 2:-2] = True  # cells whose neighbours are inside too
    for i, r in enumerate(regions):
        _same(accs[i], want[i], (name, r), count=nsteps - 2)
        e, s = accs[i].get()
        sel = wide_inner[_slices(r)]
        assert np.array_equal(e[:, :, :, sel], want_ref[i].S[:, :, :, sel]) and np.array_equal(s[:, :, :, sel], want_ref[i].state[:, :, :, sel]), (name, "oracle", r)
    assert max(w.S.max() for w in want) > 0 and all(np.isfinite(w.S).all() for w in want)
    assert min(w.S[4].min() for w in want) < 0  # (a plain product of two differences takes both signs)
    eng.run(nsteps, sd.Nt - nsteps)  # nothing a later step reads has changed
    for n in range(nsteps, ref_sd.Nt):
        ref.step(n)
    assert np.array_equal(sd.u_out, ref_sd.u_out) and np.abs(ref_sd.u_out).max() > 0
    eng.close()
    ref.close()


@pytest.mark.parametrize("name", ["fcc2_outside", "fcc1_outside"])
def test_fcc_grids_take_the_cell_alone(name):
    sd = cases.make_sd(name, "double")
    N = (sd.Nx, sd.Ny, sd.Nz)
    eng = engine.HipEngine(sd)
    r = ([3, 1, 2], [min(29, N[0]), min(27, N[1]), min(25, N[2])], [1, 2, 3])
    v = eng.vector_band_accumulator(*r, comp=(0,), pre_sos=PRE[None], band_sos=BANDS, prod=[(0, 0, 0)], nbin=3)
    b = eng.band_accumulator(*r, pre_sos=PRE, band_sos=BANDS, nbin=3)
    for a in (1, 2, 3):
        with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
            eng.vector_band_accumulator(*r, comp=(0, a), pre_sos=_pre_per((0, a)), band_sos=BANDS, prod=[(0, 1, 0)], nbin=3)
        assert "comp" in str(ei.value) and "fcc_flag" in str(ei.value), str(ei.value)
    for n in range(12):
        v.add(n // 4)
        b.add(n // 4)
        eng.run(n, 1)
    (vs, vst), (bs, bst) = v.get(), b.get()
    assert np.array_equal(vs[0], bs) and np.array_equal(vst[0], bst) and bs.max() > 0
    eng.close()


# ---- 2. the kernel alone: fields with a denormal, a -0.0, a large value, a difference that cancels and one that is itself denormal ----------------
@pytest.mark.parametrize("layout", [engine.PF_LAYOUT_FILE, engine.PF_LAYOUT_EXCHANGED], ids=["file_order", "exchanged"])
@pytest.mark.parametrize("prec", ["single", "double"])
def test_three_samples_are_the_exact_cascade(prec, layout):
    sd = sim_data.SimData.from_sim(synth.shoebox(*KERNEL_N, Nt=4, Nm=1, Mb=3), prec, build_mask=False)
    sd.scale_input()
    dt = np.float32 if prec == "single" else np.float64
    tiny = np.finfo(dt).tiny
    rng = np.random.default_rng(97)
    state = engine._state_arrays(sd)[0]
    state["u_prev"] = rng.standard_normal(KERNEL_N).astype(dt)
    fields = []
    for k in range(3):
        u = rng.standard_normal(KERNEL_N).astype(dt)
        u[5, 5, 5 + k % 2] = dt(1e-40) if prec == "single" else dt(1e-310)  # a denormal of the field's format
        u[5, 5, 6 - k % 2] = dt(-0.0)
        u[5, 5, 9] = dt(2.0 ** 60) if prec == "single" else dt(2.0 ** 500)  # (its square is finite in double; the sections below never amplify)
        u[5, 4, 20] = u[5, 6, 20] = dt(0.75)  # d_y of (5, 5, 20) cancels to exactly 0
        u[5, 5, 29], u[5, 5, 31] = dt(1.5) * tiny, dt(1.25) * tiny  # d_z of (5, 5, 30) is itself denormal
        assert u[5, 5, 5 + k % 2] != 0 and abs(u[5, 5, 5 + k % 2]) < tiny
        assert u[5, 6, 20] - u[5, 4, 20] == 0 and 0 < u[5, 5, 29] - u[5, 5, 31] < tiny
        fields.append(u)
    # sections whose gain stays below 1 over three samples: |b|, |a| <= 0.3 (no inf - inf, so no NaN reaches array_equal)
    pre8 = np.concatenate([rng.uniform(-0.3, 0.3, (4, 8, 3)), np.ones((4, 8, 1)), rng.uniform(-0.3, 0.3, (4, 8, 2))], axis=2)
    band16 = np.concatenate([rng.uniform(-0.3, 0.3, (16, 8, 3)), np.ones((16, 8, 1)), rng.uniform(-0.3, 0.3, (16, 8, 2))], axis=2)
    comps = {1: (0,), 2: (3, 0), 4: (2, 0, 3, 1)}
    prods = {1: [(0, 0, 1), (0, 0, 0)] * 5, 2: [(0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (1, 1, 0)],
             4: [(0, 2, 0), (1, 3, 1), (2, 2, 0), (3, 0, 1), (1, 1, 0), (0, 0, 1), (3, 3, 0), (2, 1, 1), (0, 1, 0), (2, 3, 0)]}
    eng = engine.HipEngine(sd, layout=layout)
    assert eng.layout()[2] == (layout == engine.PF_LAYOUT_EXCHANGED)
    cfg = [(ncomp, nband, nsec, npre, nprod) for ncomp in (1, 2, 4) for nband in (1, 16) for nsec in (0, 1, 8) for npre in (0, 8) for nprod in (1, 10)
           if (nband == 1) == (nprod == 1) or nsec == 1]  # (nband and nprod together, and crossed at one section count)
    accs, want = [], []
    for ncomp, nband, nsec, npre, nprod in cfg:
        comp = comps[ncomp]
        for r in KERNEL_REGIONS:
            pre, bands, prod = pre8[:ncomp, :npre], band16[:nband, :nsec], prods[ncomp][:nprod]
            a = eng.vector_band_accumulator(*r, comp=comp, pre_sos=pre, band_sos=bands, prod=prod, nbin=2)
            assert (a.ncomp, a.npre, a.nband, a.nsec, a.nprod) == (ncomp, npre, nband, nsec, nprod) and a.count == 0 and not a.get()[0].any()
            accs.append(a)
            want.append((VFold(ncomp, pre, bands, prod, 2, a.shape[3:]), r, comp, (ncomp, nband, nsec, npre, nprod)))
    for k, bin in enumerate((0, 1, 1)):  # a bin change inside the fold, then two samples of one bin
        state["u_cur"] = fields[k]
        eng.load_state(state)
        for a, (w, r, comp, _) in zip(accs, want):
            a.add(bin)
            w.add(_of_grid(fields[k], r, comp), bin)
    for a, (w, r, comp, c) in zip(accs, want):
        assert np.isfinite(w.S).all() and np.isfinite(w.state).all()
        _same(a, w, (prec, c, r), count=3)
    # the special cells, in a region that holds them: the differences themselves (no sections, |d * d|)
    r = ([5, 5, 3], [6, 6, 66], [1, 1, 1])
    a = eng.vector_band_accumulator(*r, comp=(2, 3), band_sos=np.zeros((1, 0, 6)), prod=[(0, 0, 0), (1, 1, 0)], nbin=1, depth=1)
    a.add(0)
    s = a.get()[0]
    dz = float(fields[2][5, 5, 31] - fields[2][5, 5, 29])
    assert s[0, 0, 0, 0, 0, 20 - 3] == 0.0 and s[1, 0, 0, 0, 0, 30 - 3] == dz * dz and dz != 0
    assert s[1, 0, 0, 0, 0, 30 - 3] != 0 or prec == "double"  # (the fp32 denormal survived the conversion; 1e-308 ** 2 underflows in any arithmetic)
    eng.close()


# ---- 3. the depth of the ring and the greedy pieces of a fold change no bit ---------------------------------------------------------------------------
def test_depth_changes_no_bit():
    sd = cases.make_sd("cart_mb11", "single")
    N = (sd.Nx, sd.Ny, sd.Nz)
    regions = [([3, 1, 2], [25, 19, 21], [1, 2, 3]), ([1, 1, 11], [N[0] - 1, N[1] - 1, 12], [1, 1, 1])]
    eng = engine.HipEngine(sd)
    depths = (1, 3, 5, 7, 8)
    comp, prod = (0, 2, 3), [(0, 0, 0), (0, 1, 0), (1, 2, 1)]
    pre = _pre_per(comp)
    accs = {(d, i): eng.vector_band_accumulator(*r, comp=comp, pre_sos=pre, band_sos=BANDS, prod=prod, nbin=4, depth=d) for d in depths for i, r in enumerate(regions)}
    want = [VFold(3, pre, BANDS, prod, 4, accs[(1, i)].shape[3:]) for i in range(len(regions))]
    eng.run(0, 20)
    for s in range(11):
        n = 20 + s
        bin = s // 3  # bins of 3 steps: they change inside the folds
        for i, r in enumerate(regions):
            want[i].add(_components(eng.get_region(1, *_widened(r, comp)), r, comp), bin)
        for a in accs.values():
            a.add(bin)
        if s == 6:  # after the seventh sample: 1 pending at depth 3, 2 at depth 5 (one piece), 7 at depth 8 (4 + 2 + 1), none at depth 7
            for (d, i), a in accs.items():
                _same(a, want[i], (d, i, "mid-run"), count=7)
        eng.run(n, 1)
    for (d, i), a in accs.items():  # (3 pending at depth 8: 2 + 1; 1 at depth 5; 4 at depth 7)
        _same(a, want[i], (d, i), count=11)
    assert all(w.S.max() > 0 for w in want)
    eng.close()


# ---- 4. one component, one square: a band accumulator ---------------------------------------------------------------------------------------------------
def test_the_cell_alone_is_a_band_accumulator():
    sd = cases.make_sd("cart_mb11", "single")
    eng = engine.HipEngine(sd)
    r = ([3, 1, 2], [25, 19, 21], [1, 2, 3])
    v = eng.vector_band_accumulator(*r, comp=(0,), pre_sos=PRE[None], band_sos=BANDS, prod=[(0, 0, 0)], nbin=5, depth=3)
    b = eng.band_accumulator(*r, pre_sos=PRE, band_sos=BANDS, nbin=5, depth=4)
    for n in range(20):
        v.add(n // 4)
        b.add(n // 4)
        eng.run(n, 1)
    (vs, vst), (bs, bst) = v.get(), b.get()
    assert vs.shape == (1,) + bs.shape and vst.shape == (1,) + bst.shape
    assert np.array_equal(vs[0], bs) and np.array_equal(vst[0], bst) and bs.max() > 0 and v.count == b.count == 20
    eng.close()


# ---- 5. engines that share no kernel, layout or decomposition ----------------------------------------------------------------------------------------
def _cut_regions(N):
    """a box across every cut of both chains (x and z), the planes on both sides of every possible cut with the difference ALONG the cut axis: the
    cuts of chain3 (x) and chain2z (z) are read from the chains themselves in the test; these are the regions every engine takes"""
    return [([1, 2, 1], [N[0] - 1, N[1] - 2, N[2] - 1], [3, 1, 5]), ([2, 1, 3], [N[0] - 2, N[1] - 1, N[2] - 3], [1, 7, 1])]


CUTS = {}  # kind -> the chain's cuts, learned from the first chain made (the same for every precision's scene of one kind? no: keyed by (kind, prec))


def _chain_cuts(sampled, kind):  # noqa: F811
    key = (kind, sampled.prec)
    if key not in CUTS:
        obj, _ = sampled.make(kind)
        CUTS[key] = [obj.slab(g)["x0"] for g in range(1, obj.nslabs)]
        obj.close()
    return CUTS[key]


@pytest.mark.parametrize("kind", ["v25", "v40", "exchanged", "chain3", "chain2z"])
def test_sums_of_every_engine_and_chain(sampled, kind):  # noqa: F811
    N = sampled.n
    comp, prod = (0, 1, 3), [(0, 0, 0), (1, 1, 0), (0, 1, 0), (0, 2, 1), (2, 2, 0)]
    regions = [(r, comp) for r in _cut_regions(N)]
    for ck, a in (("chain3", 0), ("chain2z", 2)):  # the planes on both sides of every cut, the difference along the cut axis
        for x in _chain_cuts(sampled, ck):
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
    pr = [[p for p in prod if max(p[0], p[1]) < len(c)] for _, c in regions]
    accs = [obj.vector_band_accumulator(*r, comp=c, pre_sos=_pre_per(c), band_sos=BANDS, prod=p, nbin=3) for (r, c), p in zip(regions, pr)]
    want = [VFold(len(c), _pre_per(c), BANDS, p, 3, a.shape[3:]) for (r, c), p, a in zip(regions, pr, accs)]
    want_ref = [VFold(len(c), _pre_per(c), BANDS, p, 3, a.shape[3:]) for (r, c), p, a in zip(regions, pr, accs)]
    for k, n in enumerate(SAMPLES):  # (v40 steps in triples: run(n, 3) between the samples)
        bin = k // 2
        for i, (r, c) in enumerate(regions):
            want[i].add(_components(obj.get_region(1, *_widened(r, c)), r, c), bin)
            accs[i].add(bin)
            want_ref[i].add(_of_grid(sampled.ref_u[n], r, c), bin)
        obj.run(n, 3)
    wide_inner = np.zeros(N, dtype=bool)
    wide_inner[2:-2, 2:-2, 2:-2] = True
    got = []
    for i, (r, c) in enumerate(regions):
        _same(accs[i], want[i], (kind, sampled.prec, r), count=len(SAMPLES))
        e, s = accs[i].get()
        sel = wide_inner[_slices(r)]
        assert np.array_equal(e[..., sel], want_ref[i].S[..., sel]) and np.array_equal(s[..., sel], want_ref[i].state[..., sel]) and e.max() > 0, (kind, "oracle", r)
        got.append((e, s))
    # all five give the same arrays: the first kind's are kept and every later one is compared with them
    key = sampled.prec
    if key not in SHARED:
        SHARED[key] = got
    else:
        for (e, s), (e0, s0) in zip(got, SHARED[key]):
            assert np.array_equal(e, e0) and np.array_equal(s, s0), (kind, "against the first engine")
    out, after = sd.u_out.copy(), obj.save_state()
    obj.close()
    sampled.check_end(out, after, f"{kind} after vector band accumulators")


SHARED = {}


@pytest.mark.parametrize("one_thread", [False, True], ids=["slab_threads", "one_thread"])
def test_a_chain_inside_a_pair_takes_no_sample(one_thread):
    sd = sim_data.SimData.from_sim(synth.shoebox(**PAIRS_KW), "single", build_mask=False)
    sd.scale_input()
    flags = engine.PF_MULTI_FORCE_PAIRS | engine.PF_MULTI_NO_TRIPLES | (engine.PF_MULTI_ONE_THREAD if one_thread else 0)
    m = engine.HipMulti(sd, [0, 0], multi_flags=flags, air_variant=40, verify_exchange=2)
    assert m.slab(0)["steps_per_pass"] == 2 and m.slab(1)["steps_per_pass"] == 2
    r = ([1, 1, 1], [sd.Nx - 1, sd.Ny - 1, sd.Nz - 1], [3, 1, 5])  # both slabs hold cells of it
    comp, prod = (0, 1), [(0, 1, 0), (1, 1, 0)]
    acc = m.vector_band_accumulator(*r, comp=comp, pre_sos=_pre_per(comp), band_sos=BANDS, prod=prod, nbin=3, depth=4)
    want = VFold(2, _pre_per(comp), BANDS, prod, 3, acc.shape[3:])
    taken, refused = [], []
    for n in range(12):
        try:
            acc.add(n // 4)
        except engine.PfError as e:
            assert e.code == 4 and "PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES" in str(e), str(e)
            refused.append(n)
        else:
            taken.append(n)
            want.add(_components(m.get_region(1, *_widened(r, comp)), r, comp), n // 4)
            _same(acc, want, n)  # (whatever a refused add before it had done would show here)
        assert acc.count == len(taken)
        m.run(n, 1)
    assert taken == list(range(0, 12, 2)) and refused == list(range(1, 12, 2)), (taken, refused)
    _same(acc, want, "end")
    assert want.S[1].max() > 0
    m.run(12, sd.Nt - 12)
    ref = sim_data.SimData.from_sim(synth.shoebox(**PAIRS_KW), "single")
    ref.scale_input()
    oracle.run_sim(ref)
    assert np.array_equal(sd.u_out, ref.u_out)
    m.close()


# ---- 6. the square of the cell equals the receivers' ------------------------------------------------------------------------------------------------------
def test_squares_equal_receivers():
    sd = cases.make_sd("cart_outside", "double")
    rcv = [(24, 22, 20), (2, 23, 3), (12, 12, 12)]
    rows = [[int(v) for v in sd.out_ixyz].index((x * sd.Ny + y) * sd.Nz + z) for x, y, z in rcv]
    step_bin = 8
    nbin = -(-sd.Nt // step_bin)
    eng = engine.HipEngine(sd)
    comp, prod = (2, 0), [(1, 1, 0), (0, 1, 0)]
    accs = [eng.vector_band_accumulator([x, y, z], [x + 1, y + 1, z + 1], comp=comp, pre_sos=_pre_per(comp), band_sos=BANDS, prod=prod, nbin=nbin) for x, y, z in rcv]
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
        assert np.array_equal(e[0], want.E) and np.array_equal(s[1], want.state), row
        live += want.E.max() > 0
    assert live >= 2  # (the receiver inside the closed box hears nothing: the source stands outside)


# ---- 7. continue from saved sums and filter state ----------------------------------------------------------------------------------------------------
def test_a_resumed_run_continues_sums_and_state():
    r = ([3, 1, 2], [25, 19, 21], [1, 2, 3])
    comp = (0, 2)
    kw = dict(comp=comp, pre_sos=_pre_per(comp), band_sos=BANDS, prod=[(0, 0, 0), (0, 1, 0), (0, 1, 1)], nbin=5, depth=4)

    def run(eng, acc, n0, n1):
        for n in range(n0, n1):
            acc.add(n // 4)
            eng.run(n, 1)

    sd = cases.make_sd("cart_mb11", "single")
    eng = engine.HipEngine(sd)
    acc = eng.vector_band_accumulator(*r, **kw)
    run(eng, acc, 0, 20)
    whole = acc.get()
    eng.close()
    sd = cases.make_sd("cart_mb11", "single")
    eng = engine.HipEngine(sd)
    acc = eng.vector_band_accumulator(*r, **kw)
    run(eng, acc, 0, 9)
    (sums, fstate), count, state = acc.get(), acc.count, eng.save_state()
    eng.close()  # (destroys the accumulator with it)
    assert count == 9 and np.abs(fstate).max() > 0
    results = []
    for restore in (True, False):
        sd = cases.make_sd("cart_mb11", "single")
        eng = engine.HipEngine(sd)
        eng.load_state(state)
        acc = eng.vector_band_accumulator(*r, **kw)
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
    lo1, hi1 = [1, 1, 1], [N[0] - 1, N[1] - 1, N[2] - 1]
    comp = (0, 2)
    ok = dict(comp=comp, pre_sos=_pre_per(comp), band_sos=BANDS, prod=[(0, 1, 0)], nbin=2)
    nine = np.repeat(_pre_per(comp), 9, axis=1)
    bad = BANDS.copy()
    bad[1, 0, 4] = np.inf
    badpre = _pre_per(comp).copy()
    badpre[1, 0, 2] = np.nan
    eleven = [(0, 1, 0)] * 11
    for kw, field in ((dict(band_sos=np.zeros((0, 2, 6))), "nband"), (dict(band_sos=np.repeat(BANDS, 6, axis=0)[:17]), "nband"), (dict(pre_sos=nine), "npre"),
                      (dict(band_sos=np.repeat(BANDS, 5, axis=1)[:, :9]), "nsec"), (dict(nbin=0), "nbin"), (dict(depth=9), "depth"), (dict(depth=-1), "depth"),
                      (dict(band_sos=bad), "band_sos[1][0][3]"), (dict(pre_sos=badpre), "pre_sos[1][0][2]"),
                      (dict(comp=(), pre_sos=None), "ncomp"), (dict(comp=(0, 1, 2, 3, 0), pre_sos=None), "ncomp"), (dict(comp=(0, 4)), "comp[1]"), (dict(comp=(0, -1)), "comp[1]"),
                      (dict(comp=(2, 2)), "repeated"), (dict(prod=[]), "nprod"), (dict(prod=eleven), "nprod"), (dict(prod=[(0, 2, 0)]), "prod[0][1]"),
                      (dict(prod=[(0, 0, 0), (-1, 0, 0)]), "prod[1][0]"), (dict(prod=[(0, 1, 2)]), "prod[0][2]")):
        with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
            eng.vector_band_accumulator(lo1, hi1, **{**ok, **kw})
        assert ei.value.code == 1 and field in str(ei.value), str(ei.value)
    with pytest.raises(engine.PfError, match="a0"):
        eng.vector_band_accumulator(lo1, hi1, **{**ok, "pre_sos": _pre_per(comp) * 2.0})
    for lo, hi, st, field in (([0, 0, 0], [N[0], N[1] + 1, N[2]], [1, 1, 1], "hi[1]"), ([0, 0, 0], N, [1, 0, 1], "stride[1]"), ([-1, 0, 0], N, [1, 1, 1], "lo[0]")):
        with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
            eng.vector_band_accumulator(lo, hi, st, **ok)
        assert field in str(ei.value), str(ei.value)
    # the one-cell rule, by the axis's name; the other axes may touch the faces
    for a, name in enumerate("xyz"):
        for lo, hi in (([0, 0, 0], list(N)), ):
            for side in (0, 1):
                l, h = list(lo), list(hi)
                if side == 0:
                    h[a] = N[a] - 1  # the first cell on the face
                else:
                    l[a] = 1  # the last cell on the face
                with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
                    eng.vector_band_accumulator(l, h, comp=(0, a + 1), pre_sos=_pre_per(comp), band_sos=BANDS, prod=[(0, 1, 0)], nbin=2)
                assert f"along file {name}" in str(ei.value) and f"lo[{a}]" in str(ei.value), str(ei.value)
        l, h = [0, 0, 0], list(N)
        l[a], h[a] = 1, N[a] - 1
        eng.vector_band_accumulator(l, h, comp=(0, a + 1), pre_sos=_pre_per(comp), band_sos=BANDS, prod=[(0, 1, 0)], nbin=1).close()
    L = engine.lib()
    vp = ctypes.c_void_p
    r = engine.PfRegion((ctypes.c_int64 * 3)(0, 0, 0), (ctypes.c_int64 * 3)(*N), (ctypes.c_int64 * 3)(1, 1, 1))
    h = vp()
    c0 = (ctypes.c_int32 * 1)(0)
    p0 = (ctypes.c_int32 * 3)(0, 0, 0)
    assert L.pf_engine_vband_create(eng._h, None, 1, c0, 0, None, 1, 0, None, 1, p0, 1, 0, ctypes.byref(h)) == 1 and b"null pf_region" in L.pf_last_error()
    assert L.pf_engine_vband_create(eng._h, ctypes.byref(r), 1, c0, 0, None, 1, 0, None, 1, p0, 1, 0, None) == 1 and b"null out" in L.pf_last_error()
    assert L.pf_engine_vband_create(None, ctypes.byref(r), 1, c0, 0, None, 1, 0, None, 1, p0, 1, 0, ctypes.byref(h)) == 1 and b"null engine" in L.pf_last_error()
    assert L.pf_engine_vband_create(eng._h, ctypes.byref(r), 1, None, 0, None, 1, 0, None, 1, p0, 1, 0, ctypes.byref(h)) == 1 and b"null comp" in L.pf_last_error()
    assert L.pf_engine_vband_create(eng._h, ctypes.byref(r), 1, c0, 0, None, 1, 0, None, 1, None, 1, 0, ctypes.byref(h)) == 1 and b"null prod" in L.pf_last_error()
    assert L.pf_engine_vband_create(eng._h, ctypes.byref(r), 1, c0, 1, None, 1, 0, None, 1, p0, 1, 0, ctypes.byref(h)) == 1 and b"null pre_sos" in L.pf_last_error()
    assert L.pf_engine_vband_create(eng._h, ctypes.byref(r), 1, c0, 0, None, 1, 1, None, 1, p0, 1, 0, ctypes.byref(h)) == 1 and b"null band_sos" in L.pf_last_error()
    assert L.pf_multi_vband_create(None, ctypes.byref(r), 1, c0, 0, None, 1, 0, None, 1, p0, 1, 0, ctypes.byref(h)) == 1
    acc = eng.vector_band_accumulator([0, 0, 0], N, comp=(0,), band_sos=np.zeros((2, 0, 6)), prod=[(0, 0, 0)], nbin=2)
    assert (acc.ncomp, acc.npre, acc.nband, acc.nsec) == (1, 0, 2, 0) and acc.state_shape[1] == 0
    buf = np.empty(acc.shape)
    bp = buf.ctypes.data_as(vp)
    for bin in (-2, 2):
        assert L.pf_engine_vband_add(eng._h, acc._a, bin) == 1 and b"bin" in L.pf_last_error()
    assert L.pf_engine_vband_add(eng._h, None, 0) == 1 and b"null pf_vbandacc" in L.pf_last_error()
    assert L.pf_engine_vband_get(eng._h, acc._a, None, None) == 1 and b"null sums" in L.pf_last_error()
    assert L.pf_engine_vband_get(eng._h, None, bp, None) == 1 and b"null pf_vbandacc" in L.pf_last_error()
    assert L.pf_engine_vband_set(eng._h, None, None, None, 0) == 1 and b"null pf_vbandacc" in L.pf_last_error()
    assert L.pf_engine_vband_set(eng._h, acc._a, None, None, -1) == 1 and b"count" in L.pf_last_error()
    assert L.pf_engine_vband_destroy(eng._h, None) == 1 and L.pf_vbandacc_count(None) < 0
    for call in (lambda: L.pf_engine_vband_add(other._h, acc._a, 0), lambda: L.pf_engine_vband_get(other._h, acc._a, bp, None),
                 lambda: L.pf_engine_vband_set(other._h, acc._a, None, None, 0), lambda: L.pf_engine_vband_destroy(other._h, acc._a)):
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
    assert np.array_equal(e[0, :, 1], np.stack([u * u, u * u])) and not e[0, :, 0].any() and acc.count == 1 and e.max() > 0 and s.size == 0
    # a one-rank cost model has no field of the scene
    m = engine.HipMulti(cases.make_sd("cart_mb11", "single"), [0, 0], only_slab=1)
    with pytest.raises(engine.PfError, match="pffdtd_hip error 4") as ei:
        m.vector_band_accumulator(lo1, hi1, **ok)
    assert ei.value.code == 4 and "only_slab" in str(ei.value)
    m.close()
    # a chain names the axis too, against the scene's faces
    m = engine.HipMulti(cases.make_sd("cart_mb11", "single"), [0, 0], multi_flags=engine.PF_MULTI_NO_PAIRS | engine.PF_MULTI_NO_TRIPLES)
    with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
        m.vector_band_accumulator([0, 1, 1], hi1, comp=(0, 1), pre_sos=_pre_per(comp), band_sos=BANDS, prod=[(0, 1, 0)], nbin=2)
    assert "along file x" in str(ei.value)
    m.close()
    # the engine with the energy diagnostic answers
    sd2 = cases.make_sd("cart_mb11", "double")
    en = engine.HipEngine(sd2, energy=True)
    en.energy_cfg(sd2.h, sd2.c, sd2.Ts, sd2.DEF)
    en.run_energy(0, 9, np.zeros(sd2.Nt), np.zeros(sd2.Nt + 1), np.zeros(sd2.Nt + 1))
    a2 = en.vector_band_accumulator([3, 1, 2], [25, 19, 21], [1, 2, 3], comp=(1,), band_sos=np.zeros((1, 0, 6)), prod=[(0, 0, 0)], nbin=1)
    a2.add(0)
    full = en.get_grid(1)
    g = full[4:26:1, 1:19:2, 2:21:3] - full[2:24:1, 1:19:2, 2:21:3]
    assert np.array_equal(a2.get()[0][0, 0, 0], g * g) and a2.get()[0].any()
    en.close()
    # the engine still runs to the oracle's receivers
    eng.run(steps, sd.Nt - steps)
    ref = cases.make_sd("cart_mb11", "single")
    oracle.run_sim(ref)
    assert np.array_equal(sd.u_out, ref.u_out) and np.abs(ref.u_out).max() > 0
    eng.close()
    other.close()
