"""GPU: the lattice-difference components of the vector band accumulators on FCC grids (comp 4 / 5 / 6 of pf_engine_vband_* / pf_multi_vband_*,
kernel k_region_lat): per cell, the sum of the four pair differences over the eight FCC neighbours at +-1 along file x / y / z,
    L_a(c) = ((u[c+o0] - u[c-o0]) + (u[c+o1] - u[c-o1])) + ((u[c+o2] - u[c-o2]) + (u[c+o3] - u[c-o3]))
seven operations in the field's own precision, in STORED coordinates (on a folded grid: folded ones, the fold row included), run through the
sections and products of tests/test_hip_vband.py.

The bar: sums and filter state are bit for bit those of VFold over the numpy restatement of L_a on the frames get_region(1, ...) gives for the region
widened by one cell on all three axes at the same moments, in every cell, and over the oracle's fields inside.  The frame is read right AFTER the
add: on a folded grid an add whose cells read the fold row Ny - 1 first makes that row the copy of row Ny - 2 of u^n (an engine whose shell lives in
memory writes it only at the start of the next step), and get_region then gives exactly the operands; checkerboard and folded grids, both
layouts, single engines and chains give the same arrays; the depth of the ring changes no bit.  Every comparison is np.array_equal.  (This file
sorts behind tests/test_hip_autotune.py: see tests/test_hip_spectra_engines.py for why its chains of three slabs must.)
"""
import numpy as np
import pytest

import cases
import oracle
from pffdtd_amd import engine, sim_data, synth
from test_hip_accum import KERNEL_N, KERNEL_REGIONS
from test_hip_bandacc import BANDS, PRE
from test_hip_region import PAIRS_KW, _slices
from test_hip_vband import VFold, _same

pytestmark = pytest.mark.gpu

COMP4 = (0, 4, 5, 6)  # u, L_x, L_y, L_z
PROD5 = [(0, 0, 0), (2, 2, 0), (0, 2, 0), (0, 2, 1), (1, 3, 0)]
# the + offsets o0 .. o3 (include/pffdtd_hip.h), in the order of synth.FCC_OFFS
LAT_OFFS = {4: [(1, 1, 0), (1, 0, 1), (1, -1, 0), (1, 0, -1)], 5: [(1, 1, 0), (0, 1, 1), (-1, 1, 0), (0, 1, -1)], 6: [(0, 1, 1), (1, 0, 1), (0, -1, 1), (-1, 0, 1)]}
NO_PASSES = engine.PF_MULTI_NO_PAIRS | engine.PF_MULTI_NO_TRIPLES


def test_the_offsets_are_the_fcc_stencils():
    offs = [tuple(int(v) for v in o) for o in synth.FCC_OFFS]
    for comp, plus in LAT_OFFS.items():
        a = comp - 4
        assert plus == [o for o in offs if o[a] == 1]  # the neighbours at +1 along the axis, in FCC_OFFS's order
        assert all(tuple(-v for v in o) in offs for o in plus) and np.array(plus).sum(axis=0).tolist() == [4 * (k == a) for k in range(3)]


def _wide(r):
    """the region of the cells actually read: one cell more on both sides of all three axes, stride 1"""
    lo, hi, st = r
    last = [lo[a] + (hi[a] - lo[a] - 1) // st[a] * st[a] for a in range(3)]
    return [lo[a] - 1 for a in range(3)], [last[a] + 2 for a in range(3)], [1, 1, 1]


def _components(frame, r, comp):
    """frame: the field over _wide(r) -> the components over r, each in the field's dtype: the contract's association"""
    st = r[2]
    n = [(frame.shape[a] - 3) // st[a] + 1 for a in range(3)]

    def at(o, sign=1):
        return frame[tuple(slice(1 + sign * o[a], 1 + sign * o[a] + (n[a] - 1) * st[a] + 1, st[a]) for a in range(3))]

    out = []
    for k in comp:
        if k == 0:
            out.append(at((0, 0, 0)))
        else:
            d = [at(o) - at(o, -1) for o in LAT_OFFS[k]]
            out.append((d[0] + d[1]) + (d[2] + d[3]))
        assert out[-1].dtype == frame.dtype and out[-1].shape == tuple(n)
    return out


def _of_grid(u, r, comp):
    return _components(u[_slices(_wide(r))], r, comp)


def _pre_per(comp, pre=PRE):
    return np.stack([pre] * len(comp))


def _scene_regions(N):
    regions = [([2, 1, 2], [N[0] - 1, N[1] - 1, N[2] - 1], [2, 1, 3])]  # a strided box around the source
    for a in range(3):  # the planes at index 1 and N - 2: the widened region holds a face cell, which forces the ghost shell (folded, y = Ny - 2: the fold row)
        for k in (1, N[a] - 2):
            lo, hi = [1, 1, 1], [N[0] - 1, N[1] - 1, N[2] - 1]
            lo[a], hi[a] = k, k + 1
            regions.append((lo, hi, [1, 1, 1]))
    regions.append(([N[0] // 3, N[1] - 2, 5], [N[0] // 3 + 1, N[1] - 1, 6], [1, 1, 1]))  # one cell, beside the last row
    return regions


# ---- 1. the small scenes: frames, the oracle, the fold row, and the run goes on ---------------------------------------------------------------------
@pytest.mark.parametrize("name,prec", [("fcc1_outside", "double"), ("fcc2_outside", "double"), ("fcc2_lossy", "single"), ("fcc2_balcony", "single")])
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
    folded = int(sd.fcc_flag) == 2
    regions = _scene_regions(N)
    nbin = -(-(nsteps - 4) // step_bin)
    eng = engine.HipEngine(sd)
    pre = _pre_per(COMP4)
    accs = [eng.vector_band_accumulator(*r, comp=COMP4, pre_sos=pre, band_sos=BANDS, prod=PROD5, nbin=nbin) for r in regions]
    want = [VFold(4, pre, BANDS, PROD5, nbin, a.shape[3:]) for a in accs]
    want_ref = [VFold(4, pre, BANDS, PROD5, nbin, a.shape[3:]) for a in accs]
    fold_rows = 0
    eng.run(0, 2)
    for n in range(2, nsteps):  # every step from 2; the first two samples only run the filters
        bin = -1 if n < 4 else (n - 4) // step_bin
        for i, r in enumerate(regions):
            accs[i].add(bin)
            frame = eng.get_region(1, *_wide(r))  # the same moment: the operands of this add
            if folded and _wide(r)[1][1] == N[1]:  # the frame's last row is the fold row: the copy of row Ny - 2
                assert np.array_equal(frame[:, -1, :], frame[:, -2, :]), (name, n, r)
                fold_rows += bool(frame[:, -1, :].any())
            want[i].add(_components(frame, r, COMP4), bin)
            want_ref[i].add(_of_grid(ref_u[n], r, COMP4), bin)
        eng.run(n, 1)
    assert fold_rows > 0 or not folded  # (live rows, not zeros against zeros)
    wide_inner = np.zeros(N, dtype=bool)
    wide_inner[3:-3, 3:-3, 3:-3] = True  # the cell and all its neighbours lie in [2, N - 2)
    for i, r in enumerate(regions):
        _same(accs[i], want[i], (name, r), count=nsteps - 2)
        e, s = accs[i].get()
        sel = wide_inner[_slices(r)]
        assert np.array_equal(e[:, :, :, sel], want_ref[i].S[:, :, :, sel]) and np.array_equal(s[:, :, :, sel], want_ref[i].state[:, :, :, sel]), (name, "oracle", r)
    assert max(w.S.max() for w in want) > 0 and all(np.isfinite(w.S).all() for w in want)
    assert max(w.S[1].max() for w in want) > 0 and max(w.S[4].max() for w in want) > 0
    assert min(w.S[2].min() for w in want) < 0 < max(w.S[2].max() for w in want)  # (the plain product of the cell and L_y takes both signs)
    eng.run(nsteps, sd.Nt - nsteps)  # nothing a later step reads has changed
    for n in range(nsteps, ref_sd.Nt):
        ref.step(n)
    assert np.array_equal(sd.u_out, ref_sd.u_out) and np.abs(ref_sd.u_out).max() > 0
    eng.close()
    ref.close()


# ---- 2. the kernel alone: fields put in, with a denormal, a -0.0, a large value, a pair difference that cancels and one that is itself denormal -------
@pytest.mark.parametrize("flag", [1, 2], ids=["checkerboard", "folded"])
@pytest.mark.parametrize("layout", [engine.PF_LAYOUT_FILE, engine.PF_LAYOUT_EXCHANGED], ids=["file_order", "exchanged"])
@pytest.mark.parametrize("prec", ["single", "double"])
def test_three_samples_are_the_exact_cascade(prec, layout, flag):
    sim = synth.shoebox(*KERNEL_N, Nt=4, fcc=True, Nm=1, Mb=3)
    if flag == 2:  # 264 x 7 x 70 stored: the regions' row y = 5 = Ny - 2 reads the fold row
        synth.fold_fcc(sim)
        synth.sort_sim(sim)
    sd = sim_data.SimData.from_sim(sim, prec, build_mask=False)
    sd.scale_input()
    N = (sd.Nx, sd.Ny, sd.Nz)
    assert N == (KERNEL_N if flag == 1 else (KERNEL_N[0], KERNEL_N[1] // 2 + 1, KERNEL_N[2])) and int(sd.fcc_flag) == flag
    dt = np.float32 if prec == "single" else np.float64
    tiny = np.finfo(dt).tiny
    rng = np.random.default_rng(101)
    state = engine._state_arrays(sd)[0]
    state["u_prev"] = rng.standard_normal(N).astype(dt)
    fields = []
    for k in range(3):
        u = rng.standard_normal(N).astype(dt)  # every cell, the holes of the checkerboard too
        u[5, 5, 5 + k % 2] = dt(1e-40) if prec == "single" else dt(1e-310)  # denormals of the field's format: a cell, and a neighbour of (5, 5, 5 / 6)
        u[5, 4, 6 + k % 2] = dt(1e-40) if prec == "single" else dt(1e-310)
        u[5, 5, 6 - k % 2] = dt(-0.0)
        u[4, 4, 7] = dt(-0.0)
        u[5, 5, 9] = u[6, 4, 10] = dt(2.0 ** 60) if prec == "single" else dt(2.0 ** 500)  # (its square is finite in double; the sections below never amplify)
        u[6, 4, 20] = u[4, 6, 20] = dt(0.75)  # the pair o2 of L_y at (5, 5, 20) -- and of L_x -- cancels to exactly 0
        for x, y, z in ((6, 6, 30), (4, 4, 30), (5, 4, 29), (5, 4, 31), (4, 6, 30), (6, 4, 30)):  # L_y of (5, 5, 30): only its pairs o1 and o3 live,
            u[x, y, z] = 0
        u[5, 4, 29], u[5, 4, 31] = dt(1.25) * tiny, dt(0.0)
        if flag == 1:  # (on the folded grid row 6 is the fold row: the engine's copy of row 5; the denormal pair is checked on the checkerboard)
            u[5, 6, 31], u[5, 6, 29] = dt(1.5) * tiny, dt(0.0)  # ... o1 is itself denormal, o3 is 0
            assert 0 < u[5, 6, 31] - u[5, 4, 29] < tiny and u[4, 6, 20] - u[6, 4, 20] == 0
        fields.append(u)
    # sections whose gain stays below 1 over three samples: |b|, |a| <= 0.3 (no inf - inf, so no NaN reaches array_equal)
    pre8 = np.concatenate([rng.uniform(-0.3, 0.3, (4, 8, 3)), np.ones((4, 8, 1)), rng.uniform(-0.3, 0.3, (4, 8, 2))], axis=2)
    band16 = np.concatenate([rng.uniform(-0.3, 0.3, (16, 8, 3)), np.ones((16, 8, 1)), rng.uniform(-0.3, 0.3, (16, 8, 2))], axis=2)
    comps = [(5,), (0, 5), (4, 6), (0, 4, 5, 6)]
    prods = {1: [(0, 0, 1), (0, 0, 0)], 2: [(0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1)], 4: [(0, 2, 0), (1, 3, 1), (2, 2, 0), (3, 0, 1), (1, 1, 0), (3, 3, 0), (2, 1, 1)]}
    eng = engine.HipEngine(sd, layout=layout)
    assert eng.layout()[2] == (layout == engine.PF_LAYOUT_EXCHANGED)
    accs, want = [], []
    for comp in comps:
        for depth in (1, 3, 8):
            for npre, nband, nsec in ((0, 1, 0), (2, 3, 2)):
                for r in KERNEL_REGIONS:
                    pre, bands, prod = pre8[:len(comp), :npre], band16[:nband, :nsec], prods[len(comp)]
                    a = eng.vector_band_accumulator(*r, comp=comp, pre_sos=pre, band_sos=bands, prod=prod, nbin=2, depth=depth)
                    assert a.ncomp == len(comp) and a.count == 0 and not a.get()[0].any()
                    accs.append(a)
                    want.append((VFold(len(comp), pre, bands, prod, 2, a.shape[3:]), r, comp, (depth, npre, nband, nsec)))
    holes = 0
    for k, bin in enumerate((0, 1, 1)):  # a bin change inside the fold, then two samples of one bin
        state["u_cur"] = fields[k]
        eng.load_state(state)
        frames = {}
        for a, (w, r, comp, _) in zip(accs, want):
            a.add(bin)
            key = tuple(tuple(v) for v in r)
            if key not in frames:  # the cells as the engine holds them after the first add (the fold row of a folded grid is the engine's)
                frames[key] = eng.get_region(1, *_wide(r))
                inner = fields[k][_slices(_wide(r))]
                rows = slice(None) if flag == 1 else slice(0, -1)
                assert np.array_equal(frames[key][:, rows, :], inner[:, rows, :])  # what was put in, the holes' values too
                if flag == 2:
                    assert np.array_equal(frames[key][:, -1, :], frames[key][:, -2, :])  # the fold row
            w.add(_components(frames[key], r, comp), bin)
        if flag == 1:
            ix, iy, iz = np.meshgrid(*[np.arange(n) for n in N], indexing="ij")
            holes += int(np.count_nonzero(fields[k][(ix + iy + iz) % 2 == 1][:1000]))
        if k == 1:  # a get in between: 2 pending at depth 3 and 8, none at depth 1
            for a, (w, r, comp, c) in zip(accs, want):
                _same(a, w, (prec, "mid", c, comp, r), count=2)
    assert holes > 0 or flag == 2
    for a, (w, r, comp, c) in zip(accs, want):
        assert np.isfinite(w.S).all() and np.isfinite(w.state).all()
        _same(a, w, (prec, c, comp, r), count=3)
    # the special cells, in a region that holds them: the differences themselves (no sections, L * L)
    r = ([5, 5, 3], [6, 6, 66], [1, 1, 1])
    a = eng.vector_band_accumulator(*r, comp=(5, 4), band_sos=np.zeros((1, 0, 6)), prod=[(0, 0, 0), (1, 1, 0)], nbin=1, depth=1)
    a.add(0)
    s = a.get()[0]
    f = eng.get_region(1, [0, 0, 0], list(N))
    for p, comp in enumerate((5, 4)):
        for z in (20, 30, 6, 7, 9, 10):
            d = [f[5 + o[0], 5 + o[1], z + o[2]] - f[5 - o[0], 5 - o[1], z - o[2]] for o in LAT_OFFS[comp]]
            L = float((d[0] + d[1]) + (d[2] + d[3]))
            assert s[p, 0, 0, 0, 0, z - 3] == L * L, (comp, z)
    if flag == 1:
        Ly = float(fields[2][5, 6, 31] - fields[2][5, 4, 29])  # L_y of (5, 5, 30) is one denormal pair difference
        assert Ly != 0 and abs(Ly) < tiny and s[0, 0, 0, 0, 0, 30 - 3] == Ly * Ly
        assert s[0, 0, 0, 0, 0, 30 - 3] != 0 or prec == "double"  # (the fp32 denormal survived the conversion; 1e-308 ** 2 underflows in any arithmetic)
    eng.close()


# ---- 3. single engines and chains, cut along x and along file z, give the same arrays ---------------------------------------------------------------
CHAINS = {"single": None, "chain2": ([0, 0], 0), "chain3": ([0, 0, 0], 0), "chain2z": ([0, 0], engine.PF_MULTI_CUT_Z), "chain3z": ([0, 0, 0], engine.PF_MULTI_CUT_Z)}


def _make(kind, sd):
    if CHAINS[kind] is None:
        return engine.HipEngine(sd)
    devices, flags = CHAINS[kind]
    return engine.HipMulti(sd, devices, multi_flags=flags | NO_PASSES, verify_exchange=2)


def test_sums_of_a_single_engine_and_of_chains():
    # the source stands at (3, 3, 3), outside the closed box: the wave runs around it, a cell per step, and has reached every cut by step 24
    name, prec, first, nsteps = "fcc2_outside", "double", 24, 34
    ref_sd = cases.make_sd(name, prec)
    N = (ref_sd.Nx, ref_sd.Ny, ref_sd.Nz)
    cuts = {0: set(), 2: set()}
    for kind, spec in CHAINS.items():  # the cuts of every chain, read from the chains themselves
        if spec is None:
            continue
        m = _make(kind, cases.make_sd(name, prec))
        assert m.nslabs == len(spec[0]) and m.info()["cut_along_z"] == kind.endswith("z") and all(m.slab(g)["steps_per_pass"] == 0 for g in range(m.nslabs))
        cuts[2 if kind.endswith("z") else 0].update(m.slab(g)["x0"] for g in range(1, m.nslabs))
        m.close()
    assert len(cuts[0]) >= 2 and len(cuts[2]) >= 2
    comp, prod = (0, 4, 5, 6), [(0, 0, 0), (1, 1, 0), (0, 2, 0), (0, 3, 1), (1, 3, 0)]
    regions = [([1, 2, 1], [N[0] - 1, N[1] - 2, N[2] - 1], [3, 1, 5]), ([2, 1, 3], [N[0] - 2, N[1] - 1, N[2] - 3], [1, 7, 1])]  # a box across every cut
    for a, xs in cuts.items():  # the planes beside every cut, on both of its sides
        for x in sorted(xs):
            for k in (x - 1, x):
                lo, hi = [1, 1, 1], [N[0] - 1, N[1] - 1, N[2] - 1]
                lo[a], hi[a] = k, k + 1
                regions.append((lo, hi, [1, 1, 1]))
    ref = oracle.Engine(ref_sd)
    ref_u = {}
    for n in range(nsteps):
        if n >= first:
            ref_u[n] = ref.grid(1).copy()
        ref.step(n)
    for n in range(nsteps, ref_sd.Nt):
        ref.step(n)
    ref.close()
    wide_inner = np.zeros(N, dtype=bool)
    wide_inner[3:-3, 3:-3, 3:-3] = True
    pre = _pre_per(comp)
    base = None
    for kind in CHAINS:
        sd = cases.make_sd(name, prec)
        obj = _make(kind, sd)
        accs = [obj.vector_band_accumulator(*r, comp=comp, pre_sos=pre, band_sos=BANDS, prod=prod, nbin=3) for r in regions]
        want = [VFold(4, pre, BANDS, prod, 3, a.shape[3:]) for a in accs]
        want_ref = [VFold(4, pre, BANDS, prod, 3, a.shape[3:]) for a in accs]
        obj.run(0, first)
        for n in range(first, nsteps):
            bin = (n - first) // 4
            for i, r in enumerate(regions):
                accs[i].add(bin)
                want[i].add(_components(obj.get_region(1, *_wide(r)), r, comp), bin)
                want_ref[i].add(_of_grid(ref_u[n], r, comp), bin)
            obj.run(n, 1)
        got = []
        for i, r in enumerate(regions):
            _same(accs[i], want[i], (kind, r), count=nsteps - first)
            e, s = accs[i].get()
            sel = wide_inner[_slices(r)]
            assert np.array_equal(e[..., sel], want_ref[i].S[..., sel]) and np.array_equal(s[..., sel], want_ref[i].state[..., sel]) and e.max() > 0, (kind, "oracle", r)
            got.append((e, s))
        if base is None:
            base = got
        else:
            for (e, s), (e0, s0) in zip(got, base):
                assert np.array_equal(e, e0) and np.array_equal(s, s0), (kind, "against the single engine")
        obj.run(nsteps, sd.Nt - nsteps)
        assert np.array_equal(sd.u_out, ref_sd.u_out) and np.abs(sd.u_out).max() > 0, kind
        obj.close()


@pytest.mark.parametrize("one_thread", [False, True], ids=["slab_threads", "one_thread"])
def test_a_chain_inside_a_pair_takes_no_sample(one_thread):
    """slabs in blocked 13-point pairs, stepped one step at a time.  (fcc2_outside is 30 x 17 x 26 stored: a pair's box needs 16 planes and 24 rows,
    so no slab of it ever pairs; this is the scene of the other accumulators' tests of this kind as a folded FCC grid, 100 x 36 x 276 stored.)"""
    flags = engine.PF_MULTI_FORCE_PAIRS | engine.PF_MULTI_NO_TRIPLES | (engine.PF_MULTI_ONE_THREAD if one_thread else 0)
    def scene():
        return synth.sort_sim(synth.fold_fcc(synth.shoebox(**PAIRS_KW, fcc=True)))

    sd = sim_data.SimData.from_sim(scene(), "single", build_mask=False)
    sd.scale_input()
    m = engine.HipMulti(sd, [0, 0], multi_flags=flags, air_variant=40, verify_exchange=2)
    assert m.slab(0)["steps_per_pass"] == 2 and m.slab(1)["steps_per_pass"] == 2, (m.slab(0), m.slab(1))
    r = ([1, 1, 1], [sd.Nx - 1, sd.Ny - 1, sd.Nz - 1], [3, 1, 5])  # both slabs hold cells of it
    comp, prod = (0, 5), [(0, 1, 0), (1, 1, 0)]
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
            want.add(_components(m.get_region(1, *_wide(r)), r, comp), n // 4)  # (after the add: the fold row is the add's)
            _same(acc, want, n)  # (whatever a refused add before it had done would show here)
        assert acc.count == len(taken)
        m.run(n, 1)
    assert taken == list(range(0, 12, 2)) and refused == list(range(1, 12, 2)), (taken, refused)
    _same(acc, want, "end")
    assert want.S[1].max() > 0
    m.run(12, sd.Nt - 12)
    ref = sim_data.SimData.from_sim(scene(), "single")
    ref.scale_input()
    oracle.run_sim(ref)
    assert np.array_equal(sd.u_out, ref.u_out)
    m.close()


# ---- 4. continue from saved sums and filter state ----------------------------------------------------------------------------------------------------
def test_a_resumed_run_continues_sums_and_state():
    r = ([3, 1, 2], [25, 15, 21], [1, 2, 3])
    comp = (0, 5, 4)
    kw = dict(comp=comp, pre_sos=_pre_per(comp), band_sos=BANDS, prod=[(0, 0, 0), (0, 1, 0), (1, 2, 1)], nbin=5, depth=4)

    def run(eng, acc, n0, n1):
        for n in range(n0, n1):
            acc.add(n // 4)
            eng.run(n, 1)

    sd = cases.make_sd("fcc2_outside", "single")
    eng = engine.HipEngine(sd)
    acc = eng.vector_band_accumulator(*r, **kw)
    run(eng, acc, 0, 20)
    whole = acc.get()
    eng.close()
    sd = cases.make_sd("fcc2_outside", "single")
    eng = engine.HipEngine(sd)
    acc = eng.vector_band_accumulator(*r, **kw)
    run(eng, acc, 0, 9)
    (sums, fstate), count, state = acc.get(), acc.count, eng.save_state()
    eng.close()
    assert count == 9 and np.abs(fstate).max() > 0
    results = []
    for restore in (True, False):
        sd = cases.make_sd("fcc2_outside", "single")
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
    assert np.array_equal(results[0][0], whole[0]) and np.array_equal(results[0][1], whole[1]) and whole[0][2].max() > 0
    assert not np.array_equal(results[1][0], whole[0])  # the control: with the filter state zeroed at set a sum differs


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_field_and_leave_the_engine_running():
    sd = cases.make_sd("fcc2_outside", "single")
    eng = engine.HipEngine(sd)
    N = [sd.Nx, sd.Ny, sd.Nz]
    lo1, hi1 = [1, 1, 1], [N[0] - 1, N[1] - 1, N[2] - 1]
    comp = (0, 5)
    ok = dict(comp=comp, pre_sos=_pre_per(comp), band_sos=BANDS, prod=[(0, 1, 0)], nbin=2)
    # a lattice difference on a Cartesian engine, by the component's name
    cart_sd = cases.make_sd("cart_mb11", "single")
    cart = engine.HipEngine(cart_sd)
    for k in (4, 5, 6):
        with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
            cart.vector_band_accumulator([1, 1, 1], [cart_sd.Nx - 1, cart_sd.Ny - 1, cart_sd.Nz - 1], **{**ok, "comp": (0, k)})
        assert ei.value.code == 1 and "comp[1]" in str(ei.value) and "fcc_flag" in str(ei.value), str(ei.value)
    cart.close()
    for kw, field in ((dict(comp=(0, 7)), "comp[1]"), (dict(comp=(0, -1)), "comp[1]"), (dict(comp=(5, 5)), "repeated"), (dict(comp=(0, 4, 5, 6, 1), pre_sos=None), "ncomp")):
        with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
            eng.vector_band_accumulator(lo1, hi1, **{**ok, **kw})
        assert ei.value.code == 1 and field in str(ei.value), str(ei.value)
    for a in (1, 2, 3):  # the axis differences stay refused on an FCC grid, and say where to go
        with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
            eng.vector_band_accumulator(lo1, hi1, **{**ok, "comp": (0, a)})
        assert "comp" in str(ei.value) and "fcc_flag" in str(ei.value) and "4 / 5 / 6" in str(ei.value), str(ei.value)
    # the one-cell rule on all six faces, whichever lattice component is asked for, by the axis's name
    for k in (4, 5, 6):
        for a, name in enumerate("xyz"):
            for side in (0, 1):
                l, h = list(lo1), list(hi1)
                if side == 0:
                    l[a] = 0  # the first cell on the face
                else:
                    h[a] = N[a]  # the last cell on the face
                with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
                    eng.vector_band_accumulator(l, h, **{**ok, "comp": (0, k)})
                assert f"along file {name}" in str(ei.value) and f"lo[{a}]" in str(ei.value) and "lattice" in str(ei.value), str(ei.value)
    with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:  # the first offending axis
        eng.vector_band_accumulator([1, 0, 0], hi1, **ok)
    assert "along file y" in str(ei.value)
    eng.vector_band_accumulator(lo1, hi1, **ok).close()
    # a chain names the axis too, against the scene's faces; a one-rank cost model has no field of the scene
    m = engine.HipMulti(cases.make_sd("fcc2_outside", "single"), [0, 0], multi_flags=NO_PASSES)
    with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
        m.vector_band_accumulator([1, 1, 0], hi1, **ok)
    assert "along file z" in str(ei.value) and "pf_multi_vband_create" in str(ei.value)
    with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
        m.vector_band_accumulator(lo1, hi1, **{**ok, "comp": (0, 2)})
    assert "fcc_flag" in str(ei.value)
    m.vector_band_accumulator(lo1, hi1, **ok).close()
    m.close()
    m = engine.HipMulti(cases.make_sd("fcc2_outside", "single"), [0, 0], only_slab=1)
    with pytest.raises(engine.PfError, match="pffdtd_hip error 4") as ei:
        m.vector_band_accumulator(lo1, hi1, **ok)
    assert ei.value.code == 4 and "only_slab" in str(ei.value)
    m.close()
    # the engine still runs to the oracle's receivers
    eng.run(0, sd.Nt)
    ref = cases.make_sd("fcc2_outside", "single")
    oracle.run_sim(ref)
    assert np.array_equal(sd.u_out, ref.u_out) and np.abs(ref.u_out).max() > 0
    eng.close()
