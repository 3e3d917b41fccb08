"""GPU: the wall absorption maps (pf_engine_absorb_* / pf_multi_absorb_*, engine.Absorption): the energy every step loses per frequency-dependent
node, per material and at the open boundary, and the sources' input.

  1. against the reference PYTHON engine: its E_lost / E_in series (tests/golden/energy_*.npz) and their split (absorption_*.npz, made by
     make_golden_absorption.py), fp64, to the tolerance test_hip_energy.py applies to those series: 1e-9 of the series' peak;
  2. against the engine's own state, independent of the new kernels: after every step save_state, and numpy restates the three terms from
     consecutive vh1 / u arrays in the kernels' order of operations.  Every term is then the same double on both sides and only the ORDER of the sums
     differs: two sums of N terms differ by at most (N - 1) * 2^-52 * sum |terms| to first order, so with one bin per step the bounds are
     Nbl * 2^-52 (materials) and Nba * 2^-52 (open boundary) relative -- their terms are non-negative -- and Ns * 2^-52 * sum |terms| absolute for
     the input, whose terms change sign; a node's own sum has at most twelve non-negative terms: 1e-14 relative;
  3. the same run twice gives the same bytes, and a run cut by a checkpoint mid-bin the bytes of the run in one piece;
  4. chains of 2 and 3 slabs, both cut axes: nodes bit-equal to the single engine, bins to the bounds of 2., and sample-then-step with nothing
     between equal to sample, get, step; a chain cut by a checkpoint mid-bin: nodes bit-equal, bins to the chain's bound (a chain's set gives the
     scene's bins to slab 0, so the resumed chain adds the same terms in another order);
  5. the refusals, by message.

Two scenes.  MIXED is the issue's: 16 x 14 x 12, three materials of 1 / 12 / 5 branches in one wave, Nbl = 265 (two workgroups, a tail of 9).  Its box is
closed, so a source inside never reaches the ABC shell and the open boundary's row is zero there.  WIDE is the same room on 28 x 24 x 20 with the walls
five cells in and TWO sources, one inside the box (the walls absorb) and one outside it (the ABC shell absorbs): every row of the output is live, on
every layout -- exchanged axes, fcc_flag 0 / 1 / 2, chains -- and the FCC forms hold 454 lossy nodes, more than one workgroup of 256.
"""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

from pffdtd_amd import absorption, engine, sim_data, synth

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
from make_golden import digest  # noqa: E402
from energy_cases import ENERGY_CASES  # noqa: E402

EPS = 2.0 ** -52
NO_PASSES = engine.PF_MULTI_NO_PAIRS | engine.PF_MULTI_NO_TRIPLES
MIXED = dict(Nx=16, Ny=14, Nz=12, Nt=40, Nm=3, Mb=[1, 12, 5], rigid_every=13, sig="dhann30")  # waves of mixed materials, Nbl no multiple of 64
WIDE = dict(MIXED, Nx=28, Ny=24, Nz=20, wall=5)
OUTSIDE = [2, 2, 2]  # a source cell between the ghost layer and WIDE's walls


def _observe(obj, sd, nbin):
    return obj.absorption(*absorption.scales(sd), nbin=nbin)


def _run(obj, a, n0, n1, bin_of, between=None):
    """the samples before the steps n0 .. n1 (the first one primes) and the steps n0 .. n1 - 1"""
    for n in range(n0, n1 + 1):
        a.add(n, bin_of(max(n - 1, 0)))
        if between:
            between(n)
        if n < n1:
            obj.run(n, 1)


# ---- 1. the reference ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ENERGY_CASES))
def test_the_split_of_the_python_reference(name):
    old, new = np.load(GOLDEN / f"energy_{name}.npz"), np.load(GOLDEN / f"absorption_{name}.npz")
    sim = synth.shoebox(**ENERGY_CASES[name])
    assert digest(sim) == str(old["digest"]) == str(new["digest"])
    sd = sim_data.SimData.from_sim(sim, "double")  # no scale_input: the Python engine does not rescale
    eng = engine.HipEngine(sd)
    a = _observe(eng, sd, sd.Nt)
    _run(eng, a, 0, sd.Nt, lambda s: s)
    got = a.get()
    assert a.count == sd.Nt
    eng.close()
    lost, E_in = np.diff(old["E_lost"]), np.diff(old["E_in"])
    for mine, ref, what in ((got["materials"].sum(1) + got["open_boundary"], lost, "E_lost"), (got["input"], E_in, "E_in"), (got["materials"], new["materials"], "materials"),
                            (got["open_boundary"], new["open_boundary"], "open boundary"), (got["nodes"], new["wall_nodes"].sum(0), "nodes")):
        err, scale = np.abs(mine - ref).max() if ref.size else 0.0, max(np.abs(ref).max() if ref.size else 0.0, 1e-300)
        print(f"{name} {what}: max |difference| {err:.3e}, peak {scale:.3e}")
        assert err <= 1e-9 * scale, what
    assert got["input"].any() and got["open_boundary"].any() == bool(new["open_boundary"].any())


# ---- 2. the engine's own state ------------------------------------------------------------------------------------------------------------------------
def _host_terms(sd, scales, before, after, step):
    """the three term lists of step `step` from the states before and after it, in the kernels' order of operations"""
    E, ws, ab, ins = scales
    f8 = np.float64
    v = before["vh1"].astype(f8) + after["vh1"].astype(f8)
    Ek = np.zeros((sd.Nbl, 12))
    if sd.Nbl:
        Ek[:, :E.shape[1]] = E[sd.mat_bnl]
    s = np.zeros(sd.Nbl)
    for m in range(12):
        s = s + (v[:, m] * v[:, m]) * Ek[:, m]
    wall = ws * (sd.ssaf_bnl.astype(f8) * s)
    d = after["u_cur"].reshape(-1)[sd.bna_ixyz].astype(f8) - before["u_prev"].reshape(-1)[sd.bna_ixyz].astype(f8)
    q = sd.Q_bna.astype(f8)
    abc = ab * ((2.0 ** -q * q) * (d * d))
    d = after["u_cur"].reshape(-1)[sd.in_ixyz].astype(f8) - before["u_prev"].reshape(-1)[sd.in_ixyz].astype(f8)
    inp = ins * (d * sd.in_sigs[:, step].astype(sd.real).astype(f8))
    return wall, abc, inp


STATE_CASES = {f"{p}_fcc{f}": dict(prec=p, fcc=f, wide=True) for p in ("single", "double") for f in (0, 1, 2)}
STATE_CASES["single_exchanged"] = dict(prec="single", fcc=0, wide=True, layout=engine.PF_LAYOUT_EXCHANGED)
STATE_CASES["single_small"] = dict(prec="single", fcc=0)
STATE_CASES["double_small"] = dict(prec="double", fcc=0)
STATE_CASES["single_free_space"] = dict(prec="single", fcc=0, box=False)


def _scene(fcc=0, box=True, Nt=40, wide=False):
    """MIXED, or WIDE with its second source outside the box"""
    kw = {**(WIDE if wide else MIXED), "Nt": Nt}
    sim = synth.shoebox(**kw, fcc=fcc > 0, box=box)
    if wide:
        c, d = sim["comms_out"], synth.shoebox(**kw, fcc=fcc > 0, box=box, src=OUTSIDE)["comms_out"]
        c["in_ixyz"], c["in_sigs"] = np.concatenate([c["in_ixyz"], d["in_ixyz"]]), np.concatenate([c["in_sigs"], d["in_sigs"]])
        c["Ns"] = np.int64(c["in_ixyz"].size)
    return synth.fold_fcc(sim) if fcc == 2 else sim


@pytest.mark.parametrize("case", list(STATE_CASES))
def test_the_sums_restated_from_saved_states(case):
    c = STATE_CASES[case]
    steps, wide = 12, c.get("wide", False)
    sd = sim_data.SimData.from_sim(_scene(c["fcc"], c.get("box", True), Nt=steps, wide=wide), c["prec"])
    if c.get("box", True):
        assert sd.Nbl % 64 != 0 and sd.Nbl > 256 and all((sd.mat_bnl == k).any() for k in range(3)), sd.Nbl
    else:
        assert sd.Nbl == 0
    assert sd.Nba > 0 and sd.Ns > 0
    eng = engine.HipEngine(sd, layout=c.get("layout", 0))
    if "layout" in c:
        assert eng.layout()[2]
    scales = absorption.scales(sd)
    a = _observe(eng, sd, steps)
    states = {}
    _run(eng, a, 0, steps, lambda s: s, between=lambda n: states.__setitem__(n, eng.save_state()))
    got = a.get()
    eng.close()
    nodes = np.zeros(sd.Nbl)
    worst = {"node": 0.0, "material": 0.0, "open": 0.0, "input": 0.0}
    for s in range(steps):
        wall, abc, inp = _host_terms(sd, scales, states[s], states[s + 1], s)
        nodes = nodes + wall
        for k in range(sd.Nm):
            ref = wall[sd.mat_bnl == k].sum()
            err = abs(got["materials"][s, k] - ref)
            worst["material"] = max(worst["material"], err / ref if ref else err)
            assert err <= sd.Nbl * EPS * ref, (s, k, got["materials"][s, k], ref)
        ref = abc.sum()
        worst["open"] = max(worst["open"], abs(got["open_boundary"][s] - ref) / ref if ref else 0.0)
        assert abs(got["open_boundary"][s] - ref) <= sd.Nba * EPS * ref, (s, got["open_boundary"][s], ref)
        worst["input"] = max(worst["input"], abs(got["input"][s] - inp.sum()) / max(np.abs(inp).sum(), 1e-300))
        assert abs(got["input"][s] - inp.sum()) <= sd.Ns * EPS * np.abs(inp).sum(), (s, got["input"][s], inp.sum())
    if sd.Nbl:
        worst["node"] = (np.abs(got["nodes"] - nodes) / np.maximum(nodes, 1e-300)).max()
        assert np.all(np.abs(got["nodes"] - nodes) <= 1e-14 * nodes)
        assert nodes.max() > 0 and got["materials"].sum(0).all()
    assert got["open_boundary"].any() == (wide or not c.get("box", True))  # (MIXED's closed box keeps its one source's field off the ABC shell)
    assert got["input"].any()
    print(case, "Nbl", sd.Nbl, "Nba", sd.Nba, "worst relative differences", worst)


# ---- 3. determinism and resume ------------------------------------------------------------------------------------------------------------------------
def _same_bytes(x, y):
    return all(x[k].tobytes() == y[k].tobytes() for k in ("nodes", "materials", "open_boundary", "input"))


def test_the_same_bits_twice_and_across_a_checkpoint():
    steps, cut, per_bin = 40, 25, 15  # bins of the steps 0 .. 14, 15 .. 29, 30 .. 39: the cut lies inside the second, a bin boundary in the second part
    bin_of = lambda s: s // per_bin  # noqa: E731

    def whole():
        sd = sim_data.SimData.from_sim(_scene(), "single")
        eng = engine.HipEngine(sd)
        a = _observe(eng, sd, 3)
        _run(eng, a, 0, steps, bin_of)
        out = a.get(), a.count, sd.u_out.copy()
        eng.close()
        return out

    one, count, u_out = whole()
    again = whole()
    assert count == steps and _same_bytes(one, again[0])
    assert one["materials"].all() and one["input"].all()

    sd = sim_data.SimData.from_sim(_scene(), "single")
    eng = engine.HipEngine(sd)
    a = _observe(eng, sd, 3)
    _run(eng, a, 0, cut, bin_of)
    part, state, n_part = a.get(), eng.save_state(), a.count
    eng.close()
    assert n_part == cut and not part["materials"][2].any()
    sd2 = sim_data.SimData.from_sim(_scene(), "single")
    eng = engine.HipEngine(sd2)
    eng.load_state(state)
    a = _observe(eng, sd2, 3)
    a.set(part, n_part)
    assert a.count == cut
    _run(eng, a, cut, steps, bin_of)  # (its first add primes from the loaded state)
    resumed = a.get()
    assert a.count == steps
    eng.close()
    assert _same_bytes(one, resumed)
    assert np.array_equal(sd2.u_out[:, cut:steps], u_out[:, cut:steps])


# ---- 4. chains ----------------------------------------------------------------------------------------------------------------------------------------
CHAINS = {"chain2": ([0, 0], engine.PF_MULTI_CUT_X), "chain3": ([0, 0, 0], engine.PF_MULTI_CUT_X), "chain2z": ([0, 0], engine.PF_MULTI_CUT_Z),
          "chain3z": ([0, 0, 0], engine.PF_MULTI_CUT_Z)}


@pytest.fixture(scope="module")
def single_run():
    """WIDE on one engine, one bin per step: the sums, and per step the sum of |input terms| for the input row's bound"""
    steps = 16
    sd = sim_data.SimData.from_sim(_scene(Nt=steps, wide=True), "single")
    eng = engine.HipEngine(sd)
    a = _observe(eng, sd, steps)
    states = {}
    _run(eng, a, 0, steps, lambda s: s, between=lambda n: states.__setitem__(n, eng.save_state()))
    got = a.get()
    eng.close()
    scales = absorption.scales(sd)
    in_abs = np.array([np.abs(_host_terms(sd, scales, states[s], states[s + 1], s)[2]).sum() for s in range(steps)])
    return steps, got, in_abs


@pytest.mark.parametrize("kind", list(CHAINS))
def test_chains_against_the_single_engine(kind, single_run):
    steps, ref, in_abs = single_run
    devices, flags = CHAINS[kind]
    outs = []
    for read_between in (True, False):
        sd = sim_data.SimData.from_sim(_scene(Nt=steps, wide=True), "single")
        m = engine.HipMulti(sd, devices, multi_flags=flags | NO_PASSES, verify_exchange=2)
        assert m.info()["cut_along_z"] == (flags == engine.PF_MULTI_CUT_Z)
        a = _observe(m, sd, steps)
        _run(m, a, 0, steps, lambda s: s, between=(lambda n: a.get()) if read_between else None)
        outs.append(a.get())
        assert a.count == steps and m.info()["exchange_verified"] is not False
        m.close()
    got, unread = outs
    assert _same_bytes(got, unread)  # sample, step with nothing between = sample, get, step
    assert got["nodes"].tobytes() == ref["nodes"].tobytes()
    assert np.all(np.abs(got["materials"] - ref["materials"]) <= sd.Nbl * EPS * ref["materials"])
    assert np.all(np.abs(got["open_boundary"] - ref["open_boundary"]) <= sd.Nba * EPS * ref["open_boundary"])
    assert np.all(np.abs(got["input"] - ref["input"]) <= sd.Ns * EPS * in_abs)
    assert ref["materials"].sum(0).all() and ref["input"].any() and ref["open_boundary"].any() and got["open_boundary"].any()


@pytest.mark.parametrize("kind", ["chain2", "chain3z"])
def test_a_chain_across_a_checkpoint(kind, single_run):
    """A chain's set gives the scene's bins to slab 0 and zeros to the others, so the bin the cut lies in is summed in another order than in the chain
    in one piece -- ((a0 + a1) + b0) + b1 against (a0 + b0) + (a1 + b1): the nodes, each one slab's own, are bit-equal, the bins agree to the chain's
    bound (every value passes through far fewer than Nbl additions of non-negative terms; the input row: Ns * 2^-52 of the bin's sum of |terms|)."""
    steps, cut, per_bin = 16, 10, 6  # bins of the steps 0 .. 5, 6 .. 11, 12 .. 15: the cut lies inside the second
    assert single_run[0] == steps
    in_abs = np.array([single_run[2][b * per_bin:(b + 1) * per_bin].sum() for b in range(3)])
    bin_of = lambda s: s // per_bin  # noqa: E731
    devices, flags = CHAINS[kind]

    def chain():
        sd = sim_data.SimData.from_sim(_scene(Nt=steps, wide=True), "single")
        return sd, engine.HipMulti(sd, devices, multi_flags=flags | NO_PASSES, verify_exchange=2)

    sd, m = chain()
    a = _observe(m, sd, 3)
    _run(m, a, 0, steps, bin_of)
    one, u_out = a.get(), sd.u_out.copy()
    m.close()
    sd, m = chain()
    a = _observe(m, sd, 3)
    _run(m, a, 0, cut, bin_of)
    part, state, n_part = a.get(), m.save_state(), a.count
    m.close()
    assert n_part == cut and part["materials"][1].any() and not part["materials"][2].any()
    sd, m = chain()
    m.load_state(state)
    a = _observe(m, sd, 3)
    a.set(part, n_part)
    back = a.get()
    assert _same_bytes(back, part) and a.count == cut  # (a get straight after the set: x + 0.0 changes no bit)
    _run(m, a, cut, steps, bin_of)
    got = a.get()
    assert a.count == steps
    m.close()
    assert got["nodes"].tobytes() == one["nodes"].tobytes()
    assert np.all(np.abs(got["materials"] - one["materials"]) <= sd.Nbl * EPS * one["materials"]) and one["materials"].all()
    assert np.all(np.abs(got["open_boundary"] - one["open_boundary"]) <= sd.Nba * EPS * one["open_boundary"]) and one["open_boundary"].all()
    assert np.all(np.abs(got["input"] - one["input"]) <= sd.Ns * EPS * in_abs)
    assert np.array_equal(sd.u_out[:, cut:steps], u_out[:, cut:steps])


# ---- 5. the refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_message():
    sd = sim_data.SimData.from_sim(_scene(), "single")
    eng, other = engine.HipEngine(sd), engine.HipEngine(sim_data.SimData.from_sim(_scene(), "single"))
    a = _observe(eng, sd, 3)
    L = engine.lib()
    with pytest.raises(engine.PfError, match="bin = 3 outside 0 .. 2") as ei:
        a.add(0, 3)
    assert ei.value.code == 1
    with pytest.raises(engine.PfError, match="bin = -1 outside"):
        a.add(0, -1)
    a.add(0, 0)
    eng.run(0, 2)
    with pytest.raises(engine.PfError, match="n = 2 after n = 0") as ei:  # a gap: step 0's old branch currents are gone
        a.add(2, 0)
    assert ei.value.code == 4 and a.count == 0
    a.set(None, 0)
    a.add(2, 0)  # (after a set the next add primes again)
    eng.step_begin(2)
    for f in (lambda: a.add(3, 0), a.get, lambda: a.set(None, 0)):
        with pytest.raises(engine.PfError, match="split-phase") as ei:
            f()
        assert ei.value.code == 4
    eng.step_end(2)
    a.add(3, 0)
    assert a.count == 1
    # another engine's handle, a handle of another kind, null arguments
    assert L.pf_engine_absorb_add(other._h, a._a, 4, 0) == 1 and b"another engine" in L.pf_last_error()
    assert L.pf_engine_absorb_get(other._h, a._a, None, None, None, None) == 1 and b"another engine" in L.pf_last_error()
    acc = eng.accumulator([1, 1, 1], [3, 3, 3])
    assert L.pf_engine_absorb_add(eng._h, acc._a, 4, 0) == 1 and b"pf_absorb" in L.pf_last_error()
    assert L.pf_engine_accum_get(eng._h, a._a, None) == 1
    out = ctypes.c_void_p()
    E = np.zeros((sd.Nm, 12))
    assert L.pf_engine_absorb_create(eng._h, None, 1.0, 1.0, 1.0, 1, ctypes.byref(out)) == 1 and b"null E" in L.pf_last_error()
    assert L.pf_engine_absorb_create(eng._h, E.ctypes.data_as(ctypes.c_void_p), 1.0, 1.0, 1.0, 0, ctypes.byref(out)) == 1 and b"nbin" in L.pf_last_error()
    assert L.pf_engine_absorb_add(eng._h, None, 0, 0) == 1 and b"null pf_absorb" in L.pf_last_error() and L.pf_absorb_count(None) < 0
    assert a.count == 1
    eng.close()
    other.close()
