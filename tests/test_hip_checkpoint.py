"""GPU: checkpoint and resume (pf_engine_save_state / _load_state, pf_multi_*, pffdtd_amd/checkpoint.py, the CLI's --checkpoint / --resume).

The bar is the oracle's bits: a run that is saved, destroyed and continued in a new engine -- of any kernel family, storage layout, as one
domain or as a chain of slabs -- gives the receivers and the fields of a run in one piece.  Every resume test carries a control: the same
continuation with the restored branch state zeroed must CHANGE a receiver sample, so no test passes on a state that does not matter.
"""
import ctypes
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import cases
import oracle
from pffdtd_amd import checkpoint, engine, h5io, sim_data, synth
from test_hip_tb2 import triple_scene

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
STOP = 31  # steps before the checkpoint of the small scenes (after them every lossy node of these scenes is non-zero in the oracle)


def _interior(a):
    return a[1:-1, 1:-1, 1:-1]


def _zeroed(state):
    st = dict(state)
    st["vh1"], st["gh1"] = np.zeros_like(state["vh1"]), np.zeros_like(state["gh1"])
    return st


def _continue(make, state, n0, n1, head):
    """a new engine or chain from make() -> (obj, sd) loads `state`, runs steps n0 .. n1-1 and takes the rows before n0 from `head`
    -> (u_out, state after)"""
    obj, sd = make()
    obj.load_state(state)
    obj.run(n0, n1 - n0)
    sd.u_out[:, :n0] = head[:, :n0]
    out, after = sd.u_out.copy(), obj.save_state()
    obj.close()
    return out, after


def _assert_sensitive(make, state, n0, n1, head, good):
    """the control: with the restored branch state zeroed the continuation must differ"""
    assert np.count_nonzero(state["vh1"]) > 0 and np.count_nonzero(state["gh1"]) > 0
    bad, _ = _continue(make, _zeroed(state), n0, n1, head)
    assert not np.array_equal(bad, good), "the branch state does not reach a receiver: the test would pass without it"


# ---- 1. resume equals the uninterrupted oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["single", "double"])
@pytest.mark.parametrize("name,numerics", [("cart_mb11", 0), ("cart_lroom", 0), ("fcc1_lossy", 0), ("fcc2_mb11", 0), ("cart_mb11", 2)],
                         ids=["cart_mb11", "cart_lroom", "fcc1_lossy", "fcc2_mb11", "cart_mb11_safeguarded"])
def test_resume_equals_the_uninterrupted_oracle(name, numerics, prec):
    sg = numerics == engine.PF_NUM_GPU_SAFEGUARDED
    ref = cases.make_sd(name, prec)
    oracle.run_sim(ref, safeguarded=sg)
    ref_g = cases.make_sd(name, prec)
    e = oracle.Engine(ref_g, safeguarded=sg)
    for n in range(ref_g.Nt):
        e.step(n)
    ref_u0, ref_u1 = e.grid(0).copy(), e.grid(1).copy()
    e.close()
    assert np.array_equal(ref_g.u_out, ref.u_out) and np.abs(ref.u_out).max() > 0

    def make():
        sd = cases.make_sd(name, prec)
        return engine.HipEngine(sd, numerics=numerics, readout_chunk=16), sd

    a, sd_a = make()
    a.run(0, STOP)
    state = a.save_state()
    a.close()  # engine A is gone: all that is left is the state and its receiver rows
    print(f"{name} {prec}: {np.count_nonzero(np.any(state['vh1'] != 0, axis=1))} of {sd_a.Nbl} lossy nodes with branch state after {STOP} steps")
    out, after = _continue(make, state, STOP, ref.Nt, sd_a.u_out)
    assert np.array_equal(out, ref.u_out), f"u_out max|d|={np.abs(out - ref.u_out).max()}"
    assert np.array_equal(_interior(after["u_cur"]), _interior(ref_u1))
    assert np.array_equal(_interior(after["u_prev"]), _interior(ref_u0))
    _assert_sensitive(make, state, STOP, ref.Nt, sd_a.u_out, out)


# ---- 2. the state one step after set_grid ----------------------------------------------------------------------------------------
def test_the_state_one_step_after_set_grid_is_complete():
    """The reference starts u1b / u2b at zero whatever the fields hold, so one step after pf_engine_set_grid u2b is NOT u^{n-1} at the nodes:
    a load that regathered it from the grid would leave the oracle's bits."""
    prec, steps = "double", 10
    ref = cases.make_sd("cart_mb11", prec)
    rng = np.random.default_rng(41)
    init = [(rng.standard_normal((ref.Nx, ref.Ny, ref.Nz)) * 1e-2).astype(np.float64) for _ in range(2)]
    e = oracle.Engine(ref)
    for k in (0, 1):
        e.grid(k)[...] = init[k]
    for n in range(steps):
        e.step(n)
    ref_u1 = e.grid(1).copy()
    e.close()

    def make():
        sd = cases.make_sd("cart_mb11", prec)
        return engine.HipEngine(sd), sd

    a, sd_a = make()
    for k in (0, 1):
        a.set_grid(k, init[k])
    a.run(0, 1)
    state = a.save_state()
    a.close()
    flat = sd_a.bnl_ixyz
    assert np.count_nonzero(state["u2b"]) == 0 and np.count_nonzero(init[0].reshape(-1)[flat]) > 0  # (what a regathered u2b would hold)
    assert np.array_equal(state["u1b"], state["u_cur"].reshape(-1)[flat])
    out, after = _continue(make, state, 1, steps, sd_a.u_out)
    assert np.array_equal(out[:, :steps], ref.u_out[:, :steps])
    assert np.array_equal(_interior(after["u_cur"]), _interior(ref_u1))
    _assert_sensitive(make, state, 1, steps, sd_a.u_out, out)
    # and the regathered u2b does change the result (the guard of this test's own point)
    wrong = dict(state)
    wrong["u2b"] = state["u_prev"].reshape(-1)[flat].copy()
    bad, _ = _continue(make, wrong, 1, steps, sd_a.u_out)
    assert not np.array_equal(bad, out)


# ---- 3 - 6. triples, wall regions, bricks; the canonical state; portability; rewind ------------------------------------------------
N_SAVE, N_END = 7, 15  # two triples and a single step, then eight more


class Triple:
    """the scene of tests 3 - 6 in one precision: the oracle's trajectory from seeded random fields, computed once and never changed"""

    def __init__(self, prec):
        self.prec = prec
        self.n = (48, 100, 280 if prec == "single" else 264)
        self.sim = triple_scene(Nt=N_END, n=self.n)
        dt = np.float32 if prec == "single" else np.float64
        rng = np.random.default_rng(53)
        self.init = [(rng.standard_normal(self.n) * 1e-2).astype(dt) for _ in range(2)]
        ref = sim_data.SimData.from_sim(self.sim, prec)
        ref.scale_input()
        e = oracle.Engine(ref)
        for k in (0, 1):
            e.grid(k)[...] = self.init[k]
        self.ref_fields = {}
        for n in range(N_END):
            if n == N_SAVE:
                self.ref_fields[n] = (e.grid(0).copy(), e.grid(1).copy())
            e.step(n)
        self.ref_fields[N_END] = (e.grid(0).copy(), e.grid(1).copy())
        e.close()
        self.ref_out = ref.u_out.copy()
        self.Nbl = ref.Nbl
        z = np.zeros
        self.start = {"u_prev": self.init[0], "u_cur": self.init[1], "u1b": z(ref.Nbl, dt), "u2b": z(ref.Nbl, dt), "vh1": z((ref.Nbl, 12), dt), "gh1": z((ref.Nbl, 12), dt)}
        self.saved = {}

    def sd(self):
        sd = sim_data.SimData.from_sim(self.sim, self.prec, build_mask=False)
        sd.scale_input()
        return sd

    def maker(self, kind):
        def make():
            sd = self.sd()
            if kind == "v25":
                return engine.HipEngine(sd, air_variant=25, timing=True), sd
            if kind == "v40":
                return engine.HipEngine(sd, air_variant=40, timing=True), sd
            if kind == "exchanged":
                return engine.HipEngine(sd, layout=engine.PF_LAYOUT_EXCHANGED, timing=True), sd
            if kind == "chain3":
                return engine.HipMulti(sd, [0, 0, 0], verify_exchange=2), sd
            if kind == "chain2z":
                return engine.HipMulti(sd, [0, 0], multi_flags=engine.PF_MULTI_CUT_Z, verify_exchange=2), sd
            raise KeyError(kind)
        return make

    def state_at_save(self, kind):
        """`kind` from the random fields to step N_SAVE -> (state, its receiver rows, timing or chain info); computed once per kind"""
        if kind not in self.saved:
            obj, sd = self.maker(kind)()
            obj.load_state(self.start)  # (what two set_grid calls on a new engine do; a chain has no set_grid)
            obj.run(0, N_SAVE)
            st = obj.save_state()
            extra = obj.timing() if isinstance(obj, engine.HipEngine) else obj.info()
            if kind == "exchanged":
                assert obj.layout()[2]
            obj.close()
            self.saved[kind] = (st, sd.u_out.copy(), extra)
        return self.saved[kind]

    def check_end(self, out, after, label):
        assert np.array_equal(out, self.ref_out), f"{label}: u_out max|d|={np.abs(out - self.ref_out).max()}"
        for k, f in zip(("u_prev", "u_cur"), self.ref_fields[N_END]):
            assert np.array_equal(_interior(after[k]), _interior(f)), (label, k)


@pytest.fixture(scope="module", params=["single", "double"])
def triple(request):
    return Triple(request.param)


def test_triples_with_wall_regions_and_bricks_resume(triple):
    make = triple.maker("v40")
    state, head, tm = triple.state_at_save("v40")
    assert tm["tb_steps_per_pass"] == 3 and tm["wall_bricks"] > 0, tm
    assert np.array_equal(head[:, :N_SAVE], triple.ref_out[:, :N_SAVE])
    b, sd = make()
    b.load_state(state)
    b.run(N_SAVE, N_END - N_SAVE)
    tm_b = b.timing()
    sd.u_out[:, :N_SAVE] = head[:, :N_SAVE]
    out, after = sd.u_out.copy(), b.save_state()
    b.close()
    assert tm_b["tb_steps_per_pass"] == 3 and tm_b["wall_bricks"] > 0 and tm_b["tb2_launches"] > 0, tm_b
    triple.check_end(out, after, "v40 -> v40")
    _assert_sensitive(make, state, N_SAVE, N_END, head, out)


KINDS = ["v25", "v40", "exchanged", "chain3", "chain2z"]


def test_the_state_is_canonical(triple):
    """five engines that share no kernel, layout or decomposition save the same arrays"""
    base, _, _ = triple.state_at_save("v25")
    assert np.count_nonzero(np.any(base["vh1"] != 0, axis=1)) > triple.Nbl // 2  # (random fields: every wall is live)
    for k, f in zip(("u_prev", "u_cur"), triple.ref_fields[N_SAVE]):
        assert np.array_equal(_interior(base[k]), _interior(f)), k
    mb = np.asarray([11, 3])[triple.sd().mat_bnl]
    unused = np.arange(12)[None, :] >= mb[:, None]
    assert unused.any()
    for kind in KINDS[1:]:
        st, head, extra = triple.state_at_save(kind)
        if kind == "chain2z":
            assert extra["cut_along_z"] and extra["nslabs"] == 2, extra
        if kind == "chain3":
            assert not extra["cut_along_z"] and extra["nslabs"] == 3, extra
        for k in ("u1b", "u2b", "vh1", "gh1"):
            assert np.array_equal(st[k], base[k]), (kind, k, int(np.count_nonzero(st[k] != base[k])))
        for k in ("u_prev", "u_cur"):
            assert np.array_equal(_interior(st[k]), _interior(base[k])), (kind, k)
        for k in ("vh1", "gh1"):
            assert not st[k][unused].any(), (kind, k)  # the all-zero tail of the unused branch slots
        assert np.array_equal(head[:, :N_SAVE], triple.ref_out[:, :N_SAVE]), kind


@pytest.mark.parametrize("src,dst", [("v25", "chain3"), ("v25", "exchanged"), ("chain3", "v40"), ("chain2z", "v25")])
def test_a_state_is_portable(triple, src, dst):
    state, head, _ = triple.state_at_save(src)
    make = triple.maker(dst)
    obj, sd = make()
    obj.load_state(state)
    obj.run(N_SAVE, N_END - N_SAVE)
    sd.u_out[:, :N_SAVE] = head[:, :N_SAVE]
    out, after = sd.u_out.copy(), obj.save_state()
    info = obj.info() if isinstance(obj, engine.HipMulti) else None
    obj.close()
    triple.check_end(out, after, f"{src} -> {dst}")
    if info is not None:  # the first exchanges after the load were checksummed again, on planes that were not all zeros
        assert info["exchange_verified"] is True and info["exchange_nonzero"] and info["exchanges_checked"] >= 2, info
    if (src, dst) == ("v25", "chain3"):
        _assert_sensitive(make, state, N_SAVE, N_END, head, out)


@pytest.mark.parametrize("kind", ["v40", "chain3"])
def test_rewind(triple, kind):
    """one engine runs 0 .. 14, loads its own state of step 7 and runs 7 .. 14 again: nothing of the first pass leaks into the second"""
    obj, sd = triple.maker(kind)()
    obj.load_state(triple.start)
    obj.run(0, N_SAVE)
    mid = obj.save_state()
    obj.run(N_SAVE, N_END - N_SAVE)
    first_out, first = sd.u_out.copy(), obj.save_state()
    sd.u_out[:, N_SAVE:] = 0
    obj.load_state(mid)
    obj.run(N_SAVE, N_END - N_SAVE)
    second_out, second = sd.u_out.copy(), obj.save_state()
    obj.close()
    assert np.array_equal(first_out, triple.ref_out)
    assert np.array_equal(second_out, first_out)
    for k in engine.STATE_KEYS:
        a, b = (first[k], second[k]) if first[k].ndim != 3 else (_interior(first[k]), _interior(second[k]))
        assert np.array_equal(a, b), k
    assert np.count_nonzero(mid["vh1"]) > 0 and not np.array_equal(mid["vh1"], first["vh1"])  # (the rewind had something to undo)


def test_a_chain_inside_a_pass_refuses_and_is_saved_after_it():
    """Slabs that step in blocked pairs or triples can only be saved between passes: one step into a pass pf_multi_save_state refuses
    (PF_ERR_STATE) and leaves the chain usable; once the pass has ended it saves, and that state continues to the oracle's bits in a new
    chain and in a single domain."""
    kw = dict(Nx=100, Ny=70, Nz=276, Nt=24, wall=3, Nm=1, Mb=3, src=[47, 30, 100], rcv=[[30, 25, 96], [66, 36, 110], [48, 35, 104], [47, 4, 101]])
    ref = sim_data.SimData.from_sim(synth.shoebox(**kw), "single")
    ref.scale_input()
    rng = np.random.default_rng(67)  # seeded random fields: every wall is live from step 0 (the wave from the source needs 30 steps to a wall)
    init = [(rng.standard_normal((ref.Nx, ref.Ny, ref.Nz)) * 1e-2).astype(np.float32) for _ in range(2)]
    e = oracle.Engine(ref)
    for k in (0, 1):
        e.grid(k)[...] = init[k]
    for n in range(ref.Nt):
        e.step(n)
    e.close()
    start = engine._state_arrays(ref)[0]
    start["u_prev"], start["u_cur"] = init

    def make_chain():
        sd = sim_data.SimData.from_sim(synth.shoebox(**kw), "single", build_mask=False)
        sd.scale_input()
        return engine.HipMulti(sd, [0, 0], multi_flags=engine.PF_MULTI_FORCE_PAIRS, air_variant=40, verify_exchange=2), sd

    def make_single():
        sd = sim_data.SimData.from_sim(synth.shoebox(**kw), "single", build_mask=False)
        sd.scale_input()
        return engine.HipEngine(sd), sd

    m, sd = make_chain()
    spp = m.slab(0)["steps_per_pass"]  # 2: pairs, 3: triples (whichever the slabs' wall regions allow)
    assert spp in (2, 3) and m.slab(1)["steps_per_pass"] == spp
    n_in, n_ok = 4 * spp + 1, 5 * spp  # one step into the fifth pass; its end
    m.load_state(start)
    m.run(0, n_in)
    with pytest.raises(engine.PfError, match="pffdtd_hip error 4") as ei:
        m.save_state()
    assert ei.value.code == 4
    with pytest.raises(engine.PfError, match="pffdtd_hip error 4"):
        m.load_state(engine._state_arrays(sd)[0])
    m.run(n_in, n_ok - n_in)  # (the refusal left the chain as it was)
    state = m.save_state()
    m.run(n_ok, sd.Nt - n_ok)
    assert np.array_equal(sd.u_out, ref.u_out)
    head = sd.u_out.copy()
    m.close()
    for make in (make_chain, make_single):
        out, _ = _continue(make, state, n_ok, ref.Nt, head)
        assert np.array_equal(out, ref.u_out), make.__name__
    _assert_sensitive(make_single, state, n_ok, ref.Nt, head, ref.u_out)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    sd = cases.make_sd("cart_mb11", "single")
    eng = engine.HipEngine(sd, slab_first=True, slab_last=True)
    eng.run(0, 3)
    eng.step_begin(3)
    with pytest.raises(engine.PfError, match="pffdtd_hip error 4") as ei:  # PF_ERR_STATE
        eng.save_state()
    assert ei.value.code == 4
    blank = engine._state_arrays(sd)[0]
    with pytest.raises(engine.PfError, match="pffdtd_hip error 4"):
        eng.load_state(blank)
    eng.step_end(3)
    st = eng.save_state()  # (between runs again)
    arr, cst = engine._state_arrays(sd, st)
    cst.vh1 = None  # a null array with Nbl > 0
    assert sd.Nbl > 0
    L = engine.lib()
    assert L.pf_engine_save_state(eng._h, ctypes.byref(cst)) == 1 and b"null" in L.pf_last_error()  # PF_ERR_ARG
    assert L.pf_engine_load_state(eng._h, ctypes.byref(cst)) == 1
    assert L.pf_engine_save_state(eng._h, None) == 1
    eng.load_state(blank)
    eng.close()
    sd2 = cases.make_sd("cart_mb11", "double")
    en = engine.HipEngine(sd2, energy=True)
    with pytest.raises(engine.PfError, match="pffdtd_hip error 4"):
        en.save_state()
    with pytest.raises(engine.PfError, match="pffdtd_hip error 4"):
        en.load_state(engine._state_arrays(sd2)[0])
    en.close()
    # a scene without frequency-dependent nodes: the four node arrays may be NULL
    sd3 = cases.make_sd("cart_rigid", "single")
    assert sd3.Nbl == 0
    er = engine.HipEngine(sd3)
    er.run(0, 5)
    st3 = er.save_state()
    er.load_state(st3)
    er.close()


# ---- 8. the command line ------------------------------------------------------------------------------------------------------------
def _cli(folder, *args):
    import os
    r = subprocess.run([sys.executable, "-m", "pffdtd_amd.fdtd_main", "--precision", "single", *args], cwd=folder,
                       env={**os.environ, "PYTHONPATH": str(ROOT)}, capture_output=True, text=True, timeout=300)
    return r


def _plates_room():
    """a room that run_single runs as TWO slabs cut along file z (pf__axis_exchange_pays): most of its boundary nodes sit on horizontal
    plates deep inside -- surfaces normal to z, whose nodes follow each other along file x -- and file x is the long axis"""
    n = (200, 76, 64)
    air = np.zeros(n, dtype=bool)
    air[3:-3, 3:-3, 3:-3] = True
    for z in range(18, 44, 5):
        air[18:-18, 18:-18, z] = False
    return synth.room(air, Nt=48, Nm=2, Mb=[11, 3], src=[100, 38, 30], rcv=[[102, 40, 30], [30, 30, 20], [170, 50, 35], [100, 10, 32]])


@pytest.mark.parametrize("scene", ["box", "two_slabs"])
def test_cli_stop_and_resume(tmp_path, scene):
    sim = synth.sort_sim(cases.make_sim("cart_mb11")) if scene == "box" else _plates_room()
    whole, parts = tmp_path / "whole", tmp_path / "parts"
    for d in (whole, parts):
        d.mkdir()
        synth.write_folder(sim, d)
    r = _cli(whole)
    assert r.returncode == 0, r.stderr[-2000:]
    assert ("--2 slabs on device" in r.stdout) == (scene == "two_slabs"), r.stdout[-1500:]
    ref = h5io.read(whole / "sim_outs.h5", "u_out")
    assert np.abs(ref).max() > 0
    r = _cli(parts, "--stop-after", str(STOP), "--checkpoint", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert not (parts / "sim_outs.h5").exists() and (parts / "ck.h5").exists() and f"stopped after {STOP}" in r.stdout, r.stdout[-1500:]
    r = _cli(parts, "--resume", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"--resumed at step {STOP}" in r.stdout
    got = h5io.read(parts / "sim_outs.h5", "u_out")
    assert got.tobytes() == ref.tobytes()
    # control: the same resume from a checkpoint whose branch state is zeroed gives other samples
    sd = sim_data.SimData.from_folder(parts, "single", build_mask=False)
    sd.scale_input()
    n, state, u_out = checkpoint.read(parts / "ck.h5", sd)
    assert n == STOP and np.count_nonzero(state["vh1"]) > 0
    sd.u_out[...] = u_out
    checkpoint.write(parts / "ck0.h5", sd, n, _zeroed(state))
    r = _cli(parts, "--resume", "ck0.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert h5io.read(parts / "sim_outs.h5", "u_out").tobytes() != ref.tobytes()


def test_cli_resume_refuses_a_folder_with_other_materials(tmp_path):
    sim = synth.sort_sim(cases.make_sim("cart_mb11"))
    synth.write_folder(sim, tmp_path)
    r = _cli(tmp_path, "--stop-after", str(STOP), "--checkpoint", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    other = tmp_path / "other"
    other.mkdir()
    sim2 = synth.sort_sim(cases.make_sim("cart_mb11"))
    sim2["sim_mats"]["mat_00_DEF"] = np.asarray(sim2["sim_mats"]["mat_00_DEF"]) * 1.01  # another sim_mats.h5
    synth.write_folder(sim2, other)
    r = _cli(other, "--resume", str(tmp_path / "ck.h5"))
    assert r.returncode != 0 and "cannot resume" in r.stderr and "mat_quads differs" in r.stderr, (r.stdout[-800:], r.stderr[-800:])
    assert not (other / "sim_outs.h5").exists()
