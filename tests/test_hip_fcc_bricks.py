"""GPU: 13-point blocked pairs with the whole shell in bricks (air_variant 42: pf_brick_fcc.h / pf_fcc_shell_cut.h /
Engine::step_pair_fcc_bricks) must leave every bit where the CPU oracle puts it.  Scenes are the smallest folded FCC grids at which a
13-point box exists (tests/test_hip_tb2.py: fcc_scene); every engine is created with timing on and must report pair launches and bricks."""
import functools
import re

import numpy as np
import pytest

import oracle
import rooms
from pffdtd_amd import engine, sim_data, synth

pytestmark = pytest.mark.gpu

NUMERICS = [(engine.PF_NUM_CPU_EXACT, "exact"), (engine.PF_NUM_GPU_SAFEGUARDED, "safeguarded")]
REASON = "13-point pairs with the shell in bricks"


def fcc_scene(n=(36, 70, 280), Nt=25, src=None, blocks=(), wall=3, rcv=None, Nm=2, Mb=(11, 3)):
    """folded FCC room with a stored grid of n (unfolded Ny = 2 (n[1] - 1)), as tests/test_hip_tb2.py builds it"""
    Nyu = 2 * (n[1] - 1)
    src = src or [n[0] // 2, n[1] // 2, n[2] // 2]
    src = [src[0], src[1], src[2] + (sum(src) % 2)]  # an existing (even) node of the subgrid
    rcv = rcv or [[src[0] + dx, src[1] + dy, src[2] + dz + ((dx + dy + dz) % 2)] for dx, dy, dz in ((2, 3, -4), (-5, 2, 6), (3, -6, 9), (-2, -3, -8))]
    sim = synth.shoebox(n[0], Nyu, n[2], Nt=Nt, fcc=True, Nm=Nm, Mb=list(Mb), src=src, rcv=rcv, blocks=blocks, wall=wall)
    synth.fold_fcc(sim)
    synth.sort_sim(sim)
    return sim


def even(p):
    return [p[0], p[1], p[2] + (sum(p) % 2)]


def box_room(Nt=25):
    """scene 1: source at the centre, receivers near it and three cells off four walls (x low, x high, y low, z low)"""
    n = (36, 70, 280)
    c = even([18, 35, 140])
    rcv = [even(p) for p in ([20, 38, 136], [13, 37, 146], [6, 33, 141], [29, 36, 139], [17, 6, 142], [19, 34, 6])]
    return fcc_scene(n=n, Nt=Nt, src=c, rcv=rcv)


def run42(sim, prec, numerics=engine.PF_NUM_CPU_EXACT, variant=42, init=None, pieces=None, **kw):
    sd = sim_data.SimData.from_sim(sim, prec, build_mask=False)
    sd.scale_input()
    eng = engine.HipEngine(sd, air_variant=variant, timing=True, numerics=numerics, **kw)
    try:
        if init is not None:
            for k in (0, 1):
                eng.set_grid(k, init[k])
        for n0, ns in (pieces or [(0, sd.Nt)]):
            eng.run(n0, ns)
        tm = eng.timing()
        g = [eng.get_grid(0).copy(), eng.get_grid(1).copy()]
    finally:
        eng.close()
    return sd.u_out.copy(), g, tm


@functools.lru_cache(maxsize=None)
def _oracle_from_source(key, prec, safeguarded):
    sim = SCENES[key]()
    ref = sim_data.SimData.from_sim(sim, prec)
    ref.scale_input()
    e = oracle.Engine(ref, safeguarded=safeguarded)
    for i in range(ref.Nt):
        e.step(i)
    g = [e.grid(0).copy(), e.grid(1).copy()]
    e.close()
    for a in g:
        a.setflags(write=False)
    out = ref.u_out.copy()
    out.setflags(write=False)
    return out, g


def _oracle_from_fields(sim, prec, init, safeguarded=False):
    ref = sim_data.SimData.from_sim(sim, prec)
    ref.scale_input()
    e = oracle.Engine(ref, safeguarded=safeguarded)
    for k in (0, 1):
        e.grid(k)[...] = init[k]
    for i in range(ref.Nt):
        e.step(i)
    g = [e.grid(0).copy(), e.grid(1).copy()]
    e.close()
    return ref.u_out.copy(), g


def interior(a):
    return a[1:-1, 1:-1, 1:-1]


def assert_bricks(tm):
    assert tm["tb2_launches"] > 0 and tm["fcc_shell_bricks"] > 0, tm


SCENES = {
    "box": box_room,
    "blocks": lambda: fcc_scene(Nt=45, blocks=((12, 17, 20, 40, 60, 130), (22, 24, 8, 12, 150, 260)), src=[19, 45, 138]),
    "balcony": lambda: rooms.build_fcc("balcony", 45),
}


# ---- 1. box room ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["single", "double"])
@pytest.mark.parametrize("numerics,label", NUMERICS, ids=[m[1] for m in NUMERICS])
def test_box_room_gives_the_oracles_bits(prec, numerics, label):
    """36 x 70 x 280, Mb = [11, 3], 25 steps: receivers near the source and three cells off four walls equal the oracle's in the same
    numerics, both state grids' interiors the single-step engine's; receiver rings of the default depth and of 6 steps."""
    sg = numerics == engine.PF_NUM_GPU_SAFEGUARDED
    ref_out, ref_g = _oracle_from_source("box", prec, sg)
    assert (np.abs(ref_out).max(axis=1) > 0).sum() >= 3  # (the source's neighbours and the x walls' receivers are reached in 25 steps)
    sim = box_room()
    base_out, base_g, tm0 = run42(sim, prec, numerics, variant=0, debug=0x4000)  # single steps
    assert tm0["tb2_launches"] == 0 and tm0["fcc_shell_bricks"] == 0 and np.array_equal(base_out, ref_out)
    for chunk in (0, 6):
        out, g, tm = run42(sim, prec, numerics, readout_chunk=chunk)
        assert_bricks(tm)
        assert np.array_equal(out, ref_out), chunk
        for a, b, c in zip(g, base_g, ref_g):
            assert np.array_equal(interior(a), interior(b)), chunk
            assert np.array_equal(interior(a), interior(c)), chunk


# ---- 2. every ghost live --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["single", "double"])
@pytest.mark.parametrize("numerics,label", NUMERICS, ids=[m[1] for m in NUMERICS])
def test_every_ghost_live_from_random_fields(prec, numerics, label):
    """38 x 67 x 286, walls at depth 7, seeded random u^{n-1}, u^n, 10 steps: the reflected-ghost rule on faces, edges, corners and the
    fold row, ABC counts 1-3 -- every interior cell against the oracle stepped from the same fields."""
    n = (38, 67, 286)
    sim = fcc_scene(n=n, Nt=10, wall=7, src=[19, 33, 143])
    dt = np.float32 if prec == "single" else np.float64
    rng = np.random.default_rng(29)
    init = [(rng.standard_normal(n) * 1e-2).astype(dt) for _ in range(2)]
    ref_out, ref_g = _oracle_from_fields(sim, prec, init, numerics == engine.PF_NUM_GPU_SAFEGUARDED)
    out, g, tm = run42(sim, prec, numerics, init=init)
    assert_bricks(tm)
    assert np.array_equal(out, ref_out)
    for a, b in zip(g, ref_g):
        assert np.array_equal(interior(a), interior(b))


# ---- 3. branch state ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["single", "double"])
@pytest.mark.parametrize("mb", [[12, 5], [1], [4, 2], [11, 3, 7]], ids=["Mb12_5", "Mb1", "Mb4_2", "Mb11_3_7"])
def test_branch_state_over_many_pairs(mb, prec):
    """38 x 67 x 280 (the unfolded 13-point grid needs even dimensions, as the reference's setup does: 37 planes cannot be built), materials
    with 12 / 5, 1, 4 / 2 and 11 / 3 / 7 branches mixed along the walls, 63 steps from random fields: the branch state double buffer, both
    branch-slot bounds of the kernel, node values through the five buffers -- receivers and every interior cell against the oracle."""
    n = (38, 67, 280)
    rcv = [even(p) for p in ([21, 36, 138], [6, 30, 140], [31, 31, 139], [18, 6, 142], [20, 33, 6], [19, 34, 273])]
    sim = fcc_scene(n=n, Nt=63, src=[18, 33, 140], rcv=rcv, Nm=len(mb), Mb=mb)
    dt = np.float32 if prec == "single" else np.float64
    rng = np.random.default_rng(31)
    init = [(rng.standard_normal(n) * 1e-2).astype(dt) for _ in range(2)]
    ref_out, ref_g = _oracle_from_fields(sim, prec, init)
    out, g, tm = run42(sim, prec, init=init)
    assert_bricks(tm)
    assert np.array_equal(out, ref_out)
    for a, b in zip(g, ref_g):
        assert np.array_equal(interior(a), interior(b))


# ---- 4. geometry in the box and at the shell ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["single", "double"])
@pytest.mark.parametrize("key", ["blocks", "balcony"])
def test_geometry_in_the_box_and_at_the_shell(key, prec, monkeypatch, capfd):
    """The two-block room (both blocks inside the box: single-step tiles, their nodes with the list kernel) and the balcony that hangs on
    the x-high wall and reaches into the box, 45 steps -- the oracle's receivers and the oracle's fields.  The balcony's nodes lie partly in
    bricks and partly in the rest list: the engine's own account (its PFFDTD_VERBOSE line) must leave some boundary nodes to the list kernel,
    and fewer than the balcony has -- a plain box leaves none, so the others are bricks'."""
    ref_out, ref_g = _oracle_from_source(key, prec, False)
    assert np.abs(ref_out).max() > 0
    sim = SCENES[key]()
    monkeypatch.setenv("PFFDTD_VERBOSE", "1")
    for chunk in (0, 6):
        capfd.readouterr()
        out, g, tm = run42(sim, prec, readout_chunk=chunk)
        said = re.findall(r"13-point shell in bricks:.* (\d+) of (\d+) boundary nodes left to the list kernel", capfd.readouterr().err)
        assert_bricks(tm)
        assert tm["tb2_dirty_tiles"] > 0, tm
        assert said, "the engine did not say how it cut the shell"
        rest = int(said[-1][0])
        if key == "balcony":
            sd = sim_data.SimData.from_sim(sim, prec, build_mask=False)
            x, z = sd.bn_ixyz // (sd.Ny * sd.Nz), sd.bn_ixyz % sd.Nz
            balcony = int(((x >= 27) & (x <= 31) & (z >= 59) & (z <= 64)).sum())  # the nodes around air[28:, 30:110, 60:64] in front of the x-high wall's layers
            assert 0 < rest < balcony, (rest, balcony)
        else:
            assert rest > 0, rest
        assert np.array_equal(out, ref_out), chunk
        for a, b in zip(g, ref_g):
            assert np.array_equal(interior(a), interior(b)), chunk


# ---- 4b. the arrangement that runs without per-launch events -------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["single", "double"])
@pytest.mark.parametrize("key", ["box", "blocks"])
def test_timing_off_bricks_run_beside_the_pair_kernel(key, prec):
    """With per-launch events on, the pair kernel waits for the bricks (its recorded duration is its own); with them off -- what callers and
    the benchmark run -- bricks, the box's single-step tiles and the rest nodes run BESIDE it on the second stream.  Timing switched off
    after creation: the same bits, and the engine still counts its bricks."""
    ref_out, ref_g = _oracle_from_source(key, prec, False)
    sim = SCENES[key]()
    sd = sim_data.SimData.from_sim(sim, prec, build_mask=False)
    sd.scale_input()
    eng = engine.HipEngine(sd, air_variant=42, timing=True)
    try:
        eng.set_timing(False)
        eng.run(0, sd.Nt)
        tm = eng.timing()
        g = [eng.get_grid(0).copy(), eng.get_grid(1).copy()]
    finally:
        eng.close()
    assert tm["fcc_shell_bricks"] > 0 and tm["tb2_launches"] == 0, tm  # (no events: no launches counted)
    assert np.array_equal(sd.u_out, ref_out)
    for a, b in zip(g, ref_g):
        assert np.array_equal(interior(a), interior(b))


# ---- 5. run pieces --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["single", "double"])
def test_run_pieces_mix_pairs_and_closing_single_steps(prec):
    """run(0, 7); run(7, 6); run(13, 1); run(14, Nt - 14): pairs, closing single steps with their flips in memory, pairs again"""
    ref_out, ref_g = _oracle_from_source("box", prec, False)
    sim = box_room()
    out, g, tm = run42(sim, prec, pieces=[(0, 7), (7, 6), (13, 1), (14, 25 - 14)])
    assert_bricks(tm)
    assert np.array_equal(out, ref_out)
    for a, b in zip(g, ref_g):
        assert np.array_equal(interior(a), interior(b))


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def _create(sim, **kw):
    sd = sim_data.SimData.from_sim(sim, "single", build_mask=False)
    sd.scale_input()
    engine.HipEngine(sd, air_variant=42, **kw).close()


def test_a_seven_point_scene_is_refused():
    sim = synth.shoebox(36, 64, 280, Nt=8, Nm=2, Mb=[11, 3], src=[18, 32, 140], rcv=[[20, 30, 141]])
    with pytest.raises(engine.PfError, match=REASON + ".*not a folded FCC grid"):
        _create(sim)


def test_a_slab_of_a_chain_is_refused():
    with pytest.raises(engine.PfError, match=REASON + ".*slab of a chain"):
        _create(box_room(8), slab_first=False)


def test_exchanged_storage_is_refused():
    with pytest.raises(engine.PfError, match=REASON + ".*PF_LAYOUT_EXCHANGED"):
        _create(box_room(8), layout=engine.PF_LAYOUT_EXCHANGED)


def test_a_source_two_cells_off_the_shell_is_refused():
    """the box of this room begins at x = 5: a source at x = 6 is two cells from the shell cell at x = 4"""
    sim = fcc_scene(Nt=8, src=[6, 35, 141], rcv=[[18, 35, 141]])
    with pytest.raises(engine.PfError, match=REASON + ".*source.*within 2 cells of the shell"):
        _create(sim)
    _create(fcc_scene(Nt=8, src=[7, 35, 140], rcv=[[18, 35, 141]]))  # three cells: fine


# ---- 7. unchanged ---------------------------------------------------------------------------------------------------------------------
def test_variant_40_is_unchanged():
    ref_out, ref_g = _oracle_from_source("box", "single", False)
    out, g, tm = run42(box_room(), "single", variant=40)
    assert tm["tb2_launches"] > 0 and tm["fcc_shell_bricks"] == 0, tm
    assert np.array_equal(out, ref_out)
    for a, b in zip(g, ref_g):
        assert np.array_equal(interior(a), interior(b))
