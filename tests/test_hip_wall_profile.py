"""GPU: wall profiles (pf_wall.h: wall_body<..., GD, HI, PR>).  Where every alike block of a three-step wall launch carries the node words of
a plain box wall -- two node layers at pencil depths 2 and 3, the inner one frequency-dependent or rigid --, the engine launches k_wall2 with
those words compiled in (pf_timing.wall_profile: bit 0 the x / y regions, bit 3 the column strips).  The profiled bodies make the same
upd7 / upd_rigid / fd_regs calls with the same operands as the bodies that read the words from their blocks (PF_DBG_RUNTIME_NODES, 0x20), so
both must leave every bit where the CPU oracle puts it.

Whole fields: every cell of both state grids between the two engines (ghost shell included, as the engine materialises it), and every interior
cell against the oracle (the oracle's ghost shell holds what its own mirror pass left there, the engine's is virtual: tests/test_hip_tb2.py
compares the same cells).  Receivers: all of them, all steps."""
import numpy as np
import pytest

import oracle
from pffdtd_amd import engine, sim_data, synth

pytestmark = pytest.mark.gpu

RUNTIME_NODES = 0x20  # csrc/pf_debug.h: PF_DBG_RUNTIME_NODES
N = (48, 100, 280)    # the box room of the test_three_steps_* tests (tests/test_hip_tb2.py: triple_scene)


def room(Nt, n=N, wall=3, Mb=(11, 3), **kw):
    """source in the middle; receivers beside it, in the wall layers of every axis and in the shell"""
    src = [n[0] // 2, n[1] // 2, n[2] // 2]
    lo, hi = wall + 1, [d - wall - 3 for d in n]
    rcv = [[src[0] + 2, src[1] - 1, src[2] + 3], [lo, src[1] - 3, src[2] + 2], [hi[0], src[1] + 2, src[2] - 5], [src[0], hi[1], src[2] + 4],
           [src[0] + 3, n[1] - 12, src[2] - 3], [lo + 1, lo, src[2] + 1], [src[0] - 2, src[1] + 1, hi[2]], [src[0] + 1, src[1] + 2, lo]]
    return synth.shoebox(*n, Nt=Nt, Nm=len(Mb), Mb=list(Mb), src=src, rcv=rcv, wall=wall, **kw)


def oracle_run(sim, numerics):
    sd = sim_data.SimData.from_sim(sim, "single")
    sd.scale_input()
    e = oracle.Engine(sd, safeguarded=numerics == engine.PF_NUM_GPU_SAFEGUARDED)
    for k in range(sd.Nt):
        e.step(k)
    ref = (sd.u_out.copy(), e.grid(0).copy(), e.grid(1).copy())
    e.close()
    assert np.abs(ref[0]).max() > 0 and np.abs(ref[2]).max() > 0
    return ref


def hip_run(sim, numerics, debug=0, pieces=None):
    sd = sim_data.SimData.from_sim(sim, "single", build_mask=False)
    sd.scale_input()
    eng = engine.HipEngine(sd, air_variant=40, timing=True, numerics=numerics, debug=debug)
    for n0, n in (pieces or ((0, sd.Nt),)):
        eng.run(n0, n)
    tm = eng.timing()
    got = (sd.u_out.copy(), eng.get_grid(0).copy(), eng.get_grid(1).copy())
    eng.close()
    assert tm["steps"] == sd.Nt, tm
    return got, tm


def same_bits(got, ref, what, interior=True):
    assert np.array_equal(got[0], ref[0]), (what, "receivers")
    for a, b in zip(got[1:], ref[1:]):
        if interior:
            a, b = a[1:-1, 1:-1, 1:-1], b[1:-1, 1:-1, 1:-1]
        assert np.array_equal(a, b), (what, "field")


def check(sim, numerics, want_profile, want3=9, pieces=None):
    """default engine (profile as `want_profile`), the same engine with run-time node words, the oracle: the same bits"""
    ref = oracle_run(sim, numerics)
    got, tm = hip_run(sim, numerics, pieces=pieces)
    assert tm["tb2_launches"] > 0 and (sum(tm["wall_blocks"]) > 0 or not want_profile), tm
    assert tm["wall_three_steps"] == want3 and tm["wall_profile"] == want_profile, tm
    rt, tm_rt = hip_run(sim, numerics, debug=RUNTIME_NODES, pieces=pieces)
    assert tm_rt["wall_three_steps"] == want3 and tm_rt["wall_profile"] == 0, tm_rt
    same_bits(got, ref, "profile against the oracle")
    same_bits(rt, ref, "run-time node words against the oracle")
    same_bits(got, rt, "profile against run-time node words", interior=False)
    return tm


@pytest.mark.parametrize("numerics", [engine.PF_NUM_CPU_EXACT, engine.PF_NUM_GPU_SAFEGUARDED], ids=["exact", "safeguarded"])
@pytest.mark.parametrize("Mb", [(1, 1), (4, 3), (11, 3), (12, 3)], ids=["Mb1", "Mb4", "Mb11", "Mb12"])
def test_profiled_walls_give_the_oracles_bits(Mb, numerics):
    """Branch counts 1 and 4 (kernels that move four branch states per node) and 11 and 12 (twelve), two materials with different counts.  41
    steps: thirteen triples and a closing PAIR, which the x / y regions take with their two-step kernel (no profile there)."""
    tm = check(room(41, Mb=Mb), numerics, 9)
    assert tm["tb_steps_per_pass"] == 3 and tm["wall_bricks"] > 0, tm


@pytest.mark.parametrize("numerics", [engine.PF_NUM_CPU_EXACT, engine.PF_NUM_GPU_SAFEGUARDED], ids=["exact", "safeguarded"])
def test_profiled_rigid_walls_give_the_oracles_bits(numerics):
    """lossy=False: both node layers rigid -- the profile without a frequency-dependent node, whatever the materials' branch counts."""
    check(room(41, lossy=False), numerics, 9)


def test_profiled_walls_across_run_boundaries():
    """run(0, 7); run(7, 13); run(20, 20): runs that end in a single step, in a single step after four triples, and in a pair."""
    check(room(40), engine.PF_NUM_CPU_EXACT, 9, pieces=((0, 7), (7, 13), (20, 20)))


def test_profiled_walls_in_another_room():
    """other extents on every axis (odd ones; a second column tile of the box kernel): the profile's words depend on (mode, side, pencil) only"""
    check(room(20, n=(47, 101, 528)), engine.PF_NUM_CPU_EXACT, 9)


def test_deeper_walls_take_no_profile():
    """wall=4: node layers at depths 3 and 4 -- no three-step regions at all for this room (the engine steps in pairs), and no profile"""
    tm = check(room(23, n=(50, 96, 280), wall=4), engine.PF_NUM_CPU_EXACT, 0, want3=0)
    assert tm["tb_steps_per_pass"] == 2, tm


def test_mixed_node_structure_takes_no_profile():
    """every 13th frequency-dependent node rigid: the blocks' pencils differ, so neither three steps in one pass nor a profile"""
    tm = check(room(31, rigid_every=13), engine.PF_NUM_CPU_EXACT, 0, want3=0)
    assert tm["wall_blocks"][1] > 0, tm


def test_a_profile_needs_every_block():
    """One frequency-dependent node of the x-low wall made rigid by hand, in the middle of a block: that block's pencils differ, so the x / y
    regions report no profile (they fall back to two steps + one), and no region reports a profile without three steps in one pass."""
    sim = room(25)
    v = sim["vox_out"]
    ix, iy, iz = synth._ind2sub(v["bn_ixyz"], N[1], N[2])
    k = np.flatnonzero((ix == 3) & (iy == 50) & (iz == 140))
    assert k.size == 1 and v["mat_bn"][k[0]] >= 0
    v["mat_bn"][k[0]] = -1
    ref = oracle_run(sim, engine.PF_NUM_CPU_EXACT)
    got, tm = hip_run(sim, engine.PF_NUM_CPU_EXACT)
    assert (tm["wall_profile"] & 1) == 0 and (tm["wall_profile"] & ~tm["wall_three_steps"]) == 0, tm
    same_bits(got, ref, "one rigid node among the frequency-dependent ones")


def test_two_materials_with_different_branch_counts():
    """Nm = 3 with 11, 3 and 7 branches, assigned cell by cell ((x + 2 y + 3 z) mod 3): every wave of the wall kernels holds nodes of all three,
    so branches beyond a node's own count must leave its value and state alone."""
    check(room(29, Mb=(11, 3, 7)), engine.PF_NUM_CPU_EXACT, 9)
