"""GPU: the uniform-branch-count form of the profiled three-step wall kernels (pf_wall.h: fd_regs<..., UNI>, wall_body<..., UB, USK>) and the
u^{n+1} stores they leave out where nothing reads them.

Where every material of a scene has the same number of branches -- 11 or 12 (their own instantiations) or 1 .. 4 (the four-branch kernel, surplus
branches skipped by a wave-uniform test) -- the engine launches bodies without the per-node guard (pf_timing.wall_uniform_branches: that count;
0: the guarded form, which other counts and mixed counts keep).  A launch group of such bodies whose cells hold no receiver does not store
u^{n+1} into the scratch grid in a triple where nothing steps singly (pf_timing.wall_unread_skipped: bit 0 the x / y regions, bit 3 the column
strips).  Both forms make the same arithmetic in the same order, so every case must leave every bit where the CPU oracle puts it, and where the
forcing switches (PF_DBG_BRANCH_SELECTS | PF_DBG_STORE_UNREAD) put it: all receivers, both state grids."""
import numpy as np
import pytest

import oracle
from pffdtd_amd import engine, sim_data, synth

pytestmark = pytest.mark.gpu

BRANCH_SELECTS, STORE_UNREAD = 0x1, 0x2  # csrc/pf_debug.h
N = (48, 100, 280)                       # the box room of tests/test_hip_wall_profile.py
SRC = [N[0] // 2, N[1] // 2, N[2] // 2]
IN_BOX = [[SRC[0] + 2, SRC[1] - 1, SRC[2] + 3], [SRC[0] - 3, SRC[1] + 4, SRC[2] - 6]]  # receivers well inside the box kernel's cells
IN_X_WALL = [4, SRC[1] - 3, SRC[2] + 2]  # in the air cells of the x-low wall region (wall = 3: node layers at 2 and 3)
IN_STRIP = [SRC[0] + 1, SRC[1] + 2, 4]   # ... of the z-low column strip
NUMERICS = pytest.mark.parametrize("numerics", [engine.PF_NUM_CPU_EXACT, engine.PF_NUM_GPU_SAFEGUARDED], ids=["exact", "safeguarded"])


def room(Nt, Mb, rcv=None):
    """rcv = None: receivers beside the source, in the wall layers of every axis and in the shell (every region keeps its stores)"""
    if rcv is None:
        lo, hi = 4, [d - 6 for d in N]
        rcv = [IN_BOX[0], [lo, SRC[1] - 3, SRC[2] + 2], [hi[0], SRC[1] + 2, SRC[2] - 5], [SRC[0], hi[1], SRC[2] + 4],
               [SRC[0] + 3, N[1] - 12, SRC[2] - 3], [lo + 1, lo, SRC[2] + 1], [SRC[0] - 2, SRC[1] + 1, hi[2]], [SRC[0] + 1, SRC[1] + 2, lo]]
    return synth.shoebox(*N, Nt=Nt, Nm=len(Mb), Mb=list(Mb), src=SRC, rcv=rcv, wall=3)


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
        if interior:  # (the oracle's ghost shell holds what its mirror pass left there, the engine's is virtual: tests/test_hip_tb2.py)
            a, b = a[1:-1, 1:-1, 1:-1], b[1:-1, 1:-1, 1:-1]
        assert np.array_equal(a, b), (what, "field")


def check(sim, numerics, want_uniform, want_skipped, pieces=None):
    """default engine (forms as stated), the same engine with the guarded form and every store forced, the oracle: the same bits"""
    ref = oracle_run(sim, numerics)
    got, tm = hip_run(sim, numerics, pieces=pieces)
    print("timing:", {k: tm[k] for k in ("wall_three_steps", "wall_profile", "wall_uniform_branches", "wall_unread_skipped", "tb2_dirty_tiles")})
    assert tm["tb_steps_per_pass"] == 3 and tm["wall_three_steps"] == 9 and tm["wall_profile"] == 9, tm
    assert tm["wall_uniform_branches"] == want_uniform and tm["wall_unread_skipped"] == want_skipped, tm
    forced, tm_f = hip_run(sim, numerics, debug=BRANCH_SELECTS | STORE_UNREAD, pieces=pieces)
    assert tm_f["wall_profile"] == 9 and tm_f["wall_uniform_branches"] == 0 and tm_f["wall_unread_skipped"] == 0, tm_f
    same_bits(got, ref, "default forms against the oracle")
    same_bits(forced, ref, "guarded form, every store, against the oracle")
    same_bits(got, forced, "default forms against the forced ones", interior=False)
    return tm


@NUMERICS
@pytest.mark.parametrize("Mb", [(11,), (11, 11, 11), (12,), (4, 4), (1,)], ids=["Mb11", "Mb11x3", "Mb12", "Mb4x2", "Mb1"])
def test_uniform_counts_give_the_oracles_bits(Mb, numerics):
    """One and three materials with 11 branches (the headline's case), 12, and the four-branch kernel's 4 and 1.  41 steps: thirteen triples
    and a closing pair; receivers in every region, so all stores stay."""
    check(room(41, Mb), numerics, Mb[0], 0)


@NUMERICS
def test_uniform_counts_without_unread_stores(numerics):
    """the same with every receiver inside the box: both launch groups leave u^{n+1} of their cells out, 41 = 3 * 13 + 2 steps"""
    check(room(41, (11,), rcv=IN_BOX), numerics, 11, 9)


def test_an_uninstantiated_uniform_count_keeps_the_guarded_form():
    """seven branches everywhere: no instantiation of the uniform form (11, 12 and 1 .. 4 have one), so the guarded one runs -- and stores"""
    check(room(29, (7, 7), rcv=IN_BOX), engine.PF_NUM_CPU_EXACT, 0, 0)


def test_mixed_counts_keep_the_guarded_form():
    check(room(29, (11, 3, 7), rcv=IN_BOX), engine.PF_NUM_CPU_EXACT, 0, 0)


@pytest.mark.parametrize("rcv, skipped", [(IN_BOX + [IN_X_WALL], 8), (IN_BOX + [IN_STRIP], 1), (IN_BOX + [IN_X_WALL, IN_STRIP], 0)],
                         ids=["x-wall", "strip", "both"])
def test_a_receiver_in_a_region_keeps_that_groups_stores(rcv, skipped):
    """k_io of step n + 1 reads u^{n+1} at the receivers: the group that owns such a cell stores, the other does not"""
    check(room(32, (11,), rcv=rcv), engine.PF_NUM_CPU_EXACT, 11, skipped)


@pytest.mark.parametrize("Mb", [(11,), (4, 4)], ids=["Mb11", "Mb4x2"])
def test_uniform_counts_across_run_boundaries(Mb):
    """run(0, 7); run(7, 13): runs that end in a single step after two and after four triples, the scratch grid's wall cells never written"""
    check(room(20, Mb, rcv=IN_BOX), engine.PF_NUM_CPU_EXACT, Mb[0], 9, pieces=((0, 7), (7, 13)))
