"""GPU: the staged form of the three-step column-strip kernels (pf_wall.h: wall_body's STG bodies, csrc/pf_strip_map.h).

Where every material of a scene has the same branch count (11, 12, or 1 .. 4), the column strips' three-step kernel loads and stores its tile row
by row -- consecutive lanes move consecutive 16 bytes of one row -- and turns rows into pencils and back in LDS (pf_timing.wall_strips_staged = 1).
PF_DBG_STRIPS_PER_LANE launches the per-lane form of the same bodies (every lane loads and stores its own pencil), and scenes with mixed counts have no
staged body at all: both report 0.  The staged form re-orders which lane issues which address and nothing else, so every case must leave every bit where
the CPU oracle puts it: every receiver sample, every interior cell of both state grids.

Shapes: 280 columns is the narrowest grid whose strips take three steps per pass; 70 rows make one whole lane tile and a short one, 67 a partial last
tile of another length.  7 steps = two triples and a single step, 8 = two triples and a pair.  One receiver sits in the air cells of the z-low strip (so
that the strip launch stores u^{n+1} as well, through the tile), one in the box; one case keeps both in the box (the strips then leave u^{n+1} out)."""
import numpy as np
import pytest

import oracle
from pffdtd_amd import engine, sim_data, synth

pytestmark = pytest.mark.gpu

STRIPS_PER_LANE = 0x4  # csrc/pf_debug.h
SHAPES = [(40, 70, 280), (38, 67, 280)]


def room(N, Nt, Mb, strip_rcv=True):
    src = [N[0] // 2, N[1] // 2, N[2] // 2]
    in_box = [src[0] + 2, src[1] - 1, src[2] + 3]
    second = [src[0] + 1, src[1] + 2, 4] if strip_rcv else [src[0] - 3, src[1] + 4, src[2] - 6]  # z = 4: an air cell of the z-low strip (wall = 3)
    return synth.shoebox(*N, Nt=Nt, Nm=len(Mb), Mb=list(Mb), src=src, rcv=[in_box, second], wall=3)


def oracle_run(sim):
    sd = sim_data.SimData.from_sim(sim, "single")
    sd.scale_input()
    e = oracle.Engine(sd, safeguarded=False)
    for k in range(sd.Nt):
        e.step(k)
    ref = (sd.u_out.copy(), e.grid(0).copy(), e.grid(1).copy())
    e.close()
    assert np.abs(ref[0]).max() > 0 and np.abs(ref[2]).max() > 0
    return ref


def hip_run(sim, debug=0):
    sd = sim_data.SimData.from_sim(sim, "single", build_mask=False)
    sd.scale_input()
    eng = engine.HipEngine(sd, air_variant=40, timing=True, numerics=engine.PF_NUM_CPU_EXACT, debug=debug)
    eng.run(0, sd.Nt)
    tm = eng.timing()
    got = (sd.u_out.copy(), eng.get_grid(0).copy(), eng.get_grid(1).copy())
    eng.close()
    assert tm["steps"] == sd.Nt, tm
    return got, tm


def same_bits(got, ref, what):
    assert got[0].shape == ref[0].shape and np.array_equal(got[0], ref[0]), (what, "receivers")
    for a, b in zip(got[1:], ref[1:]):
        assert a.shape == b.shape, (what, a.shape, b.shape)
        # (every interior cell; the oracle's ghost shell holds what its mirror pass left there, the engine's is virtual: tests/test_hip_tb2.py)
        assert np.array_equal(a[1:-1, 1:-1, 1:-1], b[1:-1, 1:-1, 1:-1]), (what, "field")


def check(sim, want_staged, want_uniform):
    ref = oracle_run(sim)
    got, tm = hip_run(sim)
    print("timing:", {k: tm[k] for k in ("wall_three_steps", "wall_profile", "wall_uniform_branches", "wall_unread_skipped", "wall_strips_staged")})
    assert tm["tb_steps_per_pass"] == 3 and tm["wall_three_steps"] & 8, tm  # the strips take three steps in one pass
    assert tm["wall_uniform_branches"] == want_uniform and tm["wall_strips_staged"] == want_staged, tm
    per_lane, tm_p = hip_run(sim, debug=STRIPS_PER_LANE)
    assert tm_p["wall_three_steps"] & 8 and tm_p["wall_uniform_branches"] == want_uniform and tm_p["wall_strips_staged"] == 0, tm_p
    same_bits(got, ref, "default form against the oracle")
    same_bits(per_lane, ref, "per-lane form against the oracle")
    return tm


@pytest.mark.parametrize("Nt", [7, 8])
@pytest.mark.parametrize("Mb", [(11,), (12,), (4,)], ids=["Mb11", "Mb12", "Mb4-skip"])
@pytest.mark.parametrize("N", SHAPES, ids=["40x70x280", "38x67x280"])
def test_staged_strips_give_the_oracles_bits(N, Mb, Nt):
    """one material with 11 branches (the headline's kernel), 12, and four (the kernel that skips surplus branches by a wave-uniform test)"""
    check(room(N, Nt, Mb), 1, Mb[0])


@pytest.mark.parametrize("Nt", [7, 8])
def test_staged_strips_that_leave_the_unread_field_out(Nt):
    """both receivers in the box: the strips store u^{n+2} and u^{n+3} only (the headline's arrangement)"""
    tm = check(room(SHAPES[0], Nt, (11,), strip_rcv=False), 1, 11)
    assert tm["wall_unread_skipped"] & 8, tm


def test_mixed_branch_counts_keep_the_per_lane_form():
    """no staged body exists for the guarded kernels: the per-lane form is reported, and the bits are the oracle's"""
    check(room(SHAPES[1], 8, (11, 3, 7)), 0, 0)
