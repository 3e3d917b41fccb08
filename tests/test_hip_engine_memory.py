"""GPU: creating and closing an engine gives the device back everything it took -- on every creation path, the one that fails late included.

Per case: one creation + close as a warm-up (the runtime loads code objects and grows its own pools on first use), free device memory read after
torch.cuda.synchronize(), three more creations + closes, free memory read again.  drift = free before - free after.  Two caps:
  * below the bytes of ONE state grid of the case -- a leaked grid (state, spare, scratch, placement candidate) is always caught;
  * at most what the same test showed on the commit before the engine's allocations got one owner (csrc/pf_devmem.h), plus 2 MiB, the runtime's
    allocation granule: that commit's success paths free everything by reading, so its drift is the runtime's own.
profiles/engine_memory_drift.txt, measured once with this file on that commit's build (one MI355X, bytes: drift, one state grid):
    box_fp32 0 / 44390400, narrow_fp32 0 / 26880000, narrow_fp64 0 / 37632000, fcc_bricks 0 / 2903040, place_grids 0 / 3612672, late_failure 0 / 5529600
(the late failure leaks nothing there either: every list and table it had uploaded was one the old destroy() named).
Cases, at the small shapes the suite already uses for these paths: box_fp32 (tests/test_hip_autotune.py: a box exists, so pairs or triples and their
wall regions are built and measured, placement candidates allocated and dropped), narrow_fp32 (single steps, measured into a scratch grid),
narrow_fp64, fcc_bricks (tests/test_hip_fcc_bricks.py: the smallest folded 13-point scene, air_variant 42), place_grids (tests/test_hip_slabs.py:
slab 0 of two of a 96 x 64 x 280 room, a caller-owned pool of five, pairs forced: the wall tables are built inside pf_engine_place_grids; the
caller's tensors must be readable and zero after close()), late_failure (tests/test_hip_rooms.py: leaning_z with air_variant 40 -- PF_ERR_ARG "no
boundary-free tiles" after every list and table is uploaded)."""
import pytest
import torch

import rooms
from pffdtd_amd import engine, sim_data, slab, synth
from test_hip_fcc_bricks import fcc_scene

pytestmark = pytest.mark.gpu

GRANULE = 2 << 20
# profiles/engine_memory_drift.txt
PARENT_DRIFT = {"box_fp32": 0, "narrow_fp32": 0, "narrow_fp64": 0, "fcc_bricks": 0, "place_grids": 0, "late_failure": 0}


def _sd(sim, prec):
    sd = sim_data.SimData.from_sim(sim, prec, build_mask=False)
    sd.scale_input()
    return sd


def _shoebox(n, prec):
    rcv = [[n[0] // 2 + 3, n[1] // 2, n[2] // 2 - 2], [6, 7, 8], [n[0] - 9, n[1] - 10, n[2] - 11]]
    return _sd(synth.shoebox(*n, Nt=12, Nm=2, Mb=[11, 3], rcv=rcv), prec)


def _grid_bytes(sd, rb):
    """one state grid, in whichever of the two storage orders is smaller"""
    return min(sd.Nx * sd.Ny * engine.grid_pitch(sd.Nz, rb), sd.Nz * sd.Ny * engine.grid_pitch(sd.Nx, rb)) * rb


def _automatic(n, prec):
    sd = _shoebox(n, prec)
    return sd, (lambda: engine.HipEngine(sd, device=0).close()), None


def _fcc_bricks():
    sd = _sd(fcc_scene(Nt=8), "single")

    def create():
        eng = engine.HipEngine(sd, device=0, air_variant=42)
        tm = eng.timing()
        eng.close()
        assert tm["fcc_shell_bricks"] > 0, tm
    return sd, create, None


def _place_grids():
    full = _sd(synth.shoebox(96, 64, 280, Nt=6, Nm=2, Mb=[11, 3], src=None, rcv=[[50, 30, 140]]), "single")
    loc, info = slab.split(full, 2, 0)
    P = engine.grid_pitch(loc.Nz, 4)
    pool = [torch.zeros((loc.Nx, loc.Ny * P), dtype=torch.float32, device="cuda:0") for _ in range(5)]
    ptrs = [g.data_ptr() for g in pool]

    def create():
        eng = engine.HipEngine(loc, device=0, slab_first=info.first, slab_last=info.last, x_global0=info.xlo, air_variant=40,
                               ext_u0=ptrs[0], ext_u1=ptrs[1])
        paired, idx = eng.place_grids(ptrs)
        tm = eng.timing()
        eng.close()
        assert paired and sorted(set(idx)) == sorted(idx) and sum(tm["wall_blocks"]) > 0, (paired, idx, tm)

    def after():  # the pool is the caller's: close() freed none of it
        torch.cuda.synchronize()
        assert all(float(g.abs().max()) == 0.0 for g in pool)
    return loc, create, after


def _late_failure():
    sd = _sd(rooms.build("leaning_z", 11), "single")

    def create():
        with pytest.raises(engine.PfError, match="no boundary-free tiles"):
            engine.HipEngine(sd, device=0, air_variant=40)
    return sd, create, None


CASES = {
    "box_fp32": lambda: _automatic((96, 340, 340), "single"),
    "narrow_fp32": lambda: _automatic((150, 140, 309), "single"),
    "narrow_fp64": lambda: _automatic((160, 140, 210), "double"),
    "fcc_bricks": _fcc_bricks,
    "place_grids": _place_grids,
    "late_failure": _late_failure,
}


def _free():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


@pytest.mark.parametrize("case", list(CASES))
def test_creating_and_closing_returns_the_device_memory(case):
    sd, create, after = CASES[case]()
    create()  # warm-up
    free0 = _free()
    for _ in range(3):
        create()
    drift = free0 - _free()
    grid = _grid_bytes(sd, 8 if case == "narrow_fp64" else 4)
    print(f"engine memory drift [{case}]: {drift} bytes over three creations (one state grid: {grid} bytes, parent: {PARENT_DRIFT[case]})")
    if after:
        after()
    assert drift < grid, f"{case}: {drift} bytes gone after three creations -- a state grid of this case has {grid}"
    assert drift <= PARENT_DRIFT[case] + GRANULE, f"{case}: {drift} bytes gone after three creations, {PARENT_DRIFT[case]} before the owner"
