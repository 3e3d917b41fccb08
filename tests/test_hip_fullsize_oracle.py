"""GPU: the DEFAULT engine path against the CPU oracle at the sizes the speed figures come from -- every receiver sample and every
interior cell of both state grids, np.array_equal.

tests/test_hip_tb2.py and tests/test_hip_parity.py pin the kernels to the oracle on grids of up to 48 x 100 x 280 cells (one or two
column tiles, a handful of row tiles, every byte offset below 2^24); tests/test_hip_fullsize.py compares the kernel FAMILIES with
each other on large grids, which a defect in anything they share (sim_data's re-basing, init_walls' tables, the mask kernels, k_io,
the ABC tables, set_grid / get_grid) passes.  Here oracle.Engine (oracle/pf_oracle_impl.inc: OpenMP, itself pinned bit for bit to the
compiled reference by tests/test_oracle_pinned.py) steps the same scene from the same fields as a HipEngine created with its default
options, on grids with hundreds of tiles per plane, thousands of wall-region blocks and plane offsets beyond 2^31 and 2^32 bytes.

The comparison (tests/fullsize_oracle.py, run_case): two SimData of the scene (the oracle's with the node mask), scale_input() on
both; the oracle's two grids filled in place with seeded U(-1, 1) * 1e-3 -- every cell live from step 0: ghost layer, ABC shell, both
wall layers, box --; the engine is handed the same fields with set_grid() before the oracle's first step; K oracle steps, run(0, K)
on the device (or the listed run() pieces); then receivers, both grids' interiors (the outermost layer is the ghost shell, which the
fused kernels keep virtual: tests/test_hip_parity.py), and from timing() / layout() that the intended path ran.  A difference is
reported once, with the first differing (x, y, z), both values and the number of differing cells.

Column strips (cases B; pf_engine_walls.inc, wl_lo_option / wl_hi_option, worked through on the CPU for fp32 with walls at depth 2-3,
i.e. a box that starts at column 8, moved in fours when a sliver of at most 64 columns goes to the strips):
  * three steps in one pass (wall_three_steps == 9) needs the 20-cell form on BOTH sides, which only a moved box has (a box from column 8
    takes the 12-cell form on the low side) -- and a box is only moved after its sliver was cut off, so its column tiles are all full:
    Nz = 1013 .. 1024 (box 12 .. 1004 or 16 .. 1008, four tiles of 248).  B1 has Nz = 1016.
  * B2, Nz = 1003: box 8 .. 992, a last column tile of 240 columns, the low strip as 12-cell pencils, the high one as 20-cell pencils:
    two steps + one for the strips (wall_three_steps == 1).
  * the form cut in two (a 12-cell wall part and a node-free 16-cell part) cannot be reached in fp32 without the debug switch: on the
    low side it needs a strip of more than 18 and at most 18 columns at once, on the high side Nz <= t1 + 16 (the wall part fits) rules
    out Nz > t1 + 16 (the 20-cell pencil does not).  fp64 prefers it: case E's 768 x 768 x 1042 takes it on the high side.
  * B3, Nz = 1029: neither strip fits the pencils of a triple's box (20 .. 1012): the engine falls back to pairs.

Measured on the GPU box (one MI355X, 16 usable CPUs of the host; first run of this module, `--durations=0`):
  * host memory: MemTotal 3170 GB, MemAvailable 3009 - 3030 GB.  E2's 58 GB of oracle grids plus the 29 GB of one get_grid copy fit many
    times over: E2 compares whole get_grid copies like every other case (the x-block view of the device grids, device_view=True, is
    kept for hosts with less than ~100 GB free and is checked against get_grid at small size below).
  * the oracle's yardstick -- bench.py's cpu_baseline leg (the compiled reference, 512^3, Mb = 11 lossy walls, 16 threads) in the same visit:
    7-point fp32 6.32, 13-point fp32 4.41, 7-point fp64 4.58, 13-point fp64 3.41 Gvoxel-updates/s.  Every exact-arithmetic oracle leg below
    runs at 0.8 - 1.2 of its figure (none is twice as slow: the thread count is right).  The safeguarded oracle (fesetround around every
    sum) runs at 2.1 Gvox/s, a third of the exact one's speed: its own arithmetic, not the threads.
  * wall time per case in seconds -- scene with mask and in-place fill / engine creation (tables, autotune, placement search) / set_grid /
    oracle (its Gvox/s) / device run / comparison of receivers and both grids / whole test:
      A1  1024^3 fp32 K=21              1.7 / 2.5 / 0.4 /  4.2 (5.4) / <0.1 / 1.6 / 12.2    triples, wall_three_steps 9, 2016 alike blocks, 768 bricks
      A2  the same, K=20                1.7 / 2.3 / 0.4 /  3.3 (6.4) / <0.1 / 1.6 / 11.4    7 launches: six triples and a pair
      A3  the same, K=7+8+6             1.7 / 2.3 / 0.4 /  3.7 (6.0) / <0.1 / 1.6 / 11.5
      A4  the same, safeguarded         1.7 / 2.4 / 0.3 / 10.6 (2.1) / <0.1 / 1.6 / 18.3
      B1  1021 x 1003 x 1016 K=13       1.8 / 4.0 / 0.3 /  2.2 (6.1) / <0.1 / 1.7 / 11.8    triples, wall_three_steps 9, 2016 blocks, 760 bricks
      B2  1021 x 1003 x 1003 K=13       1.8 / 2.4 / 0.3 /  2.2 (6.1) / <0.1 / 1.7 / 10.3    triples, wall_three_steps 1, 2028 blocks, 756 bricks
      B3  1021 x 1003 x 1029 K=13       1.7 / 2.4 / 0.3 /  1.9 (7.3) / <0.1 / 1.5 / 10.0    pairs, single-step shell (no wall regions), 2 tiles step singly
      C   1024^3 folded FCC fp32 K=8    1.8 / 1.7 / 0.4 /  2.4 (3.6) / <0.1 / 1.8 / 11.0    blocked pairs (4 launches)
      D   CTK 894 x 579 x 309 K=9       0.4 / 1.3 / 0.1 /  0.3 (4.3) / <0.1 / 0.3 /  4.2    single steps (air_path 1), stored 309 x 579 x 894, pitch 896
      D   MV 2852 x 552 x 850 K=9       2.7 / 8.2 / 0.7 /  2.9 (4.2) / <0.1 / 2.8 / 30.3    blocked pairs, 4792 tiles step singly, stored 850 x 552 x 2852, pitch 2880
      E1  768 x 768 x 1042 fp64 K=13    1.7 / 2.4 / 0.6 /  2.4 (3.4) / <0.1 / 1.9 / 10.8    triples, regions two steps + one (wall_three_steps 0), 2490 blocks, 644 bricks
      E2  1536^3 folded FCC fp64 K=4    8.9 / 7.7 / 1.9 /  4.5 (3.2) /  0.1 / 9.9 / 41.9    blocked pairs (2 launches)
    (the whole test also holds the scene's set-up -- the rooms' voxelisation -- and the second SimData.)  The module takes about four minutes
    on the GPU box, a minute of which is the session fixture's build.
  * that the cases can fail: with the value of k_tb3's third stage scaled by 1 + 2^-22 in a scratch copy (clean tiles only, pf_tb3.h), A1
    reported "receivers: 154 of 336 samples differ; first at receiver node 0, step 3", "grid 0: 1033510040 of 1067462648 interior cells
    differ; first at (x, y, z) = (3, 3, 8): device -0.0008487123 (-0x1.bcf83cp-11), oracle -0.0008487121 (-0x1.bcf836p-11)" and the like for
    grid 1 (after 21 steps the error has spread from the box to every cell of the room; step 3 is the first sample a third stage feeds).
"""
import tempfile
from pathlib import Path

import numpy as np
import pytest

import fullsize_oracle as fo
from pffdtd_amd import engine, scenes, sim_data, synth

pytestmark = pytest.mark.gpu


def _maker(sim, prec):
    def make(mask):
        sd = sim_data.SimData.from_sim(sim, prec, build_mask=mask)
        sd.scale_input()
        return sd
    return make


# ---- A: the headline, exactly as bench.py builds it (bench.py: build_scene; default source and receivers) --------------------
def _headline(K):
    return _maker(synth.shoebox(1024, 1024, 1024, Nt=K, Nm=1, Mb=11, lossy=True), "single")


def _expect_headline(K):
    def check(tm, lay):
        assert tm["tb_steps_per_pass"] == 3 and tm["tb2_launches"] > 0, tm
        assert tm["wall_three_steps"] == 9, tm  # bit 0: the x / y regions, bit 3: the column strips -- both as k_wall2<..., NS = 3>
        assert tm["wall_bricks"] > 0 and tm["tb2_dirty_tiles"] == 0 and tm["steps"] == K, tm
        assert not lay[2]
    return check


def test_A1_headline_seven_triples():
    """1024^3 fp32, Mb = 11, lossy walls, PF_NUM_CPU_EXACT, K = 21: k_tb3 triples, the whole shell in one pass with the box kernel
    (k_wall2<..., NS = 3> for the x / y regions and the column strips, bricks for the frame), grids the engine owns and places."""
    fo.run_case(_headline(21), [(0, 21)], seed=101, expect=_expect_headline(21), name="A1")


def test_A2_headline_six_triples_and_a_pair():
    """the same with K = 20 -- the run length of the driver's headline line: six triples and a pair on the triples' tiles"""
    fo.run_case(_headline(20), [(0, 20)], seed=102, expect=_expect_headline(20), name="A2")


def test_A3_headline_split_into_three_runs():
    """the 21 steps of A1 as run(0, 7); run(7, 8); run(15, 6) on one engine: triples do not survive a run() boundary
    (Engine::run), so this walks the triple -> single, triple -> pair and back hand-overs at full size"""
    fo.run_case(_headline(21), [(0, 7), (7, 8), (15, 6)], seed=101, expect=_expect_headline(21), name="A3")


def test_A4_headline_in_the_gpu_safeguarded_arithmetic():
    """A1 with numerics = PF_NUM_GPU_SAFEGUARDED against oracle.Engine(..., safeguarded=True): the oracle's restatement of the
    reference's CUDA arithmetic is UNPINNED (no compiled reference produces these bits on a CPU) -- an independent C implementation all
    the same, not a sibling kernel."""
    fo.run_case(_headline(21), [(0, 21)], seed=104, numerics=engine.PF_NUM_GPU_SAFEGUARDED, expect=_expect_headline(21), name="A4")


# ---- B: shoeboxes that are awkward at scale ----------------------------------------------------------------------------------
def _awkward(Nz, K=13):
    """1021 planes (odd; the box's 1009 planes in 16 x chunks of 64), 1003 rows (the box's 991 rows: 49 tiles of 20 and one of 11), two
    materials of 11 and 3 branches.  The source cell (p .. p + 1 on every axis) straddles a corner of k_tb3's tiles on all three axes:
    x chunks from plane 6 in steps of 64, row tiles from row 6 in steps of 20, column tiles of 248 from the box's first column.
    Receivers (the eight corner nodes of a cell each; never on a boundary node, as the reference's set-up guarantees) follow
    triple_scene's pattern of tests/test_hip_tb2.py: beside the source; in the two layers of cells between the walls and the box -- the
    wall regions' cells -- of the near x face and of the far x, y and z faces; in an edge of the frame (outside the box on x and y, a
    brick's cells); in a far corner; in the last, partial row tile and in the last column tile."""
    n = (1021, 1003, Nz)
    z0 = {1016: 12, 1003: 8, 1029: 8}[Nz]  # the box's first column (B3's pairs: 8)
    src = [6 + 64 * 8 - 1, 6 + 20 * 25 - 1, z0 + 2 * 248 - 1]
    lo, hi = 4, [d - 6 for d in n]  # walls at depth 2 and 3, the triples' box from depth 6: the two layers of cells between them
    rcv = [[src[0] + 2, src[1] - 1, src[2] + 3], [lo, src[1] - 3, src[2] + 2], [hi[0], src[1] + 2, src[2] - 5], [src[0], hi[1], src[2] + 4],
           [src[0] - 2, src[1] + 1, hi[2]], [lo, lo, src[2] + 1], [hi[0], 700, hi[2]], [300, n[1] - 12, 400], [700, 300, n[2] - 40]]
    return _maker(synth.shoebox(*n, Nt=K, Nm=2, Mb=[11, 3], src=src, rcv=rcv, wall=3), "single")


def test_B1_awkward_box_strips_of_20_cell_pencils_on_both_sides():
    """1021 x 1003 x 1016: triples, both column strips as one region of 20-cell pencils each -> the whole shell takes three steps in one pass"""
    def check(tm, lay):
        assert tm["tb_steps_per_pass"] == 3 and tm["tb2_launches"] > 0 and tm["steps"] == 13, tm
        assert tm["wall_three_steps"] == 9 and sum(tm["wall_blocks"]) > 0 and tm["wall_bricks"] > 0, tm
    fo.run_case(_awkward(1016), [(0, 13)], seed=201, expect=check, name="B1")


def test_B2_awkward_box_strips_of_12_and_20_cell_pencils():
    """1021 x 1003 x 1003: triples with a partial last column tile (240 of 248 columns); low strip 12-cell pencils, high strip 20-cell pencils
    -> the x / y regions take three steps in one pass, the column strips two steps + one"""
    def check(tm, lay):
        assert tm["tb_steps_per_pass"] == 3 and tm["tb2_launches"] > 0 and tm["steps"] == 13, tm
        assert tm["wall_three_steps"] == 1 and sum(tm["wall_blocks"]) > 0 and tm["wall_bricks"] > 0, tm
    fo.run_case(_awkward(1003), [(0, 13)], seed=202, expect=check, name="B2")


def test_B3_strips_too_wide_fall_back_to_pairs():
    """1021 x 1003 x 1029: a triple's box would leave strips of 20 and 17 columns beside a pitch of 1056, which no form of pencils fits: pairs
    (oracle-checked so far at 47 x 101 x 283 only)"""
    def check(tm, lay):
        assert tm["tb_steps_per_pass"] == 2 and tm["tb2_launches"] > 0 and tm["steps"] == 13, tm
    fo.run_case(_awkward(1029), [(0, 13)], seed=203, expect=check, name="B3")


# ---- C: 13-point folded FCC, 1024^3 stored -----------------------------------------------------------------------------------
def test_C_folded_fcc_1024_cubed():
    """bench.py --fcc: synth.shoebox(1024, 2046, 1024, fcc=True) folded and sorted, fp32, K = 8.  The default measures a blocked pair with its
    shell against a single step when the engine is created (Engine::autotune_fcc) and keeps the pairs at this size (k_tb2_fcc_w):
    asserted, so a default that changes its mind is noticed here."""
    sim = synth.shoebox(1024, 2046, 1024, Nt=8, fcc=True, Nm=1, Mb=11, lossy=True)
    synth.fold_fcc(sim)
    synth.sort_sim(sim)

    def check(tm, lay):
        assert tm["tb2_launches"] > 0 and tm["tb2_cells"] > 0 and tm["steps"] == 8, tm
    fo.run_case(_maker(sim, "single"), [(0, 8)], seed=301, expect=check, name="C")


# ---- D: the reference's rooms at full size -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,grid", [("ctk_cart_gpu", (894, 579, 309)), ("mv_fcc_gpu", (2852, 552, 850))])
def test_D_reference_rooms_at_full_size(name, grid):
    """CTK 894 x 579 x 309 (7-point) and Musikverein 2852 x 552 x 850 folded (13-point) from the scene exports in pffdtd_amd/data/models, set up
    as tools/config_family_check.py does, K = 9.  The engine stores these with the file's x and z axes exchanged (asserted): the exchanged-axes
    kernels and the transposing set_grid / get_grid are what is checked, and the boundary pass is a gather over real geometry
    (k_boundary<float, true>), which no shoebox has."""
    from pffdtd_amd.sim_setup import sim_setup
    with tempfile.TemporaryDirectory() as d:
        mats = scenes.write_materials(Path(d) / "materials")
        folder = Path(d) / name
        sim_setup(**scenes.setup_kwargs(name, folder, mats, save_folder_gpu=folder, compress=0))

        def make(mask):
            sd = sim_data.SimData.from_folder(folder, "single", build_mask=mask)
            sd.scale_input()
            return sd

        def check(tm, lay):
            assert lay[2] and lay[0] == grid[::-1], lay  # x and z exchanged
            assert tm["steps"] == 9, tm
            # (what the default picks for these rooms is measured when the engine is created; on the GPU box: CTK single steps, Musikverein blocked
            # pairs around its geometry -- the case checks whichever it is)
        fo.run_case(make, [(0, 9)], seed=401, expect=check, name=name)


# ---- E: fp64 -------------------------------------------------------------------------------------------------------------------
def _fp64_box(K=13):
    n = (768, 768, 1042)  # fp64 triples: 120 core columns per tile -- box 8 .. 1032 in eight tiles of 120 and one of 64; the high strip cut in two
    src = [n[0] // 2, n[1] // 2, n[2] // 2]
    rcv = [[src[0] + 2, src[1] - 1, src[2] + 3], [4, src[1] - 3, src[2] + 2], [src[0], n[1] - 6, src[2] + 4], [src[0] - 2, src[1] + 1, n[2] - 6], [4, 4, src[2] + 1]]
    return _maker(synth.shoebox(*n, Nt=K, Nm=2, Mb=[11, 3], src=src, rcv=rcv, wall=3), "double")


def test_E1_fp64_box_default_path():
    """768 x 768 x 1042 fp64, 7-point, K = 13, default options.  What the default picks for fp64 at this size is decided by a measurement when
    the engine is created (Engine::autotune); on the GPU box it is triples (k_tb3 with 120 core columns per tile, nine column tiles, the last of 64
    columns; the wall regions two steps + one, the high column strip cut in two): asserted -- so the fp64 triples are oracle-checked at scale
    by the default path itself and no forced run is needed."""
    def check(tm, lay):
        assert tm["steps"] == 13, tm
        assert tm["tb_steps_per_pass"] == 3 and tm["tb2_launches"] > 0, tm
        assert tm["wall_three_steps"] == 0 and sum(tm["wall_blocks"]) > 0 and tm["wall_bricks"] > 0 and tm["tb2_dirty_tiles"] == 0, tm
    fo.run_case(_fp64_box(), [(0, 13)], seed=501, expect=check, name="E1")



def test_E2_fp64_folded_fcc_1536_cubed():
    """BASELINE configs[4]: folded FCC fp64, stored grid 1536^3, K = 4 -- plane offsets pass 2^31 bytes at plane 114 and 2^32 at plane 228.
    The oracle's grids are 58 GB and one get_grid copy 29 GB: with that much host memory free (the GPU box has 3 TB) whole copies are compared
    like everywhere else; with less, x blocks of the engine's device grids (fullsize_oracle.device_blocks); with less than the oracle needs,
    the case is skipped with the measured figure.  The default runs blocked pairs here (asserted)."""
    need = 2 * 1536 ** 3 * 8 / 1e9
    avail = fo.mem_available_gb()
    if avail is not None and avail < need + 12:
        pytest.skip(f"the oracle's two grids need {need:.0f} GB of host memory plus ~12 GB of tables; MemAvailable is {avail:.0f} GB")
    n = 1536
    sim = synth.shoebox(n, 2 * (n - 1), n, Nt=4, fcc=True, Nm=1, Mb=11, lossy=True)
    synth.fold_fcc(sim)
    synth.sort_sim(sim)
    view = avail is not None and avail < need + 12 + n ** 3 * 8 / 1e9  # no room for a get_grid copy beside the oracle: x blocks of the device grids

    def check(tm, lay):
        assert tm["steps"] == 4 and lay[0] == (n, n, n) and not lay[2], (tm, lay)
        assert tm["tb2_launches"] > 0, tm
    fo.run_case(_maker(sim, "double"), [(0, 4)], seed=502, device_view=view, expect=check, name="E2")


# ---- the helper's two ways of reading the device grids agree (small, so that the x-block view is exercised wherever E2 does not need it) ----
@pytest.mark.parametrize("layout", [engine.PF_LAYOUT_FILE, engine.PF_LAYOUT_EXCHANGED], ids=["file_order", "exchanged"])
@pytest.mark.parametrize("prec", ["single", "double"])
def test_device_view_reads_what_get_grid_reads(prec, layout):
    n = (48, 100, 280)
    sim = synth.shoebox(*n, Nt=6, Nm=2, Mb=[11, 3], wall=3)
    sd = _maker(sim, prec)(False)
    eng = engine.HipEngine(sd, layout=layout)
    assert eng.layout()[2] == (layout == engine.PF_LAYOUT_EXCHANGED)
    rng = np.random.default_rng(5)
    for k in (0, 1):
        eng.set_grid(k, ((rng.random(n) * 2 - 1) * 1e-3).astype(sd.real))
    eng.run(0, 6)
    for k in (0, 1):
        g = eng.get_grid(k)
        assert np.abs(g).max() > 0
        fo.compare_interior(fo.device_blocks(eng, k), g, f"grid {k}")
        bad = g.copy()
        bad[20, 30, 40] += 1
        with pytest.raises(fo.Mismatch, match=r"1 of .* first at \(x, y, z\) = \(20, 30, 40\)"):
            fo.compare_interior(fo.device_blocks(eng, k), bad, f"grid {k}")
    eng.close()
