"""GPU: sources and receivers anywhere in the grid (tests/io_lists.py) against the CPU oracle, bit for bit.

The host rules that read the two lists -- TB3_MAXSRC and src_tiles / inside (init_tb2_impl), the receivers' rim flags, "a source within a
cell / two cells of the shell" (init_walls), cut_shell's refusal, fused_ok's ghost-cell receivers, the slab cut's CUT_CLEAR, sorted_perm's
stable order, k_io's cdiv(Nr + 1, 128) blocks -- each get lists that take them down every branch.  Every case starts from seeded random
u^{n-1}, u^n of 1e-2 (a single engine: set_grid; a chain: load_state with zero node state), compares ALL receiver rows and the interior of
both final fields with oracle.Engine by np.array_equal, asserts which path ran from pf_timing and prints the timing dict."""
import functools

import numpy as np
import pytest

import cases
import io_lists as io
from pffdtd_amd import engine, sim_data, synth

pytestmark = pytest.mark.gpu
SG = engine.PF_NUM_GPU_SAFEGUARDED


def _interior(a):
    return a[1:-1, 1:-1, 1:-1]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _sd(sim, prec, mask=False):
    sd = sim_data.SimData.from_sim(sim, prec, build_mask=mask)
    sd.scale_input()
    return sd


def _run(sim, prec, init, pieces, label, **kw):
    """one HipEngine from `init` over `pieces` of run() -> (u_out, u^{n-1}, u^n, timing, layout exchanged?)"""
    sd = _sd(sim, prec)
    eng = engine.HipEngine(sd, **kw)
    try:
        for k in (0, 1):
            eng.set_grid(k, init[k])
        for n0, ns in pieces:
            eng.run(n0, ns)
        tm, ex = eng.timing(), eng.layout()[2]
        g = [eng.get_grid(0), eng.get_grid(1)]
    finally:
        eng.close()
    print(f"{label} {prec} {pieces}: {tm}")
    return sd.u_out.copy(), g[0], g[1], tm, ex


def _same(got, ref, label):
    assert np.array_equal(got[0], ref[0]), f"{label}: u_out differs in {np.count_nonzero((got[0] != ref[0]).any(axis=1))} of {ref[0].shape[0]} rows, max|d| = {np.abs(got[0] - ref[0]).max()}"
    for k in (1, 2):
        assert np.array_equal(_interior(got[k]), _interior(ref[k])), f"{label}: field {k - 1} differs in {np.count_nonzero(_interior(got[k]) != _interior(ref[k]))} cells"


# ---- T. three steps per pass -----------------------------------------------------------------------------------------------------------
T_PIECES = ([(0, io.T_NT)], [(0, 7), (7, 13), (20, 2)])


def _t_sim(prec, key):
    rb = 4 if prec == "single" else 8
    sim = io.t_scene(prec, **(dict(rigid_every=9) if key == "walls" else {}))
    n = io._dims(sim)
    src = {"src33": io.SRC33(n), "shell2": io.SRC_SHELL2(n, rb), "shell1": io.SRC_SHELL1(n, rb)}.get(key) or (io.SRC_WALLS(sim, rb) if key == "walls" else io.SRC24(n))
    rcv = {"rcv256": io.RCV256, "rcv321": io.RCV321, "ghost": io.RCV_GHOST}.get(key)
    return io.scatter(sim, src, rcv(sim) if rcv else None)  # (no receiver list named: the scene's own few receiver cells)


@functools.lru_cache(maxsize=None)
def _t_ref(prec, key, safeguarded=False):
    """the oracle from the random fields, once per scene: (u_out, u^{n-1}, u^n), read-only"""
    sim = _t_sim(prec, key)
    ref = io.oracle_run(_sd(sim, prec, mask=True), io.random_fields(io._dims(sim), prec), safeguarded)
    assert np.isfinite(ref[0]).all() and io.live_rows(ref[0]).all()
    return _frozen(*ref)


def _t_case(prec, key, path, numerics=0, **kw):
    sim = _t_sim(prec, key)
    init = io.random_fields(io._dims(sim), prec)
    ref = _t_ref(prec, key, numerics == SG)
    kw.setdefault("air_variant", 40)
    for pieces in T_PIECES:
        got = _run(sim, prec, init, pieces, f"T/{key}", timing=True, numerics=numerics, **kw)
        tm = got[3]
        assert tm["steps"] == io.T_NT and path(tm), (key, pieces, tm)
        _same(got, ref, f"T/{key} {prec} {pieces} {kw}")


def _triples_clean_bricks(tm):
    return tm["tb_steps_per_pass"] == 3 and tm["tb2_launches"] > 0 and tm["tb2_dirty_tiles"] == 0 and tm["wall_bricks"] > 0


@pytest.mark.parametrize("prec", ["single", "double"])
@pytest.mark.parametrize("mode", ["default", "tiles_single", "pairs", "safeguarded"])
def test_24_sources_over_tile_borders_inside_k_tb3(mode, prec):
    """SRC24, the scene's own receivers: 24 <= TB3_MAXSRC nodes, all inside the box and two cells off the shell, so k_tb3<..., SRC> adds them in
    registers in every tile within two cells of one (no tile steps singly) and the bricks stand.  debug 0x40: their tiles step singly, k_io adds
    them; 0x20000: pairs; and the GPU-safeguarded arithmetic."""
    if mode == "default":
        _t_case(prec, "src24", _triples_clean_bricks)
    elif mode == "tiles_single":
        _t_case(prec, "src24", lambda tm: tm["tb_steps_per_pass"] == 3 and tm["tb2_dirty_tiles"] > 0 and tm["wall_bricks"] > 0, debug=0x40)
    elif mode == "pairs":
        _t_case(prec, "src24", lambda tm: tm["tb_steps_per_pass"] == 2 and tm["tb2_launches"] > 0 and tm["tb2_dirty_tiles"] > 0, debug=0x20000)
    else:
        _t_case(prec, "src24", _triples_clean_bricks, numerics=SG)


@pytest.mark.parametrize("prec", ["single", "double"])
def test_33_sources_are_left_to_k_io(prec):
    """SRC33: one more than TB3_MAXSRC, so src_tiles is off: the tiles within two cells of a source step singly and k_io adds all 33"""
    _t_case(prec, "src33", lambda tm: tm["tb_steps_per_pass"] == 3 and tm["tb2_dirty_tiles"] > 0)


@pytest.mark.parametrize("prec", ["single", "double"])
@pytest.mark.parametrize("key", ["shell2", "shell1"])
def test_a_source_two_cells_and_one_cell_inside_the_boxs_z_edge(key, prec):
    """init_walls: a source two cells inside the box (z = z1 - 3) leaves the frame's bricks; one cell inside (z1 - 2) the bricks go and the wall
    regions stay (generic blocks for the frame)"""
    if key == "shell2":
        _t_case(prec, key, lambda tm: tm["tb_steps_per_pass"] == 3 and tm["wall_bricks"] > 0)
    else:
        _t_case(prec, key, lambda tm: tm["tb_steps_per_pass"] == 3 and tm["wall_bricks"] == 0 and sum(tm["wall_blocks"]) > 0)


@pytest.mark.parametrize("prec", ["single", "double"])
def test_sources_in_the_walls_the_abc_shell_and_outside_the_room(prec):
    """SRC_WALLS (rigid_every = 9): every source outside the triples' box -- init_walls refuses the wall regions ("a source within a cell of the
    shell"), init_tb2 then drops the triples and builds the pairs' geometry, whose k_io adds the samples between the steps wherever they lie.
    The pairs' box starts a cell nearer the walls and the sources still lie outside it, so its wall regions are refused too: pairs with a
    single-step shell."""
    _t_case(prec, "walls", lambda tm: tm["tb_steps_per_pass"] == 2 and tm["tb2_launches"] > 0 and sum(tm["wall_blocks"]) == 0 and tm["wall_bricks"] == 0)


@pytest.mark.parametrize("prec", ["single", "double"])
@pytest.mark.parametrize("key,chunk", [("rcv256", 0), ("rcv321", 7)])
def test_receivers_in_three_blocks_of_k_io_on_shell_and_boundary_nodes(key, chunk, prec):
    """Nr = 256: k_io's thread Nr, which alone adds the sources, is the first thread of a third block; Nr = 321 with a readout ring of seven
    steps.  Receivers on ABC-shell cells and boundary nodes lie outside the box (no rim flag needed: the shell's kernels store u^{n+1});
    those in the box flag their tiles to store it."""
    _t_case(prec, key, _triples_clean_bricks, readout_chunk=chunk)


@pytest.mark.parametrize("prec", ["single", "double"])
def test_a_receiver_in_a_ghost_cell_takes_the_fused_kernels_away(prec):
    """RCV_GHOST.  Engine::fused_ok: a receiver that reads a ghost cell fails the fused path's preconditions (the fused kernels keep the ghost
    shell virtual: its copy in memory is not maintained).  Engine::init then REFUSES air_variant 40 -- a forced path that cannot run is an
    error -- and air_variant 0 takes the unfused kernel sequence with the flips in memory: no blocked launches, air_path -1, the oracle's bits
    on every row, the ghost cells' included."""
    sim = _t_sim(prec, "ghost")
    with pytest.raises(engine.PfError, match="fused-path preconditions do not hold"):
        engine.HipEngine(_sd(sim, prec), air_variant=40).close()
    _t_case(prec, "ghost", lambda tm: tm["tb2_launches"] == 0 and tm["tb_steps_per_pass"] == 0 and tm["air_path"] == -1, air_variant=0)


# ---- S. single steps ---------------------------------------------------------------------------------------------------------------------
S_NT = 26
S_SCENES = {"cart_outside_oddz": "single", "cart_mb11": "double", "fcc1_outside": "single"}


def _s_sim(name):
    fcc = cases.CASES[name][1] > 0
    sim = cases.make_sim(name, Nt=S_NT, sig="dhann30")
    return io.scatter(sim, io.air_nodes(sim, 40, 5, seed=11, fcc=fcc), io.RCV321(sim, fcc=fcc), seed=2)


def _s_init(name):
    sim = _s_sim(name)
    n = io._dims(sim)
    init = io.random_fields(n, S_SCENES[name], seed=67)
    if cases.CASES[name][1] > 0:  # the fields live on the even-parity subgrid
        odd = (np.add.outer(np.add.outer(np.arange(n[0]), np.arange(n[1])), np.arange(n[2])) % 2) == 1
        for a in init:
            a[odd] = 0
    return sim, init


@functools.lru_cache(maxsize=None)
def _s_ref(name):
    sim, init = _s_init(name)
    ref = io.oracle_run(_sd(sim, S_SCENES[name], mask=True), init)
    assert np.isfinite(ref[0]).all() and io.live_rows(ref[0]).all()
    return _frozen(*ref)


S_MODES = {  # engine options, the path they must take (air_path: 0 lean fused kernel, 1 barrier-free kernel with virtual ghosts, -1 the unfused sequence)
    "v3": (dict(air_variant=3, timing=True), lambda tm, ex: tm["air_path"] == -1 and not ex),
    "v4": (dict(air_variant=4, timing=True), lambda tm, ex: tm["air_path"] == 1 and not ex),
    "v25": (dict(air_variant=25, timing=True), lambda tm, ex: tm["air_path"] == 0 and not ex),
    "exchanged": (dict(layout=engine.PF_LAYOUT_EXCHANGED, timing=True), lambda tm, ex: ex),  # (sorted_perm then sorts both lists by the STORAGE index)
    "graph": (dict(debug=0x800000), lambda tm, ex: not ex),  # (PF_DBG_GRAPH: six steps per hipGraph; it needs timing off)
}


@pytest.mark.parametrize("name", list(S_SCENES))
@pytest.mark.parametrize("mode", list(S_MODES))
def test_single_steps_with_shuffled_lists_and_duplicates(mode, name):
    """40 seeded air nodes, shuffled, five of them repeats, and RCV321 of that grid, on every single-step kernel family, with the grid stored
    with exchanged axes (both lists are then sorted by another key: only a STABLE sort keeps two entries of one node in list order, and the
    oracle's loop adds them in list order) and replayed from a hipGraph."""
    if mode == "v25" and cases.CASES[name][1] > 0:
        with pytest.raises(engine.PfError, match="7-point Cartesian only"):  # (variant 25's own precondition; 3 and 4 hold on all three scenes)
            engine.HipEngine(_sd(_s_sim(name), S_SCENES[name]), air_variant=25).close()
        return
    prec = S_SCENES[name]
    sim, init = _s_init(name)
    kw, path = S_MODES[mode]
    got = _run(sim, prec, init, [(0, 3), (3, 17), (20, S_NT - 20)], f"S/{name}/{mode}", readout_chunk=16, **kw)
    assert got[3]["tb2_launches"] == 0 and got[3]["tb_steps_per_pass"] == 0 and path(got[3], got[4]), (got[3], got[4])
    _same(got, _s_ref(name), f"S/{name}/{mode}")


# ---- F. 13-point pairs and shell bricks ----------------------------------------------------------------------------------------------------
F_N, F_NT = (36, 70, 280), 14  # the stored (folded) grid of tests/test_hip_fcc_bricks.py: fcc_scene; unfolded Ny = 138


def _f_sim(near_shell):
    """The pairs' box of this scene starts at x = 5 (wall layers at depth 2 and 3, two cells of reach: init_tb2_impl) and ends before x = 31, and
    cut_shell wants every source in [box0 + 2, box1 - 2) on every axis: x = 7 is the first plane it accepts, x = 6 is one cell from the shell.
    y and z stay far inside (folded rows 17 .. 57, columns 20 .. 250)."""
    Nyu = 2 * (F_N[1] - 1)
    sim = synth.shoebox(F_N[0], Nyu, F_N[2], Nt=F_NT, fcc=True, Nm=2, Mb=[11, 3], wall=3, sig="dhann30")
    n = io._dims(sim)
    src = [(7, 17, 20), (28, 57, 249), (18, 35, 141), (12, 100, 60), (25, 120, 201), (9, 80, 133), (18, 35, 141), (20, 40, 100), (27, 19, 30),
           (8, 118, 248), (12, 100, 60), (16, 52, 222)]  # ten nodes, two of them twice; unfolded rows 80 .. 120 fold onto 57 .. 17
    if near_shell:
        src[5] = (6, 81, 133)
    rng = np.random.default_rng(19)
    rcv = []
    while len(rcv) < 120:
        p = [int(rng.integers(1, n[a] - 1)) for a in range(3)]
        rcv.append(io._even(p, n, [2]))
    bn = [tuple(int(q) for q in p) for p in zip(*synth._ind2sub(np.asarray(sim["vox_out"]["bn_ixyz"]), n[1], n[2]))]
    rcv += [bn[0], bn[len(bn) // 3], bn[len(bn) // 2], bn[-1]] + io.boundary_nodes(sim, True)[5:7]  # six boundary nodes
    rcv += [(10, 68, 100), (11, 69, 100), (30, 68, 12), (21, 69, 200)]  # the two unfolded rows that fold onto the last stored row, Ny - 2
    assert len(rcv) == 130
    io.scatter(sim, src, [rcv[int(k)] for k in rng.permutation(130)], seed=4)
    synth.fold_fcc(sim)
    synth.sort_sim(sim)
    return sim


@functools.lru_cache(maxsize=None)
def _f_ref(prec, near_shell):
    ref = io.oracle_run(_sd(_f_sim(near_shell), prec, mask=True), io.random_fields(F_N, prec, seed=71))
    assert np.isfinite(ref[0]).all() and io.live_rows(ref[0]).all()
    return _frozen(*ref)


@pytest.mark.parametrize("prec", ["single", "double"])
@pytest.mark.parametrize("variant", [40, 42])
@pytest.mark.parametrize("near_shell", [False, True], ids=["two_cells_off_the_shell", "one_cell_off_the_shell"])
def test_13_point_pairs_with_twelve_sources_and_130_receivers(near_shell, variant, prec):
    """Twelve even-parity sources (two repeats) at least two cells from the shell: air_variant 42 steps the shell in bricks.  One of them one
    cell from the shell: cut_shell refuses ("within 2 cells of the shell") and air_variant 42, which is that path forced, is an error; the
    same list under 40 steps the shell singly -- fcc_shell_bricks == 0.  130 even-parity receivers, boundary nodes and fold-row nodes among
    them."""
    sim = _f_sim(near_shell)
    if near_shell and variant == 42:
        with pytest.raises(engine.PfError, match="lies within 2 cells of the shell"):
            engine.HipEngine(_sd(sim, prec), air_variant=42).close()
        return
    got = _run(sim, prec, io.random_fields(F_N, prec, seed=71), [(0, 9), (9, F_NT - 9)], f"F/{variant}/{near_shell}", air_variant=variant, timing=True)
    tm = got[3]
    assert tm["tb2_launches"] > 0 and tm["tb_steps_per_pass"] == 2 and (tm["fcc_shell_bricks"] > 0) == (variant == 42), tm
    _same(got, _f_ref(prec, near_shell), f"F/{variant} {prec}")


# ---- C. chains -------------------------------------------------------------------------------------------------------------------------
C_NT = 21


def _c_sim(band, along_z):
    """_RING_SCENE of tests/test_hip_multi.py with sources spread along the cut axis -- a node on every 6th x plane from 7 to 115 (19 nodes: no
    plane is CUT_CLEAR = 8 planes from all of them, every slab gets some), or on every plane 30 .. 95 (66 nodes: more than TB3_MAXSRC in the
    middle slab, nodes on both sides of every cut); along z the same counts over 276 columns (every 14th plane from 7; planes 80 .. 145, over
    the even split's first cut at 92) --, three nodes twice, shuffled, and RCV321: rows on both sides of every cut.  The band keeps to rows
    30 .. 40, one row tile of a slab's box: spread over all rows, its 40-odd nodes in the middle slab leave that slab no tile to step in
    pairs, and a chain that was ASKED for pairs (PF_MULTI_FORCE_PAIRS, air_variant 40) then refuses the scene ("no boundary-free tiles")."""
    from test_hip_multi import _RING_SCENE
    sim = synth.shoebox(**dict(_RING_SCENE, Nt=C_NT, sig="dhann30"))
    n = io._dims(sim)
    rng = np.random.default_rng(31 + 2 * band + along_z)
    if along_z:
        planes = list(range(80, 146)) if band else list(range(7, 7 + 14 * 19, 14))
        src = [(int(rng.integers(10, n[0] - 10)), int(rng.integers(30, 41) if band else rng.integers(10, n[1] - 10)), p) for p in planes]
    else:
        planes = list(range(30, 96)) if band else list(range(7, 116, 6))
        src = [(p, int(rng.integers(30, 41) if band else rng.integers(10, n[1] - 10)), int(rng.integers(20, n[2] - 25))) for p in planes]
    assert len(src) == (66 if band else 19)
    src += [src[int(k)] for k in rng.choice(len(src), size=3, replace=False)]
    return io.scatter(sim, [src[int(k)] for k in rng.permutation(len(src))], io.RCV321(sim), seed=6)


@functools.lru_cache(maxsize=None)
def _c_ref(band, along_z):
    sim = _c_sim(band, along_z)
    ref = io.oracle_run(_sd(sim, "single", mask=True), io.random_fields(io._dims(sim), "single", seed=73))
    assert np.isfinite(ref[0]).all() and io.live_rows(ref[0]).all()
    return _frozen(*ref)


FORCE = engine.PF_MULTI_FORCE_PAIRS
C_CHAINS = {"two": ([0, 0], FORCE), "three": ([0, 0, 0], FORCE), "three_no_triples": ([0, 0, 0], FORCE | engine.PF_MULTI_NO_TRIPLES),
            "three_cut_z": ([0, 0, 0], engine.PF_MULTI_CUT_Z)}  # (a chain cut along file z takes single steps only: pf_multi_create refuses it pairs)


@pytest.mark.parametrize("band", [False, True], ids=["every_6th_plane", "band_of_66_planes"])
@pytest.mark.parametrize("chain", list(C_CHAINS))
def test_chains_with_sources_at_every_cut(chain, band):
    """pf_slab_cut.h: no cut can keep CUT_CLEAR planes from these sources, so the cuts stay where the cost puts them, with sources in the edge
    planes and beside them; every slab's engine then applies the single domain's rules to its share (more than TB3_MAXSRC in the middle slab
    of the band: k_io adds them, their tiles step singly).  Slabs asked for pairs step three times per pass, with PF_MULTI_NO_TRIPLES twice;
    a chain cut along file z stores its slabs with exchanged axes, which have no blocked steps.  Every exchange is checked; receivers and
    both fields equal the single-domain oracle's.
    The band on three slabs is cut with PF_MULTI_EVEN_SPLIT: the cost-balanced split does find planes clear of a band (22 and 104 of 124: measured
    at creation) and moves both cuts there, which leaves no node beside a cut -- and end slabs of 22 and 20 planes, too thin for a box,
    which a chain forced to pairs refuses.  The even split cuts at 42 and 83, inside the band."""
    devs, flags = C_CHAINS[chain]
    if band and len(devs) == 3:
        flags |= engine.PF_MULTI_EVEN_SPLIT
    along_z = bool(flags & engine.PF_MULTI_CUT_Z)
    sim = _c_sim(band, along_z)
    ref = _c_ref(band, along_z)
    sd = _sd(sim, "single")
    init = io.random_fields(io._dims(sim), "single", seed=73)
    z = np.zeros
    start = {"u_prev": init[0], "u_cur": init[1], "u1b": z(sd.Nbl, np.float32), "u2b": z(sd.Nbl, np.float32), "vh1": z((sd.Nbl, 12), np.float32), "gh1": z((sd.Nbl, 12), np.float32)}
    m = engine.HipMulti(sd, devs, multi_flags=flags, air_variant=0 if along_z else 40, verify_exchange=C_NT, timing=1)
    try:
        m.load_state(start)
        m.run(0, 20)
        m.run(20, 1)
        info = m.info()
        slabs = [m.slab(g) for g in range(len(devs))]
        tms = [s["engine"].timing() for s in slabs]
        after = m.save_state()
    finally:
        m.close()
    for s, tm in zip(slabs, tms):
        print(f"C/{chain}/{'band' if band else '6th'} planes [{s['x0']}, {s['x1']}) steps per pass {s['steps_per_pass']}: {tm}")
    assert info["exchange_verified"] is True and info["exchanges_checked"] == C_NT and info["cut_along_z"] == along_z, info
    spp = [tm["tb_steps_per_pass"] for tm in tms]
    assert spp == [0 if along_z else (2 if flags & engine.PF_MULTI_NO_TRIPLES else 3)] * len(devs), spp
    assert all((tm["tb2_launches"] > 0) != along_z for tm in tms), [tm["tb2_launches"] for tm in tms]
    if band and not along_z:  # the middle slab holds more than TB3_MAXSRC nodes: k_io adds them, their tiles step singly
        assert tms[len(devs) // 2]["tb2_dirty_tiles"] > 0, tms[len(devs) // 2]
    _same((sd.u_out, after["u_prev"], after["u_cur"]), ref, f"C/{chain}/{band}")
