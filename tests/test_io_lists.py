"""CPU: the scene editor of tests/io_lists.py keeps its contract, the scenes built with it CAN fail (on the oracle alone: the order of two
duplicates and every single source change u_out, no receiver row is dead), and the slab chain's Python path (pffdtd_amd/slab.py) carries
lists that leave no cut clear of sources.  The GPU cases are tests/test_hip_io_lists.py."""
import functools

import numpy as np
import pytest

import cases
import io_lists as io
import oracle  # noqa: F401
from pffdtd_amd import sim_data, synth
from slab_harness import run_in_process


# ---- 1. the editor's contract ------------------------------------------------------------------------------------------------------------
def _small(fcc=False):
    return synth.shoebox(24, 22, 20, Nt=40, fcc=fcc, Nm=2, Mb=[2, 3], sig="dhann30")


def test_scatter_keeps_order_duplicates_and_gives_every_row_a_signal():
    sim = _small()
    peak = np.abs(sim["comms_out"]["in_sigs"][0]).max()
    base = sim["comms_out"]["in_sigs"][0] / peak
    src = [(5, 6, 7), (12, 3, 9), (5, 6, 7), (4, 4, 4), (20, 19, 17), (12, 3, 9), (5, 6, 7), (9, 9, 9), (10, 9, 9)]
    rcv = [(0, 0, 0), (23, 21, 19), (7, 7, 7), (7, 7, 7), (1, 2, 3)]
    assert io.scatter(sim, src, rcv, seed=3) is sim
    c = sim["comms_out"]
    assert c["in_ixyz"].tolist() == [(x * 22 + y) * 20 + z for x, y, z in src] and int(c["Ns"]) == 9  # the order given, unsorted, duplicates kept
    assert c["in_sigs"].shape == (9, 40)
    fac = np.random.default_rng(3).uniform(0.2, 1.0, size=9)
    for k in range(9):
        assert np.array_equal(c["in_sigs"][k], np.roll(base, k % 7) * fac[k] * (-1.0) ** k), k
    assert (np.abs(c["in_sigs"]).max(axis=1) >= 0.2 - 1e-12).all() and (np.abs(c["in_sigs"]).max(axis=1) <= 1.0).all()
    assert len({c["in_sigs"][k].tobytes() for k in range(9)}) == 9  # a duplicate node's rows differ too
    assert c["out_ixyz"].tolist() == [(x * 22 + y) * 20 + z for x, y, z in rcv] and int(c["Nr"]) == 5
    assert c["out_reorder"].tolist() == [0, 1, 2, 3, 4] and c["out_alpha"].shape[0] == 5 and (c["out_alpha"] == 1).all()
    sd = sim_data.SimData.from_sim(sim, "single")  # the loader takes the edited scene as it is
    assert sd.Ns == 9 and sd.Nr == 5 and sd.in_sigs.shape == (9, 40) and sd.u_out.shape == (5, 40)


def test_scatter_edits_one_list_and_leaves_the_other():
    sim = _small()
    before = {k: np.array(v) for k, v in sim["comms_out"].items()}
    io.scatter(sim, rcv_nodes=[(3, 3, 3)])
    for k in ("in_ixyz", "in_sigs", "Ns", "Nt", "diff"):
        assert np.array_equal(sim["comms_out"][k], before[k]), k
    io.scatter(sim, src_nodes=[(3, 3, 3)])
    assert sim["comms_out"]["out_ixyz"].tolist() == [(3 * 22 + 3) * 20 + 3]


def test_scatter_refuses_odd_parity_nodes_folded_scenes_and_nodes_outside_the_grid():
    sim = _small(fcc=True)
    with pytest.raises(ValueError, match="odd-parity"):
        io.scatter(sim, src_nodes=[(4, 4, 4), (4, 4, 5)])
    with pytest.raises(ValueError, match="odd-parity"):
        io.scatter(sim, rcv_nodes=[(1, 1, 1)])
    io.scatter(sim, src_nodes=[(4, 4, 4), (5, 4, 5)], rcv_nodes=[(1, 1, 2)])
    with pytest.raises(ValueError, match="outside the grid"):
        io.scatter(sim, rcv_nodes=[(24, 1, 1)])
    synth.fold_fcc(sim)
    with pytest.raises(ValueError, match="before synth.fold_fcc"):
        io.scatter(sim, src_nodes=[(4, 4, 4)])


@pytest.mark.parametrize("prec", ["single", "double"])
def test_named_lists_have_their_sizes_clamp_z_and_stay_off_the_boundary(prec):
    rb = 4 if prec == "single" else 8
    sim = io.t_scene(prec, rigid_every=9)
    n = io._dims(sim)
    box = io.triple_box(n, rb)
    assert box == ((6, 42), (6, 94), (16, 264 if rb == 4 else 256))
    bn = set(np.asarray(sim["vox_out"]["bn_ixyz"]).tolist())
    s24, s33 = io.SRC24(n), io.SRC33(n)
    assert len(s24) == 24 and len(s33) == 33 and s33[:24] == s24 and len(set(s33)) == 33 - 3
    assert s24.count(s24[0]) == 3 and s24[12] == s24[20] == s24[0] and s24.count(s24[3]) == 2 and s24[16] == s24[3]
    assert max(p[2] for p in io._clamp([(1, 1, 10 ** 6)], n)) == n[2] - 12
    for name, lst in (("SRC24", s24), ("SRC33", s33), ("SRC_SHELL2", io.SRC_SHELL2(n, rb))):
        for p in lst:  # at least two cells inside the box: the bricks' rule in init_walls
            assert all(box[a][0] + 2 <= p[a] <= box[a][1] - 3 for a in range(3)), (name, p)
            assert p[2] <= n[2] - 12 or name == "SRC_SHELL2", (name, p)  # (the shell lists' last node goes by the box's edge, not by the clamp)
    s2, s1, s0 = io.SRC_SHELL2(n, rb), io.SRC_SHELL1(n, rb), io.SRC_SHELL0(n, rb)
    assert s2[:-1] == s1[:-1] == s0[:-1] == s24[:-1]
    assert (s2[-1][2], s1[-1][2], s0[-1][2]) == (box[2][1] - 3, box[2][1] - 2, box[2][1] - 1)
    r256, r321, rg = io.RCV256(sim), io.RCV321(sim), io.RCV_GHOST(sim)
    assert len(r256) == 256 and len(r321) == 321 and len(rg) == 331 and rg[:321] == r321
    for lst in (r256, r321):
        a = np.array(lst)
        assert (a >= 1).all() and (a <= np.array(n) - 2).all()
        assert len(lst) - len(set(lst)) >= 7  # the repeats
        on_bn = [p for p in lst if int(io.flat([p], n)[0]) in bn]
        shell = [p for p in lst if any(p[k] in (1, n[k] - 2) for k in range(3))]
        assert len(set(on_bn)) >= 6 and len(set(shell)) >= 6
    g = np.array(rg[321:])
    assert ((g == 0) | (g == np.array(n) - 1)).any(axis=1).all() and (0, 0, 0) in rg and tuple(np.array(n) - 1) in rg
    # no source list but SRC_WALLS touches a boundary node
    for lst in (s24, s33, s2, s1, s0):
        assert not set(io.flat(lst, n).tolist()) & bn
    sw = io.SRC_WALLS(sim, rb)
    assert len(sw) == 12 and len(set(sw)) == 11
    assert len(set(io.flat(sw, n).tolist()) & bn) >= 3
    for p in sw:  # outside the box, interior nodes of the grid
        assert not all(box[a][0] <= p[a] < box[a][1] for a in range(3)) and all(1 <= p[a] <= n[a] - 2 for a in range(3)), p
    assert sum(1 for p in sw if any(p[a] in (1, n[a] - 2) for a in range(3))) >= 2


# ---- 2. the scenes can fail: the oracle alone --------------------------------------------------------------------------------------------
def _near(nodes):
    seen = []
    for p in nodes:
        if p not in seen:
            seen.append(p)
    return [(x + 1, y, z) for x, y, z in seen]


@functools.lru_cache(maxsize=None)
def _control(prec, drop=-1, swap=False):
    """the oracle's u_out of case T's scene from its random fields: SRC24 (entry `drop` left out; the signals of the duplicates 0 and 12
    swapped), receivers RCV_GHOST and one node beside every source"""
    sim = io.t_scene(prec)
    n = io._dims(sim)
    io.scatter(sim, io.SRC24(n), io.RCV_GHOST(sim) + _near(io.SRC24(n)))
    c = sim["comms_out"]
    if swap:
        c["in_sigs"][[0, 12]] = c["in_sigs"][[12, 0]]
    if drop >= 0:
        keep = np.arange(24) != drop
        c["in_ixyz"], c["in_sigs"], c["Ns"] = c["in_ixyz"][keep], c["in_sigs"][keep], np.int64(23)
    sd = sim_data.SimData.from_sim(sim, prec)
    sd.in_sigs *= 4.0  # (scale_input's norm, 2^2 in both precisions, as a constant: dropping a row must not rescale the others)
    return io.oracle_run(sd, io.random_fields(n, prec))[0]


@pytest.mark.parametrize("prec", ["single", "double"])
def test_on_the_oracle_duplicate_order_and_every_source_matter_and_no_row_is_dead(prec):
    ref = _control(prec)
    assert np.isfinite(ref).all()
    assert io.live_rows(ref).all() and np.count_nonzero(ref == 0) == 0  # cap on dead rows with random fields: zero
    assert ref.shape == (331 + 21, io.T_NT)
    swapped = _control(prec, swap=True)
    changed = np.count_nonzero(swapped != ref)
    print(f"{prec}: swapping the duplicates 0 and 12 changes {changed} of {ref.size} samples")
    assert changed > 0, "the order of two entries of one node does not reach a receiver"
    for k in range(24):
        rows = np.count_nonzero((_control(prec, drop=k) != ref).any(axis=1))
        assert rows >= 1, f"source entry {k} reaches no receiver row"


# ---- 3. slabs by the Python path -----------------------------------------------------------------------------------------------------------
def _slab_sim(name, along_z):
    """the case's scene with one source node in every interior plane of the cut axis (no plane is clear of sources) and six repeats, shuffled;
    200 seeded receivers, two on the low and two on the high ghost plane of the cut axis"""
    kw, flag = cases.CASES[name]
    sim = synth.shoebox(**kw)
    n = io._dims(sim)
    fcc = flag > 0
    ax = 2 if along_z else 0
    rng = np.random.default_rng(17 + ax)

    def node(p, lo):
        q = [int(rng.integers(lo, n[a] - lo)) for a in range(3)]
        q[ax] = p
        if fcc and sum(q) % 2:
            q[1] += 1 if q[1] + 1 < n[1] - lo else -1
        return tuple(q)

    src = [node(p, 2) for p in range(1, n[ax] - 1)]
    src += [src[int(k)] for k in rng.choice(len(src), size=6, replace=False)]
    src = [src[int(k)] for k in rng.permutation(len(src))]
    rcv = [node(int(rng.integers(1, n[ax] - 1)), 1) for _ in range(196)] + [node(0, 1), node(0, 1), node(n[ax] - 1, 1), node(n[ax] - 1, 1)]
    rcv = [rcv[int(k)] for k in rng.permutation(200)]
    io.scatter(sim, src, rcv, seed=23)
    if flag == 2:
        synth.fold_fcc(sim)
        synth.sort_sim(sim)
    return sim, len(src)


@functools.lru_cache(maxsize=None)
def _slab_reference(name, prec, along_z):
    sd = sim_data.SimData.from_sim(_slab_sim(name, along_z)[0], prec)
    sd.scale_input()
    oracle.run_sim(sd)
    return sd.u_out.copy()


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("name,prec", [("cart_outside", "single"), ("cart_lossy", "double"), ("fcc2_outside", "double")])
@pytest.mark.parametrize("along_z", [False, True], ids=["cut_x", "cut_z"])
def test_slabs_with_a_source_in_every_plane_equal_the_single_domain(name, prec, G, along_z):
    ref = _slab_reference(name, prec, along_z)
    live = io.live_rows(ref).mean()
    print(f"{name} {prec} cut along {'z' if along_z else 'x'}: {100 * live:.0f} % of 200 rows live")
    assert np.isfinite(ref).all() and live >= 0.8  # (driven by their sources alone)
    sim, ns = _slab_sim(name, along_z)
    sd = sim_data.SimData.from_sim(sim, prec)
    sd.scale_input()
    assert sd.Ns == ns == (sd.Nz if along_z else sd.Nx) - 2 + 6 and sd.Nr == 200
    out = run_in_process(sd, G, along_z)
    assert np.array_equal(out, ref)
