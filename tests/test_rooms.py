"""CPU: synth.room (a room from any air mask) and the rooms of tests/rooms.py.

  * room(box mask) is shoebox, dataset by dataset: the plain box, blocks, rigid_every, lossy=False, FCC, wall=2;
  * every room: the boundary list sorted and unique, saf_bn the count of zero adjacency bits, solid-side nodes rigid, no source or receiver
    node on a boundary node -- and the oracle, started from seeded random fields, gives every receiver a non-zero, finite row (so the GPU
    tests of tests/test_hip_rooms.py compare something everywhere);
  * the oracle pinned to the compiled reference on three small rooms: tests/test_oracle_pinned.py (cases cart_pillar, cart_lroom, fcc2_balcony).
"""
import numpy as np
import pytest

import fullsize_oracle as fo
import rooms
from pffdtd_amd import sim_data, synth

BOXES = {
    "plain": dict(Nx=24, Ny=22, Nz=20, Nt=12, Nm=2, Mb=[2, 3], src=[12, 11, 10], rcv=[[8, 9, 7], [16, 14, 5]]),
    "blocks": dict(Nx=48, Ny=100, Nz=280, Nt=5, wall=3, Nm=2, Mb=[11, 3], src=[24, 70, 140], rcv=[[30, 20, 20], [4, 47, 142]],
                   blocks=((14, 18, 30, 40, 60, 130), (30, 30, 8, 12, 150, 260))),
    "rigid_every": dict(Nx=26, Ny=20, Nz=23, Nt=9, Nm=3, Mb=[11, 1, 12], rigid_every=7, sig="dhann30", src=[13, 10, 11], rcv=[[5, 5, 5]]),
    "rigid": dict(Nx=20, Ny=23, Nz=27, Nt=8, lossy=False, diff=False, src=[10, 11, 13], rcv=[[4, 17, 21], [14, 4, 4]]),
    "fcc": dict(Nx=24, Ny=28, Nz=20, Nt=10, fcc=True, Nm=2, Mb=[2, 3], rigid_every=5, sig="hann10", src=[12, 14, 10], rcv=[[7, 9, 8], [18, 20, 5]]),
    "fcc_blocks": dict(Nx=36, Ny=40, Nz=44, Nt=6, fcc=True, Nm=2, Mb=[11, 3], src=[8, 8, 8], rcv=[[28, 30, 36]], blocks=((12, 17, 14, 22, 10, 30),)),
    "wall2": dict(Nx=20, Ny=18, Nz=22, Nt=7, wall=2, Nm=1, Mb=3, src=[10, 9, 11], rcv=[[3, 3, 3], [15, 13, 17]]),
    "wall5": dict(Nx=23, Ny=25, Nz=35, Nt=7, wall=5, Nm=2, Mb=[3, 5], h=0.1, c=340.0, src=[11, 12, 17], rcv=[[6, 6, 6], [15, 17, 27]]),
}


@pytest.mark.parametrize("name", list(BOXES))
def test_room_of_a_box_mask_is_shoebox(name):
    kw = dict(BOXES[name])
    want = synth.shoebox(**kw)
    n = (kw.pop("Nx"), kw.pop("Ny"), kw.pop("Nz"))
    air = rooms.box_air(n, wall=kw.pop("wall", 3), blocks=kw.pop("blocks", ()))
    got = synth.room(air, **kw)
    assert got.keys() == want.keys()
    for f in want:
        assert list(got[f]) == list(want[f]), f
        for k in want[f]:
            a, b = np.asarray(got[f][k]), np.asarray(want[f][k])
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (f, k)
    assert int(want["vox_out"]["Nb"]) > 0


def test_room_refuses_air_in_the_outer_layers_and_cells_on_the_surface():
    n = (20, 18, 22)
    air = rooms.box_air(n)
    kw = dict(Nt=4, src=[9, 9, 9], rcv=[[5, 5, 5]])
    synth.room(air, **kw)
    for a in range(3):
        for i in (0, 1, -1, -2):
            bad = air.copy()
            bad[(slice(None),) * a + (i,)] = True
            with pytest.raises(AssertionError, match="outermost"):
                synth.room(bad, **kw)
    with pytest.raises(AssertionError, match="default"):
        synth.room(air, Nt=4)
    for cell in ([3, 9, 9], [2, 9, 9], [9, 15, 9], [9, 9, 0]):  # a corner on an air-side node, in the wall, on the far wall's nodes, in the solid
        with pytest.raises(AssertionError, match="corner node"):
            synth.room(air, Nt=4, src=[9, 9, 9], rcv=[cell])
        with pytest.raises(AssertionError, match="corner node"):
            synth.room(air, Nt=4, src=cell, rcv=[[9, 9, 9]])


def _all_rooms():
    out = [(name, prec, False) for name in rooms.ROOMS for prec in ("single", "double")]
    out += [(name, "single", True) for name in ("pillar", "balcony")]
    return out


def _build(name, prec, exchanged, Nt=4):
    if name.startswith("fcc_"):
        return rooms.build_fcc(name[4:], Nt)
    return rooms.build(name, Nt, prec=prec, exchanged=exchanged)


def check_invariants(sim, folded=False):
    v, c = sim["vox_out"], sim["comms_out"]
    bn, adj, mat, saf = v["bn_ixyz"], v["adj_bn"], v["mat_bn"], v["saf_bn"]
    assert bn.size == int(v["Nb"]) > 0 and adj.shape == (bn.size, 12 if int(sim["sim_consts"]["fcc_flag"]) else 6)
    assert (np.diff(bn) > 0).all(), "sorted and unique"
    assert np.array_equal(saf, (~adj).sum(axis=1).astype(np.float64)) and saf.min() >= 1
    assert mat.min() >= -1 and mat.max() < int(sim["sim_mats"]["Nmat"]) and (mat >= 0).any() and (mat < 0).any()
    assert not np.isin(c["in_ixyz"], bn).any() and not np.isin(c["out_ixyz"], bn).any()
    n = int(v["Nx"]) * int(v["Ny"]) * int(v["Nz"])
    assert 0 <= bn[0] and bn[-1] < n


@pytest.mark.parametrize("name,prec,exchanged", _all_rooms() + [("fcc_pillar", "single", False), ("fcc_balcony", "single", False)],
                         ids=lambda v: {True: "exchanged", False: "file"}.get(v, v))
def test_room_invariants(name, prec, exchanged):
    sim = _build(name, prec, exchanged)
    check_invariants(sim)
    if not name.startswith("fcc_"):  # solid-side nodes are rigid, air-side ones carry (x + 2 y + 3 z) mod Nm
        air = rooms.air_mask(name, rooms.size(name, prec))
        if exchanged:
            air = air.transpose(2, 1, 0)
        v = sim["vox_out"]
        x, y, z = synth._ind2sub(v["bn_ixyz"], air.shape[1], air.shape[2])
        ins = air[x, y, z]
        assert (v["mat_bn"][~ins] == -1).all() and np.array_equal(v["mat_bn"][ins], ((x + 2 * y + 3 * z)[ins] % 2).astype(np.int8))
        # the room differs from the plain box: more nodes than the box's, or nodes elsewhere
        box = synth.room(rooms.box_air(air.shape), 1, src=[20, 20, 20], rcv=[[20, 20, 20]])["vox_out"]["bn_ixyz"]
        assert not np.array_equal(box, v["bn_ixyz"])


@pytest.mark.parametrize("safeguarded", [False, True], ids=["exact", "safeguarded"])
@pytest.mark.parametrize("name,prec", [(name, prec) for name in rooms.ROOMS for prec in ("single", "double")] + [("fcc_pillar", "single"), ("fcc_balcony", "double")])
def test_oracle_reaches_every_receiver_from_random_fields(name, prec, safeguarded):
    """what fullsize_oracle.run_case asks of its reference before it compares anything: from seeded random fields, K = 11, every receiver
    row of the oracle non-zero and all of it finite"""
    K = 11
    sim = _build(name, prec, False, Nt=K)

    def make(mask):
        sd = sim_data.SimData.from_sim(sim, prec, build_mask=mask)
        sd.scale_input()
        return sd
    e, sd = fo.oracle_half(make, K, seed=7, safeguarded=safeguarded)
    try:
        fo.step_oracle(e, K)
        out = sd.u_out[:, :K]
        assert (np.abs(out).max(axis=1) > 0).all() and np.isfinite(out).all()
        assert np.isfinite(e.grid(0)).all() and np.isfinite(e.grid(1)).all()
    finally:
        e.close()
