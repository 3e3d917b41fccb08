"""Rooms whose geometry meets the walls (pffdtd_amd.synth.room): named air masks on a wall=3 box, each with a source and receivers of its own.
synth.shoebox builds a plain box with blocks that stand strictly inside it; here pillars stand on floors, balconies hang on walls, walls lean
and floors step, so the wall regions, the frame's bricks and the dirty tiles of the blocked kernels meet nodes no plain wall has.

Sizes: (48, 100, 280) for fp32 and (48, 100, 264) for fp64 -- the smallest the suite uses at which triples with three-step wall regions and
bricks exist (tests/test_hip_tb2.py: triple_scene).  Receivers are cells (their eight corner nodes p .. p + 1 carry the sample): beside the
geometry, in the two layers of cells between the walls and the triples' box (the wall regions' cells), in the frame, in the box."""
import numpy as np

from pffdtd_amd import synth

N32, N64 = (48, 100, 280), (48, 100, 264)
SIZES = {"leaning_z_wide": ((48, 100, 528), (48, 100, 528))}  # rooms at a size of their own (fp32, fp64)
WALL = 3


def size(name, prec="single"):
    n32, n64 = SIZES.get(name, (N32, N64))
    return n32 if prec == "single" else n64


def box_air(n, wall=WALL, blocks=()):
    """the air mask of synth.shoebox(*n, wall=wall, blocks=blocks)"""
    air = np.zeros(n, dtype=np.bool_)
    air[wall:n[0] - wall, wall:n[1] - wall, wall:n[2] - wall] = True
    for (x0, x1, y0, y1, z0, z1) in blocks:
        air[x0:x1 + 1, y0:y1 + 1, z0:z1 + 1] = False
    return air


def _pillar(air, n):
    air[30:36, :, 100:112] = False        # from the y-low wall to the y-high wall: the y regions' pencils along its sides hold a node in every cell


def _balcony(air, n):
    air[38:, 20:80, 60:64] = False        # hangs on the x-high wall


def _floor_step(air, n):
    air[:, 50:, :5] = False               # the z-low wall two cells deeper over half the room: extra geometry in a column strip only


def _l_room(air, n):
    air[24:, 50:, :] = False              # two faces wall over half their area only; the inner walls lie in the box


def _leaning_z(air, n):
    X, _, Z = np.ogrid[:n[0], :n[1], :n[2]]
    air &= Z < n[2] - 10 - X // 2         # a staircase wall through the high strip and into the box


def _leaning_x(air, n):
    X, Y, _ = np.ogrid[:n[0], :n[1], :n[2]]
    air &= X >= 3 + Y // 16               # the x-low wall's layers at depths 2 .. 9: from the region's pencils into the box


def _corner_block(air, n):
    air[:12, :14, :30] = False            # touches three walls and lies in the frame: bricks hold extra nodes


def _partition(air, n):
    door = air[20, 40:61, 100:181].copy()
    air[20, :, :] = False                 # one cell thick, touches all four y / z walls
    air[20, 40:61, 100:181] = door        # ... but for a doorway


# name -> (mask builder, source cell, receiver cells); z entries may be callables of Nz (the far z wall moves with the size)
def _far(d):
    return lambda nz: nz - d


ROOMS = {
    "pillar": (_pillar, [24, 50, 118], [[26, 49, 121], [4, 47, 142], [42, 52, 135], [24, 94, 144], [27, 88, 117], [5, 4, 141], [22, 51, _far(6)], [25, 52, 4],
                                        [27, 4, 104], [37, 94, 108], [32, 30, 97], [32, 60, 113], [27, 50, 105]]),
    "balcony": (_balcony, [30, 50, 70], [[32, 49, 73], [4, 47, 142], [42, 52, 135], [24, 94, 144], [27, 88, 137], [5, 4, 141], [22, 51, _far(6)], [25, 52, 4],
                                         [35, 50, 61], [42, 30, 57], [42, 70, 65], [40, 17, 61], [42, 81, 62]]),
    "floor_step": (_floor_step, [24, 50, 30], [[26, 49, 33], [4, 47, 142], [42, 52, 135], [24, 94, 144], [27, 88, 137], [5, 4, 141], [22, 51, _far(6)], [25, 30, 4],
                                               [25, 70, 6], [25, 47, 4], [25, 51, 6], [4, 80, 6], [42, 94, 6]]),
    "l_room": (_l_room, [12, 40, 140], [[14, 39, 143], [4, 47, 142], [42, 32, 135], [12, 94, 144], [15, 88, 137], [5, 4, 141], [10, 51, _far(6)], [13, 52, 4],
                                        [21, 60, 139], [30, 47, 150], [21, 47, 141], [42, 4, 120], [40, 30, _far(6)]]),
    "leaning_z": (_leaning_z, [24, 50, 200], [[26, 49, 203], [4, 47, 142], [42, 52, 135], [24, 94, 144], [27, 88, 137], [5, 4, 141], [25, 52, 4],
                                              [4, 51, _far(16)], [22, 51, _far(26)], [42, 50, _far(36)], [42, 94, _far(36)], [10, 4, _far(19)]]),
    # the same staircase in a room of two column tiles: at 280 columns it crosses every tile of the box, and the blocked kernels have nothing to do
    "leaning_z_wide": (_leaning_z, [24, 50, 448], [[26, 49, 451], [4, 47, 142], [42, 52, 135], [24, 94, 144], [27, 88, 137], [5, 4, 141], [25, 52, 4], [22, 51, 250],
                                                   [4, 51, _far(16)], [22, 51, _far(26)], [42, 50, _far(36)], [42, 94, _far(36)], [10, 4, _far(19)]]),
    "leaning_x": (_leaning_x, [24, 50, 140], [[26, 49, 143], [4, 7, 142], [42, 52, 135], [24, 94, 144], [27, 88, 137], [5, 4, 141], [22, 51, _far(6)], [25, 52, 4],
                                              [7, 47, 142], [10, 94, 140], [8, 60, 4], [9, 75, _far(6)], [6, 30, 139]]),
    "corner_block": (_corner_block, [16, 18, 34], [[18, 17, 37], [4, 47, 142], [42, 52, 135], [24, 94, 144], [27, 88, 137], [13, 4, 20], [22, 51, _far(6)], [25, 52, 4],
                                                   [4, 15, 20], [5, 6, 31], [13, 15, 10], [13, 15, 4], [4, 4, 31]]),
    "partition": (_partition, [24, 50, 140], [[26, 49, 143], [4, 47, 142], [42, 52, 135], [24, 94, 144], [27, 88, 137], [5, 4, 141], [22, 51, _far(6)], [25, 52, 4],
                                              [17, 50, 140], [22, 30, 90], [17, 94, 200], [22, 4, 50], [17, 70, _far(6)], [22, 41, 101]]),
}


def air_mask(name, n):
    air = box_air(n)
    ROOMS[name][0](air, n)
    return air


def cells(name, n):
    """-> (source cell, receiver cells) of a room at size n"""
    _, src, rcv = ROOMS[name]
    fix = lambda p: [int(v(n[2]) if callable(v) else v) for v in p]
    return fix(src), [fix(p) for p in rcv]


def build(name, Nt, prec="single", Mb=(11, 3), exchanged=False, rcv_in_box=False, **kw):
    """the room `name` at the size of its precision.  exchanged: built with x and z exchanged (the mask transposed, every cell reversed).
    rcv_in_box: only the receivers well inside the triples' box (8 cells from the x / y faces, 16 from the z faces)."""
    n = size(name, prec)
    air = air_mask(name, n)
    src, rcv = cells(name, n)
    if rcv_in_box:
        rcv = [p for p in rcv if all(m <= v <= d - m - 2 for v, d, m in zip(p, n, (8, 8, 16)))]
        assert len(rcv) >= 2
    if exchanged:
        air, src, rcv = np.ascontiguousarray(air.transpose(2, 1, 0)), src[::-1], [p[::-1] for p in rcv]
    return synth.room(air, Nt, Nm=len(Mb), Mb=list(Mb), src=src, rcv=rcv, **kw)


# ---- 13-point rooms on the grid of tests/test_hip_tb2.py's fcc_scene: stored (36, 70, 280), unfolded Ny = 138 -------------------------------
NFCC = (36, 70, 280)


def _fcc_pillar(air):
    air[22:28, :, 100:112] = False


def _fcc_balcony(air):
    air[28:, 30:110, 60:64] = False


FCC_ROOMS = {"pillar": (_fcc_pillar, [18, 34, 120], [[20, 37, 116], [13, 36, 126], [29, 30, 105], [19, 60, 97], [24, 100, 115], [4, 20, 140], [18, 5, 104]]),
             "balcony": (_fcc_balcony, [18, 34, 70], [[20, 37, 66], [13, 36, 76], [24, 50, 57], [30, 90, 67], [30, 26, 61], [4, 20, 140], [24, 100, 60]])}


def build_fcc(name, Nt, Mb=(11, 3)):
    """a 13-point room, folded and sorted like fcc_scene's (cells moved by one in z onto the even subgrid where needed)"""
    n = (NFCC[0], 2 * (NFCC[1] - 1), NFCC[2])
    air = box_air(n)
    mask, src, rcv = FCC_ROOMS[name]
    mask(air)
    even = lambda p: [p[0], p[1], p[2] + (sum(p) % 2)]
    sim = synth.room(air, Nt, fcc=True, Nm=len(Mb), Mb=list(Mb), src=even(src), rcv=[even(p) for p in rcv])
    synth.fold_fcc(sim)
    synth.sort_sim(sim)
    return sim


# ---- small rooms for tests/cases.py (the oracle against the compiled reference) ---------------------------------------------------------------
def _small_pillar(air):
    air[16:19, :, 9:12] = False           # wall to wall along y


def _small_lroom(air):
    air[15:, 14:, :] = False


def _small_balcony(air):
    air[22:, 8:24, 10:12] = False         # on the x-high wall


SMALL = {"pillar": _small_pillar, "lroom": _small_lroom, "balcony": _small_balcony}


def small_air(name, n):
    air = box_air(n)
    SMALL[name](air)
    return air


# ---- rooms for a chain of slabs cut along x: (124, 70, 276), the size of tests/test_hip_multi.py's triples test --------------------------------
NCHAIN = (124, 70, 276)


def _chain_pillar(air):
    air[38:46, :, 100:112] = False        # wall to wall along y; planes 38 .. 45 straddle the first cut of a three-slab chain (x = 39)


def _chain_floor_step(air):
    air[:, 35:, :5] = False               # through every slab


# name -> (mask builder, source cell, receiver cells): a chain has no set_grid, so the runs are source-driven -- the source within a dozen cells of
# the geometry and of a wall, receivers beside the geometry, in the wall layers and on both sides of the cuts (x = 39, 86 for three slabs, 62 for two; the far cut at the reach of 41 steps)
CHAIN_ROOMS = {
    "box": (lambda air: None, [50, 10, 108], [[52, 12, 104], [40, 10, 110], [41, 9, 106], [47, 4, 108], [50, 10, 96], [60, 8, 108], [62, 11, 107], [44, 20, 120], [36, 6, 103],
                                              [84, 10, 108], [86, 10, 108]]),
    "pillar": (_chain_pillar, [50, 10, 108], [[52, 12, 104], [40, 10, 114], [41, 9, 113], [47, 4, 108], [47, 12, 104], [60, 8, 108], [62, 11, 107], [42, 20, 96], [35, 6, 103],
                                              [39, 4, 97], [43, 30, 113], [84, 10, 108], [86, 10, 108]]),
    "floor_step": (_chain_floor_step, [50, 30, 16], [[52, 32, 12], [40, 33, 8], [41, 36, 7], [42, 28, 4], [50, 40, 6], [60, 35, 7], [62, 34, 9], [48, 4, 10], [45, 50, 6],
                                                     [84, 30, 16], [86, 30, 16]]),
}


def build_chain(name, Nt, Mb=(11, 3)):
    air = box_air(NCHAIN)
    mask, src, rcv = CHAIN_ROOMS[name]
    mask(air)
    return synth.room(air, Nt, Nm=len(Mb), Mb=list(Mb), src=src, rcv=rcv)
