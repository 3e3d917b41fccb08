"""Source and receiver lists anywhere in the grid: one scene editor (scatter) and the named lists of tests/test_io_lists.py (CPU) and
tests/test_hip_io_lists.py (GPU).  The engine's host rules read both lists -- how many nodes, in which tiles, how near the shell, on which
side of a cut -- and the suite's scenes all had one source cell and a few receiver cells in plain air.

Nodes are FILE coordinates (x, y, z).  The named lists are functions of the grid size n = (Nx, Ny, Nz) -- and, where they need the boundary
lists, of the scene --, so that the fp64 shapes with 264 columns get lists of their own; every z is clamped to Nz - 12.

The box of a three-step pass (Engine::init_tb2_impl) on the 48 x 100 x 280 shoebox with wall = 3, as triple_box() below works it out:
x [6, 42), y [6, 94), z [16, 264) in fp32 and z [16, 256) on the 264-column grid in fp64; tiles of 20 rows from y = 6 (borders at 26, 46,
66, 86), x chunks of 12 planes from x = 6 (borders at 18, 30), and ONE column tile of 248 columns in fp32, two of 120 in fp64 (border at
136).  init_walls keeps the wall regions while every source is at least one cell inside that box, the frame's bricks while every source is
at least two cells inside.
"""
import numpy as np

from pffdtd_amd import synth


def _dims(sim):
    v = sim["vox_out"]
    return int(v["Nx"]), int(v["Ny"]), int(v["Nz"])


def _as_nodes(nodes, n, what):
    a = np.asarray(nodes, dtype=np.int64).reshape(-1, 3)
    if a.size and ((a < 0).any() or (a >= np.asarray(n)).any()):
        raise ValueError(f"{what}: a node outside the grid {n}")
    return a


def flat(nodes, n):
    a = np.asarray(nodes, dtype=np.int64).reshape(-1, 3)
    return (a[:, 0] * n[1] + a[:, 1]) * n[2] + a[:, 2]


def scatter(sim, src_nodes=None, rcv_nodes=None, seed=0):
    """Replace the source and / or receiver list of sim["comms_out"] (in place; returns sim).  The order given is kept, unsorted, and
    duplicates stay.  Row k of in_sigs = the scene's first signal over its peak, rolled by k % 7 samples, times a seeded factor in [0.2, 1]
    with alternating sign: every listed node, a duplicate too, has a signal of its own.  Receivers: identity out_reorder, out_alpha of ones.
    On an FCC scene an odd-parity node is refused.  Runs BEFORE synth.fold_fcc (the nodes are coordinates of the unfolded grid)."""
    c, n = sim["comms_out"], _dims(sim)
    fcc = int(sim["sim_consts"]["fcc_flag"])
    if fcc == 2:
        raise ValueError("scatter edits the unfolded scene: call it before synth.fold_fcc")
    for what, nodes in (("src_nodes", src_nodes), ("rcv_nodes", rcv_nodes)):
        if nodes is not None and fcc and (_as_nodes(nodes, n, what).sum(axis=1) % 2).any():
            raise ValueError(f"{what}: an odd-parity node on an FCC grid")
    if src_nodes is not None:
        a = _as_nodes(src_nodes, n, "src_nodes")
        base = np.asarray(c["in_sigs"], dtype=np.float64)[0]
        base = base / np.abs(base).max()
        fac = np.random.default_rng(seed).uniform(0.2, 1.0, size=a.shape[0])
        c["in_ixyz"] = flat(a, n)
        c["Ns"] = np.int64(a.shape[0])
        c["in_sigs"] = np.stack([np.roll(base, k % 7) * fac[k] * (-1.0) ** k for k in range(a.shape[0])]).reshape(a.shape[0], base.size)
    if rcv_nodes is not None:
        a = _as_nodes(rcv_nodes, n, "rcv_nodes")
        c["out_ixyz"] = flat(a, n)
        c["Nr"] = np.int64(a.shape[0])
        c["out_reorder"] = np.arange(a.shape[0], dtype=np.int64)
        c["out_alpha"] = np.ones((a.shape[0], 1))
    return sim


def _clamp(nodes, n):
    return [(x, y, min(z, n[2] - 12)) for x, y, z in nodes]


# ---- the box of a three-step pass ----------------------------------------------------------------------------------------------------
def triple_box(n, real_bytes, wall=3):
    """((x0, x1), (y0, y1), (z0, z1)), upper bounds exclusive: the box Engine::init_tb2_impl(triple = true) gives a single-domain 7-point
    engine on a shoebox whose wall planes (depth wall - 1 and wall on every face, each more than half boundary nodes) push it to depth
    wall + 3, the column range rounded to whole vectors, a sliver of up to 256 bytes left to the right strip, then shifted so that both
    column strips become wall regions (wl_lo_option / wl_hi_option, pf_engine_walls.inc).  A restatement of those rules for the tests' list
    builders; the GPU tests pin it through wall_bricks and wall_blocks, which change when a source crosses these bounds."""
    Nx, Ny, Nz = n
    f32 = real_bytes == 4
    V = 4 if f32 else 2
    m = max(4, wall + 3)
    mz = (m + 3) // 4 * 4
    TC = (64 - 2 * (1 if f32 else 2)) * V
    P = -(-Nz // (128 // real_bytes)) * (128 // real_bytes)
    z0, z1full = mz, (Nz - mz) // 4 * 4
    z1 = z1full
    nz, rem = z1 - z0, (z1 - z0) % TC
    if nz > TC and rem > 0 and rem * real_bytes <= 256:
        z1 -= rem

    def lo_opt(t0, ps):
        split, wide = t0 >= 10 and t0 - 2 <= 16, f32 and t0 + 2 <= 20
        if t0 + 2 <= 12:
            return 1
        if split and (ps or not wide):
            return 2
        return 3 if wide else 0

    def hi_opt(t1, ps):
        z2 = (t1 - 2) // 4 * 4
        za, zw = min(z2, P - 12), -(-(Nz - 12) // 4) * 4
        s0, z20 = zw + 4, min(z2, P - 20)
        split = zw >= 0 and zw + 12 <= P and s0 > t1 and s0 + 2 - z2 <= 16 and z2 + 16 <= P and Nz - 1 - zw <= 11
        wide = f32 and z20 >= 0 and z20 + 20 >= Nz and t1 - z20 >= 2
        if za >= 0 and za + 12 >= Nz and t1 - za >= 2:
            return 1
        if split and (ps or not wide):
            return 2
        return 3 if wide else 0

    if z1 < z1full:
        ps, best = not f32, (1 << 30, 0)
        for sh in range(0, z1full - z1 + 1, 4):
            lo, hi = lo_opt(z0 + sh, ps), hi_opt(z1 + sh, ps)
            need = max(z0 + sh + 2, Nz - (z1 + sh - 2) // 4 * 4) + (((lo == 2) + (hi == 2)) * 100 if lo and hi else 1000)
            if need < best[0]:
                best = (need, sh)
        z0, z1 = z0 + best[1], z1 + best[1]
    return (m, Nx - m), (m, Ny - m), (z0, z1)


# ---- sources -----------------------------------------------------------------------------------------------------------------------
def SRC24(n):
    """24 nodes at least two cells inside the box of the 48 x 100 x 280 scene (both precisions), two of them listed three and two times, out
    of order.  Against the list the task named, runs were moved onto the borders init_tb2_impl really has and every node moved at least two
    cells inside the box (bricks: x 8..39, y 8..91, z 18..261, fp64 18..253), since the same list must leave the frame's bricks standing:
      0-1    along y over the row-tile border 45 | 46
      2-4    along y over the row-tile border 25 | 26, then a diagonal step
      5-7    a diagonal over the x-chunk border 29 | 30, the row-tile border 45 | 46 and fp64's column-tile border 135 | 136 (fp32 has a
             single column tile of 248 columns: no column border exists there)
      10, 11 the lowest and highest corners that are still two cells inside the box on all three axes
      13-15  along x over the x-chunk border 17 | 18
      17-18  along y over the row-tile border 65 | 66
      12, 20 node 0 again; 16: node 3 again"""
    return _clamp([(24, 45, 140), (24, 46, 140), (12, 25, 30), (12, 26, 30), (13, 26, 31), (29, 45, 135),
                   (30, 45, 136), (30, 46, 137), (20, 70, 200), (35, 80, 60), (8, 8, 18), (39, 91, 261),
                   (24, 45, 140), (17, 43, 128), (18, 43, 128), (19, 43, 128), (12, 26, 30), (22, 65, 19),
                   (22, 66, 19), (38, 12, 258), (24, 45, 140), (9, 88, 133), (26, 26, 26), (33, 61, 190)], n)


def SRC33(n):
    """SRC24 and nine more nodes of the box: 33 > TB3_MAXSRC, so k_tb3 leaves the samples to k_io"""
    return SRC24(n) + _clamp([(10, 30, 40), (15, 55, 90), (21, 12, 111), (27, 77, 222), (31, 20, 160), (36, 36, 36), (14, 84, 240),
                             (25, 47, 139), (32, 67, 73)], n)


def _shell(n, real_bytes, depth):
    """SRC24 with its last node `depth` cells inside the box's z-high edge (z1 - 1 - depth; x and y stay deep inside)"""
    z1 = triple_box(n, real_bytes)[2][1]
    s = SRC24(n)
    return s[:-1] + [(s[-1][0], s[-1][1], z1 - 1 - depth)]


def SRC_SHELL2(n, real_bytes):
    """the last node two cells inside the box's z-high edge (z = z1 - 3, the last z init_walls' brick rule accepts): the bricks stay"""
    return _shell(n, real_bytes, 2)


def SRC_SHELL1(n, real_bytes):
    """one cell inside (z = z1 - 2, the last z the wall regions' rule accepts): the bricks go, the regions stay"""
    return _shell(n, real_bytes, 1)


def SRC_SHELL0(n, real_bytes):
    """on the box's outermost cell (z = z1 - 1): the wall regions go too"""
    return _shell(n, real_bytes, 0)


def boundary_nodes(sim, lossy):
    """(x, y, z) of the scene's frequency-dependent (lossy = True) or rigid boundary nodes, in list order"""
    v, n = sim["vox_out"], _dims(sim)
    ii = np.asarray(v["bn_ixyz"])[(np.asarray(v["mat_bn"]) >= 0) == lossy]
    return [tuple(int(q) for q in p) for p in zip(*synth._ind2sub(ii, n[1], n[2]))]


def SRC_WALLS(sim, real_bytes, wall=3):
    """12 nodes outside the box of the three-step pass: air cells between the boundary skin (depth `wall`) and the box on four faces, a
    frequency-dependent boundary node, a rigid one on the air side (a scene built with rigid_every), two ABC-shell cells (index 1: a face
    cell and the far corner cell; both lie outside the closed room, as does the rigid outer wall layer's node), and a duplicate."""
    n = _dims(sim)
    (x0, x1), (y0, y1), (z0, z1) = triple_box(n, real_bytes, wall)
    cx, cy, cz = n[0] // 2, n[1] // 2, n[2] // 2
    lossy, rigid = boundary_nodes(sim, True), boundary_nodes(sim, False)
    air_side = [p for p in rigid if all(wall <= p[a] <= n[a] - 1 - wall for a in range(3))]  # (rigid_every's nodes: the inner wall layer)
    outer = [p for p in rigid if any(p[a] in (wall - 1, n[a] - wall) for a in range(3))]
    assert lossy and air_side and outer, "SRC_WALLS needs a scene with frequency-dependent and rigid_every nodes"
    nodes = [(x0 - 2, cy, cz), (x1 + 1, cy + 3, cz - 5), (cx, y0 - 1, cz + 7), (cx + 2, cy, z1 + 2),
             lossy[len(lossy) // 3], air_side[len(air_side) // 2], (1, cy - 4, cz + 9), (n[0] - 2, n[1] - 2, n[2] - 2),
             outer[len(outer) // 4], (cx - 3, cy + 6, z0 - 3), (x0 - 2, cy, cz), lossy[-1]]
    assert len(nodes) == 12
    return nodes


def air_nodes(sim, count, dup, seed, fcc=False, margin=3):
    """`count` seeded nodes of the scene, shuffled, `dup` of them repeats: interior nodes at least `margin` cells off every face of the grid
    and off every boundary node (sources must be interior nodes; the reference adds them wherever the list says)"""
    n = _dims(sim)
    rng = np.random.default_rng(seed)
    bn = set(np.asarray(sim["vox_out"]["bn_ixyz"]).tolist())
    out = []
    while len(out) < count - dup:
        p = [int(rng.integers(margin, n[a] - margin)) for a in range(3)]
        if fcc and sum(p) % 2:
            p[2] += 1 if p[2] + 1 < n[2] - margin else -1
        if int(flat([p], n)[0]) not in bn and tuple(p) not in out:
            out.append(tuple(p))
    out += [out[int(k)] for k in rng.choice(len(out), size=dup, replace=False)]
    return [out[int(k)] for k in rng.permutation(len(out))]


# ---- receivers ---------------------------------------------------------------------------------------------------------------------
def _even(p, n, free):
    """p with even parity: one of the `free` axes moved by a cell, staying in [1, N - 2]"""
    p = list(p)
    if sum(p) % 2:
        a = free[0]
        p[a] += 1 if p[a] + 1 <= n[a] - 2 else -1
    return tuple(p)


def _receivers(sim, count, seed, fcc):
    n = _dims(sim)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count - 19):  # seeded draws from the interior [1, N - 2] of every axis
        p = tuple(int(rng.integers(1, n[a] - 1)) for a in range(3))
        out.append(_even(p, n, [2]) if fcc else p)
    mid = [d // 2 for d in n]
    shell = [(1, mid[1], mid[2]), (n[0] - 2, mid[1] + 1, mid[2] - 2), (mid[0], 1, mid[2] + 3), (mid[0] - 2, n[1] - 2, mid[2]),
             (mid[0] + 1, mid[1] - 3, 1), (mid[0], mid[1] + 2, n[2] - 2)]  # six ABC-shell cells, one per face
    for a, p in enumerate(shell):
        out.append(_even(p, n, [k for k in range(3) if k != a // 2]) if fcc else p)
    bnl = boundary_nodes(sim, True)
    allbn = [tuple(int(q) for q in p) for p in zip(*synth._ind2sub(np.asarray(sim["vox_out"]["bn_ixyz"]), n[1], n[2]))]
    out +=[allbn[0], allbn[len(allbn) // 2], allbn[-1]]  # first, middle and last of bn_ixyz
    out += [bnl[len(bnl) // 5], bnl[len(bnl) // 2 + 1], bnl[-2]] if len(bnl) >= 3 else [allbn[1], allbn[2], allbn[3]]  # three of bnl_ixyz
    out += [out[int(k)] for k in rng.choice(len(out), size=7, replace=False)]  # seven repeats
    assert len(out) == count
    return [out[int(k)] for k in rng.permutation(count)]


def RCV256(sim, seed=5, fcc=False):
    """exactly 256 nodes (k_io's thread that adds the sources is then the first thread of a third block): 237 seeded draws from the interior
    [1, N - 2] of every axis, six ABC-shell cells, six boundary nodes (first, middle and last of bn_ixyz, three of bnl_ixyz), seven repeats;
    shuffled"""
    return _receivers(sim, 256, seed, fcc)


def RCV321(sim, seed=7, fcc=False):
    """the same make with 321 nodes: three blocks of receivers, the source thread in the third"""
    return _receivers(sim, 321, seed, fcc)


def ghost_cells(n):
    """ten ghost cells: one on each of the six faces, two edge cells, the corners (0, 0, 0) and (Nx-1, Ny-1, Nz-1)"""
    Nx, Ny, Nz = n
    mx, my, mz = Nx // 2, Ny // 2, Nz // 2
    return [(0, my, mz), (Nx - 1, my + 1, mz - 1), (mx, 0, mz + 2), (mx + 1, Ny - 1, mz), (mx - 1, my, 0), (mx, my - 2, Nz - 1),
            (0, 0, mz), (Nx - 1, my, Nz - 1), (0, 0, 0), (Nx - 1, Ny - 1, Nz - 1)]


def RCV_GHOST(sim, seed=7):
    """RCV321 and ten ghost cells (Engine::fused_ok: a receiver that reads a ghost cell takes the fused kernels away)"""
    return RCV321(sim, seed) + ghost_cells(_dims(sim))


def live_rows(u_out):
    """per receiver row: has it a non-zero sample?"""
    return np.abs(u_out).max(axis=1) > 0


# ---- the scene of the three-step cases and the oracle's run from random fields ---------------------------------------------------------
T_NT = 22


def t_scene(prec, **kw):
    """48 x 100 x 280 (264 columns in fp64), wall = 3, Mb = [11, 3], 22 steps of a differentiated Hann pulse: the smallest room whose box
    steps three times per pass with wall regions and bricks around it (tests/test_hip_tb2.py: triple_scene)"""
    from test_hip_tb2 import triple_scene
    return triple_scene(Nt=T_NT, n=(48, 100, 280 if prec == "single" else 264), wall=3, sig="dhann30", **kw)


def random_fields(n, prec, seed=61):
    """seeded random u^{n-1}, u^n of 1e-2: every cell live from step 0"""
    rng = np.random.default_rng(seed)
    dt = np.float32 if prec == "single" else np.float64
    return [(rng.standard_normal(n) * 1e-2).astype(dt) for _ in range(2)]


def oracle_run(sd, init=None, safeguarded=False):
    """oracle.Engine over sd.Nt steps from `init` (None: zero fields) -> (u_out, u^{n-1}, u^n); sd needs its bit mask"""
    import oracle
    e = oracle.Engine(sd, safeguarded=safeguarded)
    if init is not None:
        for k in (0, 1):
            e.grid(k)[...] = init[k]
    for k in range(sd.Nt):
        e.step(k)
    out = (sd.u_out.copy(), e.grid(0).copy(), e.grid(1).copy())
    e.close()
    return out
