"""Helper of tests/test_hip_fullsize_oracle.py: one scene stepped by the CPU oracle (oracle.Engine, OpenMP) and by the HIP engine
with its default options from the same seeded random fields, then compared bit for bit -- every receiver sample and every
interior cell of both state grids.  The oracle half (scene with mask, in-place fill, K steps) needs no GPU
(tests/test_fullsize_oracle_helper.py runs it, and the comparison's report, on the CPU).

Host memory: the oracle's two grids are the only full-size host arrays that live through a case; the device grids come back one
at a time (HipEngine.get_grid: one more full-size array) or, with device_view=True, one x block at a time through a torch view
of the engine's own device grids (HipEngine.state_grids + layout), so that no full-size copy exists."""
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

import oracle

XB = 16          # planes per block of the fill and of the comparison
AMPLITUDE = 1e-3  # the range bench.py's fields have


def mem_available_gb():
    """MemAvailable of /proc/meminfo in GB (None where there is no such file)"""
    try:
        for line in Path("/proc/meminfo").read_text().splitlines():
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024 / 1e9
    except OSError:
        pass
    return None


def fill_random(e, seed):
    """Both grids of an oracle.Engine, in place: U(-1, 1) * 1e-3 in the grid's precision, every cell (ghost layer, ABC shell, wall layers,
    box).  Each (grid, x block) has a generator of its own, so the values do not depend on how the blocks are spread over threads, and
    no second full-size array exists."""
    def one(args):
        k, x0 = args
        g = e.grid(k)
        rng = np.random.default_rng([seed, k, x0])
        blk = rng.random(g[x0:x0 + XB].shape, dtype=g.dtype)
        blk *= 2
        blk -= 1
        blk *= AMPLITUDE
        g[x0:x0 + XB] = blk
    jobs = [(k, x0) for k in (0, 1) for x0 in range(0, e.sd.Nx, XB)]
    with ThreadPoolExecutor(max_workers=min(8, oracle.default_threads())) as pool:
        list(pool.map(one, jobs))


def oracle_half(make_sd, K, seed, safeguarded=False):
    """-> (oracle.Engine with filled grids, not stepped yet; its SimData).  make_sd(build_mask) -> SimData, input already scaled."""
    sd = make_sd(True)
    assert sd.Nt >= K
    e = oracle.Engine(sd, safeguarded=safeguarded)
    fill_random(e, seed)
    return e, sd


def step_oracle(e, K):
    for n in range(K):
        e.step(n)


class Mismatch(AssertionError):
    pass


def compare_interior(block_of, ref, label):
    """ref[1:-1, 1:-1, 1:-1] against the same cells of the device grid, x block by x block; block_of(x0, x1) -> the device grid's planes
    x0 .. x1 - 1 in file order, (x1 - x0, Ny, Nz).  A difference raises Mismatch with the first differing cell (x, y, z), both values
    and the number of differing cells."""
    Nx = ref.shape[0]
    first, count = None, 0
    for x0 in range(1, Nx - 1, XB):
        x1 = min(x0 + XB, Nx - 1)
        got, want = block_of(x0, x1)[:, 1:-1, 1:-1], ref[x0:x1, 1:-1, 1:-1]
        assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape, got.dtype, want.dtype)
        if np.array_equal(got, want):
            continue
        bad = got != want
        count += int(bad.sum())
        if first is None:
            i = np.argwhere(bad)[0]
            first = ((x0 + int(i[0]), 1 + int(i[1]), 1 + int(i[2])), got[tuple(i)], want[tuple(i)])
    if first is not None:
        (x, y, z), g, w = first
        raise Mismatch(f"{label}: {count} of {(Nx - 2) * (ref.shape[1] - 2) * (ref.shape[2] - 2)} interior cells differ; first at "
                       f"(x, y, z) = ({x}, {y}, {z}): device {g!r} ({float(g).hex()}), oracle {w!r} ({float(w).hex()})")


def host_blocks(a):
    return lambda x0, x1: a[x0:x1]


class _DevPtr:
    """a device pointer with the array interface torch reads"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}


def device_blocks(eng, which):
    """block_of for compare_interior over the engine's OWN device grid `which` (0: u^{n-1}, 1: u^n), no full-size host copy: a torch view
    of the stored grid (planes, rows, pitch), brought to file order where the engine stores the file's x and z axes exchanged.  The ghost
    shell stays virtual here (compare_interior does not look at it)."""
    import torch
    eng.sync()
    dims, pitch, exchanged = eng.layout()
    ptr = eng.state_grids()[which]
    t = torch.as_tensor(_DevPtr(ptr, (dims[0], dims[1], pitch), "<f4" if eng.dtype == np.float32 else "<f8"), device="cuda")
    t = t[:, :, :dims[2]]
    if exchanged:
        t = t.permute(2, 1, 0)
    return lambda x0, x1: t[x0:x1].contiguous().cpu().numpy()


def run_case(make_sd, runs, seed=1, numerics=0, device_view=False, expect=None, log=print, name="", **engine_kw):
    """The comparison.  make_sd(build_mask) -> a scaled SimData of the scene (called twice: the oracle's with the mask, the engine's
    without, each with its own u_out); runs = [(n0, nsteps), ...] consecutive from 0: the oracle steps them one by one, the engine takes
    one run() per entry.  expect(timing, layout) asserts which path ran.  engine_kw: none for the default path; air_variant / debug to narrow
    a failure down (or to force a path the default does not take).  -> dict of wall times (s) and the engine's timing."""
    from pffdtd_amd import engine
    K = sum(n for _, n in runs)
    assert [n0 for n0, _ in runs] == [sum(n for _, n in runs[:i]) for i in range(len(runs))], runs
    T = {}
    t = time.time()
    e, sd_ref = oracle_half(make_sd, K, seed, safeguarded=numerics == engine.PF_NUM_GPU_SAFEGUARDED)
    T["scene+fill"] = time.time() - t
    t = time.time()
    sd_hip = make_sd(False)
    eng = engine.HipEngine(sd_hip, numerics=numerics, timing=True, **engine_kw)  # default options otherwise: air_variant 0, no debug, its own grids
    T["create"] = time.time() - t
    try:
        t = time.time()
        for k in (0, 1):
            eng.set_grid(k, e.grid(k))  # before the oracle's first step
        T["set_grid"] = time.time() - t
        t = time.time()
        step_oracle(e, K)
        T["oracle"] = time.time() - t
        T["oracle_gvox_s"] = sd_ref.Npts * K / T["oracle"] / 1e9
        t = time.time()
        for n0, n in runs:
            eng.run(n0, n)
        eng.sync()
        T["device"] = time.time() - t
        tm, lay = eng.timing(), eng.layout()
        T["timing"], T["layout"] = tm, lay
        log(f"[{name}] grid {sd_ref.Nx} x {sd_ref.Ny} x {sd_ref.Nz} {np.dtype(sd_ref.real).name} K={K}: " +
            ", ".join(f"{k} {v:.1f}" for k, v in T.items() if isinstance(v, float)) +
            f"; steps/pass {tm['tb_steps_per_pass']} tb2_launches {tm['tb2_launches']} wall_three_steps {tm['wall_three_steps']} wall_blocks {tm['wall_blocks']} "
            f"bricks {tm['wall_bricks']} dirty {tm['tb2_dirty_tiles']} air_path {tm['air_path']} layout {lay}")
        t = time.time()
        ref_out, out = sd_ref.u_out[:, :K], sd_hip.u_out[:, :K]
        assert (np.abs(ref_out).max(axis=1) > 0).all(), "a receiver row of the oracle is all zeros: nothing would be compared there"
        assert np.isfinite(ref_out).all()
        found = []  # every difference is reported, the fields' too when the receivers already differ: the first cell names the tile or pencil
        if not np.array_equal(out, ref_out):
            r, n = np.argwhere(out != ref_out)[0]
            found.append(f"receivers: {int((out != ref_out).sum())} of {out.size} samples differ; first at receiver node {r}, step {n}: "
                         f"device {out[r, n]!r}, oracle {ref_out[r, n]!r}")
        for k in (0, 1):
            g = None if device_view else eng.get_grid(k)
            try:
                compare_interior(device_blocks(eng, k) if device_view else host_blocks(g), e.grid(k), f"grid {k}")
            except Mismatch as ex:
                found.append(str(ex))
            del g
        if found:
            raise Mismatch("\n".join(found))
        T["compare"] = time.time() - t
        log(f"[{name}] compare {T['compare']:.1f} s: receivers and every interior cell of both grids equal")
        if expect is not None:
            expect(tm, lay)
    finally:
        eng.close()
        e.close()
        del e, eng
    return T
