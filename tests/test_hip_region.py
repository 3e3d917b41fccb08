"""GPU: field regions (pf_engine_get_region / pf_multi_get_region, pffdtd_amd/fields.py, the CLI's --field-planes / --field-box).

The bar: every cell of a region -- ghost cells and the folded row included -- is bit for bit the cell get_grid(which) gives (a chain: the cell
its own save_state writes), its interior cells are the oracle's, and asking changes nothing: the run continues to the oracle's receivers and
fields.  Regions are asked for BEFORE the whole-grid copy they are compared with, so the ghost shell they show is the one they materialised
themselves.  Every comparison is np.array_equal.

The box of the issue, [3:29:1, 1:27:2, 2:25:3], is cut to the grid where a scene is smaller (cart_mb11 is 26 x 20 x 22, the folded grids have
fewer rows): it keeps its odd start, its strides and extents that are no multiple of 32.
"""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import cases
import oracle
from pffdtd_amd import engine, fields, h5io, sim_data, synth
from test_hip_checkpoint import N_END, N_SAVE, STOP, Triple, _plates_room

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _slices(r):
    lo, hi, st = r
    return tuple(slice(lo[a], hi[a], st[a]) for a in range(3))


def _regions(N, extra=()):
    """the whole grid last (it would materialise the shell for everybody after it)"""
    full = lambda: ([0, 0, 0], list(N), [1, 1, 1])
    out = []
    for a in range(3):
        for k in (N[a] // 2, 0, N[a] - 1):
            lo, hi, st = full()
            lo[a], hi[a] = k, k + 1
            out.append((lo, hi, st))
    out.append(([3, 1, 2], [min(29, N[0]), min(27, N[1]), min(25, N[2])], [1, 2, 3]))
    out.append(([N[0] // 3, N[1] - 2, 5], [N[0] // 3 + 1, N[1] - 1, 6], [1, 1, 1]))  # 1 x 1 x 1
    out.extend(extra)
    out.append(full())
    return out


def _check_regions(obj, regions, whole, ref_fields, label):
    """whole(which) -> the object's own whole field, asked for AFTER the regions; ref_fields[which]: the oracle's"""
    N = ref_fields[0].shape
    inner = np.zeros(N, dtype=bool)
    inner[1:-1, 1:-1, 1:-1] = True
    got = {(w, i): obj.get_region(w, *r) for w in (1, 0) for i, r in enumerate(regions)}
    for w in (0, 1):
        g = whole(w)
        assert np.abs(g).max() > 0
        for i, r in enumerate(regions):
            s = _slices(r)
            want = g[s]
            assert got[(w, i)].shape == want.shape and got[(w, i)].dtype == g.dtype, (label, w, r)
            assert np.array_equal(got[(w, i)], want), (label, w, r, int(np.count_nonzero(got[(w, i)] != want)))
            sel = inner[s]
            assert np.array_equal(got[(w, i)][sel], ref_fields[w][s][sel]), (label, "oracle", w, r)


# ---- 1. the four small scenes: every region equals get_grid's cells, and the oracle's inside ---------------------------------------------
@pytest.mark.parametrize("name,prec", [("cart_outside", "double"), ("cart_mb11", "single"), ("fcc2_outside", "double"), ("fcc1_outside", "double")])
def test_regions_equal_get_grid_and_the_oracle(name, prec):
    nsteps = 23
    ref_sd = cases.make_sd(name, prec)
    ref = oracle.Engine(ref_sd)
    for n in range(nsteps):
        ref.step(n)
    ref_fields = [ref.grid(0).copy(), ref.grid(1).copy()]
    sd = cases.make_sd(name, prec)
    eng = engine.HipEngine(sd)
    eng.run(0, nsteps)
    _check_regions(eng, _regions((sd.Nx, sd.Ny, sd.Nz)), eng.get_grid, ref_fields, name)
    # nothing a later step reads has changed
    eng.run(nsteps, sd.Nt - nsteps)
    for n in range(nsteps, ref_sd.Nt):
        ref.step(n)
    assert np.array_equal(sd.u_out, ref_sd.u_out) and np.abs(ref_sd.u_out).max() > 0
    assert np.array_equal(eng.get_region(1, [1, 1, 1], [sd.Nx - 1, sd.Ny - 1, sd.Nz - 1]), ref.grid(1)[1:-1, 1:-1, 1:-1])
    ref.close()
    eng.close()


# ---- 2. five engines that share no kernel, layout or decomposition ------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["single", "double"])
def triple(request):
    return Triple(request.param)


@pytest.mark.parametrize("kind", ["v25", "v40", "exchanged", "chain3", "chain2z"])
def test_regions_of_every_engine_and_chain(triple, kind):
    obj, sd = triple.maker(kind)()
    obj.load_state(triple.start)
    obj.run(0, N_SAVE)
    N = triple.n
    extra = [([1, 2, 1], [N[0] - 1, N[1] - 2, N[2] - 1], [3, 1, 5])]  # crosses every cut, strides 3 (x) and 5 (z)
    if isinstance(obj, engine.HipMulti):
        info = obj.info()
        a = 2 if kind == "chain2z" else 0
        assert info["cut_along_z"] == (kind == "chain2z") and info["nslabs"] == (2 if kind == "chain2z" else 3), info
        for g in range(obj.nslabs):  # planes exactly on x0 and x1 - 1 of every slab
            for k in (obj.slab(g)["x0"], obj.slab(g)["x1"] - 1):
                lo, hi = [0, 0, 0], list(N)
                lo[a], hi[a] = k, k + 1
                extra.append((lo, hi, [1, 1, 1]))
        saved = {}

        def whole(w):
            if not saved:
                saved.update(obj.save_state())
            return saved["u_cur" if w else "u_prev"]
    else:
        tm = obj.timing()
        if kind == "v40":
            assert tm["tb_steps_per_pass"] == 3, tm
        if kind == "exchanged":
            assert obj.layout()[2]
        whole = obj.get_grid
    _check_regions(obj, _regions(N, extra), whole, triple.ref_fields[N_SAVE], f"{kind} {triple.prec}")
    obj.run(N_SAVE, N_END - N_SAVE)  # the state is what it was: on to the oracle's receivers and final fields
    out, after = sd.u_out.copy(), obj.save_state()
    obj.close()
    triple.check_end(out, after, f"{kind} after get_region")


# ---- 3. a region larger than the staging buffer moves in pieces ----------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [engine.PF_LAYOUT_FILE, engine.PF_LAYOUT_EXCHANGED], ids=["file_order", "exchanged"])
def test_a_region_larger_than_the_staging_buffer(layout):
    n = (132, 182, 182)
    sd = sim_data.SimData.from_sim(synth.shoebox(*n, Nt=4, Nm=1, Mb=3), "double", build_mask=False)
    sd.scale_input()
    eng = engine.HipEngine(sd, layout=layout)
    assert eng.layout()[2] == (layout == engine.PF_LAYOUT_EXCHANGED)
    rng = np.random.default_rng(71)
    a = rng.standard_normal(n)
    eng.set_grid(1, a)
    lo, hi = [1, 1, 1], [131, 181, 181]
    assert 130 * 180 * 180 * 8 > 32 << 20  # PF_REGION_STAGE_BYTES: two pieces
    got = eng.get_region(1, lo, hi)
    assert np.array_equal(got, a[1:131, 1:181, 1:181])
    got = eng.get_region(1, [0, 0, 0], n, [1, 1, 1])  # the whole grid, faces included: what get_grid gives
    assert np.array_equal(got, eng.get_grid(1))
    got = eng.get_region(1, [1, 0, 3], [132, 182, 182], [2, 3, 1])
    assert np.array_equal(got, eng.get_grid(1)[1::2, ::3, 3:])
    eng.close()


# ---- 4. refusals; the energy diagnostic; the receiver ring ----------------------------------------------------------------------------------
def test_refusals_and_what_is_left_alone():
    prec, steps = "single", 5
    ref = cases.make_sd("cart_mb11", prec)
    rng = np.random.default_rng(73)
    init = [(rng.standard_normal((ref.Nx, ref.Ny, ref.Nz)) * 1e-2).astype(np.float32) for _ in range(2)]
    e = oracle.Engine(ref)
    for k in (0, 1):
        e.grid(k)[...] = init[k]
    for n in range(steps):
        e.step(n)
    ref_u1 = e.grid(1).copy()
    e.close()
    assert np.abs(ref.u_out[:, :steps]).min() > 0
    sd = cases.make_sd("cart_mb11", prec)
    eng = engine.HipEngine(sd, slab_first=True, slab_last=True, readout_chunk=16)
    for k in (0, 1):
        eng.set_grid(k, init[k])
    N = [sd.Nx, sd.Ny, sd.Nz]
    for lo, hi, st, names in (([-1, 0, 0], N, [1, 1, 1], "lo[0]"), ([0, 0, 0], [N[0], N[1] + 1, N[2]], [1, 1, 1], "hi[1]"),
                              ([0, 0, 5], [N[0], N[1], 5], [1, 1, 1], "lo[2]"), ([0, 7, 0], [N[0], 3, N[2]], [1, 1, 1], "lo[1]"),
                              ([0, 0, 0], N, [1, 0, 1], "stride[1]"), ([0, 0, 0], N, [-2, 1, 1], "stride[0]")):
        with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:  # PF_ERR_ARG
            eng.get_region(1, lo, hi, st)
        assert ei.value.code == 1 and names in str(ei.value), str(ei.value)
    with pytest.raises(engine.PfError, match="pffdtd_hip error 1") as ei:
        eng.get_region(2, [0, 0, 0], N)
    assert "which" in str(ei.value)
    L = engine.lib()
    r = engine.PfRegion((ctypes.c_int64 * 3)(0, 0, 0), (ctypes.c_int64 * 3)(*N), (ctypes.c_int64 * 3)(1, 1, 1))
    buf = np.empty(N, dtype=np.float32)
    assert L.pf_engine_get_region(eng._h, 1, None, buf.ctypes.data_as(ctypes.c_void_p)) == 1 and b"null pf_region" in L.pf_last_error()
    assert L.pf_engine_get_region(eng._h, 1, ctypes.byref(r), None) == 1 and b"null host" in L.pf_last_error()
    assert L.pf_engine_get_region(None, 1, ctypes.byref(r), buf.ctypes.data_as(ctypes.c_void_p)) == 1
    assert L.pf_multi_get_region(None, 1, ctypes.byref(r), buf.ctypes.data_as(ctypes.c_void_p)) == 1
    assert L.pf_region_count(None, None) < 0
    counts = (ctypes.c_int64 * 3)()
    r2 = engine.PfRegion((ctypes.c_int64 * 3)(3, 1, 2), (ctypes.c_int64 * 3)(29, 27, 25), (ctypes.c_int64 * 3)(1, 2, 3))
    assert L.pf_region_count(ctypes.byref(r2), counts) == 26 * 13 * 8 and list(counts) == [26, 13, 8]
    # split-phase steps: refused inside one; between them it answers, and the receiver ring stays where it is
    for n in range(steps):
        eng.step_begin(n)
        if n == 2:
            with pytest.raises(engine.PfError, match="pffdtd_hip error 4") as ei:  # PF_ERR_STATE
                eng.get_region(1, [0, 0, 0], N)
            assert ei.value.code == 4
        eng.step_end(n)
    got = eng.get_region(1, [1, 1, 1], [N[0] - 1, N[1] - 1, N[2] - 1])
    assert np.array_equal(got, ref_u1[1:-1, 1:-1, 1:-1])
    assert not sd.u_out.any()  # five samples wait in the ring: get_region did not flush them
    eng.flush_outputs()
    assert np.array_equal(sd.u_out[:, :steps], ref.u_out[:, :steps])
    eng.close()
    # the energy diagnostic (the reference plots with it on): no checkpoint there, but regions
    sd2 = cases.make_sd("cart_mb11", "double")
    en = engine.HipEngine(sd2, energy=True)
    en.energy_cfg(sd2.h, sd2.c, sd2.Ts, sd2.DEF)
    en.run_energy(0, 9, np.zeros(sd2.Nt), np.zeros(sd2.Nt + 1), np.zeros(sd2.Nt + 1))
    g = en.get_grid(1)
    assert np.abs(g).max() > 0 and np.array_equal(en.get_region(1, [3, 1, 2], [26, 20, 22], [1, 2, 3]), g[3:26:1, 1:20:2, 2:22:3])
    en.close()
    # a one-rank cost model has no field of the scene
    sd3 = cases.make_sd("cart_mb11", "single")
    m = engine.HipMulti(sd3, [0, 0], only_slab=1)
    with pytest.raises(engine.PfError, match="pffdtd_hip error 4") as ei:
        m.get_region(1, [0, 0, 0], N)
    assert ei.value.code == 4 and "only_slab" in str(ei.value)
    m.close()


PAIRS_KW = dict(Nx=100, Ny=70, Nz=276, Nt=24, wall=3, Nm=1, Mb=3, src=[47, 30, 100], rcv=[[30, 25, 96], [66, 36, 110], [48, 35, 104], [47, 4, 101]])


@pytest.mark.parametrize("one_thread", [False, True], ids=["slab_threads", "one_thread"])
def test_a_chain_inside_a_pair_refuses_and_answers_a_step_later(tmp_path, one_thread):
    """slabs in blocked pairs after an odd run: u^{n+1} is not complete in memory, PF_ERR_STATE, the chain stays usable; one step later the pair has
    ended and the region is the oracle's.  A FieldWriter asked at the odd step takes its frame one step late and records where; the frame's cell
    at a receiver is that receiver's sample."""
    ref = sim_data.SimData.from_sim(synth.shoebox(**PAIRS_KW), "single")
    ref.scale_input()
    n_in = 9
    rng = np.random.default_rng(67)  # seeded random fields: every receiver is live from step 0
    init = [(rng.standard_normal((ref.Nx, ref.Ny, ref.Nz)) * 1e-2).astype(np.float32) for _ in range(2)]
    start = engine._state_arrays(ref)[0]
    start["u_prev"], start["u_cur"] = init
    e = oracle.Engine(ref)
    for k in (0, 1):
        e.grid(k)[...] = init[k]
    for n in range(ref.Nt):
        if n == n_in + 1:
            want = e.grid(1).copy()
        e.step(n)
    e.close()
    sd = sim_data.SimData.from_sim(synth.shoebox(**PAIRS_KW), "single", build_mask=False)
    sd.scale_input()
    flags = engine.PF_MULTI_FORCE_PAIRS | engine.PF_MULTI_NO_TRIPLES | (engine.PF_MULTI_ONE_THREAD if one_thread else 0)
    m = engine.HipMulti(sd, [0, 0], multi_flags=flags, air_variant=40, verify_exchange=2)
    assert m.slab(0)["steps_per_pass"] == 2 and m.slab(1)["steps_per_pass"] == 2
    m.load_state(start)
    m.run(0, n_in)
    box = ([1, 1, 1], [sd.Nx - 1, sd.Ny - 1, sd.Nz - 1], [3, 1, 5])
    with pytest.raises(engine.PfError, match="pffdtd_hip error 4") as ei:
        m.get_region(1, *box)
    assert ei.value.code == 4
    planes = fields.parse_planes("x=30,z=101", (sd.Nx, sd.Ny, sd.Nz))
    fw = fields.FieldWriter(tmp_path / "f.h5", sd, planes + [box], every=3, first=n_in)
    assert fw.due(n_in) and not fw.due(n_in + 1) and fw.next_step(n_in + 1) == n_in + 3
    n = fw.take(m, n_in)  # advances the one step itself
    assert n == n_in + 1
    assert np.array_equal(m.get_region(1, *box), want[_slices(box)])
    m.run(n, sd.Nt - n)
    assert np.array_equal(sd.u_out, ref.u_out)
    m.close()
    regions, steps, frames = fields.read(tmp_path / "f.h5")
    assert steps == [n] and regions.shape == (3, 9)
    assert np.array_equal(frames[(2, n)], want[_slices(box)].astype(np.float64) * sd.infac)
    assert np.array_equal(frames[(0, n)][0, 1:-1, 1:-1], want[30, 1:-1, 1:-1].astype(np.float64) * sd.infac)
    row = lambda x, y, z: [int(v) for v in sd.out_ixyz].index((x * sd.Ny + y) * sd.Nz + z)
    r0, r3 = row(30, 25, 96), row(47, 4, 101)
    assert frames[(0, n)][0, 25, 96] == sd.u_out[r0, n] * sd.infac and frames[(1, n)][47, 4, 0] == sd.u_out[r3, n] * sd.infac
    assert sd.u_out[r0, n] != 0 and sd.u_out[r3, n] != 0


# ---- 5. frames equal receivers ------------------------------------------------------------------------------------------------------------------
def test_frames_equal_receivers(tmp_path):
    """receivers of cart_outside at (24, 22, 20), (2, 23, 3), (12, 12, 12): the planes x = 24, y = 23 and z = 12 hold one each"""
    sd = cases.make_sd("cart_outside", "double")
    rcv = [(24, 22, 20), (2, 23, 3), (12, 12, 12)]
    rows = [[int(v) for v in sd.out_ixyz].index((x * sd.Ny + y) * sd.Nz + z) for x, y, z in rcv]
    eng = engine.HipEngine(sd)
    first, every = 2, 7
    fw = fields.FieldWriter(tmp_path / "f.h5", sd, fields.parse_planes("x=24,y=23,z=12", (sd.Nx, sd.Ny, sd.Nz)), every, first)
    n = 0
    while n < sd.Nt:
        k = min(fw.next_step(n + 1), sd.Nt) - n
        eng.run(n, k)
        n += k
        if fw.due(n):
            assert fw.take(eng, n) == n
    eng.close()
    ref = cases.make_sd("cart_outside", "double")
    oracle.run_sim(ref)
    assert np.array_equal(sd.u_out, ref.u_out)
    regions, steps, frames = fields.read(tmp_path / "f.h5")
    assert steps == list(range(first, sd.Nt, every))
    seen = 0
    for s in steps:
        for i, cell in ((0, (0, 22, 20)), (1, (2, 0, 3)), (2, (12, 12, 0))):  # the receiver's cell inside its plane (a frame keeps the region's three axes)
            assert frames[(i, s)][cell] == sd.u_out[rows[i], s] * sd.infac, (i, s)
            seen += sd.u_out[rows[i], s] != 0
    assert seen >= len(steps) // 2  # (the comparison is not one of zeros with zeros)


# ---- 6. the command line ----------------------------------------------------------------------------------------------------------------------
def _cli(folder, *args, env=None):
    r = subprocess.run([sys.executable, "-m", "pffdtd_amd.fdtd_main", "--precision", "single", *args], cwd=folder,
                       env={**os.environ, "PYTHONPATH": str(ROOT), **(env or {})}, capture_output=True, text=True, timeout=300)
    return r


def _oracle_frames(folder, steps):
    """the oracle's u^n of the folder's scene at `steps`, its receivers after rescale_output, infac"""
    sd = sim_data.SimData.from_folder(folder, "single")
    sd.scale_input()
    e = oracle.Engine(sd)
    out = {}
    for n in range(sd.Nt):
        if n in steps:
            out[n] = e.grid(1).copy()
        e.step(n)
    e.close()
    return out, (sd.u_out * sd.infac)[sd.out_reorder, :], sd.infac, (sd.Nx, sd.Ny, sd.Nz)


def _check_file(path, specs, want_steps, folder, shifted=False):
    """-> (the steps of the file's frames, the oracle's sim_outs rows)"""
    regions, steps, frames = fields.read(path)
    ref, ref_out, infac, N = _oracle_frames(folder, set(steps))
    assert [tuple(r) for r in regions] == [tuple(lo) + tuple(hi) + tuple(st) for lo, hi, st in specs]
    if shifted:  # a chain inside a pass takes a frame up to five steps late, never early, and says where
        assert len(steps) == len(want_steps) and all(w <= s <= w + 5 for s, w in zip(steps, want_steps)), (steps, want_steps)
    else:
        assert steps == want_steps, (steps, want_steps)
    inner = np.zeros(N, dtype=bool)
    inner[1:-1, 1:-1, 1:-1] = True
    for (i, s), f in frames.items():
        sl = _slices(specs[i])
        assert f.dtype == np.float64 and f.shape == ref[s][sl].shape
        assert np.array_equal(f[inner[sl]], (ref[s][sl].astype(np.float64) * infac)[inner[sl]]), (i, s)
    assert sum(any(np.abs(f).max() > 0 for (i, _), f in frames.items() if i == k) for k in range(len(specs))) >= 2  # (not zeros against zeros; a ghost plane or a far corner may stay 0)
    return steps, ref_out


def test_cli_frames_stop_and_resume(tmp_path):
    sim = synth.sort_sim(cases.make_sim("cart_mb11"))
    plain, whole, parts = tmp_path / "plain", tmp_path / "whole", tmp_path / "parts"
    for d in (plain, whole, parts):
        d.mkdir()
        synth.write_folder(sim, d)
    _, ref_out, _, N = _oracle_frames(plain, set())
    r = _cli(plain)
    assert r.returncode == 0, r.stderr[-2000:]
    assert not (plain / "sim_fields.h5").exists() and "field frame" not in r.stdout
    assert np.array_equal(h5io.read(plain / "sim_outs.h5", "u_out"), ref_out)  # without the arguments: the run every earlier version gives
    args = ("--field-planes", "x=13,y=0,z=21", "--field-box", "3:26:1,1:20:2,2:22:3", "--field-every", "6")
    specs = fields.parse_planes("x=13,y=0,z=21", N) + [fields.parse_box("3:26:1,1:20:2,2:22:3", N)]
    r = _cli(whole, *args)
    assert r.returncode == 0, r.stderr[-2000:]
    assert h5io.read(whole / "sim_outs.h5", "u_out").tobytes() == h5io.read(plain / "sim_outs.h5", "u_out").tobytes()
    steps, _ = _check_file(whole / "sim_fields.h5", specs, list(range(0, 80, 6)), whole)
    r = _cli(parts, *args, "--stop-after", str(STOP), "--checkpoint", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert fields.read(parts / "sim_fields.h5")[1] == [s for s in steps if s <= STOP]  # a stopped run keeps its frames
    r = _cli(parts, *args, "--resume", "ck.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert h5io.read(parts / "sim_outs.h5", "u_out").tobytes() == h5io.read(whole / "sim_outs.h5", "u_out").tobytes()
    a, b = fields.read(whole / "sim_fields.h5"), fields.read(parts / "sim_fields.h5")
    assert a[1] == b[1] and all(a[2][k].tobytes() == b[2][k].tobytes() for k in a[2])


@pytest.mark.parametrize("scene", ["two_slabs_cut_along_z", "chain_in_pairs"])
def test_cli_frames_of_a_chain_every_five_steps(tmp_path, scene):
    if scene == "chain_in_pairs":  # two slabs of 100 planes: blocked passes, frames may shift
        sim = synth.shoebox(200, 70, 276, Nt=24, wall=3, Nm=1, Mb=3, src=[97, 30, 100], rcv=[[30, 25, 96], [166, 36, 110]])
        extra, box, planes, nt = ("--devices", "0,0"), "1:199:3,2:68:1,1:275:5", "x=99,x=100,z=101", 24
    else:
        sim, extra, box, planes, nt = _plates_room(), (), "3:29:1,1:27:2,2:25:3", "x=100,y=38,z=31,z=32", 48
    synth.write_folder(sim, tmp_path)
    r = _cli(tmp_path, *extra, "--field-planes", planes, "--field-box", box, "--field-every", "5", "--field-first", "3", "--field-file", "frames.h5")
    assert r.returncode == 0, r.stderr[-2000:]
    assert ("--2 slabs on devices [0, 0], cut along file x" if scene == "chain_in_pairs" else "--2 slabs on device 0, cut along file z") in r.stdout, r.stdout[:1500]
    N = tuple(int(h5io.read(tmp_path / "vox_out.h5", k)) for k in ("Nx", "Ny", "Nz"))
    specs = fields.parse_planes(planes, N) + [fields.parse_box(box, N)]
    steps, ref_out = _check_file(tmp_path / "frames.h5", specs, list(range(3, nt, 5)), tmp_path, shifted=scene == "chain_in_pairs")
    assert np.array_equal(h5io.read(tmp_path / "sim_outs.h5", "u_out"), ref_out)
    print(scene, "frames at steps", steps)
    assert all(f"--field frame at step {s} of {nt}" in r.stdout for s in steps)
