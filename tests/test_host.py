"""Host logic that needs no GPU: loader checks, ABC list, file I/O, the C-ABI library's exports, slab partition."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import cases
from pffdtd_amd import engine, h5io, sim_data, slab, synth

ROOT = Path(__file__).resolve().parent.parent


def test_library_exports_every_declared_symbol():
    """libpffdtd_hip.so must load on a CPU-only box and export everything include/*.h declares."""
    from pffdtd_amd import voxelizer
    L = ctypes.CDLL(str(engine.lib_path()))
    for header, exports, nmin in (("pffdtd_hip.h", engine.EXPORTS, 18), ("pffdtd_vox.h", voxelizer.EXPORTS, 5)):
        hdr = (ROOT / "include" / header).read_text()
        declared = set(re.findall(r"\b(pf_[a-z_0-9]+)\s*\(", hdr))
        assert len(declared) >= nmin
        missing = [s for s in sorted(declared) if not hasattr(L, s)]
        assert not missing, missing
        assert set(exports) == declared
    # the development / test switches are no part of the boundary: their hook is exported but declared in csrc/pf_debug.h only, and
    # pf_opts holds no such field
    hdr = (ROOT / "include" / "pffdtd_hip.h").read_text()
    for name in engine.INTERNAL_EXPORTS:
        assert hasattr(L, name) and name not in hdr
    assert not re.search(r"\b(debug|test_[a-z_]+);", hdr)
    assert len(engine.PfOpts._fields_) <= 20


def test_native_rccl_entry_points_refuse_bad_arguments_without_touching_a_device():
    """pf_rccl_* (one process per device): argument errors come back as PF_ERR_ARG with a message, before librccl or a device is needed."""
    L = engine.lib()
    comm = ctypes.c_void_p()
    assert L.pf_rccl_unique_id(None) == 1 and b"null" in L.pf_last_error()
    assert L.pf_rccl_comm_create(None, 2, 0, 0, ctypes.byref(comm)) == 1 and not comm.value
    assert L.pf_rccl_comm_create(b"\0" * 128, 2, 2, 0, ctypes.byref(comm)) == 1 and not comm.value  # rank outside [0, nranks)
    assert L.pf_rccl_exchange(None, None, -1, -1) == 1
    L.pf_rccl_comm_destroy(None)  # (a null communicator: nothing to do)


def test_struct_layout_matches_header():
    """ctypes mirror of pf_simdata: same size as the C struct (checked through a tiny compiled probe)."""
    import subprocess
    import tempfile
    src = '#include <stdio.h>\n#include "pffdtd_hip.h"\nint main(){printf("%zu %zu %zu %zu", sizeof(pf_simdata), sizeof(pf_opts), sizeof(pf_timing), sizeof(pf_multi_info));}'
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "p.c"
        c.write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(Path(d) / "p")], check=True)
        out = subprocess.run([str(Path(d) / "p")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(sim_data.PfSimData)
    assert int(out[1]) == ctypes.sizeof(engine.PfOpts)
    assert int(out[2]) == ctypes.sizeof(engine.PfTiming)
    assert int(out[3]) == ctypes.sizeof(engine.PfMultiInfo)


def test_no_device_is_an_error_not_a_fallback():
    if engine.device_count() > 0:
        pytest.skip("a GPU is visible")
    sd = cases.make_sd("cart_rigid", "double")
    with pytest.raises(engine.PfError, match="no HIP device"):
        engine.HipEngine(sd)
    with pytest.raises(engine.PfError):
        engine.run_sim(sd)


@pytest.mark.parametrize("dims,flag", [((12, 10, 9), 0), ((10, 12, 14), 1), ((10, 8, 14), 2)])
def test_abc_list_against_bruteforce(dims, flag):
    """abc_nodes == the triple loop of fdtd_data.h:621-675."""
    Nx, Ny, Nz = dims
    Nyf = 2 * (Ny - 1) if flag == 2 else Ny
    idx, Q = [], []
    for ix in range(1, Nx - 1):
        for iy in range(1, Nyf - 1):
            for iz in range(1, Nz - 1):
                if flag > 0 and (ix + iy + iz) % 2 == 1:
                    continue
                q = int(ix in (1, Nx - 2)) + int(iy in (1, Nyf - 2)) + int(iz in (1, Nz - 2))
                if q:
                    y = Nyf - iy - 1 if (flag == 2 and iy >= Nyf // 2) else iy
                    idx.append(ix * Nz * Ny + y * Nz + iz)
                    Q.append(q)
    idx, Q = np.array(idx), np.array(Q)
    if flag == 2:
        o = np.argsort(idx, kind="stable")
        idx, Q = idx[o], Q[o]
    bna, Qb = sim_data.abc_nodes(Nx, Ny, Nz, flag)
    assert np.array_equal(bna, idx) and np.array_equal(Qb, Q)
    if flag == 2:
        assert np.unique(bna).size == bna.size


def test_loader_rejects_what_the_reference_asserts():
    sim = cases.make_sim("cart_lossy")
    bad = {k: dict(v) for k, v in sim.items()}
    bad["sim_consts"]["l2"] = np.float64(0.5)  # CFL: fdtd_data.h:180
    with pytest.raises(ValueError, match="CFL"):
        sim_data.SimData.from_sim(bad)
    bad = {k: dict(v) for k, v in sim.items()}
    bad["comms_out"]["diff"] = np.int8(0)  # single precision needs a differentiated input: fdtd_data.h:392
    with pytest.raises(ValueError, match="single precision"):
        sim_data.SimData.from_sim(bad, "single")
    sim_data.SimData.from_sim(bad, "double")
    bad = {k: dict(v) for k, v in sim.items()}
    bad["vox_out"]["bn_ixyz"] = bad["vox_out"]["bn_ixyz"].copy()
    bad["vox_out"]["bn_ixyz"][0] = 0  # fdtd_data.h:510
    with pytest.raises(ValueError, match="interior"):
        sim_data.SimData.from_sim(bad)
    bad = {k: dict(v) for k, v in sim.items()}
    bad["sim_mats"]["Mb"] = np.array([13, 3], dtype=np.int8)  # > MMb
    with pytest.raises(ValueError):
        sim_data.SimData.from_sim(bad)


def test_scale_input_matches_reference_formula():
    sd = cases.make_sd("cart_lossy", "single", scale=False)
    m = np.abs(sd.in_sigs).max()
    infac = sd.scale_input()
    assert infac == 1.0 / (4.0 / m)  # norm1 = 2^2, infac = 1/inv_infac: fdtd_data.h:891-896
    assert np.abs(sd.in_sigs).max() == pytest.approx(4.0, rel=1e-15)


def test_h5_folder_roundtrip(tmp_path):
    sim = cases.make_sim("fcc2_lossy")
    synth.write_folder(sim, tmp_path, gzip=3)
    back = synth.read_folder(tmp_path)
    for f in sim:
        for k, v in sim[f].items():
            if k in back[f]:
                assert np.array_equal(np.asarray(v), np.asarray(back[f][k])), (f, k)
    assert back["vox_out"]["adj_bn"].dtype == np.bool_  # h5py-style enum
    assert np.ndim(back["vox_out"]["Nx"]) == 0          # rank-0 scalars, as the reference asserts (fdtd_data.h:830)
    with pytest.raises(FileNotFoundError):
        synth.read_folder(tmp_path / "nope")


def test_partition_rule():
    """The reference's even split (gpu_engine.h:532-550), from the library's one implementation of the cut."""
    import copy
    sd = copy.copy(cases.make_sd("cart_lossy", "single"))
    sd.Nx = 10  # (the even rule looks at the plane count only)
    assert slab.partition(sd, 3) == [(0, 4), (4, 7), (7, 10)]  # remainder to the first ranks
    sd.Nx = 1024
    assert slab.partition(sd, 8)[3] == (384, 512)
    sd.Nx = 4
    with pytest.raises(ValueError):
        slab.partition(sd, 4)  # assert(ngpus < Nx), gpu_engine.h:682


@pytest.mark.parametrize("G", [2, 3])
def test_split_covers_every_list_entry_once(G):
    sd = cases.make_sd("cart_outside", "double")
    seen = {k: 0 for k in ("Nb", "Nbl", "Nba", "Ns")}
    rows = []
    for r in range(G):
        loc, info = slab.split(sd, G, r)
        for k in seen:
            seen[k] += getattr(loc, k)
        rows += loc.out_rows.tolist()
        assert loc.Nx == info.Nxh and loc.Npts == loc.Nx * loc.Ny * loc.Nz
        for arr in (loc.bn_ixyz, loc.bnl_ixyz, loc.bna_ixyz, loc.in_ixyz):
            ix = arr // (loc.Ny * loc.Nz)
            assert ((ix >= 1) & (ix <= loc.Nx - 2)).all()  # everything a slab updates is interior to it
    assert seen == {k: getattr(sd, k) for k in seen}
    assert sorted(rows) == list(range(sd.Nr))


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("balance", [False, True])
def test_split_along_file_z_covers_every_list_entry_once(G, balance):
    """chains cut along FILE Z (rooms: the slab engines store the x and z axes exchanged): every list entry lands in exactly one
    slab, interior to it along z, and maps back to its global index"""
    sd = cases.make_sd("cart_outside", "double")
    seen = {k: 0 for k in ("Nb", "Nbl", "Nba", "Ns")}
    rows, back = [], []
    for r in range(G):
        loc, info = slab.split(sd, G, r, balance=balance, along_z=True)
        assert info.along_z and loc.Nx == sd.Nx and loc.Nz == info.Nxh and loc.Npts == loc.Nx * loc.Ny * loc.Nz
        for k in seen:
            seen[k] += getattr(loc, k)
        rows += loc.out_rows.tolist()
        for arr in (loc.bn_ixyz, loc.bnl_ixyz, loc.bna_ixyz, loc.in_ixyz):
            iz = arr % loc.Nz
            assert ((iz >= 1) & (iz <= loc.Nz - 2)).all()  # everything a slab updates is interior to it along z
        back.append((loc.bn_ixyz // loc.Nz) * sd.Nz + loc.bn_ixyz % loc.Nz + info.xlo)
    assert seen == {k: getattr(sd, k) for k in seen}
    assert sorted(rows) == list(range(sd.Nr))
    assert np.array_equal(np.sort(np.concatenate(back)), np.sort(sd.bn_ixyz))


def test_weighted_partition_covers_and_balances():
    sd = cases.make_sd("cart_lossy", "double")
    for G in (2, 3, 5):
        parts = slab.partition_weighted(sd, G)
        assert parts[0][0] == 0 and parts[-1][1] == sd.Nx
        assert all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
        assert all(x1 - x0 >= 2 for x0, x1 in parts)
    # a scene whose only boundary nodes are two whole wall planes near the ends: the end slabs must get fewer planes
    import copy
    big = copy.copy(sd)
    big.Nx, big.Ny, big.Nz = 200, 32, 32
    NzNy = big.Ny * big.Nz
    big.bn_ixyz = np.concatenate([3 * NzNy + np.arange(NzNy), 196 * NzNy + np.arange(NzNy)])
    big.bnl_ixyz, big.Nbl = big.bn_ixyz, big.bn_ixyz.size
    big.Nb, big.Npts = big.bn_ixyz.size, 200 * NzNy
    big.adj_bn = np.zeros(big.Nb, dtype=sd.adj_bn.dtype)
    big.in_ixyz = np.array([100 * NzNy + 5], dtype=np.int64)
    big.in_sigs = np.zeros((1, sd.Nt))
    big.Ns = 1
    big.mat_bnl = np.zeros(big.Nbl, dtype=np.int8)
    big.Mb = np.array([11], dtype=np.int8)
    p4 = slab.partition_weighted(big, 4)
    sizes = [b - a for a, b in p4]
    assert sizes[0] < sizes[1] and sizes[3] < sizes[2] and sum(sizes) == 200
    # and the balanced split is still a valid decomposition
    seen = 0
    for r in range(3):
        loc, info = slab.split(sd, 3, r, balance=True)
        seen += loc.Nb
    assert seen == sd.Nb


@pytest.mark.parametrize("name", ["cart_lossy", "cart_outside", "fcc2_outside", "cart_mb11"])
def test_the_librarys_cut_is_the_only_one(name):
    """pf_slab_partition_axis (no device needed) is what the C chain AND pffdtd_amd.slab cut with: both rules, both axes, and the
    properties the balanced cut promises -- a decomposition, no cut within eight planes of a source, costs within a few planes of equal
    between the cuts that no source pushed aside."""
    sd = cases.make_sd(name, "single")
    for G in (1, 2, 3, 5):
        base, rem = divmod(sd.Nx, G)
        sizes = [base + (1 if g < rem else 0) for g in range(G)]  # gpu_engine.h:532-550
        assert [b - a for a, b in engine.slab_partition(sd, G, even=True)] == sizes
        assert slab.partition(sd, G) == engine.slab_partition(sd, G, even=True)
        for az in (False, True):
            n = sd.Nz if az else sd.Nx
            if G >= n // 2:
                continue
            for k in (1.0, 0.4, 2.5):  # (the factor the library measures at creation, round 5)
                parts = slab.partition_weighted(sd, G, az, k)
                assert parts == engine.slab_partition(sd, G, even=False, wall_scale=k, along_z=az)
                assert parts[0][0] == 0 and parts[-1][1] == n and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
                assert all(x1 - x0 >= 2 for x0, x1 in parts)
    with pytest.raises(engine.PfError):
        engine.slab_partition(sd, sd.Nx)  # gpu_engine.h:682


def test_a_cut_pushed_aside_by_a_source_does_not_leave_a_thick_rank():
    """Round 6: the headline scene's source sits at Nx / 2, exactly where an even number of ranks cuts; the cut keeps eight planes from it,
    and the ranks on either side share their part of the planes equally (before: 125 and 142 planes side by side at 1024 planes / 8 ranks)."""
    import copy
    sd = copy.copy(cases.make_sd("cart_lossy", "single"))
    sd.Nx, sd.Ny, sd.Nz = 1024, 8, 8
    per = sd.Ny * sd.Nz
    sd.Npts = sd.Nx * per
    sd.Nb = sd.Nbl = sd.Nba = 0
    sd.bn_ixyz = sd.bnl_ixyz = sd.bna_ixyz = np.zeros(0, dtype=np.int64)
    sd.adj_bn = sd.adj_bn[:0]; sd.K_bn = sd.K_bn[:0]; sd.mat_bnl = sd.mat_bnl[:0]; sd.ssaf_bnl = sd.ssaf_bnl[:0]; sd.Q_bna = sd.Q_bna[:0]
    sd.in_ixyz = np.array([512 * per + 9], dtype=np.int64)
    sd.in_sigs = np.zeros((1, sd.Nt)); sd.Ns = 1
    sd.out_ixyz = np.array([100 * per + 9], dtype=np.int64); sd.out_reorder = np.zeros(1, dtype=np.int64); sd.Nr = 1
    parts = slab.partition_weighted(sd, 8)
    cuts = [a for a, _ in parts[1:]]
    assert all(not (512 - 8 < x <= 512 + 8) for x in cuts), cuts
    sizes = [b - a for a, b in parts]
    assert max(sizes) - min(sizes) <= 6 and max(sizes) <= 131, sizes


def test_the_c_chains_cut_under_sanitizers(tmp_path):
    """csrc/pf_slab_cut.h -- what pf_multi_create cuts a scene with -- has no device in it: tests/slab_cut_check.cpp drives it on a small
    unsorted scene (G = 2, 3, 5, both axes, both split rules, fp32 and fp64) and on scenes whose sources leave the split no plane clear of
    them, or few (a source in every plane, on every 6th, a band of 66; G = 2, 3, 8), as a program of its own, built with the host compiler
    under the address and undefined-behaviour sanitizers; it names every violated condition on stderr."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "slab_cut_check"
    subprocess.run([cxx, "-std=c++17", "-O0", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "include"), "-I", str(ROOT / "pffdtd_amd" / "csrc"), str(ROOT / "tests" / "slab_cut_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
