"""CPU: the host side of the directional band maps on FCC grids (pffdtd_amd/directional.py, stencil="lattice"): the gradient's section for a
difference that spans eight cells, the lattice difference of a plane wave against i k_a p with a bound derived here, the fold's coordinates against
synth.fold_fcc, the file of a folded grid (stencil, fcc_flag, the physical rows, the sign of S in the mirrored cells) and every refusal of a resume
-- with a vector band accumulator object that folds in numpy, no device."""
import types

import numpy as np
import pytest
from scipy.signal import butter

from pffdtd_amd import directional, synth
from test_directional_host import C, H, TS, FakeVBand, _run, _section

# the + offsets o0 .. o3 of the lattice differences 4 / 5 / 6 (include/pffdtd_hip.h), in the order of synth.FCC_OFFS
LAT_OFFS = {4: [(1, 1, 0), (1, 0, 1), (1, -1, 0), (1, 0, -1)], 5: [(1, 1, 0), (0, 1, 1), (-1, 1, 0), (0, 1, -1)], 6: [(0, 1, 1), (1, 0, 1), (0, -1, 1), (-1, 0, 1)]}
NF = (6, 5, 7)  # a folded grid: Ny = 5 stored rows, a room of 8
REGIONS_F = [((1, 1, 3), (5, 4, 4), (1, 1, 1)), ((1, 1, 1), (5, 4, 6), (2, 2, 3))]


def _sd(Nt=40, fcc_flag=2, n=NF):
    return types.SimpleNamespace(Nt=Nt, Ts=TS, infac=0.37, Nx=n[0], Ny=n[1], Nz=n[2], diff=True, h=H, c=C, fcc_flag=fcc_flag)


def lattice(u, lo, hi, st, comp):
    """the contract's numpy restatement: L_a over the region of the whole grid u, in u's dtype, the association of include/pffdtd_hip.h"""
    def at(o, sign):
        return u[tuple(slice(lo[a] + sign * o[a], hi[a] + sign * o[a], st[a]) for a in range(3))]
    d = [at(o, 1) - at(o, -1) for o in LAT_OFFS[comp]]
    return (d[0] + d[1]) + (d[2] + d[3])


class LatVBand(FakeVBand):
    """FakeVBand whose components 4 / 5 / 6 are the lattice differences: its add with the component's line changed"""

    def add(self, bin):
        u = self.field()
        npre, nsec = self.pre.shape[1], self.bands.shape[1]
        xs = []
        for c, k in enumerate(self.comp):
            x = u[self._sl(-1, 0)] if k == 0 else lattice(u, self.lo, self.hi, self.st, k)
            assert x.dtype == u.dtype
            x = x.astype(np.float64)
            for q in range(npre):
                x = _section(self.pre[c, q], self.state[c, q], x)
            xs.append(x)
        for b in range(self.bands.shape[0]):
            ys = []
            for c, x in enumerate(xs):
                for s in range(nsec):
                    x = _section(self.bands[b, s], self.state[c, npre + b * nsec + s], x)
                ys.append(x)
            if bin >= 0:
                for p, (i, j, mode) in enumerate(self.prod):
                    self.S[p, b, bin] = self.S[p, b, bin] + (np.fabs(ys[i] * ys[j]) if mode else ys[i] * ys[j])
        self.count += 1


class LatEngine:
    """u^n = a seeded random field per step"""

    def __init__(self, n=NF):
        self.n, self.N = 0, n

    def field(self):
        return np.random.default_rng(3000 + self.n).standard_normal(self.N).astype(np.float32)

    def vector_band_accumulator(self, lo, hi, stride=(1, 1, 1), comp=(0,), pre_sos=None, band_sos=None, prod=((0, 0, 0),), nbin=1, depth=0):
        return LatVBand(lo, hi, stride, comp, pre_sos, band_sos, prod, nbin, self.field)


class AxisEngine(LatEngine):
    """the same fields with central differences (a Cartesian scene of this size)"""

    def vector_band_accumulator(self, lo, hi, stride=(1, 1, 1), comp=(0,), pre_sos=None, band_sos=None, prod=((0, 0, 0),), nbin=1, depth=0):
        return FakeVBand(lo, hi, stride, comp, pre_sos, band_sos, prod, nbin, self.field)


def test_fake_lattice_band_is_the_contract():
    """the numpy accumulator of this file, without sections: the products of the cell and of L_y"""
    eng = LatEngine()
    lo, hi, st = REGIONS_F[1]
    a = eng.vector_band_accumulator(lo, hi, st, comp=(0, 5), pre_sos=np.zeros((2, 0, 6)), band_sos=np.zeros((1, 0, 6)), prod=[(0, 1, 0), (1, 1, 0)], nbin=1)
    u = eng.field()
    a.add(0)
    c0 = u[tuple(slice(lo[k], hi[k], st[k]) for k in range(3))].astype(np.float64)
    L = lattice(u, lo, hi, st, 5).astype(np.float64)
    assert np.array_equal(a.S[0, 0, 0], c0 * L) and np.array_equal(a.S[1, 0, 0], L * L) and a.count == 1 and L.any()


def test_gradient_sections_span():
    for diff in (True, False):
        old = directional.gradient_sections(TS, H, C, diff, 10.0, 4)
        two = directional.gradient_sections(TS, H, C, diff, 10.0, 4, span=2)
        assert np.array_equal(old[0], two[0]) and np.array_equal(old[1], two[1])
        b, a = butter(1, 2 * TS * 10.0, btype="high")
        g2 = -(C / (2 * H)) * (TS / 2) * b[0]  # today's expression, to the bit
        assert np.array_equal(two[1][-1], [g2, g2, 0.0, 1.0, a[1], 0.0])
        omni, grad = directional.gradient_sections(TS, H, C, diff, 10.0, 4, span=8)
        g8 = -(C / (8.0 * H)) * (TS / 2.0) * float(b[0])
        assert np.array_equal(omni, old[0]) and np.array_equal(grad[:-1], old[1][:-1])
        assert np.array_equal(grad[-1], [g8, g8, 0.0, 1.0, a[1], 0.0]) and g8 < 0
        assert abs(grad[-1][0] * 4 - g2) <= 4 * np.finfo(float).eps * abs(g2)  # a quarter of the central difference's gain
    assert directional.LATTICE_SPAN == 8


@pytest.mark.parametrize("h", [H, C * TS], ids=["h_cart_limit", "h_fcc_limit"])
@pytest.mark.parametrize("f", [125.0, 1000.0])
@pytest.mark.parametrize("deg", [0.0, 60.0, 90.0, 180.0])
def test_a_plane_wave_gives_i_k_p(f, deg, h):
    """p = exp(i k.x) sampled analytically on the twelve neighbours of the origin (p(0) = 1), k at `deg` to the axis in two planes through it.
    A pair gives u[+o] - u[-o] = 2 i sin(x_m), x_m = h k.o_m, and the four x_m of a component sum to h k.(4 e_a) = 4 h k_a, so
        L_a / (8 h) - i k_a = (i / (4 h)) sum_m (sin x_m - x_m),     |sin x - x| <= |x|^3 / 6:
        |L_a / (8 h) - i k_a p| <= sum_m |x_m|^3 / (24 h)
    plus the rounding of this test's own double arithmetic: 12 values of modulus 1, 7 operations on values of modulus <= 8, each rounded to
    2^-53 relative -- below 64 * 2^-53 absolute in L_a, i.e. 8 * 2^-53 / h after the division."""
    kabs = 2 * np.pi * f / C
    th = np.deg2rad(deg)
    cos_t, sin_t = (np.cos(th) if deg != 90.0 else 0.0), np.sin(th)
    for comp in (4, 5, 6):
        a = comp - 4
        for other in ([(a + 1) % 3], [(a + 1) % 3, (a + 2) % 3]):  # the transverse part along one axis, and along the diagonal of the two
            k = np.zeros(3)
            k[a] = kabs * cos_t
            for b in other:
                k[b] = kabs * sin_t / np.sqrt(len(other))
            d = [np.exp(1j * h * np.dot(k, o)) - np.exp(-1j * h * np.dot(k, o)) for o in LAT_OFFS[comp]]
            L = (d[0] + d[1]) + (d[2] + d[3])
            x = np.array([h * np.dot(k, o) for o in LAT_OFFS[comp]])
            assert abs(x.sum() - 4 * h * k[a]) <= 8 * np.finfo(float).eps * np.abs(x).sum()
            bound = (np.abs(x) ** 3).sum() / (24 * h) + 8 * 2.0 ** -53 / h
            err = abs(L / (8 * h) - 1j * k[a])
            print(f"comp {comp}, f {f:g} Hz, theta {deg:g}, transverse {other}: L / 8h = {L / (8 * h):.9g}, i k_a = {1j * k[a]:.9g}, error {err:.3e}, bound {bound:.3e}")
            assert err <= bound
            assert bound <= 0.05 * kabs  # (the bound says something: a twentieth of |k| at most at these wavelengths)


def test_fold_coordinates_against_fold_fcc():
    Nx, Ny, Nz = 24, 22, 20  # the room (the size of the parity case fcc1_lossy); folded: 12 stored rows
    sim = synth.shoebox(Nx, Ny, Nz, Nt=4, fcc=True, Nm=1, Mb=2)
    ix, iy, iz = np.meshgrid(np.arange(Nx), np.arange(Ny), np.arange(Nz), indexing="ij")
    nodes = ((ix + iy + iz) % 2 == 0)
    node_list = ((ix * Ny + iy) * Nz + iz)[nodes].astype(np.int64)  # every node of the checkerboard
    sim["comms_out"]["out_ixyz"] = node_list.copy()
    synth.fold_fcc(sim)
    Nyf = int(sim["vox_out"]["Ny"])
    assert Nyf == Ny // 2 + 1 and int(sim["sim_consts"]["fcc_flag"]) == 2
    stored = np.asarray(sim["comms_out"]["out_ixyz"])
    fx, fy, fz, upper = directional.fold_coordinates(((0, 0, 0), (Nx, Nyf, Nz), (1, 1, 1)), Nyf)
    assert fx.shape == (Nx, Nyf, Nz) and fy.dtype == np.int64 and upper.dtype == bool
    back = ((fx * Ny + fy) * Nz + fz).reshape(-1)  # the node every stored cell says it holds
    assert np.array_equal(back[stored], node_list)  # ... is the node that was folded onto it
    assert np.array_equal(upper.reshape(-1)[stored], (node_list // Nz) % Ny >= Ny // 2)
    own = np.ones((Nx, Nyf, Nz), dtype=bool)
    own[:, Nyf - 1, :] = False
    assert np.array_equal(np.sort(stored), np.flatnonzero(own.reshape(-1)))  # every cell of rows 0 .. Ny - 2, once
    assert np.all(fy[:, Nyf - 1, :] == -1) and np.all(fy[:, :Nyf - 1, :] >= 0)  # the fold's ghost row is flagged
    # a strided region is the same table, cut
    r = ((1, 2, 0), (23, 12, 19), (2, 3, 4))
    sx, sy, sz, su = directional.fold_coordinates(r, Nyf)
    sl = tuple(slice(r[0][a], r[1][a], r[2][a]) for a in range(3))
    assert np.array_equal(sx, fx[sl]) and np.array_equal(sy, fy[sl]) and np.array_equal(sz, fz[sl]) and np.array_equal(su, upper[sl])


def test_file_of_a_folded_grid_and_resume(tmp_path):
    sd = _sd()
    kw = dict(bands_hz=[500.0, 1000.0], axes=[2, 3], bin_ms=0.4, first=3, stencil="lattice")
    whole = directional.FieldDirectional(tmp_path / "whole.h5", sd, REGIONS_F, **kw)
    assert whole.comp.tolist() == [0, 5, 6] and whole.axes.tolist() == [2, 3]
    assert np.array_equal(whole.pre_sos[1], directional.gradient_sections(TS, H, C, True, 10.0, 4, span=8)[1])
    _run(whole, LatEngine(), 0, 40)
    whole.write()
    w = directional.read(tmp_path / "whole.h5", raw=True)
    assert w["stencil"] == "lattice" and w["fcc_flag"] == 2 and list(w["axes"]) == [2, 3] and list(w["sampling"]) == [3, 10, 37]
    prod = [tuple(p) for p in w["prod"].tolist()]
    assert prod == [(0, 0, 0), (1, 1, 0), (0, 1, 0), (0, 1, 1), (2, 2, 0), (0, 2, 0), (0, 2, 1)]
    k2 = 0.37 * 0.37
    for i, r in enumerate(REGIONS_F):
        _, iy, _, upper = directional.fold_coordinates(r, NF[1])
        assert np.array_equal(w["iy"][i], iy) and w["iy"][i].shape == whole.accs[i].shape[3:] and upper.any() and not upper.all()
        sums, S = w["sums"][i], w["S"][i]
        assert np.array_equal(sums, whole.accs[i].get()[0])  # the raw sums stay in storage form
        for p, row in enumerate(prod):
            if row == (0, 1, 0):  # the one product with an odd number of y factors and mode 0: the room's sign in the mirrored cells
                assert np.array_equal(S[p][..., upper], -(sums[p][..., upper] * k2)) and np.array_equal(S[p][..., ~upper], sums[p][..., ~upper] * k2)
                assert np.abs(S[p][..., upper]).max() > 0
            else:
                assert np.array_equal(S[p], sums[p] * k2), row
    # a checkerboard (flag 1) has no fold: no rows, no sign
    flat = directional.FieldDirectional(tmp_path / "flat.h5", _sd(fcc_flag=1), REGIONS_F, **kw)
    _run(flat, LatEngine(), 0, 40)
    flat.write()
    f1 = directional.read(tmp_path / "flat.h5", raw=True)
    assert f1["stencil"] == "lattice" and f1["fcc_flag"] == 1 and "iy" not in f1
    assert all(np.array_equal(f1["S"][i], f1["sums"][i] * k2) and np.array_equal(f1["sums"][i], w["sums"][i]) for i in range(2))
    # a run stopped at step 17 and resumed: bit for bit
    path = tmp_path / "dir.h5"
    a = directional.FieldDirectional(path, sd, REGIONS_F, **kw)
    _run(a, LatEngine(), 0, 17)
    a.write()
    b = directional.FieldDirectional(path, sd, REGIONS_F, resume_at=17, **kw)
    assert b.count == 14
    eng = LatEngine()
    b.attach(eng)
    _run(b, eng, 17, 40)
    b.write()
    r = directional.read(path, raw=True)
    for key in ("S", "sums", "state", "iy"):
        for i in range(2):
            assert np.array_equal(r[key][i], w[key][i]), (key, i)
    # every refusal of a resume
    a = directional.FieldDirectional(path, sd, REGIONS_F, **kw)
    _run(a, LatEngine(), 0, 17)
    a.write()
    for field, sd2, regions, k2_ in (("regions", sd, REGIONS_F[:1], kw), ("bands", sd, REGIONS_F, {**kw, "bands_hz": [500.0]}), ("axes", sd, REGIONS_F, {**kw, "axes": [3, 2]}),
                                     ("first", sd, REGIONS_F, {**kw, "first": 2}), ("bin_steps", sd, REGIONS_F, {**kw, "bin_ms": 0.8}),
                                     ("pre_sos", sd, REGIONS_F, {**kw, "lowcut_hz": 20.0}), ("band_sos", sd, REGIONS_F, {**kw, "order": 2}),
                                     ("Ts", types.SimpleNamespace(**{**vars(sd), "Ts": TS * 1.0000001}), REGIONS_F, kw)):
        with pytest.raises(ValueError, match=field):
            directional.FieldDirectional(path, sd2, regions, resume_at=17, **k2_)
    with pytest.raises(ValueError, match="count"):
        directional.FieldDirectional(path, sd, REGIONS_F, resume_at=18, **kw)
    with pytest.raises(ValueError, match="no directional file"):
        directional.FieldDirectional(tmp_path / "none.h5", sd, REGIONS_F, resume_at=17, **kw)
    # a changed stencil: the same regions, bands and axes on a Cartesian scene with stencil="axis"
    with pytest.raises(ValueError, match="stencil"):
        directional.FieldDirectional(path, _sd(fcc_flag=0), REGIONS_F, resume_at=17, **{**kw, "stencil": "axis"})
    # ... and a file of stencil="axis" asked to continue as "lattice"
    cart = directional.FieldDirectional(tmp_path / "cart.h5", _sd(fcc_flag=0), REGIONS_F, **{**kw, "stencil": "axis"})
    _run(cart, AxisEngine(), 0, 17)
    cart.write()
    c = directional.read(tmp_path / "cart.h5")
    assert c["stencil"] == "axis" and c["fcc_flag"] == 0 and "iy" not in c
    with pytest.raises(ValueError, match="stencil"):
        directional.FieldDirectional(tmp_path / "cart.h5", sd, REGIONS_F, resume_at=17, **kw)


def test_new_refusals_of_field_directional():
    kw = dict(bands_hz=[500.0], axes=[2], bin_ms=0.4)
    with pytest.raises(ValueError, match='stencil="lattice"') as ei:
        directional.FieldDirectional("unused.h5", _sd(fcc_flag=0), REGIONS_F, stencil="lattice", **kw)
    assert "fcc_flag" in str(ei.value)
    with pytest.raises(ValueError, match="stencil") as ei:
        directional.FieldDirectional("unused.h5", _sd(), REGIONS_F, stencil="diagonal", **kw)
    assert "diagonal" in str(ei.value)
    for flag in (1, 2):  # today's refusal now points to the stencil
        with pytest.raises(ValueError, match="fcc_flag") as ei:
            directional.FieldDirectional("unused.h5", _sd(fcc_flag=flag), REGIONS_F, **kw)
        assert 'stencil="lattice"' in str(ei.value)
    with pytest.raises(ValueError, match="axes"):  # the axes stay 1 .. 3
        directional.FieldDirectional("unused.h5", _sd(), REGIONS_F, stencil="lattice", **{**kw, "axes": [5]})
    fd = directional.FieldDirectional("unused.h5", _sd(fcc_flag=1), REGIONS_F, [125.0], [2, 1, 3], 5.0, stencil="lattice")
    assert fd.comp.tolist() == [0, 5, 4, 6] and fd.prod.shape == (10, 3)
