"""GPU: field accumulators on engines that share no kernel, layout or decomposition (part 4 of tests/test_hip_accum.py, in a file of its own).

Why its own file: tests run in the order of their files' names, and tests/test_hip_autotune.py::test_engine_survives_a_full_device fails whenever a
chain of three slabs on this scene has run in the same process before it -- the existing chain tests of test_hip_region.py do that to it too when they
are put in front of it; they never are, because their files sort behind it.  This file sorts behind it as well.

v25, v40, exchanged storage, a chain of 3 along x and a chain of 2 along file z, all on `triple_scene` (48 x 100 x 280 / 264) from random fields, in
both precisions: the sums equal the numpy fold of the object's own get_region frames in every cell and of an oracle trajectory inside, and the run
ends on the oracle's receivers and fields.  Every comparison is np.array_equal.
"""
import numpy as np
import pytest

import oracle
from pffdtd_amd import engine, sim_data
from test_hip_accum import _fold, _inner, _w5
from test_hip_checkpoint import N_END, Triple
from test_hip_region import _slices

pytestmark = pytest.mark.gpu
SAMPLES = list(range(0, N_END, 3))  # v40 steps in triples: run(n, 3) between the samples
NO_PASSES = engine.PF_MULTI_NO_PAIRS | engine.PF_MULTI_NO_TRIPLES


class Sampled(Triple):
    """Triple's scene and trajectory, and the oracle's u^n at the sample steps (computed once, never changed)"""

    def __init__(self, prec):
        super().__init__(prec)
        ref = sim_data.SimData.from_sim(self.sim, prec)
        ref.scale_input()
        e = oracle.Engine(ref)
        for k in (0, 1):
            e.grid(k)[...] = self.init[k]
        self.ref_u = {}
        for n in range(SAMPLES[-1] + 1):
            if n in SAMPLES:
                self.ref_u[n] = e.grid(1).copy()
            e.step(n)
        e.close()

    def make(self, kind):
        if kind == "chain3":
            sd = self.sd()
            return engine.HipMulti(sd, [0, 0, 0], multi_flags=NO_PASSES, verify_exchange=2), sd
        if kind == "chain2z":
            sd = self.sd()
            return engine.HipMulti(sd, [0, 0], multi_flags=engine.PF_MULTI_CUT_Z | NO_PASSES, verify_exchange=2), sd
        return self.maker(kind)()


@pytest.fixture(scope="module", params=["single", "double"])
def sampled(request):
    return Sampled(request.param)


def _chain_regions(obj, N, kind):
    """a box across every cut with strides 3 and 5, an x and a z plane; for a chain the planes on x0 and x1 - 1 of every slab"""
    out = [([1, 2, 1], [N[0] - 1, N[1] - 2, N[2] - 1], [3, 1, 5]), ([N[0] // 2, 0, 0], [N[0] // 2 + 1, N[1], N[2]], [1, 1, 1]),
           ([0, 0, N[2] // 2], [N[0], N[1], N[2] // 2 + 1], [1, 1, 1])]
    if isinstance(obj, engine.HipMulti):
        a = 2 if kind == "chain2z" else 0
        for g in range(obj.nslabs):
            for k in (obj.slab(g)["x0"], obj.slab(g)["x1"] - 1):
                lo, hi = [0, 0, 0], list(N)
                lo[a], hi[a] = k, k + 1
                out.append((lo, hi, [1, 1, 1]))
    return out


@pytest.mark.parametrize("kind", ["v25", "v40", "exchanged", "chain3", "chain2z"])
def test_sums_of_every_engine_and_chain(sampled, kind):
    obj, sd = sampled.make(kind)
    N = sampled.n
    if isinstance(obj, engine.HipMulti):
        info = obj.info()
        assert info["cut_along_z"] == (kind == "chain2z") and info["nslabs"] == (2 if kind == "chain2z" else 3), info
        assert all(obj.slab(g)["steps_per_pass"] == 0 for g in range(obj.nslabs))
    elif kind == "v40":
        assert obj.timing()["tb_steps_per_pass"] == 3
    elif kind == "exchanged":
        assert obj.layout()[2]
    obj.load_state(sampled.start)
    regions = _chain_regions(obj, N, kind)
    accs = [obj.accumulator(*r, nchan=5) for r in regions]
    want = [np.zeros(a.shape) for a in accs]
    want_ref = [np.zeros(a.shape) for a in accs]
    for n in SAMPLES:
        w = _w5(n)
        for i, r in enumerate(regions):
            _fold(want[i], w, obj.get_region(1, *r))
            accs[i].add(w)
            _fold(want_ref[i], w, sampled.ref_u[n][_slices(r)])
        obj.run(n, 3)
    inner = _inner(N)
    for i, r in enumerate(regions):
        got = accs[i].get()
        assert accs[i].count == len(SAMPLES) and np.array_equal(got, want[i]), (kind, sampled.prec, r, int(np.count_nonzero(got != want[i])))
        sel = inner[_slices(r)]
        assert np.array_equal(got[:, sel], want_ref[i][:, sel]) and np.abs(got).max() > 0, (kind, sampled.prec, "oracle", r)
    out, after = sd.u_out.copy(), obj.save_state()
    obj.close()
    sampled.check_end(out, after, f"{kind} after accumulators")


def test_a_chain_with_default_flags_adds_all_or_nothing(sampled):
    """the chain of the issue with default flags: an add succeeds or is refused with PF_ERR_STATE, and a refused add leaves count and sums as they
    were.  (Slabs of 16 planes take single steps, so on this scene no add is refused; tests/test_hip_accum.py forces pairs and sees the refusals.)"""
    obj, sd = sampled.maker("chain3")()
    obj.load_state(sampled.start)
    N = sampled.n
    r = ([1, 2, 1], [N[0] - 1, N[1] - 2, N[2] - 1], [3, 1, 5])
    acc = obj.accumulator(*r, nchan=5)
    want = np.zeros(acc.shape)
    ok = refused = compared = 0
    for n in range(N_END):
        w = _w5(n)
        count = acc.count
        try:
            acc.add(w)
        except engine.PfError as e:
            assert e.code == 4, str(e)
            refused += 1
            assert acc.count == count
        else:
            ok += 1
            _fold(want, w, obj.get_region(1, *r))
            assert acc.count == count + 1
        try:  # (get is valid between passes only, like add: where it answers, the sums are those of the samples that were taken and of no other)
            got = acc.get()
        except engine.PfError as e:
            assert e.code == 4, str(e)
        else:
            compared += 1
            assert np.array_equal(got, want), n
        obj.run(n, 1)
    assert ok > 0 and ok + refused == N_END and compared >= ok
    assert np.array_equal(acc.get(), want) and acc.count == ok
    print("default-flag chain:", ok, "samples taken,", refused, "refused")
    out, after = sd.u_out.copy(), obj.save_state()
    obj.close()
    sampled.check_end(out, after, "default chain after refused adds")
