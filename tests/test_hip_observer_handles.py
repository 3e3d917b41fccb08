"""GPU: the handles of the five kinds of region observer (pf_accum, pf_bandacc, pf_vbandacc, pf_decim, pf_vdecim) are told apart -- by engine, by
kind, and an engine's from a chain's.  Two engines on one device and a two-slab chain, one object of each kind on each; every handle is refused
(PF_ERR_ARG, the function's name in the message) by the other engine's functions of its own kind, by its own engine's functions of every other kind,
and a chain's handle by the engine's functions with the message that names pf_multi_*.  After all the refusals every rightful object takes two more
samples and returns, bit for bit, what the same objects of an engine that saw no refusal return."""
import ctypes

import numpy as np
import pytest
from scipy.signal import butter

import cases
from pffdtd_amd import engine

pytestmark = pytest.mark.gpu

KINDS = ("accum", "bandacc", "vband", "decim", "vdecim")
LO, HI = [2, 2, 2], [5, 5, 5]  # 3 x 3 x 3 around the source, away from the faces
PRE = butter(2, 0.05, "high", output="sos")  # [1, 6]
PRE2 = np.stack([PRE, butter(2, 0.08, "high", output="sos")])  # [2, 1, 6]
BAND = butter(2, [0.1, 0.3], "band", output="sos")[None, :1]  # [1, 1, 6]
TAPS = np.random.default_rng(5).uniform(-1.0, 1.0, 5)
BEFORE, AFTER = 3, 2  # samples before and after the refusals


def _make(owner):
    return {"accum": owner.accumulator(LO, HI, nchan=2),
            "bandacc": owner.band_accumulator(LO, HI, pre_sos=PRE, band_sos=BAND, nbin=2),
            "vband": owner.vector_band_accumulator(LO, HI, comp=(0, 2), pre_sos=PRE2, band_sos=BAND, prod=((0, 1, 0),), nbin=2),
            "decim": owner.decimating_recorder(LO, HI, pre_sos=PRE, taps=TAPS, factor=2, cap=8),
            "vdecim": owner.vector_decimating_recorder(LO, HI, comp=(0, 2), pre_sos=PRE2, taps=TAPS, factor=2, cap=8)}


def _sample(eng, objs, n0, steps):
    for n in range(n0, n0 + steps):
        eng.run(n, 1)
        objs["accum"].add([1.0, -0.5 * n])
        objs["bandacc"].add(n % 2)
        objs["vband"].add(n % 2)
        objs["decim"].add()
        objs["vdecim"].add()


def _results(objs):
    out = [objs["accum"].get(), *objs["bandacc"].get(), *objs["vband"].get()]
    for k in ("decim", "vdecim"):
        first, frames = objs[k].read()
        assert first == 0
        out += [frames, *objs[k].get_state()]
    out.append(np.array([objs[k].count for k in KINDS]))
    return out


def test_a_handle_is_its_engines_and_its_kinds_alone():
    L = engine.lib()
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    flags = engine.PF_MULTI_NO_PAIRS | engine.PF_MULTI_NO_TRIPLES
    sds = [cases.make_sd("cart_outside", "double") for _ in range(4)]
    A, B, fresh = engine.HipEngine(sds[0]), engine.HipEngine(sds[1]), engine.HipEngine(sds[2])
    M = engine.HipMulti(sds[3], [0, 0], multi_flags=flags)
    assert M.info()["nslabs"] == 2
    objs, objs_b, objs_m, objs_f = _make(A), _make(B), _make(M), _make(fresh)
    _sample(A, objs, 0, BEFORE)
    _sample(fresh, objs_f, 0, BEFORE)

    w = np.ones(2)
    buf = np.zeros(4096)  # more than any get, read or get_state of these objects writes
    wp, bp = w.ctypes.data_as(vp), buf.ctypes.data_as(vp)
    first, nread = i64(), i64()
    fb, nb = ctypes.byref(first), ctypes.byref(nread)
    # per kind: the calls that take (engine, handle), by the name that must stand in the message
    calls = {
        "accum": {"add": lambda e, a: L.pf_engine_accum_add(e, a, wp), "get": lambda e, a: L.pf_engine_accum_get(e, a, bp),
                  "destroy": lambda e, a: L.pf_engine_accum_destroy(e, a)},
        "bandacc": {"add": lambda e, a: L.pf_engine_bandacc_add(e, a, 0), "get": lambda e, a: L.pf_engine_bandacc_get(e, a, bp, None),
                    "destroy": lambda e, a: L.pf_engine_bandacc_destroy(e, a)},
        "vband": {"add": lambda e, a: L.pf_engine_vband_add(e, a, 0), "get": lambda e, a: L.pf_engine_vband_get(e, a, bp, None),
                  "destroy": lambda e, a: L.pf_engine_vband_destroy(e, a)},
        "decim": {"add": lambda e, a: L.pf_engine_decim_add(e, a), "read": lambda e, a: L.pf_engine_decim_read(e, a, bp, 1, fb, nb),
                  "get_state": lambda e, a: L.pf_engine_decim_get_state(e, a, bp, None), "destroy": lambda e, a: L.pf_engine_decim_destroy(e, a)},
        "vdecim": {"add": lambda e, a: L.pf_engine_vdecim_add(e, a), "read": lambda e, a: L.pf_engine_vdecim_read(e, a, bp, 1, fb, nb),
                   "get_state": lambda e, a: L.pf_engine_vdecim_get_state(e, a, bp, None), "destroy": lambda e, a: L.pf_engine_vdecim_destroy(e, a)},
    }

    def refused(kind, fn, e, a, *also):
        rc, msg = calls[kind][fn](e, a), L.pf_last_error().decode()
        assert rc == 1 and f"pf_engine_{kind}_{fn}" in msg and all(s in msg for s in also), (kind, fn, rc, msg)

    refusals = 0
    for kind in KINDS:
        # another engine's functions of the handle's own kind
        for fn in calls[kind]:
            refused(kind, fn, B._h, objs[kind]._a, "another engine")
            refusals += 1
        # its own engine's functions of every other kind
        for other in KINDS:
            if other != kind:
                for fn in calls[other]:
                    if fn != "destroy":
                        refused(other, fn, A._h, objs[kind]._a)
                        refusals += 1
        # a chain's handle at an engine's door
        for fn in calls[kind]:
            refused(kind, fn, A._h, objs_m[kind]._a, "another engine", f"pf_multi_{kind}_")
            refusals += 1
    refused("vdecim", "read", A._h, objs["decim"]._a)  # (named in particular: the two recorders share their device code)
    refused("decim", "read", A._h, objs["vdecim"]._a)
    assert refusals == 2 * sum(len(c) for c in calls.values()) + sum(len(calls[o]) - 1 for k in KINDS for o in KINDS if o != k)
    assert [objs[k].count for k in KINDS] == [BEFORE] * 5 and [objs_b[k].count for k in KINDS] == [0] * 5 and [objs_m[k].count for k in KINDS] == [0] * 5

    _sample(A, objs, BEFORE, AFTER)
    _sample(fresh, objs_f, BEFORE, AFTER)
    got, want = _results(objs), _results(objs_f)
    assert len(got) == len(want) == 12
    for i, (g, x) in enumerate(zip(got, want)):
        assert g.shape == x.shape and np.array_equal(g, x), i
    assert np.abs(got[0]).max() > 0 and got[5].shape == (3, 3, 3, 3) and got[8].shape == (3, 2, 3, 3, 3)
    # the other engine's and the chain's objects are whole too
    _sample(B, objs_b, 0, 1)
    _sample(M, objs_m, 0, 1)
    assert [objs_b[k].count for k in KINDS] == [1] * 5 and [objs_m[k].count for k in KINDS] == [1] * 5
    for o in (objs, objs_b, objs_m, objs_f):
        for a in o.values():
            a.close()
    M.close()
    for e in (A, B, fresh):
        e.close()
