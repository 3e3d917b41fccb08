"""ctypes binding of libpffdtd_hip.so (include/pffdtd_hip.h): the only compute path of this package.

There is no CPU fallback: if the HIP library is missing or no GPU is visible, construction raises.
"""
import ctypes
import importlib.util
import os
import sys
from pathlib import Path

import numpy as np

from .sim_data import PfSimData

_HERE = Path(__file__).resolve().parent
_LIB = None

PF_NUM_CPU_EXACT = 0
PF_NUM_GPU_SAFEGUARDED = 2


class PfOpts(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("numerics", ctypes.c_int32), ("slab_first", ctypes.c_int32),
                ("slab_last", ctypes.c_int32), ("readout_chunk", ctypes.c_int32), ("air_variant", ctypes.c_int32),
                ("air_chunk", ctypes.c_int32), ("timing", ctypes.c_int32), ("ext_u0", ctypes.c_void_p),
                ("ext_u1", ctypes.c_void_p), ("x_global0", ctypes.c_int32), ("layout", ctypes.c_int32),
                ("energy", ctypes.c_int32), ("multi_flags", ctypes.c_int32), ("transport", ctypes.c_int32),
                ("verify_exchange", ctypes.c_int32), ("only_slab", ctypes.c_int32), ("wall_scale", ctypes.c_double)]


# Development / test switches (csrc/pf_debug.h: the PF_DBG_* bits, the chain's fault injection).  Not fields of pf_opts: they reach the
# library through its internal hook, for the NEXT create call of this thread.
_HOOKS = ("debug", "test_drop_exchange", "test_faults")


def _set_hooks(debug=0, test_drop_exchange=0, test_faults=0):
    lib().pf_internal_hooks(int(debug), int(test_drop_exchange), int(test_faults))


class PfTiming(ctypes.Structure):
    _fields_ = [("air_ms_total", ctypes.c_double), ("air_launches", ctypes.c_int64),
                ("step_ms_total", ctypes.c_double), ("steps", ctypes.c_int64),
                ("tb2_ms_total", ctypes.c_double), ("tb2_launches", ctypes.c_int64), ("tb2_cells", ctypes.c_int64),
                ("tune_ms", ctypes.c_double * 3), ("air_path", ctypes.c_int64), ("tb2_lw", ctypes.c_int64),
                ("tb2_dirty_tiles", ctypes.c_int64), ("place_candidates", ctypes.c_int64), ("place_ms", ctypes.c_double * 3),
                ("wall_blocks", ctypes.c_int64 * 2), ("tb_steps_per_pass", ctypes.c_int64), ("wall_bricks", ctypes.c_int64), ("wall_three_steps", ctypes.c_int64),
                ("wall_profile", ctypes.c_int64), ("wall_uniform_branches", ctypes.c_int64), ("wall_unread_skipped", ctypes.c_int64),
                ("wall_strips_staged", ctypes.c_int64),
                ("fcc_shell_bricks", ctypes.c_int64)]


class PfMultiInfo(ctypes.Structure):
    _fields_ = [("nslabs", ctypes.c_int32), ("transport", ctypes.c_int32), ("rccl_self", ctypes.c_int32),
                ("exchange_verified", ctypes.c_int32), ("exchanges_checked", ctypes.c_int64),
                ("exchange_nonzero", ctypes.c_int32), ("cut_along_z", ctypes.c_int32), ("plane_bytes", ctypes.c_int64),
                ("last_run_seconds", ctypes.c_double), ("transport_name", ctypes.c_char * 64),
                ("transport_note", ctypes.c_char * 256), ("wall_scale", ctypes.c_double), ("wall_measured", ctypes.c_int32)]


class PfState(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("u_prev", "u_cur", "u1b", "u2b", "vh1", "gh1")]


class PfRegion(ctypes.Structure):
    _fields_ = [("lo", ctypes.c_int64 * 3), ("hi", ctypes.c_int64 * 3), ("stride", ctypes.c_int64 * 3)]


STATE_KEYS = tuple(k for k, _ in PfState._fields_)
PF_MMB = 12


class PfError(RuntimeError):
    code = None  # the pf_status behind it, where a library call returned one (4 = PF_ERR_STATE: call sequence violated)


def _state_arrays(sd, state=None):
    """The six arrays of a pf_state for scene sd (new ones, or `state`'s checked and made contiguous) and the struct that names them."""
    dt = np.float32 if sd.real_bytes == 4 else np.float64
    shapes = {"u_prev": (sd.Nx, sd.Ny, sd.Nz), "u_cur": (sd.Nx, sd.Ny, sd.Nz), "u1b": (sd.Nbl,), "u2b": (sd.Nbl,),
              "vh1": (sd.Nbl, PF_MMB), "gh1": (sd.Nbl, PF_MMB)}
    arr = {}
    for k in STATE_KEYS:
        if state is None:
            arr[k] = np.zeros(shapes[k], dtype=dt)
        else:
            a = np.ascontiguousarray(state[k], dtype=dt)
            if a.size != int(np.prod(shapes[k])):
                raise PfError(f"state[{k!r}] has {a.size} elements, the scene needs {int(np.prod(shapes[k]))}")
            arr[k] = a.reshape(shapes[k])
    st = PfState(**{k: arr[k].ctypes.data_as(ctypes.c_void_p) if arr[k].size else None for k in STATE_KEYS})
    return arr, st


EXPORTS = ["pf_last_error", "pf_version", "pf_device_count", "pf_grid_bytes", "pf_grid_pitch", "pf_opts_default",
           "pf_run_sim", "pf_engine_create", "pf_engine_destroy", "pf_engine_run", "pf_engine_step_begin",
           "pf_engine_halo_ptrs", "pf_engine_step_end", "pf_engine_state_grids", "pf_engine_layout", "pf_engine_place_grids", "pf_engine_place_grids5", "pf_engine_set_spares", "pf_engine_stream", "pf_engine_sync",
           "pf_engine_flush_outputs", "pf_engine_get_grid", "pf_engine_set_grid", "pf_engine_save_state", "pf_engine_load_state",
           "pf_multi_save_state", "pf_multi_load_state", "pf_region_count", "pf_engine_get_region", "pf_multi_get_region", "pf_engine_timing", "pf_engine_set_timing",
           "pf_engine_accum_create", "pf_engine_accum_add", "pf_engine_accum_get", "pf_engine_accum_set", "pf_engine_accum_destroy", "pf_accum_count",
           "pf_multi_accum_create", "pf_multi_accum_add", "pf_multi_accum_get", "pf_multi_accum_set", "pf_multi_accum_destroy",
           "pf_engine_bandacc_create", "pf_engine_bandacc_add", "pf_engine_bandacc_get", "pf_engine_bandacc_set", "pf_engine_bandacc_destroy", "pf_bandacc_count",
           "pf_multi_bandacc_create", "pf_multi_bandacc_add", "pf_multi_bandacc_get", "pf_multi_bandacc_set", "pf_multi_bandacc_destroy",
           "pf_engine_vband_create", "pf_engine_vband_add", "pf_engine_vband_get", "pf_engine_vband_set", "pf_engine_vband_destroy", "pf_vbandacc_count",
           "pf_multi_vband_create", "pf_multi_vband_add", "pf_multi_vband_get", "pf_multi_vband_set", "pf_multi_vband_destroy",
           "pf_engine_decim_create", "pf_engine_decim_add", "pf_engine_decim_read", "pf_engine_decim_get_state", "pf_engine_decim_set_state", "pf_engine_decim_destroy",
           "pf_decim_count", "pf_decim_pending",
           "pf_multi_decim_create", "pf_multi_decim_add", "pf_multi_decim_read", "pf_multi_decim_get_state", "pf_multi_decim_set_state", "pf_multi_decim_destroy",
           "pf_engine_vdecim_create", "pf_engine_vdecim_add", "pf_engine_vdecim_read", "pf_engine_vdecim_get_state", "pf_engine_vdecim_set_state", "pf_engine_vdecim_destroy",
           "pf_vdecim_count", "pf_vdecim_pending",
           "pf_multi_vdecim_create", "pf_multi_vdecim_add", "pf_multi_vdecim_read", "pf_multi_vdecim_get_state", "pf_multi_vdecim_set_state", "pf_multi_vdecim_destroy",
           "pf_engine_absorb_create", "pf_engine_absorb_add", "pf_engine_absorb_get", "pf_engine_absorb_set", "pf_engine_absorb_destroy", "pf_absorb_count",
           "pf_multi_absorb_create", "pf_multi_absorb_add", "pf_multi_absorb_get", "pf_multi_absorb_set", "pf_multi_absorb_destroy",
           "pf_engine_energy_cfg", "pf_engine_run_energy", "pf_run_sim_devices", "pf_slab_partition", "pf_slab_partition_w", "pf_slab_partition_axis", "pf_slab_wall_scale",
           "pf_multi_create", "pf_multi_run", "pf_multi_get_info", "pf_multi_get_slab", "pf_multi_destroy",
           "pf_rccl_unique_id", "pf_rccl_comm_create", "pf_rccl_exchange", "pf_rccl_comm_destroy"]


INTERNAL_EXPORTS = ["pf_internal_hooks"]  # csrc/pf_debug.h: exported, but no part of the drop-in boundary (not in include/)

PF_MULTI_EVEN_SPLIT, PF_MULTI_ONE_THREAD, PF_MULTI_NO_PAIRS, PF_MULTI_FORCE_PAIRS, PF_MULTI_CUT_Z, PF_MULTI_CUT_X = 1, 2, 4, 8, 16, 32
PF_MULTI_NO_TRIPLES = 64
PF_MULTI_MEASURE_WEIGHTS = 128
PF_TRANSPORT_AUTO, PF_TRANSPORT_PEER, PF_TRANSPORT_RCCL, PF_TRANSPORT_HOST = 0, 1, 2, 3
PF_LAYOUT_AUTO, PF_LAYOUT_EXCHANGED, PF_LAYOUT_FILE = 0, 1, 2


def _preload_torch_hip():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so.7 (same soname as /opt/rocm's).  The copy loaded first serves
    the whole process, and torch only finds its GPUs through its own.  So that the order of `import torch` and the first
    engine call does not matter, load torch's copy (without importing torch) before libpffdtd_hip.so pulls in the system
    one.  PFFDTD_SYSTEM_HIP=1 keeps the system runtime (engine-only hosts that never import torch)."""
    if "torch" in sys.modules or os.environ.get("PFFDTD_SYSTEM_HIP") == "1":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    p = Path(spec.submodule_search_locations[0]) / "lib" / "libamdhip64.so"
    if p.exists():
        try:
            ctypes.CDLL(str(p), mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def lib_path():
    return _HERE / "libpffdtd_hip.so"


def lib():
    """Load libpffdtd_hip.so; raises if it has not been built (no silent fallback)."""
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not p.exists():
            raise PfError(f"{p} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _preload_torch_hip()
        L = ctypes.CDLL(str(p))
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
        L.pf_last_error.restype = ctypes.c_char_p
        L.pf_version.restype = ctypes.c_char_p
        L.pf_device_count.restype = ctypes.c_int
        L.pf_grid_bytes.restype = ctypes.c_size_t
        L.pf_grid_bytes.argtypes = [i64, i64, i64, i32]
        L.pf_grid_pitch.restype = i64
        L.pf_grid_pitch.argtypes = [i64, i32]
        L.pf_opts_default.argtypes = [ctypes.POINTER(PfOpts)]
        L.pf_internal_hooks.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
        L.pf_internal_hooks.restype = None
        L.pf_run_sim.restype = ctypes.c_double
        L.pf_run_sim.argtypes = [ctypes.POINTER(PfSimData)]
        L.pf_engine_create.argtypes = [ctypes.POINTER(PfSimData), ctypes.POINTER(PfOpts), ctypes.POINTER(vp)]
        L.pf_engine_destroy.argtypes = [vp]
        L.pf_engine_destroy.restype = None
        L.pf_engine_run.argtypes = [vp, i64, i64]
        L.pf_engine_step_begin.argtypes = [vp, i64]
        L.pf_engine_step_end.argtypes = [vp, i64]
        L.pf_engine_halo_ptrs.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp),
                                          ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
        L.pf_engine_state_grids.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp)]
        L.pf_engine_layout.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i32)]
        L.pf_engine_place_grids.argtypes = [vp, ctypes.POINTER(vp), i32, ctypes.POINTER(i32)]
        L.pf_engine_place_grids5.argtypes = [vp, ctypes.POINTER(vp), i32, ctypes.POINTER(i32)]
        L.pf_engine_stream.restype = vp
        L.pf_engine_stream.argtypes = [vp, i32]
        L.pf_engine_sync.argtypes = [vp]
        L.pf_engine_flush_outputs.argtypes = [vp]
        L.pf_engine_get_grid.argtypes = [vp, i32, vp]
        L.pf_engine_set_grid.argtypes = [vp, i32, vp]
        L.pf_engine_timing.argtypes = [vp, ctypes.POINTER(PfTiming), i32]
        for f in (L.pf_engine_save_state, L.pf_engine_load_state, L.pf_multi_save_state, L.pf_multi_load_state):
            f.argtypes = [vp, ctypes.POINTER(PfState)]
        L.pf_region_count.restype = i64
        L.pf_region_count.argtypes = [ctypes.POINTER(PfRegion), ctypes.POINTER(i64)]
        for f in (L.pf_engine_get_region, L.pf_multi_get_region):
            f.argtypes = [vp, i32, ctypes.POINTER(PfRegion), vp]
        L.pf_engine_set_timing.argtypes = [vp, i32]
        for pre in ("pf_engine", "pf_multi"):
            getattr(L, pre + "_accum_create").argtypes = [vp, ctypes.POINTER(PfRegion), i32, i32, ctypes.POINTER(vp)]
            getattr(L, pre + "_accum_add").argtypes = [vp, vp, vp]
            getattr(L, pre + "_accum_get").argtypes = [vp, vp, vp]
            getattr(L, pre + "_accum_set").argtypes = [vp, vp, vp, i64]
            getattr(L, pre + "_accum_destroy").argtypes = [vp, vp]
            getattr(L, pre + "_bandacc_create").argtypes = [vp, ctypes.POINTER(PfRegion), i32, vp, i32, i32, vp, i64, i32, ctypes.POINTER(vp)]
            getattr(L, pre + "_bandacc_add").argtypes = [vp, vp, i64]
            getattr(L, pre + "_bandacc_get").argtypes = [vp, vp, vp, vp]
            getattr(L, pre + "_bandacc_set").argtypes = [vp, vp, vp, vp, i64]
            getattr(L, pre + "_bandacc_destroy").argtypes = [vp, vp]
            getattr(L, pre + "_vband_create").argtypes = [vp, ctypes.POINTER(PfRegion), i32, vp, i32, vp, i32, i32, vp, i32, vp, i64, i32, ctypes.POINTER(vp)]
            getattr(L, pre + "_vband_add").argtypes = [vp, vp, i64]
            getattr(L, pre + "_vband_get").argtypes = [vp, vp, vp, vp]
            getattr(L, pre + "_vband_set").argtypes = [vp, vp, vp, vp, i64]
            getattr(L, pre + "_vband_destroy").argtypes = [vp, vp]
            getattr(L, pre + "_decim_create").argtypes = [vp, ctypes.POINTER(PfRegion), i32, vp, i32, vp, i32, i64, i32, ctypes.POINTER(vp)]
            getattr(L, pre + "_decim_add").argtypes = [vp, vp]
            getattr(L, pre + "_decim_read").argtypes = [vp, vp, vp, i64, ctypes.POINTER(i64), ctypes.POINTER(i64)]
            getattr(L, pre + "_decim_get_state").argtypes = [vp, vp, vp, vp]
            getattr(L, pre + "_decim_set_state").argtypes = [vp, vp, vp, vp, i64]
            getattr(L, pre + "_decim_destroy").argtypes = [vp, vp]
            getattr(L, pre + "_vdecim_create").argtypes = [vp, ctypes.POINTER(PfRegion), i32, vp, i32, vp, i32, vp, i32, i64, i32, ctypes.POINTER(vp)]
            getattr(L, pre + "_vdecim_add").argtypes = [vp, vp]
            getattr(L, pre + "_vdecim_read").argtypes = [vp, vp, vp, i64, ctypes.POINTER(i64), ctypes.POINTER(i64)]
            getattr(L, pre + "_vdecim_get_state").argtypes = [vp, vp, vp, vp]
            getattr(L, pre + "_vdecim_set_state").argtypes = [vp, vp, vp, vp, i64]
            getattr(L, pre + "_vdecim_destroy").argtypes = [vp, vp]
            getattr(L, pre + "_absorb_create").argtypes = [vp, vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, i32, ctypes.POINTER(vp)]
            getattr(L, pre + "_absorb_add").argtypes = [vp, vp, i64, i64]
            getattr(L, pre + "_absorb_get").argtypes = [vp, vp, vp, vp, vp, vp]
            getattr(L, pre + "_absorb_set").argtypes = [vp, vp, vp, vp, vp, vp, i64]
            getattr(L, pre + "_absorb_destroy").argtypes = [vp, vp]
        L.pf_absorb_count.restype = i64
        L.pf_absorb_count.argtypes = [vp]
        L.pf_accum_count.restype = i64
        L.pf_accum_count.argtypes = [vp]
        L.pf_bandacc_count.restype = i64
        L.pf_bandacc_count.argtypes = [vp]
        L.pf_vbandacc_count.restype = i64
        L.pf_vbandacc_count.argtypes = [vp]
        for f in (L.pf_decim_count, L.pf_decim_pending, L.pf_vdecim_count, L.pf_vdecim_pending):
            f.restype = i64
            f.argtypes = [vp]
        dp = ctypes.POINTER(ctypes.c_double)
        L.pf_engine_energy_cfg.argtypes = [vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, dp]
        L.pf_engine_run_energy.argtypes = [vp, i64, i64, dp, dp, dp]
        L.pf_run_sim_devices.restype = ctypes.c_double
        L.pf_run_sim_devices.argtypes = [ctypes.POINTER(PfSimData), i32, ctypes.POINTER(i32), ctypes.POINTER(PfOpts)]
        L.pf_slab_partition.argtypes = [ctypes.POINTER(PfSimData), i32, i32, ctypes.POINTER(i64)]
        L.pf_slab_partition_w.argtypes = [ctypes.POINTER(PfSimData), i32, i32, ctypes.c_double, ctypes.POINTER(i64)]
        L.pf_slab_partition_axis.argtypes = [ctypes.POINTER(PfSimData), i32, i32, ctypes.c_double, i32, ctypes.POINTER(i64)]
        L.pf_slab_wall_scale.argtypes = [ctypes.POINTER(PfSimData), i32, i32, ctypes.POINTER(PfOpts)]
        L.pf_slab_wall_scale.restype = ctypes.c_double
        L.pf_engine_set_spares.argtypes = [vp, vp, vp]
        L.pf_multi_create.argtypes = [ctypes.POINTER(PfSimData), i32, ctypes.POINTER(i32), ctypes.POINTER(PfOpts), ctypes.POINTER(vp)]
        L.pf_multi_run.argtypes = [vp, i64, i64]
        L.pf_multi_get_info.argtypes = [vp, ctypes.POINTER(PfMultiInfo)]
        L.pf_multi_get_slab.argtypes = [vp, i32, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(vp)]
        L.pf_multi_destroy.argtypes = [vp]
        L.pf_multi_destroy.restype = None
        L.pf_rccl_unique_id.argtypes = [ctypes.c_char_p]
        L.pf_rccl_comm_create.argtypes = [ctypes.c_char_p, i32, i32, i32, ctypes.POINTER(ctypes.c_void_p)]
        L.pf_rccl_exchange.argtypes = [ctypes.c_void_p, ctypes.c_void_p, i32, i32]
        L.pf_rccl_comm_destroy.argtypes = [ctypes.c_void_p]
        L.pf_rccl_comm_destroy.restype = None
        _LIB = L
    return _LIB


def _check(rc):
    if rc != 0:
        e = PfError(f"pffdtd_hip error {rc}: {lib().pf_last_error().decode()}")
        e.code = int(rc)
        raise e


def _region(what, lo, hi, stride):
    try:
        return PfRegion((ctypes.c_int64 * 3)(*[int(v) for v in lo]), (ctypes.c_int64 * 3)(*[int(v) for v in hi]), (ctypes.c_int64 * 3)(*[int(v) for v in stride]))
    except TypeError as e:
        raise PfError(f"{what}: lo, hi and stride are three integers each ({e})")


def _cells(r):
    """the counts (c0, c1, c2) of a region: the cells lo + k * stride < hi"""
    counts = (ctypes.c_int64 * 3)()
    if lib().pf_region_count(ctypes.byref(r), counts) < 0:
        _check(1)  # (PF_ERR_ARG: pf_last_error names the field)
    return tuple(int(c) for c in counts)


def _get_region(call, handle, dtype, which, lo, hi, stride):
    """pf_engine_get_region / pf_multi_get_region -> ndarray of shape counts, the cells lo + k * stride < hi in FILE coordinates x, y, z"""
    r = _region("get_region", lo, hi, stride)
    a = np.empty(_cells(r), dtype=dtype)
    _check(call(handle, int(which), ctypes.byref(r), a.ctypes.data_as(ctypes.c_void_p)))
    return a


class _Observer:
    """What the region observers share: the owner that made them, the C handle `_a`, the C functions `_f` of the owner's prefix, count and close.
    An owner closed first took its observers with it: the handle is dead."""
    _kind = ""  # pf_engine_<_kind>_* / pf_multi_<_kind>_*
    _handle = ""  # pf_<_handle>_count
    _noun = "accumulator"

    def _bind(self, owner, prefix, names):
        L = lib()
        self._owner, self._f = owner, {k: getattr(L, f"{prefix}_{self._kind}_{k}") for k in names}
        self._a = ctypes.c_void_p()
        return L

    def _number(self, name):
        if not (self._a.value and self._alive()):
            raise PfError(f"{type(self).__name__}.{name}: the {self._noun} or its owner is closed")
        return int(getattr(lib(), f"pf_{self._handle}_{name}")(self._a))

    @property
    def count(self):
        """samples added so far, or the count given to set / set_state"""
        return self._number("count")

    def _alive(self):
        return bool(getattr(self._owner, "_h", None) and self._owner._h.value)

    def close(self):
        if getattr(self, "_a", None) and self._a.value:
            if self._alive():
                _check(self._f["destroy"](self._owner._h, self._a))
            self._a = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Accumulator(_Observer):
    """Running sums of a region of the field on the device (pf_engine_accum_* / pf_multi_accum_*): acc[m] += w[m] * double(u^n) at every add.
    Made by HipEngine.accumulator / HipMulti.accumulator; it lives no longer than the object that made it."""
    _kind, _handle = "accum", "accum"

    def __init__(self, owner, prefix, lo, hi, stride, nchan, depth):
        r = _region("accumulator", lo, hi, stride)
        self._bind(owner, prefix, ("create", "add", "get", "set", "destroy"))
        _check(self._f["create"](owner._h, ctypes.byref(r), int(nchan), int(depth), ctypes.byref(self._a)))
        self.nchan = int(nchan)
        self.shape = (self.nchan,) + _cells(r)  # of get()

    def add(self, w):
        """the sample of the step the owner stands at: acc[m] += w[m] * double(u^n), w: nchan doubles"""
        w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
        if w.size != self.nchan:
            raise PfError(f"Accumulator.add: {w.size} weights for {self.nchan} channels")
        _check(self._f["add"](self._owner._h, self._a, w.ctypes.data_as(ctypes.c_void_p)))

    def get(self):
        """-> float64 [nchan, c0, c1, c2]: the sums so far (pending samples folded in, nothing reset)"""
        a = np.empty(self.shape, dtype=np.float64)
        _check(self._f["get"](self._owner._h, self._a, a.ctypes.data_as(ctypes.c_void_p)))
        return a

    def set(self, a, count):
        """replace sums and count (a = None: zeros); pending samples are dropped -- how a resumed run continues"""
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.size != int(np.prod(self.shape)):
                raise PfError(f"Accumulator.set: {a.size} sums, the accumulator holds {int(np.prod(self.shape))}")
        _check(self._f["set"](self._owner._h, self._a, None if a is None else a.ctypes.data_as(ctypes.c_void_p), int(count)))


def _sos5(name, sos, lead):
    """scipy-style rows [.., 6] (b0 b1 b2 a0 a1 a2, a0 = 1) -> float64 [.., 5] as the C ABI takes them; `lead` leading dimensions"""
    a = np.asarray([] if sos is None else sos, dtype=np.float64)
    if a.size == 0:
        return np.zeros((0,) * lead + (5,))
    if a.ndim != lead + 1 or a.shape[-1] != 6:
        raise PfError(f"band_accumulator: {name} has shape {a.shape}: {'[npre, 6]' if lead == 1 else '[nband, nsec, 6]'} rows b0 b1 b2 a0 a1 a2 are expected")
    if not np.all(a[..., 3] == 1.0):
        raise PfError(f"band_accumulator: {name}: a0 != 1 in a section (normalise the rows: scipy's sos output has a0 = 1)")
    return np.ascontiguousarray(a[..., [0, 1, 2, 4, 5]])


def _pre3(what, pre_sos, ncomp):
    """a vector kind's pre_sos [ncomp, npre, 6] -> float64 [ncomp, npre, 5]"""
    p = np.asarray([] if pre_sos is None else pre_sos, dtype=np.float64)
    if p.size == 0:
        return np.zeros((ncomp, 0, 5))
    if p.ndim != 3 or p.shape[0] != ncomp:
        raise PfError(f"{what}: pre_sos has shape {p.shape}: [ncomp = {ncomp}, npre, 6] is expected (pad a shorter cascade with 1 0 0 1 0 0)")
    return _sos5("pre_sos", p, 2)


def _ptr(a):
    """an array for the C ABI; None, or an array without elements: null"""
    return None if a is None or a.size == 0 else a.ctypes.data_as(ctypes.c_void_p)


def _float64_or_none(what, noun, arrays):
    """a set's optional arrays (name, array or None, the shape it stands for) -> float64, contiguous, of that size -- or None: zeros"""
    out = []
    for name, a, shape in arrays:
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.size != int(np.prod(shape)):
                raise PfError(f"{what}: {name} has {a.size} elements, the {noun} holds {int(np.prod(shape))}")
        out.append(a)
    return out


class _Bands(_Observer):
    """What the two band accumulators share: all but the components and products of the vector kind, which `_make` takes as the arguments that stand
    around the filters' in its create call and as the leading axes of its arrays."""

    def _make(self, owner, prefix, r, pre, band_sos, nbin, depth, comp=(), prod=(), lead=((), ())):
        b = np.asarray([] if band_sos is None else band_sos, dtype=np.float64)
        if b.ndim == 3 and b.shape[1] == 0:  # nband bands without sections: plain squares (products) of what the pre sections give
            band = np.zeros((b.shape[0], 0, 5))
        else:
            band = _sos5("band_sos", band_sos, 2)
        self._bind(owner, prefix, ("create", "add", "get", "set", "destroy"))
        self.npre, self.nband, self.nsec, self.nbin = int(pre.shape[-2]), int(band.shape[0]), int(band.shape[1]), int(nbin)
        _check(self._f["create"](owner._h, ctypes.byref(r), *comp, self.npre, _ptr(pre), self.nband, self.nsec, _ptr(band), *prod, self.nbin, int(depth), ctypes.byref(self._a)))
        cells = _cells(r)
        self.shape = lead[0] + (self.nband, self.nbin) + cells  # of get()'s sums
        self.state_shape = lead[1] + (self.npre + self.nband * self.nsec, 2) + cells  # ... and state

    def add(self, bin):
        """the sample of the step the owner stands at, its squares (products) summed into time bin `bin` (-1: the filters run, nothing is summed)"""
        _check(self._f["add"](self._owner._h, self._a, int(bin)))

    def get(self, state=True):
        """-> (sums float64 of `shape`, state float64 of `state_shape` or None): pending samples folded in, nothing reset"""
        e = np.empty(self.shape, dtype=np.float64)
        s = np.empty(self.state_shape, dtype=np.float64) if state else None
        _check(self._f["get"](self._owner._h, self._a, e.ctypes.data_as(ctypes.c_void_p), _ptr(s)))
        return e, s

    def set(self, sums, state, count):
        """replace sums, filter state and count (None: zeros); pending samples are dropped -- how a resumed run continues"""
        arrs = _float64_or_none(f"{type(self).__name__}.set", "accumulator", (("sums", sums, self.shape), ("state", state, self.state_shape)))
        _check(self._f["set"](self._owner._h, self._a, *map(_ptr, arrs), int(count)))


class BandAccumulator(_Bands):
    """Per cell of a region, on the device (pf_engine_bandacc_* / pf_multi_bandacc_*): u^n through the shared sections pre_sos [npre, 6], then per
    band through band_sos [nband, nsec, 6] (scipy's sos rows, a0 = 1), squared and summed into time bin `bin` at every add(bin).
    sums are [nband, nbin, c0, c1, c2], state [npre + nband * nsec, 2, c0, c1, c2].
    Made by HipEngine.band_accumulator / HipMulti.band_accumulator; it lives no longer than the object that made it."""
    _kind, _handle = "bandacc", "bandacc"

    def __init__(self, owner, prefix, lo, hi, stride, pre_sos, band_sos, nbin, depth):
        r = _region("band_accumulator", lo, hi, stride)
        self._make(owner, prefix, r, _sos5("pre_sos", pre_sos, 1), band_sos, nbin, depth)


class VectorBandAccumulator(_Bands):
    """Per cell of a region, on the device (pf_engine_vband_* / pf_multi_vband_*): the components `comp` (0: the cell of u^n, 1 / 2 / 3: its central
    difference along file x / y / z on a Cartesian grid, 4 / 5 / 6: the lattice difference along file x / y / z of an FCC grid -- the four pair
    differences over the eight FCC neighbours at +-1 along the axis, in stored coordinates, ~ 8 h du/da) through their own sections pre_sos [ncomp, npre, 6], then per band through band_sos [nband, nsec, 6] (scipy's
    sos rows, a0 = 1; state per component); the products prod [nprod, 3] -- rows (i, j, mode), mode 1: the absolute value -- of two filtered
    components are summed into time bin `bin` at every add(bin).
    sums are [nprod, nband, nbin, c0, c1, c2], state [ncomp, npre + nband * nsec, 2, c0, c1, c2].
    Made by HipEngine.vector_band_accumulator / HipMulti.vector_band_accumulator; it lives no longer than the object that made it."""
    _kind, _handle = "vband", "vbandacc"

    def __init__(self, owner, prefix, lo, hi, stride, comp, pre_sos, band_sos, prod, nbin, depth):
        r = _region("vector_band_accumulator", lo, hi, stride)
        comp = np.ascontiguousarray(np.asarray(comp).reshape(-1), dtype=np.int32)
        prod = np.asarray([] if prod is None else prod)
        if prod.size and (prod.ndim != 2 or prod.shape[1] != 3):
            raise PfError(f"vector_band_accumulator: prod has shape {prod.shape}: [nprod, 3] rows (i, j, mode) are expected")
        prod = np.ascontiguousarray(prod.reshape(-1, 3), dtype=np.int32)
        self.ncomp, self.nprod = int(comp.size), int(prod.shape[0])
        self._make(owner, prefix, r, _pre3("vector_band_accumulator", pre_sos, self.ncomp), band_sos, nbin, depth, comp=(self.ncomp, _ptr(comp)),
                   prod=(self.nprod, _ptr(prod)), lead=((self.nprod,), (self.ncomp,)))


class DecimatingRecorder(_Observer):
    """Per cell of a region, on the device (pf_engine_decim_* / pf_multi_decim_*): every sample u^n through the shared sections pre_sos [npre, 6] and a
    FIR of taps `taps`, every `factor`-th output kept as a frame; up to `cap` frames wait on the device for read().
    Made by HipEngine.decimating_recorder / HipMulti.decimating_recorder; it lives no longer than the object that made it."""
    _kind, _handle, _noun = "decim", "decim", "recorder"

    def __init__(self, owner, prefix, lo, hi, stride, pre_sos, taps, factor, cap, depth):
        r = _region("decimating_recorder", lo, hi, stride)
        self._make("decimating_recorder", owner, prefix, r, _sos5("pre_sos", pre_sos, 1), taps, factor, cap, depth)

    def _make(self, what, owner, prefix, r, pre, taps, factor, cap, depth, comp=(), lead=()):
        """what the two recorders share; comp, lead: the vector kind's arguments of create and the leading axis of its arrays"""
        h = np.ascontiguousarray([] if taps is None else taps, dtype=np.float64)
        if h.ndim != 1:
            raise PfError(f"{what}: taps has shape {h.shape}: a vector of ntap values is expected")
        self._bind(owner, prefix, ("create", "add", "read", "get_state", "set_state", "destroy"))
        self.npre, self.ntap, self.factor = int(pre.shape[-2]), int(h.size), int(factor)
        self.cap = int(cap) if cap else 64  # frames kept on the device between two reads
        _check(self._f["create"](owner._h, ctypes.byref(r), *comp, self.npre, _ptr(pre), self.ntap, _ptr(h), self.factor, self.cap, int(depth), ctypes.byref(self._a)))
        self.cells = _cells(r)
        self.slots = -(-self.ntap // self.factor)  # P
        self._frame = lead + self.cells  # a frame of read()
        self.acc_shape = lead + (self.slots,) + self.cells  # of get_state()'s acc
        self.state_shape = lead + (self.npre, 2) + self.cells  # ... and state

    def add(self):
        """the sample of the step the owner stands at; PfError (code 4) and nothing changed where it would complete a frame while `cap` frames wait"""
        _check(self._f["add"](self._owner._h, self._a))

    def read(self, max_frames=None):
        """-> (first, frames float64 [nread, c0, c1, c2] -- a vector recorder's: [nread, ncomp, c0, c1, c2]): the oldest complete frames in order (all of
        them, or max_frames), marked read"""
        n = self.pending if max_frames is None else int(max_frames)
        out = np.empty((max(n, 0),) + self._frame, dtype=np.float64)
        first, nread = ctypes.c_int64(), ctypes.c_int64()
        _check(self._f["read"](self._owner._h, self._a, _ptr(out), n, ctypes.byref(first), ctypes.byref(nread)))
        return int(first.value), out[:nread.value]

    def get_state(self):
        """-> (acc float64 [P, c0, c1, c2] in slot order, state float64 [npre, 2, c0, c1, c2]; a vector recorder's: with a leading ncomp): pending samples
        folded in, nothing reset"""
        a, s = np.empty(self.acc_shape, dtype=np.float64), np.empty(self.state_shape, dtype=np.float64)
        _check(self._f["get_state"](self._owner._h, self._a, a.ctypes.data_as(ctypes.c_void_p), _ptr(s)))
        return a, s

    def set_state(self, acc, state, count):
        """replace the outputs in flight, the filter state and the count (None: zeros); pending samples and unread frames are dropped"""
        arrs = _float64_or_none("DecimatingRecorder.set_state", "recorder", (("acc", acc, self.acc_shape), ("state", state, self.state_shape)))
        _check(self._f["set_state"](self._owner._h, self._a, *map(_ptr, arrs), int(count)))

    @property
    def pending(self):
        """frames complete and not yet read"""
        return self._number("pending")


class VectorDecimatingRecorder(DecimatingRecorder):
    """Per cell of a region, on the device (pf_engine_vdecim_* / pf_multi_vdecim_*): the components `comp` of a VectorBandAccumulator (0: the cell of
    u^n, 1 / 2 / 3: its central difference along file x / y / z on a Cartesian grid, 4 / 5 / 6: the lattice difference of an FCC grid) through their
    own sections pre_sos [ncomp, npre, 6], then each through the FIR `taps`, every `factor`-th output kept as a frame [ncomp, c0, c1, c2]; up to
    `cap` frames wait on the device for read().  All but the creation is a DecimatingRecorder's.
    Made by HipEngine.vector_decimating_recorder / HipMulti.vector_decimating_recorder; it lives no longer than the object that made it."""
    _kind, _handle = "vdecim", "vdecim"

    def __init__(self, owner, prefix, lo, hi, stride, comp, pre_sos, taps, factor, cap, depth):
        what = "vector_decimating_recorder"
        r = _region(what, lo, hi, stride)
        comp = np.ascontiguousarray(np.asarray(comp).reshape(-1), dtype=np.int32)
        self.ncomp, self.comp = int(comp.size), tuple(int(c) for c in comp)
        self._make(what, owner, prefix, r, _pre3(what, pre_sos, self.ncomp), taps, factor, cap, depth, comp=(self.ncomp, _ptr(comp)), lead=(self.ncomp,))


class Absorption(_Observer):
    """The energy every step takes out of the room, on the device (pf_engine_absorb_* / pf_multi_absorb_*): per frequency-dependent node, per material
    and time bin, with the open boundary's loss and the sources' input.  E: the materials' loss coefficients [Nm, 12] (DEF[..., 1], zero padded).
    add(n, bin) before step n; the first add after creation or set only primes.  Broadband: see include/pffdtd_hip.h.
    Made by HipEngine.absorption / HipMulti.absorption; it lives no longer than the object that made it."""
    _kind, _handle, _noun = "absorb", "absorb", "absorption map"

    def __init__(self, owner, prefix, E, wall_scale, abc_scale, in_scale, nbin):
        sd = owner.sd
        self.Nm, self.Nbl, self.nbin = int(sd.Nm), int(sd.Nbl), int(nbin)
        E = np.ascontiguousarray(E, dtype=np.float64)
        if E.size != self.Nm * PF_MMB:
            raise PfError(f"absorption: E has {E.size} elements, the scene's {self.Nm} materials need [Nm, {PF_MMB}]")
        self._bind(owner, prefix, ("create", "add", "get", "set", "destroy"))
        _check(self._f["create"](owner._h, E.ctypes.data_as(ctypes.c_void_p), float(wall_scale), float(abc_scale), float(in_scale), self.nbin, ctypes.byref(self._a)))
        self._shapes = (("nodes", (self.Nbl,)), ("materials", (self.nbin, self.Nm)), ("open_boundary", (self.nbin,)), ("input", (self.nbin,)))

    def add(self, n, bin):
        """before step n (the state is u^{n-1}, u^n): step n - 1's losses and input go into time bin `bin`; PfError (code 4) for a gap in n"""
        _check(self._f["add"](self._owner._h, self._a, int(n), int(bin)))

    def get(self):
        """-> dict of float64 arrays: nodes [Nbl] in the order of sd.bnl_ixyz, materials [nbin, Nm], open_boundary [nbin], input [nbin]; nothing reset"""
        out = {k: np.zeros(shape, dtype=np.float64) for k, shape in self._shapes}
        _check(self._f["get"](self._owner._h, self._a, *(out[k].ctypes.data_as(ctypes.c_void_p) for k, _ in self._shapes)))
        return out

    def set(self, sums, count):
        """replace the sums (a dict as get()'s; None, or a missing key: zeros) and the count; the next add primes -- how a resumed run continues"""
        sums = sums or {}
        arrs = _float64_or_none("Absorption.set", "absorption map", tuple((k, sums.get(k), shape) for k, shape in self._shapes))
        _check(self._f["set"](self._owner._h, self._a, *map(_ptr, arrs), int(count)))


def device_count():
    return int(lib().pf_device_count())


def grid_pitch(Nz, real_bytes):
    return int(lib().pf_grid_pitch(int(Nz), int(real_bytes)))


def run_sim(sd):
    """`double run_sim(struct SimData*)` (cpu_engine.h:52 / gpu_engine.h:665): fills sd.u_out, returns seconds."""
    s = sd.as_struct()
    el = lib().pf_run_sim(ctypes.byref(s))
    if el < 0:
        raise PfError(f"pf_run_sim failed: {lib().pf_last_error().decode()}")
    return el


def run_sim_devices(sd, devices, multi_flags=0, **opts):
    """pf_run_sim_devices: run_sim on a chain of Z-slabs, slab g on HIP device devices[g] (ids may repeat = virtual
    slabs on one GPU).  opts: numerics, air_variant, readout_chunk, debug.  Fills sd.u_out, returns seconds."""
    L = lib()
    s = sd.as_struct()
    o = _multi_opts(multi_flags, opts)
    devs = (ctypes.c_int32 * len(devices))(*[int(d) for d in devices])
    el = L.pf_run_sim_devices(ctypes.byref(s), len(devices), devs, ctypes.byref(o))
    if el < 0:
        raise PfError(f"pf_run_sim_devices failed: {L.pf_last_error().decode()}")
    return el


def _multi_opts(multi_flags, opts):
    """pf_opts from keyword arguments; `debug` / `test_*` go to the library's internal hook (pending for the create call that follows)."""
    o = PfOpts()
    lib().pf_opts_default(ctypes.byref(o))
    hooks = {k: opts[k] for k in _HOOKS if k in opts}
    for k, v in opts.items():
        if k not in _HOOKS:
            setattr(o, k, float(v) if k == "wall_scale" else int(v))
    o.multi_flags = int(multi_flags)
    _set_hooks(**hooks)
    return o


class HipMulti:
    """A chain of Z-slabs on several devices behind ONE C object (pf_multi_create): one persistent host thread per slab,
    ghost planes by peer copies or RCCL.  devices[g] = HIP device of slab g (ids may repeat: virtual slabs on one GPU).
    opts: pf_opts fields common to all slabs (numerics, air_variant, readout_chunk, debug, timing, transport,
    verify_exchange)."""

    def __init__(self, sd, devices, multi_flags=0, **opts):
        L = lib()
        self.sd = sd
        self._s = sd.as_struct()
        o = _multi_opts(multi_flags, opts)
        devs = (ctypes.c_int32 * len(devices))(*[int(d) for d in devices])
        self._h = ctypes.c_void_p()
        _check(L.pf_multi_create(ctypes.byref(self._s), len(devices), devs, ctypes.byref(o), ctypes.byref(self._h)))
        self.nslabs = len(devices)

    def run(self, n0, nsteps):
        _check(lib().pf_multi_run(self._h, int(n0), int(nsteps)))

    def info(self):
        i = PfMultiInfo()
        _check(lib().pf_multi_get_info(self._h, ctypes.byref(i)))
        return {"nslabs": i.nslabs, "transport": i.transport, "transport_name": i.transport_name.decode(),
                "rccl_self": bool(i.rccl_self), "exchanges_checked": i.exchanges_checked,
                "exchange_verified": None if i.exchange_verified < 0 else bool(i.exchange_verified),
                "exchange_nonzero": bool(i.exchange_nonzero), "cut_along_z": bool(i.cut_along_z), "plane_bytes": i.plane_bytes,
                "last_run_seconds": i.last_run_seconds, "transport_note": i.transport_note.decode(),
                "wall_scale": i.wall_scale, "wall_measured": bool(i.wall_measured)}

    def save_state(self):
        """The whole scene's state between two steps in its canonical form (pf_multi_save_state): a dict of numpy arrays,
        u_prev / u_cur (Nx, Ny, Nz), u1b / u2b (Nbl,), vh1 / gh1 (Nbl, 12)."""
        arr, st = _state_arrays(self.sd)
        _check(lib().pf_multi_save_state(self._h, ctypes.byref(st)))
        return arr

    def load_state(self, state):
        """pf_multi_load_state: continue with run(n, ...) from the step the state was saved at."""
        arr, st = _state_arrays(self.sd, state)
        _check(lib().pf_multi_load_state(self._h, ctypes.byref(st)))

    def get_region(self, which, lo, hi, stride=(1, 1, 1)):
        """A strided box of u^{n-1} (which = 0) or u^n (1) of the whole scene (pf_multi_get_region): every slab cuts the part it owns on its own
        device.  PfError with code 4 while a slab is inside a blocked pass: advance a step and ask again."""
        return _get_region(lib().pf_multi_get_region, self._h, np.float32 if self.sd.real_bytes == 4 else np.float64, which, lo, hi, stride)

    def accumulator(self, lo, hi, stride=(1, 1, 1), nchan=1, depth=0):
        """Running sums of a region of the whole scene (pf_multi_accum_create): every slab sums the part it owns on its own device.  add raises
        PfError with code 4, and changes nothing, while any slab is inside a blocked pass: create the chain with PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES."""
        return Accumulator(self, "pf_multi", lo, hi, stride, nchan, depth)

    def band_accumulator(self, lo, hi, stride=(1, 1, 1), pre_sos=None, band_sos=None, nbin=1, depth=0):
        """Band-filtered squares of a region of the whole scene in time bins (pf_multi_bandacc_create): every slab keeps the part it owns.  add raises
        PfError with code 4, and changes nothing, while any slab is inside a blocked pass."""
        return BandAccumulator(self, "pf_multi", lo, hi, stride, pre_sos, band_sos, nbin, depth)

    def vector_band_accumulator(self, lo, hi, stride=(1, 1, 1), comp=(0,), pre_sos=None, band_sos=None, prod=((0, 0, 0),), nbin=1, depth=0):
        """Band-filtered products of components of the whole scene's field in time bins (pf_multi_vband_create): every slab keeps the part it owns; a
        difference across a cut reads the slab's ghost plane.  add raises PfError (code PF_ERR_STATE) inside a pair or triple, as accumulator."""
        return VectorBandAccumulator(self, "pf_multi", lo, hi, stride, comp, pre_sos, band_sos, prod, nbin, depth)

    def decimating_recorder(self, lo, hi, stride=(1, 1, 1), pre_sos=None, taps=None, factor=1, cap=0, depth=0):
        """Low-pass filtered, decimated frames of a region of the whole scene (pf_multi_decim_create): every slab keeps the part it owns.  add raises
        PfError (code 4) and takes no sample while a slab is inside a pair or triple, or when `cap` frames wait unread."""
        return DecimatingRecorder(self, "pf_multi", lo, hi, stride, pre_sos, taps, factor, cap, depth)

    def vector_decimating_recorder(self, lo, hi, stride=(1, 1, 1), comp=(0,), pre_sos=None, taps=None, factor=1, cap=0, depth=0):
        """Low-pass filtered, decimated frames of up to four components of a region of the whole scene (pf_multi_vdecim_create): every slab keeps the
        part it owns, a difference across a cut reads the slab's ghost plane.  add raises PfError (code 4) where a slab stands inside a pair or triple."""
        return VectorDecimatingRecorder(self, "pf_multi", lo, hi, stride, comp, pre_sos, taps, factor, cap, depth)

    def absorption(self, E, wall_scale, abc_scale, in_scale, nbin=1):
        """The wall absorption maps of the whole scene (pf_multi_absorb_create): every slab accounts the nodes of the planes it owns.  add raises
        PfError with code 4, and changes nothing, while any slab is inside a blocked pass."""
        return Absorption(self, "pf_multi", E, wall_scale, abc_scale, in_scale, nbin)

    def slab(self, g):
        """-> dict(x0, x1, device, paired, steps_per_pass, engine): engine = a non-owning HipEngine view of slab g's engine (state_grids, timing)"""
        x0, x1, dev, pr, eh = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_void_p()
        _check(lib().pf_multi_get_slab(self._h, int(g), ctypes.byref(x0), ctypes.byref(x1), ctypes.byref(dev), ctypes.byref(pr), ctypes.byref(eh)))
        # (the C chain reports 0 = single steps, 1 = pairs, 3 = triples: here `paired` is strictly a boolean, `steps_per_pass` 0 / 2 / 3)
        spp = {0: 0, 1: 2, 3: 3}.get(int(pr.value), 2)
        return {"x0": x0.value, "x1": x1.value, "device": dev.value, "paired": spp > 0, "steps_per_pass": spp, "engine": _EngineView(eh, self.sd.real_bytes)}

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().pf_multi_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _EngineView:
    """Borrowed handle of an engine owned by a HipMulti: inspection calls only."""

    def __init__(self, handle, real_bytes):
        self._h = handle
        self.dtype = np.float32 if real_bytes == 4 else np.float64

    state_grids = lambda self: HipEngine.state_grids(self)  # noqa: E731
    layout = lambda self: HipEngine.layout(self)  # noqa: E731
    timing = lambda self, reset=False: HipEngine.timing(self, reset)  # noqa: E731
    sync = lambda self: HipEngine.sync(self)  # noqa: E731
    set_timing = lambda self, on: HipEngine.set_timing(self, on)  # noqa: E731
    get_region = lambda self, which, lo, hi, stride=(1, 1, 1): HipEngine.get_region(self, which, lo, hi, stride)  # noqa: E731  (the slab's LOCAL coordinates)


def slab_partition(sd, nslabs, even=False, wall_scale=1.0, along_z=False):
    """Owned plane ranges [(x0, x1)] of pf_run_sim_devices' slabs (wall_scale: factor on the wall planes' weights; along_z: the cut
    along FILE Z of rooms stored with exchanged axes).  Host code only: works without a device."""
    s = sd.as_struct()
    cuts = (ctypes.c_int64 * (nslabs + 1))()
    _check(lib().pf_slab_partition_axis(ctypes.byref(s), int(nslabs), int(bool(even)), float(wall_scale), int(bool(along_z)), cuts))
    return [(int(cuts[g]), int(cuts[g + 1])) for g in range(nslabs)]


def slab_wall_scale(sd, nslabs, device=0, **opts):
    """pf_slab_wall_scale: the factor on the wall planes' weights measured for this scene on `device` (None: not measured)."""
    s = sd.as_struct()
    o = _multi_opts(0, opts)
    k = float(lib().pf_slab_wall_scale(ctypes.byref(s), int(nslabs), int(device), ctypes.byref(o)))
    return k if k > 0 else None


class HipEngine:
    """One engine instance = one grid (or one Z-slab) resident on one MI355X."""

    def __init__(self, sd, device=0, numerics=PF_NUM_CPU_EXACT, slab_first=True, slab_last=True, air_variant=0,
                 air_chunk=0, timing=False, readout_chunk=0, ext_u0=None, ext_u1=None, debug=0, x_global0=0, energy=False, layout=0):
        L = lib()
        self.sd = sd
        self._s = sd.as_struct()
        o = PfOpts()
        L.pf_opts_default(ctypes.byref(o))
        o.device, o.numerics = int(device), int(numerics)
        o.slab_first, o.slab_last = int(bool(slab_first)), int(bool(slab_last))
        o.air_variant, o.air_chunk, o.timing, o.readout_chunk = int(air_variant), int(air_chunk), int(bool(timing)), \
            int(readout_chunk)
        o.x_global0 = int(x_global0)
        o.layout = int(layout)
        o.energy = int(bool(energy))
        if ext_u0 is not None and ext_u1 is not None:
            o.ext_u0, o.ext_u1 = int(ext_u0), int(ext_u1)
        self._h = ctypes.c_void_p()
        _set_hooks(debug=debug)
        _check(L.pf_engine_create(ctypes.byref(self._s), ctypes.byref(o), ctypes.byref(self._h)))
        self.dtype = np.float32 if sd.real_bytes == 4 else np.float64

    def run(self, n0, nsteps):
        _check(lib().pf_engine_run(self._h, int(n0), int(nsteps)))

    def step_begin(self, n):
        _check(lib().pf_engine_step_begin(self._h, int(n)))

    def step_end(self, n):
        _check(lib().pf_engine_step_end(self._h, int(n)))

    def halo_ptrs(self):
        vp = ctypes.c_void_p
        slo, shi, rlo, rhi, nb = vp(), vp(), vp(), vp(), ctypes.c_size_t()
        _check(lib().pf_engine_halo_ptrs(self._h, ctypes.byref(slo), ctypes.byref(shi), ctypes.byref(rlo),
                                         ctypes.byref(rhi), ctypes.byref(nb)))
        return slo.value, shi.value, rlo.value, rhi.value, nb.value

    def state_grids(self):
        """Device pointers (u^{n-1}, u^n) of the state grids between runs (pf_engine_state_grids)."""
        vp = ctypes.c_void_p
        up, uc = vp(), vp()
        _check(lib().pf_engine_state_grids(self._h, ctypes.byref(up), ctypes.byref(uc)))
        return up.value, uc.value

    def layout(self):
        """-> ((planes, rows, columns) as stored, pitch in elements, exchanged): exchanged = the engine stores the file's x and z
        axes exchanged; a state grid holds planes * rows * pitch elements (pf_engine_layout)."""
        dims, pitch, ex = (ctypes.c_int64 * 3)(), ctypes.c_int64(), ctypes.c_int32()
        _check(lib().pf_engine_layout(self._h, dims, ctypes.byref(pitch), ctypes.byref(ex)))
        return (int(dims[0]), int(dims[1]), int(dims[2])), int(pitch.value), bool(ex.value)

    def place_grids(self, ptrs):
        """Offer a pool of >= 4 zero-filled caller-owned grids to a slab engine (pf_engine_place_grids).  -> (paired, idx):
        idx[0:2] = positions of the state grids in the pool, idx[2:4] = the spares (or -1 when it steps singly)."""
        arr = (ctypes.c_void_p * len(ptrs))(*[int(p) for p in ptrs])
        idx = (ctypes.c_int32 * 4)()
        _check(lib().pf_engine_place_grids(self._h, arr, len(ptrs), idx))
        return idx[2] >= 0, list(idx)

    def place_grids5(self, ptrs):
        """The same with room for triples (pf_engine_place_grids5).  -> (steps per pass: 3 triples, 2 pairs, 0 single steps; idx[0:5]):
        idx[2:4] = the grids the blocked kernel writes, idx[4] = the u^{n+1} grid of the triples (or -1)."""
        arr = (ctypes.c_void_p * len(ptrs))(*[int(p) for p in ptrs])
        idx = (ctypes.c_int32 * 5)()
        _check(lib().pf_engine_place_grids5(self._h, arr, len(ptrs), idx))
        return (3 if idx[4] >= 0 else (2 if idx[2] >= 0 else 0)), list(idx)

    def set_spares(self, ptr2, ptr3):
        """Two more caller-owned state grids: lets a slab engine step in temporally blocked pairs.  -> True if it will."""
        rc = lib().pf_engine_set_spares(self._h, ctypes.c_void_p(ptr2), ctypes.c_void_p(ptr3))
        if rc not in (0, 1):
            _check(rc)
        return rc == 0

    def stream(self, which):
        return lib().pf_engine_stream(self._h, int(which))

    def sync(self):
        _check(lib().pf_engine_sync(self._h))

    def flush_outputs(self):
        _check(lib().pf_engine_flush_outputs(self._h))

    def get_grid(self, which):
        a = np.empty((self.sd.Nx, self.sd.Ny, self.sd.Nz), dtype=self.dtype)
        _check(lib().pf_engine_get_grid(self._h, int(which), a.ctypes.data_as(ctypes.c_void_p)))
        return a

    def get_region(self, which, lo, hi, stride=(1, 1, 1)):
        """A strided box of u^{n-1} (which = 0) or u^n (1) without copying the grid (pf_engine_get_region): the cells lo + k * stride < hi in
        FILE coordinates, as get_grid(which)[lo[0]:hi[0]:stride[0], lo[1]:hi[1]:stride[1], lo[2]:hi[2]:stride[2]]."""
        return _get_region(lib().pf_engine_get_region, self._h, self.dtype, which, lo, hi, stride)

    def accumulator(self, lo, hi, stride=(1, 1, 1), nchan=1, depth=0):
        """Running sums of the region's cells over the steps, on the device (pf_engine_accum_create): an Accumulator whose add(w) takes u^n --
        get_region(1, lo, hi, stride) at the same moment -- as acc[m] += w[m] * double(u^n).  depth: samples folded in together (0: the default)."""
        return Accumulator(self, "pf_engine", lo, hi, stride, nchan, depth)

    def band_accumulator(self, lo, hi, stride=(1, 1, 1), pre_sos=None, band_sos=None, nbin=1, depth=0):
        """Per cell of the region, on the device (pf_engine_bandacc_create): u^n through the second-order sections pre_sos [npre, 6] and, per band,
        band_sos [nband, nsec, 6] (scipy's rows, a0 = 1), squared, summed into the time bin given to add(bin) -- a BandAccumulator."""
        return BandAccumulator(self, "pf_engine", lo, hi, stride, pre_sos, band_sos, nbin, depth)

    def vector_band_accumulator(self, lo, hi, stride=(1, 1, 1), comp=(0,), pre_sos=None, band_sos=None, prod=((0, 0, 0),), nbin=1, depth=0):
        """Per cell of the region, on the device (pf_engine_vband_create): the components comp (0: the cell of u^n, 1 / 2 / 3: its central difference
        along file x / y / z, 4 / 5 / 6: the lattice difference of an FCC grid along file x / y / z) through pre_sos [ncomp, npre, 6] and, per band, band_sos [nband, nsec, 6]; the products prod [nprod, 3] = (i, j, mode) of
        two filtered components summed into the time bin given to add(bin) -- a VectorBandAccumulator."""
        return VectorBandAccumulator(self, "pf_engine", lo, hi, stride, comp, pre_sos, band_sos, prod, nbin, depth)

    def decimating_recorder(self, lo, hi, stride=(1, 1, 1), pre_sos=None, taps=None, factor=1, cap=0, depth=0):
        """Per cell of the region, on the device (pf_engine_decim_create): every sample u^n through the sections pre_sos [npre, 6] and the FIR `taps`,
        every factor-th output kept as a frame, up to `cap` (0: 64) of them between two reads -- a DecimatingRecorder."""
        return DecimatingRecorder(self, "pf_engine", lo, hi, stride, pre_sos, taps, factor, cap, depth)

    def vector_decimating_recorder(self, lo, hi, stride=(1, 1, 1), comp=(0,), pre_sos=None, taps=None, factor=1, cap=0, depth=0):
        """Per cell of the region, on the device (pf_engine_vdecim_create): the components comp (as vector_band_accumulator's) through their own sections
        pre_sos [ncomp, npre, 6] and each through the FIR `taps`, every factor-th output kept as a frame [ncomp, c0, c1, c2] -- a VectorDecimatingRecorder."""
        return VectorDecimatingRecorder(self, "pf_engine", lo, hi, stride, comp, pre_sos, taps, factor, cap, depth)

    def absorption(self, E, wall_scale, abc_scale, in_scale, nbin=1):
        """The energy every step takes out of the room per wall node, per material and time bin, on the device (pf_engine_absorb_create): an
        Absorption whose add(n, bin) is called before step n.  E [Nm, 12]: the materials' loss coefficients; the scales: include/pffdtd_hip.h."""
        return Absorption(self, "pf_engine", E, wall_scale, abc_scale, in_scale, nbin)

    def set_grid(self, which, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert a.size == self.sd.Npts
        _check(lib().pf_engine_set_grid(self._h, int(which), a.ctypes.data_as(ctypes.c_void_p)))

    def save_state(self):
        """The whole state between two steps in its canonical form (pf_engine_save_state): a dict of numpy arrays, u_prev / u_cur
        (Nx, Ny, Nz) in file order, u1b / u2b (Nbl,) and vh1 / gh1 (Nbl, 12) in the order of sd.bnl_ixyz.  The step index and
        the receiver rows before it (sd.u_out) are the caller's."""
        arr, st = _state_arrays(self.sd)
        _check(lib().pf_engine_save_state(self._h, ctypes.byref(st)))
        return arr

    def load_state(self, state):
        """pf_engine_load_state: this engine now holds `state` (from any engine or chain of the same scene and precision);
        continue with run(n, ...)."""
        arr, st = _state_arrays(self.sd, state)
        _check(lib().pf_engine_load_state(self._h, ctypes.byref(st)))

    def energy_cfg(self, h, c, Ts, DEF_list):
        """DEF_list: the materials' (Mb,3) arrays (sim_mats.h5 mat_XX_DEF)."""
        tab = np.zeros((max(len(DEF_list), 1), 12, 3), dtype=np.float64)
        for k, d in enumerate(DEF_list):
            tab[k, :d.shape[0]] = d
        self._DEF = tab
        dp = ctypes.POINTER(ctypes.c_double)
        _check(lib().pf_engine_energy_cfg(self._h, float(h), float(c), float(Ts), tab.ctypes.data_as(dp)))

    def run_energy(self, n0, nsteps, H_tot, E_lost, E_in):
        dp = ctypes.POINTER(ctypes.c_double)
        for a in (H_tot, E_lost, E_in):
            assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
        _check(lib().pf_engine_run_energy(self._h, int(n0), int(nsteps), H_tot.ctypes.data_as(dp),
                                          E_lost.ctypes.data_as(dp), E_in.ctypes.data_as(dp)))

    def timing(self, reset=False):
        t = PfTiming()
        _check(lib().pf_engine_timing(self._h, ctypes.byref(t), int(reset)))
        return {"air_ms_total": t.air_ms_total, "air_launches": t.air_launches, "step_ms_total": t.step_ms_total,
                "steps": t.steps, "tb2_ms_total": t.tb2_ms_total, "tb2_launches": t.tb2_launches, "tb2_cells": t.tb2_cells,
                "tune_ms": list(t.tune_ms), "air_path": t.air_path, "tb2_lw": t.tb2_lw, "tb2_dirty_tiles": t.tb2_dirty_tiles,
                "place_candidates": t.place_candidates, "place_ms": list(t.place_ms), "wall_blocks": list(t.wall_blocks),
                "tb_steps_per_pass": t.tb_steps_per_pass, "wall_bricks": t.wall_bricks, "wall_three_steps": t.wall_three_steps, "wall_profile": t.wall_profile,
                "wall_uniform_branches": t.wall_uniform_branches, "wall_unread_skipped": t.wall_unread_skipped, "wall_strips_staged": t.wall_strips_staged,
                "fcc_shell_bricks": t.fcc_shell_bricks}

    def set_timing(self, on):
        _check(lib().pf_engine_set_timing(self._h, int(bool(on))))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().pf_engine_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
