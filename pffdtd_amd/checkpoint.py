"""Checkpoint files: a run's whole state between two steps, in one HDF5 file.

    write(path, sd, n, state)          state = HipEngine.save_state() / HipMulti.save_state() taken before step n
    read(path, sd) -> (n, state, u_out)

The file holds the six arrays of the canonical state (include/pffdtd_hip.h: pf_state), the step index n the run continues at, the
receiver rows so far (sd.u_out, raw: before rescale_output) and a fingerprint of the scene: its sizes and precision, and a SHA-256 of
each list the state's meaning hangs on.  `read` refuses a file whose fingerprint is not the scene's, and says which field differs.
A file is written under `path + ".tmp"` and moved into place with os.replace: a writer that is killed never leaves half a file under
the real name, and a leftover .tmp is never read.
"""
import hashlib
import os

import numpy as np

from . import h5io
from .engine import STATE_KEYS

SIZES = ("Nx", "Ny", "Nz", "Nt", "Nb", "Nbl", "Ns", "Nr", "Nm", "fcc_flag", "real_bytes")
HASHED = ("bn_ixyz", "adj_bn", "bnl_ixyz", "mat_bnl", "ssaf_bnl", "in_ixyz", "out_ixyz", "in_sigs", "Mb", "mat_quads", "mat_beta")  # (vox_out, comms_out, sim_mats)
FORMAT = 1


class CheckpointMismatch(ValueError):
    pass


def fingerprint(sd):
    """-> {field: int | 32 bytes}: the sizes, and per hashed list the SHA-256 of its dtype, shape and bytes"""
    fp = {k: int(getattr(sd, k)) for k in SIZES}
    for k in HASHED:
        a = np.ascontiguousarray(getattr(sd, k))
        h = hashlib.sha256(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.tobytes())
        fp["sha256_" + k] = h.digest()
    return fp


def write(path, sd, n, state):
    path = os.fspath(path)
    tmp = path + ".tmp"
    real = np.float32 if sd.real_bytes == 4 else np.float64
    h5io.write(tmp, "format", np.int64(FORMAT), append=False)
    h5io.write(tmp, "n", np.int64(n))
    for k, v in fingerprint(sd).items():
        h5io.write(tmp, k, np.frombuffer(v, dtype=np.uint8) if isinstance(v, bytes) else np.int64(v))
    for k in STATE_KEYS:
        a = np.asarray(state[k])
        if a.dtype != real:
            raise TypeError(f"state[{k!r}] is {a.dtype}, the scene's precision is {np.dtype(real)}")
        h5io.write(tmp, k, a)
    h5io.write(tmp, "u_out", np.asarray(sd.u_out, dtype=np.float64))
    os.replace(tmp, path)  # the one moment the file appears under its name


def read(path, sd):
    path = os.fspath(path)
    fmt = int(h5io.read(path, "format"))
    if fmt != FORMAT:
        raise CheckpointMismatch(f"{path}: checkpoint format {fmt}, this version reads {FORMAT}")
    for k, v in fingerprint(sd).items():
        if isinstance(v, bytes):
            got = bytes(np.asarray(h5io.read(path, k, h5io.U8)).tobytes())
            if got != v:
                raise CheckpointMismatch(f"{path}: checkpoint is of another scene: {k[len('sha256_'):]} differs")
        else:
            got = int(h5io.read(path, k))
            if got != v:
                raise CheckpointMismatch(f"{path}: checkpoint is of another scene: {k} is {got} there, {v} here")
    code = h5io.F32 if sd.real_bytes == 4 else h5io.F64
    state = {k: h5io.read(path, k, code) for k in STATE_KEYS}
    u_out = h5io.read(path, "u_out", h5io.F64)
    return int(h5io.read(path, "n")), state, u_out
