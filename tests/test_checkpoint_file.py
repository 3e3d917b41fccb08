"""CPU: checkpoint files (pffdtd_amd/checkpoint.py) -- round trip, scene fingerprint, atomic publication."""
import os

import numpy as np
import pytest

import cases
from pffdtd_amd import checkpoint
from pffdtd_amd.engine import STATE_KEYS


def _state(sd, seed):
    """a synthetic state with every bit pattern a run could leave: negative zeros, denormals, huge and tiny values"""
    rng = np.random.default_rng(seed)
    dt = np.float32 if sd.real_bytes == 4 else np.float64
    shapes = {"u_prev": (sd.Nx, sd.Ny, sd.Nz), "u_cur": (sd.Nx, sd.Ny, sd.Nz), "u1b": (sd.Nbl,), "u2b": (sd.Nbl,), "vh1": (sd.Nbl, 12), "gh1": (sd.Nbl, 12)}
    st = {}
    for k in STATE_KEYS:
        a = (rng.standard_normal(shapes[k]) * 10.0 ** rng.integers(-30, 30, size=shapes[k])).astype(dt)
        a.reshape(-1)[::7] = -0.0
        a.reshape(-1)[3::11] = np.finfo(dt).tiny / 4  # a denormal
        st[k] = a
    return st


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("prec", ["single", "double"])
def test_a_checkpoint_file_round_trips_bit_for_bit(tmp_path, prec):
    sd = cases.make_sd("cart_mb11", prec)
    assert sd.Nbl > 0
    st = _state(sd, 5)
    sd.u_out[...] = np.random.default_rng(6).standard_normal(sd.u_out.shape) * 1e-300
    p = tmp_path / "ck.h5"
    checkpoint.write(p, sd, 31, st)
    assert not os.path.exists(str(p) + ".tmp")
    n, got, u_out = checkpoint.read(p, cases.make_sd("cart_mb11", prec))  # (a scene built anew: the fingerprint is of its contents)
    assert n == 31
    for k in STATE_KEYS:
        assert got[k].dtype == st[k].dtype and got[k].shape == st[k].shape, k
        assert np.array_equal(_bits(got[k]), _bits(st[k])), k
    assert u_out.shape == sd.u_out.shape and np.array_equal(_bits(u_out), _bits(sd.u_out))


def test_a_checkpoint_of_another_scene_is_refused_by_name(tmp_path):
    sd = cases.make_sd("cart_mb11", "single")
    p = tmp_path / "ck.h5"
    checkpoint.write(p, sd, 12, _state(sd, 7))
    other = cases.make_sd("cart_mb11", "single")
    other.mat_bnl = other.mat_bnl.copy()
    other.mat_bnl[sd.Nbl // 2] ^= 1  # one entry
    with pytest.raises(checkpoint.CheckpointMismatch, match="mat_bnl"):
        checkpoint.read(p, other)
    with pytest.raises(checkpoint.CheckpointMismatch, match="Nt"):
        checkpoint.read(p, cases.make_sd("cart_mb11", "single", Nt=81))
    with pytest.raises(checkpoint.CheckpointMismatch, match="real_bytes"):
        checkpoint.read(p, cases.make_sd("cart_mb11", "double"))
    checkpoint.read(p, cases.make_sd("cart_mb11", "single"))  # (and the scene itself is accepted)


def test_a_state_of_the_wrong_precision_is_not_written(tmp_path):
    sd = cases.make_sd("cart_mb11", "single")
    with pytest.raises(TypeError, match="precision"):
        checkpoint.write(tmp_path / "ck.h5", sd, 3, _state(cases.make_sd("cart_mb11", "double"), 1))
    assert not (tmp_path / "ck.h5").exists()


def test_a_leftover_tmp_file_is_ignored_and_replace_publishes(tmp_path, monkeypatch):
    sd = cases.make_sd("cart_mb11", "single")
    p = tmp_path / "ck.h5"
    st = _state(sd, 9)
    checkpoint.write(p, sd, 20, st)
    good = p.read_bytes()
    (tmp_path / "ck.h5.tmp").write_bytes(b"half a file from a writer that was killed")
    n, got, _ = checkpoint.read(p, sd)  # the leftover next to a good file: not looked at
    assert n == 20 and np.array_equal(_bits(got["vh1"]), _bits(st["vh1"]))
    # a writer that dies before os.replace leaves the good file as it was; os.replace is what publishes the new one
    calls = []

    def dying_replace(src, dst):
        calls.append((os.fspath(src), os.fspath(dst)))
        raise KeyboardInterrupt

    monkeypatch.setattr(checkpoint.os, "replace", dying_replace)
    with pytest.raises(KeyboardInterrupt):
        checkpoint.write(p, sd, 40, _state(sd, 10))
    assert calls == [(str(p) + ".tmp", str(p))]
    assert p.read_bytes() == good
    monkeypatch.undo()
    assert checkpoint.read(p, sd)[0] == 20
    checkpoint.write(p, sd, 40, _state(sd, 10))  # (over the leftover .tmp of the dead writer)
    assert checkpoint.read(p, sd)[0] == 40 and not os.path.exists(str(p) + ".tmp")
