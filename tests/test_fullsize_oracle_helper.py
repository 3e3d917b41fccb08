"""The oracle half of tests/fullsize_oracle.py on the CPU (scene with mask, seeded in-place fill, K oracle steps, finite and non-zero
receivers) and the report its comparison gives -- so that the plumbing of tests/test_hip_fullsize_oracle.py is exercised without a GPU."""
import numpy as np
import pytest

import fullsize_oracle as fo
from pffdtd_amd import sim_data, synth


def _make(prec, n=(40, 44, 52), K=5):
    sim = synth.shoebox(*n, Nt=K, Nm=2, Mb=[11, 3], rcv=[[20, 22, 30], [4, 20, 25], [30, n[1] - 6, 25]])

    def make(mask):
        sd = sim_data.SimData.from_sim(sim, prec, build_mask=mask)
        sd.scale_input()
        return sd
    return make


@pytest.mark.parametrize("prec", ["single", "double"])
def test_fill_is_seeded_in_range_and_covers_every_cell(prec):
    e, sd = fo.oracle_half(_make(prec), 5, seed=7)
    g = [e.grid(k).copy() for k in (0, 1)]
    e2, _ = fo.oracle_half(_make(prec), 5, seed=7)
    e3, _ = fo.oracle_half(_make(prec), 5, seed=8)
    for k in (0, 1):
        assert g[k].dtype == sd.real and g[k].shape == (sd.Nx, sd.Ny, sd.Nz)
        assert np.abs(g[k]).max() <= 1e-3 * (1 + 1e-6) and np.abs(g[k]).max() > 0.99e-3 and abs(g[k].mean()) < 2e-5
        assert (g[k] != 0).mean() > 0.999  # ghost layer, shell, walls, box: all live
        assert np.array_equal(g[k], e2.grid(k)) and not np.array_equal(g[k], e3.grid(k))
    assert not np.array_equal(g[0], g[1])
    for x in (e, e2, e3):
        x.close()


def test_oracle_half_steps_and_every_receiver_hears_the_field():
    e, sd = fo.oracle_half(_make("single"), 5, seed=3)
    before = e.grid(1).copy()
    fo.step_oracle(e, 5)
    out = sd.u_out[:, :5]
    assert np.isfinite(out).all() and (np.abs(out).max(axis=1) > 0).all()
    assert np.isfinite(e.grid(1)).all() and not np.array_equal(e.grid(1), before)
    e.close()


def test_comparison_reports_the_first_cell_both_values_and_the_count():
    rng = np.random.default_rng(1)
    ref = rng.random((40, 9, 11), dtype=np.float32)
    got = ref.copy()
    got[0], got[:, 0], got[:, :, -1] = 5, 6, 7  # the ghost layer is not compared
    fo.compare_interior(fo.host_blocks(got), ref, "grid 0")
    got[33, 2, 5] = np.nextafter(got[33, 2, 5], np.float32(2))  # one bit, in the third x block
    got[17, 7, 9] += 1
    got[17, 3, 1] = -got[17, 3, 1]
    with pytest.raises(fo.Mismatch) as ex:
        fo.compare_interior(fo.host_blocks(got), ref, "grid 0")
    msg = str(ex.value)
    assert "grid 0: 3 of 2394 interior cells differ" in msg and "(x, y, z) = (17, 3, 1)" in msg, msg
    assert repr(got[17, 3, 1]) in msg and repr(ref[17, 3, 1]) in msg, msg
