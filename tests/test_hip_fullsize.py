"""GPU, large grids: size-independent properties and agreement between the kernel families.  (Point-wise oracle parity of the default path at
1024^3 ... 1536^3 is tests/test_hip_fullsize_oracle.py's; what this module adds is the agreement of ALL families with each other, also
beyond 2^32 CELLS -- 4224 x 1024 x 1024 -- which the oracle cases do not reach, linearity and causality.)
  * three independent interior-kernel families (lean fused / barrier-free marching / naive one-thread-per-cell) must
    produce identical bits on a 512^3 lossy room;
  * linearity: doubling the input doubles every receiver sample exactly (power-of-two scaling is exact in fp);
  * causality: nothing arrives at a receiver before the wave front can (one cell per step at most).
"""
import numpy as np
import pytest

from pffdtd_amd import engine, sim_data, synth

pytestmark = pytest.mark.gpu
N, NT = 512, 24


@pytest.fixture(scope="module")
def scene():
    sim = synth.shoebox(N, N, N, Nt=NT, Nm=2, Mb=[11, 3], rcv=[[N // 2 + 3, N // 2, N // 2 - 2], [N // 2 + 40, N // 2, N // 2]])
    sd = sim_data.SimData.from_sim(sim, "single", build_mask=False)
    sd.scale_input()
    return sd


def _run(sd, **kw):
    sd.u_out[:] = 0
    eng = engine.HipEngine(sd, **kw)
    eng.run(0, sd.Nt)
    plane = eng.get_grid(1)[N // 2].copy()
    eng.close()
    return sd.u_out.copy(), plane


def test_kernel_families_agree_bitwise_at_512(scene):
    ref_out, ref_plane = _run(scene, air_variant=3)  # the reference's kernel sequence: memory flips, marching kernel, ABC lists
    assert np.abs(ref_out).max() > 0
    for v in (0, 4, 25, 40, 3 + 256):  # 40: temporally blocked pairs (auto keeps them for >= 600-cell cross-sections)
        out, plane = _run(scene, air_variant=v)
        assert np.array_equal(out, ref_out), f"variant {v}"
        assert np.array_equal(plane[1:-1, 1:-1], ref_plane[1:-1, 1:-1]), f"variant {v}"


def test_linearity_and_causality_at_512(scene):
    out1, _ = _run(scene)
    keep = scene.in_sigs.copy()
    scene.in_sigs *= 2.0
    out2, _ = _run(scene)
    scene.in_sigs[:] = keep
    assert np.array_equal(out2, 2.0 * out1)
    # receiver 2 sits 40 cells from the source cell: silent for at least the first 38 samples
    far = out1[8:16]
    assert not far[:, :38].any() and np.abs(out1[0:8, :12]).max() > 0


def test_fcc_kernel_families_agree_beyond_2p32_cells():
    """The same for the 13-point folded-FCC kernels (auto = barrier-free with in-kernel ABC, unfused, virtual-ghost, naive)
    on a stored grid of 4224 x 1024 x 1024."""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, str(root / "tools" / "big_grid_check.py"), "--fcc", "4224", "1024", "1024", "8"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "big-grid check OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def test_kernel_families_agree_beyond_2p32_cells():
    """4224 x 1024 x 1024 = 1.03 x 2^32 cells (35 GB of state, source and receivers at linear indices beyond 2^32):
    blocked pairs, lean single steps, barrier-free and unfused kernels leave identical bits in every cell
    (tools/big_grid_check.py, random initial fields; needs ~150 GB of device memory)."""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, str(root / "tools" / "big_grid_check.py"), "4224", "1024", "1024", "10"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "big-grid check OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    import re
    m = re.search(r"variant 40: .* blocked launches (\d+)", r.stdout)
    assert m and int(m.group(1)) > 0, r.stdout[-1500:]  # the blocked pairs really ran


def _tool(args, timeout=1500):
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    return subprocess.run([sys.executable, str(root / "tools" / args[0])] + args[1:], capture_output=True, text=True, timeout=timeout)


def test_fp64_fcc_kernel_families_agree_at_1536_cubed():
    """BASELINE configs[4] on one GPU: folded FCC fp64, stored grid 1536^3 = 0.84 x 2^32 cells, 58 GB of state -- the
    64-bit index arithmetic of the fp64 13-point kernels (pitch 1536, 2.36e6-element planes, offsets beyond 2^31 BYTES
    from plane 114 on, beyond 2^32 bytes from plane 228 on): the families agree on every cell."""
    r = _tool(["big_grid_check.py", "--fcc", "--double", "1536", "1536", "1536", "6"])
    assert r.returncode == 0 and "big-grid check OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


@pytest.mark.parametrize("name", ["ctk_cart_gpu", "mv_fcc_gpu"])
def test_reference_configurations_at_full_size(name):
    """BASELINE configs[1] (CTK 894x579x309, 7-point) and configs[2] (Musikverein 2852x552x850 folded, 13-point) built from
    the reference's scene exports on this box: kernel families agree on every cell and receiver."""
    r = _tool(["config_family_check.py", name, "10"])
    assert r.returncode == 0 and "config family check OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
