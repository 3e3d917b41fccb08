"""The Z-slab time loop (pffdtd_amd/slab.py + pffdtd_amd/dist.py) on CPU: world_size-2/3 gloo processes, each
slab stepped by the CPU ORACLE (test infrastructure standing in for the HIP stepper), must reproduce the
single-domain oracle bit for bit.  This covers the partition, the index re-basing, the exchange schedule and the
output merge -- everything of the N>1 path except the HIP kernels themselves (covered by -m gpu tests).
"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import cases
import oracle
from pffdtd_amd import dist as pdist
from pffdtd_amd import slab
from slab_harness import OracleSlabStepper, run_in_process


def _reference(name, prec):
    sd = cases.make_sd(name, prec)
    oracle.run_sim(sd)
    return sd.u_out.copy()


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("name,prec", [("cart_outside", "single"), ("fcc2_outside", "double"), ("cart_lossy", "double")])
@pytest.mark.parametrize("along_z", [False, True])
def test_in_process_slabs_equal_single_domain(name, prec, G, along_z):
    """G slabs in one process, planes copied directly: isolates slab.split from the transport.  along_z: the chain cut along
    FILE Z (what rooms get: their engines store the x and z axes exchanged)."""
    ref = _reference(name, prec)
    sd = cases.make_sd(name, prec)
    out = run_in_process(sd, G, along_z)  # (balance=(G == 3): the cost-balanced cut for three slabs, the even one for two)
    assert np.array_equal(out, ref)


def _worker(rank, world, port, name, prec, q, along_z=False):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        oracle.lib().oracle_set_threads(2)
        sd = cases.make_sd(name, prec)
        loc, info = slab.split(sd, world, rank, along_z=along_z)
        runner = pdist.SlabRunner(OracleSlabStepper(loc, info), info)
        runner.verify_steps = sd.Nt  # checksum every exchange against the senders' planes (bench.py does a few)
        runner.run(0, sd.Nt)
        runner.finish()
        verified = runner.exchange_verified
        # the check must also be able to FAIL: corrupt one received plane on the last rank and look again
        if rank == world - 1:
            runner.st.halo_tensors()[2][3] += 1.0
        runner._verify_exchange()
        caught = runner.exchange_verified is False
        out = pdist.gather_outputs(sd, loc, info)
        if rank == 0:
            q.put((out.copy(), verified, caught))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("along_z", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_gloo_slab_chain_equals_single_domain(world, along_z):
    name, prec = "cart_outside", "single"
    ref = _reference(name, prec)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000) + world + (10 if along_z else 0)
    procs = [ctx.Process(target=_worker, args=(r, world, port, name, prec, q, along_z)) for r in range(world)]
    for p in procs:
        p.start()
    out, verified, caught = q.get(timeout=240)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert np.array_equal(out, ref)
    assert verified is True and caught is True
