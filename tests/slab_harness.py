"""The slab chain's Python path on the CPU, shared by tests/test_slab_exchange.py and tests/test_io_lists.py: a slab stepper backed by the
CPU oracle and the in-process time loop that copies the ghost planes directly."""
import contextlib

import numpy as np
import torch

import oracle
from pffdtd_amd import slab


class OracleSlabStepper:
    """Same interface as pffdtd_amd.dist.HipSlabStepper, backed by oracle.Engine (CPU, tests only)."""

    def __init__(self, loc, info):
        self.loc, self.info = loc, info
        self.zcut = bool(getattr(info, "along_z", False))  # a chain cut along file z: the exchanged "planes" are z columns
        self.e = oracle.Engine(loc, slab_first=info.first, slab_last=info.last, along_z=self.zcut)
        self._staged = None

    def step_begin(self, n):
        self.e.step(n)  # whole step; the new state is u1 after the rotation
        self._staged = None

    def halo_tensors(self):
        g = self.e.grid(1)
        if self.zcut:  # strided in the file layout: staged through contiguous buffers, written back in step_end
            if self._staged is None:
                Nz = self.loc.Nz
                c = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1))  # noqa: E731
                self._staged = (c(g[:, :, 1]), c(g[:, :, Nz - 2]), c(g[:, :, 0]), c(g[:, :, Nz - 1]))
            return self._staged
        Nx = self.loc.Nx
        f = lambda a: torch.from_numpy(a.reshape(-1))  # noqa: E731  (views: irecv writes in place)
        return f(g[1]), f(g[Nx - 2]), f(g[0]), f(g[Nx - 1])

    def comm_context(self):
        return contextlib.nullcontext()

    def step_end(self, n):
        if self.zcut and self._staged is not None:
            g = self.e.grid(1)
            if not self.info.first:
                g[:, :, 0] = self._staged[2].numpy().reshape(g.shape[0], g.shape[1])
            if not self.info.last:
                g[:, :, -1] = self._staged[3].numpy().reshape(g.shape[0], g.shape[1])

    def finish(self):
        pass


def run_in_process(sd, G, along_z, balance=None):
    """G slabs of `sd` in one process, planes copied directly -> the merged u_out (sd.u_out, filled in place)"""
    balance = (G == 3) if balance is None else balance
    parts = [slab.split(sd, G, r, balance=balance, along_z=along_z) for r in range(G)]
    st = [OracleSlabStepper(loc, info) for loc, info in parts]
    for n in range(sd.Nt):
        for s in st:
            s.step_begin(n)
        planes = [s.halo_tensors() for s in st]
        for r in range(G - 1):
            planes[r + 1][2].copy_(planes[r][1])      # my last updated plane -> right neighbour's low ghost
            planes[r][3].copy_(planes[r + 1][0])      # right neighbour's first updated plane -> my high ghost
        for s in st:
            s.step_end(n)
    return slab.merge_outputs(sd, [p[0] for p in parts])
