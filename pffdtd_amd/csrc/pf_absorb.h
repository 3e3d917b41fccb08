// pf_absorb.h -- device side of the wall absorption maps (include/pffdtd_hip.h: pf_absorb): the energy one time step takes out of the room, split
// per frequency-dependent node, per material and per time bin, with the loss at the open boundary (the ABC nodes) and the energy the sources put in
// beside it.  The terms are the reference Python engine's E_lost and E_in (python/fdtd/sim_fdtd.py:615-620), taken BETWEEN two steps from what
// is in memory there on every path: the branch currents vh1 (pf::st_idx layout) against a copy of the step before, and u^n against the kept
// u^{n-2} at the ABC and source nodes.  One streaming pass over the node list per sample: no ring, nothing to fold later.
//   prev      Real   [round_up(Nbl, 64) * 12]  vh1 at the sample before, same layout
//   node_sum  double [Nbl]                     running loss per node, ENGINE order (get / set permute through the engine's lperm)
//   bins      double [nbin][Nm + 2]            per time bin: the materials' rows, then the open boundary's, then the input's
//   part      double [blocks][slots]           one sample's partial sums per workgroup (k_absorb_fold adds them in block order)
// Determinism: no floating-point atomics.  A node's loss is summed over its branches in ascending order without contraction (__dmul_rn / __dadd_rn);
// a workgroup's sum per material is a fixed xor-butterfly over each wave (lanes of another material contribute +0.0, which changes no bit), once per material present in the wave, and
// the waves added in wave order; k_absorb_fold adds the workgroups' partials in 64 contiguous runs, in order, and the 64 run sums by the same
// butterfly.  The order depends on the node order and the node count alone, so the same run gives the same bits, and a resumed run the bits of
// the one-piece run.
// Traffic of the wall kernel per node with Mb branches: vh1 and prev read, prev written (3 * Mb Reals), node_sum read and written (16 B), ssaf and
// the material (sizeof(Real) + 1): 149 B at Mb = 11 in fp32.  Plain C++, wave64, no assumption about Nbl % 64.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "pffdtd_hip.h"
#include "pf_kernels.h"

namespace pf {

constexpr int ABS_WG = 256; // lanes per workgroup of the sample kernels: four waves

// the sum of v over the 64 lanes of a wave, in every lane: a fixed tree
__device__ __forceinline__ double absorb_wave_sum(double v) {
#pragma unroll
   for (int off = 32; off > 0; off >>= 1) v = __dadd_rn(v, __shfl_xor(v, off, 64));
   return v;
}
// s: the wave's sum; the workgroup's sum, waves in order, to *dst (called once per kernel, by all lanes; `lds` holds ABS_WG / 64 doubles)
__device__ __forceinline__ void absorb_block_store(double s, double *lds, double *dst) {
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   if (lane == 0) lds[wave] = s;
   __syncthreads();
   if (threadIdx.x == 0) {
      double t = lds[0];
      for (int w = 1; w < ABS_WG / 64; w++) t = __dadd_rn(t, lds[w]);
      *dst = t;
   }
}

// One lane per frequency-dependent node.  E: [Nm][12] loss coefficients; scale: V_fac * 0.25 * h / l.  account = 0: the first sample, prev <- vh1 only.
template <typename Real>
static __global__ void __launch_bounds__(ABS_WG) k_absorb_wall(const Real *__restrict__ vh1, Real *__restrict__ prev, const Real *__restrict__ ssaf, const int8_t *__restrict__ mat,
                                                               const int8_t *__restrict__ Mb, const double *__restrict__ E, int64_t Nbl, int Nm, double scale, int account,
                                                               double *__restrict__ node_sum, double *__restrict__ part) {
   __shared__ double lds[ABS_WG / 64][PF_MNM];
   const int64_t li = (int64_t)blockIdx.x * ABS_WG + threadIdx.x;
   const bool live = li < Nbl;
   const int k = live ? (int)mat[li] : -1;
   const int M = live ? (int)Mb[k] : 0;
   double s = 0.0;
   for (int m = 0; m < M; m++) { // (a wave reads one contiguous 64-lane row per branch and array)
      const int64_t j = st_idx(m, li);
      const Real vn = vh1[j];
      if (account) {
         const double v = __dadd_rn((double)prev[j], (double)vn);
         s = __dadd_rn(s, __dmul_rn(__dmul_rn(v, v), E[k * 12 + m]));
      }
      prev[j] = vn;
   }
   if (!account) return; // (uniform over the grid)
   const double e = live ? __dmul_rn(scale, __dmul_rn((double)ssaf[li], s)) : 0.0;
   if (live) node_sum[li] = __dadd_rn(node_sum[li], e); // the owning lane: a plain read-modify-write
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   for (int q = lane; q < Nm; q += 64) lds[wave][q] = 0.0; // (the wave's own row: its later stores follow in program order)
   unsigned long long todo = __ballot(live);
   while (todo) { // the materials PRESENT in the wave, in the order of their first lane: the wave's masked sum of each
      const int q = __shfl(k, __ffsll(todo) - 1, 64);
      const bool mine = k == q;
      const double w = absorb_wave_sum(mine ? e : 0.0);
      if (lane == 0) lds[wave][q] = w;
      todo &= ~__ballot(mine);
   }
   __syncthreads();
   if ((int)threadIdx.x < Nm) { // the workgroup's sums, waves in order
      double t = lds[0][threadIdx.x];
      for (int w = 1; w < ABS_WG / 64; w++) t = __dadd_rn(t, lds[w][threadIdx.x]);
      part[(int64_t)blockIdx.x * Nm + threadIdx.x] = t;
   }
}

// One lane per ABC node: coef * (u^n - kept u^{n-2})^2 with coef = 2^-Q * Q (exact); keep <- u^{n-1}.  scale: 0.5 * V_fac * h / l.
template <typename Real>
static __global__ void __launch_bounds__(ABS_WG) k_absorb_abc(const Real *__restrict__ u0, const Real *__restrict__ u1, const int64_t *__restrict__ idx, const int8_t *__restrict__ Q,
                                                              int64_t n, double scale, int account, Real *__restrict__ keep, double *__restrict__ part) {
   __shared__ double lds[ABS_WG / 64];
   const int64_t i = (int64_t)blockIdx.x * ABS_WG + threadIdx.x;
   double e = 0.0;
   if (i < n) {
      const int64_t jj = idx[i];
      if (account) {
         const double d = __dadd_rn((double)u1[jj], -(double)keep[i]), q = (double)Q[i];
         e = __dmul_rn(scale, __dmul_rn(ldexp(q, -(int)Q[i]), __dmul_rn(d, d)));
      }
      keep[i] = u0[jj];
   }
   if (!account) return;
   absorb_block_store(absorb_wave_sum(e), lds, part + blockIdx.x);
}

// One lane per source node: (u^n - kept u^{n-2}) * the sample the engine added at step n - 1; keep <- u^{n-1}.  scale: 0.5 * V_fac * h / l2.
template <typename Real>
static __global__ void __launch_bounds__(ABS_WG) k_absorb_in(const Real *__restrict__ u0, const Real *__restrict__ u1, const int64_t *__restrict__ idx, const Real *__restrict__ in_sigs,
                                                             int64_t Ns, int64_t Nt, int64_t step, double scale, int account, Real *__restrict__ keep, double *__restrict__ part) {
   __shared__ double lds[ABS_WG / 64];
   const int64_t i = (int64_t)blockIdx.x * ABS_WG + threadIdx.x;
   double e = 0.0;
   if (i < Ns) {
      const int64_t jj = idx[i];
      if (account) {
         const double d = __dadd_rn((double)u1[jj], -(double)keep[i]);
         e = __dmul_rn(scale, __dmul_rn(d, (double)in_sigs[i * Nt + step]));
      }
      keep[i] = u0[jj];
   }
   if (!account) return;
   absorb_block_store(absorb_wave_sum(e), lds, part + blockIdx.x);
}

// dst[slot] += the sum over the workgroups b of part[b * nslot + slot]: one wave per slot; lane j adds the partials of run j (contiguous, in order), the
// runs' sums go through the butterfly
static __global__ void __launch_bounds__(64) k_absorb_fold(const double *__restrict__ part, int64_t nblocks, int nslot, double *__restrict__ dst) {
   const int slot = blockIdx.x, lane = threadIdx.x;
   const int64_t run = (nblocks + 63) / 64, b0 = lane * run, b1 = b0 + run < nblocks ? b0 + run : nblocks;
   double s = 0.0;
   for (int64_t b = b0; b < b1; b++) s = __dadd_rn(s, part[b * nslot + slot]);
   s = absorb_wave_sum(s);
   if (lane == 0) dst[slot] = __dadd_rn(dst[slot], s);
}

// node sums between engine order and the order of sd->bnl_ixyz (perm[li] = the file row of engine node li, as k_state_pack)
static __global__ void k_absorb_rows(double *__restrict__ eng, double *__restrict__ file, const int64_t *__restrict__ perm, int64_t Nbl, int to_file) {
   const int64_t li = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   if (li >= Nbl) return;
   if (to_file) file[perm[li]] = eng[li]; else eng[li] = file[perm[li]];
}

} // namespace pf
