// pf_band.h -- device side of the band accumulators (include/pffdtd_hip.h: pf_bandacc): per cell of a region, the sample u^n runs through a cascade
// of second-order sections -- npre shared ones, then nsec of each of nband bands --, is squared and summed into time bins,
//    x = double(u);  x -> pre sections;  per band b: y = x -> the band's sections;  E[b][bin] = E[b][bin] + y * y
// which is what an energy decay per octave band needs of every cell (pffdtd_amd/decay.py).  A section is b0 b1 b2 a1 a2 (a0 = 1) with state s1, s2
// per cell, transposed direct form II, every operation rounded to double once, NO fma, in exactly this association:
//    y  = b0*x + s1
//    s1 = (b1*x - a1*y) + s2
//    s2 = b2*x - a2*y
// (numpy written with these three lines gives the same bits; the build has -ffp-contract=off and the pragma below says so again.)
//   E     double [nband * nbin][cstride]           cstride = the cell count rounded up to a multiple of 2: every row starts 16-byte aligned
//   st    double [(npre + nband*nsec) * 2][cstride]  s1, s2 of section q in rows 2q, 2q + 1; pre sections first, then band 0's, band 1's, ...
//   coef  double [(npre + nband*nsec) * 5]          uploaded once, at creation
//   ring  Real   [depth][cells]                     the region's cells at the samples not folded in yet (k_region_cut, as pf_accum.h)
//   xpre  double [depth][cstride]                   npre > 0 only: the pending samples after the shared sections
//   bins  int32  [depth]                            the pending samples' bins (-1: filter, sum nothing), uploaded with every fold
// A fold of NT pending samples is k_band_pre<Real, NT> (npre > 0: one thread per two cells runs the shared sections once and writes xpre -- the
// other choice, every band recomputing them, has band b read the shared state while band 0 stores it) and k_band_fold<In, NT> on a grid of
// (cdiv(cdiv(cells, 2), 256), nband): bands in parallel, so a 64^2 plane still fills the chip.  A thread owns two adjacent cells (16-byte loads and
// stores, lanes along cells: whole lines), reads and widens its NT inputs once and walks the sections: two state words per cell loaded, NT samples
// through the section in registers, stored once -- state traffic is 1 / NT of the depth-1 form.  Consecutive samples of one bin are summed in a
// register from the loaded E in call order; a bin change inside a fold stores and loads.  The padding cell of an odd count filters zeros.
// coef[...] and bins[...] do not depend on the lane: scalar loads.  No atomics, no LDS, no scratch (tools/kernel_resources.py k_band).  64-bit
// indices, every access guarded by the cell count (c even and c < cells, so c + 1 < cstride).
//
// The host side is the vector band accumulators' (pf_engine_vband.inc: VBand with one component and one product, whose S, st, coef and ring are
// the arrays above); band_section is also pf_vband.h's and pf_vdecim.h's.
//
// PF_BAND_DEFAULT_DEPTH: the fastest of the measured depths 1, 4, 8, 16 on the plane cases of tools/field_decay_cost.py (profiles/field_decay.txt).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pf {

constexpr int PF_BAND_MAX_BANDS = 16;
constexpr int PF_BAND_MAX_SECTIONS = 8;
constexpr int PF_BAND_MAX_DEPTH = 16;
constexpr int PF_BAND_DEFAULT_DEPTH = 16;

// NT samples of two cells through section q (coefficients k[5], state rows 2q and 2q + 1), in place
template <int NT>
__device__ __forceinline__ void band_section(double *__restrict__ st, const double *__restrict__ k, int64_t q, int64_t c, int64_t cstride, double (&xa)[NT], double (&xb)[NT]) {
#pragma clang fp contract(off)
   const double b0 = k[0], b1 = k[1], b2 = k[2], a1 = k[3], a2 = k[4];
   double2 *p1 = reinterpret_cast<double2 *>(st + (2 * q) * cstride + c), *p2 = reinterpret_cast<double2 *>(st + (2 * q + 1) * cstride + c);
   double2 s1 = *p1, s2 = *p2;
#pragma unroll
   for (int t = 0; t < NT; t++) {
      const double ya = b0 * xa[t] + s1.x, yb = b0 * xb[t] + s1.y;
      s1.x = (b1 * xa[t] - a1 * ya) + s2.x;
      s1.y = (b1 * xb[t] - a1 * yb) + s2.y;
      s2.x = b2 * xa[t] - a2 * ya;
      s2.y = b2 * xb[t] - a2 * yb;
      xa[t] = ya;
      xb[t] = yb;
   }
   *p1 = s1;
   *p2 = s2;
}

// grid: cdiv(cdiv(cells, 2), 256) blocks of 256 threads; npre >= 1
template <typename Real, int NT>
static __global__ void __launch_bounds__(256) k_band_pre(double *__restrict__ st, double *__restrict__ xpre, const Real *__restrict__ ring, const double *__restrict__ coef,
                                                         int64_t cells, int64_t cstride, int npre) {
#pragma clang fp contract(off)
   const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
   if (c >= cells) return;
   const bool two = c + 1 < cells;
   double xa[NT], xb[NT];
#pragma unroll
   for (int t = 0; t < NT; t++) {
      xa[t] = (double)ring[(int64_t)t * cells + c];
      xb[t] = two ? (double)ring[(int64_t)t * cells + c + 1] : 0.0;
   }
   for (int q = 0; q < npre; q++) band_section<NT>(st, coef + 5 * q, q, c, cstride, xa, xb);
#pragma unroll
   for (int t = 0; t < NT; t++) *reinterpret_cast<double2 *>(xpre + (int64_t)t * cstride + c) = make_double2(xa[t], xb[t]);
}

// grid: (cdiv(cdiv(cells, 2), 256), nband) blocks of 256 threads.  x: the ring (xstride = cells) or xpre (xstride = cstride)
template <typename In, int NT>
static __global__ void __launch_bounds__(256) k_band_fold(double *__restrict__ E, double *__restrict__ st, const In *__restrict__ x, const double *__restrict__ coef,
                                                          const int32_t *__restrict__ bins, int64_t cells, int64_t cstride, int64_t xstride, int npre, int nsec, int nbin) {
#pragma clang fp contract(off)
   const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
   if (c >= cells) return;
   const bool two = c + 1 < cells;
   const int b = blockIdx.y;
   double xa[NT], xb[NT];
#pragma unroll
   for (int t = 0; t < NT; t++) {
      xa[t] = (double)x[(int64_t)t * xstride + c];
      xb[t] = two ? (double)x[(int64_t)t * xstride + c + 1] : 0.0;
   }
   const int64_t q0 = npre + (int64_t)b * nsec;
   for (int s = 0; s < nsec; s++) band_section<NT>(st, coef + 5 * (q0 + s), q0 + s, c, cstride, xa, xb);
   int cur = -1;
   double2 e = make_double2(0.0, 0.0);
   double2 *row = nullptr;
#pragma unroll
   for (int t = 0; t < NT; t++) {
      const int bin = bins[t];
      if (bin < 0 || bin >= nbin) continue; // (-1: the filters ran, nothing is summed)
      if (bin != cur) {
         if (cur >= 0) *row = e;
         row = reinterpret_cast<double2 *>(E + ((int64_t)b * nbin + bin) * cstride + c);
         e = *row;
         cur = bin;
      }
      e.x = e.x + xa[t] * xa[t];
      e.y = e.y + xb[t] * xb[t];
   }
   if (cur >= 0) *row = e;
}

} // namespace pf
