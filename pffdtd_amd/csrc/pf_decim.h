// pf_decim.h -- device side of the decimating recorders (include/pffdtd_hip.h: pf_decim): per cell of a region, the sample u^n runs through npre
// shared second-order sections (pf_band.h's k_band_pre and its three lines, unchanged) and then through a linear-phase FIR of ntap taps h, of which
// every D-th output is kept:
//    frame m = sum_k h[k] x[m D - k]                     (the terms before sample 0 are not added)
// The sum is formed in ARRIVAL order.  P = ceil(ntap / D) outputs are in flight at any time, one per slot of `acc`; the sample with index n meets
// tap k = m D - n of the output m that slot p carries (q = ceil(n / D), m = q + ((p - q) mod P)):
//    acc[p] = acc[p] + h[k] * x          product rounded to double, then the sum: NO fma
//    k == 0:  frame m = acc[p];  acc[p] = +0.0
// so a numpy loop over time gives the same bits at every ring depth.  m, k and the frame's device row do not depend on the cell: the host works them
// out per pending sample and slot and uploads them with every fold (as pf_band.h's bins):
//   acc    double [P][cstride]              cstride = the cell count rounded up to a multiple of 2: every row starts 16-byte aligned
//   frames double [cap][cstride]            frame m in row m mod cap
//   taps   double [ntap]                    uploaded once, at creation
//   ring   Real   [depth][cells]            the region's cells at the samples not folded in yet (k_region_cut)
//   xpre   double [depth][cstride]          npre > 0 only: the pending samples after the shared sections
//   plan   int32  [depth][P]                the tap a pending sample meets in a slot, or -1 (the slot idles: k >= ntap)
//   orow   int32  [depth][P]                the device row of the frame the sample completes in a slot, or -1
// A fold of NT pending samples is k_band_pre<Real, NT> (npre > 0) and k_decim_fold<In, NT, S> on a grid of (cdiv(cdiv(cells, 2), 256), cdiv(P, S)):
// groups of S slots in parallel.  A thread owns two adjacent cells (16-byte loads and stores, lanes along cells: whole lines), loads and widens its
// NT inputs once, holds its group's S slots in registers -- acc loaded once, stored once -- and walks the NT samples in order; a completing slot
// stores its pair into the frame's row and restarts from +0.0.  Slots are independent, so S never changes a bit.  plan[...], orow[...] and
// taps[...] do not depend on the lane: scalar loads.  No atomics, no LDS, no scratch (tools/kernel_resources.py k_decim).  64-bit indices, every
// access guarded by the cell count (c even and c < cells, so c + 1 < cstride).  The padding cell of an odd count filters zeros.
//
// PF_DECIM_SLOTS (S) and PF_DECIM_DEFAULT_DEPTH: tools/field_recording_cost.py (profiles/field_recording.txt).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pf {

constexpr int PF_DECIM_MAX_TAPS = 4096;
constexpr int PF_DECIM_MAX_FACTOR = 64;
constexpr int PF_DECIM_MAX_SLOTS = 128; // P
constexpr int PF_DECIM_MAX_DEPTH = 16;
constexpr int PF_DECIM_DEFAULT_DEPTH = 16;
#ifndef PF_DECIM_SLOTS_N // (tools/field_recording_cost.py builds the library once per candidate)
#define PF_DECIM_SLOTS_N 4
#endif
constexpr int PF_DECIM_SLOTS = PF_DECIM_SLOTS_N; // S

// grid: (cdiv(cdiv(cells, 2), 256), cdiv(P, S)) blocks of 256 threads.  x: the ring (xstride = cells) or xpre (xstride = cstride); plan, orow: [NT][P]
template <typename In, int NT, int S>
static __global__ void __launch_bounds__(256) k_decim_fold(double *__restrict__ acc, double *__restrict__ frames, const In *__restrict__ x, const double *__restrict__ taps,
                                                           const int32_t *__restrict__ plan, const int32_t *__restrict__ orow, int64_t cells, int64_t cstride,
                                                           int64_t xstride, int P) {
#pragma clang fp contract(off)
   const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
   if (c >= cells) return;
   const bool two = c + 1 < cells;
   const int p0 = (int)blockIdx.y * S;
   double xa[NT], xb[NT];
#pragma unroll
   for (int t = 0; t < NT; t++) {
      xa[t] = (double)x[(int64_t)t * xstride + c];
      xb[t] = two ? (double)x[(int64_t)t * xstride + c + 1] : 0.0;
   }
   double2 a[S];
#pragma unroll
   for (int s = 0; s < S; s++) a[s] = p0 + s < P ? *reinterpret_cast<const double2 *>(acc + (int64_t)(p0 + s) * cstride + c) : make_double2(0.0, 0.0);
#pragma unroll
   for (int t = 0; t < NT; t++) {
#pragma unroll
      for (int s = 0; s < S; s++) {
         if (p0 + s >= P) continue;
         const int k = plan[t * P + p0 + s];
         if (k < 0) continue; // (the slot idles at this sample)
         const double h = taps[k];
         a[s].x = a[s].x + h * xa[t];
         a[s].y = a[s].y + h * xb[t];
         const int row = orow[t * P + p0 + s];
         if (row >= 0) {
            *reinterpret_cast<double2 *>(frames + (int64_t)row * cstride + c) = a[s];
            a[s] = make_double2(0.0, 0.0);
         }
      }
   }
#pragma unroll
   for (int s = 0; s < S; s++)
      if (p0 + s < P) *reinterpret_cast<double2 *>(acc + (int64_t)(p0 + s) * cstride + c) = a[s];
}

} // namespace pf
