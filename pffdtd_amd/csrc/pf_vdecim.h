// pf_vdecim.h -- device side of the decimating recorders, scalar and vector (include/pffdtd_hip.h: pf_decim, pf_vdecim): per cell of a region, up
// to four COMPONENTS of the field -- the cell itself or a difference, sampled exactly as a vector band accumulator samples them (pf_vband.h:
// k_region_cut, k_region_diff, k_region_lat into the component's ring slot) -- run through their own npre second-order sections (k_vband_pre,
// unchanged) and then, each on its own, through a linear-phase FIR of ntap taps h, of which every D-th output is kept: an impulse response per
// cell, in B-format with four components.  The scalar recorder (pf_decim) is the one component 0.
//    frame m = sum_k h[k] x[m D - k]                     (the terms before sample 0 are not added)
// The sum is formed in ARRIVAL order.  P = ceil(ntap / D) outputs are in flight at any time, one per slot of `acc`; the sample with index n meets
// tap = m D - n of the output m that slot p carries (q = ceil(n / D), m = q + ((p - q) mod P)):
//    x_k = double(component k);  x_k -> pre sections of k;  per slot p:  acc[k][p] = acc[k][p] + h[tap] * x_k      product rounded to double, then the sum: NO fma
//    tap == 0:  frame m of component k = acc[k][p];  acc[k][p] = +0.0
// so a numpy loop over time gives the same bits at every ring depth.  m, the tap and the frame's device row depend on neither the cell nor the
// component: the host works them out once per pending sample and slot and uploads them with every fold (plan, orow; as pf_vband.h's bins):
//   acc    double [ncomp][P][cstride]           cstride = the cell count rounded up to a multiple of 2: every row starts 16-byte aligned
//   frames double [cap][ncomp][cstride]         frame m of component k in row (m mod cap) * ncomp + k: n frames are n * ncomp consecutive rows
//   st     double [ncomp][npre * 2][cstride]    taps double [ntap] (uploaded once, at creation)     coef double [ncomp][npre][5]
//   ring   Real   [ncomp][depth][cells]         the region's components at the samples not folded in yet
//   xpre   double [ncomp][depth][cstride]       npre > 0 only: the pending samples after the sections
//   plan   int32  [depth][P]                    the tap a pending sample meets in a slot, or -1 (the slot idles: tap >= ntap)
//   orow   int32  [depth][P]                    the frame (m mod cap) the sample completes in a slot, or -1
// A fold of NT pending samples is k_vband_pre<Real, NT> (npre > 0; grid.y = the component) and ONE k_vdecim_fold<In, NT, S> on a grid of
// (cdiv(cdiv(cells, 2), 256), cdiv(P, S), ncomp): groups of S slots in parallel, blockIdx.z is the component.  A thread owns two adjacent cells
// (16-byte loads and stores, lanes along cells: whole lines), loads and widens its NT inputs once, holds its group's S slots in registers -- acc
// loaded once, stored once -- and walks the NT samples in order; a completing slot stores its pair into the frame's row and restarts from +0.0.
// plan[...], orow[...] and taps[...] do not depend on the lane: scalar loads.  No atomics, no LDS, no scratch (tools/kernel_resources.py
// k_vdecim).  64-bit indices, every access guarded by the cell count (c even and c < cells, so c + 1 < cstride).  The padding cell of an odd
// count filters zeros.  Components and slots are independent of each other, so neither the grid's z nor S changes a bit.
//
// PF_DECIM_SLOTS (S) and PF_DECIM_DEFAULT_DEPTH: tools/field_recording_cost.py (profiles/field_recording.txt, measured with one component).
// PF_VDECIM_DEFAULT_DEPTH: the fastest of the depths 1, 4, 8, 16 for four components on the plane cases of tools/field_recording_cost.py --axes
// (profiles/field_vector_recording.txt); the two agree.
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
constexpr int PF_VDECIM_DEFAULT_DEPTH = PF_DECIM_DEFAULT_DEPTH;

// grid: (cdiv(cdiv(cells, 2), 256), cdiv(P, S), ncomp) blocks of 256 threads.  x: the ring (xstride = cells) or xpre (xstride = cstride) at the first of
// the NT samples, xcomp elements between two components; acomp = P * cstride: between two components' acc blocks; plan, orow: [NT][P]
template <typename In, int NT, int S>
static __global__ void __launch_bounds__(256) k_vdecim_fold(double *__restrict__ acc, double *__restrict__ frames, const In *__restrict__ x, const double *__restrict__ taps,
                                                            const int32_t *__restrict__ plan, const int32_t *__restrict__ orow, int64_t cells, int64_t cstride,
                                                            int64_t xstride, int64_t xcomp, int64_t acomp, int ncomp, int P) {
#pragma clang fp contract(off)
   const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
   if (c >= cells) return;
   const bool two = c + 1 < cells;
   const int p0 = (int)blockIdx.y * S, k = (int)blockIdx.z;
   const In *xk = x + (int64_t)k * xcomp;
   double *ak = acc + (int64_t)k * acomp;
   double xa[NT], xb[NT];
#pragma unroll
   for (int t = 0; t < NT; t++) {
      xa[t] = (double)xk[(int64_t)t * xstride + c];
      xb[t] = two ? (double)xk[(int64_t)t * xstride + c + 1] : 0.0;
   }
   double2 a[S];
#pragma unroll
   for (int s = 0; s < S; s++) a[s] = p0 + s < P ? *reinterpret_cast<const double2 *>(ak + (int64_t)(p0 + s) * cstride + c) : make_double2(0.0, 0.0);
#pragma unroll
   for (int t = 0; t < NT; t++) {
#pragma unroll
      for (int s = 0; s < S; s++) {
         if (p0 + s >= P) continue;
         const int tap = plan[t * P + p0 + s];
         if (tap < 0) continue; // (the slot idles at this sample)
         const double h = taps[tap];
         a[s].x = a[s].x + h * xa[t];
         a[s].y = a[s].y + h * xb[t];
         const int row = orow[t * P + p0 + s];
         if (row >= 0) {
            *reinterpret_cast<double2 *>(frames + ((int64_t)row * ncomp + k) * cstride + c) = a[s];
            a[s] = make_double2(0.0, 0.0);
         }
      }
   }
#pragma unroll
   for (int s = 0; s < S; s++)
      if (p0 + s < P) *reinterpret_cast<double2 *>(ak + (int64_t)(p0 + s) * cstride + c) = a[s];
}

} // namespace pf
