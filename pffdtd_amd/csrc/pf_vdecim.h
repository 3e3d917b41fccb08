// pf_vdecim.h -- device side of the vector decimating recorders (include/pffdtd_hip.h: pf_vdecim): per cell of a region, up to four COMPONENTS of
// the field -- the cell itself or a difference, sampled exactly as a vector band accumulator samples them (pf_vband.h: k_region_cut, k_region_diff,
// k_region_lat into the component's ring slot) -- run through their own second-order sections (k_vband_pre, unchanged) and then, each on its own,
// through pf_decim.h's FIR in ARRIVAL order, every D-th output kept: a B-format impulse response per cell.
//    x_k = double(component k);  x_k -> pre sections of k;  per slot p:  acc[k][p] = acc[k][p] + h[tap] * x_k      product, then sum: NO fma
//    tap == 0:  frame m of component k = acc[k][p];  acc[k][p] = +0.0
// The tap a pending sample meets in a slot and the frame row it completes (plan, orow: pf_decim.h) depend on neither the cell nor the component: the
// host works them out once per sample.
//   acc    double [ncomp][P][cstride]           cstride = the cell count rounded up to a multiple of 2
//   frames double [cap][ncomp][cstride]         frame m of component k in row (m mod cap) * ncomp + k: n frames are n * ncomp consecutive rows
//   st     double [ncomp][npre * 2][cstride]    taps double [ntap]     coef double [ncomp][npre][5]
//   ring   Real   [ncomp][depth][cells]         xpre double [ncomp][depth][cstride] (npre > 0 only)      plan, orow int32 [depth][P]
// A fold of NT pending samples is k_vband_pre<Real, NT> (npre > 0; grid.y = the component) and ONE k_vdecim_fold<In, NT, S> on a grid of
// (cdiv(cdiv(cells, 2), 256), cdiv(P, S), ncomp): blockIdx.z is the component, everything else is k_decim_fold -- a thread owns two adjacent cells
// (16-byte loads and stores), holds its group's S slots in registers and walks the NT samples in order; plan, orow and taps are scalar loads.  No
// atomics, no LDS, no scratch (tools/kernel_resources.py k_vdecim).  64-bit indices, every access guarded by the cell count.  Components and slots
// are independent of each other, so neither the grid's z nor S changes a bit.
//
// PF_VDECIM_DEFAULT_DEPTH: the fastest of the depths 1, 4, 8, 16 for four components on the plane cases of tools/field_recording_cost.py --axes
// (profiles/field_vector_recording.txt); it equals the scalar recorder's.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "pf_decim.h"

namespace pf {

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
