// pf_accum.h -- device side of the field accumulators (include/pffdtd_hip.h: pf_accum): running sums of a region's cells over the time steps,
//    acc[m][c] += w_m(n) * double(u^n[c])        m < nchan channels, c < cells of the region, dense in the region's order (z fastest),
// with cos / -sin weights a running DFT of every cell (pffdtd_amd/spectra.py).  16 bytes per cell and channel, whatever the run's length.
//   acc   double [nchan][cstride]   cstride = the cell count rounded up to a multiple of 2: every channel's row starts 16-byte aligned
//   ring  Real   [depth][cells]     the region's cells at the samples not folded in yet, cut there by k_region_cut (pf_region.h) as they are taken
//   wt    double [depth][nchan]     the weights of those samples
// k_accum_fold<Real, NT> folds NT pending samples in at once.  A thread owns two adjacent cells (one 16-byte load and store per channel, lanes
// along cells: whole lines); it reads its NT values of the ring once, widens them (fp32 denormals survive v_cvt_f64_f32: the build leaves the
// denormal mode alone) and walks the channels.  Per sample and cell this moves 16 * nchan / NT + 2 * sizeof(Real) bytes where the plain form
// (NT = 1) moves 16 * nchan + sizeof(Real).  Every channel sees its samples in the order they were taken,
//    a = acc;  a = a + wt[t][m] * u_t   for t = 0 .. NT-1   (one multiply rounded to double, one add rounded to double: NO fma -- the build has
//                                                            -ffp-contract=off, the pragma below says so again for this function)
// so the depth of the ring never changes a bit of a sum, and numpy's acc += w * u.astype(float64) gives the same bits.
// wt[t * nchan + m] does not depend on the lane: the compiler fetches it with scalar loads (s_load_dwordx2 in the ISA; tools/kernel_resources.py
// k_accum_fold: no scratch, no LDS).  No atomics.  64-bit indices, every access guarded by the cell count.
//
// PF_ACCUM_DEFAULT_DEPTH: the faster of the measured depths on the plane cases of tools/field_accum_cost.py (profiles/field_spectra.txt).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pf {

constexpr int PF_ACCUM_MAX_CHANNELS = 256;
constexpr int PF_ACCUM_MAX_DEPTH = 16;
constexpr int PF_ACCUM_DEFAULT_DEPTH = 8;

// grid: cdiv(cdiv(cells, 2), 256) blocks of 256 threads
template <typename Real, int NT>
static __global__ void __launch_bounds__(256) k_accum_fold(double *__restrict__ acc, const Real *__restrict__ ring, const double *__restrict__ wt, int64_t cells, int64_t cstride, int nchan) {
#pragma clang fp contract(off)
   const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
   if (c >= cells) return;
   const bool two = c + 1 < cells; // (false: the odd tail, the last thread's second cell is padding)
   double ua[NT], ub[NT];
#pragma unroll
   for (int t = 0; t < NT; t++) {
      ua[t] = (double)ring[(int64_t)t * cells + c];
      ub[t] = two ? (double)ring[(int64_t)t * cells + c + 1] : 0.0;
   }
   for (int m = 0; m < nchan; m++) {
      double *row = acc + (int64_t)m * cstride + c;
      const double *w = wt + m;
      if (two) {
         double2 a = *reinterpret_cast<const double2 *>(row);
#pragma unroll
         for (int t = 0; t < NT; t++) {
            const double wm = w[(int64_t)t * nchan];
            a.x = a.x + wm * ua[t];
            a.y = a.y + wm * ub[t];
         }
         *reinterpret_cast<double2 *>(row) = a;
      } else {
         double a = row[0];
#pragma unroll
         for (int t = 0; t < NT; t++) a = a + w[(int64_t)t * nchan] * ua[t];
         row[0] = a;
      }
   }
}

} // namespace pf
