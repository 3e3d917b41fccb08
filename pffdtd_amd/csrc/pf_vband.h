// pf_vband.h -- device side of the band accumulators, vector (include/pffdtd_hip.h: pf_vbandacc) and scalar (pf_bandacc): per cell of a region, up to
// four COMPONENTS of the field -- the cell itself (0) or the central difference along file x / y / z (1 / 2 / 3), d_a = u^n[c + e_a] - u^n[c - e_a] in
// the field's own precision -- run through a cascade of second-order sections each, and PRODUCTS of two filtered components are summed into time bins,
//    x_k = double(component k);  x_k -> pre sections of k;  per band b: y_k = x_k -> the band's sections (state per component);
//    S[p][b][bin] = S[p][b][bin] + y_i * y_j          (mode 1: + fabs(y_i * y_j))         for every product p = (i, j, mode)
// which is what a lateral energy fraction or an intensity map needs of every cell (pffdtd_amd/directional.py).  The SCALAR band accumulator is the
// one component 0 with the one product (0, 0, 0): E[b][bin] = E[b][bin] + y * y, what an energy decay per octave band needs (pffdtd_amd/decay.py).
// The section is pf_band.h's band_section: three lines, every operation rounded to double once, NO fma (the build has -ffp-contract=off, the
// pragmas below say so again).
//   S     double [nprod * nband * nbin][cstride]            cstride = the cell count rounded up to a multiple of 2: every row starts 16-byte aligned
//   st    double [ncomp][(npre + nband*nsec) * 2][cstride]   component k's s1, s2 of section q in rows 2q, 2q + 1 of its block; pre sections first,
//                                                           then band 0's, band 1's, ...
//   coef  double [(ncomp*npre + nband*nsec) * 5]            the components' pre sections, then the bands' (shared by the components); uploaded once
//   ring  Real   [ncomp][depth][cells]                      the components at the samples not folded in yet: component 0 by k_region_cut
//                                                           (pf_region.h), a difference by k_region_diff below -- a fold reads Real whatever
//                                                           the component
//   xpre  double [ncomp][depth][cstride]                    npre > 0 only: the pending samples after the components' pre sections
//   bins  int32  [depth]                                    the pending samples' bins (-1: filter, sum nothing), uploaded with every fold
//   prod  int32  [nprod][3]
// (the scalar kind: ncomp = nprod = 1, so S is its E [nband * nbin][cstride] and st its [(npre + nband*nsec) * 2][cstride].)
// k_region_diff<Real, EXCH> is k_region_cut with the two neighbour loads and ONE subtraction, rounded once in Real.  The subtraction is done in
// registers before anything goes to LDS, so the tiled form keeps ONE 32 x 33 tile of Real and the bank picture of pf_region.h as it is (two
// operand tiles would double the LDS for nothing: the operands are never needed apart).  On exchanged storage a difference along file x has its
// operands one element apart (same lines), along file z one storage plane apart.
// k_region_lat<Real, EXCH> is the same kernel for the LATTICE differences of an FCC grid (comp 4 / 5 / 6: the four pair differences over the eight
// FCC neighbours at +-1 along file x / y / z, seven operations in Real): ONE launch per sample for ALL the requested ones -- a mask says which --,
// each of the at most twelve distinct neighbours loaded once, the sums formed in registers, one 32 x 33 tile of Real PER REQUESTED component in the
// tiled form (dynamic LDS; the bank picture of pf_region.h per tile), each component stored into its own ring slot.  Stored coordinates, no parity
// logic: a folded grid's fold row is a row like any other, a checkerboard's hole is computed from holes.
// A fold of NT pending samples is k_vband_pre<Real, NT> (npre > 0; grid.y = the component: one thread per two cells runs the pre sections once and
// writes xpre -- the other choice, every band recomputing them, has band b read the shared state while band 0 stores it) and ONE
// k_vband_fold<In, NC, NT> on a grid of (cdiv(cdiv(cells, 2), 256), nband): bands in parallel, so a 64^2 plane still fills the chip.  A thread owns
// two adjacent cells (16-byte loads and stores, lanes along cells: whole lines), reads and widens its inputs once and runs all NC components'
// sections of its band over the NT samples in registers -- two state words per cell loaded, NT samples through the section, stored once: state
// traffic is 1 / NT of the depth-1 form; y[NC][NT] of two cells, 2 * NC * NT doubles, never go to memory -- and then walks the products and, per
// product, the bins: consecutive samples of one bin are summed in a register from the loaded S in call order, a bin change stores and loads.  The
// padding cell of an odd count filters zeros.  The components of a product are picked with selects on (i == k), uniform over the wave: no indexed
// register file, hence no scratch.  prod, coef and bins do not depend on the lane: scalar loads.  No atomics, no LDS in the folds, no scratch
// (tools/kernel_resources.py k_vband).  64-bit indices, every access guarded by the cell count (c even and c < cells, so c + 1 < cstride).
// Instantiated for NC = 1 .. 4 and NT in {1, 2, 4, 8}: a partly filled ring is folded greedily (7 = 4 + 2 + 1), the samples still in call order,
// so the pieces never change a bit.  The SCALAR kind's objects are this kind's with one component and one product, but its folds are launched on
// pf_band.h's k_band_pre / k_band_fold, which compute the same bits: on these kernels it measured 0.3 .. 1 % slower per sample
// (profiles/field_decay_refactor.txt), and a refactor is to cost nothing.
//
// PF_VBAND_DEFAULT_DEPTH: the fastest of the depths 1, 2, 4, 8 on the plane case of tools/field_directional_cost.py (profiles/field_directional.txt),
// and of its --fcc case with the lattice differences (profiles/field_directional_fcc.txt).  The scalar kind's ring: pf_band.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "pf_band.h"
#include "pf_region.h"

namespace pf {

constexpr int PF_VBAND_MAX_COMP = 4;
constexpr int PF_VBAND_MAX_PROD = 10;
constexpr int PF_VBAND_MAX_DEPTH = 8;
constexpr int PF_VBAND_DEFAULT_DEPTH = 8;

// grid and arguments as k_region_cut; dx, dy, dz: the difference's unit vector in FILE coordinates (one of them 1).  The caller keeps the region one
// cell clear of both faces along that axis, so both neighbours are cells of the grid.
template <typename Real, bool EXCH>
static __global__ void __launch_bounds__(256) k_region_diff(const Real *__restrict__ st, Real *__restrict__ stage, RegionPiece q, int64_t Ny, int64_t P, int tiled, int bz_log2,
                                                            int dx, int dy, int dz) {
#pragma clang fp contract(off)
   // storage offset of one cell along the difference axis
   const int64_t step = EXCH ? ((int64_t)dz * Ny + dy) * P + dx : ((int64_t)dx * Ny + dy) * P + dz;
   if (EXCH && tiled) {
      __shared__ Real tile[32][33];
      const int a = threadIdx.x & 31, b = threadIdx.x >> 5; // 32 x 8
      const int64_t j = blockIdx.y, kt = (int64_t)blockIdx.x * 32, it = (int64_t)blockIdx.z * 32;
      const int64_t fy = q.lo1 + j * q.s1;
#pragma unroll
      for (int r = 0; r < 4; r++) { // lanes along file x: the storage's unit-stride axis
         const int64_t i = it + a, k = kt + b + 8 * r;
         if (i < q.n0 && k < q.n2) {
            const int64_t at = ((q.lo2 + k * q.s2) * Ny + fy) * P + q.lo0 + i * q.s0;
            tile[b + 8 * r][a] = st[at + step] - st[at - step];
         }
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; r++) { // lanes along file z: the slot's
         const int64_t i = it + b + 8 * r, k = kt + a;
         if (i < q.n0 && k < q.n2) stage[(i * q.n1 + j) * q.n2 + k] = tile[a][b + 8 * r];
      }
      return;
   }
   const int bz = 1 << bz_log2;
   const int64_t k = (int64_t)blockIdx.x * bz + (threadIdx.x & (bz - 1));
   const int64_t j = (int64_t)blockIdx.y * (256 >> bz_log2) + (threadIdx.x >> bz_log2);
   const int64_t i = blockIdx.z;
   if (k >= q.n2 || j >= q.n1) return;
   const int64_t fx = q.lo0 + i * q.s0, fy = q.lo1 + j * q.s1, fz = q.lo2 + k * q.s2;
   const int64_t at = EXCH ? (fz * Ny + fy) * P + fx : (fx * Ny + fy) * P + fz;
   stage[(i * q.n1 + j) * q.n2 + k] = st[at + step] - st[at - step];
}

// The twelve FCC neighbours of a cell in FILE coordinates, named by the plane they lie in and the signs of its two offsets: xy_pm = (+1, -1, 0),
// xz_mp = (-1, 0, +1), yz_pp = (0, +1, +1).  A lattice difference along an axis reads the eight of them that sit at +-1 along it.
template <typename Real> struct LatNb {
   Real xy_pp, xy_mm, xy_pm, xy_mp, xz_pp, xz_mm, xz_pm, xz_mp, yz_pp, yz_mm, yz_pm, yz_mp;
};

// the neighbours of the cell at storage offset `at` that `mask` (bit 0 / 1 / 2: the lattice difference along file x / y / z) needs, each loaded once;
// sx, sy, sz: the storage offsets of one cell along file x, y, z.  The caller keeps the region one cell clear of all six faces.
template <typename Real>
static __device__ __forceinline__ LatNb<Real> lat_load(const Real *__restrict__ st, int64_t at, int64_t sx, int64_t sy, int64_t sz, int mask) {
   LatNb<Real> n{};
   if (mask & 3) { n.xy_pp = st[at + sx + sy]; n.xy_mm = st[at - sx - sy]; n.xy_pm = st[at + sx - sy]; n.xy_mp = st[at - sx + sy]; }
   if (mask & 5) { n.xz_pp = st[at + sx + sz]; n.xz_mm = st[at - sx - sz]; n.xz_pm = st[at + sx - sz]; n.xz_mp = st[at - sx + sz]; }
   if (mask & 6) { n.yz_pp = st[at + sy + sz]; n.yz_mm = st[at - sy - sz]; n.yz_pm = st[at + sy - sz]; n.yz_mp = st[at - sy + sz]; }
   return n;
}
// L_a = ((u[c+o0] - u[c-o0]) + (u[c+o1] - u[c-o1])) + ((u[c+o2] - u[c-o2]) + (u[c+o3] - u[c-o3])), the offsets of include/pffdtd_hip.h: seven operations,
// each rounded once in Real
template <typename Real> static __device__ __forceinline__ Real lat_x(const LatNb<Real> &n) {
#pragma clang fp contract(off)
   return ((n.xy_pp - n.xy_mm) + (n.xz_pp - n.xz_mm)) + ((n.xy_pm - n.xy_mp) + (n.xz_pm - n.xz_mp));
}
template <typename Real> static __device__ __forceinline__ Real lat_y(const LatNb<Real> &n) {
#pragma clang fp contract(off)
   return ((n.xy_pp - n.xy_mm) + (n.yz_pp - n.yz_mm)) + ((n.xy_mp - n.xy_pm) + (n.yz_pm - n.yz_mp));
}
template <typename Real> static __device__ __forceinline__ Real lat_z(const LatNb<Real> &n) {
#pragma clang fp contract(off)
   return ((n.yz_pp - n.yz_mm) + (n.xz_pp - n.xz_mm)) + ((n.yz_mp - n.yz_pm) + (n.xz_mp - n.xz_pm));
}

// The lattice differences of an FCC grid (comp 4 / 5 / 6), ALL the requested ones in one launch: grid and arguments as k_region_cut, mask as
// lat_load's, ox / oy / oz: the ring slot of the difference along file x / y / z (read only where its mask bit is set).  The tiled form keeps one
// 32 x 33 tile of Real per REQUESTED component in dynamic LDS (popcount(mask) * 32 * 33 * sizeof(Real) bytes, in the order x, y, z): the pair
// differences and their sums are formed in registers before anything goes to LDS, as k_region_diff.
template <typename Real, bool EXCH>
static __global__ void __launch_bounds__(256) k_region_lat(const Real *__restrict__ st, Real *__restrict__ ox, Real *__restrict__ oy, Real *__restrict__ oz, RegionPiece q, int64_t Ny,
                                                           int64_t P, int tiled, int bz_log2, int mask) {
#pragma clang fp contract(off)
   const int64_t sx = EXCH ? 1 : Ny * P, sy = P, sz = EXCH ? Ny * P : 1;
   if (EXCH && tiled) {
      extern __shared__ __align__(16) unsigned char lat_lds[];
      Real(*tile)[32][33] = reinterpret_cast<Real(*)[32][33]>(lat_lds);
      const int tx = 0, ty = mask & 1, tz = (mask & 1) + ((mask >> 1) & 1); // a component's tile
      const int a = threadIdx.x & 31, b = threadIdx.x >> 5; // 32 x 8
      const int64_t j = blockIdx.y, kt = (int64_t)blockIdx.x * 32, it = (int64_t)blockIdx.z * 32;
      const int64_t fy = q.lo1 + j * q.s1;
#pragma unroll
      for (int r = 0; r < 4; r++) { // lanes along file x: the storage's unit-stride axis
         const int64_t i = it + a, k = kt + b + 8 * r;
         if (i < q.n0 && k < q.n2) {
            const LatNb<Real> n = lat_load(st, ((q.lo2 + k * q.s2) * Ny + fy) * P + q.lo0 + i * q.s0, sx, sy, sz, mask);
            if (mask & 1) tile[tx][b + 8 * r][a] = lat_x(n);
            if (mask & 2) tile[ty][b + 8 * r][a] = lat_y(n);
            if (mask & 4) tile[tz][b + 8 * r][a] = lat_z(n);
         }
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; r++) { // lanes along file z: the slot's
         const int64_t i = it + b + 8 * r, k = kt + a;
         if (i < q.n0 && k < q.n2) {
            const int64_t o = (i * q.n1 + j) * q.n2 + k;
            if (mask & 1) ox[o] = tile[tx][a][b + 8 * r];
            if (mask & 2) oy[o] = tile[ty][a][b + 8 * r];
            if (mask & 4) oz[o] = tile[tz][a][b + 8 * r];
         }
      }
      return;
   }
   const int bz = 1 << bz_log2;
   const int64_t k = (int64_t)blockIdx.x * bz + (threadIdx.x & (bz - 1));
   const int64_t j = (int64_t)blockIdx.y * (256 >> bz_log2) + (threadIdx.x >> bz_log2);
   const int64_t i = blockIdx.z;
   if (k >= q.n2 || j >= q.n1) return;
   const int64_t fx = q.lo0 + i * q.s0, fy = q.lo1 + j * q.s1, fz = q.lo2 + k * q.s2;
   const LatNb<Real> n = lat_load(st, EXCH ? (fz * Ny + fy) * P + fx : (fx * Ny + fy) * P + fz, sx, sy, sz, mask);
   const int64_t o = (i * q.n1 + j) * q.n2 + k;
   if (mask & 1) ox[o] = lat_x(n);
   if (mask & 2) oy[o] = lat_y(n);
   if (mask & 4) oz[o] = lat_z(n);
}

// grid: (cdiv(cdiv(cells, 2), 256), ncomp) blocks of 256 threads; npre >= 1.  ring, xpre: at the first of the NT samples; rcomp, xcomp, scomp: elements
// between two components' blocks of the ring, of xpre, of the state
template <typename Real, int NT>
static __global__ void __launch_bounds__(256) k_vband_pre(double *__restrict__ st, double *__restrict__ xpre, const Real *__restrict__ ring, const double *__restrict__ coef,
                                                          int64_t cells, int64_t cstride, int64_t rcomp, int64_t xcomp, int64_t scomp, int npre) {
#pragma clang fp contract(off)
   const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
   if (c >= cells) return;
   const bool two = c + 1 < cells;
   const int k = blockIdx.y;
   const Real *x = ring + (int64_t)k * rcomp;
   double xa[NT], xb[NT];
#pragma unroll
   for (int t = 0; t < NT; t++) {
      xa[t] = (double)x[(int64_t)t * cells + c];
      xb[t] = two ? (double)x[(int64_t)t * cells + c + 1] : 0.0;
   }
   double *sk = st + (int64_t)k * scomp;
   const double *ck = coef + (int64_t)k * npre * 5;
   for (int q = 0; q < npre; q++) band_section<NT>(sk, ck + 5 * q, q, c, cstride, xa, xb);
   double *o = xpre + (int64_t)k * xcomp;
#pragma unroll
   for (int t = 0; t < NT; t++) *reinterpret_cast<double2 *>(o + (int64_t)t * cstride + c) = make_double2(xa[t], xb[t]);
}

// grid: (cdiv(cdiv(cells, 2), 256), nband) blocks of 256 threads.  x: the ring (xstride = cells) or xpre (xstride = cstride) at the first of the NT samples,
// xcomp elements between two components; bcoef: the bands' coefficients
template <typename In, int NC, int NT>
static __global__ void __launch_bounds__(256) k_vband_fold(double *__restrict__ S, double *__restrict__ st, const In *__restrict__ x, const double *__restrict__ bcoef,
                                                           const int32_t *__restrict__ bins, const int32_t *__restrict__ prod, int64_t cells, int64_t cstride, int64_t xstride,
                                                           int64_t xcomp, int64_t scomp, int npre, int nsec, int nband, int nbin, int nprod) {
#pragma clang fp contract(off)
   const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
   if (c >= cells) return;
   const bool two = c + 1 < cells;
   const int b = blockIdx.y;
   double ya[NC][NT], yb[NC][NT];
#pragma unroll
   for (int k = 0; k < NC; k++) {
      const In *xk = x + (int64_t)k * xcomp;
#pragma unroll
      for (int t = 0; t < NT; t++) {
         ya[k][t] = (double)xk[(int64_t)t * xstride + c];
         yb[k][t] = two ? (double)xk[(int64_t)t * xstride + c + 1] : 0.0;
      }
   }
   const int64_t q0 = npre + (int64_t)b * nsec;
#pragma unroll
   for (int k = 0; k < NC; k++)
      for (int s = 0; s < nsec; s++) band_section<NT>(st + (int64_t)k * scomp, bcoef + 5 * ((int64_t)b * nsec + s), q0 + s, c, cstride, ya[k], yb[k]);
   for (int p = 0; p < nprod; p++) {
      const int pi = prod[3 * p], pj = prod[3 * p + 1], mode = prod[3 * p + 2];
      int cur = -1;
      double2 e = make_double2(0.0, 0.0);
      double2 *row = nullptr;
#pragma unroll
      for (int t = 0; t < NT; t++) {
         const int bin = bins[t];
         if (bin < 0 || bin >= nbin) continue; // (-1: the filters ran, nothing is summed)
         if (bin != cur) {
            if (cur >= 0) *row = e;
            row = reinterpret_cast<double2 *>(S + (((int64_t)p * nband + b) * nbin + bin) * cstride + c);
            e = *row;
            cur = bin;
         }
         double ia = ya[0][t], ib = yb[0][t], ja = ya[0][t], jb = yb[0][t];
#pragma unroll
         for (int k = 1; k < NC; k++) { // (pi, pj are uniform: selects, never an indexed register file)
            ia = pi == k ? ya[k][t] : ia;
            ib = pi == k ? yb[k][t] : ib;
            ja = pj == k ? ya[k][t] : ja;
            jb = pj == k ? yb[k][t] : jb;
         }
         double va = ia * ja, vb = ib * jb;
         if (mode) { va = fabs(va); vb = fabs(vb); }
         e.x = e.x + va;
         e.y = e.y + vb;
      }
      if (cur >= 0) *row = e;
   }
}

} // namespace pf
