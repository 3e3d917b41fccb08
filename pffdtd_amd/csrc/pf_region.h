// pf_region.h -- device side of pf_engine_get_region (include/pffdtd_hip.h: pf_region): a strided box of one field, cut out of the engine's storage
// into a compact staging buffer in the FILE's order, stage[(i * c1 + j) * c2 + k] = the cell (lo0 + i * s0, lo1 + j * s1, lo2 + k * s2) in file
// coordinates.  One kernel, two forms:
//   * direct: a thread per cell of the region, lanes along file z (the buffer's unit stride) -- `bz` (a power of two <= 256) lanes along k, the
//     other 256 / bz along j, so a region that is thin along z still fills its waves.  On file-order storage ((fx * Ny + fy) * P + fz) a region
//     with stride 1 along z reads and writes whole rows.  On exchanged storage ((fz * Ny + fy) * P + fx) this is the form of the THIN regions, a
//     single x or a single z: one side is strided whichever way the lanes run.
//   * tiled (exchanged storage, at least 2 cells along both x and z): 32 x 32 cells over (file x, file z) of one row j through a 32 x 33 LDS tile, as
//     k_state_planes (pf_state.h) -- storage is read with lanes along file x, the buffer written with lanes along file z.  The pad column keeps both
//     passes off each other's banks: rows of 33 Reals put the 32 lanes of a half wave on 32 different banks (fp32: 33 a mod 32; fp64, ds_read_b64:
//     66 a mod 64 = 2 a), and the row-wise pass is unit stride.
// Plain C++, wave64, 64-bit indices, every access guarded by the region's counts: no assumption about the counts, the strides or the grid.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pf {

// the piece of a region one launch cuts: first cell and stride in file coordinates, counts per axis (n0 * n1 * n2 cells = the staging buffer's extent)
struct RegionPiece { int64_t lo0, lo1, lo2, s0, s1, s2, n0, n1, n2; };

// grid: direct (cdiv(n2, bz), cdiv(n1, 256 / bz), n0); tiled (cdiv(n2, 32), n1, cdiv(n0, 32)).  256 threads.
// Ny, P: rows per plane and row pitch of the storage.
template <typename Real, bool EXCH>
static __global__ void __launch_bounds__(256) k_region_cut(const Real *__restrict__ st, Real *__restrict__ stage, RegionPiece q, int64_t Ny, int64_t P, int tiled, int bz_log2) {
   if (EXCH && tiled) {
      __shared__ Real tile[32][33];
      const int a = threadIdx.x & 31, b = threadIdx.x >> 5; // 32 x 8
      const int64_t j = blockIdx.y, kt = (int64_t)blockIdx.x * 32, it = (int64_t)blockIdx.z * 32;
      const int64_t fy = q.lo1 + j * q.s1;
#pragma unroll
      for (int r = 0; r < 4; r++) { // lanes along file x: the storage's unit-stride axis
         const int64_t i = it + a, k = kt + b + 8 * r;
         if (i < q.n0 && k < q.n2) tile[b + 8 * r][a] = st[((q.lo2 + k * q.s2) * Ny + fy) * P + q.lo0 + i * q.s0];
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; r++) { // lanes along file z: the buffer's
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
   stage[(i * q.n1 + j) * q.n2 + k] = EXCH ? st[(fz * Ny + fy) * P + fx] : st[(fx * Ny + fy) * P + fz];
}

} // namespace pf
