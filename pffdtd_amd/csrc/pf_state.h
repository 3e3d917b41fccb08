// pf_state.h -- device side of pf_engine_save_state / pf_engine_load_state (include/pffdtd_hip.h: pf_state): the conversion between the
// engine's own arrangement of a run's state and its canonical form, the one the reference's run_sim carries across its loop in the FILE's terms.
//   * node state: the engine keeps the lossy nodes sorted by storage index and their branch state in blocks of 64 nodes
//     ([node / 64][branch][node % 64], pf::st_idx); the canonical arrays follow sd->bnl_ixyz, [row * PF_MMB + branch] (cpu_engine.h:363-402).
//     k_state_pack / k_state_unpack move one tile of 64 nodes x 12 branches of both arrays through LDS: the engine's side in whole 64-lane
//     rows, the canonical side in runs of 12 (whole lines where the permutation is contiguous).  One read and one write of the state.
//   * fields of an engine that stores the file's x and z axes exchanged: k_state_to_file / k_state_from_file transpose PF_STATE_STAGE_PLANES
//     file planes at a time between the grid and a compact staging buffer in file order, 32 x 32 tiles through LDS.
// Plain C++, wave64, no assumption about Nbl % 64 or the grid's dimensions.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "pf_kernels.h"

namespace pf {

constexpr int STATE_STAGE_PLANES = 32; // file planes per chunk of a field: the staging buffer holds this many, whatever the grid's size
constexpr int64_t PF_REGION_STAGE_BYTES = (int64_t)32 << 20; // pf_engine_get_region (pf_region.h): its staging buffer holds at most this much, whatever the region's size
constexpr int STATE_LDS_ROW = 13;     // a node's 12 branches, padded: the two access patterns of a tile both spread over the banks

// perm[li] = row of sd->bnl_ixyz that the engine's lossy node li is (duplicates of an index keep a row each); mat / Mb: the node's material,
// its branch count.  Branch slots m >= Mb[mat] are written as 0.  One block = one wave = one tile of 64 nodes.
template <typename Real>
static __global__ void __launch_bounds__(64) k_state_pack(const Real *__restrict__ vh1, const Real *__restrict__ gh1, const Real *__restrict__ u1b,
                                                          const Real *__restrict__ u2b, const int64_t *__restrict__ perm, const int8_t *__restrict__ mat,
                                                          const int8_t *__restrict__ Mb, int64_t Nbl, Real *__restrict__ cvh, Real *__restrict__ cgh,
                                                          Real *__restrict__ cu1, Real *__restrict__ cu2) {
   __shared__ Real tv[64 * STATE_LDS_ROW], tg[64 * STATE_LDS_ROW];
   __shared__ int64_t row[64];
   const int lane = threadIdx.x;
   const int64_t li0 = (int64_t)blockIdx.x * 64, li = li0 + lane;
   const bool live = li < Nbl;
   const int M = live ? (int)Mb[mat[li]] : 0;
   row[lane] = live ? perm[li] : -1;
   if (live) { cu1[row[lane]] = u1b[li]; cu2[row[lane]] = u2b[li]; }
#pragma unroll
   for (int m = 0; m < 12; m++) { // (the arrays hold round_up(Nbl, 64) * 12 elements: a whole row of the last tile is there, but only live lanes count)
      const int64_t s = st_idx(m, li);
      tv[lane * STATE_LDS_ROW + m] = (live && m < M) ? vh1[s] : (Real)0;
      tg[lane * STATE_LDS_ROW + m] = (live && m < M) ? gh1[s] : (Real)0;
   }
   __syncthreads();
#pragma unroll
   for (int k = 0; k < 12; k++) {
      const int j = k * 64 + lane, nd = j / 12, m = j - nd * 12;
      const int64_t r = row[nd];
      if (r >= 0) { cvh[r * 12 + m] = tv[nd * STATE_LDS_ROW + m]; cgh[r * 12 + m] = tg[nd * STATE_LDS_ROW + m]; }
   }
}

// the other way; slots m >= Mb[mat] and the lanes past Nbl of the last tile receive 0 (what a new engine holds there)
template <typename Real>
static __global__ void __launch_bounds__(64) k_state_unpack(Real *__restrict__ vh1, Real *__restrict__ gh1, Real *__restrict__ u1b, Real *__restrict__ u2b,
                                                            const int64_t *__restrict__ perm, const int8_t *__restrict__ mat, const int8_t *__restrict__ Mb,
                                                            int64_t Nbl, const Real *__restrict__ cvh, const Real *__restrict__ cgh,
                                                            const Real *__restrict__ cu1, const Real *__restrict__ cu2) {
   __shared__ Real tv[64 * STATE_LDS_ROW], tg[64 * STATE_LDS_ROW];
   __shared__ int64_t row[64];
   const int lane = threadIdx.x;
   const int64_t li0 = (int64_t)blockIdx.x * 64, li = li0 + lane;
   const bool live = li < Nbl;
   const int M = live ? (int)Mb[mat[li]] : 0;
   row[lane] = live ? perm[li] : -1;
   if (live) { u1b[li] = cu1[row[lane]]; u2b[li] = cu2[row[lane]]; }
   __syncthreads();
#pragma unroll
   for (int k = 0; k < 12; k++) {
      const int j = k * 64 + lane, nd = j / 12, m = j - nd * 12;
      const int64_t r = row[nd];
      tv[nd * STATE_LDS_ROW + m] = r >= 0 ? cvh[r * 12 + m] : (Real)0;
      tg[nd * STATE_LDS_ROW + m] = r >= 0 ? cgh[r * 12 + m] : (Real)0;
   }
   __syncthreads();
#pragma unroll
   for (int m = 0; m < 12; m++) {
      const int64_t s = st_idx(m, li); // < round_up(Nbl, 64) * 12: inside the arrays for every lane of the last tile
      vh1[s] = m < M ? tv[lane * STATE_LDS_ROW + m] : (Real)0;
      gh1[s] = m < M ? tg[lane * STATE_LDS_ROW + m] : (Real)0;
   }
}

// Exchanged-axes storage st[(fz * Ny + fy) * P + fx]  <->  file planes [x0, x0 + nx) in file order, compact: stage[((fx - x0) * fNy + fy) * fNz + fz].
// grid (z tiles, fNy, x tiles) x 256 threads; a tile is 32 file-x by 32 file-z cells of one row fy.
template <typename Real, bool TO_FILE>
static __global__ void __launch_bounds__(256) k_state_planes(Real *__restrict__ st, Real *__restrict__ stage, int64_t x0, int64_t nx, int64_t fNy, int64_t fNz,
                                                             int64_t Ny, int64_t P) {
   __shared__ Real tile[32][33];
   const int a = threadIdx.x & 31, b = threadIdx.x >> 5; // 32 x 8
   const int64_t fy = blockIdx.y, zt = (int64_t)blockIdx.x * 32, xt = (int64_t)blockIdx.z * 32;
   if (TO_FILE) {
#pragma unroll
      for (int r = 0; r < 4; r++) { // lanes along file x: unit stride in storage
         const int64_t xl = xt + a, fz = zt + b + 8 * r;
         if (xl < nx && fz < fNz) tile[b + 8 * r][a] = st[(fz * Ny + fy) * P + x0 + xl];
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; r++) { // lanes along file z: unit stride in the file
         const int64_t xl = xt + b + 8 * r, fz = zt + a;
         if (xl < nx && fz < fNz) stage[(xl * fNy + fy) * fNz + fz] = tile[a][b + 8 * r];
      }
   } else {
#pragma unroll
      for (int r = 0; r < 4; r++) {
         const int64_t xl = xt + b + 8 * r, fz = zt + a;
         if (xl < nx && fz < fNz) tile[a][b + 8 * r] = stage[(xl * fNy + fy) * fNz + fz];
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; r++) {
         const int64_t xl = xt + a, fz = zt + b + 8 * r;
         if (xl < nx && fz < fNz) st[(fz * Ny + fy) * P + x0 + xl] = tile[b + 8 * r][a];
      }
   }
}

} // namespace pf
