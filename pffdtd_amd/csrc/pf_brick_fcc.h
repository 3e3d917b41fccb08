// pf_brick_fcc.h -- the WHOLE shell of a 13-point blocked pair as bricks (folded FCC grids, CPU-exact or safeguarded arithmetic).
//
// k_brick (pf_brick.h) steps the twelve bars of the 7-point frame; here every cell outside the pair kernel's box -- x slabs, row strips,
// column strips, faces included -- belongs to a brick (pf_fcc_shell_cut.h cuts them): one workgroup holds the brick and a halo of `ns`
// cells in LDS and takes `ns` <= 2 plain single steps of the reference's loop on a region that shrinks by one cell per step (not on a
// face that ends at the grid's own shell).  Every cell is generic -- air with the ABC loss its info word names, rigid node,
// frequency-dependent node --, the branch ODEs run dense over the brick's node list; a brick reads u^{n-1}, u^n and the old branch
// state only and is independent of every other launch of the pass.
//
// THE GHOST RULE.  Ghost cells are never loaded or stored.  The flips of a step (oracle/pf_oracle_impl.inc:219-248) run fold row, then z,
// then y, then x, each over the full range of the other axes, so a ghost cell equals the cell whose coordinates are reflected axis by
// axis, independently: index 0 -> 2, index N-1 -> N-3 -- and on the folded axis y = Ny-1 -> Ny-2.  A neighbour at (x +- 1, y +- 1, z) of
// a cell at index 1 or N-2 is therefore read from the LDS cell at the reflected coordinates (edge and corner ghosts included); the
// second step applies the same rule to the brick's own u^{n+1}.
//
// Arithmetic: upd13 / upd_rigid<12> / abc_loss of pf_kernels.h, fd_regs of pf_wall.h, the twelve neighbours in the oracle's order
// (oracle/pf_oracle_impl.inc:277-289, adjacency bits :332-343) -- bit-identical to it.  Branch state and node values as in k_brick:
// sv_in -> registers for all steps -> sv_out for the nodes the brick owns; node values of step s go to O[s - 1]; halo nodes are
// evaluated but not stored.
#pragma once
#include "pf_brick.h"
#include "pf_fcc_shell_cut.h"

namespace pf {

static_assert(pf_fcc::BRICK_T == BRICK_T && pf_fcc::BRICK_KN == BRICK_KN, "the cut counts nodes for k_brick's thread layout");
static_assert(sizeof(pf_fcc::Node) == 8, "two words per node");
// (pf_fcc::lds_bytes, the host-only cut's count of a brick's LDS, is brick_lds_bytes of pf_brick.h as long as a branch is four Reals)
static_assert(sizeof(MatQuadT<float>) == 4 * sizeof(float) && sizeof(MatQuadT<double>) == 4 * sizeof(double), "pf_fcc::lds_bytes counts four Reals per branch");

template <typename Real> struct BrickFccParams {
   const Real *A, *B;     // u^{n-1}, u^n
   Real *G[2];            // where steps 1 .. ns go
   Real *O[2];            // node values of those steps (lossy arrays' order)
   int64_t plane;
   int32_t Nx, Ny, Nz, P;
   const pf_fcc::Brick *brk;
   const uint16_t *info;  // pf_fcc::INFO_*: adjacency bits | node | frequency-dependent; air cells: ABC count << 14
   const pf_fcc::Node *los;
   const Real *x2, *x1;   // node values u^{n-1}, u^n (lossy arrays' order): the u2b of steps 1 and 2; nobody writes them during the pass
   const Real *sv_in, *sg_in;
   Real *sv_out, *sg_out;
   const Real *ssaf;
   const int8_t *mat, *Mb;
   const MatQuadT<Real> *mq;
   const Real *beta;
   Real lo2, sl2, l;
   int32_t nmat, ns;
};

// frequency-dependent nodes a thread carries at most: BRICK_KN -- but one in fp64 with twelve branch slots, where two nodes' state (96 registers)
// beside the twelve neighbours of a cell do not fit the register file without scratch (the cut is told: pf_fcc::Scene::max_nodes)
template <typename Real, int MC> constexpr int brick_fcc_kn() { return (sizeof(Real) == 8 && MC > WALL_MC[0]) ? 1 : BRICK_KN; }

template <typename Real, int MC, bool SG>
__global__ __launch_bounds__(BRICK_T) void k_brick_fcc(BrickFccParams<Real> bp, Real a1, Real a2) {
   constexpr int KN = brick_fcc_kn<Real, MC>();
   extern __shared__ __attribute__((aligned(16))) unsigned char brick_fcc_smem[];
   const pf_fcc::Brick bk = bp.brk[blockIdx.x];
   const int tid = threadIdx.x;
   const uint32_t ey = (uint32_t)bk.en[1], ez = (uint32_t)bk.en[2];
   const uint32_t ncell = (uint32_t)bk.en[0] * ey * ez;
   const int syx = (int)(ey * ez), sy = (int)ez;
   MatQuadT<Real> *lmq = (MatQuadT<Real> *)brick_fcc_smem;
   Real *lbeta = (Real *)(lmq + bp.nmat * 12);
   int32_t *lM = (int32_t *)(lbeta + bp.nmat);
   Real *uo = (Real *)(((uintptr_t)(lM + bp.nmat) + 15) & ~(uintptr_t)15), *uc = uo + ncell, *un = uc + ncell;
   for (int i = tid; i < bp.nmat * 12; i += BRICK_T) lmq[i] = bp.mq[i];
   for (int i = tid; i < bp.nmat; i += BRICK_T) { lbeta[i] = bp.beta[i]; lM[i] = bp.Mb[i]; }
   const BrickLds<Real> lds{lmq, lbeta, lM};
   // this thread's frequency-dependent nodes: state and parameters, for all the steps
   Real fv[KN][12], fg[KN][12], fsf[KN], fx2[KN], fx1[KN];
   int32_t fk[KN], fli[KN];
   uint32_t fc[KN];
#pragma unroll
   for (int k = 0; k < KN; k++) {
      const uint32_t j = (uint32_t)tid + (uint32_t)k * BRICK_T;
      fc[k] = 0xffffffffu; fli[k] = 0; fk[k] = 0; fsf[k] = Real(0); fx2[k] = Real(0); fx1[k] = Real(0);
#pragma unroll
      for (int m = 0; m < 12; m++) { fv[k][m] = Real(0); fg[k][m] = Real(0); }
      if (j < bk.nlos) {
         const pf_fcc::Node e = bp.los[bk.los_off + j];
         fc[k] = e.cell; fli[k] = (int32_t)e.li;
#pragma unroll
         for (int m = 0; m < 12; m++)
            if (m < MC) { fv[k][m] = bp.sv_in[st_idx(m, fli[k])]; fg[k][m] = bp.sg_in[st_idx(m, fli[k])]; }
         fsf[k] = bp.ssaf[fli[k]];
         fk[k] = bp.mat[fli[k]];
         fx2[k] = bp.x2[fli[k]];
         fx1[k] = bp.x1[fli[k]];
      }
   }
   // u^{n-1}, u^n of the extended box
   for (uint32_t idx = tid; idx < ncell; idx += BRICK_T) {
      const uint32_t iz = idx % ez, t = idx / ez, iy = t % ey, ix = t / ey;
      const int64_t a = (int64_t)(bk.e0[0] + (int)ix) * bp.plane + (int64_t)(bk.e0[1] + (int)iy) * bp.P + (bk.e0[2] + (int)iz);
      uo[idx] = bp.A[a];
      uc[idx] = bp.B[a];
   }
   __syncthreads();
   const int N[3] = {bp.Nx, bp.Ny, bp.Nz};
   for (int s = 1; s <= bp.ns; s++) {
      // what this step can compute: `s` cells off every face of the extended box -- but a face that ends at the grid's own shell
      // (index 1 / N-2: beyond it only the mirrored ghost cell) loses nothing
      int lo[3], hi[3];
#pragma unroll
      for (int d = 0; d < 3; d++) {
         lo[d] = bk.e0[d] > 1 ? s : 0;
         hi[d] = bk.e0[d] + bk.en[d] < N[d] - 1 ? bk.en[d] - s : bk.en[d];
      }
      for (uint32_t idx = tid; idx < ncell; idx += BRICK_T) {
         const uint32_t iz = idx % ez, t = idx / ez, iy = t % ey, ix = t / ey;
         if ((int)ix < lo[0] || (int)ix >= hi[0] || (int)iy < lo[1] || (int)iy >= hi[1] || (int)iz < lo[2] || (int)iz >= hi[2]) continue;
         const int gx = bk.e0[0] + (int)ix, gy = bk.e0[1] + (int)iy, gz = bk.e0[2] + (int)iz;
         const uint32_t w = bp.info[bk.info_off + idx];
         const Real c = uc[idx], old = uo[idx];
         // the ghost rule: the step towards a ghost cell lands on its mirror image, axis by axis
         const int xp = gx == bp.Nx - 2 ? -syx : syx, xm = gx == 1 ? syx : -syx;
         const int yp = gy == bp.Ny - 2 ? 0 : sy, ym = gy == 1 ? sy : -sy; // (the fold: y = Ny-1 is y = Ny-2)
         const int zp = gz == bp.Nz - 2 ? -1 : 1, zm = gz == 1 ? 1 : -1;
         const Real *q = uc + idx;
         const Real nb[12] = {q[xp + yp], q[xm + ym], q[yp + zp], q[ym + zm], q[xp + zp], q[xm + zm],
                              q[xp + ym], q[xm + yp], q[yp + zm], q[ym + zp], q[xp + zm], q[xm + zp]};
         Real p;
         if (w & pf_fcc::INFO_NODE) p = upd_rigid<SG, 12>(a2, bp.sl2, w & pf_fcc::INFO_ADJ, c, old, nb); // boundary node
         else {
            p = upd13<SG>(a1, a2, c, old, nb);
            const uint32_t Q = w >> pf_fcc::INFO_Q_SHIFT;
            if (Q) p = abc_loss<SG>(p, old, bp.l * (Real)Q);
         }
         un[idx] = p;
      }
      __syncthreads();
      // the branch ODEs of the frequency-dependent nodes, dense; a node the step could not compute (halo) carries garbage from here
      // on, which nothing valid ever reads
#pragma unroll
      for (int k = 0; k < KN; k++) {
         if (fc[k] != 0xffffffffu) {
            const uint32_t cell = fc[k] & 0x7fffffffu;
            const Real u2 = s == 1 ? fx2[k] : fx1[k]; // the node's value two steps back: the engine's node-value buffers
            const Real u = fd_regs<Real, MC>(un[cell], u2, fsf[k], fk[k], fv[k], fg[k], fv[k], fg[k], lds, bp.lo2);
            un[cell] = u;
            if (fc[k] >> 31) bp.O[s - 1][fli[k]] = u;
         }
      }
      __syncthreads();
      { // the owned cells of this step
         Real *G = bp.G[s - 1];
         const uint32_t oy = (uint32_t)(bk.o1[1] - bk.o0[1]), oz = (uint32_t)(bk.o1[2] - bk.o0[2]), nown = (uint32_t)(bk.o1[0] - bk.o0[0]) * oy * oz;
         for (uint32_t j = tid; j < nown; j += BRICK_T) {
            const uint32_t kz = j % oz, t = j / oz, ky = t % oy, kx = t / oy;
            const int gx = bk.o0[0] + (int)kx, gy = bk.o0[1] + (int)ky, gz = bk.o0[2] + (int)kz;
            const uint32_t idx = ((uint32_t)(gx - bk.e0[0]) * ey + (uint32_t)(gy - bk.e0[1])) * ez + (uint32_t)(gz - bk.e0[2]);
            G[(int64_t)gx * bp.plane + (int64_t)gy * bp.P + gz] = un[idx];
         }
      }
      Real *t = uo; uo = uc; uc = un; un = t;
      // (no barrier: the next step writes what was `uo`, last read before the barrier above; the stores read what is `uc` now)
   }
#pragma unroll
   for (int k = 0; k < KN; k++) {
      if (fc[k] != 0xffffffffu && (fc[k] >> 31)) {
#pragma unroll
         for (int m = 0; m < 12; m++)
            if (m < MC) { bp.sv_out[st_idx(m, fli[k])] = fv[k][m]; bp.sg_out[st_idx(m, fli[k])] = fg[k][m]; }
      }
   }
}

} // namespace pf
