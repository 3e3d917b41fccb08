// pf_engine_state.inc -- part of `template <typename Real> struct Engine` (pf_engine_class.inc includes it INSIDE the class body; not a translation unit):
// pf_engine_save_state / pf_engine_load_state -- the whole state between two steps in its canonical form (include/pffdtd_hip.h: pf_state; kernels: pf_state.h).
// Between runs the state is (u0, u1) = u^{n-1}, u^n, the node values ub[2], ub[1] = u2b, u1b, and the branch state (vh1, gh1) -- whichever of the
// double-buffered copies end_pass left under those names.  Everything else the step drivers touch is scratch that a step writes before it reads.
   int state_refused(const char *what) {
      if (in_step || in_pass()) return set_err(PF_ERR_STATE, "%s inside a split-phase step or pass: valid between runs only", what);
      if (op.energy) return set_err(PF_ERR_STATE, "%s: an engine with the energy diagnostic keeps its sums with the caller (no checkpoint)", what);
      return PF_OK;
   }
   // one field, grid <-> host array in file order.  File-order storage: the pitched copy get_grid / set_grid use (no staging).  Exchanged axes:
   // pf::STATE_STAGE_PLANES file planes at a time through `stage` (that many compact file planes)
   int state_field(Real *grid, Real *host, bool to_host, Real *stage) {
      if (!swz) {
         if (to_host) HIPCHK(hipMemcpy2D(host, Nz * sizeof(Real), grid, P * sizeof(Real), Nz * sizeof(Real), Nx * Ny, hipMemcpyDeviceToHost));
         else HIPCHK(hipMemcpy2D(grid, P * sizeof(Real), host, Nz * sizeof(Real), Nz * sizeof(Real), Nx * Ny, hipMemcpyHostToDevice));
         return PF_OK;
      }
      const int64_t fplane = fNy * fNz;
      for (int64_t x0 = 0; x0 < fNx; x0 += pf::STATE_STAGE_PLANES) {
         const int64_t nx = std::min<int64_t>(pf::STATE_STAGE_PLANES, fNx - x0);
         const dim3 g((unsigned)cdiv(fNz, 32), (unsigned)fNy, (unsigned)cdiv(nx, 32));
         const size_t bytes = (size_t)(nx * fplane) * sizeof(Real);
         if (to_host) {
            hipLaunchKernelGGL((pf::k_state_planes<Real, true>), g, dim3(256), 0, s_main, grid, stage, x0, nx, fNy, fNz, Ny, P);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(host + x0 * fplane, stage, bytes, hipMemcpyDeviceToHost, s_main));
         } else {
            HIPCHK(hipMemcpyAsync(stage, host + x0 * fplane, bytes, hipMemcpyHostToDevice, s_main));
            hipLaunchKernelGGL((pf::k_state_planes<Real, false>), g, dim3(256), 0, s_main, grid, stage, x0, nx, fNy, fNz, Ny, P);
            HIPCHK(hipGetLastError());
         }
         HIPCHK(hipStreamSynchronize(s_main)); // (the one staging buffer is free again; a pageable host array makes the copy synchronous anyway)
      }
      return PF_OK;
   }
   // what both calls allocate for their duration: the fields' staging buffer (exchanged axes only) and the canonical node arrays on the device
   struct StateScratch {
      pf::DevMem &mem;
      Real *stage = nullptr, *node = nullptr;
      ~StateScratch() { mem.release(stage); mem.release(node); }
   };
   int state_scratch(StateScratch &sc) {
      int rc;
      if (swz && (rc = dalloc(&sc.stage, std::min<int64_t>(pf::STATE_STAGE_PLANES, fNx) * fNy * fNz))) return rc;
      if (Nbl && (rc = dalloc(&sc.node, Nbl * (2 * PF_MMB + 2)))) return rc; // vh1 | gh1 | u1b | u2b
      return PF_OK;
   }
   int state_args(const pf_state *st, const char *what) {
      if (!st) return set_err(PF_ERR_ARG, "%s: null pf_state", what);
      if (!st->u_prev || !st->u_cur) return set_err(PF_ERR_ARG, "%s: null field array", what);
      if (Nbl > 0 && (!st->u1b || !st->u2b || !st->vh1 || !st->gh1)) return set_err(PF_ERR_ARG, "%s: null node array (the scene has %ld frequency-dependent nodes)", what, (long)Nbl);
      return PF_OK;
   }
   int save_state(pf_state *st) override {
      int rc;
      if ((rc = state_args(st, "pf_engine_save_state"))) return rc;
      if ((rc = state_refused("pf_engine_save_state"))) return rc;
      HIPCHK(hipSetDevice(op.device));
      if ((rc = flush())) return rc;
      if ((rc = sync())) return rc;
      StateScratch sc{mem};
      if ((rc = state_scratch(sc))) return rc;
      if (lean || vg) { launch_flips(s_main, grids()); HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(s_main)); } // the virtual ghost shell of u^n, as get_grid(1)
      if ((rc = state_field(u0, (Real *)st->u_prev, true, sc.stage))) return rc;
      if ((rc = state_field(u1, (Real *)st->u_cur, true, sc.stage))) return rc;
      if (Nbl) {
         const size_t nb = (size_t)Nbl * PF_MMB;
         Real *cvh = sc.node, *cgh = cvh + nb, *cu1 = cgh + nb, *cu2 = cu1 + Nbl;
         hipLaunchKernelGGL((pf::k_state_pack<Real>), dim3((unsigned)cdiv(Nbl, 64)), dim3(64), 0, s_main, vh1, gh1, ub[1], ub[2], d_lperm, d_mat, d_Mb, Nbl, cvh, cgh, cu1, cu2);
         HIPCHK(hipGetLastError());
         HIPCHK(hipMemcpyAsync(st->vh1, cvh, nb * sizeof(Real), hipMemcpyDeviceToHost, s_main));
         HIPCHK(hipMemcpyAsync(st->gh1, cgh, nb * sizeof(Real), hipMemcpyDeviceToHost, s_main));
         HIPCHK(hipMemcpyAsync(st->u1b, cu1, (size_t)Nbl * sizeof(Real), hipMemcpyDeviceToHost, s_main));
         HIPCHK(hipMemcpyAsync(st->u2b, cu2, (size_t)Nbl * sizeof(Real), hipMemcpyDeviceToHost, s_main));
         HIPCHK(hipStreamSynchronize(s_main));
      }
      return PF_OK;
   }
   // After it the engine is a new engine that holds this state: nothing a run before the call left behind is read again.  The grids and node buffers keep
   // their roles (so the captured six-step graph, which replays only at the rotation phase it was captured at, still names the right buffers); their
   // contents are replaced, and every buffer that is scratch between runs goes back to the zeros a new engine has.
   int load_state(const pf_state *st) override {
      int rc;
      if ((rc = state_args(st, "pf_engine_load_state"))) return rc;
      if ((rc = state_refused("pf_engine_load_state"))) return rc;
      HIPCHK(hipSetDevice(op.device));
      if ((rc = flush())) return rc; // rows of the steps before: the caller's (sd->u_out)
      if ((rc = sync())) return rc;
      StateScratch sc{mem};
      if ((rc = state_scratch(sc))) return rc;
      state_touched = true;
      // the targets of the blocked passes (the triples' u^{n+1} grid among them)
      for (Real *g : {bufC, bufD, bufE})
         if (g && g != u0 && g != u1) HIPCHK(hipMemsetAsync(g, 0, (size_t)npad * sizeof(Real), s_main));
      if ((rc = state_field(u0, (Real *)st->u_prev, false, sc.stage))) return rc;
      if ((rc = state_field(u1, (Real *)st->u_cur, false, sc.stage))) return rc;
      const size_t nst = (size_t)round_up(Nbl, 64) * PF_MMB * sizeof(Real);
      HIPCHK(hipMemsetAsync(ub[0], 0, (size_t)std::max<int64_t>(Nbl, 1) * sizeof(Real), s_main));
      for (Real *x : {ubx[0], ubx[1]}) if (x) HIPCHK(hipMemsetAsync(x, 0, (size_t)std::max<int64_t>(Nbl, 1) * sizeof(Real), s_main));
      for (Real *x : {vh1b, gh1b}) if (x) HIPCHK(hipMemsetAsync(x, 0, nst, s_main));
      if (Nr) HIPCHK(hipMemsetAsync(ring, 0, (size_t)(Nr * ring_depth) * sizeof(Real), s_main));
      ring_fill = 0;
      if (Nbl) {
         const size_t nb = (size_t)Nbl * PF_MMB;
         Real *cvh = sc.node, *cgh = cvh + nb, *cu1 = cgh + nb, *cu2 = cu1 + Nbl;
         HIPCHK(hipMemcpyAsync(cvh, st->vh1, nb * sizeof(Real), hipMemcpyHostToDevice, s_main));
         HIPCHK(hipMemcpyAsync(cgh, st->gh1, nb * sizeof(Real), hipMemcpyHostToDevice, s_main));
         HIPCHK(hipMemcpyAsync(cu1, st->u1b, (size_t)Nbl * sizeof(Real), hipMemcpyHostToDevice, s_main));
         HIPCHK(hipMemcpyAsync(cu2, st->u2b, (size_t)Nbl * sizeof(Real), hipMemcpyHostToDevice, s_main));
         hipLaunchKernelGGL((pf::k_state_unpack<Real>), dim3((unsigned)cdiv(Nbl, 64)), dim3(64), 0, s_main, vh1, gh1, ub[1], ub[2], d_lperm, d_mat, d_Mb, Nbl, cvh, cgh, cu1, cu2);
         HIPCHK(hipGetLastError());
      }
      HIPCHK(hipStreamSynchronize(s_main));
      return PF_OK;
   }
