// pf_engine_region.inc -- part of `template <typename Real> struct Engine` (pf_engine_class.inc includes it INSIDE the class body; not a translation unit):
// pf_engine_get_region -- a strided box of u^{n-1} or u^n in the FILE's coordinates, cut on the device from whichever layout the engine stores
// (kernel: pf_region.h) into one staging buffer of at most pf::PF_REGION_STAGE_BYTES and copied to the host from there (large regions that are evenly
// pitched rows of file-order storage: copied as they lie, without the buffer).  Nothing the next step reads
// changes: the only device writes are the staging buffer and, for a region of u^n that touches a face of the grid in a virtual-ghost mode, the
// ghost shell get_grid(1) and save_state write too.  The receiver ring is left alone.
   struct RegionScratch {
      pf::DevMem &mem;
      Real *stage = nullptr;
      ~RegionScratch() { mem.release(stage); }
   };
   // host: dense, or (pitch > the region's z count) rows `pitch` elements apart -- a slab's columns of a chain's output (pf_region_cut.h)
   int get_region(int which, const pf_region *r, void *host, int64_t pitch) override {
      const char *what = "pf_engine_get_region";
      if (!r || !host) return set_err(PF_ERR_ARG, "%s: null %s", what, !r ? "pf_region" : "host array");
      if (which != 0 && which != 1) return set_err(PF_ERR_ARG, "%s: which = %d (0: u^{n-1}, 1: u^n)", what, which);
      const int64_t N[3] = {fNx, fNy, fNz};
      int64_t c[3];
      char msg[256];
      const int64_t total = pf_cut::region_check(r, N, c, msg, sizeof msg);
      if (total < 0) return set_err(PF_ERR_ARG, "%s: %s", what, msg);
      if (pitch <= 0) pitch = c[2];
      if (pitch < c[2]) return set_err(PF_ERR_ARG, "%s: output pitch %ld < the region's %ld cells along z", what, (long)pitch, (long)c[2]);
      if (in_step || in_pass()) return set_err(PF_ERR_STATE, "%s inside a split-phase step or pass (u^{n+1} is not complete in memory): valid between runs only", what);
      HIPCHK(hipSetDevice(op.device));
      int rc = sync();
      if (rc) return rc;
      const Real *src = which == 0 ? u0 : u1;
      bool shell = false; // does the region hold a cell of a face of the grid?
      for (int a = 0; a < 3; a++) shell = shell || r->lo[a] == 0 || r->lo[a] + (c[a] - 1) * r->stride[a] == N[a] - 1;
      if ((lean || vg) && which == 1 && shell) { // the virtual ghost shell, exactly as get_grid(1) writes it out
         launch_flips(s_main, grids());
         HIPCHK(hipGetLastError());
      }
      const int64_t cap = pf::PF_REGION_STAGE_BYTES / (int64_t)sizeof(Real);
      // More than the buffer holds, of file-order storage, unit strides, whole columns of y (or one plane): the region's rows are evenly pitched in
      // storage -- one pitched copy, as get_grid, and no staging at all (in pieces through the buffer the whole grid took 2.5 % longer than get_grid)
      if (!swz && total > cap && r->stride[0] == 1 && r->stride[1] == 1 && r->stride[2] == 1 && (c[1] == Ny || c[0] == 1)) {
         HIPCHK(hipStreamSynchronize(s_main));
         const Real *first = src + (r->lo[0] * Ny + r->lo[1]) * P + r->lo[2];
         HIPCHK(hipMemcpy2D(host, (size_t)pitch * sizeof(Real), first, (size_t)P * sizeof(Real), (size_t)c[2] * sizeof(Real), (size_t)(c[0] * c[1]), hipMemcpyDeviceToHost));
         return PF_OK;
      }
      // pieces along the slowest axis that does not fit the buffer whole: each is contiguous in the dense output
      const bool planes = c[1] * c[2] <= cap && c[1] <= 65535; // (a launch's grid has at most 65535 blocks along y and z)
      const int64_t n0 = planes ? std::min<int64_t>({c[0], cap / (c[1] * c[2]), (int64_t)65535}) : 1;
      const int64_t n1 = planes ? c[1] : (c[2] <= cap ? std::min<int64_t>({c[1], cap / c[2], (int64_t)65535}) : 1);
      const int64_t n2 = std::min(c[2], cap);
      RegionScratch sc{mem};
      if ((rc = dalloc(&sc.stage, n0 * n1 * n2))) return rc;
      std::vector<Real> rows; // a pitched output: the piece lands here first
      const bool dense = pitch == c[2];
      if (!dense) { try { rows.resize((size_t)(n0 * n1 * n2)); } catch (const std::bad_alloc &) { return set_err(PF_ERR_ARG, "%s: no host memory for a piece of the region", what); } }
      for (int64_t i0 = 0; i0 < c[0]; i0 += n0)
         for (int64_t j0 = 0; j0 < c[1]; j0 += n1)
            for (int64_t k0 = 0; k0 < c[2]; k0 += n2) {
               const pf::RegionPiece q{r->lo[0] + i0 * r->stride[0], r->lo[1] + j0 * r->stride[1], r->lo[2] + k0 * r->stride[2], r->stride[0], r->stride[1], r->stride[2],
                                       std::min(n0, c[0] - i0), std::min(n1, c[1] - j0), std::min(n2, c[2] - k0)};
               const bool tiled = swz && q.n0 >= 2 && q.n2 >= 2;
               int bzl = 0;
               while (bzl < 8 && ((int64_t)1 << bzl) < q.n2) bzl++;
               const dim3 g = tiled ? dim3((unsigned)cdiv(q.n2, 32), (unsigned)q.n1, (unsigned)cdiv(q.n0, 32))
                                    : dim3((unsigned)cdiv(q.n2, (int64_t)1 << bzl), (unsigned)cdiv(q.n1, 256 >> bzl), (unsigned)q.n0);
               if (swz) hipLaunchKernelGGL((pf::k_region_cut<Real, true>), g, dim3(256), 0, s_main, src, sc.stage, q, Ny, P, tiled ? 1 : 0, bzl);
               else hipLaunchKernelGGL((pf::k_region_cut<Real, false>), g, dim3(256), 0, s_main, src, sc.stage, q, Ny, P, 0, bzl);
               HIPCHK(hipGetLastError());
               const int64_t cells = q.n0 * q.n1 * q.n2;
               Real *out = (Real *)host + (i0 * c[1] + j0) * pitch + k0;
               HIPCHK(hipMemcpyAsync(dense ? out : rows.data(), sc.stage, (size_t)cells * sizeof(Real), hipMemcpyDeviceToHost, s_main));
               HIPCHK(hipStreamSynchronize(s_main)); // (the one staging buffer is free again)
               if (!dense)
                  for (int64_t row = 0; row < q.n0 * q.n1; row++) memcpy(out + row * pitch, rows.data() + row * q.n2, (size_t)q.n2 * sizeof(Real));
            }
      return PF_OK;
   }
