// pf_engine_accum.inc -- part of `template <typename Real> struct Engine` (pf_engine_class.inc includes it INSIDE the class body; not a translation unit):
// the field accumulators (kernel: pf_accum.h), running sums acc[m][cell] += w[m] * double(u^n[cell]) over a region of the field, on the device.
// A sample is u^n of the region exactly as pf_engine_get_region(1, ...) gives it at the same moment -- the same kernel (k_region_cut) cuts it, into the
// next slot of the accumulator's ring instead of a staging buffer, and the virtual ghost shell is materialised under the same condition.  When the ring
// is full its samples are folded into the sums (k_accum_fold); get, set and destroy fold or drop what is pending.  Nothing a later step reads changes:
// the device writes are the accumulator's own three arrays and that ghost shell.  The receiver ring is left alone.  All device memory is `mem`'s.
   struct Accum {
      pf_region r{};
      int64_t c[3] = {0, 0, 0}, cells = 0, cstride = 0;
      int nchan = 0, depth = 0, fill = 0;   // fill: samples in the ring
      bool shell = false;                   // the region holds a cell of a face of the grid
      double *acc = nullptr, *wt = nullptr;
      Real *ring = nullptr;
      std::vector<double> hwt;              // [depth][nchan]: the pending samples' weights as the caller gave them
   };
   std::vector<std::unique_ptr<Accum>> accums;

   Accum *accum_of(void *h) const {
      for (const auto &a : accums) if (a.get() == h) return a.get();
      return nullptr;
   }
   void accum_free(Accum *a) { mem.release(a->acc); mem.release(a->ring); mem.release(a->wt); }

   int accum_create(const pf_region *r, int nchan, int depth, void **out) override {
      const char *what = "pf_engine_accum_create";
      if (!r || !out) return set_err(PF_ERR_ARG, "%s: null %s", what, !r ? "pf_region" : "out");
      *out = nullptr;
      if (nchan < 1 || nchan > pf::PF_ACCUM_MAX_CHANNELS) return set_err(PF_ERR_ARG, "%s: nchan = %d outside 1 .. %d", what, nchan, pf::PF_ACCUM_MAX_CHANNELS);
      if (depth < 0 || depth > pf::PF_ACCUM_MAX_DEPTH) return set_err(PF_ERR_ARG, "%s: depth = %d outside 0 (default) .. %d", what, depth, pf::PF_ACCUM_MAX_DEPTH);
      const int64_t N[3] = {fNx, fNy, fNz};
      char msg[256];
      std::unique_ptr<Accum> a(new Accum());
      a->cells = pf_cut::region_check(r, N, a->c, msg, sizeof msg);
      if (a->cells < 0) return set_err(PF_ERR_ARG, "%s: %s", what, msg);
      a->r = *r;
      a->nchan = nchan;
      a->depth = depth ? depth : pf::PF_ACCUM_DEFAULT_DEPTH;
      a->cstride = round_up(a->cells, 2);
      for (int k = 0; k < 3; k++) a->shell = a->shell || r->lo[k] == 0 || r->lo[k] + (a->c[k] - 1) * r->stride[k] == N[k] - 1;
      try { a->hwt.assign((size_t)a->depth * nchan, 0.0); } catch (const std::bad_alloc &) { return set_err(PF_ERR_ARG, "%s: no host memory", what); }
      HIPCHK(hipSetDevice(op.device));
      int rc;
      if ((rc = dzalloc(&a->acc, (int64_t)nchan * a->cstride)) || (rc = dalloc(&a->ring, (int64_t)a->depth * a->cells)) || (rc = dalloc(&a->wt, (int64_t)a->depth * nchan))) {
         accum_free(a.get());
         return rc;
      }
      HIPCHK(hipDeviceSynchronize()); // (the memset ran on the null stream; our streams are non-blocking)
      *out = a.get();
      accums.push_back(std::move(a));
      return PF_OK;
   }

   // what add, get and set share: the handle is this engine's, the engine stands between two runs, its streams have drained
   int accum_enter(const char *what, void *h, Accum **a) {
      if (!h) return set_err(PF_ERR_ARG, "%s: null pf_accum", what);
      if (!(*a = accum_of(h))) return set_err(PF_ERR_ARG, "%s: the pf_accum belongs to another engine", what);
      if (in_step || in_pass()) return set_err(PF_ERR_STATE, "%s inside a split-phase step or pass (u^{n+1} is not complete in memory): valid between runs only", what);
      HIPCHK(hipSetDevice(op.device));
      return sync();
   }

   template <int NT> void launch_fold(Accum *a) {
      hipLaunchKernelGGL((pf::k_accum_fold<Real, NT>), dim3((unsigned)cdiv(cdiv(a->cells, 2), 256)), dim3(256), 0, s_main, a->acc, a->ring, a->wt, a->cells, a->cstride, a->nchan);
   }
   int accum_fold(Accum *a) {
      if (a->fill == 0) return PF_OK;
      HIPCHK(hipMemcpyAsync(a->wt, a->hwt.data(), (size_t)a->fill * a->nchan * sizeof(double), hipMemcpyHostToDevice, s_main));
      switch (a->fill) {
#define PF_FOLD(n) case n: launch_fold<n>(a); break;
         PF_FOLD(1) PF_FOLD(2) PF_FOLD(3) PF_FOLD(4) PF_FOLD(5) PF_FOLD(6) PF_FOLD(7) PF_FOLD(8)
         PF_FOLD(9) PF_FOLD(10) PF_FOLD(11) PF_FOLD(12) PF_FOLD(13) PF_FOLD(14) PF_FOLD(15) PF_FOLD(16)
#undef PF_FOLD
         default: return set_err(PF_ERR_STATE, "internal: %d samples in an accumulator's ring", a->fill);
      }
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(s_main)); // (hwt is free again)
      a->fill = 0;
      return PF_OK;
   }

   // u^n of a region -> a ring slot of `cells` Reals, dense (the accumulators' and the band accumulators' sample)
   int region_to_slot(const pf_region &r, const int64_t *c, bool shell, Real *slot) {
      if ((lean || vg) && shell) { // the virtual ghost shell, exactly as get_region(1) writes it out
         launch_flips(s_main, grids());
         HIPCHK(hipGetLastError());
      }
      // u^n of the region -> the next ring slot.  Pieces only where a launch's grid demands them (at most 65535 blocks along y and z): blocks of
      // planes, or -- more than 65535 rows in a plane -- runs of rows of one plane; both contiguous in the slot
      const bool planes = c[1] <= 65535;
      const int64_t n0 = planes ? std::min<int64_t>(c[0], 65535) : 1, n1 = planes ? c[1] : 65535;
      for (int64_t i0 = 0; i0 < c[0]; i0 += n0)
         for (int64_t j0 = 0; j0 < c[1]; j0 += n1) {
            const pf::RegionPiece q{r.lo[0] + i0 * r.stride[0], r.lo[1] + j0 * r.stride[1], r.lo[2], r.stride[0], r.stride[1], r.stride[2],
                                    std::min(n0, c[0] - i0), std::min(n1, c[1] - j0), c[2]};
            const bool tiled = swz && q.n0 >= 2 && q.n2 >= 2;
            int bzl = 0;
            while (bzl < 8 && ((int64_t)1 << bzl) < q.n2) bzl++;
            const dim3 g = tiled ? dim3((unsigned)cdiv(q.n2, 32), (unsigned)q.n1, (unsigned)cdiv(q.n0, 32))
                                 : dim3((unsigned)cdiv(q.n2, (int64_t)1 << bzl), (unsigned)cdiv(q.n1, 256 >> bzl), (unsigned)q.n0);
            Real *out = slot + (i0 * c[1] + j0) * c[2];
            if (swz) hipLaunchKernelGGL((pf::k_region_cut<Real, true>), g, dim3(256), 0, s_main, (const Real *)u1, out, q, Ny, P, tiled ? 1 : 0, bzl);
            else hipLaunchKernelGGL((pf::k_region_cut<Real, false>), g, dim3(256), 0, s_main, (const Real *)u1, out, q, Ny, P, 0, bzl);
            HIPCHK(hipGetLastError());
         }
      return PF_OK;
   }

   int accum_add(void *h, const double *w) override {
      const char *what = "pf_engine_accum_add";
      if (!w) return set_err(PF_ERR_ARG, "%s: null weights", what);
      Accum *a;
      int rc = accum_enter(what, h, &a);
      if (rc) return rc;
      if ((rc = region_to_slot(a->r, a->c, a->shell, a->ring + (int64_t)a->fill * a->cells))) return rc;
      memcpy(a->hwt.data() + (size_t)a->fill * a->nchan, w, (size_t)a->nchan * sizeof(double));
      a->fill++;
      if (a->fill == a->depth) return accum_fold(a);
      return PF_OK;
   }

   // host: [nchan][cells] dense (pitch, chstride = 0), or -- a slab's part of a chain's array -- rows `pitch` and channels `chstride` doubles apart
   int accum_get(void *h, double *host, int64_t pitch, int64_t chstride) override {
      const char *what = "pf_engine_accum_get";
      if (!host) return set_err(PF_ERR_ARG, "%s: null host array", what);
      Accum *a;
      int rc = accum_enter(what, h, &a);
      if (rc) return rc;
      if ((rc = accum_fold(a))) return rc;
      if (pitch <= 0) pitch = a->c[2];
      if (chstride <= 0) chstride = a->cells;
      if (pitch < a->c[2]) return set_err(PF_ERR_ARG, "%s: output pitch %ld < the region's %ld cells along z", what, (long)pitch, (long)a->c[2]);
      const size_t row = (size_t)a->cells * sizeof(double);
      if (pitch == a->c[2]) { // a channel's cells are contiguous in the caller's array
         HIPCHK(hipMemcpy2D(host, (size_t)chstride * sizeof(double), a->acc, (size_t)a->cstride * sizeof(double), row, (size_t)a->nchan, hipMemcpyDeviceToHost));
         return PF_OK;
      }
      std::vector<double> tmp;
      try { tmp.resize((size_t)a->cells); } catch (const std::bad_alloc &) { return set_err(PF_ERR_ARG, "%s: no host memory for a channel of the region", what); }
      for (int m = 0; m < a->nchan; m++) {
         HIPCHK(hipMemcpy(tmp.data(), a->acc + (int64_t)m * a->cstride, row, hipMemcpyDeviceToHost));
         for (int64_t rw = 0; rw < a->c[0] * a->c[1]; rw++) memcpy(host + m * chstride + rw * pitch, tmp.data() + rw * a->c[2], (size_t)a->c[2] * sizeof(double));
      }
      return PF_OK;
   }

   // host null: zeros.  Pending samples are dropped.
   int accum_set(void *h, const double *host, int64_t pitch, int64_t chstride) override {
      const char *what = "pf_engine_accum_set";
      Accum *a;
      int rc = accum_enter(what, h, &a);
      if (rc) return rc;
      if (pitch <= 0) pitch = a->c[2];
      if (chstride <= 0) chstride = a->cells;
      if (pitch < a->c[2]) return set_err(PF_ERR_ARG, "%s: input pitch %ld < the region's %ld cells along z", what, (long)pitch, (long)a->c[2]);
      a->fill = 0;
      const size_t row = (size_t)a->cells * sizeof(double);
      if (!host) { HIPCHK(hipMemset(a->acc, 0, (size_t)a->nchan * a->cstride * sizeof(double))); HIPCHK(hipDeviceSynchronize()); return PF_OK; }
      if (pitch == a->c[2]) {
         HIPCHK(hipMemcpy2D(a->acc, (size_t)a->cstride * sizeof(double), host, (size_t)chstride * sizeof(double), row, (size_t)a->nchan, hipMemcpyHostToDevice));
         return PF_OK;
      }
      std::vector<double> tmp;
      try { tmp.resize((size_t)a->cells); } catch (const std::bad_alloc &) { return set_err(PF_ERR_ARG, "%s: no host memory for a channel of the region", what); }
      for (int m = 0; m < a->nchan; m++) {
         for (int64_t rw = 0; rw < a->c[0] * a->c[1]; rw++) memcpy(tmp.data() + rw * a->c[2], host + m * chstride + rw * pitch, (size_t)a->c[2] * sizeof(double));
         HIPCHK(hipMemcpy(a->acc + (int64_t)m * a->cstride, tmp.data(), row, hipMemcpyHostToDevice));
      }
      return PF_OK;
   }

   int accum_destroy(void *h) override {
      const char *what = "pf_engine_accum_destroy";
      if (!h) return set_err(PF_ERR_ARG, "%s: null pf_accum", what);
      Accum *a = accum_of(h);
      if (!a) return set_err(PF_ERR_ARG, "%s: the pf_accum belongs to another engine", what);
      HIPCHK(hipSetDevice(op.device));
      if (s_main) HIPCHK(hipStreamSynchronize(s_main));
      accum_free(a);
      accums.erase(std::find_if(accums.begin(), accums.end(), [&](const std::unique_ptr<Accum> &p) { return p.get() == a; }));
      return PF_OK;
   }
   bool between_runs() const override { return !(in_step || in_pass()); }
