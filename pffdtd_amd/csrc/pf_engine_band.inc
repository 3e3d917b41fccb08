// pf_engine_band.inc -- part of `template <typename Real> struct Engine` (pf_engine_class.inc includes it INSIDE the class body, after
// pf_engine_accum.inc; not a translation unit): the band accumulators (kernels: pf_band.h).  Per cell of a region the sample u^n runs through npre
// shared second-order sections and then, per band, through nsec sections; its square is summed into the time bin the caller names.  The sample
// is taken exactly as a field accumulator's (region_to_slot: k_region_cut into the next ring slot, the ghost shell under the same condition); a
// full ring is folded (k_band_pre, k_band_fold), and get, set and destroy fold or drop what is pending.  Nothing a later step reads changes.
// All device memory is `mem`'s.
   struct Band {
      pf_region r{};
      int64_t c[3] = {0, 0, 0}, cells = 0, cstride = 0;
      int npre = 0, nband = 0, nsec = 0, nbin = 0, depth = 0, fill = 0; // fill: samples in the ring
      bool shell = false;
      double *E = nullptr, *st = nullptr, *coef = nullptr, *xpre = nullptr;
      int32_t *bins = nullptr;
      Real *ring = nullptr;
      std::vector<int32_t> hbins; // [depth]: the pending samples' bins
      int nsect() const { return npre + nband * nsec; }
   };
   std::vector<std::unique_ptr<Band>> bands;

   Band *band_of(void *h) const {
      for (const auto &a : bands) if (a.get() == h) return a.get();
      return nullptr;
   }
   void band_free(Band *a) { mem.release(a->E); mem.release(a->st); mem.release(a->coef); mem.release(a->xpre); mem.release(a->bins); mem.release(a->ring); }

   int band_create(const pf_region *r, int npre, const double *pre_sos, int nband, int nsec, const double *band_sos, int64_t nbin, int depth, void **out) override {
      const char *what = "pf_engine_bandacc_create";
      if (!r || !out) return set_err(PF_ERR_ARG, "%s: null %s", what, !r ? "pf_region" : "out");
      *out = nullptr;
      if (nband < 1 || nband > pf::PF_BAND_MAX_BANDS) return set_err(PF_ERR_ARG, "%s: nband = %d outside 1 .. %d", what, nband, pf::PF_BAND_MAX_BANDS);
      if (npre < 0 || npre > pf::PF_BAND_MAX_SECTIONS) return set_err(PF_ERR_ARG, "%s: npre = %d outside 0 .. %d", what, npre, pf::PF_BAND_MAX_SECTIONS);
      if (nsec < 0 || nsec > pf::PF_BAND_MAX_SECTIONS) return set_err(PF_ERR_ARG, "%s: nsec = %d outside 0 .. %d", what, nsec, pf::PF_BAND_MAX_SECTIONS);
      if (nbin < 1 || nbin > INT32_MAX) return set_err(PF_ERR_ARG, "%s: nbin = %ld outside 1 .. %d", what, (long)nbin, INT32_MAX);
      if (depth < 0 || depth > pf::PF_BAND_MAX_DEPTH) return set_err(PF_ERR_ARG, "%s: depth = %d outside 0 (default) .. %d", what, depth, pf::PF_BAND_MAX_DEPTH);
      if (npre > 0 && !pre_sos) return set_err(PF_ERR_ARG, "%s: null pre_sos with npre = %d", what, npre);
      if (nsec > 0 && !band_sos) return set_err(PF_ERR_ARG, "%s: null band_sos with nsec = %d", what, nsec);
      for (int i = 0; i < npre * 5; i++) if (!std::isfinite(pre_sos[i])) return set_err(PF_ERR_ARG, "%s: pre_sos[%d][%d] is not finite", what, i / 5, i % 5);
      for (int i = 0; i < nband * nsec * 5; i++)
         if (!std::isfinite(band_sos[i])) return set_err(PF_ERR_ARG, "%s: band_sos[%d][%d][%d] is not finite", what, i / (5 * nsec), i / 5 % nsec, i % 5);
      const int64_t N[3] = {fNx, fNy, fNz};
      char msg[256];
      std::unique_ptr<Band> a(new Band());
      a->cells = pf_cut::region_check(r, N, a->c, msg, sizeof msg);
      if (a->cells < 0) return set_err(PF_ERR_ARG, "%s: %s", what, msg);
      a->r = *r;
      a->npre = npre; a->nband = nband; a->nsec = nsec; a->nbin = (int)nbin;
      a->depth = depth ? depth : pf::PF_BAND_DEFAULT_DEPTH;
      a->cstride = round_up(a->cells, 2);
      for (int k = 0; k < 3; k++) a->shell = a->shell || r->lo[k] == 0 || r->lo[k] + (a->c[k] - 1) * r->stride[k] == N[k] - 1;
      std::vector<double> hcoef;
      try {
         a->hbins.assign((size_t)a->depth, -1);
         hcoef.assign((size_t)std::max(a->nsect(), 1) * 5, 0.0);
      } catch (const std::bad_alloc &) { return set_err(PF_ERR_ARG, "%s: no host memory", what); }
      if (npre) memcpy(hcoef.data(), pre_sos, (size_t)npre * 5 * sizeof(double));
      if (nsec) memcpy(hcoef.data() + (size_t)npre * 5, band_sos, (size_t)nband * nsec * 5 * sizeof(double));
      HIPCHK(hipSetDevice(op.device));
      int rc;
      if ((rc = dzalloc(&a->E, (int64_t)nband * nbin * a->cstride)) || (rc = dzalloc(&a->st, (int64_t)a->nsect() * 2 * a->cstride)) ||
          (rc = dalloc(&a->ring, (int64_t)a->depth * a->cells)) || (rc = dalloc(&a->coef, (int64_t)hcoef.size())) || (rc = dalloc(&a->bins, (int64_t)a->depth)) ||
          (npre && (rc = dalloc(&a->xpre, (int64_t)a->depth * a->cstride)))) {
         band_free(a.get());
         return rc;
      }
      HIPCHK(hipMemcpy(a->coef, hcoef.data(), hcoef.size() * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipDeviceSynchronize()); // (the memsets ran on the null stream; our streams are non-blocking)
      *out = a.get();
      bands.push_back(std::move(a));
      return PF_OK;
   }

   // what add, get and set share: the handle is this engine's, the engine stands between two runs, its streams have drained
   int band_enter(const char *what, void *h, Band **a) {
      if (!h) return set_err(PF_ERR_ARG, "%s: null pf_bandacc", what);
      if (!(*a = band_of(h))) return set_err(PF_ERR_ARG, "%s: the pf_bandacc belongs to another engine", what);
      if (in_step || in_pass()) return set_err(PF_ERR_STATE, "%s inside a split-phase step or pass (u^{n+1} is not complete in memory): valid between runs only", what);
      HIPCHK(hipSetDevice(op.device));
      return sync();
   }

   template <int NT> void launch_band_fold(Band *a) {
      const unsigned gx = (unsigned)cdiv(cdiv(a->cells, 2), 256);
      if (a->npre) {
         hipLaunchKernelGGL((pf::k_band_pre<Real, NT>), dim3(gx), dim3(256), 0, s_main, a->st, a->xpre, (const Real *)a->ring, (const double *)a->coef, a->cells, a->cstride, a->npre);
         hipLaunchKernelGGL((pf::k_band_fold<double, NT>), dim3(gx, (unsigned)a->nband), dim3(256), 0, s_main, a->E, a->st, (const double *)a->xpre, (const double *)a->coef,
                            (const int32_t *)a->bins, a->cells, a->cstride, a->cstride, a->npre, a->nsec, a->nbin);
      } else
         hipLaunchKernelGGL((pf::k_band_fold<Real, NT>), dim3(gx, (unsigned)a->nband), dim3(256), 0, s_main, a->E, a->st, (const Real *)a->ring, (const double *)a->coef,
                            (const int32_t *)a->bins, a->cells, a->cstride, a->cells, a->npre, a->nsec, a->nbin);
   }
   int band_fold(Band *a) {
      if (a->fill == 0) return PF_OK;
      HIPCHK(hipMemcpyAsync(a->bins, a->hbins.data(), (size_t)a->fill * sizeof(int32_t), hipMemcpyHostToDevice, s_main));
      switch (a->fill) {
#define PF_FOLD(n) case n: launch_band_fold<n>(a); break;
         PF_FOLD(1) PF_FOLD(2) PF_FOLD(3) PF_FOLD(4) PF_FOLD(5) PF_FOLD(6) PF_FOLD(7) PF_FOLD(8)
         PF_FOLD(9) PF_FOLD(10) PF_FOLD(11) PF_FOLD(12) PF_FOLD(13) PF_FOLD(14) PF_FOLD(15) PF_FOLD(16)
#undef PF_FOLD
         default: return set_err(PF_ERR_STATE, "internal: %d samples in a band accumulator's ring", a->fill);
      }
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(s_main)); // (hbins is free again)
      a->fill = 0;
      return PF_OK;
   }

   int band_add(void *h, int64_t bin) override {
      const char *what = "pf_engine_bandacc_add";
      Band *a;
      int rc;
      if (h && (a = band_of(h)) && (bin < -1 || bin >= a->nbin)) return set_err(PF_ERR_ARG, "%s: bin = %ld outside -1 .. %d", what, (long)bin, a->nbin - 1);
      if ((rc = band_enter(what, h, &a))) return rc;
      if ((rc = region_to_slot(a->r, a->c, a->shell, a->ring + (int64_t)a->fill * a->cells))) return rc;
      a->hbins[(size_t)a->fill] = (int32_t)bin;
      a->fill++;
      if (a->fill == a->depth) return band_fold(a);
      return PF_OK;
   }

   // (A: any of the region observers -- Band, VBand, Decim, VDecim --, for its c, cells and cstride.)
   // `nrows` device rows, cstride doubles apart, <-> the caller's: dense (pitch, rowstride = 0) or -- a slab's part of a chain's array -- the region's
   // rows `pitch` and the device rows `rowstride` doubles apart
   template <typename A> int band_rows(const char *what, A *a, double *dev, int64_t nrows, double *host, int64_t pitch, int64_t rowstride, bool out) {
      if (pitch <= 0) pitch = a->c[2];
      if (rowstride <= 0) rowstride = a->cells;
      if (pitch < a->c[2]) return set_err(PF_ERR_ARG, "%s: pitch %ld < the region's %ld cells along z", what, (long)pitch, (long)a->c[2]);
      if (nrows == 0) return PF_OK;
      const size_t row = (size_t)a->cells * sizeof(double);
      if (pitch == a->c[2]) { // a row's cells are contiguous in the caller's array
         if (out) HIPCHK(hipMemcpy2D(host, (size_t)rowstride * sizeof(double), dev, (size_t)a->cstride * sizeof(double), row, (size_t)nrows, hipMemcpyDeviceToHost));
         else HIPCHK(hipMemcpy2D(dev, (size_t)a->cstride * sizeof(double), host, (size_t)rowstride * sizeof(double), row, (size_t)nrows, hipMemcpyHostToDevice));
         return PF_OK;
      }
      std::vector<double> tmp;
      try { tmp.resize((size_t)a->cells); } catch (const std::bad_alloc &) { return set_err(PF_ERR_ARG, "%s: no host memory for a row of the region", what); }
      for (int64_t m = 0; m < nrows; m++) {
         if (out) HIPCHK(hipMemcpy(tmp.data(), dev + m * a->cstride, row, hipMemcpyDeviceToHost));
         for (int64_t rw = 0; rw < a->c[0] * a->c[1]; rw++) {
            double *hp = host + m * rowstride + rw * pitch, *tp = tmp.data() + rw * a->c[2];
            if (out) memcpy(hp, tp, (size_t)a->c[2] * sizeof(double)); else memcpy(tp, hp, (size_t)a->c[2] * sizeof(double));
         }
         if (!out) HIPCHK(hipMemcpy(dev + m * a->cstride, tmp.data(), row, hipMemcpyHostToDevice));
      }
      return PF_OK;
   }

   // sums [nband][nbin][cells], state [npre + nband*nsec][2][cells] (may be null)
   int band_get(void *h, double *sums, double *state, int64_t pitch, int64_t rowstride) override {
      const char *what = "pf_engine_bandacc_get";
      if (!sums) return set_err(PF_ERR_ARG, "%s: null sums array", what);
      Band *a;
      int rc = band_enter(what, h, &a);
      if (rc || (rc = band_fold(a))) return rc;
      if ((rc = band_rows(what, a, a->E, (int64_t)a->nband * a->nbin, sums, pitch, rowstride, true))) return rc;
      return state ? band_rows(what, a, a->st, (int64_t)a->nsect() * 2, state, pitch, rowstride, true) : PF_OK;
   }

   // null: zeros.  Pending samples are dropped.
   int band_set(void *h, const double *sums, const double *state, int64_t pitch, int64_t rowstride) override {
      const char *what = "pf_engine_bandacc_set";
      Band *a;
      int rc = band_enter(what, h, &a);
      if (rc) return rc;
      a->fill = 0;
      if (sums) { if ((rc = band_rows(what, a, a->E, (int64_t)a->nband * a->nbin, const_cast<double *>(sums), pitch, rowstride, false))) return rc; }
      else HIPCHK(hipMemset(a->E, 0, (size_t)a->nband * a->nbin * a->cstride * sizeof(double)));
      if (state) { if ((rc = band_rows(what, a, a->st, (int64_t)a->nsect() * 2, const_cast<double *>(state), pitch, rowstride, false))) return rc; }
      else if (a->nsect()) HIPCHK(hipMemset(a->st, 0, (size_t)a->nsect() * 2 * a->cstride * sizeof(double)));
      HIPCHK(hipDeviceSynchronize());
      return PF_OK;
   }

   int band_destroy(void *h) override {
      const char *what = "pf_engine_bandacc_destroy";
      if (!h) return set_err(PF_ERR_ARG, "%s: null pf_bandacc", what);
      Band *a = band_of(h);
      if (!a) return set_err(PF_ERR_ARG, "%s: the pf_bandacc belongs to another engine", what);
      HIPCHK(hipSetDevice(op.device));
      if (s_main) HIPCHK(hipStreamSynchronize(s_main));
      band_free(a);
      bands.erase(std::find_if(bands.begin(), bands.end(), [&](const std::unique_ptr<Band> &p) { return p.get() == a; }));
      return PF_OK;
   }
