// pf_engine_band.inc -- part of `template <typename Real> struct Engine` (pf_engine_class.inc includes it INSIDE the class body, after
// pf_engine_accum.inc; not a translation unit): the band accumulators (kernels: pf_band.h).  Per cell of a region the sample u^n runs through npre
// shared second-order sections and then, per band, through nsec sections; its square is summed into the time bin the caller names.  The sample
// is an observer's with the one component 0 (observer_sample); a full ring is folded (k_band_pre, k_band_fold), and get, set and destroy fold or
// drop what is pending.
   struct Band : Observer {
      int npre = 0, nband = 0, nsec = 0, nbin = 0;
      double *E = nullptr, *st = nullptr, *coef = nullptr, *xpre = nullptr;
      int32_t *bins = nullptr;
      std::vector<int32_t> hbins; // [depth]: the pending samples' bins
      Band() : Observer(pfeng::OBS_BAND) {}
      int nsect() const { return npre + nband * nsec; }
      double *sums() const { return E; }
      int64_t erows() const { return (int64_t)nband * nbin; }
      int64_t srows() const { return (int64_t)nsect() * 2; }
   };

   int band_create(const pf_region *r, int npre, const double *pre_sos, int nband, int nsec, const double *band_sos, int64_t nbin, int depth, void **out) override {
      const char *what = "pf_engine_bandacc_create";
      static const int32_t cell[1] = {0};
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
      std::unique_ptr<Band> a(new Band());
      int rc = observer_region(what, r, 1, cell, a.get());
      if (rc) return rc;
      a->npre = npre; a->nband = nband; a->nsec = nsec; a->nbin = (int)nbin;
      a->depth = depth ? depth : pf::PF_BAND_DEFAULT_DEPTH;
      std::vector<double> hcoef;
      try {
         a->hbins.assign((size_t)a->depth, -1);
         hcoef.assign((size_t)std::max(a->nsect(), 1) * 5, 0.0);
      } catch (const std::bad_alloc &) { return set_err(PF_ERR_ARG, "%s: no host memory", what); }
      if (npre) memcpy(hcoef.data(), pre_sos, (size_t)npre * 5 * sizeof(double));
      if (nsec) memcpy(hcoef.data() + (size_t)npre * 5, band_sos, (size_t)nband * nsec * 5 * sizeof(double));
      HIPCHK(hipSetDevice(op.device));
      Band *b = a.get();
      if ((rc = observer_alloc(b, &b->E, b->erows() * b->cstride, true)) || (rc = observer_alloc(b, &b->st, b->srows() * b->cstride, true)) ||
          (rc = observer_alloc(b, &b->ring, (int64_t)b->depth * b->cells, false)) || (rc = observer_alloc(b, &b->coef, (int64_t)hcoef.size(), false)) ||
          (rc = observer_alloc(b, &b->bins, (int64_t)b->depth, false)) || (npre && (rc = observer_alloc(b, &b->xpre, (int64_t)b->depth * b->cstride, false))))
         return observer_release(b, rc);
      HIPCHK(hipMemcpy(a->coef, hcoef.data(), hcoef.size() * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipDeviceSynchronize()); // (the memsets ran on the null stream; our streams are non-blocking)
      observer_keep(a, out);
      return PF_OK;
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

   // what the two kinds of band accumulator share (A: Band with fold = band_fold, VBand with vband_fold): they differ in the create and in the fold
   template <typename A, typename Fold> int bands_add(const char *what, int kind, void *h, int64_t bin, Fold fold) {
      A *a = observer_of<A>(h, kind);
      int rc;
      if (a && (bin < -1 || bin >= a->nbin)) return set_err(PF_ERR_ARG, "%s: bin = %ld outside -1 .. %d", what, (long)bin, a->nbin - 1);
      if ((rc = observer_enter(what, h, kind, &a)) || (rc = observer_sample(a))) return rc;
      a->hbins[(size_t)a->fill] = (int32_t)bin;
      a->fill++;
      if (a->fill == a->depth) return fold(a);
      return PF_OK;
   }
   // sums [erows][cells], state [srows][cells] (may be null)
   template <typename A, typename Fold> int bands_get(const char *what, int kind, void *h, double *sums, double *state, int64_t pitch, int64_t rowstride, Fold fold) {
      if (!sums) return set_err(PF_ERR_ARG, "%s: null sums array", what);
      A *a;
      int rc = observer_enter(what, h, kind, &a);
      if (rc || (rc = fold(a))) return rc;
      return observer_rows2(what, a, a->sums(), a->erows(), sums, a->st, a->srows(), state, pitch, rowstride, true);
   }
   // null: zeros.  Pending samples are dropped.
   template <typename A> int bands_set(const char *what, int kind, void *h, const double *sums, const double *state, int64_t pitch, int64_t rowstride) {
      A *a;
      const int rc = observer_enter(what, h, kind, &a);
      if (rc) return rc;
      a->fill = 0;
      return observer_rows2(what, a, a->sums(), a->erows(), sums, a->st, a->srows(), state, pitch, rowstride, false);
   }

   int band_add(void *h, int64_t bin) override { return bands_add<Band>("pf_engine_bandacc_add", pfeng::OBS_BAND, h, bin, [&](Band *a) { return band_fold(a); }); }
   // sums [nband][nbin][cells], state [npre + nband*nsec][2][cells]
   int band_get(void *h, double *sums, double *state, int64_t pitch, int64_t rowstride) override {
      return bands_get<Band>("pf_engine_bandacc_get", pfeng::OBS_BAND, h, sums, state, pitch, rowstride, [&](Band *a) { return band_fold(a); });
   }
   int band_set(void *h, const double *sums, const double *state, int64_t pitch, int64_t rowstride) override {
      return bands_set<Band>("pf_engine_bandacc_set", pfeng::OBS_BAND, h, sums, state, pitch, rowstride);
   }
