// pf_engine_vband.inc -- part of `template <typename Real> struct Engine` (pf_engine_class.inc includes it INSIDE the class body, after
// pf_engine_accum.inc; not a translation unit): the band accumulators, scalar (pf_bandacc) and vector (pf_vbandacc) (kernels: pf_vband.h).  Per cell
// of a region up to four components -- the cell of u^n itself, or a difference (pf_engine_observe.inc: observer_region's rules, observer_sample) --
// run through their own pre sections and, per band, through the band's sections (state per component); products of two filtered components are
// summed into the time bin the caller names.  A full ring is folded (k_vband_pre, k_vband_fold, in greedy pieces of 8, 4, 2, 1 samples); get, set
// and destroy fold or drop what is pending.
// The SCALAR accumulator is this one with the one component 0 and the one product (0, 0, 0), its square (`scalar`: pf_engine_bandacc_create's): a
// handle type of its own (pfeng::OBS_BAND), which the vector accumulator's functions refuse and the reverse, a ring of up to 16 samples (the vector
// kind's: 8), and pre_sos [npre][5] by that name in a refusal.  `what` is the public function's name.  Its object, create, add, get and set are the
// vector kind's; only its fold launches kernels of its own (pf_band.h: k_band_pre, k_band_fold, the ring in one launch), which give the same bits
// and measured 0.3 .. 1 % faster per sample than k_vband_fold with one component (profiles/field_decay_refactor.txt).
   static int vband_kind(bool scalar) { return scalar ? pfeng::OBS_BAND : pfeng::OBS_VBAND; }
   struct VBand : Observer {
      int npre = 0, nband = 0, nsec = 0, nprod = 0, nbin = 0;
      double *S = nullptr, *st = nullptr, *coef = nullptr, *xpre = nullptr;
      int32_t *bins = nullptr, *prod = nullptr;
      std::vector<int32_t> hbins; // [depth]: the pending samples' bins
      explicit VBand(bool scalar) : Observer(vband_kind(scalar)) {}
      int nsect() const { return npre + nband * nsec; } // per component
      int64_t srows() const { return (int64_t)this->ncomp * nsect() * 2; }
      int64_t erows() const { return (int64_t)nprod * nband * nbin; }
   };

   int vband_create(const char *what, bool scalar, const pf_region *r, int ncomp, const int32_t *comp, int npre, const double *pre_sos, int nband, int nsec, const double *band_sos,
                    int nprod, const int32_t *prod, int64_t nbin, int depth, void **out) override {
      const int max_depth = scalar ? pf::PF_BAND_MAX_DEPTH : pf::PF_VBAND_MAX_DEPTH;
      if (!r || !out) return set_err(PF_ERR_ARG, "%s: null %s", what, !r ? "pf_region" : "out");
      *out = nullptr;
      std::unique_ptr<VBand> a(new VBand(scalar));
      int rc = observer_region(what, r, ncomp, comp, a.get());
      if (rc) return rc;
      if (nband < 1 || nband > pf::PF_BAND_MAX_BANDS) return set_err(PF_ERR_ARG, "%s: nband = %d outside 1 .. %d", what, nband, pf::PF_BAND_MAX_BANDS);
      if (npre < 0 || npre > pf::PF_BAND_MAX_SECTIONS) return set_err(PF_ERR_ARG, "%s: npre = %d outside 0 .. %d", what, npre, pf::PF_BAND_MAX_SECTIONS);
      if (nsec < 0 || nsec > pf::PF_BAND_MAX_SECTIONS) return set_err(PF_ERR_ARG, "%s: nsec = %d outside 0 .. %d", what, nsec, pf::PF_BAND_MAX_SECTIONS);
      if (nprod < 1 || nprod > pf::PF_VBAND_MAX_PROD) return set_err(PF_ERR_ARG, "%s: nprod = %d outside 1 .. %d", what, nprod, pf::PF_VBAND_MAX_PROD);
      if (!prod) return set_err(PF_ERR_ARG, "%s: null prod", what);
      for (int p = 0; p < nprod; p++) {
         for (int m = 0; m < 2; m++)
            if (prod[3 * p + m] < 0 || prod[3 * p + m] >= ncomp) return set_err(PF_ERR_ARG, "%s: prod[%d][%d] = %d is no component index (ncomp = %d)", what, p, m, prod[3 * p + m], ncomp);
         if (prod[3 * p + 2] != 0 && prod[3 * p + 2] != 1) return set_err(PF_ERR_ARG, "%s: prod[%d][2] = %d: the mode is 0 (plain) or 1 (absolute value)", what, p, prod[3 * p + 2]);
      }
      if (nbin < 1 || nbin > INT32_MAX) return set_err(PF_ERR_ARG, "%s: nbin = %ld outside 1 .. %d", what, (long)nbin, INT32_MAX);
      if (depth < 0 || depth > max_depth) return set_err(PF_ERR_ARG, "%s: depth = %d outside 0 (default) .. %d", what, depth, max_depth);
      if (npre > 0 && !pre_sos) return set_err(PF_ERR_ARG, "%s: null pre_sos with npre = %d", what, npre);
      if (nsec > 0 && !band_sos) return set_err(PF_ERR_ARG, "%s: null band_sos with nsec = %d", what, nsec);
      for (int i = 0; i < ncomp * npre * 5; i++) {
         if (std::isfinite(pre_sos[i])) continue;
         if (scalar) return set_err(PF_ERR_ARG, "%s: pre_sos[%d][%d] is not finite", what, i / 5, i % 5);
         return set_err(PF_ERR_ARG, "%s: pre_sos[%d][%d][%d] is not finite", what, i / (5 * npre), i / 5 % npre, i % 5);
      }
      for (int i = 0; i < nband * nsec * 5; i++)
         if (!std::isfinite(band_sos[i])) return set_err(PF_ERR_ARG, "%s: band_sos[%d][%d][%d] is not finite", what, i / (5 * nsec), i / 5 % nsec, i % 5);
      a->npre = npre; a->nband = nband; a->nsec = nsec; a->nprod = nprod; a->nbin = (int)nbin;
      a->depth = depth ? depth : scalar ? pf::PF_BAND_DEFAULT_DEPTH : pf::PF_VBAND_DEFAULT_DEPTH;
      std::vector<double> hcoef;
      try {
         a->hbins.assign((size_t)a->depth, -1);
         hcoef.assign((size_t)std::max(ncomp * npre + nband * nsec, 1) * 5, 0.0);
      } catch (const std::bad_alloc &) { return set_err(PF_ERR_ARG, "%s: no host memory", what); }
      if (npre) memcpy(hcoef.data(), pre_sos, (size_t)ncomp * npre * 5 * sizeof(double));
      if (nsec) memcpy(hcoef.data() + (size_t)ncomp * npre * 5, band_sos, (size_t)nband * nsec * 5 * sizeof(double));
      HIPCHK(hipSetDevice(op.device));
      VBand *b = a.get();
      if ((rc = observer_alloc(b, &b->S, b->erows() * b->cstride, true)) || (rc = observer_alloc(b, &b->st, std::max<int64_t>(b->srows(), 1) * b->cstride, true)) ||
          (rc = observer_alloc(b, &b->ring, (int64_t)ncomp * b->depth * b->cells, false)) || (rc = observer_alloc(b, &b->coef, (int64_t)hcoef.size(), false)) ||
          (rc = observer_alloc(b, &b->bins, (int64_t)b->depth, false)) || (rc = observer_alloc(b, &b->prod, (int64_t)nprod * 3, false)) ||
          (npre && (rc = observer_alloc(b, &b->xpre, (int64_t)ncomp * b->depth * b->cstride, false))))
         return observer_release(b, rc);
      HIPCHK(hipMemcpy(a->coef, hcoef.data(), hcoef.size() * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(a->prod, prod, (size_t)nprod * 3 * sizeof(int32_t), hipMemcpyHostToDevice));
      HIPCHK(hipDeviceSynchronize()); // (the memsets ran on the null stream; our streams are non-blocking)
      observer_keep(a, out);
      return PF_OK;
   }

   // NT samples from ring position t0 on
   template <int NC, int NT> void launch_vband_fold(VBand *a, int t0) {
      const unsigned gx = (unsigned)cdiv(cdiv(a->cells, 2), 256);
      const int64_t scomp = (int64_t)a->nsect() * 2 * a->cstride, rcomp = (int64_t)a->depth * a->cells, xcomp = (int64_t)a->depth * a->cstride;
      const double *bcoef = a->coef + (int64_t)a->ncomp * a->npre * 5;
      const Real *ring = a->ring + (int64_t)t0 * a->cells;
      const int32_t *bins = a->bins + t0;
      if (a->npre) {
         double *xpre = a->xpre + (int64_t)t0 * a->cstride;
         hipLaunchKernelGGL((pf::k_vband_pre<Real, NT>), dim3(gx, (unsigned)a->ncomp), dim3(256), 0, s_main, a->st, xpre, ring, (const double *)a->coef, a->cells, a->cstride, rcomp,
                            xcomp, scomp, a->npre);
         hipLaunchKernelGGL((pf::k_vband_fold<double, NC, NT>), dim3(gx, (unsigned)a->nband), dim3(256), 0, s_main, a->S, a->st, (const double *)xpre, bcoef, bins,
                            (const int32_t *)a->prod, a->cells, a->cstride, a->cstride, xcomp, scomp, a->npre, a->nsec, a->nband, a->nbin, a->nprod);
      } else
         hipLaunchKernelGGL((pf::k_vband_fold<Real, NC, NT>), dim3(gx, (unsigned)a->nband), dim3(256), 0, s_main, a->S, a->st, ring, bcoef, bins, (const int32_t *)a->prod, a->cells,
                            a->cstride, a->cells, rcomp, scomp, a->npre, a->nsec, a->nband, a->nbin, a->nprod);
   }
   template <int NC> void launch_vband_pieces(VBand *a) { // greedy: 7 = 4 + 2 + 1, the samples still in call order
      int t0 = 0;
      while (t0 < a->fill) {
         const int left = a->fill - t0;
         if (left >= 8) { launch_vband_fold<NC, 8>(a, t0); t0 += 8; }
         else if (left >= 4) { launch_vband_fold<NC, 4>(a, t0); t0 += 4; }
         else if (left >= 2) { launch_vband_fold<NC, 2>(a, t0); t0 += 2; }
         else { launch_vband_fold<NC, 1>(a, t0); t0 += 1; }
      }
   }
   // the scalar kind: the whole ring, NT = fill samples, in one launch of its own kernels (pf_band.h) -- with one component and one product its
   // arrays ARE theirs: S [nband * nbin][cstride], st [(npre + nband*nsec) * 2][cstride], coef with the pre sections first
   template <int NT> void launch_band_fold(VBand *a) {
      const unsigned gx = (unsigned)cdiv(cdiv(a->cells, 2), 256);
      if (a->npre) {
         hipLaunchKernelGGL((pf::k_band_pre<Real, NT>), dim3(gx), dim3(256), 0, s_main, a->st, a->xpre, (const Real *)a->ring, (const double *)a->coef, a->cells, a->cstride, a->npre);
         hipLaunchKernelGGL((pf::k_band_fold<double, NT>), dim3(gx, (unsigned)a->nband), dim3(256), 0, s_main, a->S, a->st, (const double *)a->xpre, (const double *)a->coef,
                            (const int32_t *)a->bins, a->cells, a->cstride, a->cstride, a->npre, a->nsec, a->nbin);
      } else
         hipLaunchKernelGGL((pf::k_band_fold<Real, NT>), dim3(gx, (unsigned)a->nband), dim3(256), 0, s_main, a->S, a->st, (const Real *)a->ring, (const double *)a->coef,
                            (const int32_t *)a->bins, a->cells, a->cstride, a->cells, a->npre, a->nsec, a->nbin);
   }
   int vband_fold(VBand *a) {
      if (a->fill == 0) return PF_OK;
      if (a->fill > a->depth) return set_err(PF_ERR_STATE, "internal: %d samples in a vector band accumulator's ring of %d", a->fill, a->depth);
      HIPCHK(hipMemcpyAsync(a->bins, a->hbins.data(), (size_t)a->fill * sizeof(int32_t), hipMemcpyHostToDevice, s_main));
      switch (a->kind == pfeng::OBS_BAND ? -a->fill : a->ncomp) {
         case 1: launch_vband_pieces<1>(a); break;
         case 2: launch_vband_pieces<2>(a); break;
         case 3: launch_vband_pieces<3>(a); break;
         case 4: launch_vband_pieces<4>(a); break;
#define PF_FOLD(n) case -n: launch_band_fold<n>(a); break;
         PF_FOLD(1) PF_FOLD(2) PF_FOLD(3) PF_FOLD(4) PF_FOLD(5) PF_FOLD(6) PF_FOLD(7) PF_FOLD(8)
         PF_FOLD(9) PF_FOLD(10) PF_FOLD(11) PF_FOLD(12) PF_FOLD(13) PF_FOLD(14) PF_FOLD(15) PF_FOLD(16)
#undef PF_FOLD
         default: return set_err(PF_ERR_STATE, "internal: %d components, %d samples in a band accumulator", a->ncomp, a->fill);
      }
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(s_main)); // (hbins is free again)
      a->fill = 0;
      return PF_OK;
   }

   int vband_add(const char *what, bool scalar, void *h, int64_t bin) override {
      const int kind = vband_kind(scalar);
      VBand *a = observer_of<VBand>(h, kind);
      int rc;
      if (a && (bin < -1 || bin >= a->nbin)) return set_err(PF_ERR_ARG, "%s: bin = %ld outside -1 .. %d", what, (long)bin, a->nbin - 1);
      if ((rc = observer_enter(what, h, kind, &a)) || (rc = observer_sample(a))) return rc;
      a->hbins[(size_t)a->fill] = (int32_t)bin;
      a->fill++;
      if (a->fill == a->depth) return vband_fold(a);
      return PF_OK;
   }
   // sums [nprod][nband][nbin][cells], state [ncomp][npre + nband*nsec][2][cells] (may be null); the scalar kind's: without the leading 1
   int vband_get(const char *what, bool scalar, void *h, double *sums, double *state, int64_t pitch, int64_t rowstride) override {
      if (!sums) return set_err(PF_ERR_ARG, "%s: null sums array", what);
      VBand *a;
      int rc = observer_enter(what, h, vband_kind(scalar), &a);
      if (rc || (rc = vband_fold(a))) return rc;
      return observer_rows2(what, a, a->S, a->erows(), sums, a->st, a->srows(), state, pitch, rowstride, true);
   }
   // null: zeros.  Pending samples are dropped.
   int vband_set(const char *what, bool scalar, void *h, const double *sums, const double *state, int64_t pitch, int64_t rowstride) override {
      VBand *a;
      const int rc = observer_enter(what, h, vband_kind(scalar), &a);
      if (rc) return rc;
      a->fill = 0;
      return observer_rows2(what, a, a->S, a->erows(), sums, a->st, a->srows(), state, pitch, rowstride, false);
   }
