// pf_engine_accum.inc -- part of `template <typename Real> struct Engine` (pf_engine_class.inc includes it INSIDE the class body, after
// pf_engine_observe.inc; not a translation unit): the field accumulators (kernel: pf_accum.h), running sums acc[m][cell] += w[m] * double(u^n[cell])
// over a region of the field, on the device.  The sample is an observer's with the one component 0 (observer_sample).  When the ring is full its
// samples are folded into the sums (k_accum_fold); get, set and destroy fold or drop what is pending.  The receiver ring is left alone.
   struct Accum : Observer {
      int nchan = 0;
      double *acc = nullptr, *wt = nullptr;
      std::vector<double> hwt; // [depth][nchan]: the pending samples' weights as the caller gave them
      Accum() : Observer(pfeng::OBS_ACCUM) {}
   };

   int accum_create(const pf_region *r, int nchan, int depth, void **out) override {
      const char *what = "pf_engine_accum_create";
      static const int32_t cell[1] = {0};
      if (!r || !out) return set_err(PF_ERR_ARG, "%s: null %s", what, !r ? "pf_region" : "out");
      *out = nullptr;
      if (nchan < 1 || nchan > pf::PF_ACCUM_MAX_CHANNELS) return set_err(PF_ERR_ARG, "%s: nchan = %d outside 1 .. %d", what, nchan, pf::PF_ACCUM_MAX_CHANNELS);
      if (depth < 0 || depth > pf::PF_ACCUM_MAX_DEPTH) return set_err(PF_ERR_ARG, "%s: depth = %d outside 0 (default) .. %d", what, depth, pf::PF_ACCUM_MAX_DEPTH);
      std::unique_ptr<Accum> a(new Accum());
      int rc = observer_region(what, r, 1, cell, a.get());
      if (rc) return rc;
      a->nchan = nchan;
      a->depth = depth ? depth : pf::PF_ACCUM_DEFAULT_DEPTH;
      try { a->hwt.assign((size_t)a->depth * nchan, 0.0); } catch (const std::bad_alloc &) { return set_err(PF_ERR_ARG, "%s: no host memory", what); }
      HIPCHK(hipSetDevice(op.device));
      if ((rc = observer_alloc(a.get(), &a->acc, (int64_t)nchan * a->cstride, true)) || (rc = observer_alloc(a.get(), &a->ring, (int64_t)a->depth * a->cells, false)) ||
          (rc = observer_alloc(a.get(), &a->wt, (int64_t)a->depth * nchan, false)))
         return observer_release(a.get(), rc);
      HIPCHK(hipDeviceSynchronize()); // (the memset ran on the null stream; our streams are non-blocking)
      observer_keep(a, out);
      return PF_OK;
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

   int accum_add(void *h, const double *w) override {
      const char *what = "pf_engine_accum_add";
      if (!w) return set_err(PF_ERR_ARG, "%s: null weights", what);
      Accum *a;
      int rc = observer_enter(what, h, pfeng::OBS_ACCUM, &a);
      if (rc || (rc = observer_sample(a))) return rc;
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
      int rc = observer_enter(what, h, pfeng::OBS_ACCUM, &a);
      if (rc || (rc = accum_fold(a))) return rc;
      return observer_rows(what, a, a->acc, a->nchan, host, pitch, chstride, true);
   }

   // host null: zeros.  Pending samples are dropped.
   int accum_set(void *h, const double *host, int64_t pitch, int64_t chstride) override {
      const char *what = "pf_engine_accum_set";
      Accum *a;
      const int rc = observer_enter(what, h, pfeng::OBS_ACCUM, &a);
      if (rc) return rc;
      a->fill = 0;
      return observer_rows2(what, a, a->acc, a->nchan, host, nullptr, 0, nullptr, pitch, chstride, false);
   }
