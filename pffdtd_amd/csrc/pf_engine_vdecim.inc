// pf_engine_vdecim.inc -- part of `template <typename Real> struct Engine` (pf_engine_class.inc includes it INSIDE the class body, after
// pf_engine_vband.inc; not a translation unit): the decimating recorders, scalar (pf_decim) and vector (pf_vdecim) (kernels: pf_vdecim.h, and
// pf_vband.h's k_vband_pre for the sections per component).  Per cell of a region up to four components -- the cell of u^n, or a difference
// (pf_engine_observe.inc: observer_region's rules, observer_sample) -- run through their own npre second-order sections and each through a FIR of
// ntap taps whose every D-th output is kept as a frame [ncomp][cells] on the device.  Per pending sample the host writes down, once for all
// components, which tap it meets in each of the P slots and which frame row it completes (plan, orow: pf_vdecim.h); a full ring is folded
// (k_vband_pre, k_vdecim_fold, in greedy pieces of 16, 8, 4, 2, 1 samples); read, get_state, set_state and destroy fold or drop what is pending.
// The SCALAR recorder is this one with the one component 0 (`scalar`: pf_engine_decim_create's): a handle type of its own (pfeng::OBS_DECIM), which
// the vector recorder's functions refuse and the reverse, and pre_sos [npre][5] by that name in a refusal.  `what` is the public function's name.
   static int vdecim_kind(bool scalar) { return scalar ? pfeng::OBS_DECIM : pfeng::OBS_VDECIM; }
   struct VDecim : Observer {
      int npre = 0, ntap = 0, D = 0, P = 0;
      int64_t cap = 0, count = 0, rd = 0; // count: samples taken (the ring's included); rd: the next frame a read gives.  ceil(count / D) frames are complete
      double *acc = nullptr, *frames = nullptr, *st = nullptr, *coef = nullptr, *taps = nullptr, *xpre = nullptr;
      int32_t *plan = nullptr, *orow = nullptr;
      std::vector<int32_t> hplan; // [2][depth][P]: the pending samples' plan, then their orow
      explicit VDecim(bool scalar) : Observer(vdecim_kind(scalar)) {}
      int64_t done() const { return (count + D - 1) / D; }
      int64_t pending() const { return done() - rd; }
      int64_t arows() const { return (int64_t)this->ncomp * P; }
      int64_t srows() const { return (int64_t)this->ncomp * npre * 2; }
   };

   int vdecim_create(const char *what, bool scalar, const pf_region *r, int ncomp, const int32_t *comp, int npre, const double *pre_sos, int ntap, const double *taps, int factor,
                     int64_t cap, int depth, void **out) override {
      if (!r || !out) return set_err(PF_ERR_ARG, "%s: null %s", what, !r ? "pf_region" : "out");
      *out = nullptr;
      std::unique_ptr<VDecim> a(new VDecim(scalar));
      int rc = observer_region(what, r, ncomp, comp, a.get());
      if (rc) return rc;
      if (npre < 0 || npre > pf::PF_BAND_MAX_SECTIONS) return set_err(PF_ERR_ARG, "%s: npre = %d outside 0 .. %d", what, npre, pf::PF_BAND_MAX_SECTIONS);
      if (ntap < 1 || ntap > pf::PF_DECIM_MAX_TAPS) return set_err(PF_ERR_ARG, "%s: ntap = %d outside 1 .. %d", what, ntap, pf::PF_DECIM_MAX_TAPS);
      if (factor < 1 || factor > pf::PF_DECIM_MAX_FACTOR) return set_err(PF_ERR_ARG, "%s: factor = %d outside 1 .. %d", what, factor, pf::PF_DECIM_MAX_FACTOR);
      const int P = (ntap + factor - 1) / factor;
      if (P > pf::PF_DECIM_MAX_SLOTS)
         return set_err(PF_ERR_ARG, "%s: P = ceil(ntap / factor) = ceil(%d / %d) = %d outputs in flight, more than %d: a larger factor or fewer taps", what, ntap, factor, P,
                        pf::PF_DECIM_MAX_SLOTS);
      if (cap < 1 || cap > INT32_MAX) return set_err(PF_ERR_ARG, "%s: cap = %ld outside 1 .. %d", what, (long)cap, INT32_MAX);
      if (depth < 0 || depth > pf::PF_DECIM_MAX_DEPTH) return set_err(PF_ERR_ARG, "%s: depth = %d outside 0 (default) .. %d", what, depth, pf::PF_DECIM_MAX_DEPTH);
      if (npre > 0 && !pre_sos) return set_err(PF_ERR_ARG, "%s: null pre_sos with npre = %d", what, npre);
      if (!taps) return set_err(PF_ERR_ARG, "%s: null taps", what);
      for (int i = 0; i < ncomp * npre * 5; i++) {
         if (std::isfinite(pre_sos[i])) continue;
         if (scalar) return set_err(PF_ERR_ARG, "%s: pre_sos[%d][%d] is not finite", what, i / 5, i % 5);
         return set_err(PF_ERR_ARG, "%s: pre_sos[%d][%d][%d] is not finite", what, i / (5 * npre), i / 5 % npre, i % 5);
      }
      for (int i = 0; i < ntap; i++) if (!std::isfinite(taps[i])) return set_err(PF_ERR_ARG, "%s: taps[%d] is not finite", what, i);
      a->npre = npre; a->ntap = ntap; a->D = factor; a->P = P; a->cap = cap;
      a->depth = depth ? depth : pf::PF_VDECIM_DEFAULT_DEPTH;
      try { a->hplan.assign((size_t)2 * a->depth * P, -1); } catch (const std::bad_alloc &) { return set_err(PF_ERR_ARG, "%s: no host memory", what); }
      HIPCHK(hipSetDevice(op.device));
      VDecim *b = a.get();
      if ((rc = observer_alloc(b, &b->acc, b->arows() * b->cstride, true)) || (rc = observer_alloc(b, &b->frames, cap * ncomp * b->cstride, true)) ||
          (rc = observer_alloc(b, &b->st, std::max<int64_t>(b->srows(), 1) * b->cstride, true)) || (rc = observer_alloc(b, &b->ring, (int64_t)ncomp * b->depth * b->cells, false)) ||
          (rc = observer_alloc(b, &b->coef, (int64_t)std::max(ncomp * npre, 1) * 5, false)) || (rc = observer_alloc(b, &b->taps, (int64_t)ntap, false)) ||
          (rc = observer_alloc(b, &b->plan, (int64_t)b->depth * P, false)) || (rc = observer_alloc(b, &b->orow, (int64_t)b->depth * P, false)) ||
          (npre && (rc = observer_alloc(b, &b->xpre, (int64_t)ncomp * b->depth * b->cstride, false))))
         return observer_release(b, rc);
      if (npre) HIPCHK(hipMemcpy(a->coef, pre_sos, (size_t)ncomp * npre * 5 * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(a->taps, taps, (size_t)ntap * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipDeviceSynchronize()); // (the memsets ran on the null stream; our streams are non-blocking)
      observer_keep(a, out);
      return PF_OK;
   }

   // NT samples from ring position t0 on, all components
   template <int NT> void launch_vdecim_fold(VDecim *a, int t0) {
      constexpr int S = pf::PF_DECIM_SLOTS;
      const dim3 g((unsigned)cdiv(cdiv(a->cells, 2), 256), (unsigned)cdiv(a->P, S), (unsigned)a->ncomp);
      const int64_t rcomp = (int64_t)a->depth * a->cells, xcomp = (int64_t)a->depth * a->cstride, scomp = (int64_t)a->npre * 2 * a->cstride, acomp = (int64_t)a->P * a->cstride;
      const Real *ring = a->ring + (int64_t)t0 * a->cells;
      const int32_t *plan = a->plan + (int64_t)t0 * a->P, *orow = a->orow + (int64_t)t0 * a->P;
      if (a->npre) {
         double *xpre = a->xpre + (int64_t)t0 * a->cstride;
         hipLaunchKernelGGL((pf::k_vband_pre<Real, NT>), dim3(g.x, (unsigned)a->ncomp), dim3(256), 0, s_main, a->st, xpre, ring, (const double *)a->coef, a->cells, a->cstride, rcomp,
                            xcomp, scomp, a->npre);
         hipLaunchKernelGGL((pf::k_vdecim_fold<double, NT, S>), g, dim3(256), 0, s_main, a->acc, a->frames, (const double *)xpre, (const double *)a->taps, plan, orow, a->cells,
                            a->cstride, a->cstride, xcomp, acomp, a->ncomp, a->P);
      } else
         hipLaunchKernelGGL((pf::k_vdecim_fold<Real, NT, S>), g, dim3(256), 0, s_main, a->acc, a->frames, ring, (const double *)a->taps, plan, orow, a->cells, a->cstride, a->cells,
                            rcomp, acomp, a->ncomp, a->P);
   }
   int vdecim_fold(VDecim *a) {
      if (a->fill == 0) return PF_OK;
      if (a->fill > a->depth) return set_err(PF_ERR_STATE, "internal: %d samples in a decimating recorder's ring of %d", a->fill, a->depth);
      const size_t half = (size_t)a->depth * a->P, n = (size_t)a->fill * a->P * sizeof(int32_t);
      HIPCHK(hipMemcpyAsync(a->plan, a->hplan.data(), n, hipMemcpyHostToDevice, s_main));
      HIPCHK(hipMemcpyAsync(a->orow, a->hplan.data() + half, n, hipMemcpyHostToDevice, s_main));
      int t0 = 0;
      while (t0 < a->fill) { // greedy: 7 = 4 + 2 + 1, the samples still in call order
         const int left = a->fill - t0;
         if (left >= 16) { launch_vdecim_fold<16>(a, t0); t0 += 16; }
         else if (left >= 8) { launch_vdecim_fold<8>(a, t0); t0 += 8; }
         else if (left >= 4) { launch_vdecim_fold<4>(a, t0); t0 += 4; }
         else if (left >= 2) { launch_vdecim_fold<2>(a, t0); t0 += 2; }
         else { launch_vdecim_fold<1>(a, t0); t0 += 1; }
      }
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(s_main)); // (hplan is free again)
      a->fill = 0;
      return PF_OK;
   }

   int vdecim_add(const char *what, bool scalar, void *h) override {
      VDecim *a;
      int rc;
      if ((rc = observer_enter(what, h, vdecim_kind(scalar), &a))) return rc;
      if (a->count % a->D == 0 && a->pending() == a->cap) // (host arithmetic, before the cut: nothing has changed)
         return set_err(PF_ERR_STATE, "%s: sample %ld would complete frame %ld while cap = %ld frames are complete and unread: read some first", what, (long)a->count,
                        (long)(a->count / a->D), (long)a->cap);
      if ((rc = observer_sample(a))) return rc;
      const int64_t n = a->count, q = (n + a->D - 1) / a->D;
      int32_t *plan = a->hplan.data() + (size_t)a->fill * a->P, *orow = plan + (size_t)a->depth * a->P;
      for (int p = 0; p < a->P; p++) { // once per sample, for every component
         const int64_t m = q + (((p - q) % a->P) + a->P) % a->P, k = m * a->D - n; // the output slot p carries, and the tap this sample meets in it
         plan[p] = k < a->ntap ? (int32_t)k : -1;
         orow[p] = k == 0 ? (int32_t)(m % a->cap) : -1;
      }
      a->fill++;
      a->count++;
      if (a->fill == a->depth) return vdecim_fold(a);
      return PF_OK;
   }

   // the oldest min(max_frames, pending) frames in order, [nread][ncomp][cells]: n frames are n * ncomp consecutive device rows; they are marked read
   int vdecim_read(const char *what, bool scalar, void *h, double *frames, int64_t max_frames, int64_t *first, int64_t *nread, int64_t pitch, int64_t rowstride) override {
      if (!first || !nread) return set_err(PF_ERR_ARG, "%s: null %s", what, !first ? "first" : "nread");
      if (max_frames < 0) return set_err(PF_ERR_ARG, "%s: max_frames = %ld < 0", what, (long)max_frames);
      if (max_frames > 0 && !frames) return set_err(PF_ERR_ARG, "%s: null frames array", what);
      VDecim *a;
      int rc = observer_enter(what, h, vdecim_kind(scalar), &a);
      if (rc || (rc = vdecim_fold(a))) return rc;
      const int64_t n = std::min(max_frames, a->pending()), row0 = a->rd % a->cap, n1 = std::min(n, a->cap - row0); // rows row0 .., then the ring of frames wraps
      if (rowstride <= 0) rowstride = a->cells;
      const int64_t nc = a->ncomp;
      if ((rc = observer_rows(what, a, a->frames + row0 * nc * a->cstride, n1 * nc, frames, pitch, rowstride, true))) return rc;
      if ((rc = observer_rows(what, a, a->frames, (n - n1) * nc, frames + n1 * nc * rowstride, pitch, rowstride, true))) return rc;
      *first = a->rd;
      *nread = n;
      a->rd += n;
      return PF_OK;
   }

   // acc [ncomp][P][cells] in slot order, state [ncomp][npre][2][cells] (may be null); nothing is reset
   int vdecim_get_state(const char *what, bool scalar, void *h, double *acc, double *state, int64_t pitch, int64_t rowstride) override {
      if (!acc) return set_err(PF_ERR_ARG, "%s: null acc array", what);
      VDecim *a;
      int rc = observer_enter(what, h, vdecim_kind(scalar), &a);
      if (rc || (rc = vdecim_fold(a))) return rc;
      return observer_rows2(what, a, a->acc, a->arows(), acc, a->st, a->srows(), state, pitch, rowstride, true);
   }

   // null: zeros.  Pending samples and unread frames are dropped; the next frame to complete is ceil(count / D)
   int vdecim_set_state(const char *what, bool scalar, void *h, const double *acc, const double *state, int64_t pitch, int64_t rowstride, int64_t count) override {
      if (count < 0) return set_err(PF_ERR_ARG, "%s: count = %ld < 0", what, (long)count);
      VDecim *a;
      int rc = observer_enter(what, h, vdecim_kind(scalar), &a);
      if (rc) return rc;
      a->fill = 0;
      if ((rc = observer_rows2(what, a, a->acc, a->arows(), acc, a->st, a->srows(), state, pitch, rowstride, false))) return rc;
      a->count = count;
      a->rd = a->done();
      return PF_OK;
   }

   int vdecim_info(bool scalar, void *h, int64_t *count, int64_t *pending) const override {
      const VDecim *a = observer_of<VDecim>(h, vdecim_kind(scalar));
      if (!a) return PF_ERR_ARG;
      *count = a->count;
      *pending = a->pending();
      return PF_OK;
   }
