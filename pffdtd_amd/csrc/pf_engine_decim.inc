// pf_engine_decim.inc -- part of `template <typename Real> struct Engine` (pf_engine_class.inc includes it INSIDE the class body, after
// pf_engine_vband.inc; not a translation unit): the decimating recorders (kernels: pf_decim.h, and pf_band.h's k_band_pre for the shared sections).
// Per cell of a region every sample u^n runs through npre second-order sections and a FIR of ntap taps whose every D-th output is kept as a frame
// on the device.  The sample is taken exactly as a band accumulator's (region_to_slot: k_region_cut into the next ring slot, the ghost shell under
// the same condition); per pending sample the host writes down which tap it meets in each of the P slots and which frame row it completes (plan,
// orow); a full ring is folded (k_band_pre, k_decim_fold, in greedy pieces of 16, 8, 4, 2, 1 samples); read, get_state, set_state and destroy fold
// or drop what is pending.  Nothing a later step reads changes.  All device memory is `mem`'s.
   struct Decim {
      pf_region r{};
      int64_t c[3] = {0, 0, 0}, cells = 0, cstride = 0;
      int npre = 0, ntap = 0, D = 0, P = 0, depth = 0, fill = 0; // fill: samples in the ring
      int64_t cap = 0, count = 0, rd = 0; // count: samples taken (the ring's included); rd: the next frame a read gives.  ceil(count / D) frames are complete
      bool shell = false;
      double *acc = nullptr, *frames = nullptr, *st = nullptr, *coef = nullptr, *taps = nullptr, *xpre = nullptr;
      int32_t *plan = nullptr, *orow = nullptr;
      Real *ring = nullptr;
      std::vector<int32_t> hplan; // [2][depth][P]: the pending samples' plan, then their orow
      int64_t done() const { return (count + D - 1) / D; }
      int64_t pending() const { return done() - rd; }
   };
   std::vector<std::unique_ptr<Decim>> decims;

   Decim *decim_of(void *h) const {
      for (const auto &a : decims) if (a.get() == h) return a.get();
      return nullptr;
   }
   void decim_free(Decim *a) {
      mem.release(a->acc); mem.release(a->frames); mem.release(a->st); mem.release(a->coef); mem.release(a->taps); mem.release(a->xpre); mem.release(a->plan);
      mem.release(a->orow); mem.release(a->ring);
   }

   int decim_create(const pf_region *r, int npre, const double *pre_sos, int ntap, const double *taps, int factor, int64_t cap, int depth, void **out) override {
      const char *what = "pf_engine_decim_create";
      if (!r || !out) return set_err(PF_ERR_ARG, "%s: null %s", what, !r ? "pf_region" : "out");
      *out = nullptr;
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
      for (int i = 0; i < npre * 5; i++) if (!std::isfinite(pre_sos[i])) return set_err(PF_ERR_ARG, "%s: pre_sos[%d][%d] is not finite", what, i / 5, i % 5);
      for (int i = 0; i < ntap; i++) if (!std::isfinite(taps[i])) return set_err(PF_ERR_ARG, "%s: taps[%d] is not finite", what, i);
      const int64_t N[3] = {fNx, fNy, fNz};
      char msg[256];
      std::unique_ptr<Decim> a(new Decim());
      a->cells = pf_cut::region_check(r, N, a->c, msg, sizeof msg);
      if (a->cells < 0) return set_err(PF_ERR_ARG, "%s: %s", what, msg);
      a->r = *r;
      a->npre = npre; a->ntap = ntap; a->D = factor; a->P = P; a->cap = cap;
      a->depth = depth ? depth : pf::PF_DECIM_DEFAULT_DEPTH;
      a->cstride = round_up(a->cells, 2);
      for (int k = 0; k < 3; k++) a->shell = a->shell || r->lo[k] == 0 || r->lo[k] + (a->c[k] - 1) * r->stride[k] == N[k] - 1;
      try { a->hplan.assign((size_t)2 * a->depth * P, -1); } catch (const std::bad_alloc &) { return set_err(PF_ERR_ARG, "%s: no host memory", what); }
      HIPCHK(hipSetDevice(op.device));
      int rc;
      if ((rc = dzalloc(&a->acc, (int64_t)P * a->cstride)) || (rc = dzalloc(&a->frames, cap * a->cstride)) || (rc = dzalloc(&a->st, (int64_t)std::max(npre, 1) * 2 * a->cstride)) ||
          (rc = dalloc(&a->ring, (int64_t)a->depth * a->cells)) || (rc = dalloc(&a->coef, (int64_t)std::max(npre, 1) * 5)) || (rc = dalloc(&a->taps, (int64_t)ntap)) ||
          (rc = dalloc(&a->plan, (int64_t)a->depth * P)) || (rc = dalloc(&a->orow, (int64_t)a->depth * P)) || (npre && (rc = dalloc(&a->xpre, (int64_t)a->depth * a->cstride)))) {
         decim_free(a.get());
         return rc;
      }
      if (npre) HIPCHK(hipMemcpy(a->coef, pre_sos, (size_t)npre * 5 * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(a->taps, taps, (size_t)ntap * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipDeviceSynchronize()); // (the memsets ran on the null stream; our streams are non-blocking)
      *out = a.get();
      decims.push_back(std::move(a));
      return PF_OK;
   }

   // what add, read, get_state and set_state share: the handle is this engine's, the engine stands between two runs, its streams have drained
   int decim_enter(const char *what, void *h, Decim **a) {
      if (!h) return set_err(PF_ERR_ARG, "%s: null pf_decim", what);
      if (!(*a = decim_of(h))) return set_err(PF_ERR_ARG, "%s: the pf_decim belongs to another engine", what);
      if (in_step || in_pass()) return set_err(PF_ERR_STATE, "%s inside a split-phase step or pass (u^{n+1} is not complete in memory): valid between runs only", what);
      HIPCHK(hipSetDevice(op.device));
      return sync();
   }

   // NT samples from ring position t0 on
   template <int NT> void launch_decim_fold(Decim *a, int t0) {
      constexpr int S = pf::PF_DECIM_SLOTS;
      const unsigned gx = (unsigned)cdiv(cdiv(a->cells, 2), 256), gy = (unsigned)cdiv(a->P, S);
      const Real *ring = a->ring + (int64_t)t0 * a->cells;
      const int32_t *plan = a->plan + (int64_t)t0 * a->P, *orow = a->orow + (int64_t)t0 * a->P;
      if (a->npre) {
         double *xpre = a->xpre + (int64_t)t0 * a->cstride;
         hipLaunchKernelGGL((pf::k_band_pre<Real, NT>), dim3(gx), dim3(256), 0, s_main, a->st, xpre, ring, (const double *)a->coef, a->cells, a->cstride, a->npre);
         hipLaunchKernelGGL((pf::k_decim_fold<double, NT, S>), dim3(gx, gy), dim3(256), 0, s_main, a->acc, a->frames, (const double *)xpre, (const double *)a->taps, plan, orow,
                            a->cells, a->cstride, a->cstride, a->P);
      } else
         hipLaunchKernelGGL((pf::k_decim_fold<Real, NT, S>), dim3(gx, gy), dim3(256), 0, s_main, a->acc, a->frames, ring, (const double *)a->taps, plan, orow, a->cells, a->cstride,
                            a->cells, a->P);
   }
   int decim_fold(Decim *a) {
      if (a->fill == 0) return PF_OK;
      if (a->fill > a->depth) return set_err(PF_ERR_STATE, "internal: %d samples in a decimating recorder's ring of %d", a->fill, a->depth);
      const size_t half = (size_t)a->depth * a->P, n = (size_t)a->fill * a->P * sizeof(int32_t);
      HIPCHK(hipMemcpyAsync(a->plan, a->hplan.data(), n, hipMemcpyHostToDevice, s_main));
      HIPCHK(hipMemcpyAsync(a->orow, a->hplan.data() + half, n, hipMemcpyHostToDevice, s_main));
      int t0 = 0;
      while (t0 < a->fill) { // greedy: 7 = 4 + 2 + 1, the samples still in call order
         const int left = a->fill - t0;
         if (left >= 16) { launch_decim_fold<16>(a, t0); t0 += 16; }
         else if (left >= 8) { launch_decim_fold<8>(a, t0); t0 += 8; }
         else if (left >= 4) { launch_decim_fold<4>(a, t0); t0 += 4; }
         else if (left >= 2) { launch_decim_fold<2>(a, t0); t0 += 2; }
         else { launch_decim_fold<1>(a, t0); t0 += 1; }
      }
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(s_main)); // (hplan is free again)
      a->fill = 0;
      return PF_OK;
   }

   int decim_add(void *h) override {
      const char *what = "pf_engine_decim_add";
      Decim *a;
      int rc;
      if ((rc = decim_enter(what, h, &a))) return rc;
      if (a->count % a->D == 0 && a->pending() == a->cap) // (host arithmetic, before the cut: nothing has changed)
         return set_err(PF_ERR_STATE, "%s: sample %ld would complete frame %ld while cap = %ld frames are complete and unread: read some first", what, (long)a->count,
                        (long)(a->count / a->D), (long)a->cap);
      if ((rc = region_to_slot(a->r, a->c, a->shell, a->ring + (int64_t)a->fill * a->cells))) return rc;
      const int64_t n = a->count, q = (n + a->D - 1) / a->D;
      int32_t *plan = a->hplan.data() + (size_t)a->fill * a->P, *orow = plan + (size_t)a->depth * a->P;
      for (int p = 0; p < a->P; p++) {
         const int64_t m = q + (((p - q) % a->P) + a->P) % a->P, k = m * a->D - n; // the output slot p carries, and the tap this sample meets in it
         plan[p] = k < a->ntap ? (int32_t)k : -1;
         orow[p] = k == 0 ? (int32_t)(m % a->cap) : -1;
      }
      a->fill++;
      a->count++;
      if (a->fill == a->depth) return decim_fold(a);
      return PF_OK;
   }

   // the oldest min(max_frames, pending) frames in order, [nread][cells]; they are marked read
   int decim_read(void *h, double *frames, int64_t max_frames, int64_t *first, int64_t *nread, int64_t pitch, int64_t rowstride) override {
      const char *what = "pf_engine_decim_read";
      if (!first || !nread) return set_err(PF_ERR_ARG, "%s: null %s", what, !first ? "first" : "nread");
      if (max_frames < 0) return set_err(PF_ERR_ARG, "%s: max_frames = %ld < 0", what, (long)max_frames);
      if (max_frames > 0 && !frames) return set_err(PF_ERR_ARG, "%s: null frames array", what);
      Decim *a;
      int rc = decim_enter(what, h, &a);
      if (rc || (rc = decim_fold(a))) return rc;
      const int64_t n = std::min(max_frames, a->pending()), row0 = a->rd % a->cap, n1 = std::min(n, a->cap - row0); // rows row0 .., then the ring of frames wraps
      if (rowstride <= 0) rowstride = a->cells;
      if ((rc = band_rows(what, a, a->frames + row0 * a->cstride, n1, frames, pitch, rowstride, true))) return rc;
      if ((rc = band_rows(what, a, a->frames, n - n1, frames + n1 * rowstride, pitch, rowstride, true))) return rc;
      *first = a->rd;
      *nread = n;
      a->rd += n;
      return PF_OK;
   }

   // acc [P][cells] in slot order, state [npre][2][cells] (may be null); nothing is reset
   int decim_get_state(void *h, double *acc, double *state, int64_t pitch, int64_t rowstride) override {
      const char *what = "pf_engine_decim_get_state";
      if (!acc) return set_err(PF_ERR_ARG, "%s: null acc array", what);
      Decim *a;
      int rc = decim_enter(what, h, &a);
      if (rc || (rc = decim_fold(a))) return rc;
      if ((rc = band_rows(what, a, a->acc, a->P, acc, pitch, rowstride, true))) return rc;
      return state ? band_rows(what, a, a->st, (int64_t)a->npre * 2, state, pitch, rowstride, true) : PF_OK;
   }

   // null: zeros.  Pending samples and unread frames are dropped; the next frame to complete is ceil(count / D)
   int decim_set_state(void *h, const double *acc, const double *state, int64_t pitch, int64_t rowstride, int64_t count) override {
      const char *what = "pf_engine_decim_set_state";
      if (count < 0) return set_err(PF_ERR_ARG, "%s: count = %ld < 0", what, (long)count);
      Decim *a;
      int rc = decim_enter(what, h, &a);
      if (rc) return rc;
      a->fill = 0;
      if (acc) { if ((rc = band_rows(what, a, a->acc, a->P, const_cast<double *>(acc), pitch, rowstride, false))) return rc; }
      else HIPCHK(hipMemset(a->acc, 0, (size_t)a->P * a->cstride * sizeof(double)));
      if (state) { if ((rc = band_rows(what, a, a->st, (int64_t)a->npre * 2, const_cast<double *>(state), pitch, rowstride, false))) return rc; }
      else if (a->npre) HIPCHK(hipMemset(a->st, 0, (size_t)a->npre * 2 * a->cstride * sizeof(double)));
      HIPCHK(hipDeviceSynchronize());
      a->count = count;
      a->rd = a->done();
      return PF_OK;
   }

   int decim_info(void *h, int64_t *count, int64_t *pending) const override {
      const Decim *a = decim_of(h);
      if (!a) return PF_ERR_ARG;
      *count = a->count;
      *pending = a->pending();
      return PF_OK;
   }

   int decim_destroy(void *h) override {
      const char *what = "pf_engine_decim_destroy";
      if (!h) return set_err(PF_ERR_ARG, "%s: null pf_decim", what);
      Decim *a = decim_of(h);
      if (!a) return set_err(PF_ERR_ARG, "%s: the pf_decim belongs to another engine", what);
      HIPCHK(hipSetDevice(op.device));
      if (s_main) HIPCHK(hipStreamSynchronize(s_main));
      decim_free(a);
      decims.erase(std::find_if(decims.begin(), decims.end(), [&](const std::unique_ptr<Decim> &p) { return p.get() == a; }));
      return PF_OK;
   }
