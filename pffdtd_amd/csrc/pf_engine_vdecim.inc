// pf_engine_vdecim.inc -- part of `template <typename Real> struct Engine` (pf_engine_class.inc includes it INSIDE the class body, after
// pf_engine_decim.inc; not a translation unit): the vector decimating recorders (kernels: pf_vdecim.h, and pf_vband.h's k_vband_pre for the sections per
// component).  Per cell of a region up to four components -- the cell of u^n, or a difference -- run through their own npre second-order sections and
// each through the FIR of a decimating recorder, every D-th output kept as a frame [ncomp][cells] on the device.  The sample is taken exactly as a
// vector band accumulator's (pf_engine_vband.inc: region_to_slot, diff_to_slot, ONE lat_to_slots for all lattice components, the ghost shell and a
// folded grid's fold row under the same conditions); plan and orow are a decimating recorder's, written down once per sample for all components; a
// full ring is folded (k_vband_pre, k_vdecim_fold, in greedy pieces of 16, 8, 4, 2, 1 samples); read, get_state, set_state and destroy fold or drop
// what is pending.  Nothing a later step reads changes.  All device memory is `mem`'s.
   struct VDecim {
      pf_region r{};
      int64_t c[3] = {0, 0, 0}, cells = 0, cstride = 0;
      int ncomp = 0, comp[pf::PF_VBAND_MAX_COMP] = {0, 0, 0, 0};
      int npre = 0, ntap = 0, D = 0, P = 0, depth = 0, fill = 0; // fill: samples in the ring
      int64_t cap = 0, count = 0, rd = 0; // as Decim's
      bool shell = false;
      int lat = 0; // bit 0 / 1 / 2: the lattice difference along file x / y / z is a component
      bool fold_row = false; // ... and the region's last row is Ny - 2 (a folded grid's fold row is read)
      double *acc = nullptr, *frames = nullptr, *st = nullptr, *coef = nullptr, *taps = nullptr, *xpre = nullptr;
      int32_t *plan = nullptr, *orow = nullptr;
      Real *ring = nullptr;
      std::vector<int32_t> hplan; // [2][depth][P]: the pending samples' plan, then their orow
      int64_t done() const { return (count + D - 1) / D; }
      int64_t pending() const { return done() - rd; }
      int64_t arows() const { return (int64_t)ncomp * P; }
      int64_t srows() const { return (int64_t)ncomp * npre * 2; }
   };
   std::vector<std::unique_ptr<VDecim>> vdecims;

   VDecim *vdecim_of(void *h) const {
      for (const auto &a : vdecims) if (a.get() == h) return a.get();
      return nullptr;
   }
   void vdecim_free(VDecim *a) {
      mem.release(a->acc); mem.release(a->frames); mem.release(a->st); mem.release(a->coef); mem.release(a->taps); mem.release(a->xpre); mem.release(a->plan);
      mem.release(a->orow); mem.release(a->ring);
   }

   int vdecim_create(const pf_region *r, int ncomp, const int32_t *comp, int npre, const double *pre_sos, int ntap, const double *taps, int factor, int64_t cap, int depth,
                     void **out) override {
      const char *what = "pf_engine_vdecim_create";
      static const char *axis_name[3] = {"x", "y", "z"};
      if (!r || !out) return set_err(PF_ERR_ARG, "%s: null %s", what, !r ? "pf_region" : "out");
      *out = nullptr;
      if (ncomp < 1 || ncomp > pf::PF_VBAND_MAX_COMP) return set_err(PF_ERR_ARG, "%s: ncomp = %d outside 1 .. %d", what, ncomp, pf::PF_VBAND_MAX_COMP);
      if (!comp) return set_err(PF_ERR_ARG, "%s: null comp", what);
      for (int k = 0; k < ncomp; k++) { // (the components and their refusals: pf_engine_vband_create's)
         if (comp[k] < 0 || comp[k] > 6)
            return set_err(PF_ERR_ARG, "%s: comp[%d] = %d outside 0 (the cell) .. 6 (1 / 2 / 3: the difference along file x / y / z; 4 / 5 / 6: the lattice difference of an FCC grid)", what,
                           k, comp[k]);
         if (comp[k] >= 4 && !fcc)
            return set_err(PF_ERR_ARG, "%s: comp[%d] = %d: a lattice difference (4 / 5 / 6) on fcc_flag == 0 -- its neighbours are the FCC stencil's; 1 / 2 / 3 are the differences of a "
                                       "Cartesian grid", what, k, comp[k]);
         for (int m = 0; m < k; m++) if (comp[m] == comp[k]) return set_err(PF_ERR_ARG, "%s: comp[%d] = comp[%d] = %d: a repeated component", what, m, k, comp[k]);
      }
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
      for (int i = 0; i < ncomp * npre * 5; i++)
         if (!std::isfinite(pre_sos[i])) return set_err(PF_ERR_ARG, "%s: pre_sos[%d][%d][%d] is not finite", what, i / (5 * npre), i / 5 % npre, i % 5);
      for (int i = 0; i < ntap; i++) if (!std::isfinite(taps[i])) return set_err(PF_ERR_ARG, "%s: taps[%d] is not finite", what, i);
      const int64_t N[3] = {fNx, fNy, fNz};
      char msg[256];
      std::unique_ptr<VDecim> a(new VDecim());
      a->cells = pf_cut::region_check(r, N, a->c, msg, sizeof msg);
      if (a->cells < 0) return set_err(PF_ERR_ARG, "%s: %s", what, msg);
      bool diff[3] = {false, false, false};
      for (int k = 0; k < ncomp; k++) {
         if (comp[k] >= 1 && comp[k] <= 3) diff[comp[k] - 1] = true;
         if (comp[k] >= 4) a->lat |= 1 << (comp[k] - 4);
      }
      if (fcc && (diff[0] || diff[1] || diff[2]))
         return set_err(PF_ERR_ARG, "%s: comp: a difference component (1 / 2 / 3) on fcc_flag != 0 -- an axis neighbour at +-1 is no node of the checkerboard; comp 4 / 5 / 6 are the "
                                    "lattice differences along file x / y / z, and comp = {0} alone works on every grid", what);
      for (int k = 0; k < 3; k++) {
         const int64_t last = r->lo[k] + (a->c[k] - 1) * r->stride[k];
         if (a->lat && (r->lo[k] < 1 || last > N[k] - 2)) // (every L_a reads neighbours along all three axes)
            return set_err(PF_ERR_ARG, "%s: a lattice difference needs the region one cell clear of all six faces, along file %s too: pf_region.lo[%d] = %ld >= 1 and its last cell "
                                       "%ld <= %ld", what, axis_name[k], k, (long)r->lo[k], (long)last, (long)N[k] - 2);
         if (diff[k] && (r->lo[k] < 1 || last > N[k] - 2))
            return set_err(PF_ERR_ARG, "%s: a difference along file %s needs the region one cell clear of both faces along %s: pf_region.lo[%d] = %ld >= 1 and its last cell %ld <= %ld",
                           what, axis_name[k], axis_name[k], k, (long)r->lo[k], (long)last, (long)N[k] - 2);
         const int64_t w = diff[k] || a->lat ? 1 : 0; // the cells actually read
         if (k == 1 && a->lat && last + 1 == N[1] - 1) a->fold_row = true;
         a->shell = a->shell || r->lo[k] - w == 0 || last + w == N[k] - 1;
      }
      a->r = *r;
      a->ncomp = ncomp; a->npre = npre; a->ntap = ntap; a->D = factor; a->P = P; a->cap = cap;
      for (int k = 0; k < ncomp; k++) a->comp[k] = comp[k];
      a->depth = depth ? depth : pf::PF_VDECIM_DEFAULT_DEPTH;
      a->cstride = round_up(a->cells, 2);
      try { a->hplan.assign((size_t)2 * a->depth * P, -1); } catch (const std::bad_alloc &) { return set_err(PF_ERR_ARG, "%s: no host memory", what); }
      HIPCHK(hipSetDevice(op.device));
      int rc;
      if ((rc = dzalloc(&a->acc, a->arows() * a->cstride)) || (rc = dzalloc(&a->frames, cap * ncomp * a->cstride)) || (rc = dzalloc(&a->st, std::max<int64_t>(a->srows(), 1) * a->cstride)) ||
          (rc = dalloc(&a->ring, (int64_t)ncomp * a->depth * a->cells)) || (rc = dalloc(&a->coef, (int64_t)std::max(ncomp * npre, 1) * 5)) || (rc = dalloc(&a->taps, (int64_t)ntap)) ||
          (rc = dalloc(&a->plan, (int64_t)a->depth * P)) || (rc = dalloc(&a->orow, (int64_t)a->depth * P)) ||
          (npre && (rc = dalloc(&a->xpre, (int64_t)ncomp * a->depth * a->cstride)))) {
         vdecim_free(a.get());
         return rc;
      }
      if (npre) HIPCHK(hipMemcpy(a->coef, pre_sos, (size_t)ncomp * npre * 5 * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(a->taps, taps, (size_t)ntap * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipDeviceSynchronize()); // (the memsets ran on the null stream; our streams are non-blocking)
      *out = a.get();
      vdecims.push_back(std::move(a));
      return PF_OK;
   }

   // what add, read, get_state and set_state share: the handle is this engine's, the engine stands between two runs, its streams have drained
   int vdecim_enter(const char *what, void *h, VDecim **a) {
      if (!h) return set_err(PF_ERR_ARG, "%s: null pf_vdecim", what);
      if (!(*a = vdecim_of(h))) return set_err(PF_ERR_ARG, "%s: the pf_vdecim belongs to another engine", what);
      if (in_step || in_pass()) return set_err(PF_ERR_STATE, "%s inside a split-phase step or pass (u^{n+1} is not complete in memory): valid between runs only", what);
      HIPCHK(hipSetDevice(op.device));
      return sync();
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
      if (a->fill > a->depth) return set_err(PF_ERR_STATE, "internal: %d samples in a vector decimating recorder's ring of %d", a->fill, a->depth);
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

   int vdecim_add(void *h) override {
      const char *what = "pf_engine_vdecim_add";
      VDecim *a;
      int rc;
      if ((rc = vdecim_enter(what, h, &a))) return rc;
      if (a->count % a->D == 0 && a->pending() == a->cap) // (host arithmetic, before the cut: nothing has changed)
         return set_err(PF_ERR_STATE, "%s: sample %ld would complete frame %ld while cap = %ld frames are complete and unread: read some first", what, (long)a->count,
                        (long)(a->count / a->D), (long)a->cap);
      if ((lean || vg) && a->shell) { // the virtual ghost shell, once for all components (vband_add's rule)
         launch_flips(s_main, grids());
         HIPCHK(hipGetLastError());
      } else if (fold && a->lat && a->fold_row) { // a folded grid's row Ny - 1, the copy of row Ny - 2 of u^n: written first, as vband_add does and says why
         hipLaunchKernelGGL(pf::k_flip_y<Real>, dim3((unsigned)cdiv(Nz, 256), (unsigned)Nx), dim3(256), 0, s_main, grids().cur, Nx, Ny, P, Nz, 4);
         HIPCHK(hipGetLastError());
      }
      Real *lslot[3] = {nullptr, nullptr, nullptr};
      for (int k = 0; k < a->ncomp; k++) {
         Real *slot = a->ring + ((int64_t)k * a->depth + a->fill) * a->cells;
         if (a->comp[k] >= 4) { lslot[a->comp[k] - 4] = slot; continue; }
         if ((rc = a->comp[k] == 0 ? region_to_slot(a->r, a->c, false, slot) : diff_to_slot(a->r, a->c, a->comp[k] - 1, slot))) return rc;
      }
      if (a->lat && (rc = lat_to_slots(a->r, a->c, a->lat, lslot))) return rc; // all of them in one launch
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
   int vdecim_read(void *h, double *frames, int64_t max_frames, int64_t *first, int64_t *nread, int64_t pitch, int64_t rowstride) override {
      const char *what = "pf_engine_vdecim_read";
      if (!first || !nread) return set_err(PF_ERR_ARG, "%s: null %s", what, !first ? "first" : "nread");
      if (max_frames < 0) return set_err(PF_ERR_ARG, "%s: max_frames = %ld < 0", what, (long)max_frames);
      if (max_frames > 0 && !frames) return set_err(PF_ERR_ARG, "%s: null frames array", what);
      VDecim *a;
      int rc = vdecim_enter(what, h, &a);
      if (rc || (rc = vdecim_fold(a))) return rc;
      const int64_t n = std::min(max_frames, a->pending()), row0 = a->rd % a->cap, n1 = std::min(n, a->cap - row0); // rows row0 .., then the ring of frames wraps
      if (rowstride <= 0) rowstride = a->cells;
      const int64_t nc = a->ncomp;
      if ((rc = band_rows(what, a, a->frames + row0 * nc * a->cstride, n1 * nc, frames, pitch, rowstride, true))) return rc;
      if ((rc = band_rows(what, a, a->frames, (n - n1) * nc, frames + n1 * nc * rowstride, pitch, rowstride, true))) return rc;
      *first = a->rd;
      *nread = n;
      a->rd += n;
      return PF_OK;
   }

   // acc [ncomp][P][cells] in slot order, state [ncomp][npre][2][cells] (may be null); nothing is reset
   int vdecim_get_state(void *h, double *acc, double *state, int64_t pitch, int64_t rowstride) override {
      const char *what = "pf_engine_vdecim_get_state";
      if (!acc) return set_err(PF_ERR_ARG, "%s: null acc array", what);
      VDecim *a;
      int rc = vdecim_enter(what, h, &a);
      if (rc || (rc = vdecim_fold(a))) return rc;
      if ((rc = band_rows(what, a, a->acc, a->arows(), acc, pitch, rowstride, true))) return rc;
      return state ? band_rows(what, a, a->st, a->srows(), state, pitch, rowstride, true) : PF_OK;
   }

   // null: zeros.  Pending samples and unread frames are dropped; the next frame to complete is ceil(count / D)
   int vdecim_set_state(void *h, const double *acc, const double *state, int64_t pitch, int64_t rowstride, int64_t count) override {
      const char *what = "pf_engine_vdecim_set_state";
      if (count < 0) return set_err(PF_ERR_ARG, "%s: count = %ld < 0", what, (long)count);
      VDecim *a;
      int rc = vdecim_enter(what, h, &a);
      if (rc) return rc;
      a->fill = 0;
      if (acc) { if ((rc = band_rows(what, a, a->acc, a->arows(), const_cast<double *>(acc), pitch, rowstride, false))) return rc; }
      else HIPCHK(hipMemset(a->acc, 0, (size_t)a->arows() * a->cstride * sizeof(double)));
      if (state) { if ((rc = band_rows(what, a, a->st, a->srows(), const_cast<double *>(state), pitch, rowstride, false))) return rc; }
      else if (a->npre) HIPCHK(hipMemset(a->st, 0, (size_t)a->srows() * a->cstride * sizeof(double)));
      HIPCHK(hipDeviceSynchronize());
      a->count = count;
      a->rd = a->done();
      return PF_OK;
   }

   int vdecim_info(void *h, int64_t *count, int64_t *pending) const override {
      const VDecim *a = vdecim_of(h);
      if (!a) return PF_ERR_ARG;
      *count = a->count;
      *pending = a->pending();
      return PF_OK;
   }

   int vdecim_destroy(void *h) override {
      const char *what = "pf_engine_vdecim_destroy";
      if (!h) return set_err(PF_ERR_ARG, "%s: null pf_vdecim", what);
      VDecim *a = vdecim_of(h);
      if (!a) return set_err(PF_ERR_ARG, "%s: the pf_vdecim belongs to another engine", what);
      HIPCHK(hipSetDevice(op.device));
      if (s_main) HIPCHK(hipStreamSynchronize(s_main));
      vdecim_free(a);
      vdecims.erase(std::find_if(vdecims.begin(), vdecims.end(), [&](const std::unique_ptr<VDecim> &p) { return p.get() == a; }));
      return PF_OK;
   }
