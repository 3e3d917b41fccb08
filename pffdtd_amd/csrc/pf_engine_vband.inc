// pf_engine_vband.inc -- part of `template <typename Real> struct Engine` (pf_engine_class.inc includes it INSIDE the class body, after
// pf_engine_band.inc; not a translation unit): the vector band accumulators (kernels: pf_vband.h).  Per cell of a region up to four components --
// the cell of u^n itself, or its central difference along a file axis -- run through their own pre sections and, per band, through the band's
// sections (state per component); products of two filtered components are summed into the time bin the caller names.  Component 0 is taken
// exactly as a band accumulator's sample (region_to_slot: k_region_cut), a difference by k_region_diff into the component's ring slot; the ghost
// shell is materialised when the region WIDENED by one cell along its difference axes holds a face cell -- the get_region rule applied to the
// cells actually read.  On an FCC grid (fcc_flag 1 / 2) the difference components are the LATTICE differences 4 / 5 / 6 instead: the four pair
// differences over the eight FCC neighbours at +-1 along the axis, in stored coordinates, all requested ones by ONE k_region_lat launch per sample;
// they read along all three axes, so the region keeps one cell clear of all six faces and the widening is by one cell on every axis.  A full
// folded grid's add whose cells read the fold row Ny - 1 first makes that row the copy of row Ny - 2 of u^n (vband_add).  A full ring is folded
// (k_vband_pre, k_vband_fold, in greedy pieces of 8, 4, 2, 1 samples); get, set and destroy fold or drop what is pending.  Nothing a later step
// reads changes.  All device memory is `mem`'s.
   struct VBand {
      pf_region r{};
      int64_t c[3] = {0, 0, 0}, cells = 0, cstride = 0;
      int ncomp = 0, comp[pf::PF_VBAND_MAX_COMP] = {0, 0, 0, 0};
      int npre = 0, nband = 0, nsec = 0, nprod = 0, nbin = 0, depth = 0, fill = 0; // fill: samples in the ring
      bool shell = false;
      int lat = 0; // bit 0 / 1 / 2: the lattice difference along file x / y / z is a component
      bool fold_row = false; // ... and the region's last row is Ny - 2: its neighbours lie in the row above (a folded grid's fold row)
      double *S = nullptr, *st = nullptr, *coef = nullptr, *xpre = nullptr;
      int32_t *bins = nullptr, *prod = nullptr;
      Real *ring = nullptr;
      std::vector<int32_t> hbins; // [depth]: the pending samples' bins
      int nsect() const { return npre + nband * nsec; } // per component
      int64_t srows() const { return (int64_t)ncomp * nsect() * 2; }
      int64_t erows() const { return (int64_t)nprod * nband * nbin; }
   };
   std::vector<std::unique_ptr<VBand>> vbands;

   VBand *vband_of(void *h) const {
      for (const auto &a : vbands) if (a.get() == h) return a.get();
      return nullptr;
   }
   void vband_free(VBand *a) {
      mem.release(a->S); mem.release(a->st); mem.release(a->coef); mem.release(a->xpre); mem.release(a->bins); mem.release(a->prod); mem.release(a->ring);
   }

   int vband_create(const pf_region *r, int ncomp, const int32_t *comp, int npre, const double *pre_sos, int nband, int nsec, const double *band_sos, int nprod,
                    const int32_t *prod, int64_t nbin, int depth, void **out) override {
      const char *what = "pf_engine_vband_create";
      static const char *axis_name[3] = {"x", "y", "z"};
      if (!r || !out) return set_err(PF_ERR_ARG, "%s: null %s", what, !r ? "pf_region" : "out");
      *out = nullptr;
      if (ncomp < 1 || ncomp > pf::PF_VBAND_MAX_COMP) return set_err(PF_ERR_ARG, "%s: ncomp = %d outside 1 .. %d", what, ncomp, pf::PF_VBAND_MAX_COMP);
      if (!comp) return set_err(PF_ERR_ARG, "%s: null comp", what);
      for (int k = 0; k < ncomp; k++) {
         if (comp[k] < 0 || comp[k] > 6)
            return set_err(PF_ERR_ARG, "%s: comp[%d] = %d outside 0 (the cell) .. 6 (1 / 2 / 3: the difference along file x / y / z; 4 / 5 / 6: the lattice difference of an FCC grid)", what,
                           k, comp[k]);
         if (comp[k] >= 4 && !fcc)
            return set_err(PF_ERR_ARG, "%s: comp[%d] = %d: a lattice difference (4 / 5 / 6) on fcc_flag == 0 -- its neighbours are the FCC stencil's; 1 / 2 / 3 are the differences of a "
                                       "Cartesian grid", what, k, comp[k]);
         for (int m = 0; m < k; m++) if (comp[m] == comp[k]) return set_err(PF_ERR_ARG, "%s: comp[%d] = comp[%d] = %d: a repeated component", what, m, k, comp[k]);
      }
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
      if (depth < 0 || depth > pf::PF_VBAND_MAX_DEPTH) return set_err(PF_ERR_ARG, "%s: depth = %d outside 0 (default) .. %d", what, depth, pf::PF_VBAND_MAX_DEPTH);
      if (npre > 0 && !pre_sos) return set_err(PF_ERR_ARG, "%s: null pre_sos with npre = %d", what, npre);
      if (nsec > 0 && !band_sos) return set_err(PF_ERR_ARG, "%s: null band_sos with nsec = %d", what, nsec);
      for (int i = 0; i < ncomp * npre * 5; i++)
         if (!std::isfinite(pre_sos[i])) return set_err(PF_ERR_ARG, "%s: pre_sos[%d][%d][%d] is not finite", what, i / (5 * npre), i / 5 % npre, i % 5);
      for (int i = 0; i < nband * nsec * 5; i++)
         if (!std::isfinite(band_sos[i])) return set_err(PF_ERR_ARG, "%s: band_sos[%d][%d][%d] is not finite", what, i / (5 * nsec), i / 5 % nsec, i % 5);
      const int64_t N[3] = {fNx, fNy, fNz};
      char msg[256];
      std::unique_ptr<VBand> a(new VBand());
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
      a->ncomp = ncomp; a->npre = npre; a->nband = nband; a->nsec = nsec; a->nprod = nprod; a->nbin = (int)nbin;
      for (int k = 0; k < ncomp; k++) a->comp[k] = comp[k];
      a->depth = depth ? depth : pf::PF_VBAND_DEFAULT_DEPTH;
      a->cstride = round_up(a->cells, 2);
      std::vector<double> hcoef;
      try {
         a->hbins.assign((size_t)a->depth, -1);
         hcoef.assign((size_t)std::max(ncomp * npre + nband * nsec, 1) * 5, 0.0);
      } catch (const std::bad_alloc &) { return set_err(PF_ERR_ARG, "%s: no host memory", what); }
      if (npre) memcpy(hcoef.data(), pre_sos, (size_t)ncomp * npre * 5 * sizeof(double));
      if (nsec) memcpy(hcoef.data() + (size_t)ncomp * npre * 5, band_sos, (size_t)nband * nsec * 5 * sizeof(double));
      HIPCHK(hipSetDevice(op.device));
      int rc;
      if ((rc = dzalloc(&a->S, a->erows() * a->cstride)) || (rc = dzalloc(&a->st, std::max<int64_t>(a->srows(), 1) * a->cstride)) ||
          (rc = dalloc(&a->ring, (int64_t)ncomp * a->depth * a->cells)) || (rc = dalloc(&a->coef, (int64_t)hcoef.size())) || (rc = dalloc(&a->bins, (int64_t)a->depth)) ||
          (rc = dalloc(&a->prod, (int64_t)nprod * 3)) || (npre && (rc = dalloc(&a->xpre, (int64_t)ncomp * a->depth * a->cstride)))) {
         vband_free(a.get());
         return rc;
      }
      HIPCHK(hipMemcpy(a->coef, hcoef.data(), hcoef.size() * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(a->prod, prod, (size_t)nprod * 3 * sizeof(int32_t), hipMemcpyHostToDevice));
      HIPCHK(hipDeviceSynchronize()); // (the memsets ran on the null stream; our streams are non-blocking)
      *out = a.get();
      vbands.push_back(std::move(a));
      return PF_OK;
   }

   // what add, get and set share: the handle is this engine's, the engine stands between two runs, its streams have drained
   int vband_enter(const char *what, void *h, VBand **a) {
      if (!h) return set_err(PF_ERR_ARG, "%s: null pf_vbandacc", what);
      if (!(*a = vband_of(h))) return set_err(PF_ERR_ARG, "%s: the pf_vbandacc belongs to another engine", what);
      if (in_step || in_pass()) return set_err(PF_ERR_STATE, "%s inside a split-phase step or pass (u^{n+1} is not complete in memory): valid between runs only", what);
      HIPCHK(hipSetDevice(op.device));
      return sync();
   }

   // the central difference of u^n along file axis `axis` (0 / 1 / 2) over a region -> a ring slot: region_to_slot's pieces, k_region_diff in k_region_cut's place
   int diff_to_slot(const pf_region &r, const int64_t *c, int axis, Real *slot) {
      const bool planes = c[1] <= 65535;
      const int64_t n0 = planes ? std::min<int64_t>(c[0], 65535) : 1, n1 = planes ? c[1] : 65535;
      const int dx = axis == 0, dy = axis == 1, dz = axis == 2;
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
            if (swz) hipLaunchKernelGGL((pf::k_region_diff<Real, true>), g, dim3(256), 0, s_main, (const Real *)u1, out, q, Ny, P, tiled ? 1 : 0, bzl, dx, dy, dz);
            else hipLaunchKernelGGL((pf::k_region_diff<Real, false>), g, dim3(256), 0, s_main, (const Real *)u1, out, q, Ny, P, 0, bzl, dx, dy, dz);
            HIPCHK(hipGetLastError());
         }
      return PF_OK;
   }

   // the lattice differences `mask` (bit a: along file axis a) of u^n over a region -> their ring slots, ONE launch per piece for all of them: diff_to_slot's
   // pieces, k_region_lat in k_region_diff's place
   int lat_to_slots(const pf_region &r, const int64_t *c, int mask, Real *const *slot) {
      const bool planes = c[1] <= 65535;
      const int64_t n0 = planes ? std::min<int64_t>(c[0], 65535) : 1, n1 = planes ? c[1] : 65535;
      const size_t lds = (size_t)__builtin_popcount((unsigned)mask) * 32 * 33 * sizeof(Real);
      for (int64_t i0 = 0; i0 < c[0]; i0 += n0)
         for (int64_t j0 = 0; j0 < c[1]; j0 += n1) {
            const pf::RegionPiece q{r.lo[0] + i0 * r.stride[0], r.lo[1] + j0 * r.stride[1], r.lo[2], r.stride[0], r.stride[1], r.stride[2],
                                    std::min(n0, c[0] - i0), std::min(n1, c[1] - j0), c[2]};
            const bool tiled = swz && q.n0 >= 2 && q.n2 >= 2;
            int bzl = 0;
            while (bzl < 8 && ((int64_t)1 << bzl) < q.n2) bzl++;
            const dim3 g = tiled ? dim3((unsigned)cdiv(q.n2, 32), (unsigned)q.n1, (unsigned)cdiv(q.n0, 32))
                                 : dim3((unsigned)cdiv(q.n2, (int64_t)1 << bzl), (unsigned)cdiv(q.n1, 256 >> bzl), (unsigned)q.n0);
            const int64_t off = (i0 * c[1] + j0) * c[2];
            Real *o[3];
            for (int k = 0; k < 3; k++) o[k] = slot[k] ? slot[k] + off : nullptr;
            if (swz) hipLaunchKernelGGL((pf::k_region_lat<Real, true>), g, dim3(256), tiled ? lds : 0, s_main, (const Real *)u1, o[0], o[1], o[2], q, Ny, P, tiled ? 1 : 0, bzl, mask);
            else hipLaunchKernelGGL((pf::k_region_lat<Real, false>), g, dim3(256), 0, s_main, (const Real *)u1, o[0], o[1], o[2], q, Ny, P, 0, bzl, mask);
            HIPCHK(hipGetLastError());
         }
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
   int vband_fold(VBand *a) {
      if (a->fill == 0) return PF_OK;
      if (a->fill > a->depth) return set_err(PF_ERR_STATE, "internal: %d samples in a vector band accumulator's ring of %d", a->fill, a->depth);
      HIPCHK(hipMemcpyAsync(a->bins, a->hbins.data(), (size_t)a->fill * sizeof(int32_t), hipMemcpyHostToDevice, s_main));
      switch (a->ncomp) {
         case 1: launch_vband_pieces<1>(a); break;
         case 2: launch_vband_pieces<2>(a); break;
         case 3: launch_vband_pieces<3>(a); break;
         case 4: launch_vband_pieces<4>(a); break;
         default: return set_err(PF_ERR_STATE, "internal: %d components in a vector band accumulator", a->ncomp);
      }
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(s_main)); // (hbins is free again)
      a->fill = 0;
      return PF_OK;
   }

   int vband_add(void *h, int64_t bin) override {
      const char *what = "pf_engine_vband_add";
      VBand *a;
      int rc;
      if (h && (a = vband_of(h)) && (bin < -1 || bin >= a->nbin)) return set_err(PF_ERR_ARG, "%s: bin = %ld outside -1 .. %d", what, (long)bin, a->nbin - 1);
      if ((rc = vband_enter(what, h, &a))) return rc;
      if ((lean || vg) && a->shell) { // the virtual ghost shell, once for all components
         launch_flips(s_main, grids());
         HIPCHK(hipGetLastError());
      } else if (fold && a->lat && a->fold_row) {
         // A folded grid's row Ny - 1 is the fold's ghost, the copy of row Ny - 2 of the SAME field: it is the other half of the room, not a face of it.
         // The engines whose shell lives in memory write it at the start of the step that reads it (launch_flips), so between two runs u^n still
         // carries the row of two steps ago.  Written here, from the same row the next step copies again: nothing that step reads changes.
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
      a->hbins[(size_t)a->fill] = (int32_t)bin;
      a->fill++;
      if (a->fill == a->depth) return vband_fold(a);
      return PF_OK;
   }

   // sums [nprod][nband][nbin][cells], state [ncomp][npre + nband*nsec][2][cells] (may be null)
   int vband_get(void *h, double *sums, double *state, int64_t pitch, int64_t rowstride) override {
      const char *what = "pf_engine_vband_get";
      if (!sums) return set_err(PF_ERR_ARG, "%s: null sums array", what);
      VBand *a;
      int rc = vband_enter(what, h, &a);
      if (rc || (rc = vband_fold(a))) return rc;
      if ((rc = band_rows(what, a, a->S, a->erows(), sums, pitch, rowstride, true))) return rc;
      return state ? band_rows(what, a, a->st, a->srows(), state, pitch, rowstride, true) : PF_OK;
   }

   // null: zeros.  Pending samples are dropped.
   int vband_set(void *h, const double *sums, const double *state, int64_t pitch, int64_t rowstride) override {
      const char *what = "pf_engine_vband_set";
      VBand *a;
      int rc = vband_enter(what, h, &a);
      if (rc) return rc;
      a->fill = 0;
      if (sums) { if ((rc = band_rows(what, a, a->S, a->erows(), const_cast<double *>(sums), pitch, rowstride, false))) return rc; }
      else HIPCHK(hipMemset(a->S, 0, (size_t)a->erows() * a->cstride * sizeof(double)));
      if (state) { if ((rc = band_rows(what, a, a->st, a->srows(), const_cast<double *>(state), pitch, rowstride, false))) return rc; }
      else if (a->srows()) HIPCHK(hipMemset(a->st, 0, (size_t)a->srows() * a->cstride * sizeof(double)));
      HIPCHK(hipDeviceSynchronize());
      return PF_OK;
   }

   int vband_destroy(void *h) override {
      const char *what = "pf_engine_vband_destroy";
      if (!h) return set_err(PF_ERR_ARG, "%s: null pf_vbandacc", what);
      VBand *a = vband_of(h);
      if (!a) return set_err(PF_ERR_ARG, "%s: the pf_vbandacc belongs to another engine", what);
      HIPCHK(hipSetDevice(op.device));
      if (s_main) HIPCHK(hipStreamSynchronize(s_main));
      vband_free(a);
      vbands.erase(std::find_if(vbands.begin(), vbands.end(), [&](const std::unique_ptr<VBand> &p) { return p.get() == a; }));
      return PF_OK;
   }
