// pf_engine_observe.inc -- part of `template <typename Real> struct Engine` (pf_engine_class.inc includes it INSIDE the class body, before the kinds;
// not a translation unit): what the region observers share -- the field accumulators (pf_engine_accum.inc), the band accumulators,
// scalar and vector (pf_engine_vband.inc) and the decimating recorders, scalar and vector (pf_engine_vdecim.inc).
// An observer samples up to four components of u^n over a pf_region -- the cell itself, or a difference -- into the next slot of its ring, folds a
// full ring on the device with its kind's kernels, and moves rows of doubles to and from the caller's arrays.  Here: the one list that owns them,
// the lookup by handle and kind, what every call checks first, the component rules, the sample, and the row copies.
//
// The sample.  Component 0 is u^n of the region exactly as pf_engine_get_region(1, ...) gives it at the same moment: the same kernel (k_region_cut)
// cuts it into the ring slot.  1 / 2 / 3 are the central differences along file x / y / z (k_region_diff), 4 / 5 / 6 the LATTICE differences of an FCC
// grid (fcc_flag 1 / 2): the four pair differences over the eight FCC neighbours at +-1 along the axis, in stored coordinates, all requested ones
// by ONE k_region_lat launch per sample; they read along all three axes, so the region keeps one cell clear of all six faces.  The virtual ghost
// shell is materialised when the region WIDENED by one cell along the axes its components read holds a face cell -- the get_region rule applied to
// the cells actually read; a scalar kind (the one component 0) widens nothing.  Nothing a later step reads changes: the device writes are the
// observer's own arrays, that ghost shell and a folded grid's fold row (observer_sample).  The sample is enqueued on the main stream and not waited
// for.  A slab's next step begins on the EDGE stream, and where the ghost shell lives in memory its first kernels (launch_flips) rewrite the shell of
// u^n, which the cuts may still be reading; that stream last waited for the main stream at the end of the step before.  So a sample leaves
// obs_pending set, and step_begin then has the edge stream wait for an event recorded on the main stream (ev_obs): add followed at once by the next
// step reads what add, a read, then the step reads.  No host synchronisation (the ring exists to avoid one), and nothing at all per sample: an event
// wait enqueued here, on the idle edge stream, made the next add's synchronisation of that stream cost 9 us (profiles/observer_ordering.txt).
// All device memory is `mem`'s.
   struct Observer {
      const int kind; // pfeng::OBS_*: a handle is its kind's alone
      pf_region r{};
      int64_t c[3] = {0, 0, 0}, cells = 0, cstride = 0; // cstride: the cell count rounded up to a multiple of 2
      int ncomp = 1, comp[pf::PF_VBAND_MAX_COMP] = {0, 0, 0, 0};
      int depth = 0, fill = 0; // fill: samples in the ring
      bool shell = false;      // the cells read hold a cell of a face of the grid
      int lat = 0;             // bit 0 / 1 / 2: the lattice difference along file x / y / z is a component
      bool fold_row = false;   // ... and the region's last row is Ny - 2: its neighbours lie in the row above (a folded grid's fold row)
      Real *ring = nullptr;    // [ncomp][depth][cells]
      std::vector<void *> owned; // its device memory
      explicit Observer(int k) : kind(k) {}
      virtual ~Observer() {}
   };
   std::vector<std::unique_ptr<Observer>> observers;

   template <typename A> A *observer_of(void *h, int kind) const {
      for (const auto &a : observers) if (a.get() == h && a->kind == kind) return static_cast<A *>(a.get());
      return nullptr;
   }
   template <typename T> int observer_alloc(Observer *a, T **dst, int64_t n, bool zero) {
      const int rc = zero ? dzalloc(dst, n) : dalloc(dst, n);
      if (rc == PF_OK) a->owned.push_back(*dst);
      return rc;
   }
   int observer_release(Observer *a, int rc) {
      for (void *p : a->owned) mem.release(p);
      a->owned.clear();
      return rc;
   }
   template <typename A> void observer_keep(std::unique_ptr<A> &a, void **out) {
      *out = a.get();
      observers.push_back(std::move(a));
   }

   // what add, get, set and read share: the handle is this engine's and of this kind, the engine stands between two runs, its streams have drained
   template <typename A> int observer_mine(const char *what, void *h, int kind, A **a) {
      if (!h) return set_err(PF_ERR_ARG, "%s: null %s", what, pfeng::obs_type[kind]);
      if (!(*a = observer_of<A>(h, kind))) return set_err(PF_ERR_ARG, "%s: the %s belongs to another engine", what, pfeng::obs_type[kind]);
      return PF_OK;
   }
   template <typename A> int observer_stand(const char *what, void *h, int kind, A **a) { // (all but the drain: the absorption maps' add, pf_engine_absorb.inc)
      const int rc = observer_mine(what, h, kind, a);
      if (rc) return rc;
      if (in_step || in_pass()) return set_err(PF_ERR_STATE, "%s inside a split-phase step or pass (u^{n+1} is not complete in memory): valid between runs only", what);
      HIPCHK(hipSetDevice(op.device));
      return PF_OK;
   }
   template <typename A> int observer_enter(const char *what, void *h, int kind, A **a) {
      const int rc = observer_stand(what, h, kind, a);
      return rc ? rc : sync();
   }
   int observer_destroy(const char *what, int kind, void *h) override { // (pending samples are dropped)
      Observer *a;
      const int rc = observer_mine(what, h, kind, &a);
      if (rc) return rc;
      HIPCHK(hipSetDevice(op.device));
      if (s_main) HIPCHK(hipStreamSynchronize(s_main));
      observer_release(a, 0);
      observers.erase(std::find_if(observers.begin(), observers.end(), [&](const std::unique_ptr<Observer> &p) { return p.get() == a; }));
      return PF_OK;
   }
   bool between_runs() const override { return !(in_step || in_pass()); }

   // the region and the components of an observer: a's counts, comp, lat, fold_row and shell, or the refusal.  The scalar kinds: one component {0}.
   int observer_region(const char *what, const pf_region *r, int ncomp, const int32_t *comp, Observer *a) {
      static const char *axis_name[3] = {"x", "y", "z"};
      if (ncomp < 1 || ncomp > pf::PF_VBAND_MAX_COMP) return set_err(PF_ERR_ARG, "%s: ncomp = %d outside 1 .. %d", what, ncomp, pf::PF_VBAND_MAX_COMP);
      if (!comp) return set_err(PF_ERR_ARG, "%s: null comp", what);
      bool diff[3] = {false, false, false};
      for (int k = 0; k < ncomp; k++) {
         if (comp[k] < 0 || comp[k] > 6)
            return set_err(PF_ERR_ARG, "%s: comp[%d] = %d outside 0 (the cell) .. 6 (1 / 2 / 3: the difference along file x / y / z; 4 / 5 / 6: the lattice difference of an FCC grid)", what,
                           k, comp[k]);
         if (comp[k] >= 4 && !fcc)
            return set_err(PF_ERR_ARG, "%s: comp[%d] = %d: a lattice difference (4 / 5 / 6) on fcc_flag == 0 -- its neighbours are the FCC stencil's; 1 / 2 / 3 are the differences of a "
                                       "Cartesian grid", what, k, comp[k]);
         for (int m = 0; m < k; m++) if (comp[m] == comp[k]) return set_err(PF_ERR_ARG, "%s: comp[%d] = comp[%d] = %d: a repeated component", what, m, k, comp[k]);
         if (comp[k] >= 1 && comp[k] <= 3) diff[comp[k] - 1] = true;
         if (comp[k] >= 4) a->lat |= 1 << (comp[k] - 4);
         a->comp[k] = comp[k];
      }
      a->ncomp = ncomp;
      const int64_t N[3] = {fNx, fNy, fNz};
      char msg[256];
      a->cells = pf_cut::region_check(r, N, a->c, msg, sizeof msg);
      if (a->cells < 0) return set_err(PF_ERR_ARG, "%s: %s", what, msg);
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
      a->cstride = round_up(a->cells, 2);
      return PF_OK;
   }

   // The pieces of a region a launch's grid demands (at most 65535 blocks along y and z): blocks of planes, or -- more than 65535 rows in a plane --
   // runs of rows of one plane; both contiguous in a ring slot, `off` cells from its start.  launch(q, grid, tiled, bzl, off) launches one piece.
   template <typename F> int region_pieces(const pf_region &r, const int64_t *c, F launch) {
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
            launch(q, g, tiled, bzl, (i0 * c[1] + j0) * c[2]);
            HIPCHK(hipGetLastError());
         }
      return PF_OK;
   }
   // u^n of a region -> a ring slot of `cells` Reals, dense
   int region_to_slot(const pf_region &r, const int64_t *c, Real *slot) {
      return region_pieces(r, c, [&](const pf::RegionPiece &q, dim3 g, bool tiled, int bzl, int64_t off) {
         if (swz) hipLaunchKernelGGL((pf::k_region_cut<Real, true>), g, dim3(256), 0, s_main, (const Real *)u1, slot + off, q, Ny, P, tiled ? 1 : 0, bzl);
         else hipLaunchKernelGGL((pf::k_region_cut<Real, false>), g, dim3(256), 0, s_main, (const Real *)u1, slot + off, q, Ny, P, 0, bzl);
      });
   }
   // the central difference of u^n along file axis `axis` (0 / 1 / 2) over a region -> a ring slot
   int diff_to_slot(const pf_region &r, const int64_t *c, int axis, Real *slot) {
      const int dx = axis == 0, dy = axis == 1, dz = axis == 2;
      return region_pieces(r, c, [&](const pf::RegionPiece &q, dim3 g, bool tiled, int bzl, int64_t off) {
         if (swz) hipLaunchKernelGGL((pf::k_region_diff<Real, true>), g, dim3(256), 0, s_main, (const Real *)u1, slot + off, q, Ny, P, tiled ? 1 : 0, bzl, dx, dy, dz);
         else hipLaunchKernelGGL((pf::k_region_diff<Real, false>), g, dim3(256), 0, s_main, (const Real *)u1, slot + off, q, Ny, P, 0, bzl, dx, dy, dz);
      });
   }
   // the lattice differences `mask` (bit a: along file axis a) of u^n over a region -> their ring slots, ONE launch per piece for all of them
   int lat_to_slots(const pf_region &r, const int64_t *c, int mask, Real *const *slot) {
      const size_t lds = (size_t)__builtin_popcount((unsigned)mask) * 32 * 33 * sizeof(Real);
      return region_pieces(r, c, [&](const pf::RegionPiece &q, dim3 g, bool tiled, int bzl, int64_t off) {
         Real *o[3];
         for (int k = 0; k < 3; k++) o[k] = slot[k] ? slot[k] + off : nullptr;
         if (swz) hipLaunchKernelGGL((pf::k_region_lat<Real, true>), g, dim3(256), tiled ? lds : 0, s_main, (const Real *)u1, o[0], o[1], o[2], q, Ny, P, tiled ? 1 : 0, bzl, mask);
         else hipLaunchKernelGGL((pf::k_region_lat<Real, false>), g, dim3(256), 0, s_main, (const Real *)u1, o[0], o[1], o[2], q, Ny, P, 0, bzl, mask);
      });
   }

   // the sample of this moment: every component of u^n over the region -> position `fill` of its part of the ring
   int observer_sample(Observer *a) {
      obs_pending = true; // whatever is enqueued below, on an error's way out too: the next split-phase step orders its edge stream behind it (step_begin)
      if ((lean || vg) && a->shell) { // the virtual ghost shell, exactly as get_region(1) writes it out, once for all components
         launch_flips(s_main, grids());
         HIPCHK(hipGetLastError());
      } else if (fold && a->lat && a->fold_row) {
         // A folded grid's row Ny - 1 is the fold's ghost, the copy of row Ny - 2 of the SAME field: it is the other half of the room, not a face of it.
         // The engines whose shell lives in memory write it at the start of the step that reads it (launch_flips), so between two runs u^n still
         // carries the row of two steps ago.  Written here, from the same row the next step copies again: nothing that step reads changes.
         hipLaunchKernelGGL(pf::k_flip_y<Real>, dim3((unsigned)cdiv(Nz, 256), (unsigned)Nx), dim3(256), 0, s_main, grids().cur, Nx, Ny, P, Nz, 4);
         HIPCHK(hipGetLastError());
      }
      int rc;
      Real *lslot[3] = {nullptr, nullptr, nullptr};
      for (int k = 0; k < a->ncomp; k++) {
         Real *slot = a->ring + ((int64_t)k * a->depth + a->fill) * a->cells;
         if (a->comp[k] >= 4) { lslot[a->comp[k] - 4] = slot; continue; }
         if ((rc = a->comp[k] == 0 ? region_to_slot(a->r, a->c, slot) : diff_to_slot(a->r, a->c, a->comp[k] - 1, slot))) return rc;
      }
      if (a->lat && (rc = lat_to_slots(a->r, a->c, a->lat, lslot))) return rc; // all of them in one launch
      return PF_OK;
   }

   // `nrows` device rows, cstride doubles apart, <-> the caller's: dense (pitch, rowstride = 0) or -- a slab's part of a chain's array -- the region's
   // rows `pitch` and the device rows `rowstride` doubles apart
   int observer_rows(const char *what, const Observer *a, double *dev, int64_t nrows, double *host, int64_t pitch, int64_t rowstride, bool out) {
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
   // a get's or a set's pair of arrays: `n0` rows of d0 <-> h0, `n1` rows of d1 <-> h1.  A get (out) skips a null h1; a set zeroes what a null array names
   int observer_rows2(const char *what, const Observer *a, double *d0, int64_t n0, const double *h0, double *d1, int64_t n1, const double *h1, int64_t pitch, int64_t rowstride,
                      bool out) {
      const double *h[2] = {h0, h1};
      double *d[2] = {d0, d1};
      const int64_t n[2] = {n0, n1};
      for (int k = 0; k < 2; k++) {
         int rc;
         if (h[k]) { if ((rc = observer_rows(what, a, d[k], n[k], const_cast<double *>(h[k]), pitch, rowstride, out))) return rc; }
         else if (!out && n[k]) HIPCHK(hipMemset(d[k], 0, (size_t)n[k] * a->cstride * sizeof(double)));
      }
      if (!out) HIPCHK(hipDeviceSynchronize());
      return PF_OK;
   }
