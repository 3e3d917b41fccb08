// pf_engine_absorb.inc -- part of `template <typename Real> struct Engine` (pf_engine_class.inc includes it INSIDE the class body, after
// pf_engine_observe.inc; not a translation unit): the wall absorption maps (kernels: pf_absorb.h), the energy each step takes out of the room per
// frequency-dependent node, per material and per time bin, with the open boundary's loss and the sources' input beside them.  An observer of a kind
// of its own that reads the WALLS, not a region of the air: the branch currents vh1 of two consecutive samples and u^n, u^{n-1} at the ABC and
// source nodes -- the engine's own sorted lists (d_bna / d_Q, d_in / d_insig), which init re-based to storage indices like the receivers', so
// exchanged-axes storage and a slab's local planes need nothing more.  A sample is one streaming pass that folds as it reads: no ring, nothing
// pending.  It is enqueued on the main stream and not waited for; it reads u0, u1 and vh1, which the next step overwrites, so it leaves obs_pending
// set like observer_sample (step_begin orders a slab's edge stream behind it).
// add(n, bin): the engine stands before step n, the state is (u^{n-1}, u^n).  The first add after create or set only primes (prev <- vh1, the keeps
// <- u^{n-1}); every later one must have n = last + 1 and puts step n - 1's three quantities into `bin`.
// The maps are BROADBAND: the loss is quadratic in the branch currents, so a band's share cannot be filtered out of the sums afterwards -- octave-band
// absorption needs a band-limited source (one run per band) or filters per node in front of the square.
   struct Absorb : Observer {
      int nbin = 0, Nm = 0, row = 0; // row = Nm + 2: a bin's materials, the open boundary, the input
      Real *prev = nullptr, *keep_abc = nullptr, *keep_in = nullptr;
      double *node_sum = nullptr, *bins = nullptr, *E = nullptr, *part = nullptr; // part: the wall's [blocks][Nm], then the ABC's and the sources' [blocks]
      double scale[3] = {0, 0, 0}; // wall, open boundary, input
      int64_t nblk[3] = {0, 0, 0};
      bool primed = false;
      int64_t last = -1, count = 0; // the n of the last add; steps accounted
      Absorb() : Observer(pfeng::OBS_ABSORB) {}
   };

   int absorb_create(const double *E, double wall_scale, double abc_scale, double in_scale, int nbin, void **out) override {
      const char *what = "pf_engine_absorb_create";
      if (!out) return set_err(PF_ERR_ARG, "%s: null out", what);
      *out = nullptr;
      if (!E) return set_err(PF_ERR_ARG, "%s: null E (the materials' loss coefficients, [Nm * %d])", what, PF_MMB);
      if (nbin < 1) return set_err(PF_ERR_ARG, "%s: nbin = %d < 1", what, nbin);
      std::unique_ptr<Absorb> a(new Absorb());
      a->nbin = nbin; a->Nm = sd.Nm; a->row = sd.Nm + 2;
      a->scale[0] = wall_scale; a->scale[1] = abc_scale; a->scale[2] = in_scale;
      a->nblk[0] = cdiv(Nbl, pf::ABS_WG); a->nblk[1] = cdiv(Nba, pf::ABS_WG); a->nblk[2] = cdiv(Ns, pf::ABS_WG);
      HIPCHK(hipSetDevice(op.device));
      int rc;
      if ((rc = observer_alloc(a.get(), &a->prev, round_up(Nbl, 64) * PF_MMB, true)) || (rc = observer_alloc(a.get(), &a->keep_abc, Nba, true)) ||
          (rc = observer_alloc(a.get(), &a->keep_in, Ns, true)) || (rc = observer_alloc(a.get(), &a->node_sum, Nbl, true)) ||
          (rc = observer_alloc(a.get(), &a->bins, (int64_t)nbin * a->row, true)) || (rc = observer_alloc(a.get(), &a->E, (int64_t)std::max<int>(sd.Nm, 1) * PF_MMB, true)) ||
          (rc = observer_alloc(a.get(), &a->part, a->nblk[0] * sd.Nm + a->nblk[1] + a->nblk[2], true)))
         return observer_release(a.get(), rc);
      if (sd.Nm) HIPCHK(hipMemcpy(a->E, E, (size_t)sd.Nm * PF_MMB * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipDeviceSynchronize()); // (the memsets ran on the null stream; our streams are non-blocking)
      observer_keep(a, out);
      return PF_OK;
   }

   int absorb_add(void *h, int64_t n, int64_t bin) override {
      const char *what = "pf_engine_absorb_add";
      Absorb *a;
      const int rc = observer_stand(what, h, pfeng::OBS_ABSORB, &a);
      if (rc) return rc;
      if (bin < 0 || bin >= a->nbin) return set_err(PF_ERR_ARG, "%s: bin = %ld outside 0 .. %d", what, (long)bin, a->nbin - 1);
      if (a->primed && n != a->last + 1)
         return set_err(PF_ERR_STATE, "%s: n = %ld after n = %ld: a step between two samples was not seen (its branch currents are gone); sample before every step, or set and "
                                      "start again", what, (long)n, (long)a->last);
      if (n < (a->primed ? 1 : 0) || n > Nt) return set_err(PF_ERR_ARG, "%s: n = %ld outside %d .. Nt = %ld", what, (long)n, a->primed ? 1 : 0, (long)Nt);
      const int acc = a->primed ? 1 : 0;
      double *pw = a->part, *pa = pw + a->nblk[0] * a->Nm, *pi = pa + a->nblk[1], *dst = a->bins + bin * a->row;
      obs_pending = true; // whatever is enqueued below: the next split-phase step orders its edge stream behind it (step_begin)
      if (Nbl) {
         hipLaunchKernelGGL((pf::k_absorb_wall<Real>), dim3((unsigned)a->nblk[0]), dim3(pf::ABS_WG), 0, s_main, (const Real *)vh1, a->prev, (const Real *)d_ssaf, (const int8_t *)d_mat,
                            (const int8_t *)d_Mb, (const double *)a->E, Nbl, a->Nm, a->scale[0], acc, a->node_sum, pw);
         if (acc) hipLaunchKernelGGL(pf::k_absorb_fold, dim3((unsigned)a->Nm), dim3(64), 0, s_main, (const double *)pw, a->nblk[0], a->Nm, dst);
      }
      if (Nba) {
         hipLaunchKernelGGL((pf::k_absorb_abc<Real>), dim3((unsigned)a->nblk[1]), dim3(pf::ABS_WG), 0, s_main, (const Real *)u0, (const Real *)u1, (const int64_t *)d_bna,
                            (const int8_t *)d_Q, Nba, a->scale[1], acc, a->keep_abc, pa);
         if (acc) hipLaunchKernelGGL(pf::k_absorb_fold, dim3(1), dim3(64), 0, s_main, (const double *)pa, a->nblk[1], 1, dst + a->Nm);
      }
      if (Ns) {
         hipLaunchKernelGGL((pf::k_absorb_in<Real>), dim3((unsigned)a->nblk[2]), dim3(pf::ABS_WG), 0, s_main, (const Real *)u0, (const Real *)u1, (const int64_t *)d_in,
                            (const Real *)d_insig, Ns, Nt, n - 1, a->scale[2], acc, a->keep_in, pi);
         if (acc) hipLaunchKernelGGL(pf::k_absorb_fold, dim3(1), dim3(64), 0, s_main, (const double *)pi, a->nblk[2], 1, dst + a->Nm + 1);
      }
      HIPCHK(hipGetLastError());
      a->primed = true;
      a->last = n;
      a->count += acc;
      return PF_OK;
   }

   // nodes: [Nbl] in the order of sd.bnl_ixyz; mats [nbin][Nm], abc [nbin], in [nbin]; a null array is skipped
   int absorb_get(void *h, double *nodes, double *mats, double *abc, double *in) override {
      const char *what = "pf_engine_absorb_get";
      Absorb *a;
      int rc = observer_enter(what, h, pfeng::OBS_ABSORB, &a);
      if (rc) return rc;
      if (nodes && Nbl) {
         double *tmp = nullptr;
         if ((rc = dalloc(&tmp, Nbl))) return rc;
         hipLaunchKernelGGL(pf::k_absorb_rows, dim3((unsigned)cdiv(Nbl, 256)), dim3(256), 0, s_main, a->node_sum, tmp, (const int64_t *)d_lperm, Nbl, 1);
         const hipError_t e = hipMemcpyAsync(nodes, tmp, (size_t)Nbl * sizeof(double), hipMemcpyDeviceToHost, s_main);
         hipStreamSynchronize(s_main);
         mem.release(tmp);
         HIPCHK(e);
      }
      std::vector<double> b;
      try { b.resize((size_t)a->nbin * a->row); } catch (const std::bad_alloc &) { return set_err(PF_ERR_ARG, "%s: no host memory for the bins", what); }
      HIPCHK(hipMemcpy(b.data(), a->bins, b.size() * sizeof(double), hipMemcpyDeviceToHost));
      for (int k = 0; k < a->nbin; k++) {
         const double *r = b.data() + (size_t)k * a->row;
         if (mats) std::copy(r, r + a->Nm, mats + (size_t)k * a->Nm);
         if (abc) abc[k] = r[a->Nm];
         if (in) in[k] = r[a->Nm + 1];
      }
      return PF_OK;
   }

   // a null array: zeros.  The next add primes.
   int absorb_set(void *h, const double *nodes, const double *mats, const double *abc, const double *in, int64_t count) override {
      const char *what = "pf_engine_absorb_set";
      Absorb *a;
      int rc = observer_enter(what, h, pfeng::OBS_ABSORB, &a);
      if (rc) return rc;
      if (count < 0) return set_err(PF_ERR_ARG, "%s: count = %ld < 0", what, (long)count);
      std::vector<double> b;
      try { b.assign((size_t)a->nbin * a->row, 0.0); } catch (const std::bad_alloc &) { return set_err(PF_ERR_ARG, "%s: no host memory for the bins", what); }
      for (int k = 0; k < a->nbin; k++) {
         double *r = b.data() + (size_t)k * a->row;
         if (mats) std::copy(mats + (size_t)k * a->Nm, mats + (size_t)(k + 1) * a->Nm, r);
         if (abc) r[a->Nm] = abc[k];
         if (in) r[a->Nm + 1] = in[k];
      }
      HIPCHK(hipMemcpy(a->bins, b.data(), b.size() * sizeof(double), hipMemcpyHostToDevice));
      if (Nbl && !nodes) HIPCHK(hipMemset(a->node_sum, 0, (size_t)Nbl * sizeof(double)));
      if (Nbl && nodes) {
         double *tmp = nullptr;
         if ((rc = dalloc(&tmp, Nbl))) return rc;
         const hipError_t e = hipMemcpyAsync(tmp, nodes, (size_t)Nbl * sizeof(double), hipMemcpyHostToDevice, s_main);
         hipLaunchKernelGGL(pf::k_absorb_rows, dim3((unsigned)cdiv(Nbl, 256)), dim3(256), 0, s_main, a->node_sum, tmp, (const int64_t *)d_lperm, Nbl, 0);
         hipStreamSynchronize(s_main);
         mem.release(tmp);
         HIPCHK(e);
      }
      HIPCHK(hipDeviceSynchronize());
      a->primed = false;
      a->last = -1;
      a->count = count;
      return PF_OK;
   }
   int64_t absorb_count(void *h) const override {
      const Absorb *a = observer_of<Absorb>(h, pfeng::OBS_ABSORB);
      return a ? a->count : -1;
   }
