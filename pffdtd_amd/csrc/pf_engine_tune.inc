// pf_engine_tune.inc -- part of `template <typename Real> struct Engine` (pf_engine.hip includes it INSIDE the class body; not a translation unit):
// creation-time measurements: which interior path (Engine::autotune*), where the grids live (search_placement, sample_placement*, place_grids*).
   // ---- which interior path?  Measured, not guessed: at creation the candidates run three times each on the real grids,
   // writing to scratch (the state is not touched): lean fused kernel, barrier-free kernel with virtual ghosts, and --
   // where a box exists -- a temporally blocked pair incl. its shell.  The boundary pass and the I/O are common to all.
   // (7-point only; explicit air_variant requests and PF_DBG_NO_AUTOTUNE skip it.)  Sizes decide in ways no static rule
   // caught: 1024^3 fp32 pair 411 > lean 377 > barrier-free 364 Gvox/s, 896^3 barrier-free 362 > pair 335 > lean 303.
   // 13-point: one in-place-equivalent single step (written to scratch) against half a blocked pair with its shell
   // 13-point single steps: lanes per row segment of k_air_fcc (64 / 32 / 16) measured where they pad the rows differently --
   // the static rule asks for a 25 % narrower padded row before it leaves 64 lanes, which rooms stored along their longest axis
   // (2852 columns = 11.1 segments of 256) never offer, although the half-empty last segment costs them 7 % of the lanes
   int autotune_fcc_lw() {
      if (!fcc || !abck || sg || vbase != 0 || (op.debug & (PF_DBG_NO_AUTOTUNE | PF_DBG_LW32 | PF_DBG_LW16)) || lw_force || !(op.slab_first && op.slab_last)) return PF_OK;
      if (Nx * Ny * Nz < ((int64_t)1 << 22)) return PF_OK;
      constexpr int V = pf::VecOf<Real>::V;
      Real *scr = try_dzalloc<Real>(npad);
      if (!scr) return PF_OK;
      Stopwatch sw;
      HIPCHK(sw.err);
      const Grids g{u0, u1, scr}; // (out of place: the state is not touched)
      auto march3 = [&] { return sw.ms(s_main, 1, 3, [&] { launch_air_march(s_main, g, 1, (int)Nx - 1); }); }; // (compared undivided)
      int best_lw = 0;
      float best = 0;
      int64_t seen = -1;
      for (int lw : {64, 32, 16}) {
         const int64_t w = cdiv(P, (int64_t)lw * V) * lw * V;
         if (w == seen) continue; // same padded width as the wider segment: the wider one wins anyway
         seen = w;
         lw_force = lw;
         const float ms = march3();
         if (best_lw == 0 || ms < 0.98f * best) { best = ms; best_lw = lw; }
      }
      lw_force = best_lw;
      // ... and the tile order: XCD-banded (the rule for large planes) against the plain order.  Rooms stored along their longest
      // axis have long rows (Musikverein: 23 segments of 128 columns) and run 1-3 % faster, and steadier, in the plain order
      // (345.0-345.3 against 335-342 Gvox/s in alternating runs); cubes keep the banded one (2.32 against 2.46 ms at 1024^3).
      order_force = 0;
      const float ms = march3();
      if (ms < 0.985f * best) best = ms; else order_force = -1;
      tune_ms[1] = best / 3;
      HIPCHK(hipStreamSynchronize(s_main));
      mem.release(scr);
      return hipGetLastError() == hipSuccess ? PF_OK : set_err(PF_ERR_HIP, "13-point segment-width measurement: kernel launch failed");
   }
   int autotune_fcc() {
      if (!tb2) return autotune_fcc_lw();
      if (vbase != 0 || (op.debug & PF_DBG_NO_AUTOTUNE)) return PF_OK;
      Stopwatch sw;
      HIPCHK(sw.err);
      HIPCHK(hipDeviceSynchronize());
      auto timed = [&](auto &&fn) { return sw.ms(s_main, 1, 3, fn) / 3; };
      const Grids g1{u0, u1, bufC}, g2{u1, bufC, bufD}; // the two steps of a pair
      for (int i = 0; i < 8 && (double)i * (double)(Nx * Ny * Nz) < 8.0e9; i++) launch_air_march(s_main, g1, 1, (int)Nx - 1); // clocks up
      HIPCHK(hipStreamSynchronize(s_main));
      tune_ms[1] = timed([&] { launch_flips(s_main, g1); launch_air_march(s_main, g1, 1, (int)Nx - 1); });
      tune_ms[2] = 0.5f * timed([&] {
         launch_tb2(s_main, 0, Pass::of_grids(u0, u1, bufC, bufD));
         launch_shell(s_main, g1);
         launch_shell(s_main, g2);
      });
      if (!(tune_ms[2] < pair_margin * tune_ms[1])) { // not worth it: drop the pair path and its two grids
         tb2 = false;
         mem.release(bufC); mem.release(bufD);
      } else {
         HIPCHK(hipMemsetAsync(bufC, 0, npad * sizeof(Real), s_main));
         HIPCHK(hipMemsetAsync(bufD, 0, npad * sizeof(Real), s_main));
      }
      HIPCHK(hipDeviceSynchronize());
      return PF_OK;
   }
   // ---- where do the pair's four grids live?  The pair kernel streams four grids at once, and its speed depends on how
   // their PHYSICAL pages fall onto the memory channels relative to each other: engines of one process, alive side by side
   // and timed in turn, keep their own speed (1024^3: 3.07 / 3.07 / 3.79 ms per launch, round after round;
   // tools/placement_probe.py) -- a property of the allocations, not of the clock state, and nothing a virtual address
   // shows; nor do pairwise copy times between the grids, or any per-grid property: it is the combination that counts (a
   // pool of 8 grids at 1024^3: 2.94 ... 4.25 ms per launch over 64 assignments, a third of them within 2 % of the best).
   // So the engine samples: besides its own grids it allocates up to four more, times the pair kernel (both directions of
   // the four-grid cycle) on two dozen random assignments of pool members to the roles u^{n-1}, u^n, u^{n+1}, u^{n+2},
   // keeps the fastest and frees the rest.  A few hundred ms, once.  With caller-owned state grids (pf_opts.ext_u0 / ext_u1)
   // only the two spares are placed, and only the forward direction is timed (the caller's grids are not written).
   // the search itself: `evals` assignments of pool members to the roles (the first as given in `first`, the others drawn with
   // a fixed-seed generator), timed with the pair kernel; fixed_ab: the state grids stay where they are (u0 / u1), only the
   // two spares are drawn; both: the reverse direction of the four-grid cycle is timed as well (writes every member)
   int search_placement(const std::vector<Real *> &pool, bool fixed_ab, bool both, int evals, const int first[4], int chosen[4]) {
      const bool verbose = getenv("PFFDTD_VERBOSE") && atoi(getenv("PFFDTD_VERBOSE")) > 0;
      Stopwatch sw;
      HIPCHK(sw.err);
      const bool sampled = tb_sample && tb_nsample > 0;
      const float scale = sampled ? (float)(1.0 / tb_sample_frac) : 1.f; // sampled times are reported as whole-launch equivalents
      // ms per launch of the pass A, B -> C, D: two launches, on the sample of the tiles or on all of them
      auto time2 = [&](Real *A, Real *B, Real *C, Real *D, bool sample) {
         const Pass p = Pass::of_grids(A, B, C, D);
         return sw.ms(s_main, 0, 2, [&] { launch_probe(s_main, 0, p, sample); }) / 2;
      };
      auto time_fwd = [&](Real *A, Real *B, Real *C, Real *D) { return time2(A, B, C, D, true) * scale; };
      auto grid = [&](int i, Real *fallback) { return i >= 0 ? pool[i] : fallback; };
      for (int i = 0; i < 4; i++) launch_probe(s_main, 0, Pass::of_grids(grid(first[0], u0), grid(first[1], u1), pool[first[2]], pool[first[3]])); // clocks up
      struct Cand { int r[4]; float ms; };
      std::vector<Cand> cands;
      auto eval = [&](const int r[4]) {
         Real *A = grid(r[0], u0), *B = grid(r[1], u1), *C = pool[r[2]], *D = pool[r[3]];
         float ms = time_fwd(A, B, C, D);
         if (both) ms = 0.5f * (ms + time_fwd(C, D, A, B));
         cands.push_back({{r[0], r[1], r[2], r[3]}, ms});
      };
      uint32_t rng = 0x9e3779b9u;
      auto next = [&](uint32_t m) { rng = rng * 1664525u + 1013904223u; return (rng >> 8) % m; };
      // Round 6: the search STOPS at the first candidate on the known fast level.  For the 7-point kernels that level is known -- the
      // compulsory bytes of a launch at 5.5 TB/s -- and on this chip about every second assignment of a pool of eight sits on it (1024^3:
      // 2.94 ms on all tiles, 3.12-3.15 on the sample, which over-states a launch by ~6 %; the slow levels start at 3.30): a sampled time
      // within 7.5 % of the level ends the draw, and the whole-launch check below confirms it.  48 candidates x 4 launches -> typically 2-4
      // (creation at 1024^3: 244 probe launches / 0.48 s -> ~50 / 0.1 s).  Small grids, fp64 and 13-point kernels sit above the level
      // whatever the pool and search as before.  PFFDTD_PLACE_FULL=1: never stop early.
      float stop_ms = 0.f;
      if (sampled && !fcc && !getenv("PFFDTD_PLACE_FULL") && !getenv("PFFDTD_PLACE_FORCE_GROW") && npad * (int64_t)sizeof(Real) >= ((int64_t)256 << 20))
         stop_ms = 1.075f * (float)((double)tb_clean_cells * 4.0 * sizeof(Real) / 5.5e12 * 1e3);
      auto done = [&]() { return stop_ms > 0.f && !cands.empty() && cands.back().ms <= stop_ms; };
      eval(first);
      const int n = (int)pool.size(), k = fixed_ab ? 2 : 4;
      auto best_of = [&]() { size_t b = 0; for (size_t i = 1; i < cands.size(); i++) if (cands[i].ms < cands[b].ms) b = i; return b; };
      // phase 1: random assignments (a third of the budget); phase 2: from the best one, replace one role's grid at a time by
      // every other pool member (a swap when that member holds another role), keep what is faster, until a full sweep
      // brings nothing or the budget is spent.  Random draws alone reach the fastest level (one tuple in ~16) in three
      // pools of four; the descent gets there from the common second-best levels.
      const int nrand = std::max(evals / 3, 2);
      for (int t = 1; t < nrand && n >= k && (n > k || !fixed_ab) && !done(); t++) {
         int idx[4], r[4] = {-1, -1, -1, -1};
         for (int i = 0; i < k; i++) { // k distinct pool members, in order
            bool dup;
            do { idx[i] = (int)next((uint32_t)n); dup = false; for (int j = 0; j < i; j++) dup |= idx[j] == idx[i]; } while (dup);
            r[4 - k + i] = idx[i];
         }
         eval(r);
      }
      bool stop = done();
      for (bool improved = true; improved && (int)cands.size() < evals && n > k && !stop;) {
         improved = false;
         for (int role = 4 - k; role < 4 && (int)cands.size() < evals && !stop; role++) {
            for (int m = 0; m < n && (int)cands.size() < evals && !stop; m++) {
               const Cand cur = cands[best_of()];
               if (cur.r[role] == m) continue;
               int r[4] = {cur.r[0], cur.r[1], cur.r[2], cur.r[3]};
               for (int q = 4 - k; q < 4; q++) if (r[q] == m) r[q] = cur.r[role]; // m holds another role: swap
               r[role] = m;
               bool seen = false;
               for (auto &c : cands) seen |= c.r[0] == r[0] && c.r[1] == r[1] && c.r[2] == r[2] && c.r[3] == r[3];
               if (seen) continue;
               eval(r);
               if (cands.back().ms < 0.995f * cur.ms) improved = true;
               stop = done();
            }
         }
      }
      size_t best = best_of();
      if (sampled) {
         // The sample ranks the candidates but over-states a launch by 5-10 % (fewer workgroups per launch, less halo sharing
         // in L2): the eight best are timed once more on ALL tiles and the fastest of those is kept; its whole-launch time
         // replaces the sample's (the caller compares it with the known fast level).
         std::vector<size_t> order(cands.size());
         std::iota(order.begin(), order.end(), 0);
         std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return cands[a].ms < cands[b].ms; });
         float best_full = 0;
         std::vector<size_t> check(order.begin(), order.begin() + std::min<size_t>(stop_ms > 0.f ? 3 : 8, order.size()));
         if (std::find(check.begin(), check.end(), (size_t)0) == check.end()) check.push_back(0); // (the as-allocated assignment, for the statistics)
         for (size_t k = 0; k < check.size(); k++) {
            Cand &c = cands[check[k]];
            Real *A = grid(c.r[0], u0), *B = grid(c.r[1], u1), *C = pool[c.r[2]], *D = pool[c.r[3]];
            float ms = time2(A, B, C, D, false);
            if (both) ms = 0.5f * (ms + time2(C, D, A, B, false));
            if (verbose) fprintf(stderr, "pffdtd_hip:   candidate %zu on all tiles: %.3f ms per launch (sample said %.3f)\n", check[k], ms, c.ms);
            c.ms = ms;
            if (k == 0 || ms < best_full) { best_full = ms; best = check[k]; }
         }
      }
      place_ms.clear();
      for (auto &c : cands) place_ms.push_back(c.ms);
      if (verbose) {
         fprintf(stderr, "pffdtd_hip: grid placement, %d candidates of a pool of %d%s:", (int)cands.size(), n, sampled ? " (timed on a sample of the tiles, scaled to a whole launch)" : "");
         for (size_t i = 0; i < cands.size(); i++) fprintf(stderr, " %.3f%s", cands[i].ms, i == best ? "*" : "");
         fprintf(stderr, " ms per launch\n");
      }
      for (int i = 0; i < 4; i++) chosen[i] = cands[best].r[i];
      return hipGetLastError() == hipSuccess ? PF_OK : set_err(PF_ERR_HIP, "placement search: kernel launch failed");
   }
   static constexpr int place_evals = 48; // the budget of one search_placement
   // the single-step paths stream two grids (u^n read, u^{n-1} read and overwritten): the same question with a smaller answer
   // (Musikverein, 13-point, 1.3e9 cells: 4.36-4.61 ms per step over the pairs of a pool of six; small grids: 1-3 %);
   // every unordered pair of the pool is timed on a whole step (both role assignments, the grids swap roles every step)
   int search_pair(const std::vector<Real *> &pool, int &bi, int &bj) {
      const bool verbose = getenv("PFFDTD_VERBOSE") && atoi(getenv("PFFDTD_VERBOSE")) > 0;
      Stopwatch sw;
      HIPCHK(sw.err);
      const Restore<int> untimed(op.timing, 0);
      auto one_step = [&](Real *a, Real *b) { // u^{n-1} in a, u^n in b, in place; all-zero state: every kernel writes zeros
         const Grids g{a, b, a};
         const Bnd bn = bnd(0, 0);
         launch_pre(s_main, g);
         launch_air(s_main, g, 1, (int)Nx - 1);
         launch_abc(s_main, g, {0, Nba});
         launch_rigid(s_main, g, bn, {0, Nb});
         launch_fd(s_main, g, bn, {0, Nbl});
      };
      auto time_pair = [&](Real *a, Real *b) { return sw.ms(s_main, 0, 1, [&] { one_step(a, b); one_step(b, a); one_step(a, b); one_step(b, a); }) / 4; };
      for (int i = 0; i < 6; i++) one_step(pool[0], pool[1]); // clocks up
      const int n = (int)pool.size();
      bi = 0; bj = 1;
      float best = 0, worst = 0, first = 0;
      place_ms.clear();
      for (int i = 0; i < n; i++)
         for (int j = i + 1; j < n; j++) {
            const float ms = time_pair(pool[i], pool[j]);
            place_ms.push_back(ms);
            if (i == 0 && j == 1) first = best = worst = ms;
            if (ms < best) { best = ms; bi = i; bj = j; }
            worst = std::max(worst, ms);
         }
      if (verbose) fprintf(stderr, "pffdtd_hip: grid placement (single steps), %d pairs of a pool of %d: as allocated %.4f, chosen %.4f, slowest %.4f ms per step\n",
                           (int)place_ms.size(), n, first, best, worst);
      for (int i = 0; i < n; i++) HIPCHK(hipMemsetAsync(pool[i], 0, npad * sizeof(Real), s_main)); // (zeros from zeros; be explicit)
      HIPCHK(hipStreamSynchronize(s_main));
      return hipGetLastError() == hipSuccess ? PF_OK : set_err(PF_ERR_HIP, "placement search: kernel launch failed");
   }
   // Candidate grids beyond the engine's own: at most `want`, never more than fit the free memory (less 3 % of the device), and
   // never so many that the engine's grids plus the pool exceed 85 % of the device (1536^3 fp64: four 29 GB grids + four
   // candidates = 232 GB = 81 %; round 3 capped at 60 %, which left that engine one candidate and cost it 4 %: 217.7 vs 226 Gvox/s).
   // The candidates live for the search only.
   int pool_extra(int want, int own) const {
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return want; }
      const double gb = (double)npad * sizeof(Real);
      const int cap = (int)std::floor((0.85 * (double)total_b - own * gb) / gb);
      const int fit = (int)std::floor(((double)free_b - 0.03 * (double)total_b) / gb);
      return std::max(0, std::min(want, std::min(cap, fit)));
   }
   bool place_single_ok() const { return !(op.debug & PF_DBG_NO_AUTOTUNE) && !op.energy && vbase == 0 && npad * (int64_t)sizeof(Real) >= ((int64_t)64 << 20); }
   // up to n more zero-filled candidate grids at the pool's end; returns how many there was room for
   int add_candidates(std::vector<Real *> &pool, int n) {
      int got = 0;
      for (; got < n; got++) {
         Real *p = try_dzalloc<Real>(npad);
         if (!p) break; // no room for another candidate
         pool.push_back(p);
      }
      return got;
   }
   int sample_placement_single() {
      if (!own_grids || !place_single_ok()) return PF_OK;
      const int extra = pool_extra(4, 2);
      if (extra == 0) return PF_OK;
      std::vector<Real *> pool = {u0, u1};
      add_candidates(pool, extra);
      int bi, bj;
      int rc = search_pair(pool, bi, bj);
      if (rc) return rc;
      u0 = pool[bi]; u1 = pool[bj];
      mem.release_rest(pool, {u0, u1});
      return PF_OK;
   }
   int sample_placement() {
      if (!tb2 || tb2_slab || !bufC || !bufD || (op.debug & PF_DBG_NO_AUTOTUNE) || vbase == 41) return PF_OK;
      const int extra = pool_extra(tb3 ? 3 : 4, tb3 ? 5 : 4);
      if (extra == 0 && !own_grids) return PF_OK;
      std::vector<Real *> pool;
      if (own_grids) { pool.push_back(u0); pool.push_back(u1); }
      if (tb3) { // (roles 2, 3 = the grids k_tb3 writes; the fifth grid is one more candidate)
         if (!bufE) return PF_OK;
         pool.push_back(bufD); pool.push_back(bufE); pool.push_back(bufC);
      } else { pool.push_back(bufC); pool.push_back(bufD); }
      add_candidates(pool, extra);
      const int first_own[4] = {0, 1, 2, 3}, first_ext[4] = {-1, -1, 0, 1};
      int w[4];
      int rc = search_placement(pool, !own_grids, own_grids, place_evals, own_grids ? first_own : first_ext, w);
      if (rc) return rc;
      // Some pools hold no fast assignment at all (seen once in ~15 boxes: best 3.37 ms of 47 candidates where 2.95 is the
      // rule; round 5, k_tb3: 3.40 of 42 on a box where the next process found 2.99).  For the 7-point kernels the fast level is
      // known -- the compulsory bytes of a launch, 4 grids x cells, at 5.5 TB/s (pairs and triples alike: 16 B per cell and launch)
      // -- so a search that ends well above it gets four more grids to choose from, three times at most.
      const float as_allocated = place_ms.empty() ? 0.f : place_ms[0];
      for (int round = 0; round < 3 && !fcc && own_grids; round++) {
         const float best = *std::min_element(place_ms.begin(), place_ms.end());
         const float target = (float)((double)tb_clean_cells * 4.0 * sizeof(Real) / 5.5e12 * 1e3);
         // (grids below 256 MiB are not bandwidth-bound: their launches sit above that level whatever the pool; the variable: tests walk
         // the growth path on any box and any size)
         const bool big = npad * (int64_t)sizeof(Real) >= ((int64_t)256 << 20);
         if ((!big || best <= 1.05f * target) && !getenv("PFFDTD_PLACE_FORCE_GROW")) break;
         if (!add_candidates(pool, pool_extra(4, (int)pool.size()))) break;
         const int cur[4] = {w[0], w[1], w[2], w[3]};
         const std::vector<float> before = place_ms;
         if ((rc = search_placement(pool, false, true, place_evals, cur, w))) return rc;
         place_ms.insert(place_ms.begin(), as_allocated); // (the statistics keep the very first candidate in front ...
         place_ms.insert(place_ms.end(), before.begin() + (before.empty() ? 0 : 1), before.end()); // ... and every candidate of the earlier rounds)
      }
      std::vector<Real *> keep;
      if (own_grids) { u0 = pool[w[0]]; u1 = pool[w[1]]; keep.push_back(u0); keep.push_back(u1); }
      if (tb3) { // the four streams of k_tb3 are u0, u1 -> bufD, bufE; bufC (u^{n+1} of the shell and of a few tiles) is any other member
         bufD = pool[w[2]]; bufE = pool[w[3]];
         bufC = nullptr;
         // The fifth grid holds little (the shell's u^{n+1}) -- except at the END of a run whose length is no multiple of three: the
         // closing pair writes u^{n+1} into it with all tiles, and the next run's first triple reads it (Engine::tb3_pick): four
         // stream combinations off the measured cycle, S1 -> (C, D), (C, D) -> S1, S2 -> (C, A), (C, A) -> S2.  A host that
         // steps in regions of 20 (bench.py as the driver runs it) meets them every region: the candidate that is fastest on
         // their sum becomes the fifth grid.
         Stopwatch sw;
         HIPCHK(sw.err);
         auto t4 = [&](Real *A, Real *B, Real *C, Real *D) { return sw.ms(s_main, 0, 1, [&] { launch_probe(s_main, 0, Pass::of_grids(A, B, C, D), true); }); };
         float best = 0;
         const bool verbose = getenv("PFFDTD_VERBOSE") && atoi(getenv("PFFDTD_VERBOSE")) > 0;
         for (Real *g : pool) {
            if (g == u0 || g == u1 || g == bufD || g == bufE) continue;
            const float ms = t4(u0, u1, g, bufD) + t4(g, bufD, u0, u1) + t4(bufD, bufE, g, u0) + t4(g, u0, bufD, bufE);
            if (verbose) fprintf(stderr, "pffdtd_hip:   fifth grid candidate: %.3f ms over the four off-cycle launches\n", ms);
            if (!bufC || ms < best) { best = ms; bufC = g; }
         }
         if (!bufC) return set_err(PF_ERR_STATE, "placement search: no fifth grid left"); // (the pool holds the engine's five)
         keep.push_back(bufC); keep.push_back(bufD); keep.push_back(bufE);
      } else {
         bufC = pool[w[2]]; bufD = pool[w[3]];
         keep.push_back(bufC); keep.push_back(bufD);
      }
      mem.release_rest(pool, keep);
      for (Real *g : keep) HIPCHK(hipMemsetAsync(g, 0, npad * sizeof(Real), s_main)); // (the pair kernel wrote zeros computed from zeros; be explicit)
      HIPCHK(hipStreamSynchronize(s_main));
      return PF_OK;
   }
   // the search over a caller's pool, from the members as offered; its launches wrote every member: all zeros again afterwards
   int search_offered(const std::vector<Real *> &pool, int w[4]) {
      const int first[4] = {0, 1, 2, 3};
      const Restore<bool> probe(tb2_probe, true);
      int rc = search_placement(pool, false, true, place_evals, first, w);
      if (rc) return rc;
      for (Real *g : pool) HIPCHK(hipMemsetAsync(g, 0, npad * sizeof(Real), s_main));
      HIPCHK(hipStreamSynchronize(s_main));
      return PF_OK;
   }
   // Slab engines (caller-owned grids): the caller offers a pool of n >= 4 zero-filled grids before the first step; the
   // engine adopts the fastest assignment of four of them -- idx[0], idx[1]: the state grids (they replace ext_u0 / ext_u1),
   // idx[2], idx[3]: the spares of pf_engine_set_spares, or idx = 0, 1, -1, -1 when this engine steps singly.
   int place_grids(void *const *grids, int n, int32_t *idx) override { return place_grids_impl(grids, n, idx, false); }
   int place_grids5(void *const *grids, int n, int32_t *idx) override { return place_grids_impl(grids, n, idx, true); }
   // five: idx has five entries and the engine may step in TRIPLES across three split-phase steps (idx[2], idx[3] = the grids k_tb3
   // writes, idx[4] = the u^{n+1} grid; idx[4] = -1: pairs or single steps as pf_engine_place_grids reports them)
   int place_grids_impl(void *const *grids, int n, int32_t *idx, bool five) {
      if (in_step || in_pass() || steps_done > 0) return set_err(PF_ERR_STATE, "pf_engine_place_grids after the first step");
      if (state_touched) return set_err(PF_ERR_STATE, "pf_engine_place_grids after pf_engine_set_grid: the placement search runs step kernels on the offered grids and zeroes them");
      if (own_grids) return set_err(PF_ERR_STATE, "pf_engine_place_grids: this engine allocated its own grids");
      if (!grids || !idx || n < 2) return set_err(PF_ERR_ARG, "pf_engine_place_grids: need a pool of at least two grids");
      for (int i = 0; i < n; i++) {
         if (!grids[i]) return set_err(PF_ERR_ARG, "pf_engine_place_grids: null grid");
         for (int j = 0; j < i; j++) if (grids[i] == grids[j]) return set_err(PF_ERR_ARG, "pf_engine_place_grids: grid offered twice");
      }
      HIPCHK(hipSetDevice(op.device));
      const std::vector<Real *> pool((Real *const *)grids, (Real *const *)grids + n);
      u0 = pool[0]; u1 = pool[1];
      idx[0] = 0; idx[1] = 1; idx[2] = idx[3] = -1;
      if (five) idx[4] = -1;
      if (five && n >= 5 && tb3_geom && tb2_geom && !(op.slab_first && op.slab_last)) {
         // triples: the wall regions must fit the triples' box (init_walls re-orders the lossy arrays: before the first step only)
         tb2_slab = true;
         if (!(op.debug & PF_DBG_NO_WALL_REGIONS)) { int rcw = init_walls(true); if (rcw) return rcw; }
         if (wl_on) {
            int w[4] = {0, 1, 2, 3};
            if (n > 5 && !(op.debug & PF_DBG_NO_AUTOTUNE)) { int rc = search_offered(pool, w); if (rc) return rc; }
            int c = -1;
            for (int i = 0; i < n && c < 0; i++) if (i != w[0] && i != w[1] && i != w[2] && i != w[3]) c = i;
            u0 = pool[w[0]]; u1 = pool[w[1]]; bufD = pool[w[2]]; bufE = pool[w[3]]; bufC = pool[c];
            for (int i = 0; i < 4; i++) idx[i] = w[i];
            idx[4] = c;
            tb3_slab = true;
            tb3_remember_home();
            return PF_OK;
         }
         tb2_slab = false; // (the regions do not fit the triples' box: pairs)
      }
      if (steps_done == 0) { int rcg = pairs_geometry(); if (rcg) return rcg; }
      if (n < 4 || !tb2_geom || (op.slab_first && op.slab_last)) { // keeps stepping singly: on the fastest pair of the pool
         if (n > 2 && place_single_ok()) {
            int bi, bj;
            int rc = search_pair(pool, bi, bj);
            if (rc) return rc;
            u0 = pool[bi]; u1 = pool[bj];
            idx[0] = bi; idx[1] = bj;
         }
         return PF_OK;
      }
      int w[4] = {0, 1, 2, 3};
      if (n > 4 && !(op.debug & PF_DBG_NO_AUTOTUNE)) { int rc = search_offered(pool, w); if (rc) return rc; }
      u0 = pool[w[0]]; u1 = pool[w[1]]; bufC = pool[w[2]]; bufD = pool[w[3]];
      for (int i = 0; i < 4; i++) idx[i] = w[i];
      tb2_slab = true;
      if (!wl_on && !(op.debug & PF_DBG_NO_WALL_REGIONS)) { int rcw = init_walls(true); if (rcw) return rcw; }
      return PF_OK;
   }
   int autotune() {
      if (fcc) return autotune_fcc();
      if (vbase != 0 || op.energy || (op.debug & PF_DBG_NO_AUTOTUNE) || !use_dpp || !(lean || vg)) return PF_OK;
      if (Nx * Ny * Nz < ((int64_t)1 << 22)) return PF_OK; // tiny grids: launch-bound either way
      Real *own = nullptr; // the scratch grid where there is no bufC to write to
      Real *const scr = bufC ? bufC : (own = try_dzalloc<Real>(npad));
      if (!scr) return PF_OK; // no room to measure: the static rules stand
      Stopwatch sw;
      HIPCHK(sw.err);
      HIPCHK(hipDeviceSynchronize());
      auto timed = [&](auto &&fn) { return sw.ms(s_main, 1, 3, fn) / 3; };
      const Grids gs{u0, u1, scr}; // a single step into scratch: the state is not touched
      {
         const Restore<bool> lean0(lean, true), vg0(vg, false); // (the launchers read them: back as they were after the two candidates)
         // the device has been idle while the host built the lists: ramp its clocks first (~20 ms of work), or the first
         // candidate is measured -- and every launch here profiled -- at idle clocks (seen: +56 % per launch)
         for (int i = 0; i < 8 && (double)i * (double)(Nx * Ny * Nz) < 8.0e9; i++) launch_air_lean(s_main, gs, 1, (int)Nx - 1);
         HIPCHK(hipStreamSynchronize(s_main));
         tune_ms[0] = timed([&] { launch_air_lean(s_main, gs, 1, (int)Nx - 1); });
         lean = false; vg = true;
         { // the barrier-free kernel, with 64 / 32 / 16 lanes per row segment where those pad the rows differently
            constexpr int V = pf::VecOf<Real>::V;
            int best_lw = 0;
            int64_t seen[3] = {0, 0, 0};
            int k = 0;
            for (int lw : {64, 32, 16}) {
               const int64_t w = cdiv(P, (int64_t)lw * V) * lw * V;
               if (k > 0 && w == seen[k - 1]) continue; // same padded width as the wider segment: the wider one wins anyway
               seen[k++] = w;
               lw_force = lw;
               const float t = timed([&] { launch_air_march(s_main, gs, 1, (int)Nx - 1); });
               if (best_lw == 0 || t < 0.98f * tune_ms[1]) { tune_ms[1] = t; best_lw = lw; }
            }
            lw_force = best_lw;
         }
      }
      if (hipGetLastError() == hipSuccess) { // (a failed launch: the static rules stand)
         if (tune_ms[1] < 0.97f * tune_ms[0]) { lean = false; vg = true; }
         else if (tune_ms[0] < 0.97f * tune_ms[1]) { lean = true; vg = false; }
      }
      // a blocked pass from the state, its node values in the three buffers and the branch state into its other copy, as the wall regions of a slab step
      const Pass bp = pass_from_state(bufC, bufD, bufE, ub[1], ub[2], state_other());
      const Grids g1 = bp.grids(0), g2 = bp.grids(1);
      const Bnd bn = bnd(0, 0);                         // (fields, node values and branch state are all zeros at creation and stay so: every boundary launch in place)
      if (tb3) {
         // three steps per pass, the boundary pass included: the single steps get theirs added (fields and branch state are all zeros
         // at creation and stay so)
         const float tb = timed([&] { launch_rigid(s_main, gs, bn, {0, Nb}); });
         tune_ms[0] += tb; tune_ms[1] += tb;
         tune_ms[2] = (1.f / 3.f) * timed([&] {
            launch_dirty_tiles(s_main, g1); launch_rigid(s_main, g1, bn.with(wl_rest), {0, wl_nrest});
            launch_walls_x(s_main, s_main, bp, 0, 2, 0xf);
            launch_tb3(s_main, 0, bp);
            launch_dirty_tiles(s_main, g2); launch_rigid(s_main, g2, bn.with(wl_rest), {0, wl_nrest});
            const Grids g3 = bp.grids(2);
            launch_shell(s_main, g3); launch_rigid(s_main, g3, bn, {0, Nb});
         });
      } else if (tb2 && wl_on) {
         // wall regions: the pair then includes the boundary pass, so the single steps get theirs added (fields and branch state
         // are all zeros at creation and stay so)
         const float tb = timed([&] { launch_rigid(s_main, gs, bn, {0, Nb}); });
         tune_ms[0] += tb; tune_ms[1] += tb;
         tune_ms[2] = 0.5f * timed([&] {
            launch_tb2(s_main, 0, bp);
            launch_dirty_tiles(s_main, g1); launch_rigid(s_main, g1, bn.with(wl_rest), {0, wl_nrest});
            launch_walls_x(s_main, s_main, bp, 0, 2, 0xf);
            launch_dirty_tiles(s_main, g2); launch_rigid(s_main, g2, bn.with(wl_rest), {0, wl_nrest});
         });
      } else if (tb2) {
         tune_ms[2] = 0.5f * timed([&] {
            launch_tb2(s_main, 0, bp);
            launch_shell(s_main, g1);
            launch_shell(s_main, g2);
         });
      }
      if (tb2) {
         if (!(tune_ms[2] < pair_margin * std::min(tune_ms[0], tune_ms[1]))) { // not worth it: drop the blocked path and its extra grids
            drop_blocking();
         } else {
            HIPCHK(hipMemsetAsync(bufC, 0, npad * sizeof(Real), s_main));
            HIPCHK(hipMemsetAsync(bufD, 0, npad * sizeof(Real), s_main));
            if (bufE) HIPCHK(hipMemsetAsync(bufE, 0, npad * sizeof(Real), s_main));
         }
      }
      HIPCHK(hipDeviceSynchronize());
      mem.release(own);
      return PF_OK;
   }
