// pf_engine_blocked_steps.inc -- part of `template <typename Real> struct Engine` (pf_engine.hip includes it INSIDE the class body; not a translation unit):
// single-domain pairs with wall regions and triples (Engine::step_pair_walls, step_triple), the five-grid role cycle, pf_engine_set_spares.
   // steps n and n+1 with the shell in pairs as well.  Order: box (both steps), then the first step of what no wall region
   // owns -- the box's dirty tiles and the boundary nodes inside it --, source / receivers of step n, the wall regions (both
   // steps; they read u^{n-1}, u^n and the old branch state only), then the second step of the dirty tiles and their nodes.
   int step_pair_walls(int64_t n) {
      hipStream_t s = s_main;
      Real *A = u0, *B = u1, *C = bufC, *D = bufD;
      // An engine that steps in triples (five grids) ends a run whose length is no multiple of three with a pair: it writes u^{n+1}, u^{n+2} into
      // the two grids a TRIPLE would have written (tb3_pick: the placed cycle's targets), not into the fifth grid -- the four streams of the
      // pair's box kernel are then the assignment the placement search measured (round 5 wrote the fifth grid: an off-cycle launch, 3.0-3.2 ms
      // where the cycle's takes 2.95, and another one for the first triple of the next run), and the state lands where a triple leaves it.
      const bool on_cycle = tb3 && bufE && bufE != A && bufE != B && bufD != A && bufD != B;
      if (on_cycle) { C = bufD; D = bufE; }
      // node values: X2 = u^{n-1}, X1 = u^n are only read; u^{n+1} -> T1, u^{n+2} -> T2, two buffers nobody reads during the pair (round 6: five
      // node-value buffers, so that a region's or a brick's halo node may be evaluated while its owner already stores)
      Real *X2 = ub[2], *X1 = ub[1], *T1 = ub[0], *T2 = ubx[0];
      auto get_ev = [&]() { std::pair<hipEvent_t, hipEvent_t> e{}; if (!ev_pool.empty()) { e = ev_pool.back(); ev_pool.pop_back(); } else { hipEventCreate(&e.first); hipEventCreate(&e.second); } return e; };
      std::pair<hipEvent_t, hipEvent_t> ev{}, ev2{}, evt{}, eva{};
      // "air" of a pair with wall regions (pf_timing.air_ms_total, the CLI's "Air update" line): the alike blocks' launches and the
      // box kernel on the main stream -- the regions' boundary nodes are inside those launches and cannot be told apart
      if (op.timing) { ev = get_ev(); ev2 = get_ev(); evt = get_ev(); eva = get_ev(); hipEventRecord(ev.first, s); hipEventRecord(eva.first, s); }
      // The wall regions read u^{n-1}, u^n and the old branch state only and write cells the box kernel does not: any order will do.
      // The generic blocks (edges, corners: a few hundred waves, each a long chain of dependent steps) go to the second stream
      // and run beside the alike blocks' launches, which are issue-bound; beside the bandwidth-bound box kernel they crawl
      // (measured: 0.47 -> 3.6 ms), so that one comes after.  debug 0x4000000: everything on the main stream.
      const bool beside = !(op.debug & 0x4000000);
      hipStream_t sw = beside ? s_edge : s_main;
      if (beside) { HIPCHK(hipEventRecord(ev_pre, s_main)); HIPCHK(hipStreamWaitEvent(s_edge, ev_pre, 0)); }
      u0_src = A; u1 = B; u0 = C;
      tb3_src_n = n;
      launch_dirty_tiles(sw);
      bnd_sel = wl_rest; bs_vout = vh1b; bs_gout = gh1b;
      ub[0] = T1; ub[2] = X2;
      launch_rigid(sw, {0, wl_nrest});
      launch_bricks(sw, A, B, C, D, nullptr, X2, X1, T1, T2, nullptr, 2); // the frame: both steps, beside the alike blocks
      launch_walls_x(s, sw, A, B, C, D, nullptr, X2, X1, T1, T2, nullptr, 2, 0xf); // (every wall launch beside the box kernel instead of before it: 492 vs 511-516 Gvox/s)
      if (op.timing) hipEventRecord(evt.first, s);
      launch_tb2(s, A, B, C, D);
      if (op.timing) { hipEventRecord(evt.second, s); tb2_ev.push_back(evt); hipEventRecord(eva.second, s); air_ev.push_back(eva); }
      if (beside) { HIPCHK(hipEventRecord(ev_edge, s_edge)); HIPCHK(hipStreamWaitEvent(s_main, ev_edge, 0)); }
      launch_io(s, n, true, src_range()); // (receivers read u^n; the source goes into u^{n+1}, which only the second step below reads -- or went in inside k_tb3<..., SRC>)
      if (ring_fill == 0) ring_n0 = n;
      ring_fill++; steps_done++;
      if (op.timing) { hipEventRecord(ev.second, s); step_ev.push_back(ev); hipEventRecord(ev2.first, s); }
      std::swap(vh1, vh1b); std::swap(gh1, gh1b); // the state after the pair (the nodes inside the box: after its first step)
      u0_src = B; u1 = C; u0 = D;
      launch_dirty_tiles(s);
      bs_vout = bs_gout = nullptr;
      ub[0] = T2; ub[2] = X1; // second step of the box's nodes: u2b = u^n of the node, its u^{n+2} where the regions put theirs
      launch_rigid(s, {0, wl_nrest});
      ub[0] = X2; ub[1] = T2; ub[2] = T1; ubx[0] = X1; // (newest in ub[1], the one before in ub[2], ub[0] free: the single steps' convention)
      bnd_sel = nullptr;
      launch_io(s, n + 1, true, src_range());
      ring_fill++; steps_done++;
      if (on_cycle) { u0_src = nullptr; u0 = C; u1 = D; bufD = A; bufE = B; } // (bufC stays the triples' u^{n+1} grid)
      else { u0_src = nullptr; u0 = C; u1 = D; bufC = A; bufD = B; }
      if (tb3) tb3_pick();
      if (op.timing) { hipEventRecord(ev2.second, s); step_ev.push_back(ev2); }
      HIPCHK(hipGetLastError());
      if (ring_fill == ring_depth) return flush();
      return PF_OK;
   }
   // tb3: which grids does the next blocked step write?  Where the five grids lie relative to each other decides the speed of k_tb3
   // (DESIGN.md, grid placement): the assignment measured at creation -- state home[0], home[1] -> home[2], home[3] and back, home[4]
   // the u^{n+1} grid -- is kept wherever the state allows; after a pair or an odd number of single steps (the end of a run) the
   // next triple is one step off that cycle and returns to it.
   void tb3_remember_home() { home[0] = u0; home[1] = u1; home[2] = bufD; home[3] = bufE; home[4] = bufC; }
   void tb3_pick() {
      if (!home[0]) return;
      if (u0 == home[0] && u1 == home[1]) { bufD = home[2]; bufE = home[3]; bufC = home[4]; return; }
      if (u0 == home[2] && u1 == home[3]) { bufD = home[0]; bufE = home[1]; bufC = home[4]; return; }
      Real *fr[3];
      int nf = 0;
      for (Real *g : home) if (g != u0 && g != u1 && nf < 3) fr[nf++] = g;
      if (nf != 3) return; // (cannot happen: the state is two of the five)
      auto is_free = [&](Real *g) { return g == fr[0] || g == fr[1] || g == fr[2]; };
      if (is_free(home[0]) && is_free(home[1])) { bufD = home[0]; bufE = home[1]; }
      else if (is_free(home[2]) && is_free(home[3])) { bufD = home[2]; bufE = home[3]; }
      else { bufD = fr[0]; bufE = fr[1]; }
      for (Real *g : fr) if (g != bufD && g != bufE) bufC = g;
   }
   // steps n, n+1 and n+2 in one go (tb3): the box by k_tb3 (u^{n+1} stays on the chip), the shell's first two steps as wall regions
   // (k_wall2, exactly as in step_pair_walls), its third as a single step out of memory (the lean kernel on the x slabs and row
   // strips, k_air_zstrip on the column strips, k_boundary over every node); the tiles that step singly (sources, receivers,
   // geometry inside the box) and the box's own boundary nodes take three single steps, the second of which reads the u^{n+1}
   // their flagged neighbours left in bufC.  State (u0, u1) -> (bufD, bufE); the old state grids become the next triple's targets.
   int step_triple(int64_t n) {
      if (n < 0 || n + 2 >= Nt) return set_err(PF_ERR_ARG, "step triple %ld outside [0,Nt=%ld)", (long)n, (long)Nt);
      hipStream_t s = s_main;
      Real *A = u0, *B = u1, *C = bufC, *D = bufD, *E = bufE;
      // node values: X2 = u^{n-1}, X1 = u^n are only read during the triple; u^{n+1} -> T1, u^{n+2} -> T2, u^{n+3} -> T3 (five buffers)
      Real *X2 = ub[2], *X1 = ub[1], *T1 = ub[0], *T2 = ubx[0], *T3 = ubx[1];
      auto get_ev = [&]() { std::pair<hipEvent_t, hipEvent_t> e{}; if (!ev_pool.empty()) { e = ev_pool.back(); ev_pool.pop_back(); } else { hipEventCreate(&e.first); hipEventCreate(&e.second); } return e; };
      std::pair<hipEvent_t, hipEvent_t> ev{}, evt{}, eva{};
      if (op.timing) { ev = get_ev(); evt = get_ev(); eva = get_ev(); hipEventRecord(ev.first, s); hipEventRecord(eva.first, s); }
      const bool beside = !(op.debug & 0x4000000);
      hipStream_t sw = beside ? s_edge : s_main; // the bricks (or the generic wall blocks) and the first step of the single-step tiles: beside the alike blocks
      if (beside) { HIPCHK(hipEventRecord(ev_pre, s_main)); HIPCHK(hipStreamWaitEvent(s_edge, ev_pre, 0)); }
      // ---- step n: single-step tiles and the box's own nodes A, B -> C; the frame's bricks A, B -> C, D, E (all three steps); wall regions
      // A, B -> C, D (x / y regions with three-step tables: -> C, D, E); box A, B -> D, E
      u0_src = A; u1 = B; u0 = C;
      tb3_src_n = n;
      launch_dirty_tiles(sw);
      bnd_sel = wl_rest; bs_vout = vh1b; bs_gout = gh1b;
      ub[0] = T1; ub[2] = X2;
      launch_rigid(sw, {0, wl_nrest});
      launch_bricks(sw, A, B, C, D, E, X2, X1, T1, T2, T3, 3);
      // receivers read u^n (B), the source goes into u^{n+1} (C) of its single-step tile, which that tile's first step (above, same stream) has
      // written and only its second step (after the box kernel) reads: the launch rides beside the walls instead of in the serial tail
      launch_io(sw, n, true, src_range()); // (sources: unless k_tb3<..., SRC> adds them itself, launch_tb3_src)
      // (debug 0x10000, an experiment: the alike blocks too beside k_tb3 instead of before it)
      hipStream_t sa = (beside && (op.debug & 0x10000)) ? s_edge : s;
      const unsigned g3 = wall_g3(); // launch groups that take all three steps in this pass
      if (g3) launch_walls_x(sa, sw, A, B, C, D, E, X2, X1, T1, T2, T3, 3, g3);
      if (0xfu & ~g3) launch_walls_x(sa, sw, A, B, C, D, nullptr, X2, X1, T1, T2, nullptr, 2, 0xfu & ~g3);
      // (the main stream joins the edge stream -- bricks, the single-step tiles' first step, receivers / source: done long before the wall launches
      // end -- BEFORE the box kernel: behind it the cross-stream wait would sit in front of the tail's first launch, 15 us of nothing)
      if (beside) { HIPCHK(hipEventRecord(ev_edge, s_edge)); HIPCHK(hipStreamWaitEvent(s_main, ev_edge, 0)); }
      if (op.timing) hipEventRecord(evt.first, s);
      launch_tb3(s, A, B, C, D, E);
      if (op.timing) { hipEventRecord(evt.second, s); tb2_ev.push_back(evt); hipEventRecord(eva.second, s); air_ev.push_back(eva); }
      if (ring_fill == 0) ring_n0 = n;
      ring_fill++; steps_done++;
      if (op.timing) { hipEventRecord(ev.second, s); step_ev.push_back(ev); ev = get_ev(); hipEventRecord(ev.first, s); }
      std::swap(vh1, vh1b); std::swap(gh1, gh1b); // the state after two (bricks, three-step regions: three) steps (the nodes inside the box: after their first)
      // ---- step n+1: single-step tiles and their nodes B, C -> D (the regions and the box have theirs)
      u0_src = B; u1 = C; u0 = D;
      launch_dirty_tiles(s);
      bs_vout = bs_gout = nullptr;
      ub[0] = T2; ub[2] = X1; // u2b = u^n of the node; its u^{n+2} where the regions put theirs
      launch_rigid(s, {0, wl_nrest});
      bnd_sel = nullptr;
      // Nothing left to step after the box kernel -- no tile steps singly (sources inside k_tb3_src), every region took its three steps --: the
      // readouts of steps n+1 and n+2 (u^{n+1} from C, u^{n+2} from D) are ONE launch instead of two dependent ones
      bool third_left = false; // does a wall region still have its third step to take?
      for (int gi = 0; gi < 4; gi++) third_left = third_left || ((((0xfu & ~g3) >> gi) & 1u) && wl_grp[gi].nreg > 0);
      const bool io_merged = src_in_kernel() && tb_ndirty == 0 && wl_nrest == 0 && !third_left && !op.timing && !(op.debug & 0x80000) && ring_fill + 2 <= ring_depth;
      if (io_merged) launch_io(s, n + 1, true, Range{0, 0}, nullptr, D);
      else launch_io(s, n + 1, true, src_range()); // receivers read u^{n+1} (C: shell, single-step tiles and the tiles that hold a receiver have it); source into u^{n+2} (D)
      ring_fill++; steps_done++;
      if (op.timing) { hipEventRecord(ev.second, s); step_ev.push_back(ev); ev = get_ev(); hipEventRecord(ev.first, s); eva = get_ev(); hipEventRecord(eva.first, s); }
      // ---- step n+2: what of the shell has not taken it yet and the single-step tiles, C, D -> E as ONE single step
      // (node values: u^{n+1} in T1, u^{n+2} in T2 -> u^{n+3} into T3; branch state in place)
      u0_src = C; u1 = D; u0 = E;
      ub[0] = T3; ub[1] = T2; ub[2] = T1;
      if (!(op.debug & 0x80000)) {
         // ... as wall regions too, in their one-step form (k_wall2<..., NS = 1>: pencils instead of a six-neighbour gather per node and
         // of the strided strip kernels; branch state in place): 4.1 GB -> 2.x GB per third step at 1024^3.  debug 0x80000: the list kernels
         // (the edge stream is only needed for generic blocks of regions that have a third step left: none with bricks and three-step regions --
         // and every event between two launches of the main stream costs microseconds of a tail that is all launch gaps)
         bool gen3 = false;
         for (int gi = 0; gi < 4; gi++) gen3 = gen3 || (((0xfu & ~g3) >> gi) & 1u && wl_grp[gi].nblk[1] > 0);
         if (beside && gen3) { HIPCHK(hipEventRecord(ev_pre, s_main)); HIPCHK(hipStreamWaitEvent(s_edge, ev_pre, 0)); }
         if (0xfu & ~g3) launch_walls_x(s, gen3 ? sw : s, C, D, E, nullptr, nullptr, T1, T2, T3, nullptr, nullptr, 1, 0xfu & ~g3);
         launch_dirty_tiles(s);
         if (op.timing) { hipEventRecord(eva.second, s); air_ev.push_back(eva); }
         bnd_sel = wl_rest;
         launch_rigid(s, {0, wl_nrest});
         bnd_sel = nullptr;
         if (beside && gen3) { HIPCHK(hipEventRecord(ev_edge, s_edge)); HIPCHK(hipStreamWaitEvent(s_main, ev_edge, 0)); }
      } else {
         launch_shell(s);
         if (op.timing) { hipEventRecord(eva.second, s); air_ev.push_back(eva); }
         launch_rigid(s, {0, Nb});
         launch_fd(s, {0, Nbl});
      }
      if (!io_merged) launch_io(s, n + 2, true, src_range());
      ring_fill++; steps_done++;
      ub[0] = T1; ub[1] = T3; ub[2] = T2; ubx[0] = X1; ubx[1] = X2; // (newest in ub[1], the one before in ub[2], ub[0] free: the single steps' convention)
      u0_src = nullptr; u0 = D; u1 = E; bufD = A; bufE = B; // bufC stays the u^{n+1} grid ...
      tb3_pick();                                           // ... on the placed cycle; off it: back towards it
      if (op.timing) { hipEventRecord(ev.second, s); step_ev.push_back(ev); }
      HIPCHK(hipGetLastError());
      if (ring_fill == ring_depth) return flush();
      return PF_OK;
   }
   // slab engines are created with the triples' box and tiles where those exist (init_tb2); a caller that hands over four grids
   // only, or whose wall regions do not fit that box, gets the pairs' geometry instead (before the first step)
   int pairs_geometry() {
      if (!tb3_geom) return PF_OK;
      free_walls();
      tb3_geom = tb3_slab = false;
      return init_tb2_impl(false);
   }
   int set_spares(void *g2, void *g3) override {
      if (in_step || pair_phase) return set_err(PF_ERR_STATE, "pf_engine_set_spares inside a step");
      if (!g2 || !g3) return set_err(PF_ERR_ARG, "pf_engine_set_spares: null grid");
      if (steps_done == 0) { int rcg = pairs_geometry(); if (rcg) return rcg; }
      if (!tb2_geom || (op.slab_first && op.slab_last)) return 1; // not an error: this engine keeps stepping singly
      bufC = (Real *)g2; bufD = (Real *)g3;
      tb2_slab = true;
      if (!wl_on && !(op.debug & 0x10000000)) { int rcw = init_walls(true); if (rcw) return rcw; }
      return PF_OK;
   }
