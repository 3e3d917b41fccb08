// pf_engine_blocked_steps.inc -- part of `template <typename Real> struct Engine` (pf_engine.hip includes it INSIDE the class body; not a translation unit):
// single-domain pairs, pairs with wall regions and triples (Engine::step_pair, step_pair_walls, step_triple), the five-grid role cycle,
// pf_engine_set_spares.
   // The pass that starts at the engine's state: it writes the grids C, D (, E); node values: u^{n-1}, u^n in ub[2], ub[1], u^{n+1} into the free buffer ub[0],
   // u^{n+2}, u^{n+3} into t2, t3; branch state (vh1, gh1) -> s1
   Pass pass_from_state(Real *C, Real *D, Real *E, Real *t2, Real *t3, BranchState s1) const {
      Pass p = Pass::of_grids(u0, u1, C, D, E);
      p.x[0] = ub[2]; p.x[1] = ub[1]; p.x[2] = ub[0]; p.x[3] = t2; p.x[4] = t3;
      p.s0 = {vh1, gh1}; p.s1 = s1;
      return p;
   }
   BranchState state_in_place() const { return {vh1, gh1}; }
   BranchState state_other() const { return {vh1b, gh1b}; }
   // The engine's state after pass p, the one assignment that ends it (the single domain's drivers and Engine::step_end).  Grids: the state is the pass's
   // last two, and the slots (bufC / bufD / bufE) those came from receive its first two -- the former state grids become the next targets.  Node values,
   // in the single steps' convention (newest in ub[1], the ones before in ub[2], ub[0] free), with x = {X2, X1, T1, T2, T3}:
   //   pairs without wall regions (T2 == X2)        ub = {X1, X2, T1}
   //   pairs with wall regions                      ub = {X2, T2, T1}; T2 a buffer of its own (a single domain's): ubx[0] = X1
   //   triples                                      ub = {T1, T3, T2}; five buffers: ubx = {X1, X2}
   // Branch state: s1, the other copy s0 (stepped in place: nothing to do).
   void end_pass(const Pass &p) {
      const int L = p.len;
      for (Real **slot : {&bufC, &bufD, &bufE}) {
         if (*slot == p.g[L]) *slot = p.g[0];
         else if (*slot == p.g[L + 1]) *slot = p.g[1];
      }
      u0 = p.g[L]; u1 = p.g[L + 1];
      const bool more = p.x[3] != p.x[0] && p.x[3] != p.x[1]; // u^{n+2} of the nodes went to a buffer of its own
      ub[1] = p.x[L + 1]; ub[2] = p.x[L];
      if (L == 3) { ub[0] = p.x[2]; if (more) { ubx[0] = p.x[1]; ubx[1] = p.x[0]; } }
      else { ub[0] = p.x[3] == p.x[0] ? p.x[1] : p.x[0]; if (more) ubx[0] = p.x[1]; }
      if (p.s1.v != p.s0.v) { vh1 = p.s1.v; gh1 = p.s1.g; vh1b = p.s0.v; gh1b = p.s0.g; }
   }
   // steps n and n+1 in one go; the state moves from (u0, u1) to (bufC, bufD), which swap roles with them
   int step_pair(int64_t n) {
      if (n < 0 || n + 1 >= Nt) return set_err(PF_ERR_ARG, "step pair %ld outside [0,Nt=%ld)", (long)n, (long)Nt);
      if (wl_on) return step_pair_walls(n);
      if (fb_on) return step_pair_fcc_bricks(n);
      hipStream_t s = s_main;
      // node values: step n reads u^{n-1} and writes the free buffer, step n+1 reads u^n and writes over u^{n-1}; branch state in place
      const Pass p = pass_from_state(bufC, bufD, nullptr, ub[2], nullptr, state_in_place());
      // the column strips update their own boundary nodes (zs_map): the list kernel visits the others and takes the strips' branch ODEs along
      const bool strips = zs_map != nullptr;
      const Range nodes = strips ? Range{0, zs_nrest} : Range{0, Nb};
      const Grids g1 = p.grids(0), g2 = p.grids(1);
      const Bnd b1 = p.bnd(0, strips ? zs_rest : nullptr), b2 = p.bnd(1, b1.sel);
      EvPair ev{}, eva{}, evt{};
      if (op.timing) { ev = ev_get(); eva = ev_get(); hipEventRecord(ev.first, s); hipEventRecord(eva.first, s); } // step events: one per step
      // The FIRST step of the shell reads u^{n-1}, u^n only and writes cells the pair kernel does not: it runs BESIDE the pair
      // kernel, on the edge stream (its launches are small and latency-bound -- strided strips, list gathers -- and fill the gaps
      // the bandwidth-bound pair kernel leaves); the second step needs the box's u^{n+1} and follows.  PF_DBG_WALLS_ONE_STREAM: one stream.
      const bool beside = !(op.debug & PF_DBG_WALLS_ONE_STREAM);
      hipStream_t sh = beside ? s_edge : s;
      if (beside) { HIPCHK(hipEventRecord(ev_pre, s)); HIPCHK(hipStreamWaitEvent(s_edge, ev_pre, 0)); }
      launch_shell(sh, g1, strips ? b1.u0b : nullptr);
      launch_rigid(sh, g1, b1, nodes, strips);
      launch_fd(sh, g1, b1, {0, Nbl});
      launch_io(sh, g1, n, true, src_range());
      // (with per-launch events on, the pair kernel waits for the shell: its recorded duration is the kernel's own, not the overlap's)
      if (op.timing && beside) { HIPCHK(hipEventRecord(ev_edge, s_edge)); HIPCHK(hipStreamWaitEvent(s, ev_edge, 0)); }
      if (op.timing) { evt = ev_get(); hipEventRecord(evt.first, s); }
      launch_tb2(s, n, p);
      if (op.timing) { hipEventRecord(evt.second, s); tb2_ev.push_back(evt); }
      if (beside && !op.timing) { HIPCHK(hipEventRecord(ev_edge, s_edge)); HIPCHK(hipStreamWaitEvent(s, ev_edge, 0)); }
      if (op.timing) { hipEventRecord(eva.second, s); air_ev.push_back(eva); eva = ev_get(); } // ("air" of the first step: the pair kernel and the shell beside it)
      if (ring_fill == 0) ring_n0 = n;
      ring_fill++; steps_done++;
      if (op.timing) { hipEventRecord(ev.second, s); step_ev.push_back(ev); ev = ev_get(); hipEventRecord(ev.first, s); hipEventRecord(eva.first, s); }
      launch_shell(s, g2, strips ? b2.u0b : nullptr);
      if (op.timing) { hipEventRecord(eva.second, s); air_ev.push_back(eva); }
      launch_rigid(s, g2, b2, nodes, strips);
      launch_fd(s, g2, b2, {0, Nbl});
      launch_io(s, g2, n + 1, true, src_range());
      ring_fill++; steps_done++;
      end_pass(p);
      if (op.timing) { hipEventRecord(ev.second, s); step_ev.push_back(ev); }
      HIPCHK(hipGetLastError());
      if (ring_fill == ring_depth) return flush();
      return PF_OK;
   }
   // steps n and n+1 with the shell in pairs as well.  Order: box (both steps), then the first step of what no wall region
   // owns -- the box's dirty tiles and the boundary nodes inside it --, source / receivers of step n, the wall regions (both
   // steps; they read u^{n-1}, u^n and the old branch state only), then the second step of the dirty tiles and their nodes.
   int step_pair_walls(int64_t n) {
      hipStream_t s = s_main;
      // An engine that steps in triples (five grids) ends a run whose length is no multiple of three with a pair: it writes u^{n+1}, u^{n+2} into
      // the two grids a TRIPLE would have written (tb3_pick: the placed cycle's targets), not into the fifth grid -- the four streams of the
      // pair's box kernel are then the assignment the placement search measured (round 5 wrote the fifth grid: an off-cycle launch, 3.0-3.2 ms
      // where the cycle's takes 2.95, and another one for the first triple of the next run), and the state lands where a triple leaves it.
      const bool on_cycle = tb3 && bufE && bufE != u0 && bufE != u1 && bufD != u0 && bufD != u1;
      // node values: u^{n-1}, u^n are only read; u^{n+1}, u^{n+2} go to two buffers nobody reads during the pair (round 6: five node-value buffers, so
      // that a region's or a brick's halo node may be evaluated while its owner already stores)
      // branch state: everything that takes both steps reads s0 and writes s1; the box's own nodes s0 -> s1 in their first step, s1 in place in their second
      const Pass p = pass_from_state(on_cycle ? bufD : bufC, on_cycle ? bufE : bufD, nullptr, ubx[0], nullptr, state_other());
      const Grids g1 = p.grids(0), g2 = p.grids(1);
      EvPair ev{}, ev2{}, evt{}, eva{};
      // "air" of a pair with wall regions (pf_timing.air_ms_total, the CLI's "Air update" line): the alike blocks' launches and the
      // box kernel on the main stream -- the regions' boundary nodes are inside those launches and cannot be told apart
      if (op.timing) { ev = ev_get(); ev2 = ev_get(); evt = ev_get(); eva = ev_get(); hipEventRecord(ev.first, s); hipEventRecord(eva.first, s); }
      // The wall regions read u^{n-1}, u^n and the old branch state only and write cells the box kernel does not: any order will do.
      // The generic blocks (edges, corners: a few hundred waves, each a long chain of dependent steps) go to the second stream
      // and run beside the alike blocks' launches, which are issue-bound; beside the bandwidth-bound box kernel they crawl
      // (measured: 0.47 -> 3.6 ms), so that one comes after.  PF_DBG_WALLS_ONE_STREAM: everything on the main stream.
      const bool beside = !(op.debug & PF_DBG_WALLS_ONE_STREAM);
      hipStream_t sw = beside ? s_edge : s_main;
      if (beside) { HIPCHK(hipEventRecord(ev_pre, s_main)); HIPCHK(hipStreamWaitEvent(s_edge, ev_pre, 0)); }
      launch_dirty_tiles(sw, g1);
      launch_rigid(sw, g1, p.bnd(0, wl_rest), {0, wl_nrest});
      launch_bricks(sw, p, 0, 2); // the frame: both steps, beside the alike blocks
      launch_walls_x(s, sw, p, 0, 2, 0xf); // (every wall launch beside the box kernel instead of before it: 492 vs 511-516 Gvox/s)
      if (op.timing) hipEventRecord(evt.first, s);
      launch_tb2(s, n, p);
      if (op.timing) { hipEventRecord(evt.second, s); tb2_ev.push_back(evt); hipEventRecord(eva.second, s); air_ev.push_back(eva); }
      if (beside) { HIPCHK(hipEventRecord(ev_edge, s_edge)); HIPCHK(hipStreamWaitEvent(s_main, ev_edge, 0)); }
      launch_io(s, g1, n, true, src_range()); // (receivers read u^n; the source goes into u^{n+1}, which only the second step below reads -- or went in inside k_tb3<..., SRC>)
      if (ring_fill == 0) ring_n0 = n;
      ring_fill++; steps_done++;
      if (op.timing) { hipEventRecord(ev.second, s); step_ev.push_back(ev); hipEventRecord(ev2.first, s); }
      launch_dirty_tiles(s, g2);
      launch_rigid(s, g2, p.bnd(1, wl_rest), {0, wl_nrest}); // second step of the box's nodes: u2b = u^n of the node, its u^{n+2} where the regions put theirs
      launch_io(s, g2, n + 1, true, src_range());
      ring_fill++; steps_done++;
      end_pass(p); // (on the cycle: bufC stays the triples' u^{n+1} grid)
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
      // grids A, B = the state -> C, D, E = bufC, bufD, bufE; node values: u^{n-1}, u^n are only read during the triple, u^{n+1}, u^{n+2}, u^{n+3} go to three
      // other buffers (five); branch state: whatever takes two or three steps in its first launch reads s0 and writes s1, every later launch of the pass s1 in place
      const Pass p = pass_from_state(bufC, bufD, bufE, ubx[0], ubx[1], state_other());
      const Grids g1 = p.grids(0), g2 = p.grids(1), g3s = p.grids(2);
      EvPair ev{}, evt{}, eva{};
      if (op.timing) { ev = ev_get(); evt = ev_get(); eva = ev_get(); hipEventRecord(ev.first, s); hipEventRecord(eva.first, s); }
      const bool beside = !(op.debug & PF_DBG_WALLS_ONE_STREAM);
      hipStream_t sw = beside ? s_edge : s_main; // the bricks (or the generic wall blocks) and the first step of the single-step tiles: beside the alike blocks
      if (beside) { HIPCHK(hipEventRecord(ev_pre, s_main)); HIPCHK(hipStreamWaitEvent(s_edge, ev_pre, 0)); }
      // ---- step n: single-step tiles and the box's own nodes A, B -> C; the frame's bricks A, B -> C, D, E (all three steps); wall regions
      // A, B -> C, D (x / y regions with three-step tables: -> C, D, E); box A, B -> D, E
      launch_dirty_tiles(sw, g1);
      launch_rigid(sw, g1, p.bnd(0, wl_rest), {0, wl_nrest});
      launch_bricks(sw, p, 0, 3);
      // receivers read u^n (B), the source goes into u^{n+1} (C) of its single-step tile, which that tile's first step (above, same stream) has
      // written and only its second step (after the box kernel) reads: the launch rides beside the walls instead of in the serial tail
      launch_io(sw, g1, n, true, src_range()); // (sources: unless k_tb3<..., SRC> adds them itself, launch_tb3_src)
      // (PF_DBG_WALLS_BESIDE_BOX, an experiment: the alike blocks too beside k_tb3 instead of before it)
      hipStream_t sa = (beside && (op.debug & PF_DBG_WALLS_BESIDE_BOX)) ? s_edge : s;
      const unsigned g3 = wall_g3(); // launch groups that take all three steps in this pass
      if (g3) launch_walls_x(sa, sw, p, 0, 3, g3);
      if (0xfu & ~g3) launch_walls_x(sa, sw, p, 0, 2, 0xfu & ~g3);
      // (the main stream joins the edge stream -- bricks, the single-step tiles' first step, receivers / source: done long before the wall launches
      // end -- BEFORE the box kernel: behind it the cross-stream wait would sit in front of the tail's first launch, 15 us of nothing)
      if (beside) { HIPCHK(hipEventRecord(ev_edge, s_edge)); HIPCHK(hipStreamWaitEvent(s_main, ev_edge, 0)); }
      if (op.timing) hipEventRecord(evt.first, s);
      launch_tb3(s, n, p);
      if (op.timing) { hipEventRecord(evt.second, s); tb2_ev.push_back(evt); hipEventRecord(eva.second, s); air_ev.push_back(eva); }
      if (ring_fill == 0) ring_n0 = n;
      ring_fill++; steps_done++;
      if (op.timing) { hipEventRecord(ev.second, s); step_ev.push_back(ev); ev = ev_get(); hipEventRecord(ev.first, s); }
      // ---- step n+1: single-step tiles and their nodes B, C -> D (the regions and the box have theirs); branch state from here on: S1 -- after two
      // (bricks, three-step regions: three) steps, the nodes inside the box: after their first
      launch_dirty_tiles(s, g2);
      launch_rigid(s, g2, p.bnd(1, wl_rest), {0, wl_nrest}); // u2b = u^n of the node; its u^{n+2} where the regions put theirs
      // Nothing left to step after the box kernel -- no tile steps singly (sources inside k_tb3_src), every region took its three steps --: the
      // readouts of steps n+1 and n+2 (u^{n+1} from C, u^{n+2} from D) are ONE launch instead of two dependent ones
      bool third_left = false; // does a wall region still have its third step to take?
      for (int gi = 0; gi < 4; gi++) third_left = third_left || ((((0xfu & ~g3) >> gi) & 1u) && wl_grp[gi].nreg > 0);
      const bool io_merged = src_in_kernel() && tb_ndirty == 0 && wl_nrest == 0 && !third_left && !op.timing && !(op.debug & PF_DBG_THIRD_STEP_LISTS) && ring_fill + 2 <= ring_depth;
      if (io_merged) launch_io(s, g2, n + 1, true, Range{0, 0}, nullptr, p.g[3]);
      else launch_io(s, g2, n + 1, true, src_range()); // receivers read u^{n+1} (C: shell, single-step tiles and the tiles that hold a receiver have it); source into u^{n+2} (D)
      ring_fill++; steps_done++;
      if (op.timing) { hipEventRecord(ev.second, s); step_ev.push_back(ev); ev = ev_get(); hipEventRecord(ev.first, s); eva = ev_get(); hipEventRecord(eva.first, s); }
      // ---- step n+2: what of the shell has not taken it yet and the single-step tiles, C, D -> E as ONE single step
      // (node values: u^{n+1}, u^{n+2} -> u^{n+3}; branch state in place)
      const Bnd b3 = p.bnd(2);
      if (!(op.debug & PF_DBG_THIRD_STEP_LISTS)) {
         // ... as wall regions too, in their one-step form (k_wall2<..., NS = 1>: pencils instead of a six-neighbour gather per node and
         // of the strided strip kernels; branch state in place): 4.1 GB -> 2.x GB per third step at 1024^3.  PF_DBG_THIRD_STEP_LISTS: the list kernels
         // (the edge stream is only needed for generic blocks of regions that have a third step left: none with bricks and three-step regions --
         // and every event between two launches of the main stream costs microseconds of a tail that is all launch gaps)
         bool gen3 = false;
         for (int gi = 0; gi < 4; gi++) gen3 = gen3 || (((0xfu & ~g3) >> gi) & 1u && wl_grp[gi].nblk[1] > 0);
         if (beside && gen3) { HIPCHK(hipEventRecord(ev_pre, s_main)); HIPCHK(hipStreamWaitEvent(s_edge, ev_pre, 0)); }
         if (0xfu & ~g3) launch_walls_x(s, gen3 ? sw : s, p, 2, 1, 0xfu & ~g3);
         launch_dirty_tiles(s, g3s);
         if (op.timing) { hipEventRecord(eva.second, s); air_ev.push_back(eva); }
         launch_rigid(s, g3s, b3.with(wl_rest), {0, wl_nrest});
         if (beside && gen3) { HIPCHK(hipEventRecord(ev_edge, s_edge)); HIPCHK(hipStreamWaitEvent(s_main, ev_edge, 0)); }
      } else {
         launch_shell(s, g3s);
         if (op.timing) { hipEventRecord(eva.second, s); air_ev.push_back(eva); }
         launch_rigid(s, g3s, b3, {0, Nb});
         launch_fd(s, g3s, b3, {0, Nbl});
      }
      if (!io_merged) launch_io(s, g3s, n + 2, true, src_range());
      ring_fill++; steps_done++;
      // the state after the triple
      end_pass(p); // bufC stays the u^{n+1} grid ...
      tb3_pick();  // ... on the placed cycle; off it: back towards it
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
      if (in_step || in_pass()) return set_err(PF_ERR_STATE, "pf_engine_set_spares inside a step");
      if (!g2 || !g3) return set_err(PF_ERR_ARG, "pf_engine_set_spares: null grid");
      if (steps_done == 0) { int rcg = pairs_geometry(); if (rcg) return rcg; }
      if (!tb2_geom || (op.slab_first && op.slab_last)) return 1; // not an error: this engine keeps stepping singly
      bufC = (Real *)g2; bufD = (Real *)g3;
      tb2_slab = true;
      if (!wl_on && !(op.debug & PF_DBG_NO_WALL_REGIONS)) { int rcw = init_walls(true); if (rcw) return rcw; }
      return PF_OK;
   }
