// pf_engine_slab_steps.inc -- part of `template <typename Real> struct Engine` (pf_engine.hip includes it INSIDE the class body; not a translation unit):
// split-phase steps of a slab of a chain: single steps, pairs and triples across two / three steps (Engine::step_begin / step_end).
   // the boundary nodes of a triple's edge planes (three per side) as one selection list for launch_boundary
   bool edge_sel3_ready() {
      if (edge_sel3) return true;
      if (edge_sel3_failed || (op.debug & PF_DBG_EDGE_SEPARATE)) return false;
      std::vector<int32_t> sel;
      if (!wl_xw[0]) for (int64_t i = bn_cut[3].lo.b; i < bn_cut[3].lo.e; i++) sel.push_back((int32_t)i); // (wl_xw: that side is no cut -- a region's and the bricks')
      if (!wl_xw[1]) for (int64_t i = bn_cut[3].hi.b; i < bn_cut[3].hi.e; i++) sel.push_back((int32_t)i);
      n_edge_sel3 = (int64_t)sel.size();
      if (upload(&edge_sel3, sel.data(), n_edge_sel3) != PF_OK) { mem.release(edge_sel3); edge_sel3_failed = true; (void)hipGetLastError(); return false; }
      return true;
   }
   int wall_streams() { // a slab's wall regions run on two streams of their own (created on first use)
      if (s_wall) return PF_OK;
      int lo_prio = 0, hi_prio = 0;
      hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio);
      HIPCHK(hipStreamCreateWithPriority(&s_wall, hipStreamNonBlocking, hi_prio));
      HIPCHK(hipStreamCreateWithPriority(&s_wall2, hipStreamNonBlocking, hi_prio));
      HIPCHK(hipEventCreateWithFlags(&ev_wall0, hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&ev_wall, hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&ev_wall2, hipEventDisableTiming));
      return PF_OK;
   }
   // split-phase step for slab chains: edge planes and every boundary list entry that lives in them first
   // (high-priority stream), interior concurrently on the main stream.
   int step_begin(int64_t n) override {
      if (in_step) return set_err(PF_ERR_STATE, "step_begin called twice");
      if (n < 0 || n >= Nt) return set_err(PF_ERR_ARG, "step %ld outside [0,Nt=%ld)", (long)n, (long)Nt);
      HIPCHK(hipSetDevice(op.device));
      if (obs_pending) { // a region observer's sample may still be reading u^n, ghost shell included, on the main stream: every form of the step begins
         // on the edge stream, which has not waited for the main stream since the step before (pf_engine_observe.inc, "The sample")
         HIPCHK(hipEventRecord(ev_obs, s_main));
         HIPCHK(hipStreamWaitEvent(s_edge, ev_obs, 0));
         obs_pending = false;
      }
      const int xl = 1, xh = (int)Nx - 2;
      // Slab engines with all four grids at hand step in temporally blocked pairs that span two split-phase steps:
      // phase 0 (step n): edge planes n -> n+1 on the edge stream; box n -> n+1, n+2 plus the shell n -> n+1 on the
      // main stream; phase 1 (step n+1): edge planes and shell n+1 -> n+2.  The exchanges in between are the usual ones.
      // Slab engines with FIVE grids and wall regions that fit step in TRIPLES across three split-phase steps (tb3_slab): the edge
      // stream owns three planes per side (single steps, exchanged after every step as always); phase 0 (step n): box n -> n+2, n+3
      // by k_tb3 -- its first and last plane leave their u^{n+1} too --, wall regions n -> n+1, n+2, the planes between edge planes and
      // box, the single-step tiles and the box's own nodes n -> n+1; phase 1: those n+1 -> n+2; phase 2: they and the whole strips
      // beside the box n+2 -> n+3 as one single step, every node of the interior planes by the list kernel.
      // A pass in flight lives in `pass` / `phase`: built here when its first step begins and kept only once nothing can fail any more (an error return
      // leaves the engine as it was), launched phase by phase as pass.grids(phase) / pass.bnd(phase); the step_end of its last step moves the engine's
      // state (Engine::end_pass).
      if (tb3_slab && (pass.len == 3 || (!in_pass() && n + 2 < Nt && ring_fill + 3 <= ring_depth && xh - xl >= 12))) {
         const int ph = phase;
         Pass p = pass;
         // round 6: with two more node-value buffers (init_walls) the triple's u^{n+2} / u^{n+3} of the nodes go where nobody reads during it --
         // what lets the wall regions and the frame's bricks take all three steps in the FIRST phase (all3); else u^{n+2} overwrites u^n and
         // u^{n+3} u^{n-1}, as before
         const bool five = ubx[0] && ubx[1], all3 = slab_all3();
         if (ph == 0) {
            if ((wl_xw[0] || wl_xw[1]) && !all3) return set_err(PF_ERR_STATE, "a slab's x wall region without three-step regions");
            { int rcs = wall_streams(); if (rcs) return rcs; }
            tb3_pick();
            p = pass_from_state(bufC, bufD, bufE, five ? ubx[0] : ub[1], five ? ubx[1] : ub[2], state_other());
         }
         // an end slab's own x wall (wl_xw): a region and bricks step it three times in phase 0 like a single domain's -- no edge planes on that side
         const bool wlo = wl_xw[0], whi = wl_xw[1];
         const int sp0 = wlo ? tbx0 : xl + 3, sp1 = whi ? tbx1 : xh - 2; // the planes between the edge planes and the box
         // (the triple's first split-phase step, in which the regions and the bricks write the other copy of the branch state, has every boundary launch write it)
         const Grids g = p.grids(ph);
         const Bnd b = p.bnd(ph);
         // The edge planes of both sides: in the second and third split-phase step of a triple they ARE the step -- four launches and two copies,
         // all launch gaps (75 us each at 1/8 of 1024^3, 150 of a triple's 760) -- so the two sides share one launch of the lean kernel (its
         // second-slab mode) and one of the boundary kernel (a selection list: the nodes of the low planes, then of the high ones)
         if (boundary_fused() && edge_sel3_ready()) {
            if (!wlo && !whi) launch_air_lean(s_edge, g, xl, xl + 3, {xh - 2, xh + 1});
            else if (!wlo) launch_air_lean(s_edge, g, xl, xl + 3);
            else launch_air_lean(s_edge, g, xh - 2, xh + 1);
            launch_rigid(s_edge, g, b.with(edge_sel3), {0, n_edge_sel3});
         } else {
            if (!wlo) { launch_air_lean(s_edge, g, xl, xl + 3); launch_rigid(s_edge, g, b, bn_cut[3].lo); }
            if (!whi) { launch_air_lean(s_edge, g, xh - 2, xh + 1); launch_rigid(s_edge, g, b, bn_cut[3].hi); }
         }
         if (!wlo) { launch_fd(s_edge, g, b, bnl_cut[3].lo); launch_io(s_edge, g, n, false, in_cut[3].lo); }
         if (!whi) { launch_fd(s_edge, g, b, bnl_cut[3].hi); launch_io(s_edge, g, n, false, in_cut[3].hi); }
         HIPCHK(hipEventRecord(ev_edge, s_edge));
         EvPair eva{}, evt{};
         if (op.timing) { eva = ev_get(); hipEventRecord(eva.first, s_main); }
         if (ph == 0) {
            HIPCHK(hipEventRecord(ev_wall0, s_main));
            HIPCHK(hipStreamWaitEvent(s_wall, ev_wall0, 0));
            HIPCHK(hipStreamWaitEvent(s_wall2, ev_wall0, 0));
            launch_tb3_src<3>(s_wall2, n, p); // the tiles around the sources (k_tb3_src): first, beside the regions
            if (all3) { // the strips beside the box and the four bars along x: all three steps now (k_wall2 NS = 3, k_brick)
               launch_bricks(s_wall2, p, 0, 3);
               launch_walls_x(s_wall, s_wall2, p, 0, 3, 0xf);
            } else launch_walls_x(s_wall, s_wall2, p, 0, 2, 0xf);
            launch_shell_planes(s_wall, g, sp0, sp1, false);
            launch_rigid(s_wall, g, b.with(wl_rest), {0, wl_nrest});
            HIPCHK(hipEventRecord(ev_wall, s_wall));
            HIPCHK(hipEventRecord(ev_wall2, s_wall2));
            wall_pending = true;
            if (op.timing) { evt = ev_get(); hipEventRecord(evt.first, s_main); }
            launch_tb3(s_main, n, p);
            if (op.timing) { hipEventRecord(evt.second, s_main); tb2_ev.push_back(evt); }
            launch_dirty_tiles(s_main, g);
            HIPCHK(hipStreamWaitEvent(s_main, ev_wall, 0)); // (a source in those planes is added after their update)
         } else if (ph == 1) {
            launch_shell_planes(s_main, g, sp0, sp1);
            launch_rigid(s_main, g, b.with(wl_rest), {0, wl_nrest});
         } else if (all3) { // the regions and the bricks are at n+3 already: the planes outside the box's x range, the single-step tiles, the box's own nodes
            launch_shell_planes(s_main, g, sp0, sp1);
            launch_rigid(s_main, g, b.with(wl_rest), {0, wl_nrest});
         } else {
            launch_shell(s_main, g, xl + 3, xh - 2);
            launch_rigid(s_main, g, b, bn_cut[3].mid);
         }
         if (op.timing) { hipEventRecord(eva.second, s_main); air_ev.push_back(eva); }
         launch_fd(s_main, g, b, bnl_cut[3].mid);
         launch_io(s_main, g, n, true, src_in_kernel() ? Range{0, 0} : in_cut[3].mid); // (sources in the box: inside k_tb3_src, Engine::launch_tb3_src)
         HIPCHK(hipGetLastError());
         pass = p;
         in_step = true;
         return PF_OK;
      }
      if (tb2_slab && !tb3_slab && (pass.len == 2 || (!in_pass() && n + 1 < Nt && ring_fill + 2 <= ring_depth && xh - xl >= 8))) {
         const bool first_half = phase == 0;
         // with wall regions (init_walls(true)): the first half also steps the row and column strips beside the box TWICE
         // (k_wall2: branch state vh1 -> vh1b, node values P2, P1 -> P0, P1), so every other boundary launch of the pair follows
         // the same buffers: first half state out of place into vh1b and node values into P0, second half both in place (P1).  Without wall regions:
         // node values as in step_pair, branch state in place
         Pass p = pass;
         if (first_half) {
            if (wl_on) { int rcs = wall_streams(); if (rcs) return rcs; }
            p = wl_on ? pass_from_state(bufC, bufD, nullptr, ub[1], nullptr, state_other()) : pass_from_state(bufC, bufD, nullptr, ub[2], nullptr, state_in_place());
         }
         const Grids g = p.grids(phase);
         const Bnd b = p.bnd(phase);
         if (fcc) {
            // 13-point: the ghost shell of u1 lives in memory; its flips touch the whole grid, ghost planes included, so
            // they go on the edge stream (ordered after the exchange that filled those planes) and the interior waits
            launch_flips(s_edge, g);
            HIPCHK(hipEventRecord(ev_pre, s_edge));
            HIPCHK(hipStreamWaitEvent(s_main, ev_pre, 0));
            launch_air_march(s_edge, g, xl, xl + 2);   // (k_air_fcc's out-of-place form)
            launch_air_march(s_edge, g, xh - 1, xh + 1);
         } else {
            // (the lean kernel explicitly, as launch_shell does: it is the one that steps out of place -- the barrier-free
            // kernel an engine may have chosen for its single steps reads u^{n-1} where it writes)
            launch_air_lean(s_edge, g, xl, xl + 2);
            launch_air_lean(s_edge, g, xh - 1, xh + 1);
         }
         launch_rigid(s_edge, g, b, bn_cut[2].lo); launch_rigid(s_edge, g, b, bn_cut[2].hi);
         launch_fd(s_edge, g, b, bnl_cut[2].lo); launch_fd(s_edge, g, b, bnl_cut[2].hi);
         launch_io(s_edge, g, n, false, in_cut[2].lo); launch_io(s_edge, g, n, false, in_cut[2].hi);
         HIPCHK(hipEventRecord(ev_edge, s_edge));
         EvPair eva{}, evt{};
         if (op.timing) { eva = ev_get(); hipEventRecord(eva.first, s_main); }
         if (first_half) {
            if (wl_on) { // beside the box kernel, on a stream of their own: a slab's regions are a few hundred waves, each a chain of dependent march steps
               // (the generic blocks -- a 0.3 ms chain of dependent steps at 1/8 of 1024^3 -- on a stream of their own: behind the
               // alike blocks' launches in ONE stream the regions, 0.52 ms, outlasted the box kernel, 0.47)
               HIPCHK(hipEventRecord(ev_wall0, s_main));
               HIPCHK(hipStreamWaitEvent(s_wall, ev_wall0, 0));
               HIPCHK(hipStreamWaitEvent(s_wall2, ev_wall0, 0));
               launch_walls_x(s_wall, s_wall2, p, 0, 2, 0xf);
               // the first step of the planes between the edge planes and the box (an end slab's x wall) and of the boundary nodes
               // no region owns: behind the alike blocks, not behind the box kernel (they only read u^{n-1}, u^n)
               launch_shell_planes(s_wall, g, xl + 2, xh - 1, false);
               launch_rigid(s_wall, g, b.with(wl_rest), {0, wl_nrest});
               HIPCHK(hipEventRecord(ev_wall, s_wall));
               HIPCHK(hipEventRecord(ev_wall2, s_wall2));
               wall_pending = true;
            }
            if (op.timing) { evt = ev_get(); hipEventRecord(evt.first, s_main); }
            launch_tb2(s_main, n, p);
            if (op.timing) { hipEventRecord(evt.second, s_main); tb2_ev.push_back(evt); }
         }
         if (wl_on && first_half) launch_dirty_tiles(s_main, g); // (the strips beside the box are the wall regions'; the planes outside it: above)
         else if (wl_on) launch_shell_planes(s_main, g, xl + 2, xh - 1);
         else launch_shell(s_main, g, xl + 2, xh - 1);
         if (op.timing) { hipEventRecord(eva.second, s_main); air_ev.push_back(eva); }
         if (wl_on && first_half) HIPCHK(hipStreamWaitEvent(s_main, ev_wall, 0)); // (a source in those planes is added after their update)
         else if (wl_on) launch_rigid(s_main, g, b.with(wl_rest), {0, wl_nrest});
         else launch_rigid(s_main, g, b, bn_cut[2].mid);
         launch_fd(s_main, g, b, bnl_cut[2].mid);
         launch_io(s_main, g, n, true, in_cut[2].mid);
         HIPCHK(hipGetLastError());
         pass = p;
         in_step = true;
         return PF_OK;
      }
      const Grids g = grids();
      const Bnd be = bnd(0, (int)Nx), bm = bnd(1, (int)Nx - 1); // (fold row: the edge stream's launches do every plane's, the main stream's the owned planes')
      if (!(lean || vg)) { // ghost flips / ABC save touch the whole grid: the interior must see them
         launch_pre(s_edge, g);
         HIPCHK(hipEventRecord(ev_pre, s_edge));
         HIPCHK(hipStreamWaitEvent(s_main, ev_pre, 0));
      }
      // edge stream: first / last owned plane
      launch_air(s_edge, g, xl, xl + 1);
      if (xh > xl) launch_air(s_edge, g, xh, xh + 1);
      launch_abc(s_edge, g, bna_cut.lo); launch_abc(s_edge, g, bna_cut.hi);
      launch_rigid(s_edge, g, be, bn_cut[1].lo); launch_rigid(s_edge, g, be, bn_cut[1].hi);
      launch_fd(s_edge, g, be, bnl_cut[1].lo); launch_fd(s_edge, g, be, bnl_cut[1].hi);
      launch_io(s_edge, g, n, false, in_cut[1].lo); launch_io(s_edge, g, n, false, in_cut[1].hi);
      HIPCHK(hipEventRecord(ev_edge, s_edge));
      // main stream: interior planes
      launch_air(s_main, g, xl + 1, xh);
      launch_abc(s_main, g, bna_cut.mid);
      launch_rigid(s_main, g, bm, bn_cut[1].mid);
      launch_fd(s_main, g, bm, bnl_cut[1].mid);
      launch_io(s_main, g, n, true, in_cut[1].mid);
      HIPCHK(hipGetLastError());
      in_step = true;
      return PF_OK;
   }
   int state_grids(void **up, void **uc) override {
      if (in_step || in_pass()) return set_err(PF_ERR_STATE, "pf_engine_state_grids inside a step");
      if (up) *up = u0;
      if (uc) *uc = u1;
      return PF_OK;
   }
   int layout(int64_t *dims, int64_t *pitch, int32_t *exchanged) override {
      if (dims) { dims[0] = Nx; dims[1] = Ny; dims[2] = Nz; }
      if (pitch) *pitch = P;
      if (exchanged) *exchanged = swz ? 1 : 0;
      return PF_OK;
   }
   int halo_ptrs(void **slo, void **shi, void **rlo, void **rhi, size_t *bytes) override {
      // the grid the step in flight writes (gpu_engine.h:1086-1126 sends the same planes)
      Real *w = grids().nxt;
      if (slo) *slo = w + plane;
      if (shi) *shi = w + (Nx - 2) * plane;
      if (rlo) *rlo = w;
      if (rhi) *rhi = w + (Nx - 1) * plane;
      if (bytes) *bytes = (size_t)plane * sizeof(Real);
      return PF_OK;
   }
   int step_end(int64_t n) override {
      if (!in_step) return set_err(PF_ERR_STATE, "step_end without step_begin");
      HIPCHK(hipSetDevice(op.device));
      // join.  The next step's edge planes (edge stream) read interior plane 2 / Nx-3: wait for the main stream.
      // The next step's interior (main stream) reads the edge planes but never the ghost planes, so it waits for
      // the edge *compute* only (ev_edge, recorded in step_begin before the exchange was issued) -- the exchange
      // itself stays off the main stream's critical path and only orders the edge stream.
      if (wall_pending) { HIPCHK(hipStreamWaitEvent(s_main, ev_wall, 0)); HIPCHK(hipStreamWaitEvent(s_main, ev_wall2, 0)); wall_pending = false; }
      HIPCHK(hipEventRecord(ev_main, s_main));
      HIPCHK(hipStreamWaitEvent(s_edge, ev_main, 0));
      HIPCHK(hipStreamWaitEvent(s_main, ev_edge, 0));
      in_step = false;
      if (in_pass()) {
         if (++phase == pass.len) { end_pass(pass); pass = Pass{}; phase = 0; }
         return after_step(n);
      }
      rotate();
      return after_step(n);
   }

