// pf_engine_slab_steps.inc -- part of `template <typename Real> struct Engine` (pf_engine.hip includes it INSIDE the class body; not a translation unit):
// split-phase steps of a slab of a chain: single steps, pairs and triples across two / three steps (Engine::step_begin / step_end).
   // the boundary nodes of a triple's edge planes (three per side) as one selection list for launch_boundary
   bool edge_sel3_ready() {
      if (edge_sel3) return true;
      if (edge_sel3_failed || (op.debug & PF_DBG_EDGE_SEPARATE)) return false;
      std::vector<int32_t> sel;
      if (!wl_xw[0]) for (int64_t i = bn_lo3.b; i < bn_lo3.e; i++) sel.push_back((int32_t)i); // (wl_xw: that side is no cut -- a region's and the bricks')
      if (!wl_xw[1]) for (int64_t i = bn_hi3.b; i < bn_hi3.e; i++) sel.push_back((int32_t)i);
      n_edge_sel3 = (int64_t)sel.size();
      if (upload(&edge_sel3, sel.data(), n_edge_sel3) != PF_OK) { edge_sel3 = nullptr; edge_sel3_failed = true; (void)hipGetLastError(); return false; }
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
      const int xl = 1, xh = (int)Nx - 2;
      // Slab engines with all four grids at hand step in temporally blocked pairs that span two split-phase steps:
      // phase 0 (step n): edge planes n -> n+1 on the edge stream; box n -> n+1, n+2 plus the shell n -> n+1 on the
      // main stream; phase 1 (step n+1): edge planes and shell n+1 -> n+2.  The exchanges in between are the usual ones.
      // Slab engines with FIVE grids and wall regions that fit step in TRIPLES across three split-phase steps (tb3_slab): the edge
      // stream owns three planes per side (single steps, exchanged after every step as always); phase 0 (step n): box n -> n+2, n+3
      // by k_tb3 -- its first and last plane leave their u^{n+1} too --, wall regions n -> n+1, n+2, the planes between edge planes and
      // box, the single-step tiles and the box's own nodes n -> n+1; phase 1: those n+1 -> n+2; phase 2: they and the whole strips
      // beside the box n+2 -> n+3 as one single step, every node of the interior planes by the list kernel.
      if (tb3_slab && (pair_phase > 0 || (n + 2 < Nt && ring_fill + 3 <= ring_depth && xh - xl >= 12))) {
         const int ph = pair_phase;
         if (ph == 0) {
            tb3_pick();
            pA = u0; pB = u1; u0_src = pA; u1 = pB; u0 = bufC;
            wsP[0] = ub[0]; wsP[1] = ub[1]; wsP[2] = ub[2];
            // round 6: with two more node-value buffers (init_walls) the triple's u^{n+2} / u^{n+3} of the nodes go where nobody reads during it --
            // what lets the wall regions and the frame's bricks take all three steps in THIS phase (ws_all3); else u^{n+2} overwrites u^n and
            // u^{n+3} u^{n-1}, as before
            ws_five = ubx[0] && ubx[1];
            wsT2 = ws_five ? ubx[0] : wsP[1]; wsT3 = ws_five ? ubx[1] : wsP[2];
            unsigned gblk = 0;
            for (int gi = 0; gi < 4; gi++) if (wl_grp[gi].nblk[0] + wl_grp[gi].nblk[1] + wl_grp[gi].nblk[2]) gblk |= 1u << gi;
            ws_all3 = ws_five && wl_nbrk > 0 && gblk != 0 && (gblk & ~wall_g3()) == 0;
            if ((wl_xw[0] || wl_xw[1]) && !ws_all3) return set_err(PF_ERR_STATE, "a slab's x wall region without three-step regions");
         }
         // an end slab's own x wall (wl_xw): a region and bricks step it three times in phase 0 like a single domain's -- no edge planes on that side
         const bool wlo = wl_xw[0], whi = wl_xw[1];
         const int sp0 = wlo ? tbx0 : xl + 3, sp1 = whi ? tbx1 : xh - 2; // the planes between the edge planes and the box
         // grids, node values and branch state as the phase machine (here and in step_end) has left them; the triple's first split-phase step, in which
         // the regions and the bricks write the other copy of the branch state, has every boundary launch write it
         const Grids g = grids();
         Bnd b = bnd(0, 0);
         if (ph == 0) b.out = {vh1b, gh1b};
         // The edge planes of both sides: in the second and third split-phase step of a triple they ARE the step -- four launches and two copies,
         // all launch gaps (75 us each at 1/8 of 1024^3, 150 of a triple's 760) -- so the two sides share one launch of the lean kernel (its
         // second-slab mode) and one of the boundary kernel (a selection list: the nodes of the low planes, then of the high ones)
         if (boundary_fused() && edge_sel3_ready()) {
            if (!wlo && !whi) launch_air_lean(s_edge, g, xl, xl + 3, {xh - 2, xh + 1});
            else if (!wlo) launch_air_lean(s_edge, g, xl, xl + 3);
            else launch_air_lean(s_edge, g, xh - 2, xh + 1);
            launch_rigid(s_edge, g, b.with(edge_sel3), {0, n_edge_sel3});
         } else {
            if (!wlo) { launch_air_lean(s_edge, g, xl, xl + 3); launch_rigid(s_edge, g, b, bn_lo3); }
            if (!whi) { launch_air_lean(s_edge, g, xh - 2, xh + 1); launch_rigid(s_edge, g, b, bn_hi3); }
         }
         if (!wlo) { launch_fd(s_edge, g, b, bnl_lo3); launch_io(s_edge, g, n, false, in_lo3); }
         if (!whi) { launch_fd(s_edge, g, b, bnl_hi3); launch_io(s_edge, g, n, false, in_hi3); }
         HIPCHK(hipEventRecord(ev_edge, s_edge));
         EvPair eva{}, evt{};
         if (op.timing) { eva = ev_get(); hipEventRecord(eva.first, s_main); }
         if (ph == 0) {
            { int rcs = wall_streams(); if (rcs) return rcs; }
            HIPCHK(hipEventRecord(ev_wall0, s_main));
            HIPCHK(hipStreamWaitEvent(s_wall, ev_wall0, 0));
            HIPCHK(hipStreamWaitEvent(s_wall2, ev_wall0, 0));
            launch_tb3_src<3>(s_wall2, n, pA, pB, bufC, bufD, bufE); // the tiles around the sources (k_tb3_src): first, beside the regions
            if (ws_all3) { // the strips beside the box and the four bars along x: all three steps now (k_wall2 NS = 3, k_brick)
               launch_bricks(s_wall2, pA, pB, bufC, bufD, bufE, wsP[2], wsP[1], wsP[0], wsT2, wsT3, b.in, b.out, 3);
               launch_walls_x(s_wall, s_wall2, pA, pB, bufC, bufD, bufE, wsP[2], wsP[1], wsP[0], wsT2, wsT3, b.in, b.out, 3, 0xf);
            } else if (ws_five) launch_walls_x(s_wall, s_wall2, pA, pB, bufC, bufD, nullptr, wsP[2], wsP[1], wsP[0], wsT2, nullptr, b.in, b.out, 2, 0xf);
            else launch_walls(s_wall, s_wall2, pA, pB, bufC, bufD, wsP[0], wsP[1], wsP[2], b.in, b.out);
            launch_shell_planes(s_wall, g, sp0, sp1, false);
            launch_rigid(s_wall, g, b.with(wl_rest), {0, wl_nrest});
            HIPCHK(hipEventRecord(ev_wall, s_wall));
            HIPCHK(hipEventRecord(ev_wall2, s_wall2));
            wall_pending = true;
            if (op.timing) { evt = ev_get(); hipEventRecord(evt.first, s_main); }
            launch_tb3(s_main, n, pA, pB, bufC, bufD, bufE);
            if (op.timing) { hipEventRecord(evt.second, s_main); tb2_ev.push_back(evt); }
            launch_dirty_tiles(s_main, g);
            HIPCHK(hipStreamWaitEvent(s_main, ev_wall, 0)); // (a source in those planes is added after their update)
         } else if (ph == 1) {
            launch_shell_planes(s_main, g, sp0, sp1);
            launch_rigid(s_main, g, b.with(wl_rest), {0, wl_nrest});
         } else if (ws_all3) { // the regions and the bricks are at n+3 already: the planes outside the box's x range, the single-step tiles, the box's own nodes
            launch_shell_planes(s_main, g, sp0, sp1);
            launch_rigid(s_main, g, b.with(wl_rest), {0, wl_nrest});
         } else {
            launch_shell(s_main, g, xl + 3, xh - 2);
            launch_rigid(s_main, g, b, bn_mid3);
         }
         if (op.timing) { hipEventRecord(eva.second, s_main); air_ev.push_back(eva); }
         launch_fd(s_main, g, b, bnl_mid3);
         launch_io(s_main, g, n, true, src_in_kernel() ? Range{0, 0} : in_mid3); // (sources in the box: inside k_tb3_src, Engine::launch_tb3_src)
         HIPCHK(hipGetLastError());
         in_step = true;
         pair_now = true; triple_now = true;
         return PF_OK;
      }
      if (tb2_slab && !tb3_slab && (pair_phase == 1 || (n + 1 < Nt && ring_fill + 2 <= ring_depth && xh - xl >= 8))) {
         const bool first_half = pair_phase == 0;
         // with wall regions (init_walls(true)): the first half also steps the row and column strips beside the box TWICE
         // (k_wall2: branch state vh1 -> vh1b, node values P2, P1 -> P0, P1), so every other boundary launch of the pair follows
         // the same buffers: first half state out of place into vh1b and node values into P0, second half both in place (P1)
         if (first_half) {
            pA = u0; pB = u1; u0_src = pA; u1 = pB; u0 = bufC;
            if (wl_on) { wsP[0] = ub[0]; wsP[1] = ub[1]; wsP[2] = ub[2]; }
         }
         const Grids g = grids();
         Bnd b = bnd(0, 0); // (no fold row: virtual-ghost modes with one do not block in pairs)
         if (wl_on && first_half) b.out = {vh1b, gh1b};
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
         launch_rigid(s_edge, g, b, bn_lo2); launch_rigid(s_edge, g, b, bn_hi2);
         launch_fd(s_edge, g, b, bnl_lo2); launch_fd(s_edge, g, b, bnl_hi2);
         launch_io(s_edge, g, n, false, in_lo2); launch_io(s_edge, g, n, false, in_hi2);
         HIPCHK(hipEventRecord(ev_edge, s_edge));
         EvPair eva{}, evt{};
         if (op.timing) { eva = ev_get(); hipEventRecord(eva.first, s_main); }
         if (first_half) {
            if (wl_on) { // beside the box kernel, on a stream of their own: a slab's regions are a few hundred waves, each a chain of dependent march steps
               { int rcs = wall_streams(); if (rcs) return rcs; }
               // (the generic blocks -- a 0.3 ms chain of dependent steps at 1/8 of 1024^3 -- on a stream of their own: behind the
               // alike blocks' launches in ONE stream the regions, 0.52 ms, outlasted the box kernel, 0.47)
               HIPCHK(hipEventRecord(ev_wall0, s_main));
               HIPCHK(hipStreamWaitEvent(s_wall, ev_wall0, 0));
               HIPCHK(hipStreamWaitEvent(s_wall2, ev_wall0, 0));
               launch_walls(s_wall, s_wall2, pA, pB, bufC, bufD, wsP[0], wsP[1], wsP[2], b.in, b.out);
               // the first step of the planes between the edge planes and the box (an end slab's x wall) and of the boundary nodes
               // no region owns: behind the alike blocks, not behind the box kernel (they only read u^{n-1}, u^n)
               launch_shell_planes(s_wall, g, xl + 2, xh - 1, false);
               launch_rigid(s_wall, g, b.with(wl_rest), {0, wl_nrest});
               HIPCHK(hipEventRecord(ev_wall, s_wall));
               HIPCHK(hipEventRecord(ev_wall2, s_wall2));
               wall_pending = true;
            }
            if (op.timing) { evt = ev_get(); hipEventRecord(evt.first, s_main); }
            launch_tb2(s_main, n, pA, pB, bufC, bufD);
            if (op.timing) { hipEventRecord(evt.second, s_main); tb2_ev.push_back(evt); }
         }
         if (wl_on && first_half) launch_dirty_tiles(s_main, g); // (the strips beside the box are the wall regions'; the planes outside it: above)
         else if (wl_on) launch_shell_planes(s_main, g, xl + 2, xh - 1);
         else launch_shell(s_main, g, xl + 2, xh - 1);
         if (op.timing) { hipEventRecord(eva.second, s_main); air_ev.push_back(eva); }
         if (wl_on && first_half) HIPCHK(hipStreamWaitEvent(s_main, ev_wall, 0)); // (a source in those planes is added after their update)
         else if (wl_on) launch_rigid(s_main, g, b.with(wl_rest), {0, wl_nrest});
         else launch_rigid(s_main, g, b, bn_mid2);
         launch_fd(s_main, g, b, bnl_mid2);
         launch_io(s_main, g, n, true, in_mid2);
         HIPCHK(hipGetLastError());
         in_step = true;
         pair_now = true;
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
      launch_abc(s_edge, g, bna_lo); launch_abc(s_edge, g, bna_hi);
      launch_rigid(s_edge, g, be, bn_lo); launch_rigid(s_edge, g, be, bn_hi);
      launch_fd(s_edge, g, be, bnl_lo); launch_fd(s_edge, g, be, bnl_hi);
      launch_io(s_edge, g, n, false, in_lo); launch_io(s_edge, g, n, false, in_hi);
      HIPCHK(hipEventRecord(ev_edge, s_edge));
      // main stream: interior planes
      launch_air(s_main, g, xl + 1, xh);
      launch_abc(s_main, g, bna_mid);
      launch_rigid(s_main, g, bm, bn_mid);
      launch_fd(s_main, g, bm, bnl_mid);
      launch_io(s_main, g, n, true, in_mid);
      HIPCHK(hipGetLastError());
      in_step = true;
      return PF_OK;
   }
   int state_grids(void **up, void **uc) override {
      if (in_step || pair_phase) return set_err(PF_ERR_STATE, "pf_engine_state_grids inside a step");
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
      // new state is u0 until step_end rotates (gpu_engine.h:1086-1126 sends the same planes)
      if (slo) *slo = u0 + plane;
      if (shi) *shi = u0 + (Nx - 2) * plane;
      if (rlo) *rlo = u0;
      if (rhi) *rhi = u0 + (Nx - 1) * plane;
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
      if (pair_now && triple_now) {
         pair_now = triple_now = false;
         if (pair_phase == 0) {        // u^{n+1} complete in bufC; node values and branch state in place from here on
            ub[0] = wsT2; ub[2] = wsP[1]; // (three buffers: both wsP[1] -- a node's u^{n+2} overwrites its u^n)
            std::swap(vh1, vh1b); std::swap(gh1, gh1b);
            u0_src = pB; u1 = bufC; u0 = bufD;
            pair_phase = 1;
         } else if (pair_phase == 1) { // u^{n+2} complete in bufD; node values: u^{n+1} in P0, u^{n+2} in T2 (= P1 with three buffers) -> u^{n+3} into T3 (= P2)
            ub[0] = wsT3; ub[1] = wsT2; ub[2] = wsP[0];
            u0_src = bufC; u1 = bufD; u0 = bufE;
            pair_phase = 2;
         } else {                      // triple done: state = (bufD, bufE), the former state grids become the next targets
            ub[0] = wsP[0]; ub[1] = wsT3; ub[2] = wsT2;
            if (ws_five) { ubx[0] = wsP[1]; ubx[1] = wsP[2]; }
            Real *D = bufD, *E = bufE;
            u0_src = nullptr; u0 = D; u1 = E; bufD = pA; bufE = pB;
            pair_phase = 0;
         }
         return after_step(n);
      }
      if (pair_now) {
         pair_now = false;
         if (wl_on) {
            if (pair_phase == 0) { // second half: node values and branch state in place
               ub[0] = ub[2] = wsP[1];
               std::swap(vh1, vh1b); std::swap(gh1, gh1b);
            } else { ub[0] = wsP[2]; ub[1] = wsP[1]; ub[2] = wsP[0]; }
         } else { Real *t = ub[2]; ub[2] = ub[1]; ub[1] = ub[0]; ub[0] = t; }
         if (pair_phase == 0) { // u^{n+1} is complete in bufC: second half reads u^n as the old state and writes bufD
            u0_src = pB; u1 = bufC; u0 = bufD;
            pair_phase = 1;
         } else {               // pair done: state = (bufC, bufD), the former state grids become the spares
            Real *C = bufC, *D = bufD;
            u0_src = nullptr; u0 = C; u1 = D; bufC = pA; bufD = pB;
            pair_phase = 0;
         }
         return after_step(n);
      }
      rotate();
      return after_step(n);
   }

