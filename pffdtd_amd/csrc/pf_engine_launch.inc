// pf_engine_launch.inc -- part of `template <typename Real> struct Engine` (pf_engine.hip includes it INSIDE the class body; not a translation unit):
// kernel launchers (blocked kernels, single-step shell, marching / lean interior kernels, boundary pass, I/O).  Each takes what it reads and
// writes as arguments (Engine::Grids, Engine::Bnd) and names no state grid or node buffer of the engine itself.
   pf::Tb2Params tile_params() const {
      pf::Tb2Params tp{};
      tp.plane = plane; tp.Nx = (int)Nx; tp.Ny = (int)Ny; tp.Nz = (int)Nz; tp.P = (int)P;
      tp.x_begin = tbx0; tp.x_end = tbx1; tp.y_begin = tby0; tp.y_end = tby1; tp.z_begin = tbz0; tp.z_end = tbz1;
      tp.chunk = tb_chunk; tp.nxc = tb_nxc; tp.nyt = tb_nyt; tp.nzt = tb_nzt;
      return tp;
   }
   // The blocked kernels take a whole pass (Engine::Pass) and read its grids only: A = g[0] = u^{n-1}, B = g[1] = u^n -> C, D, E = g[2], g[3], g[4].
   pf::Tb2Params tile_params(const Pass &p, int ns) const {
      pf::Tb2Params tp = tile_params();
      tp.A = p.g[0]; tp.B = p.g[1]; tp.C = p.g[2]; tp.D = p.g[3]; tp.E = ns == 3 ? p.g[4] : nullptr;
      return tp;
   }
   // three steps of the clean tiles: -> D = u^{n+2}, E = u^{n+3}; C: where flagged tiles leave their u^{n+1} (null: nowhere)
   void launch_tb3(hipStream_t s, int64_t n, const Pass &p, bool sample = false) {
      if (tb_xr.empty() || tb_nclean <= 0) return;
      pf::Tb2Params tp = tile_params(p, 3);
      if (!(op.slab_first && op.slab_last)) tp.band |= 2; // a slab: the planes beside the box read the u^{n+1} of its first and last plane
      sample = sample && tb_sample && tb_nsample > 0;
      const bool forked = !sample && fork_tb3_src<3>(s, n, p);
      tp.tiles = sample ? tb_sample : tb_clean;
      const dim3 g((uint32_t)(sample ? tb_nsample : tb_nclean)), b(64 * tb3_wt);
      if (sg) {
         if (tb2_probe) hipLaunchKernelGGL((pf::k_tb3<Real, tb3_r, tb3_wt, true, true>), g, b, 0, s, tp, a1, a2);
         else hipLaunchKernelGGL((pf::k_tb3<Real, tb3_r, tb3_wt, true, false>), g, b, 0, s, tp, a1, a2);
      } else {
         if (tb2_probe) hipLaunchKernelGGL((pf::k_tb3<Real, tb3_r, tb3_wt, false, true>), g, b, 0, s, tp, a1, a2);
         else hipLaunchKernelGGL((pf::k_tb3<Real, tb3_r, tb3_wt, false, false>), g, b, 0, s, tp, a1, a2);
      }
      if (forked) HIPCHK_V(hipStreamWaitEvent(s, ev_src1, 0));
   }
   // The tiles within two cells of a source (tb_srct): k_tb3_src, a handful of workgroups, each a march of one x chunk.  They read the state
   // grids only and write their own tiles' cells: independent of everything else in the pass.
   //   * single domains: forked onto the edge stream BESIDE the box kernel (fork_tb3_src, from launch_tb3 / launch_tb2) and joined behind it.
   //     Their workgroups find every CU taken at first -- a CU holds one workgroup of either kernel, 96 KB of LDS -- and start when the first
   //     round of the main launch has finished: 0.5 ms, nothing beside a 3 ms box kernel.  (Launched first, beside the wall regions instead,
   //     they starve between the regions' waves, 0.6 ms, and hold up the bricks behind them: 773 against 786 Gvox/s.)
   //   * slabs of a chain: 0.5 ms is as long as the slab's whole box kernel, and the edge stream carries the exchange -- Engine::step_begin
   //     launches them FIRST, on the wall regions' second stream, where they finish beside the regions (the rank that holds the source of
   //     an 8-rank chain: 0.250 -> 0.245 ms/step, its neighbours 0.241).
   // n: the step the pass starts at.
   template <int NS> bool fork_tb3_src(hipStream_t s, int64_t n, const Pass &p) {
      if (!src_in_kernel() || tb2_probe || !(op.slab_first && op.slab_last) || s == s_edge) return false;
      HIPCHK_V(hipEventRecord(ev_src0, s)); HIPCHK_V(hipStreamWaitEvent(s_edge, ev_src0, 0));
      launch_tb3_src<NS>(s_edge, n, p);
      HIPCHK_V(hipEventRecord(ev_src1, s_edge));
      return true;
   }
   template <int NS> void launch_tb3_src(hipStream_t se, int64_t n, const Pass &p) {
      if (!src_in_kernel() || tb2_probe) return;
      pf::Tb2Params tp = tile_params(p, NS);
      if (!(op.slab_first && op.slab_last)) tp.band |= 2;
      tp.tiles = tb_srct;
      tp.src_idx = d_in; tp.src_sig = d_insig; tp.nsrc = (int32_t)Ns; tp.src_Nt = Nt;
      tp.src_n = std::min(n, std::max<int64_t>(Nt - NS, 0)); // (the step drivers keep n + NS <= Nt)
      const dim3 g((uint32_t)tb_nsrct), b(64 * tb3_wt);
      if (sg) hipLaunchKernelGGL((pf::k_tb3_src<Real, tb3_r, tb3_wt, true, NS>), g, b, 0, se, tp, a1, a2);
      else hipLaunchKernelGGL((pf::k_tb3_src<Real, tb3_r, tb3_wt, false, NS>), g, b, 0, se, tp, a1, a2);
   }
   // the blocked kernel as the creation-time measurements see it: its four streams, p = of_grids(read, read, written, written) (k_tb3: no u^{n+1} grid)
   void launch_probe(hipStream_t s, int64_t n, const Pass &p, bool sample = false) {
      if (triples() || tb3_geom) launch_tb3(s, n, Pass::of_grids(p.g[0], p.g[1], nullptr, p.g[2], p.g[3]), sample);
      else launch_tb2(s, n, p, sample);
   }
   // two steps of the clean tiles
   void launch_tb2(hipStream_t s, int64_t n, const Pass &p, bool sample = false) {
      if (triples()) { // a pair on the triples' tiles: k_tb3's two-step form (the last two steps of a run, Engine::run)
         if (tb_xr.empty() || tb_nclean <= 0) return;
         pf::Tb2Params tp = tile_params(p, 2);
         const bool forked = fork_tb3_src<2>(s, n, p);
         tp.tiles = tb_clean;
         const dim3 g((uint32_t)tb_nclean), b(64 * tb3_wt);
         if (sg) hipLaunchKernelGGL((pf::k_tb3<Real, tb3_r, tb3_wt, true, false, 2>), g, b, 0, s, tp, a1, a2);
         else hipLaunchKernelGGL((pf::k_tb3<Real, tb3_r, tb3_wt, false, false, 2>), g, b, 0, s, tp, a1, a2);
         if (forked) HIPCHK_V(hipStreamWaitEvent(s, ev_src1, 0));
         return;
      }
      if (tb_xr.empty() || tb_nclean <= 0) return;
      pf::Tb2Params tp = tile_params(p, 2);
      tp.tiles = (tb_ndirty > 0 || tb_order_band) ? tb_clean : nullptr; // all clean: the dense order (identical to the list's)
      sample = sample && tb_sample && tb_nsample > 0;
      if (sample) tp.tiles = tb_sample;
      const dim3 g((uint32_t)(sample ? tb_nsample : tb_nclean)), b(256);
      if (fcc) {
         if (tb_lw == 64) { // 12-row tiles; k_tb2_fcc_w: half the vector arithmetic of k_tb2_fcc_x (debug 0x40000: that one, CPU-exact file order only)
            if ((op.debug & PF_DBG_FCC_PAIR_R4) && !sg && !swz) hipLaunchKernelGGL((pf::k_tb2_fcc_x<Real, 2, 8>), g, dim3(512), 0, s, tp, a1, a2);
            else if (sg) { if (swz) hipLaunchKernelGGL((pf::k_tb2_fcc_w<Real, 2, 8, true, true>), g, dim3(512), 0, s, tp, a1, a2);
                           else hipLaunchKernelGGL((pf::k_tb2_fcc_w<Real, 2, 8, true, false>), g, dim3(512), 0, s, tp, a1, a2); }
            else { if (swz) hipLaunchKernelGGL((pf::k_tb2_fcc_w<Real, 2, 8, false, true>), g, dim3(512), 0, s, tp, a1, a2);
                   else hipLaunchKernelGGL((pf::k_tb2_fcc_w<Real, 2, 8, false, false>), g, dim3(512), 0, s, tp, a1, a2); }
         } else pf::launch_tb2_fcc<Real>(s, tp, a1, a2, tb_lw, (uint32_t)(sample ? tb_nsample : tb_nclean), sg, swz);
         return;
      }
      if (swz) { // axes exchanged in storage (64-lane segments only, init_tb2)
         if (sg) hipLaunchKernelGGL((pf::k_tb2_reg<Real, 3, 4, false, 64, false, true, true>), g, b, 0, s, tp, a1, a2);
         else hipLaunchKernelGGL((pf::k_tb2_reg<Real, 3, 4, false, 64, false, false, true>), g, b, 0, s, tp, a1, a2);
         return;
      }
      if (sg) { // the reference GPU engine's arithmetic (towards-zero pairwise sums, two FMAs)
         if (tb_lw == 32) hipLaunchKernelGGL((pf::k_tb2_reg<Real, 3, 4, false, 32, false, true>), g, b, 0, s, tp, a1, a2);
         else if (tb_lw == 16) hipLaunchKernelGGL((pf::k_tb2_reg<Real, 3, 4, false, 16, false, true>), g, b, 0, s, tp, a1, a2);
         else if (tb2_probe) hipLaunchKernelGGL((pf::k_tb2_reg<Real, 3, 4, false, 64, true, true>), g, b, 0, s, tp, a1, a2);
         else hipLaunchKernelGGL((pf::k_tb2_reg<Real, 3, 4, false, 64, false, true>), g, b, 0, s, tp, a1, a2);
         return;
      }
      if (tb_lw == 32) hipLaunchKernelGGL((pf::k_tb2_reg<Real, 3, 4, false, 32>), g, b, 0, s, tp, a1, a2);
      else if (tb_lw == 16) hipLaunchKernelGGL((pf::k_tb2_reg<Real, 3, 4, false, 16>), g, b, 0, s, tp, a1, a2);
      else if (tb2_probe) hipLaunchKernelGGL((pf::k_tb2_reg<Real, 3, 4, false, 64, true>), g, b, 0, s, tp, a1, a2);
      else hipLaunchKernelGGL((pf::k_tb2_reg<Real, 3, 4, false, 64>), g, b, 0, s, tp, a1, a2);
   }
   // one out-of-place step of the dirty tiles
   void launch_dirty_tiles(hipStream_t s, const Grids &gr) {
      if (tb_xr.empty() || tb_ndirty <= 0) return;
      pf::Tb2Params tp = tile_params();
      tp.A = gr.old; tp.B = gr.cur; tp.C = gr.nxt; tp.D = nullptr;
      tp.tiles = tb_dirty; tp.mask = mask;
      tp.xsub = tb_ndirty <= 256 ? std::min(16, std::max(tb_chunk / 4, 1)) : 1; // few tiles: shorter marches (4 planes), more workgroups
      const dim3 g((uint32_t)tb_ndirty * (uint32_t)tp.xsub), b(256);
      if (fcc) return; // (13-point: k_air_fcc over its own tiling of the box's planes, sh_tiles)
      if (triples() || tb3_geom) { // k_tb3's tiles: 20 rows
         static_assert(tb3_rows == 20, "k_tb1_tile<Real, 5, 4>: 20-row tiles");
         constexpr int HL = pf::VecOf<Real>::V >= 3 ? 1 : 2; // (the tiles' column ranges are k_tb3's)
         if (sg) hipLaunchKernelGGL((pf::k_tb1_tile<Real, 5, 4, 64, true, false, HL>), g, b, 0, s, tp, a1, a2);
         else hipLaunchKernelGGL((pf::k_tb1_tile<Real, 5, 4, 64, false, false, HL>), g, b, 0, s, tp, a1, a2);
         return;
      }
      if (swz) {
         if (sg) hipLaunchKernelGGL((pf::k_tb1_tile<Real, 3, 4, 64, true, true>), g, b, 0, s, tp, a1, a2);
         else hipLaunchKernelGGL((pf::k_tb1_tile<Real, 3, 4, 64, false, true>), g, b, 0, s, tp, a1, a2);
         return;
      }
      if (sg) {
         if (tb_lw == 32) hipLaunchKernelGGL((pf::k_tb1_tile<Real, 3, 4, 32, true>), g, b, 0, s, tp, a1, a2);
         else if (tb_lw == 16) hipLaunchKernelGGL((pf::k_tb1_tile<Real, 3, 4, 16, true>), g, b, 0, s, tp, a1, a2);
         else hipLaunchKernelGGL((pf::k_tb1_tile<Real, 3, 4, 64, true>), g, b, 0, s, tp, a1, a2);
         return;
      }
      if (tb_lw == 32) hipLaunchKernelGGL((pf::k_tb1_tile<Real, 3, 4, 32>), g, b, 0, s, tp, a1, a2);
      else if (tb_lw == 16) hipLaunchKernelGGL((pf::k_tb1_tile<Real, 3, 4, 16>), g, b, 0, s, tp, a1, a2);
      else hipLaunchKernelGGL((pf::k_tb1_tile<Real, 3, 4, 64>), g, b, 0, s, tp, a1, a2);
   }
   // one out-of-place single step of everything outside the box.  strip_u0b: the column strips update their own boundary nodes (zs_map) and leave
   // the node values there (null: every node is the boundary launch's)
   void launch_shell(hipStream_t s, const Grids &g, Real *strip_u0b = nullptr) { launch_shell(s, g, 1, (int)Nx - 1, strip_u0b); }
   // 13-point: ghost flips of u1 in memory, then x slabs (whole planes), column strips, and the single-step tiles of the box
   void launch_shell_fcc(hipStream_t s, const Grids &g, int xlo, int xhi, bool flips) { // planes [xlo, xhi); flips: also the ghost shell of u^n
      if (flips) launch_flips(s, g);
      if (tb_xr.empty()) { launch_air_march(s, g, xlo, xhi); return; }
      if (tbx0 > xlo) launch_air_march(s, g, xlo, tbx0);
      if (tbx1 < xhi) launch_air_march(s, g, tbx1, xhi);
      constexpr int V = pf::VecOf<Real>::V;
      {
         pf::ZStripParams<Real> zp{};
         zp.u1 = g.cur; zp.u0s = g.old; zp.u0 = g.nxt; zp.mask = mask;
         zp.plane = plane; zp.Nx = (int)Nx; zp.Ny = (int)Ny; zp.Nz = (int)Nz; zp.P = (int)P;
         zp.x_begin = tbx0; zp.x_end = tbx1; zp.zl = tbz0; zp.zr = tbz1; zp.first = op.slab_first; zp.last = op.slab_last;
         const int64_t nthreads = (int64_t)(zp.zl / V + (P - zp.zr) / V) * (Ny - 2);
         const int xchunk = 16;
         const dim3 gz((unsigned)cdiv(nthreads, 256), (unsigned)cdiv(tbx1 - tbx0, xchunk));
         if (nthreads > 0) {
            if (sg) { if (swz) hipLaunchKernelGGL((pf::k_zstrip_fcc<Real, true, true>), gz, dim3(256), 0, s, zp, a1, a2, l, xchunk, fold ? 1 : 0);
                      else hipLaunchKernelGGL((pf::k_zstrip_fcc<Real, true, false>), gz, dim3(256), 0, s, zp, a1, a2, l, xchunk, fold ? 1 : 0); }
            else { if (swz) hipLaunchKernelGGL((pf::k_zstrip_fcc<Real, false, true>), gz, dim3(256), 0, s, zp, a1, a2, l, xchunk, fold ? 1 : 0);
                   else hipLaunchKernelGGL((pf::k_zstrip_fcc<Real, false, false>), gz, dim3(256), 0, s, zp, a1, a2, l, xchunk, fold ? 1 : 0); }
         }
      }
      if (sh_ntiles > 0) {
         pf::AirParams ap;
         ap.Ny = Ny; ap.P = P; ap.plane = plane;
         ap.x_begin = tbx0; ap.x_end = tbx1; ap.chunk = tb_chunk; ap.nxc = tb_nxc; ap.nzt = sh_nzt; ap.nyt = sh_nyt;
         ap.swizzle = 0; ap.swz = swz ? 1 : 0;
         ap.Nx = (int)Nx; ap.Nz = (int)Nz; ap.first = op.slab_first; ap.last = op.slab_last; ap.fold = fold ? 1 : 0;
         if (sg) hipLaunchKernelGGL((pf::k_air_fcc<Real, 4, 4, 1, true, true, false, true, 64>), dim3((uint32_t)sh_ntiles), dim3(256), 0, s, g.cur, g.nxt, mask, a1, a2,
                                    ap, l, g.src(), sh_tiles);
         else hipLaunchKernelGGL((pf::k_air_fcc<Real, 4, 4, 1, false, true, false, true, 64>), dim3((uint32_t)sh_ntiles), dim3(256), 0, s, g.cur, g.nxt, mask, a1, a2,
                            ap, l, g.src(), sh_tiles);
      }
      launch_dirty_tiles(s, g);
   }
   // planes [xlo, xhi) without the strips beside the box (slab pairs with wall regions): whole planes outside the box's x range
   // and the box's own single-step tiles
   void launch_shell_planes(hipStream_t s, const Grids &g, int xlo, int xhi, bool tiles = true) {
      int xa = xlo;
      for (auto &r : tb_xr) {
         if (r.first > xa) launch_air_lean(s, g, xa, r.first);
         xa = std::max(xa, r.second);
      }
      if (xhi > xa) launch_air_lean(s, g, xa, xhi);
      if (tiles) launch_dirty_tiles(s, g);
   }
   void launch_shell(hipStream_t s, const Grids &g, int xlo, int xhi, Real *strip_u0b = nullptr) { // planes [xlo, xhi) (the box lies inside)
      if (fcc) { launch_shell_fcc(s, g, xlo, xhi, !tb2_slab); return; } // (slab engines flip on the edge stream, after the exchange)
      int xa = xlo;
      if (tb_xr.size() == 1 && (vbase == 0 || vbase == 40 || vbase == 41) && tb_xr[0].first > xlo && xhi > tb_xr[0].second &&
          tb_xr[0].first - xlo <= 16 && xhi - tb_xr[0].second <= 16) {
         // the usual case: two thin x slabs, below and above the box -- one launch instead of two latency-bound ones
         launch_air_lean(s, g, xlo, tb_xr[0].first, {tb_xr[0].second, xhi});
         xa = xhi;
      }
      for (auto &r : tb_xr) { // x slabs: everything before / between / after the box's plane ranges, full planes
         if (r.first > xa) launch_air_lean(s, g, xa, r.first);
         xa = std::max(xa, r.second);
      }
      if (xhi > xa) launch_air_lean(s, g, xa, xhi);
      if (tb_xr.empty()) return;
      const int xb = tb_xr.front().first, xe = tb_xr.back().second;
      // beside the box: the two row strips in one lean launch (tile height of the default configuration: 16 rows) ...
      const int th = 8; // lean<2,4>: 8-row tiles (the strips are 5-7 rows thick in a box-shaped room)
      launch_lean_cfg<2, 4>(s, g, xb, xe, {0, 0, (int)cdiv(tby0 - 1, th), (tby1 - 1) / th});
      // ... and the two column strips
      {
         constexpr int V = pf::VecOf<Real>::V;
         pf::ZStripParams<Real> zp{};
         zp.u1 = g.cur; zp.u0s = g.old; zp.u0 = g.nxt; zp.mask = mask;
         zp.plane = plane; zp.Nx = (int)Nx; zp.Ny = (int)Ny; zp.Nz = (int)Nz; zp.P = (int)P;
         zp.x_begin = xb; zp.x_end = xe; zp.zl = szl; zp.zr = szr; zp.first = op.slab_first; zp.last = op.slab_last;
         if (zs_map && strip_u0b) { // (inside step_pair) the strips' boundary nodes are updated right here
            zp.zvec = zs_map; zp.adjv = zs_adj; zp.lossy = zs_li; zp.u0b = strip_u0b; zp.sl2 = sl2;
         }
         const int64_t nthreads = (int64_t)(zp.zl / V + (P - zp.zr) / V) * (Ny - 2);
         const int xchunk = 16;
         const dim3 gz((unsigned)cdiv(nthreads, 256), (unsigned)cdiv(xe - xb, xchunk));
         if (swz) { if (sg) hipLaunchKernelGGL((pf::k_air_zstrip<Real, true, true>), gz, dim3(256), 0, s, zp, a1, a2, l, xchunk);
                    else hipLaunchKernelGGL((pf::k_air_zstrip<Real, false, true>), gz, dim3(256), 0, s, zp, a1, a2, l, xchunk); }
         else if (sg) hipLaunchKernelGGL((pf::k_air_zstrip<Real, true>), gz, dim3(256), 0, s, zp, a1, a2, l, xchunk);
         else hipLaunchKernelGGL((pf::k_air_zstrip<Real, false>), gz, dim3(256), 0, s, zp, a1, a2, l, xchunk);
      }
      launch_dirty_tiles(s, g); // ... and the tiles of the box that hold geometry or a source
   }
   // ------------------------------------------------------------------------------------------------------------
   void launch_air(hipStream_t s, const Grids &g, int xb, int xe) {
      if (xe <= xb) return;
      EvPair ev{};
      if (op.timing) { ev = ev_get(); hipEventRecord(ev.first, s); }
      if (lean) launch_air_lean(s, g, xb, xe);
      else launch_air_march(s, g, xb, xe);
      if (op.timing) { hipEventRecord(ev.second, s); air_ev.push_back(ev); }
   }

   // x-chunk length of the marching kernels.  op.air_chunk > 0: that many planes; < 0: -air_chunk equal chunks;
   // 0: automatic, from sweeps on MI355X (tools/tune_air.py --chunks=-2,-4,...; 1024^3, 512^3, 256^3, 1/2..1/8 slabs):
   //   lean kernels (lean=true): ~64-plane chunks, but between 512 and 2048 workgroups in total -- fewer starve the
   //   CUs, more only add 2-plane prologues; barrier-free v1 kernels: ~12k workgroups, chunks of >= 6 planes.
   // The split is always even (a short last chunk idles its XCD at the end) and the chunk count even (XCD swizzle).
   int pick_chunk(int nplanes, int64_t tiles, bool lean_rule) const {
      int chunk = op.air_chunk;
      if (chunk < 0) chunk = (int)cdiv(nplanes, std::min<int64_t>(-(int64_t)chunk, nplanes));
      else if (chunk == 0) {
         tiles = std::max<int64_t>(tiles, 1);
         int64_t n;
         if (lean_rule) {
            // slab engines keep >= 1024 WGs: with fewer, every WG is resident for the whole launch and the edge-stream
            // kernels / the RCCL transfer kernel find no free CU slot until the interior launch has finished
            const bool slab = !(op.slab_first && op.slab_last);
            const int64_t lo = cdiv(slab ? 1024 : 512, tiles), hi = std::max(cdiv(2048, tiles), lo);
            n = std::min(std::max<int64_t>(nplanes / 64, lo), hi);
         } else {
            n = std::min<int64_t>(cdiv(256 * 48, tiles), std::max(nplanes / 6, 1));
         }
         if (n > 1 && (n & 1)) n++;
         n = std::max<int64_t>(1, std::min<int64_t>(n, nplanes));
         chunk = (int)cdiv(nplanes, n);
      }
      return std::max(1, std::min(chunk, nplanes));
   }

   // Lanes per row segment of the barrier-free kernels: 64 lanes x 16 B = 1 KiB of z per wave row wastes lanes on narrow
   // grids (Nz=309 -> pitch 320: two 256-column segments, 62 % used).  With 32 or 16 lanes per segment a wave stacks 2 or
   // 4 segments in y instead; pick the width with the least padding (ties: the widest).
   int pick_lw() const {
      constexpr int V = pf::VecOf<Real>::V;
      if (op.debug & (PF_DBG_LW32 | PF_DBG_LW16)) return (op.debug & PF_DBG_LW32) ? 32 : 16; // tuning override
      if (lw_force) return lw_force;                             // measured at creation (autotune)
      // narrower segments cost extra edge-column loads (two per segment and row; the 13-point kernel needs them on every
      // row of all three planes): worth it only when they save >= 10 % of the padded width (7-point) / 25 % (13-point);
      // measured: Nz=309 7-pt +10 % with 16 lanes, Nz=850 13-pt -4 % with 32 lanes
      const int64_t w64 = cdiv(P, (int64_t)64 * V) * 64 * V;
      const double need = fcc ? 0.75 : 0.90;
      int best = 64;
      int64_t best_w = w64;
      for (int lw : {32, 16}) {
         const int64_t w = cdiv(P, (int64_t)lw * V) * lw * V;
         if (w < best_w && (double)w <= need * (double)w64) { best_w = w; best = lw; }
      }
      return best;
   }
   // tile order of the marching kernels: 2 = XCD-banded inside every x chunk (pf_kernels.h: xcd_band), 1 = one contiguous run
   // of the launch per XCD (round 1), 0 = plain (air_variant | 64); PFFDTD_SWIZZLE overrides for measurements
   // Banded wins on large planes (1024^2: k_air_fcc 2.46 -> 2.32 ms, barrier-free 7-point 2.45 -> 2.29, lean 2.33 -> 2.28;
   // Musikverein 552 x 850: 3.60 -> 3.44), the per-XCD run on small ones, where a whole chunk of planes fits one L2 and a band
   // is a handful of tiles (CTK church 579 x 309, 50 tiles per chunk: 0.392 vs 0.425 ms): banded from 96 tiles per chunk.
   int swizzle_mode(int64_t tiles_per_chunk) const { return order_force >= 0 ? order_force : (tiles_per_chunk >= 96 ? 2 : 1); }
   static uint32_t grid_blocks(int swz, int nzt, int nyt, int nxc) {
      return swz == 2 ? pf::xcd_band_blocks((uint32_t)nzt * nyt, (uint32_t)nxc) : (uint32_t)nzt * nyt * nxc;
   }
   // the barrier-free marching kernels (pf_kernels.h): R = 4 rows per lane, 4 waves stacked in y
   void launch_air_march(hipStream_t s, const Grids &g, int xb, int xe) {
      const int lw = (op.debug & PF_DBG_LW64) ? 64 : pick_lw();
      if (lw == 32) launch_march_lw<32>(s, g, xb, xe);
      else if (lw == 16) launch_march_lw<16>(s, g, xb, xe);
      else launch_march_lw<64>(s, g, xb, xe);
   }
   template <int LW> void launch_march_lw(hipStream_t s, const Grids &gr, int xb, int xe) {
      constexpr int V = pf::VecOf<Real>::V, R = 4, WY = 4, WZ = 1;
      pf::AirParams ap;
      ap.Ny = Ny; ap.P = P; ap.plane = plane;
      ap.x_begin = xb; ap.x_end = xe;
      ap.nzt = (int)cdiv(P, (int64_t)WZ * LW * V);
      ap.nyt = (int)cdiv(Ny - 2, (int64_t)WY * R * (64 / LW));
      const int nplanes = xe - xb;
      const int chunk = pick_chunk(nplanes, (int64_t)ap.nzt * ap.nyt, false);
      ap.chunk = chunk;
      ap.nxc = (int)cdiv(nplanes, chunk);
      ap.swizzle = swizzle_mode((int64_t)ap.nzt * ap.nyt);
      ap.Nx = (int)Nx; ap.Nz = (int)Nz; ap.first = op.slab_first; ap.last = op.slab_last; ap.fold = fold ? 1 : 0;
      ap.swz = swz ? 1 : 0;
      const uint32_t total = grid_blocks(ap.swizzle, ap.nzt, ap.nyt, ap.nxc);
      dim3 g(total), b(64 * WY * WZ);
      if (vg && !fcc && !gr.in_place()) { // autotune alone: the 7-point kernel writing to a scratch grid (it reads u^{n-1} where it would write in place)
         hipLaunchKernelGGL((pf::k_air_cart<Real, R, WY, WZ, false, true, true, false, LW>), g, b, 0, s, gr.cur, gr.old, mask, a1, a2, ap, l, gr.nxt);
         return;
      }
      if (fcc && abck && !gr.in_place()) { // out of place (shell of a temporally blocked pair, creation-time measurement)
         if (sg) hipLaunchKernelGGL((pf::k_air_fcc<Real, R, WY, WZ, true, true, false, true, LW>), g, b, 0, s, gr.cur, gr.nxt, mask, a1, a2, ap, l, gr.old, (const int32_t *)nullptr);
         else hipLaunchKernelGGL((pf::k_air_fcc<Real, R, WY, WZ, false, true, false, true, LW>), g, b, 0, s, gr.cur, gr.nxt, mask, a1, a2, ap, l, gr.old, (const int32_t *)nullptr);
         return;
      }
#define PF_LAUNCH(K, SG) do { if (vg) hipLaunchKernelGGL((K<Real, R, WY, WZ, SG, true, true, false, LW>), g, b, 0, s, gr.cur, gr.nxt, mask, a1, a2, ap, l); \
                              else if (abck) hipLaunchKernelGGL((K<Real, R, WY, WZ, SG, true, false, true, LW>), g, b, 0, s, gr.cur, gr.nxt, mask, a1, a2, ap, l); \
                              else hipLaunchKernelGGL((K<Real, R, WY, WZ, SG, true, false, false, LW>), g, b, 0, s, gr.cur, gr.nxt, mask, a1, a2, ap, l); } while (0)
      if (fcc) { if (sg) PF_LAUNCH(pf::k_air_fcc, true); else PF_LAUNCH(pf::k_air_fcc, false); }
      else { if (sg) PF_LAUNCH(pf::k_air_cart, true); else PF_LAUNCH(pf::k_air_cart, false); }
#undef PF_LAUNCH
   }

   // the lean fused 7-point kernel (pf_air_fused.h).  R x WY = rows per lane x waves per workgroup; NT = nontemporal u0 traffic
   template <int R, int WY, bool NT = true> void launch_lean_cfg(hipStream_t s, const Grids &g, int xb, int xe, LeanExtra ex = {}) {
      pf::LeanParams fp{};
      fp.u1 = g.cur; fp.u0 = g.nxt; fp.mask = mask;
      fp.plane = plane;
      fp.Nx = (int)Nx; fp.Ny = (int)Ny; fp.Nz = (int)Nz; fp.P = (int)P;
      fp.x_begin = xb; fp.x_end = xe;
      fp.nzt = lean_nzt;
      fp.nyt = (int)cdiv(Ny - 2, (int64_t)WY * R);
      fp.u0_src = g.src(); fp.yt0 = 0; fp.yt_split = -1; fp.yt_hi0 = 0;
      // (row strips of a triple's third step: the strips' tiles reach into the box, whose u^{n+1} -- the step's old value -- is not in
      // memory: those rows are left to k_tb3's own result)
      if (ex.nyt >= 0 && triples()) { fp.skip_y0 = tby0; fp.skip_y1 = tby1; }
      if (ex.nyt >= 0) { // row strips: tiles [0, ex.nyt) and [ex.yt0, all) in units of this configuration's tile height
         const int all = fp.nyt, lo = std::min(ex.nyt, all), hi0 = std::max(std::min(ex.yt0, all), lo);
         fp.yt_split = lo; fp.yt_hi0 = hi0;
         fp.nyt = lo + (all - hi0);
         if (fp.nyt <= 0) return;
      }
      const int nplanes = xe - xb;
      int chunk = pick_chunk(nplanes, (int64_t)fp.nzt * fp.nyt, true);
      fp.chunk = chunk;
      fp.nxc = (int)cdiv(nplanes, chunk);
      if (ex.x2_end > ex.x2_begin) { // a second x slab [ex.x2_begin, ex.x2_end) in the same launch (both thin: one chunk each)
         chunk = std::max(nplanes, ex.x2_end - ex.x2_begin);
         fp.chunk = chunk;
         fp.x_lo_end = xe; fp.x2_begin = ex.x2_begin; fp.x_end = ex.x2_end;
         fp.x2_nlo = 1; fp.nxc = 2;
      }
      fp.swizzle = swizzle_mode((int64_t)fp.nzt * fp.nyt);
      fp.first = op.slab_first; fp.last = op.slab_last;
      fp.do_abc = 1;
      fp.swz = swz ? 1 : 0;
      dim3 gd(grid_blocks(fp.swizzle, fp.nzt, fp.nyt, fp.nxc)), b(64 * WY);
      if (sg) hipLaunchKernelGGL((pf::k_air_cart_lean<Real, R, WY, true, NT>), gd, b, 0, s, fp, a1, a2, l);
      else hipLaunchKernelGGL((pf::k_air_cart_lean<Real, R, WY, false, NT>), gd, b, 0, s, fp, a1, a2, l);
   }
   void launch_air_lean(hipStream_t s, const Grids &g, int xb, int xe, LeanExtra ex = {}) {
      // fastest measured on MI355X: fp32 R = 4 x 4 waves, fp64 R = 2 x 8 waves (register budget)
      if (sizeof(Real) == 8) launch_lean_cfg<2, 8>(s, g, xb, xe, ex);
      else launch_lean_cfg<4, 4>(s, g, xb, xe, ex);
   }

   void launch_pre(hipStream_t s, const Grids &g) {
      if (lean || vg) return; // ghost shell is virtual, u2ba is the old u0 in registers
      launch_flips(s, g);
      if (Nba && !abck) hipLaunchKernelGGL(pf::k_abc_save<Real>, dim3((unsigned)cdiv(Nba, 256)), dim3(256), 0, s, g.old, d_bna, u2ba, Nba);
   }
   void launch_flips(hipStream_t s, const Grids &g) {
      dim3 gy((unsigned)cdiv(Nz, 256), (unsigned)Nx);
      if (fold) hipLaunchKernelGGL(pf::k_flip_y<Real>, gy, dim3(256), 0, s, g.cur, Nx, Ny, P, Nz, 4);
      hipLaunchKernelGGL(pf::k_flip_z<Real>, dim3((unsigned)cdiv(Nx * Ny, 256)), dim3(256), 0, s, g.cur, Nx * Ny, P, Nz);
      hipLaunchKernelGGL(pf::k_flip_y<Real>, gy, dim3(256), 0, s, g.cur, Nx, Ny, P, Nz, fold ? 1 : 3);
      if (op.slab_first || op.slab_last)
         hipLaunchKernelGGL(pf::k_flip_x<Real>, dim3((unsigned)cdiv(plane, 256)), dim3(256), 0, s, g.cur, Nx, plane, op.slab_first, op.slab_last);
   }
   void launch_abc(hipStream_t s, const Grids &g, Range r) {
      if (lean || vg || abck || r.e <= r.b) return;
      if (sg) hipLaunchKernelGGL((pf::k_abc_loss<Real, true>), dim3((unsigned)cdiv(r.e - r.b, 256)), dim3(256), 0, s, g.nxt, d_bna, d_Q, u2ba, l, r.b, r.e);
      else hipLaunchKernelGGL((pf::k_abc_loss<Real, false>), dim3((unsigned)cdiv(r.e - r.b, 256)), dim3(256), 0, s, g.nxt, d_bna, d_Q, u2ba, l, r.b, r.e);
   }
   // Virtual-ghost modes: boundary nodes next to the folded ghost row read it from MEMORY, so that one row is kept
   // materialised.  In a split-phase step the main stream only touches planes [1, Nx-1): the slab's ghost planes may
   // be receiving the neighbours' data at that moment (the edge stream, ordered after the exchange, does those).
   void launch_fold_row(hipStream_t s, const Grids &g, const Bnd &bn) { // planes [bn.fold_b, bn.fold_e)
      if (!((lean || vg) && fold && need_fold_row) || bn.fold_e <= bn.fold_b) return;
      dim3 gy((unsigned)cdiv(Nz, 256), (unsigned)(bn.fold_e - bn.fold_b));
      hipLaunchKernelGGL(pf::k_flip_y<Real>, gy, dim3(256), 0, s, g.cur + (int64_t)bn.fold_b * plane, (int64_t)(bn.fold_e - bn.fold_b), Ny, P, Nz, 4);
   }
   // rigid + FD in one pass over the boundary list (plane range given on the boundary list)
   void launch_boundary(hipStream_t s, const Grids &gr, const Bnd &bn, Range r, bool strips_fd) {
      // strips_fd (inside step_pair, bn.sel = zs_rest): the branch ODEs of the column strips' lossy nodes ride along in the same launch (k_fd_sel's work)
      // (a launch of its own, k_fd_sel, until round 3: same time within noise, one kernel fewer)
      const bool with_fd = strips_fd && zs_mode == 2 && zs_nfd > 0 && r.b == 0 && r.e == zs_nrest;
      if (r.e <= r.b && !with_fd) return;
      launch_fold_row(s, gr, bn);
      const int64_t nfd = with_fd ? zs_nfd : 0;
      dim3 g((unsigned)cdiv(r.e - r.b + nfd, 128)), b(128);
#define PF_BND(F, M) hipLaunchKernelGGL((pf::k_boundary<Real, F, M>), g, b, 0, s, gr.cur, gr.nxt, d_bn, d_adj, d_lossy, a2, sl2, P, plane, bn.u0b, bn.u2b, d_ssaf, d_mat, d_Mb, d_mq, d_beta, bn.in.v, bn.in.g, bn.out.v, bn.out.g, lo2, (int64_t)mb_max, r.b, r.e, (const Real *)gr.old, bn.sel, swz ? 1 : 0, with_fd ? zs_fd : (const int32_t *)nullptr, nfd, d_bnl, bflags)
      // Each XCD walks runs of 64 consecutive workgroups
      // (8192 nodes, a few node rows) inside a window of 512, so most rows of u^n that consecutive node rows share are asked
      // for by ONE L2: fetched bytes 4.53 -> 3.7 GB on the Musikverein, 0.79-0.81 -> 0.75-0.76 ms (CTK 0.150 -> 0.141).
      // One run per XCD over the whole list fetches least (3.36 GB) and is slowest (0.90 ms: eight places in every stream);
      // profiles/r04_rooms_hbm_traffic.md.  (Box rooms in single steps: 1024^3 384 -> 388 Gvox/s; slabs: the same.)
      // PF_DBG_BND_PLAIN_ORDER: plain order; PF_DBG_BND_FETCH_ALL: fetch the neighbours inside the wall too.
      const int bnd_g = 64;
      const int bflags = ((!(op.debug & PF_DBG_BND_PLAIN_ORDER)) ? (1 | (bnd_g << 4)) : 0) | ((op.debug & PF_DBG_BND_FETCH_ALL) ? 2 : 0);
      if (fcc) { if (sg) PF_BND(true, true); else PF_BND(true, false); }
      else { if (sg) PF_BND(false, true); else PF_BND(false, false); }
#undef PF_BND
   }
   bool boundary_fused() const { return fuse_boundary; }
   void launch_rigid(hipStream_t s, const Grids &gr, const Bnd &bn, Range r, bool strips_fd = false) {
      if (boundary_fused()) { launch_boundary(s, gr, bn, r, strips_fd); return; }
      if (r.e <= r.b) return;
      launch_fold_row(s, gr, bn);
      dim3 g((unsigned)cdiv(r.e - r.b, 256)), b(256);
      if (fcc) {
         if (sg) hipLaunchKernelGGL((pf::k_rigid<Real, true, true>), g, b, 0, s, gr.cur, gr.nxt, d_bn, d_adj, a2, sl2, P, plane, r.b, r.e, swz ? 1 : 0);
         else hipLaunchKernelGGL((pf::k_rigid<Real, true, false>), g, b, 0, s, gr.cur, gr.nxt, d_bn, d_adj, a2, sl2, P, plane, r.b, r.e, swz ? 1 : 0);
      } else {
         if (sg) hipLaunchKernelGGL((pf::k_rigid<Real, false, true>), g, b, 0, s, gr.cur, gr.nxt, d_bn, d_adj, a2, sl2, P, plane, r.b, r.e, swz ? 1 : 0);
         else hipLaunchKernelGGL((pf::k_rigid<Real, false, false>), g, b, 0, s, gr.cur, gr.nxt, d_bn, d_adj, a2, sl2, P, plane, r.b, r.e, swz ? 1 : 0);
      }
   }
   void launch_fd(hipStream_t s, const Grids &g, const Bnd &bn, Range r) {
      if (boundary_fused()) return; // done by launch_boundary
      if (r.e > r.b)
         hipLaunchKernelGGL(pf::k_fd_boundary<Real>, dim3((unsigned)cdiv(r.e - r.b, 128)), dim3(128), 0, s, g.nxt, d_bnl, bn.u0b, bn.u2b, d_ssaf, d_mat, d_Mb, d_mq, d_beta, bn.in.v, bn.in.g, lo2, (int64_t)mb_max, r.b, r.e);
   }
   // receivers on/off + a range of the (sorted) source list
   void launch_io(hipStream_t s, const Grids &g, int64_t n, bool receivers, Range src, const int64_t *ctr = nullptr, const Real *u_next = nullptr) {
      const int64_t nr = receivers ? Nr : 0;
      const int64_t ns = src.e - src.b;
      if (nr == 0 && ns <= 0) return;
      // (u_next: the field the NEXT step's readout reads, taken in the same launch into the next ring column -- no sources then)
      hipLaunchKernelGGL(pf::k_io<Real>, dim3((unsigned)cdiv(nr + 1, 128)), dim3(128), 0, s, g.cur, g.nxt, d_out, ring, nr, ring_fill, ring_depth,
                         d_in + src.b, d_insig + src.b * Nt, std::max<int64_t>(ns, 0), Nt, n, ctr, u_next);
   }
