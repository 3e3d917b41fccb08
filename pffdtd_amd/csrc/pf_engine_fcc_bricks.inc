// pf_engine_fcc_bricks.inc -- part of `template <typename Real> struct Engine` (pf_engine.hip includes it INSIDE the class body; not a translation unit):
// 13-point blocked pairs with the whole shell in bricks (air_variant 42): tables (Engine::init_fcc_bricks: pf_fcc_shell_cut.h), launches of
// k_brick_fcc (pf_brick_fcc.h) and of the box's single-step tiles, Engine::step_pair_fcc_bricks.
   bool fb_want = false, fb_on = false;                   // air_variant 42 asked for / its tables stand
   pf_fcc::Brick *fb_brk = nullptr;
   uint16_t *fb_info = nullptr;                           // per cell of a brick's extended box: pf_fcc::INFO_*
   pf_fcc::Node *fb_los = nullptr;                        // per frequency-dependent node of a brick: cell | owned << 31, place in the lossy arrays
   int32_t *fb_rest = nullptr;                            // boundary nodes no brick owns (inside the box): the list kernel's
   int32_t *fb_tiles = nullptr;                           // k_air_fcc's tiles (sh_nyt x sh_nzt per x chunk) that hold a cell of a single-step tile of the box
   int64_t fb_nbrk = 0, fb_nrest = 0, fb_ntiles = 0;
   size_t fb_lds = 0;
   void free_fcc_bricks() {
      mem.release(fb_brk); mem.release(fb_info); mem.release(fb_los); mem.release(fb_rest); mem.release(fb_tiles);
      fb_nbrk = fb_nrest = fb_ntiles = 0; fb_lds = 0; fb_on = false;
   }
   // what air_variant 42 needs beyond 40, checked before anything is built (init): a folded 13-point grid, a single domain, file order
   int check_fcc_bricks() const {
      if (!fold) return set_err(PF_ERR_ARG, "air_variant 42 (13-point pairs with the shell in bricks): the scene is not a folded FCC grid (fcc_flag 2)");
      if (!(op.slab_first && op.slab_last)) return set_err(PF_ERR_ARG, "air_variant 42 (13-point pairs with the shell in bricks): not for a slab of a chain");
      if (swz) return set_err(PF_ERR_ARG, "air_variant 42 (13-point pairs with the shell in bricks): not with the axes exchanged in storage (PF_LAYOUT_EXCHANGED)");
      return PF_OK;
   }
   // LDS a brick may take: four workgroups per CU in fp32, two in fp64 (160 KiB per CU)
   static constexpr size_t fb_lds_max = sizeof(Real) == 4 ? 40 * 1024 : 64 * 1024;
   int init_fcc_bricks() {
      fb_on = false;
      if (!tb2 || tb_xr.empty() || tb_nclean <= 0 || !bufC || !bufD)
         return set_err(PF_ERR_ARG, "air_variant 42 (13-point pairs with the shell in bricks): the scene has no blocked pairs to build on (no boundary-free tiles, no room for two more grids, or the boundary pass is not fused)");
      if (Nbl >= ((int64_t)1 << 31) || Nb >= ((int64_t)1 << 31)) return set_err(PF_ERR_ARG, "air_variant 42 (13-point pairs with the shell in bricks): too many boundary nodes");
      std::vector<int64_t> hb(Nb), hbna(Nba), hsrc(Ns);
      std::vector<uint16_t> hadj(Nb);
      std::vector<int32_t> hl(Nb, -1);
      std::vector<int8_t> hq(Nba);
      if (Nb) {
         HIPCHK(hipMemcpy(hb.data(), d_bn, Nb * sizeof(int64_t), hipMemcpyDeviceToHost));
         HIPCHK(hipMemcpy(hadj.data(), d_adj, Nb * sizeof(uint16_t), hipMemcpyDeviceToHost));
         if (d_lossy) HIPCHK(hipMemcpy(hl.data(), d_lossy, Nb * sizeof(int32_t), hipMemcpyDeviceToHost));
      }
      if (Nba) {
         HIPCHK(hipMemcpy(hbna.data(), d_bna, Nba * sizeof(int64_t), hipMemcpyDeviceToHost));
         HIPCHK(hipMemcpy(hq.data(), d_Q, Nba * sizeof(int8_t), hipMemcpyDeviceToHost));
      }
      for (int64_t i = 0; i < Ns; i++) hsrc[i] = pad_idx(sd.in_ixyz[i]);
      pf_fcc::Scene sc{};
      sc.N[0] = Nx; sc.N[1] = Ny; sc.N[2] = Nz; sc.sx = plane; sc.sy = P;
      sc.box0[0] = tbx0; sc.box0[1] = tby0; sc.box0[2] = tbz0; sc.box1[0] = tbx1; sc.box1[1] = tby1; sc.box1[2] = tbz1;
      sc.Nb = Nb; sc.bn = hb.data(); sc.adj = hadj.data(); sc.lossy = hl.data();
      sc.Nba = Nba; sc.bna = hbna.data(); sc.Q = hq.data();
      sc.Ns = Ns; sc.src = hsrc.data();
      sc.ns = 2; sc.real_bytes = (int)sizeof(Real); sc.nmat = (int)sd.Nm; sc.lds_max = fb_lds_max;
      sc.max_nodes = pf::BRICK_T * (pf::wall_mc(mb_max) == pf::WALL_MC[0] ? pf::brick_fcc_kn<Real, pf::WALL_MC[0]>() : pf::brick_fcc_kn<Real, pf::WALL_MC[1]>());
      pf_fcc::Cut cut;
      const std::string why = pf_fcc::cut_shell(sc, cut);
      if (!why.empty()) return set_err(PF_ERR_ARG, "air_variant 42 (13-point pairs with the shell in bricks): %s", why.c_str());
      // k_air_fcc's tiles over the box's planes that hold a cell of a single-step tile of the box (the row strips are the bricks')
      std::vector<int32_t> tl;
      if (tb_ndirty > 0) {
         constexpr int V = pf::VecOf<Real>::V;
         const int TC = (tb_lw - 2) * V, TR = (tb_lw == 64 && fcc_wt) ? 2 * (fcc_wt - 2) : 8 * (64 / tb_lw); // (init_tb2_impl's pair tiles)
         // (the two tilings are init_tb2_impl's and k_air_fcc's: should either change, say so instead of listing the wrong tiles)
         if (cdiv(tby1 - tby0, TR) != tb_nyt || cdiv(tbz1 - tbz0, TC) != tb_nzt || sh_nyt != (int)cdiv(Ny - 2, 16) || sh_nzt != (int)cdiv(P, 64 * V))
            return set_err(PF_ERR_STATE, "air_variant 42: the box's tiles are not the %d x %d rows x columns this list assumes", TR, TC);
         std::vector<int32_t> di((size_t)tb_ndirty);
         HIPCHK(hipMemcpy(di.data(), tb_dirty, tb_ndirty * sizeof(int32_t), hipMemcpyDeviceToHost));
         std::vector<uint8_t> dirty((size_t)tb_nxc * tb_nyt * tb_nzt, 0);
         for (int32_t t : di) dirty[(size_t)t] = 1;
         for (int xc = 0; xc < tb_nxc; xc++)
            for (int yt = 0; yt < sh_nyt; yt++)
               for (int zt = 0; zt < sh_nzt; zt++) {
                  const int ya = std::max(1 + yt * 16, tby0), yb = std::min(1 + yt * 16 + 16, tby1);
                  const int za = std::max(zt * 64 * V, tbz0), zb = std::min((zt + 1) * 64 * V, tbz1);
                  if (ya >= yb || za >= zb) continue;
                  bool need = false;
                  for (int a = (ya - tby0) / TR; a <= (yb - 1 - tby0) / TR && !need; a++)
                     for (int c = (za - tbz0) / TC; c <= (zb - 1 - tbz0) / TC && !need; c++) need = dirty[((size_t)xc * tb_nyt + a) * tb_nzt + c] != 0;
                  if (need) tl.push_back((int32_t)(((int64_t)xc * sh_nyt + yt) * sh_nzt + zt));
               }
      }
      free_fcc_bricks();
      int rc;
      // the second copy of the branch state and a fourth node-value buffer: a pass never writes a buffer anybody reads during it
      if (!vh1b && (rc = dzalloc(&vh1b, round_up(Nbl, 64) * PF_MMB))) return rc;
      if (!gh1b && (rc = dzalloc(&gh1b, round_up(Nbl, 64) * PF_MMB))) return rc;
      if (!ubx[0] && (rc = dzalloc(&ubx[0], std::max<int64_t>(Nbl, 1)))) return rc;
      if ((rc = upload(&fb_brk, cut.brk.data(), (int64_t)cut.brk.size()))) return rc;
      if ((rc = upload(&fb_info, cut.info.data(), (int64_t)cut.info.size()))) return rc;
      if ((rc = upload(&fb_los, cut.los.data(), (int64_t)cut.los.size()))) return rc;
      fb_nrest = (int64_t)cut.rest.size();
      if ((rc = upload(&fb_rest, cut.rest.data(), fb_nrest))) return rc;
      fb_ntiles = (int64_t)tl.size();
      if ((rc = upload(&fb_tiles, tl.data(), fb_ntiles))) return rc;
      fb_nbrk = (int64_t)cut.brk.size(); fb_lds = cut.lds;
      fb_on = true;
      if (getenv("PFFDTD_VERBOSE") && atoi(getenv("PFFDTD_VERBOSE")) > 0)
         fprintf(stderr, "pffdtd_hip: 13-point shell in bricks: box x [%d,%d) y [%d,%d) z [%d,%d), %ld bricks (%zu cells with their halos, %zu bytes of LDS at most), owned boxes x slabs %dx%dx%d, row strips %dx%dx%d / %dx%dx%d, column strips %dx%dx%d / %dx%dx%d; %ld frequency-dependent nodes owned, %ld of %ld boundary nodes left to the list kernel, %ld single-step tiles\n",
                 tbx0, tbx1, tby0, tby1, tbz0, tbz1, (long)fb_nbrk, cut.info.size(), fb_lds, cut.tile[0][0], cut.tile[0][1], cut.tile[0][2], cut.tile[2][0], cut.tile[2][1], cut.tile[2][2],
                 cut.tile[3][0], cut.tile[3][1], cut.tile[3][2], cut.tile[4][0], cut.tile[4][1], cut.tile[4][2], cut.tile[5][0], cut.tile[5][1], cut.tile[5][2], (long)cut.nodes_owned, (long)fb_nrest, (long)Nb, (long)fb_ntiles);
      return PF_OK;
   }
   // the bricks, both steps from step `first` of the pass: windows as in launch_walls_x -- the node values of the steps go to buffers nobody reads during the pass
   void launch_fcc_bricks(hipStream_t s, const Pass &p, int first, int ns) {
      if (!fb_nbrk) return;
      pf::BrickFccParams<Real> bp{};
      bp.A = p.g[first]; bp.B = p.g[first + 1]; bp.x2 = p.x[first]; bp.x1 = p.x[first + 1];
      for (int j = 0; j < 2; j++) { bp.G[j] = p.out_g(first, ns, j); bp.O[j] = p.out_x(first, ns, j); }
      bp.plane = plane; bp.Nx = (int)Nx; bp.Ny = (int)Ny; bp.Nz = (int)Nz; bp.P = (int)P;
      bp.brk = fb_brk; bp.info = fb_info; bp.los = fb_los;
      bp.sv_in = p.in(first).v; bp.sg_in = p.in(first).g; bp.sv_out = p.s1.v; bp.sg_out = p.s1.g;
      bp.ssaf = d_ssaf; bp.mat = d_mat; bp.Mb = d_Mb; bp.mq = d_mq; bp.beta = d_beta;
      bp.lo2 = lo2; bp.sl2 = sl2; bp.l = l; bp.nmat = (int)sd.Nm; bp.ns = ns;
      const dim3 g((unsigned)fb_nbrk), b(pf::BRICK_T);
      const bool lo = pf::wall_mc(mb_max) == pf::WALL_MC[0];
      if (lo && sg) hipLaunchKernelGGL((pf::k_brick_fcc<Real, pf::WALL_MC[0], true>), g, b, fb_lds, s, bp, a1, a2);
      else if (lo) hipLaunchKernelGGL((pf::k_brick_fcc<Real, pf::WALL_MC[0], false>), g, b, fb_lds, s, bp, a1, a2);
      else if (sg) hipLaunchKernelGGL((pf::k_brick_fcc<Real, pf::WALL_MC[1], true>), g, b, fb_lds, s, bp, a1, a2);
      else hipLaunchKernelGGL((pf::k_brick_fcc<Real, pf::WALL_MC[1], false>), g, b, fb_lds, s, bp, a1, a2);
   }
   // one out-of-place step of the box's single-step tiles, by k_air_fcc over its own tiles -- which store their cells
   // of the box and no others (the cells around it are the bricks'; the tile's rows next to a ghost row are computed from whatever lies there)
   void launch_box_tiles_fcc(hipStream_t s, const Grids &g) {
      if (fb_ntiles <= 0) return;
      pf::AirParams ap;
      ap.Ny = Ny; ap.P = P; ap.plane = plane;
      ap.x_begin = tbx0; ap.x_end = tbx1; ap.chunk = tb_chunk; ap.nxc = tb_nxc; ap.nzt = sh_nzt; ap.nyt = sh_nyt;
      ap.swizzle = 0; ap.swz = 0;
      ap.Nx = (int)Nx; ap.Nz = (int)Nz; ap.first = op.slab_first; ap.last = op.slab_last; ap.fold = fold ? 1 : 0;
      ap.cy0 = tby0; ap.cy1 = tby1; ap.cz0 = tbz0; ap.cz1 = tbz1;
      if (sg) hipLaunchKernelGGL((pf::k_air_fcc<Real, 4, 4, 1, true, true, false, true, 64, true>), dim3((uint32_t)fb_ntiles), dim3(256), 0, s, g.cur, g.nxt, mask, a1, a2, ap, l, g.src(), fb_tiles);
      else hipLaunchKernelGGL((pf::k_air_fcc<Real, 4, 4, 1, false, true, false, true, 64, true>), dim3((uint32_t)fb_ntiles), dim3(256), 0, s, g.cur, g.nxt, mask, a1, a2, ap, l, g.src(), fb_tiles);
   }
   // steps n and n+1 of a 13-point engine whose shell is in bricks.  Order: the first step of what no brick owns -- the box's single-step tiles
   // and the boundary nodes inside it --, the bricks (both steps; they read u^{n-1}, u^n and the old branch state only), all beside the pair
   // kernel; source / receivers of step n; then the second step of the single-step tiles and their nodes.  No ghost cell is read between the
   // two: neither the pair kernel nor the box's tiles reach one, the bricks mirror in LDS -- the flips in memory wait for the next single step.
   int step_pair_fcc_bricks(int64_t n) {
      hipStream_t s = s_main;
      // node values: u^{n-1}, u^n are only read; u^{n+1}, u^{n+2} go to two buffers nobody reads during the pair
      // branch state: the bricks and the first step of the box's nodes read s0 and write s1; the nodes' second step s1 in place
      const Pass p = pass_from_state(bufC, bufD, nullptr, ubx[0], nullptr, state_other());
      const Grids g1 = p.grids(0), g2 = p.grids(1);
      EvPair ev{}, ev2{}, evt{}, eva{};
      if (op.timing) { ev = ev_get(); ev2 = ev_get(); evt = ev_get(); eva = ev_get(); hipEventRecord(ev.first, s); hipEventRecord(eva.first, s); }
      const bool beside = !(op.debug & PF_DBG_WALLS_ONE_STREAM); // (else everything on the main stream)
      hipStream_t sw = beside ? s_edge : s_main;
      if (beside) { HIPCHK(hipEventRecord(ev_pre, s_main)); HIPCHK(hipStreamWaitEvent(s_edge, ev_pre, 0)); }
      launch_box_tiles_fcc(sw, g1);
      launch_rigid(sw, g1, p.bnd(0, fb_rest), {0, fb_nrest});
      launch_fcc_bricks(sw, p, 0, 2);
      // (with per-launch events on, the pair kernel waits for the bricks: its recorded duration is the kernel's own, not the overlap's)
      if (op.timing && beside) { HIPCHK(hipEventRecord(ev_edge, s_edge)); HIPCHK(hipStreamWaitEvent(s, ev_edge, 0)); }
      if (op.timing) hipEventRecord(evt.first, s);
      launch_tb2(s, n, p);
      if (op.timing) { hipEventRecord(evt.second, s); tb2_ev.push_back(evt); hipEventRecord(eva.second, s); air_ev.push_back(eva); }
      if (beside && !op.timing) { HIPCHK(hipEventRecord(ev_edge, s_edge)); HIPCHK(hipStreamWaitEvent(s_main, ev_edge, 0)); }
      launch_io(s, g1, n, true, src_range()); // (receivers read u^n; the source goes into u^{n+1}, which only the second step below reads)
      if (ring_fill == 0) ring_n0 = n;
      ring_fill++; steps_done++;
      if (op.timing) { hipEventRecord(ev.second, s); step_ev.push_back(ev); hipEventRecord(ev2.first, s); }
      launch_box_tiles_fcc(s, g2);
      launch_rigid(s, g2, p.bnd(1, fb_rest), {0, fb_nrest}); // second step of the box's nodes: u2b = u^n of the node, its u^{n+2} where the bricks put theirs
      launch_io(s, g2, n + 1, true, src_range());
      ring_fill++; steps_done++;
      // the state after the pair
      end_pass(p);
      if (op.timing) { hipEventRecord(ev2.second, s); step_ev.push_back(ev2); }
      HIPCHK(hipGetLastError());
      if (ring_fill == ring_depth) return flush();
      return PF_OK;
   }
