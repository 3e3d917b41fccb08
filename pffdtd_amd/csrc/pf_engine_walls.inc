// pf_engine_walls.inc -- part of `template <typename Real> struct Engine` (pf_engine.hip includes it INSIDE the class body; not a translation unit):
// wall regions: tables (Engine::init_walls) and launches (Engine::launch_walls_x) of k_wall2, pf_wall.h.
   // ---------------- wall regions: the shell of a blocked pair in pairs (pf_wall.h) ----------------
   // Six regions around the box: two whole-plane slabs normal to x, two row strips normal to y (the box's planes), two
   // column strips normal to z (the box's planes and rows) -- every interior cell outside the box belongs to exactly one.
   // Conditions: 7-point, margins that fit the pencils (8 cells for the strided ones,
   // 12 or 20 for the column strips), no source within one cell of the shell (a source is added BETWEEN the two steps,
   // which a region that keeps u^{n+1} in registers cannot see), fused boundary pass.  Otherwise the single-step shell of
   // round 2 runs (debug PF_DBG_NO_WALL_REGIONS forces that).
   // The frequency-dependent nodes are renumbered region by region in the order the lanes visit them (march, lane, pencil
   // cell), so that a wave's branch-state accesses are contiguous; the nodes inside the box follow in list order.
   // How a column strip becomes wall regions (0: it does not fit): 1 = one region with 12-cell pencils (strips of up to 10
   // columns), 3 = one region with 20-cell pencils (fp32), 2 = cut in two: the 7 columns next to the face, 12-cell pencils, and
   // the rest, plain air, 16-cell pencils.  t0 / t1: first / one past the last column of the box.
   int wl_lo_option(int t0, bool prefer_split) const {
      const bool split_ok = t0 >= 10 && t0 + 2 - 4 <= 16, wide_ok = sizeof(Real) == 4 && t0 + 2 <= 20;
      if (t0 + 2 <= 12) return 1;
      if (split_ok && (prefer_split || !wide_ok)) return 2;
      return wide_ok ? 3 : 0;
   }
   int wl_hi_option(int t1, bool prefer_split) const {
      const int z1 = std::min((t1 - 2) / 4 * 4, (int)P - 12), zw = (int)round_up(Nz - 12, 4), s0 = zw + 4, z2 = (t1 - 2) / 4 * 4; // (s0: whole vectors are stored)
      const int z20 = std::min((t1 - 2) / 4 * 4, (int)P - 20);
      const bool split_ok = zw >= 0 && zw + 12 <= P && s0 > t1 && s0 + 2 - z2 <= 16 && z2 + 16 <= P && (int)Nz - 1 - zw <= 11;
      const bool wide_ok = sizeof(Real) == 4 && z20 >= 0 && z20 + 20 >= Nz && t1 - z20 >= 2;
      if (z1 >= 0 && z1 + 12 >= Nz && t1 - z1 >= 2) return 1;
      if (split_ok && (prefer_split || !wide_ok)) return 2;
      return wide_ok ? 3 : 0;
   }
   void free_walls() {
      mem.release(wl_pen); mem.release(wl_rec); mem.release(wl_rest); mem.release(wl_blk); mem.release(wl_brk); mem.release(wl_binfo); mem.release(wl_blos);
      mem.release(vh1b); mem.release(gh1b); mem.release(ubx[0]); mem.release(ubx[1]);
      wl_nbrk = 0; wl_brk_lds = 0; wl_ns3 = wl_ns3z = false; wl_uni = 0; wl_rcv = 0;
      for (int &p : wl_prof) p = 0;
      wl_xw[0] = wl_xw[1] = false;
      wl_on = false;
      for (auto &g : wl_grp) g = WlGroup{};
   }
   // slab = true: a slab of a chain (pairs across two split-phase steps, step_begin): only the regions normal to y and z, over
   // the box's planes -- the planes between the slab's faces and the box (two edge planes per side, which are exchanged between
   // the two steps of a pair, and whatever x slab lies between them and the box) keep their single steps, and their boundary
   // nodes stay with the list kernel (wl_rest = the nodes of the interior planes no region owns).
   int init_walls(bool slab = false) {
      wl_on = false;
      const bool single = op.slab_first && op.slab_last;
      const bool vb = getenv("PFFDTD_VERBOSE") && atoi(getenv("PFFDTD_VERBOSE")) > 1;
#define WL_NO(why) do { if (vb) fprintf(stderr, "pffdtd_hip: no wall regions (%s)\n", why); return PF_OK; } while (0)
      if (slab ? (!tb2_slab || single) : (!tb2 || !single)) WL_NO("not a pair-stepping engine of this kind");
      if (fcc || tb_xr.empty() || swz || (op.debug & PF_DBG_NO_WALL_REGIONS)) WL_NO("13-point / no box / exchanged axes / switched off");
      if (Nb > 0 && !fuse_boundary) WL_NO("boundary pass not fused");
      if (Nbl >= ((int64_t)1 << 24) || Nb >= ((int64_t)1 << 31)) WL_NO("too many nodes");
      constexpr int DPS = 8, V = pf::VecOf<Real>::V;
      if (!slab && (tbx0 + 2 > DPS || Nx - tbx1 + 2 > DPS)) WL_NO("x margins");
      if (tby0 + 2 > DPS || Ny - tby1 + 2 > DPS) WL_NO("y margins");
      if ((!slab && Nx < 2 * DPS) || Ny < 2 * DPS) WL_NO("grid too small");
      if (slab && (tbx0 < 3 || tbx1 > Nx - 3 || steps_done > 0)) WL_NO("slab: box reaches the edge planes, or stepping has begun"); // (the lossy arrays are re-ordered below: only before the first step)
      for (int64_t i = 0; i < Ns; i++) { // sources stay two cells inside the box
         int64_t ix, iy, iz;
         decode(sd.in_ixyz[i], ix, iy, iz);
         // (a slab's regions lie beside its box only: a source in the planes between a cut and the box is none of their business)
         if ((!slab && (ix < tbx0 + 1 || ix > tbx1 - 2)) || iy < tby0 + 1 || iy > tby1 - 2 || iz < tbz0 + 1 || iz > tbz1 - 2) WL_NO("a source within a cell of the shell");
      }
      // the boundary list as the device holds it (sorted by cell)
      std::vector<int64_t> hb(Nb);
      std::vector<uint16_t> hadj(Nb);
      std::vector<int32_t> hl(Nb, -1);
      if (Nb) {
         HIPCHK(hipMemcpy(hb.data(), d_bn, Nb * sizeof(int64_t), hipMemcpyDeviceToHost));
         HIPCHK(hipMemcpy(hadj.data(), d_adj, Nb * sizeof(uint16_t), hipMemcpyDeviceToHost));
         HIPCHK(hipMemcpy(hl.data(), d_lossy, Nb * sizeof(int32_t), hipMemcpyDeviceToHost));
      }
      // ---- the frame as bricks (pf_brick.h): single-domain engines; debug PF_DBG_FRAME_GENERIC: the regions' generic blocks instead (round 5)
      // The x and y regions then end where the box's cross-section ends (their pencils look alike there: only the wall they belong
      // to is within reach), and what remains of the shell -- cells outside the box's range on at least two axes -- is twelve bars:
      //   F1: x margin x y margin x all z;  F2: x margin x box rows x z margin;  F3: box planes x y margin x z margin
      // cut into bricks of `blen` cells along their length.
      struct Bar { int a0[3], a1[3], axis, nchunk, first; };
      std::vector<Bar> bars;
      std::vector<pf::Brick> hbrk;
      std::vector<uint32_t> hinfo;
      std::vector<std::vector<uint2>> hlos;
      int blen = 0;
      const int Ng[3] = {(int)Nx, (int)Ny, (int)Nz};
      // A slab of a chain that steps in triples (tb3_geom): the four bars along x beside its box (F3) only -- the planes between the cuts and the box
      // are the split-phase step's --, its y / z regions in three steps like a single domain's.
      const bool slab3 = slab && tb3_geom;
      // could the x / y regions (can3) and the column strips (can3z) take three steps per pass?  (margins that fit 10-cell / 20-cell pencils; fp64:
      // three stages of 10-cell pencils spill; debug PF_DBG_XY_TWO_PLUS_ONE / PF_DBG_STRIPS_TWO_PLUS_ONE: two steps + one)
      constexpr int DPS3 = 10;
      const bool prefer_split = (op.debug & PF_DBG_STRIPS_SPLIT) != 0 || sizeof(Real) != 4;
      const bool can3 = !wl_no_ns3 && !(op.debug & PF_DBG_XY_TWO_PLUS_ONE) && sizeof(Real) == 4 &&
                        (!op.slab_first || tbx0 + 3 <= DPS3) && (!op.slab_last || (int)Nx - tbx1 + 3 <= DPS3) && Nx >= 2 * DPS3 && tby0 + 3 <= DPS3 && (int)Ny - tby1 + 3 <= DPS3 && Ny >= 2 * DPS3;
      const bool can3z = can3 && !(op.debug & PF_DBG_STRIPS_TWO_PLUS_ONE) && wl_lo_option(tbz0, prefer_split) == 3 && wl_hi_option(tbz1, prefer_split) == 3 && tbz0 + 3 <= 20 &&
                         tbz1 - std::min((tbz1 - 2) / 4 * 4, (int)P - 20) >= 3;
      const bool xlo_shell = op.slab_first != 0, xhi_shell = op.slab_last != 0; // is x = 1 / Nx - 2 the grid's own ABC shell?
      // (a slab: all or nothing -- its third split-phase step steps whatever has not taken three steps with the list kernels, which know no owners)
      bool bricks = (!slab || (slab3 && can3 && can3z)) && !(op.debug & (PF_DBG_FRAME_GENERIC | PF_DBG_THIRD_STEP_LISTS | PF_DBG_WALLS_ALL_GENERIC)) && tbzu0 >= 2 && tbzu1 <= (int)Nz - 2 && tbzu1 - tbzu0 >= 8;
      for (int64_t i = 0; i < Ns && bricks; i++) { // a brick recomputes three steps of its halo: no source within two cells of the shell
         int64_t ix, iy, iz;
         decode(sd.in_ixyz[i], ix, iy, iz);
         if (slab && ((ix < tbx0 - 4 && !xlo_shell) || (ix > tbx1 + 3 && !xhi_shell))) continue; // (in the planes between a cut and the reach of the regions and bricks: the split-phase step's business)
         if (ix < tbx0 + 2 || ix > tbx1 - 3 || iy < tby0 + 2 || iy > tby1 - 3 || iz < tbz0 + 2 || iz > tbz1 - 3) bricks = false;
      }
      if (bricks) {
         const int X[2][2] = {{1, tbx0}, {tbx1, (int)Nx - 1}}, Y[2][2] = {{1, tby0}, {tby1, (int)Ny - 1}}, Z[2][2] = {{1, tbzu0}, {tbzu1, (int)Nz - 1}};
         auto add = [&](const int *xr, const int *yr, const int *zr, int axis) {
            Bar b{{xr[0], yr[0], zr[0]}, {xr[1], yr[1], zr[1]}, axis, 0, 0};
            if (xr[1] > xr[0] && yr[1] > yr[0] && zr[1] > zr[0]) bars.push_back(b);
         };
         const int ZA[2] = {1, (int)Nz - 1}, YB[2] = {tby0, tby1}, XB[2] = {tbx0, tbx1};
         for (int i = 0; i < 2; i++) { // (a slab: on the side that is the grid's own wall)
            if (!(i == 0 ? xlo_shell : xhi_shell)) continue;
            for (int j = 0; j < 2; j++) add(X[i], Y[j], ZA, 2);
            for (int j = 0; j < 2; j++) add(X[i], YB, Z[j], 1);
         }
         for (int i = 0; i < 2; i++) for (int j = 0; j < 2; j++) add(XB, Y[i], Z[j], 0);
         constexpr int H = pf::BRICK_HALO;
         auto ext = [&](int o0, int o1, int d, int &e0, int &e1) { e0 = std::max(o0 - H, 1); e1 = std::min(o1 + H, Ng[d] - 1); };
         bool ok = false;
         for (int L : {16, 8, 4}) { // shorter bricks where the long ones need too much LDS or hold too many frequency-dependent nodes
            blen = L; ok = true;
            hbrk.clear(); hinfo.clear(); hlos.clear();
            for (Bar &b : bars) {
               b.first = (int)hbrk.size();
               b.nchunk = (int)cdiv(b.a1[b.axis] - b.a0[b.axis], L);
               for (int c = 0; c < b.nchunk; c++) {
                  pf::Brick k{};
                  int64_t cells = 1;
                  for (int d = 0; d < 3; d++) {
                     k.o0[d] = d == b.axis ? b.a0[d] + c * L : b.a0[d];
                     k.o1[d] = d == b.axis ? std::min(b.a0[d] + (c + 1) * L, b.a1[d]) : b.a1[d];
                     int e0, e1;
                     ext(k.o0[d], k.o1[d], d, e0, e1);
                     k.e0[d] = e0; k.en[d] = e1 - e0;
                     cells *= k.en[d];
                  }
                  if (pf::brick_lds_bytes<Real>(cells, (int)sd.Nm) > 60 * 1024 || hinfo.size() + (size_t)cells >= ((size_t)1 << 31)) { ok = false; break; }
                  k.info_off = (uint32_t)hinfo.size();
                  // air cells: the ABC count by their coordinates (cpu_engine.h:225-229, fdtd_data.h:621-675)
                  for (int ix = 0; ix < k.en[0]; ix++) for (int iy = 0; iy < k.en[1]; iy++) for (int iz = 0; iz < k.en[2]; iz++) {
                     const int g[3] = {k.e0[0] + ix, k.e0[1] + iy, k.e0[2] + iz};
                     uint32_t Q = 0;
                     for (int d = 0; d < 3; d++) Q += ((g[d] == 1 && (d > 0 || xlo_shell)) || (g[d] == Ng[d] - 2 && (d > 0 || xhi_shell))) ? 1u : 0u;
                     hinfo.push_back(Q << 8);
                  }
                  hbrk.push_back(k);
               }
               if (!ok) break;
            }
            if (!ok) continue;
            hlos.assign(hbrk.size(), {});
            // the boundary nodes inside the bricks' extended boxes
            for (int64_t nb = 0; nb < Nb && ok; nb++) {
               const int64_t ix = hb[nb] / plane, rem = hb[nb] % plane, iy = rem / P, iz = rem % P;
               const int g[3] = {(int)ix, (int)iy, (int)iz};
               for (const Bar &b : bars) {
                  bool in = true;
                  for (int d = 0; d < 3 && in; d++) in = g[d] >= std::max(b.a0[d] - H, 1) && g[d] < std::min(b.a1[d] + H, Ng[d] - 1);
                  if (!in) continue;
                  const int t = g[b.axis] - b.a0[b.axis];
                  for (int c = std::max((t - H) / L - 1, 0); c <= std::min((t + H) / L + 1, b.nchunk - 1); c++) {
                     pf::Brick &k = hbrk[(size_t)(b.first + c)];
                     if (g[b.axis] < k.e0[b.axis] || g[b.axis] >= k.e0[b.axis] + k.en[b.axis]) continue;
                     // (a node on the ABC shell would take the loss before its rigid update, cpu_engine.h:225-257: not a brick's business)
                     if ((g[0] == 1 && xlo_shell) || (g[0] == Ng[0] - 2 && xhi_shell) || g[1] == 1 || g[1] == Ng[1] - 2 || g[2] == 1 || g[2] == Ng[2] - 2) { ok = false; break; }
                     const uint32_t idx = ((uint32_t)(g[0] - k.e0[0]) * (uint32_t)k.en[1] + (uint32_t)(g[1] - k.e0[1])) * (uint32_t)k.en[2] + (uint32_t)(g[2] - k.e0[2]);
                     hinfo[k.info_off + idx] = (uint32_t)(hadj[nb] & 63u) | 0x40u | (hl[nb] >= 0 ? 0x80u : 0u);
                     if (hl[nb] >= 0) {
                        bool own = true;
                        for (int d = 0; d < 3; d++) own = own && g[d] >= k.o0[d] && g[d] < k.o1[d];
                        hlos[(size_t)(b.first + c)].push_back(make_uint2(idx | (own ? 0x80000000u : 0u), (uint32_t)hl[nb]));
                     }
                  }
                  if (!ok) break;
               }
            }
            if (!ok) break; // (a node on the ABC shell: no brick length helps)
            for (const auto &v : hlos) if (v.size() > (size_t)pf::BRICK_KN * pf::BRICK_T) ok = false;
            if (ok) break;
         }
         if (!ok || hbrk.empty()) { bricks = false; bars.clear(); hbrk.clear(); hinfo.clear(); hlos.clear(); }
      }
      auto in_frame = [&](int64_t ix, int64_t iy, int64_t iz) { // does a brick own this cell?
         const int64_t g[3] = {ix, iy, iz};
         for (const Bar &b : bars) {
            bool in = true;
            for (int d = 0; d < 3 && in; d++) in = g[d] >= b.a0[d] && g[d] < b.a1[d];
            if (in) return true;
         }
         return false;
      };
      std::vector<pf::WallRegion> reg;
      std::vector<int> dps, grp;
      // three steps per pass for the x / y regions (and the column strips): triples, bricks, and what `can3` / `can3z` above say
      const bool tb3_want = slab ? slab3 : bufE != nullptr; // (a single domain: init_tb2_impl allocates the fifth grid before it calls here)
      const bool ns3 = bricks && tb3_want && can3;
      const int DPX = ns3 ? DPS3 : DPS;
      const bool ns3z = ns3 && can3z;
      auto mk = [&](int group, int mode, int nbase, int kg, int ko0, int ko1, int dp, int l0, int l1, int m0, int m1) {
         pf::WallRegion R{};
         R.mode = mode; R.nbase = nbase; R.kg = kg; R.ko0 = ko0; R.ko1 = ko1;
         // x / y regions of a single domain with the frame in bricks: tables with three lanes / two march planes / three pencil cells of halo, so
         // that their alike blocks may take THREE steps per pass (k_wall2<..., NS = 3>); the two- and one-step kernels run on the same tiles
         const bool h3 = ns3 && (mode != 2 || (ns3z && group == 3));
         R.hl = h3 ? 3 : 2; R.lt = 64 - 2 * R.hl; R.hm = h3 ? 2 : 1;
         R.kb0 = std::max(ko0 - R.hl, 0); R.kb1 = std::min(ko1 + R.hl, dp);
         R.l0 = l0; R.l1 = l1; R.m0 = m0; R.m1 = m1;
         // march steps per block.  Single domain (the regions run before the box kernel, the machine to themselves): 8 and 16
         // equal, 24-32 1-2 % slower, 48-64 7 % (1024^3).  Slab of a chain (few hundred blocks, beside the box kernel on a stream
         // of their own): a block is a chain of dependent steps, so short ones -- rank of 8: 0.473 (16) / 0.347 (8) / 0.334-0.354
         // (4) / 0.349 (3) / 0.358 (2) ms per step against 0.334-0.373 without the regions; rank of 4: 0.69 / 0.60 / 0.56-0.59
         // against 0.62-0.65; rank of 2: 1.06 (4-6) against 1.21; an end rank of 8: 0.338 against 0.388
         int want = slab ? 4 : 16;
         if (slab && ns3 && (mode != 2 || (ns3z && group == 3))) { // (three stages: a block computes two march steps more at either end than it owns)
            want = 12; // (rank of 8 at 1024^3: 4 / 8 / 12 / 16 / 24 planes = 0.256 / 0.251 / 0.243 / 0.262 / 0.275 ms per step)
            if (const char *e = getenv("PFFDTD_SLAB_WALL_CHUNK")) if (atoi(e) > 0) want = atoi(e);
         }
         if (!slab && wl_chunk_want[mode == 2 ? 1 : 0] > 0) want = wl_chunk_want[mode == 2 ? 1 : 0];
         const int len = m1 - m0, nmc = (int)std::max<int64_t>(cdiv(len, want), 1);
         R.mchunk = (int)cdiv(len, nmc);
         R.nlt = (int)cdiv(l1 - l0, R.lt);
         R.nlp = R.nlt * R.lt + 2 * R.hl;
         reg.push_back(R); dps.push_back(dp); grp.push_back(group);
      };
      // March steps per block of a single domain's regions.  With the frame gone to bricks the alike launches have the machine to themselves,
      // one after the other, and a launch whose blocks do not fill a whole number of rounds of the SIMDs' wave slots (two waves per SIMD
      // for the x / y regions' kernel, one for the column strips') ends with a round of stragglers: 2176 one-wave blocks on 1024 slots took
      // 2.5 wave-times.  So: the fewest rounds whose chunks stay under ~80 planes, as few blocks as fill them (a block computes two march
      // steps more than it owns: long chunks waste less).  PFFDTD_WALL_CHUNK=xy,z overrides (experiments).
      wl_chunk_want[0] = wl_chunk_want[1] = 0;
      if (!slab && bricks) {
         auto pick = [&](int64_t tiles, int64_t len, int64_t slots) {
            for (int64_t r = 1; r <= 8; r++) {
               const int64_t nmc = std::max<int64_t>(slots * r / std::max<int64_t>(tiles, 1), 1), ch = cdiv(len, nmc);
               if (ch <= 80) return (int)std::max<int64_t>(ch, 4);
            }
            return 16;
         };
         const int64_t lt_xy = 4 * cdiv(tbzu1 - tbzu0, ns3 ? 58 : pf::WALL_LT), lt_z = 2 * cdiv(tby1 - tby0, ns3z ? 58 : pf::WALL_LT);
         wl_chunk_want[0] = pick(lt_xy, std::max(tby1 - tby0, tbx1 - tbx0), (ns3 || sizeof(Real) == 8) ? 1024 : 2048); // (fp64: one wave per SIMD too) (the three-step kernel: one wave per SIMD; 1024^3: 73 / 37 / 25 planes = 780 / 776 / 773 Gvox/s)
         wl_chunk_want[1] = pick(lt_z, tbx1 - tbx0, 1024);
         if (const char *e = getenv("PFFDTD_WALL_CHUNK")) { int a = 0, b = 0; if (sscanf(e, "%d,%d", &a, &b) == 2 && a > 0 && b > 0) { wl_chunk_want[0] = a; wl_chunk_want[1] = b; } }
      }
      const int zl0 = bricks ? tbzu0 : 1, zl1 = bricks ? tbzu1 : (int)Nz - 1, ym0 = bricks ? tby0 : 1, ym1 = bricks ? tby1 : (int)Ny - 1;
      // (an end slab of a chain that steps in triples: the region of its own x wall, as in a single domain -- nothing is exchanged on that side, so
      // its planes need no single steps; the old arrangement keeps them with the split-phase step)
      const bool xw0 = slab ? (bricks && xlo_shell) : true, xw1 = slab ? (bricks && xhi_shell) : true;
      if (xw0) mk(0, 0, 0, 0, 1, tbx0, DPX, zl0, zl1, ym0, ym1);
      if (xw1) mk(0, 0, (int)Nx - DPX, DPX - 1, tbx1 - ((int)Nx - DPX), DPX - 1, DPX, zl0, zl1, ym0, ym1);
      mk(0, 1, 0, 0, 1, tby0, DPX, zl0, zl1, tbx0, tbx1);
      mk(0, 1, (int)Ny - DPX, DPX - 1, tby1 - ((int)Ny - DPX), DPX - 1, DPX, zl0, zl1, tbx0, tbx1);
      // The column strips.  A strip of up to 10 columns is one region with pencils of 12 cells; a wider one (a sliver of the box went
      // to it) has pencils of 20 cells (fp32; ~350 registers, one wave per SIMD).  Cutting such a strip in two -- the 7 columns next
      // to the face with the wall layers, 12-cell pencils, and the rest, plain air, 16-cell pencils without any node code, two
      // waves per SIMD each -- was measured and LOSES (1024^3: 0.54 + 0.31 ms against 0.59 ms per pair): only where the wide pencils
      // do not fit (odd widths, fp64) or with debug 0x2000000 (tests).  What that pointed at -- every load and store instruction of a
      // strip reaches 64 separate lines, a lane per row -- is measured now: the three-step bodies with a uniform branch count move their
      // tile row by row and turn rows into pencils in LDS (pf_strip_map.h, pf_wall.h STG), and the strip launch of a 1024^3 triple fell
      // from 393-406 to 337-353 us (medians of three processes each, profiles/strips_staged.txt).  A part of the gap to the x / y
      // regions, not all of it: the strips' 18 cells of air update per stage and their 170 accumulation registers stay.
      int zb = 0;
      bool zok = true;
      { // low side
         const int opt = wl_lo_option(tbz0, prefer_split);
         if (opt == 1) mk(1, 2, 0, 0, 1, tbz0, 12, tby0, tby1, tbx0, tbx1);
         else if (opt == 2) {
            mk(1, 2, 0, 0, 1, 8, 12, tby0, tby1, tbx0, tbx1);
            mk(2, 2, 4, -1, 8 - 4, tbz0 - 4, 16, tby0, tby1, tbx0, tbx1);
         } else if (opt == 3) mk(3, 2, 0, 0, 1, tbz0, 20, tby0, tby1, tbx0, tbx1);
         else zok = false;
      }
      { // high side
         const int z1 = std::min((tbz1 - 2) / 4 * 4, (int)P - 12);
         const int zw = (int)round_up(Nz - 12, 4), s0 = zw + 4;   // wall part: pencil from column zw, owned from s0 (whole vectors are stored)
         const int z2 = (tbz1 - 2) / 4 * 4;                      // the rest: pencil from column z2
         const int z20 = std::min((tbz1 - 2) / 4 * 4, (int)P - 20);
         const int opt = wl_hi_option(tbz1, prefer_split);
         if (opt == 1) { zb = z1; mk(1, 2, z1, (int)Nz - 1 - z1, tbz1 - z1, (int)Nz - 1 - z1, 12, tby0, tby1, tbx0, tbx1); }
         else if (opt == 2) {
            zb = zw;
            mk(1, 2, zw, (int)Nz - 1 - zw, 4, (int)Nz - 1 - zw, 12, tby0, tby1, tbx0, tbx1);
            mk(2, 2, z2, -1, tbz1 - z2, s0 - z2, 16, tby0, tby1, tbx0, tbx1);
         } else if (opt == 3) { zb = z20; mk(3, 2, z20, (int)Nz - 1 - z20, tbz1 - z20, (int)Nz - 1 - z20, 20, tby0, tby1, tbx0, tbx1); }
         else zok = false;
      }
      if (!zok) WL_NO("column strips too wide for the pencils");
#undef WL_NO
      const int nregs = (int)reg.size();
      // every feasibility check comes BEFORE a device array is touched (the lossy arrays are re-ordered in place below)
      std::vector<uint32_t> rloc((size_t)nregs); // a region's place in its launch group
      {
         int cnt[4] = {0, 0, 0, 0};
         for (int i = 0; i < nregs; i++) {
            if (cnt[grp[i]] >= pf::WALL_MAXREG) return PF_OK;
            rloc[i] = (uint32_t)cnt[grp[i]]++;
         }
      }
      int64_t npen = 0;
      for (int i = 0; i < nregs; i++) { reg[i].pen_off = npen; npen += (int64_t)(reg[i].m1 - reg[i].m0 + 2 * reg[i].hm) * reg[i].nlp; }
      if (npen >= ((int64_t)1 << 31)) return PF_OK;
      // a node's place in a region's frame
      auto frame = [&](const pf::WallRegion &R, int64_t ix, int64_t iy, int64_t iz, int &k, int &lc, int &m) {
         if (R.mode == 0) { k = (int)ix - R.nbase; lc = (int)iz; m = (int)iy; }
         else if (R.mode == 1) { k = (int)iy - R.nbase; lc = (int)iz; m = (int)ix; }
         else { k = (int)iz - R.nbase; lc = (int)iy; m = (int)ix; }
      };
      // owners, and the new order of the frequency-dependent nodes
      std::vector<int8_t> owner(Nb, 8);
      struct Key { int32_t r, m, lc, k, li; };
      std::vector<Key> keys;
      keys.reserve((size_t)Nbl);
      std::vector<int32_t> rest;
      for (int64_t nb = 0; nb < Nb; nb++) {
         const int64_t ix = hb[nb] / plane, rem = hb[nb] % plane, iy = rem / P, iz = rem % P;
         int r = 8, k = 0, lc = 0, m = 0;
         for (int i = 0; i < nregs; i++) {
            int kk, ll, mm;
            frame(reg[i], ix, iy, iz, kk, ll, mm);
            if (kk >= reg[i].ko0 && kk < reg[i].ko1 && ll >= reg[i].l0 && ll < reg[i].l1 && mm >= reg[i].m0 && mm < reg[i].m1) { r = i; k = kk; lc = ll; m = mm; break; }
         }
         owner[nb] = (int8_t)r;
         const Range &midr = bn_cut[tb3_geom ? 3 : 2].mid;
         if (r == 8 && bricks && in_frame(ix, iy, iz)) r = 9; // a brick's
         owner[nb] = (int8_t)r;
         if (r == 8 && (!slab || (nb >= midr.b && nb < midr.e))) rest.push_back((int32_t)nb); // (a slab's edge planes: range launches)
         if (hl[nb] >= 0) keys.push_back({r, m, lc, k, hl[nb]});
      }
      if ((int64_t)keys.size() != Nbl) return PF_OK; // (a lossy node that is no boundary node: fuse_boundary excludes it)
      std::stable_sort(keys.begin(), keys.end(), [](const Key &a, const Key &b) {
         if (a.r != b.r) return a.r < b.r;
         if (a.r >= 8) return a.li < b.li;
         if (a.m != b.m) return a.m < b.m;
         if (a.lc != b.lc) return a.lc < b.lc;
         return a.k < b.k;
      });
      std::vector<int32_t> newli((size_t)Nbl);
      for (int64_t j = 0; j < Nbl; j++) newli[keys[j].li] = (int32_t)j;
      // pencil tables: node masks, then the records in pencil order (the boundary list is sorted by cell, so a pencil's
      // nodes arrive in ascending pencil-cell order)
      std::vector<uint4> pen((size_t)npen, make_uint4(0u, 0u, 0u, 0u));
      auto visit = [&](auto &&fn) {
         for (int64_t nb = 0; nb < Nb; nb++) {
            const int64_t ix = hb[nb] / plane, rem = hb[nb] % plane, iy = rem / P, iz = rem % P;
            for (int i = 0; i < nregs; i++) {
               const pf::WallRegion &R = reg[i];
               int k, lc, m;
               frame(R, ix, iy, iz, k, lc, m);
               if (k < std::max(1, R.ko0 - (R.hl - 1)) || k > std::min(dps[i] - 2, R.ko1 + (R.hl - 2)) || lc < R.l0 - (R.hl - 1) || lc > R.l1 + (R.hl - 2) ||
                   m < R.m0 - R.hm || m > R.m1 + R.hm - 1) continue;
               fn(nb, R.pen_off + (int64_t)(m - (R.m0 - R.hm)) * R.nlp + (lc - (R.l0 - R.hl)), k);
            }
         }
      };
      visit([&](int64_t, int64_t pi, int k) { pen[(size_t)pi].x |= 1u << k; });
      int64_t nrec = 0;
      for (int64_t i = 0; i < npen; i++) { pen[(size_t)i].y = (uint32_t)nrec; nrec += __builtin_popcount(pen[(size_t)i].x); }
      if (nrec >= ((int64_t)1 << 27)) return PF_OK;
      std::vector<uint32_t> rec((size_t)std::max<int64_t>(nrec, 1), 0u);
      visit([&](int64_t nb, int64_t pi, int k) {
         uint4 &e = pen[(size_t)pi];
         const uint32_t jn = (uint32_t)__builtin_popcount(e.x & ((1u << k) - 1u));
         const uint32_t adj = (uint32_t)(hadj[nb] & 63u);
         rec[(e.y & 0x7ffffffu) + jn] = adj | (hl[nb] >= 0 ? (0x40u | ((uint32_t)newli[hl[nb]] << 8)) : 0u);
         if (jn < 5) { // the entry itself carries the first five nodes: adjacency bits, lossy flags, the first lossy one's place
            e.z |= adj << (6 * jn);
            if (hl[nb] >= 0) {
               if ((e.w & 31u) == 0u) { e.w |= (uint32_t)newli[hl[nb]] << 8; e.y |= (uint32_t)k << 27; }
               e.w |= 1u << jn;
            }
         }
      });
      int rc;
      free_walls(); // (a second call -- set_spares after place_grids -- must not leak the first one's tables)
      // Wall regions are an optimisation: when the device has no room for their tables and the second copy of the branch state, the
      // engine keeps the single-step shell instead of failing (everything is allocated BEFORE the lossy arrays are re-ordered).
      auto no_room = [&]() { free_walls(); (void)hipGetLastError(); pf__set_error(""); if (vb) fprintf(stderr, "pffdtd_hip: no wall regions (no device memory for their tables)\n"); return PF_OK; };
      vh1b = try_dzalloc<Real>(round_up(Nbl, 64) * PF_MMB);
      gh1b = vh1b ? try_dzalloc<Real>(round_up(Nbl, 64) * PF_MMB) : nullptr;
      if (!gh1b) return no_room();
      if ((rc = upload(&wl_pen, pen.data(), npen))) return no_room();
      if ((rc = upload(&wl_rec, rec.data(), nrec))) return no_room();
      wl_nrest = (int64_t)rest.size();
      if ((rc = upload(&wl_rest, rest.data(), wl_nrest))) return no_room();
      if (!slab || slab3) { // two more node-value buffers: a pass never writes a buffer anybody reads during it (launch_walls_x, pf_brick.h)
         for (int k = 0; k < 2; k++) { ubx[k] = try_dzalloc<Real>(std::max<int64_t>(Nbl, 1)); if (!ubx[k]) return no_room(); }
      }
      if (bricks) {
         std::vector<uint2> flat;
         int64_t nbown = 0;
         size_t lds = 0;
         for (size_t b = 0; b < hbrk.size(); b++) {
            hbrk[b].los_off = (uint32_t)flat.size(); hbrk[b].nlos = (uint32_t)hlos[b].size();
            for (uint2 e : hlos[b]) {
               e.y = (uint32_t)newli[e.y];
               flat.push_back(e);
               if (e.x >> 31) nbown++;
            }
            lds = std::max(lds, pf::brick_lds_bytes<Real>((int64_t)hbrk[b].en[0] * hbrk[b].en[1] * hbrk[b].en[2], (int)sd.Nm));
         }
         if ((rc = upload(&wl_brk, hbrk.data(), (int64_t)hbrk.size()))) return no_room();
         if ((rc = upload(&wl_binfo, hinfo.data(), (int64_t)hinfo.size()))) return no_room();
         if ((rc = upload(&wl_blos, flat.data(), (int64_t)flat.size()))) return no_room();
         wl_nbrk = (int64_t)hbrk.size(); wl_brk_lds = lds; wl_nbown_dbg = nbown;
      }
      // the lossy arrays in the new order (state and node-value arrays are all zeros at creation)
      if (Nbl) {
         std::vector<int64_t> bl(Nbl), bl2(Nbl);
         std::vector<Real> sf(Nbl), sf2(Nbl);
         std::vector<int8_t> mt(Nbl), mt2(Nbl);
         HIPCHK(hipMemcpy(bl.data(), d_bnl, Nbl * sizeof(int64_t), hipMemcpyDeviceToHost));
         HIPCHK(hipMemcpy(sf.data(), d_ssaf, Nbl * sizeof(Real), hipMemcpyDeviceToHost));
         HIPCHK(hipMemcpy(mt.data(), d_mat, Nbl * sizeof(int8_t), hipMemcpyDeviceToHost));
         for (int64_t j = 0; j < Nbl; j++) { bl2[newli[j]] = bl[j]; sf2[newli[j]] = sf[j]; mt2[newli[j]] = mt[j]; }
         HIPCHK(hipMemcpy(d_bnl, bl2.data(), Nbl * sizeof(int64_t), hipMemcpyHostToDevice));
         HIPCHK(hipMemcpy(d_ssaf, sf2.data(), Nbl * sizeof(Real), hipMemcpyHostToDevice));
         HIPCHK(hipMemcpy(d_mat, mt2.data(), Nbl * sizeof(int8_t), hipMemcpyHostToDevice));
         HIPCHK(hipMemcpy(bl.data(), d_lperm, Nbl * sizeof(int64_t), hipMemcpyDeviceToHost)); // (each node's row in sd.bnl_ixyz moves with it: pf_engine_state.inc)
         for (int64_t j = 0; j < Nbl; j++) bl2[newli[j]] = bl[j];
         HIPCHK(hipMemcpy(d_lperm, bl2.data(), Nbl * sizeof(int64_t), hipMemcpyHostToDevice));
         for (int64_t nb = 0; nb < Nb; nb++) if (hl[nb] >= 0) hl[nb] = newli[hl[nb]];
         HIPCHK(hipMemcpy(d_lossy, hl.data(), Nb * sizeof(int32_t), hipMemcpyHostToDevice));
      }
      for (auto &g : wl_grp) g = WlGroup{};
      for (int i = 0; i < nregs; i++) {
         WlGroup &g = wl_grp[grp[i]];
         g.reg[g.nreg++] = reg[i];
      }
      // does every region of a launch group have the standard pencil geometry of a box with margin GD on its pencil axis (pf_wall.h: wall_body<..., GD, HI>)?
      for (int gi = 0; gi < 4; gi++) {
         const WlGroup &g = wl_grp[gi];
         int gd = 0;
         for (int i = 0; i < g.nreg; i++) {
            const pf::WallRegion &R = g.reg[i];
            const int dp = gi == 0 ? DPX : (gi == 1 ? 12 : (gi == 2 ? 16 : 20));
            const int NNp = R.mode == 2 ? (int)Nz : (R.mode == 1 ? (int)Ny : (int)Nx);
            int d = -1;
            if (R.kg == 0 && R.ko0 == 1 && R.nbase == 0) d = R.ko1;
            else if (R.kg == dp - 1 && R.ko1 == dp - 1 && R.nbase == NNp - dp) d = dp - R.ko0;
            if (d <= 0 || R.hl != 3 || (gd && d != gd)) { gd = -1; break; }
            gd = d;
         }
         wl_geo[gi] = (gd > 0 && !(op.debug & PF_DBG_RUNTIME_GEOMETRY)) ? gd : 0;
      }
      // Block lists.  A block (lane tile x march chunk of a region) whose pencils all have the same structure and that touches no
      // ghost / ABC cell along its lane and march axes goes to the FAST launch with that structure attached; the others
      // (edges, corners, the ends of a march) to the generic one.
      std::vector<uint4> lists[12]; // group g: 3 g alike, 3 g + 1 generic, 3 g + 2 alike and free of nodes
      std::vector<uint4> lists2;    // x / y regions with three-step tables: their blocks once more with the chunks of a TWO-step launch (below)
      int64_t nfast = 0, ngen = 0;
      bool second = false;
      auto build = [&](int i, int mchunk) {
         const pf::WallRegion &R = reg[i];
         const int NL = R.mode == 2 ? (int)Ny : (int)Nz, NM = R.mode == 0 ? (int)Ny : (int)Nx;
         const int nmc = (int)cdiv(R.m1 - R.m0, mchunk);
         for (int c = 0; c < nmc; c++)
            for (int jt = 0; jt < R.nlt; jt++) {
               const int ms = R.m0 + c * mchunk, me = std::min(ms + mchunk, R.m1);
               const int lc0 = R.l0 - (R.hl - 1) + R.lt * jt, lc1 = std::min(R.l0 + R.lt * jt + R.lt + (R.hl - 2), R.l1 + (R.hl - 2)); // lanes 1 .. 62 within the region
               const int mlo = ms - R.hm, mhi = me + R.hm - 1; // march steps whose pencils the block evaluates
               bool fast = lc0 >= 2 && lc1 <= NL - 3 && mlo >= 2 && mhi <= NM - 3 && !(op.debug & PF_DBG_WALLS_ALL_GENERIC);
               const uint4 ref = pen[(size_t)(R.pen_off + (int64_t)(mlo - (R.m0 - R.hm)) * R.nlp + (lc0 - (R.l0 - R.hl)))];
               if (__builtin_popcount(ref.x) > 5 || __builtin_popcount(ref.w & 31u) > 1) fast = false;
               for (int m = mlo; m <= mhi && fast; m++) {
                  const uint4 *row = pen.data() + (size_t)(R.pen_off + (int64_t)(m - (R.m0 - R.hm)) * R.nlp - (R.l0 - R.hl));
                  for (int lc = lc0; lc <= lc1; lc++) {
                     const uint4 &e = row[lc];
                     if (e.x != ref.x || e.z != ref.z || (e.w & 31u) != (ref.w & 31u) || (e.y >> 27) != (ref.y >> 27)) { fast = false; break; }
                  }
               }
               const uint32_t rl = rloc[i];
               const uint4 b = make_uint4(rl | ((uint32_t)jt << 3) | ((uint32_t)c << 16), ref.x, ref.z, (ref.w & 31u) | ((ref.y >> 27) << 8));
               if (second) { if (fast) lists2.push_back(b); continue; }
               lists[3 * grp[i] + (fast ? (ref.x == 0u && R.mode == 2 ? 2 : 0) : 1)].push_back(b);
               (fast ? nfast : ngen)++;
            }
      };
      for (int i = 0; i < nregs; i++) build(i, reg[i].mchunk);
      // The x / y regions' three-step kernel runs one wave per SIMD, their two-step kernel (a run's closing pair) two: on the three-step
      // launch's blocks it would fill half its wave slots (529 us for two steps where three take 520).  A second block list with half the
      // chunk length for that launch (WlGroup::mchunk2, blk0b / nblkb).
      wl_grp[0].nblkb = 0;
      if (ns3) {
         second = true;
         for (int i = 0; i < nregs; i++) if (grp[i] == 0) { wl_grp[0].mchunk2[rloc[i]] = std::max(reg[i].mchunk / 2, 4); build(i, wl_grp[0].mchunk2[rloc[i]]); }
         second = false;
      }
      {
         std::vector<uint4> all;
         for (int q = 0; q < 12; q++) { wl_grp[q / 3].blk0[q % 3] = (uint32_t)all.size(); wl_grp[q / 3].nblk[q % 3] = (uint32_t)lists[q].size(); all.insert(all.end(), lists[q].begin(), lists[q].end()); }
         wl_grp[0].blk0b = (uint32_t)all.size(); wl_grp[0].nblkb = (uint32_t)lists2.size(); all.insert(all.end(), lists2.begin(), lists2.end());
         if ((rc = upload(&wl_blk, all.data(), (int64_t)all.size()))) return no_room(); // (the lossy arrays are re-ordered by now: consistently, which any path accepts)
      }
      // Does every alike block of a three-step launch group carry the node words of a wall profile (pf_wall.h: wall_profile_words -- the two node
      // layers of a plain box wall)?  Then the bodies with those words compiled in run (fp32: fp64 takes no three steps per pass); one block that
      // differs -- a room that is no plain box, other wall depths, mixed materials -- keeps the bodies that read the words from the block.
      for (int gi = 0; gi < 4; gi++) {
         wl_prof[gi] = 0;
         const std::vector<uint4> &bl = lists[3 * gi];
         if (sizeof(Real) != 4 || (gi != 0 && gi != 3) || wl_geo[gi] <= 0 || bl.empty() || !lists[3 * gi + 2].empty() || (op.debug & PF_DBG_RUNTIME_NODES)) continue;
         const int dp = gi == 0 ? DPX : 20;
         for (int pr = 1; pr <= pf::WALL_NPROF && !wl_prof[gi]; pr++) {
            bool all = true;
            for (const uint4 &b : bl) {
               const pf::WallRegion &R = wl_grp[gi].reg[b.x & 7u];
               const pf::WallNodes n = pf::wall_profile_words(R.mode, R.kg != 0, dp, pr);
               if (b.y != n.x || b.z != n.z || b.w != n.w) { all = false; break; }
            }
            if (all) wl_prof[gi] = pr;
         }
      }
      // Do all materials have the same branch count (pf_wall.h: fd_regs' uniform form, where wall_choose finds a kernel for the count)?  debug PF_DBG_BRANCH_SELECTS: never
      wl_uni = (sd.Nm > 0 && !(op.debug & PF_DBG_BRANCH_SELECTS)) ? mb_max : 0;
      for (int k = 0; k < sd.Nm; k++) if (sd.Mb[k] != mb_max) wl_uni = 0;
      // which launch groups own a cell with a receiver in it?  (the others' u^{n+1} need not reach the scratch grid: launch_walls_x)
      wl_rcv = 0;
      for (int64_t i = 0; i < Nr; i++) {
         int64_t ix, iy, iz;
         decode(sd.out_ixyz[i], ix, iy, iz);
         for (int r = 0; r < nregs; r++) {
            int k, lc, m;
            frame(reg[r], ix, iy, iz, k, lc, m);
            if (k >= reg[r].ko0 && k < reg[r].ko1 && lc >= reg[r].l0 && lc < reg[r].l1 && m >= reg[r].m0 && m < reg[r].m1) wl_rcv |= 1u << grp[r];
         }
      }
      wl_ns3 = ns3; wl_ns3z = ns3z;
      if ((ns3 && wl_grp[0].nblk[1] > 0) || (ns3z && (wl_grp[3].nblk[1] > 0 || wl_grp[3].nblk[2] > 0))) { // some block is not alike (a room that is no plain box), or a strip block holds
         // no node (the three-step strip launch takes list 0 only: list 2 would go unstepped): those regions keep two steps + one
         wl_no_ns3 = true;
         return init_walls(slab);
      }
      wl_on = true;
      wl_xw[0] = slab && xw0; wl_xw[1] = slab && xw1;
      if (getenv("PFFDTD_VERBOSE") && atoi(getenv("PFFDTD_VERBOSE")) > 0)
         fprintf(stderr, "pffdtd_hip: wall regions: box x [%d,%d) y [%d,%d) z [%d,%d), %ld pencils, %ld node records, %ld of %ld boundary nodes left to the list kernel, column pencils of %d cells from column %d; %ld blocks alike, %ld generic; frame: %ld bricks of %d cells along their bar (%ld cells with their halos, %ld frequency-dependent nodes owned, %zu bytes of LDS)\n",
                 tbx0, tbx1, tby0, tby1, tbz0, tbz1, (long)npen, (long)nrec, (long)wl_nrest, (long)Nb, dps.back(), zb, (long)nfast, (long)ngen, (long)wl_nbrk, blen, (long)hinfo.size(), (long)wl_nbown_dbg, wl_brk_lds);
      return PF_OK;
   }
   // The wall regions (k_wall2): `ns` steps in one launch that starts at step `first` of the pass.  Grids: g[first], g[first + 1] are read, the ns after them
   // written (ns = 3: three steps in one pass, x / y regions with three-step tables: wl_ns3; ns = 1: ONE step, the third of a triple: first = 2);
   // node values: x[first], x[first + 1] are read, the ns after them receive the steps' (three node-value buffers: u^{n+2} of a node overwrites
   // its u^n); branch state: the pass's first step reads s0, every launch writes s1.  gmask: which launch groups (bit 0: the x / y regions,
   // bits 1-3: the column strips); s_gen: the stream of the generic blocks -- edges, corners: few waves, each a long chain of dependent steps
   void launch_walls_x(hipStream_t s, hipStream_t s_gen, const Pass &p, int first, int ns, unsigned gmask) {
      pf::WallParams<Real> wp{};
      Real *const C = p.out_g(first, ns, 0);
      wp.A = p.g[first]; wp.B = p.g[first + 1]; wp.C = C; wp.D = p.out_g(first, ns, 1); wp.E = p.out_g(first, ns, 2);
      wp.plane = plane; wp.Nx = (int)Nx; wp.Ny = (int)Ny; wp.Nz = (int)Nz; wp.P = (int)P; wp.first = op.slab_first; wp.last = op.slab_last;
      wp.pen = wl_pen; wp.rec = wl_rec;
      wp.sv_in = p.in(first).v; wp.sg_in = p.in(first).g; wp.sv_out = p.s1.v; wp.sg_out = p.s1.g;
      wp.x2 = p.x[first]; wp.x1 = p.x[first + 1]; wp.o1 = p.out_x(first, ns, 0); wp.o2 = p.out_x(first, ns, 1); wp.o3 = p.out_x(first, ns, 2);
      wp.ssaf = d_ssaf; wp.mat = d_mat; wp.Mb = d_Mb; wp.mq = d_mq; wp.beta = d_beta;
      wp.lo2 = lo2; wp.sl2 = sl2; wp.l = l; wp.mmax = mb_max; wp.nmat = sd.Nm;
      for (int gi = 0; gi < 4; gi++) {
         if (!((gmask >> gi) & 1u)) continue;
         const WlGroup &g = wl_grp[gi];
         wp.nreg = g.nreg;
         for (int i = 0; i < g.nreg; i++) wp.reg[i] = g.reg[i];
         for (int q = 0; q < 3; q++) { // alike blocks, generic blocks, alike blocks without nodes (column strips only)
            if (!g.nblk[q]) continue;
            const WallChoice c = wall_choice(gi, q, ns); // (no kernel: nothing to launch -- lists init_walls never fills, pf_wall.h: wall_choices_match_table)
            wp.C = c.skip_c ? nullptr : C; wp.blk = wl_blk + (c.second ? g.blk0b : g.blk0[q]);
            for (int i = 0; i < g.nreg; i++) wp.reg[i].mchunk = c.second ? g.mchunk2[i] : g.reg[i].mchunk;
            const dim3 gd(c.second ? g.nblkb : g.nblk[q]); const hipStream_t st = q == 1 ? s_gen : s; const std::make_integer_sequence<int, pf::WALL_KERNELS<sizeof(Real) == 8>.cap> rows;
            if (sg) pf::wall_launch<Real, true>(c.k, gd, st, wp, a1, a2, rows); else pf::wall_launch<Real, false>(c.k, gd, st, wp, a1, a2, rows);
         }
      }
   }
   // the frame's bricks (pf_brick.h): `ns` steps in one launch from step `first` of the pass, windows as in launch_walls_x -- the node values of the steps go
   // to buffers nobody reads during the pass
   void launch_bricks(hipStream_t s, const Pass &p, int first, int ns) {
      if (!wl_nbrk) return;
      pf::BrickParams<Real> bp{};
      bp.x2 = p.x[first]; bp.x1 = p.x[first + 1];
      bp.A = p.g[first]; bp.B = p.g[first + 1];
      for (int j = 0; j < 3; j++) { bp.G[j] = p.out_g(first, ns, j); bp.O[j] = p.out_x(first, ns, j); }
      bp.plane = plane; bp.Nx = (int)Nx; bp.Ny = (int)Ny; bp.Nz = (int)Nz; bp.P = (int)P;
      bp.brk = wl_brk; bp.info = wl_binfo; bp.los = wl_blos;
      bp.sv_in = p.in(first).v; bp.sg_in = p.in(first).g; bp.sv_out = p.s1.v; bp.sg_out = p.s1.g;
      bp.ssaf = d_ssaf; bp.mat = d_mat; bp.Mb = d_Mb; bp.mq = d_mq; bp.beta = d_beta;
      bp.lo2 = lo2; bp.sl2 = sl2; bp.l = l; bp.nmat = (int)sd.Nm; bp.ns = ns;
      bp.first = op.slab_first; bp.last = op.slab_last;
      const dim3 g((unsigned)wl_nbrk), b(pf::BRICK_T);
      const bool lo = pf::wall_mc(mb_max) == pf::WALL_MC[0];
      if (lo && sg) hipLaunchKernelGGL((pf::k_brick<Real, pf::WALL_MC[0], true>), g, b, wl_brk_lds, s, bp, a1, a2);
      else if (lo) hipLaunchKernelGGL((pf::k_brick<Real, pf::WALL_MC[0], false>), g, b, wl_brk_lds, s, bp, a1, a2);
      else if (sg) hipLaunchKernelGGL((pf::k_brick<Real, pf::WALL_MC[1], true>), g, b, wl_brk_lds, s, bp, a1, a2);
      else hipLaunchKernelGGL((pf::k_brick<Real, pf::WALL_MC[1], false>), g, b, wl_brk_lds, s, bp, a1, a2);
   }
