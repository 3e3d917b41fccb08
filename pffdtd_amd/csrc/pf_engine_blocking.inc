// pf_engine_blocking.inc -- part of `template <typename Real> struct Engine` (pf_engine.hip includes it INSIDE the class body; not a translation unit):
// the box a blocked kernel may advance by two or three steps per pass, its tiles, the strips' node tables (Engine::init_tb2*).
   // ---------------- temporal blocking: two steps per pass over the boundary-free box ----------------
   // Every boundary node of a box-shaped room sits within a few cells of a grid face; the box of cells at least two
   // cells deeper than the deepest boundary node (and off the ABC shell) sees nothing but the plain air update for two
   // consecutive steps, so k_tb2_reg may produce u^{n+1} and u^{n+2} there in one pass (16 B per cell instead of 24).
   // The shell around the box (x slabs, row strips, column strips; all boundary / ABC / source cells live there) is
   // stepped twice by the single-step kernels, out of place.  Rooms with interior geometry have no such box: tb2 stays
   // off and nothing changes.  air_variant 0 (auto) and 40 enable it, 41 = same driver with the box disabled (tests).
   // undo a temporal-blocking arrangement (its grids, tile lists, strip tables, wall regions): the engine steps singly
   void drop_blocking() {
      tb2 = tb3 = false;
      free_walls();
      mem.release(bufC); mem.release(bufD); mem.release(bufE);
      mem.release(zs_map); mem.release(zs_adj); mem.release(zs_li); mem.release(zs_rest); mem.release(zs_fd);
      zs_mode = 0;
   }
   // Three steps per pass where they can be had: single-domain 7-point engines in file-order storage, 64-lane row segments, the
   // shell as wall regions (init_walls).  The box then keeps THREE cells from anything that is not a plain air update (k_tb3
   // computes u^{n+1} two cells beyond it).  Anything else: pairs as before.  PF_DBG_NO_TRIPLES: never triples.
   int init_tb2() {
      tb3 = tb3_geom = tb3_slab = false;
      const bool single = op.slab_first && op.slab_last;
      if (!fcc && !swz && !(op.debug & (PF_DBG_NO_TRIPLES | PF_DBG_LW32 | PF_DBG_LW16 | PF_DBG_NO_WALL_REGIONS)) && vbase != 41) {
         int rc = init_tb2_impl(true);
         if (rc) return rc;
         if (single && tb2 && wl_on) { tb3 = true; return PF_OK; }
         // slab engines: the triples' box and tiles stand; whether they are used is decided when the caller hands over its grids
         // (pf_engine_place_grids5: five grids and wall regions that fit; else the pairs' geometry is rebuilt there)
         if (!single && tb2_geom) { tb3_geom = true; return PF_OK; }
         drop_blocking();
      }
      return init_tb2_impl(false);
   }
   int init_tb2_impl(bool triple) {
      tb2 = tb2_geom = tb2_slab = false;
      tb_nsrct = 0;
      const bool single = op.slab_first && op.slab_last;
      if (op.energy || (op.debug & PF_DBG_SINGLE_STEPS)) return PF_OK;
      // exchanged axes (rooms): the pair kernels work in storage coordinates and take their neighbours in the FILE's order (template
      // flag SWZ: 64-lane row segments, single-domain engines); 7-point: k_tb2_reg / k_tb1_tile / k_air_zstrip<..., SWZ>
      if (swz && !single) return PF_OK;
      // 7-point: the fused single-step kernels carry the shell; 13-point: folded grids with the flips in memory and the ABC
      // loss in the interior kernel (the automatic 13-point arrangement)
      if (fcc ? !(fold && abck) : !(lean || vg)) return PF_OK;
      if (!(vbase == 0 || vbase == 40 || vbase == 41) || !use_dpp) return PF_OK;
      if (Nb > 0 && !boundary_fused()) return PF_OK;
      // Margins of the box: three cells off every grid face (the ABC cells sit at index 1 and the box must stay two cells
      // away from anything that is not a plain air update), deeper where a wall layer hugs the face -- a face whose plane at
      // depth d <= 12 is at least half boundary nodes pushes the box to depth d + 2 (shoebox rooms: walls at depth 2-3,
      // box from depth 5).  Whatever geometry remains inside the box is dealt with tile by tile below.
      const int64_t NzNy = Nz * Ny;
      int64_t hist[6][16] = {};
      for (int64_t i = 0; i < Nb; i++) {
         int64_t ix, iy, iz; // storage coordinates
         decode(sd.bn_ixyz[i], ix, iy, iz);
         const int64_t d[6] = {ix, Nx - 1 - ix, iy, Ny - 1 - iy, iz, Nz - 1 - iz};
         for (int f = 0; f < 6; f++) if (d[f] < 16) hist[f][d[f]]++;
      }
      const int reach = triple ? 3 : 2; // how far the blocked kernel's own u^{n+1} (u^{n+2}) reach beyond the box, plus one
      auto margin = [&](int f, int64_t area) {
         int m = reach + 1;
         for (int d = 0; d <= 12; d++) if (hist[f][d] * 2 >= area) m = std::max(m, d + reach);
         return m;
      };
      constexpr int V = pf::VecOf<Real>::V;
      const int hl = (triple && V < 4) ? 2 : 1; // halo lanes per side of a row segment (k_tb3 in fp64: two, pf_tb3.h)
      // towards a neighbouring slab the box stops three planes short of the ghost plane: planes 1-2 / Nx-3..Nx-2 are the
      // edge planes of a split-phase pair (plane 1 needs the neighbour's data between the two steps; with plane 2 on the
      // edge stream as well the box kernel never reads a ghost plane, so the main stream never waits for an exchange)
      // (triples: the edge stream owns three planes per side, the box stops four short of the ghost plane)
      tbx0 = op.slab_first ? margin(0, NzNy) : reach + 1; tbx1 = (int)Nx - (op.slab_last ? margin(1, NzNy) : reach + 1);
      tby0 = margin(2, Nx * Nz); tby1 = (int)Ny - margin(3, Nx * Nz);
      const int mz0 = (margin(4, Nx * Ny) + 3) / 4 * 4, mz1 = (margin(5, Nx * Ny) + 3) / 4 * 4;
      tbz0 = mz0;
      tbzu0 = (int)margin(4, Nx * Ny); tbzu1 = (int)Nz - (int)margin(5, Nx * Ny);
      // row segments of 64 / 32 / 16 lanes (a wave stacks 1 / 2 / 4 of them in y): the width that needs the fewest lanes
      // for the box's z range (ties: the widest).  A last z tile with only a sliver of core columns costs a whole
      // workgroup per (row tile, x chunk) and re-reads lines the right column strip streams anyway: up to two 128-byte
      // lines of columns are left to the strip instead.
      {
         int64_t best = -1;
         for (int lw : {64, 32, 16}) {
            if (op.debug & (PF_DBG_LW32 | PF_DBG_LW16)) { if (lw != ((op.debug & PF_DBG_LW32) ? 32 : 16)) continue; } // tuning override (as pick_lw)
            else if (((op.debug & PF_DBG_LW64) || swz || triple) && lw != 64) continue; // (exchanged axes: the SWZ instantiations exist for 64-lane segments only; such rooms have long rows; k_tb3: 64 lanes)
            const int TC = (lw - 2 * hl) * V;
            int z1 = (int)((Nz - mz1) / 4 * 4);
            const int nz = z1 - tbz0, rem = nz % TC;
            if (nz > TC && rem > 0 && rem * (int)sizeof(Real) <= 256) z1 -= rem;
            if (z1 - tbz0 < TC / 2) continue;
            const int64_t lanes = cdiv(z1 - tbz0, TC) * lw;
            if (best < 0 || lanes < best) { best = lanes; tb_lw = lw; tbz1 = z1; }
         }
         if (best < 0) return PF_OK; // no room for a single row segment
      }
      // Wall regions (init_walls): a column strip costs one 128-byte line per row whatever its width, but its pencils live in
      // registers -- a sliver cut off the box is shared between the two strips instead of all going to the right one.
      if (!fcc && !(op.debug & PF_DBG_NO_WALL_REGIONS)) { // (slab engines too: init_walls(true))
         const int z1full = (int)((Nz - mz1) / 4 * 4);
         if (tbz1 < z1full) {
            const int rem = z1full - tbz1;
            // (the shift that lets both strips become wall regions with the fewest pencils cut in two; else the most even one)
            const bool ps = (op.debug & PF_DBG_STRIPS_SPLIT) != 0 || sizeof(Real) != 4;
            int best_sh = 0, best_need = 1 << 30;
            for (int sh = 0; sh <= rem; sh += 4) {
               const int lo = wl_lo_option(tbz0 + sh, ps), hi = wl_hi_option(tbz1 + sh, ps);
               int need = std::max(tbz0 + sh + 2, (int)Nz - ((tbz1 + sh - 2) / 4 * 4));
               need += (lo && hi) ? ((lo == 2) + (hi == 2)) * 100 : 1000;
               if (need < best_need) { best_need = need; best_sh = sh; }
            }
            tbz0 += best_sh; tbz1 += best_sh;
         }
      }
      szl = tbz0; szr = tbz1; // (widened to whole 128-byte lines or 32-byte sectors, the overlap with the box computed twice: 0-2 % slower, re-measured with the grids placed)
      if (vbase == 41) tbx1 = tbx0; // driver test: everything goes through the out-of-place single-step path
      tb_xr.clear();
      // rows of a workgroup: 4 waves x R = 3 (7-point); 13-point: 6 inner waves x R = 2 with 64-lane segments (k_tb2_fcc_x), else 4 x 2
      const int TC = (tb_lw - 2 * hl) * V, TR = triple ? tb3_rows : (fcc ? ((tb_lw == 64 && fcc_wt) ? 2 * (fcc_wt - 2) : 8 * (64 / tb_lw)) : 12 * (64 / tb_lw));
      int64_t vol = 0;
      if (tbx1 - tbx0 >= 16 && tby1 - tby0 >= 24 && tbz1 - tbz0 >= TC / 2) {
         tb_xr.push_back({tbx0, tbx1});
         const int np = tbx1 - tbx0;
         // ~16-plane chunks, even split (tools/tb2_probe.py); 13-point: ~24 (3.93 vs 4.07 ms per launch at 1024^3, 32-48 the same)
         // (k_tb3: 64 -- 3.28 ms per launch at 1024^3 against 3.57 with 32 and 3.63 with 16 in the plain tile order, tools/tb3_probe.py)
         // -- but a thin slab needs enough workgroups to fill the chip: at least ~1024 tiles, chunks of 16 planes or more (a rank of 8 at
         // 1024^3: 125 box planes in 2 chunks of 63 were 408 workgroups on 256 CUs)
         int want_chunk = fcc ? 24 : tb2_chunk;
         if (triple) {
            const int64_t tiles_yz = cdiv(tby1 - tby0, TR) * cdiv(tbz1 - tbz0, TC);
            want_chunk = (int)std::min<int64_t>(64, std::max<int64_t>(16, np / std::max<int64_t>(cdiv(1024, std::max<int64_t>(tiles_yz, 1)), 1)));
         }
         tb_chunk = (int)cdiv(np, std::max<int64_t>(cdiv(np, want_chunk), 1));
         tb_nxc = (int)cdiv(np, tb_chunk); tb_nyt = (int)cdiv(tby1 - tby0, TR); tb_nzt = (int)cdiv(tbz1 - tbz0, TC);
         const int64_t ntile = (int64_t)tb_nxc * tb_nyt * tb_nzt;
         if (ntile >= ((int64_t)1 << 31)) return PF_OK;
         std::vector<uint8_t> dirty((size_t)ntile, 0);
         // every tile whose core, grown by `grow` cells, holds this cell (pairs: one cell -- the kernel's own u^{n+1} reach one cell
         // beyond the core; triples: two)
         auto mark = [&](int64_t ii, int grow) {
            int64_t ix64, iy64, iz64;
            decode(ii, ix64, iy64, iz64);
            const int ix = (int)ix64, iy = (int)iy64, iz = (int)iz64;
            auto span = [grow](int c, int org, int size, int n, int end, int &lo, int &hi) {
               if (c < org - grow || c > end - 1 + grow) return false;
               lo = (c - grow - org) >= 0 ? (c - grow - org) / size : 0;
               hi = std::min(std::max(c + grow - org, 0) / size, n - 1);
               return lo <= hi;
            };
            int x0, x1, y0, y1, z0, z1;
            if (!span(ix, tbx0, tb_chunk, tb_nxc, tbx1, x0, x1) || !span(iy, tby0, TR, tb_nyt, tby1, y0, y1) ||
                !span(iz, tbz0, TC, tb_nzt, tbz1, z0, z1)) return;
            for (int a = x0; a <= x1; a++) for (int b = y0; b <= y1; b++) for (int c = z0; c <= z1; c++)
               dirty[((size_t)a * tb_nyt + b) * tb_nzt + c] = 1;
         };
         const int grow = triple ? 2 : 1;
         for (int64_t i = 0; i < Nb; i++) mark(sd.bn_ixyz[i], grow);
         // Sources and receivers.  Pairs: the tiles within reach of a source step singly (the source is added between the
         // steps, by k_io), and so does a receiver's tile under k_tb3 (it reads u^{n+1} from memory, which a clean tile of k_tb3 never
         // stores).  Round 6, triples (single domains and slabs of a chain): a receiver's tile merely STORES its u^{n+1} (the flag its neighbours of
         // single-step tiles carry), and the tiles within two cells of a source run k_tb3<..., SRC>, which adds the samples in registers --
         // unless a source sits in a tile that geometry keeps stepping singly (then k_io must add it in memory, and does so for all).
         // Without geometry inside the box no tile steps singly any more: the serial tail of a triple (two single steps of the source's
         // tile, each with its k_io behind it) is two receiver readouts.  debug PF_DBG_SRC_TILES_SINGLE: as before.
         std::vector<uint8_t> srcm, rcvm;
         bool src_tiles = triple && Ns > 0 && Ns <= pf::TB3_MAXSRC && !(op.debug & PF_DBG_SRC_TILES_SINGLE); // (slabs of a chain too: a rank whose source tile steps singly was the slowest of its chain)
         if (src_tiles) {
            std::vector<uint8_t> geo(dirty);
            std::fill(dirty.begin(), dirty.end(), 0);
            for (int64_t i = 0; i < Ns; i++) mark(sd.in_ixyz[i], 0); // the tiles whose core holds a source
            bool inside = true; // every source in a tile of the box, none of them in a tile that steps singly
            int64_t ncore = 0;
            for (int64_t t = 0; t < ntile; t++) { if (dirty[t]) { ncore++; if (geo[t]) inside = false; } }
            if (ncore == 0) inside = false;
            for (int64_t i = 0; i < Ns && inside; i++) {
               int64_t ix, iy, iz;
               decode(sd.in_ixyz[i], ix, iy, iz);
               if (ix < tbx0 || ix >= tbx1 || iy < tby0 || iy >= tby1 || iz < tbz0 || iz >= tbz1) inside = false;
            }
            std::fill(dirty.begin(), dirty.end(), 0);
            if (inside) {
               for (int64_t i = 0; i < Ns; i++) mark(sd.in_ixyz[i], grow);
               srcm = dirty;
            } else src_tiles = false;
            dirty = geo;
         }
         if (!src_tiles) for (int64_t i = 0; i < Ns; i++) mark(sd.in_ixyz[i], grow); // (the source is added between the steps)
         if (triple && !(op.debug & PF_DBG_SRC_TILES_SINGLE)) {
            std::vector<uint8_t> geo(dirty);
            std::fill(dirty.begin(), dirty.end(), 0);
            for (int64_t i = 0; i < Nr; i++) mark(sd.out_ixyz[i], 0);
            rcvm = dirty;
            dirty = geo;
         } else if (triple)
            for (int64_t i = 0; i < Nr; i++) mark(sd.out_ixyz[i], 0);
         std::vector<int32_t> cl, di, sr;
         for (int64_t t = 0; t < ntile; t++) {
            if (dirty[t]) { di.push_back((int32_t)t); continue; }
            if (!srcm.empty() && srcm[t]) sr.push_back((int32_t)t); else cl.push_back((int32_t)t);
            const int zt = (int)(t % tb_nzt), yt = (int)((t / tb_nzt) % tb_nyt), xc = (int)(t / ((int64_t)tb_nzt * tb_nyt));
            vol += (int64_t)(std::min(tbx0 + (xc + 1) * tb_chunk, tbx1) - (tbx0 + xc * tb_chunk)) *
                   (std::min(tby0 + (yt + 1) * TR, tby1) - (tby0 + yt * TR)) * (std::min(tbz0 + (zt + 1) * TC, tbz1) - (tbz0 + zt * TC));
         }
         tb_order_band = true;
         if (tb_order_band && !cl.empty()) {
            // XCD-banded order: hardware places block b on XCD b % 8; each XCD gets a contiguous band of the clean tiles of
            // every x chunk (tiles that share halo rows then share an L2), blocks b .. b+7 walking the 8 bands in step.
            // Measured at 1024^3, alternating runs on one box: k_tb2_reg 3.258 vs 3.295 ms per launch, whole step 427.3 vs
            // 422.2 Gvox/s; 13-point 3.94 vs 3.98 ms.  (Round 1's in-kernel band mapping of the dense grid was 6 % SLOWER:
            // it kept all XCDs on one x chunk with a rounded-up band size; here the list is simply permuted on the host.)
            std::vector<int32_t> out;
            out.reserve(cl.size());
            size_t i0 = 0;
            const int64_t per_chunk = (int64_t)tb_nyt * tb_nzt;
            while (i0 < cl.size()) {
               size_t i1 = i0;
               const int64_t xc = cl[i0] / per_chunk;
               while (i1 < cl.size() && cl[i1] / per_chunk == xc) i1++;
               const size_t n = i1 - i0, per = (n + 7) / 8;
               for (size_t p2 = 0; p2 < per; p2++)
                  for (size_t k = 0; k < 8; k++) { // balanced bands [k n / 8, (k+1) n / 8)
                     const size_t j0 = k * n / 8, j1 = (k + 1) * n / 8;
                     if (p2 < j1 - j0) out.push_back(cl[i0 + j0 + p2]);
                  }
               i0 = i1;
            }
            cl.swap(out);
         }
         tb_nclean = (int64_t)cl.size(); tb_ndirty = (int64_t)di.size(); tb_clean_cells = vol;
         int rc;
         mem.release(tb_clean); mem.release(tb_dirty); // (a second geometry: both tables go before either is replaced -- the order of a creation's allocations is part of where its grids land)
         {
            // k_tb3 keeps u^{n+1} on the chip: the clean neighbours of a tile that steps singly (26-neighbourhood) are flagged to
            // store theirs, which that tile's second step reads
            auto flag_rims = [&](std::vector<int32_t> &v) {
               if (!triple) return;
               for (auto &t : v) {
                  const int zt = (int)(t % tb_nzt), yt = (int)((t / tb_nzt) % tb_nyt), xc = (int)(t / ((int64_t)tb_nzt * tb_nyt));
                  bool rim = !rcvm.empty() && rcvm[(size_t)t] != 0; // (a receiver reads its u^{n+1} from memory)
                  if (tb_ndirty > 0)
                     for (int a = std::max(xc - 1, 0); a <= std::min(xc + 1, tb_nxc - 1) && !rim; a++)
                        for (int b = std::max(yt - 1, 0); b <= std::min(yt + 1, tb_nyt - 1) && !rim; b++)
                           for (int c = std::max(zt - 1, 0); c <= std::min(zt + 1, tb_nzt - 1) && !rim; c++)
                              rim = dirty[((size_t)a * tb_nyt + b) * tb_nzt + c] != 0;
                  if (rim) t = (int32_t)((uint32_t)t | pf::TB3_RIM);
               }
            };
            std::vector<int32_t> clf(cl);
            flag_rims(clf);
            if ((rc = upload(&tb_clean, clf.data(), tb_nclean))) return rc;
            mem.release(tb_srct);
            tb_nsrct = (int64_t)sr.size();
            if (tb_nsrct > 0) {
               flag_rims(sr);
               if ((rc = upload(&tb_srct, sr.data(), tb_nsrct))) return rc;
            }
         }
         if ((rc = upload(&tb_dirty, di.data(), tb_ndirty))) return rc;
         { // The placement search times the pair kernel on a SAMPLE of the clean tiles: every k-th x chunk, whole chunks in the
           // launch's own order (the effect it looks for is a property of how the four grids' pages lie relative to each
           // other, the same all along x), so a candidate costs 1/k of a launch (k = 4).
            int k = 4;
            if (tb_nxc < 8 * k) k = std::max(tb_nxc / 8, 1);
            std::vector<int32_t> sm;
            int64_t svol = 0;
            const int64_t per_chunk = (int64_t)tb_nyt * tb_nzt;
            for (int32_t t : cl) {
               const int xc = (int)(t / per_chunk);
               if (xc % k != k / 2) continue;
               sm.push_back(t);
               const int zt = (int)(t % tb_nzt), yt = (int)((t / tb_nzt) % tb_nyt);
               svol += (int64_t)(std::min(tbx0 + (xc + 1) * tb_chunk, tbx1) - (tbx0 + xc * tb_chunk)) *
                       (std::min(tby0 + (yt + 1) * TR, tby1) - (tby0 + yt * TR)) * (std::min(tbz0 + (zt + 1) * TC, tbz1) - (tbz0 + zt * TC));
            }
            mem.release(tb_sample);
            tb_nsample = 0; tb_sample_frac = 1.0;
            if (k > 1 && !sm.empty() && vol > 0) {
               tb_nsample = (int64_t)sm.size(); tb_sample_frac = (double)svol / (double)vol;
               if ((rc = upload(&tb_sample, sm.data(), tb_nsample))) return rc;
            }
         }
         if (tb_nclean == 0) tb_xr.clear();
         if (fcc && !tb_xr.empty()) {
            // the single-step kernel's own tiling of the box's planes: 256 (fp64: 128) columns x 16 rows x the same x
            // chunks; a tile is needed unless every interior cell of it between the column strips lies in a clean core
            sh_nzt = (int)cdiv(P, 64 * V); sh_nyt = (int)cdiv(Ny - 2, 16);
            std::vector<int32_t> sh;
            for (int xc = 0; xc < tb_nxc; xc++)
               for (int yt = 0; yt < sh_nyt; yt++)
                  for (int zt = 0; zt < sh_nzt; zt++) {
                     const int ya = 1 + yt * 16, yb = std::min(ya + 16, (int)Ny - 1);
                     const int za = std::max(zt * 64 * V, tbz0), zb = std::min((zt + 1) * 64 * V, tbz1);
                     if (za >= zb) continue; // only column-strip cells: k_zstrip_fcc
                     bool need = ya < tby0 || yb > tby1;
                     // (Stepping the box's dirty tiles tile for tile, with the pair kernel's 12-row geometry, was measured in round 5 and
                     // LOSES: Musikverein, 28 % of the cells dirty, 4.11 ms per step against 3.80 with these 16-row tiles -- two rows per
                     // wave fetch twice the lines per cell.  Second attempt, k_air_fcc itself with three rows per lane started at the pair
                     // tiles' origins, exactly the dirty tiles: 4.12 against 4.07 on one box.  Scattered tiles are slow whatever their
                     // shape: the cells they cover are not what costs.)
                     if (!need) {
                        const int t0y = (ya - tby0) / TR, t1y = (yb - 1 - tby0) / TR, t0z = (za - tbz0) / TC, t1z = (zb - 1 - tbz0) / TC;
                        for (int a = t0y; a <= t1y && !need; a++)
                           for (int c = t0z; c <= t1z && !need; c++) need = dirty[((size_t)xc * tb_nyt + a) * tb_nzt + c] != 0;
                     }
                     if (need) sh.push_back((int32_t)(((int64_t)xc * sh_nyt + yt) * sh_nzt + zt));
                  }
            sh_ntiles = (int64_t)sh.size();
            if ((rc = upload(&sh_tiles, sh.data(), sh_ntiles))) return rc;
         }
      }
      if (triple && vol == 0) return PF_OK; // (every 20-row tile holds a receiver, a source or geometry: init_tb2 tries the pairs' smaller tiles)
      if (vbase == 40 && vol == 0) return set_err(PF_ERR_ARG, "air_variant %d (temporal blocking) requested but the scene has no boundary-free tiles", op.air_variant & 255);
      // auto: the shell costs grow with the perimeter of the y-z cross-section, the gain with its area -- measured on
      // MI355X: 512^2 planes -4.5 %, 768^2 +9 %, 1024^2 +13 % for a box room; and two extra grids must be worth it.
      // Single-domain engines then time a blocked pair against the single-step kernels at creation (autotune()), so the
      // static rule only has to exclude the hopeless cases; slab engines have no such measurement and keep the strict one.
      if (vbase == 0 && single && ((double)vol < (fcc ? 0.5 : 0.35) * (double)(Nx * Ny * Nz) || tby1 - tby0 < 100 || tbz1 - tbz0 < 100)) return PF_OK;
      if (vbase == 0 && !single && ((double)vol < 0.6 * (double)(Nx * Ny * Nz) || tby1 - tby0 < 600 || tbz1 - tbz0 < 600)) return PF_OK;
      tb2_geom = true;
      if (!single) return PF_OK; // slab engines wait for pf_engine_set_spares (all four grids must be the caller's)
      int rc;
      bufC = try_dzalloc<Real>(npad);
      bufD = bufC ? try_dzalloc<Real>(npad) : nullptr;
      if (!bufD) { // no room for two more grids (state > ~45 % of the device memory): keep stepping singly
         mem.release(bufC);
         tb2_geom = false;
         return PF_OK;
      }
      if (triple) {
         bufE = try_dzalloc<Real>(npad);
         if (!bufE) return PF_OK; // (no room for a fifth grid: init_tb2 falls back to pairs)
      }
      tb2 = true;
      { int rcw = init_walls(); if (rcw) return rcw; }
      if (triple) return PF_OK; // (with wall regions: triples; without: init_tb2 starts over with the pairs' geometry)
      if (wl_on) { zs_mode = 0; return PF_OK; } // (no single-step shell: nothing for the column-strip kernel to share)
      // Boundary nodes inside the column strips are updated by k_air_zstrip, which streams their lines anyway and holds
      // their six neighbours in registers (in k_boundary the floor / ceiling nodes of a box room -- stride-P neighbours,
      // one 128-byte line of u1 and of u0 per two nodes -- cost half of the pass: 0.30 of 0.63 ms at 1024^3).  The strip
      // kernel does the RIGID update only and leaves the result in u0b[li]; the branch ODEs of the lossy ones follow in
      // extra threads of the k_boundary launch, dense over the compact arrays (mode 2).  (Doing the ODEs inside the strip kernel as well was bit-identical
      // but slower -- they ran on the few lanes per wave that hold a node, 2.92 vs 2.59 ms per step -- and was retired.)
      // PF_DBG_BND_ALL_NODES: mode 0, the list kernel visits every boundary node (the round-1 arrangement; also the fallback).
      zs_mode = fcc ? 0 : ((op.debug & PF_DBG_BND_ALL_NODES) ? 0 : 2);
      if (Nb > 0 && !tb_xr.empty() && zs_mode == 2 && Nbl < ((int64_t)1 << 31)) {
         const int xb = tb_xr.front().first, xe = tb_xr.back().second;
         constexpr int V = pf::VecOf<Real>::V;
         const int nl = szl / V, nv = nl + (int)(P - szr) / V;
         std::vector<int64_t> hb(Nb);
         HIPCHK(hipMemcpy(hb.data(), d_bn, Nb * sizeof(int64_t), hipMemcpyDeviceToHost));
         std::vector<int32_t> hl(Nb), rest, sli, fd;
         std::vector<uint16_t> hadj(Nb), sadj;
         HIPCHK(hipMemcpy(hl.data(), d_lossy, Nb * sizeof(int32_t), hipMemcpyDeviceToHost));
         HIPCHK(hipMemcpy(hadj.data(), d_adj, Nb * sizeof(uint16_t), hipMemcpyDeviceToHost));
         // The boundary list is sorted by cell, so its strip nodes come in strip order (x, y, z): node k of the strips is the
         // k-th of them; a vector's record holds the number of its first node and one bit per cell with a node.
         std::vector<uint32_t> zv((size_t)(Nx * Ny * nv), 0u);
         rest.reserve(Nb);
         bool sorted = true;
         int64_t prev = -1;
         for (int64_t nb = 0; nb < Nb; nb++) {
            const int64_t ix = hb[nb] / plane, rem = hb[nb] % plane, iy = rem / P, iz = rem % P;
            const bool in_strip = ix >= xb && ix < xe && (iz < szl || iz >= szr);
            if (!in_strip) { rest.push_back((int32_t)nb); continue; }
            if (hb[nb] <= prev) { sorted = false; break; }
            prev = hb[nb];
            const int64_t v = iz < szl ? iz / V : nl + (iz - szr) / V, i = iz < szl ? iz % V : (iz - szr) % V;
            uint32_t &rec = zv[(size_t)((ix * Ny + iy) * nv + v)];
            if ((rec & 15u) == 0) rec = (uint32_t)sadj.size() << 4;
            rec |= 1u << i;
            sadj.push_back(hadj[nb]);
            sli.push_back(hl[nb]);
            if (hl[nb] >= 0) fd.push_back(hl[nb]);
         }
         if (!sorted || sadj.size() >= ((size_t)1 << 28)) zs_mode = 0; // (the engine sorts its lists: never seen)
         else {
            zs_nrest = (int64_t)rest.size();
            if ((rc = upload(&zs_map, zv.data(), (int64_t)zv.size()))) return rc;
            if ((rc = upload(&zs_adj, sadj.data(), (int64_t)sadj.size()))) return rc;
            if ((rc = upload(&zs_li, sli.data(), (int64_t)sli.size()))) return rc;
            if ((rc = upload(&zs_rest, rest.data(), zs_nrest))) return rc;
            zs_nfd = (int64_t)fd.size();
            if ((rc = upload(&zs_fd, fd.data(), zs_nfd))) return rc;
         }
      } else zs_mode = 0;
      return PF_OK;
   }

