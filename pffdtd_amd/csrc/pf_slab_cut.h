// pf_slab_cut.h -- how a scene becomes the local problems of a chain of slabs: owned plane ranges (partition) and the lists cut to
// them, indices re-based (cut_slab).  Replaces gpu_engine.h:516-662 (split_data) and :784-823 (index localisation) of the reference.
// HOST ONLY: the public header and the standard library, no device, no RCCL, no error state -- a function that can fail returns its
// message (nullptr: fine) and pf_multi.hip feeds it to pf_last_error; tests/slab_cut_check.cpp includes this file as it is.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "pffdtd_hip.h"

namespace pf_cut {

struct Slab {
   int64_t x0 = 0, x1 = 0;       // owned global planes [x0, x1)
   int64_t xlo = 0, xhi = 0;     // global planes held locally [xlo, xhi): owned + one ghost plane per interior side
   bool first = false, last = false;
   // host arrays of the local pf_simdata
   std::vector<int64_t> bn, bnl, bna, in, out, out_reorder, out_rows;
   std::vector<int64_t> bnl_rows; // per local lossy entry: its row in the scene's bnl_ixyz (pf_state_cut.h: the canonical node state goes by those rows)
   std::vector<uint16_t> adj;
   std::vector<int8_t> K, matl, Q;
   std::vector<uint8_t> ssaf; // Real bytes
   std::vector<double> in_sigs, u_out;
   pf_simdata sd{};
};

// owned plane ranges.  even: Nx/G planes each, +1 for the first Nx%G (gpu_engine.h:532-550).  balanced: equal estimated
// cost (interior plane = 1; a full plane of lossy nodes with 11 branches = 23, of rigid nodes = 5: measured on MI355X -- round 4,
// 1024^3 as 8 ranks with wall regions in the slabs: 132 interior planes 0.310 ms per step; 119 / 114 planes + an x wall, which stays
// single steps, 0.337 / 0.329 -- an end rank is mostly fixed cost, 0.0014 ms per plane against 0.0024 inside)
// along_z: the chain is cut along FILE Z instead (slab engines then store the grid with the x and z axes exchanged: Engine::swz)
// wall_scale: the wall planes' weights (23 / 5 interior planes per full plane of lossy / rigid nodes, a fit at 1024^2 planes, Mb = 11, fp32) times
// this factor -- 1: the constants as they are; pf_multi_create MEASURES the factor on the scene at hand (slab_wall_scale_x, round 5).
// wall1 (optional): the per-plane wall cost at scale 1, in interior planes.
inline const char *partition(const pf_simdata *sd, int G, bool even, std::vector<int64_t> &cuts, bool along_z = false, double wall_scale = 1.0,
                             std::vector<double> *wall1 = nullptr) {
   const int64_t Nx = along_z ? sd->Nz : sd->Nx; // planes along the cut axis
   if (G < 1 || G >= Nx) return along_z ? "need 1 <= number of slabs < Nz: this scene's chain is cut along file z (the reference: ngpus < Nx, gpu_engine.h:682)"
                                        : "need 1 <= number of slabs < Nx (gpu_engine.h:682)";
   cuts.assign(G + 1, 0);
   cuts[G] = Nx;
   if (G == 1) return nullptr;
   if (even) {
      const int64_t base = Nx / G, rem = Nx % G;
      for (int g = 0; g < G; g++) cuts[g + 1] = cuts[g] + base + (g < rem ? 1 : 0);
      return nullptr;
   }
   const int64_t NzNy = along_z ? sd->Ny * sd->Nx : sd->Ny * sd->Nz; // cells per plane of the cut axis
   std::vector<double> nb(Nx, 0.0), nl(Nx, 0.0);
   auto plane_of = [&](int64_t ii) { return along_z ? ii % sd->Nz : ii / (sd->Ny * sd->Nz); };
   for (int64_t i = 0; i < sd->Nb; i++) nb[plane_of(sd->bn_ixyz[i])] += 1.0;
   for (int64_t i = 0; i < sd->Nbl; i++) nl[plane_of(sd->bnl_ixyz[i])] += 1.0;
   double mb_scale = 1.0;
   if (sd->Nbl > 0) {
      double s = 0;
      for (int64_t i = 0; i < sd->Nbl; i++) s += (double)sd->Mb[sd->mat_bnl[i]];
      mb_scale = s / (double)sd->Nbl / 11.0;
   }
   std::vector<double> cum(Nx + 1, 0.0);
   if (wall1) wall1->assign(Nx, 0.0);
   for (int64_t x = 0; x < Nx; x++) {
      double c = (x == 0 || x == Nx - 1) ? 0.0 : 1.0; // the global ghost planes are not updated
      const double wc = (23.0 * mb_scale * nl[x] + 5.0 * (nb[x] - nl[x])) / (double)NzNy;
      if (wall1) (*wall1)[x] = wc;
      c += wall_scale * wc;
      cum[x + 1] = cum[x] + c;
   }
   // Round 6: a cut keeps CUT_CLEAR planes from every source.  A slab in triples takes its shell's three steps in one pass, recomputing three
   // planes of halo beside its box -- which starts four planes from a cut -- from u^{n-1}, u^n alone: a source there (it is added between the
   // steps) would send the slab back to the two-steps-plus-one shell.  The headline scene's source sits at Nx / 2, exactly where an even
   // number of ranks cuts.
   constexpr int64_t CUT_CLEAR = 8;
   std::vector<int64_t> src_planes;
   for (int64_t i = 0; i < sd->Ns; i++) src_planes.push_back(plane_of(sd->in_ixyz[i]));
   auto clear_of_sources = [&](int64_t x) {
      for (int64_t p : src_planes) if (x > p - CUT_CLEAR && x <= p + CUT_CLEAR) return false; // (planes x-1 | x are the cut's two sides)
      return true;
   };
   auto nudge = [&](int64_t x, int64_t lo, int64_t hi) { // the nearest plane that is clear of every source, if the slab thicknesses allow one
      if (clear_of_sources(x)) return x;
      for (int64_t d = 1; d <= 2 * CUT_CLEAR + 2; d++) {
         if (x - d >= lo && clear_of_sources(x - d)) return x - d;
         if (x + d <= hi && clear_of_sources(x + d)) return x + d;
      }
      return x;
   };
   std::vector<char> pinned(G + 1, 0);
   bool any_pinned = false;
   for (int g = 1; g < G; g++) {
      const double target = cum[Nx] * (double)g / (double)G;
      int64_t x = (int64_t)(std::lower_bound(cum.begin(), cum.end(), target) - cum.begin());
      const int64_t lo = cuts[g - 1] + 2, hi = Nx - 2 * (int64_t)(G - g);
      x = std::max(x, lo);            // every slab updates at least one plane
      x = std::min(x, hi);
      const int64_t xn = nudge(x, lo, hi);
      if (xn != x) { pinned[g] = 1; any_pinned = true; }
      cuts[g] = xn;
   }
   // A cut that a source pushed aside leaves its two neighbours up to CUT_CLEAR planes apart (1024^3 as 8 ranks, source at Nx / 2: 125 and
   // 142 planes where 133 each was meant -- the thick one was the slowest rank of the chain): such a cut stays where it is and the ranks on
   // either side of it share THEIR part of the cost equally among themselves (four ranks over 504 planes, four over 520).
   if (any_pinned) {
      int a = 0;
      while (a < G) {
         int b = a + 1;
         while (b < G && !pinned[b]) b++;
         const double c0 = cum[cuts[a]], c1 = cum[cuts[b]];
         for (int g = a + 1; g < b; g++) {
            const double target = c0 + (c1 - c0) * (double)(g - a) / (double)(b - a);
            int64_t x = (int64_t)(std::lower_bound(cum.begin(), cum.end(), target) - cum.begin());
            const int64_t lo = cuts[g - 1] + 2, hi = cuts[b] - 2 * (int64_t)(b - g);
            x = std::min(std::max(x, lo), hi);
            cuts[g] = nudge(x, lo, hi);
         }
         a = b;
      }
   }
   return nullptr;
}

// local problem of slab g: lists cut to the planes it updates, indices re-based (gpu_engine.h:784-823).  Cut along x, the slab holds
// the file's planes [xlo, xhi) and its local file has Nx = xhi - xlo; cut along FILE Z (along_z), it holds the columns z in [xlo, xhi)
// of every row and its local file has Nz = xhi - xlo.  The axis enters through `within` and `local` alone; every list keeps the file's
// order (the engines sort their own, but a receiver's row and a source's signal go by position).
inline const char *cut_slab(const pf_simdata *sd, const std::vector<int64_t> &cuts, int g, int G, Slab &s, bool along_z = false) {
   const int64_t Nz = sd->Nz, NzNy = sd->Ny * Nz, Nt = sd->Nt, N = along_z ? Nz : sd->Nx;
   s.x0 = cuts[g]; s.x1 = cuts[g + 1];
   s.first = g == 0; s.last = g == G - 1;
   s.xlo = s.x0 - (s.first ? 0 : 1);
   s.xhi = s.x1 + (s.last ? 0 : 1);
   const int64_t upd0 = std::max<int64_t>(s.x0, 1), upd1 = std::min<int64_t>(s.x1, N - 1), nloc = s.xhi - s.xlo;
   if (upd1 - upd0 < 1) return "a slab must own at least one interior plane";
   auto within = [&](int64_t ii, int64_t p0, int64_t p1) { // is cell ii in the planes [p0, p1) of the cut axis?
      if (along_z) return ii % Nz >= p0 && ii % Nz < p1;
      return ii >= p0 * NzNy && ii < p1 * NzNy;
   };
   auto updates = [&](int64_t ii) { return within(ii, upd0, upd1); };
   auto owns = [&](int64_t ii) { return within(ii, s.x0, s.x1); };
   auto local = [&](int64_t ii) { return along_z ? (ii / Nz) * nloc + (ii % Nz - s.xlo) : ii - s.xlo * NzNy; };
   const int rb = sd->real_bytes;
   for (int64_t i = 0; i < sd->Nb; i++) {
      const int64_t ii = sd->bn_ixyz[i];
      if (!updates(ii)) continue;
      s.bn.push_back(local(ii));
      s.adj.push_back(sd->adj_bn[i]);
      if (sd->K_bn) s.K.push_back(sd->K_bn[i]);
   }
   for (int64_t i = 0; i < sd->Nbl; i++) {
      const int64_t ii = sd->bnl_ixyz[i];
      if (!updates(ii)) continue;
      s.bnl.push_back(local(ii));
      s.bnl_rows.push_back(i);
      s.matl.push_back(sd->mat_bnl[i]);
      const uint8_t *p = (const uint8_t *)sd->ssaf_bnl + (size_t)i * rb;
      s.ssaf.insert(s.ssaf.end(), p, p + rb);
   }
   for (int64_t i = 0; i < sd->Nba; i++) {
      const int64_t ii = sd->bna_ixyz[i];
      if (!updates(ii)) continue;
      s.bna.push_back(local(ii));
      s.Q.push_back(sd->Q_bna[i]);
   }
   for (int64_t i = 0; i < sd->Ns; i++) {
      const int64_t ii = sd->in_ixyz[i];
      if (!updates(ii)) continue;
      s.in.push_back(local(ii));
      s.in_sigs.insert(s.in_sigs.end(), sd->in_sigs + i * Nt, sd->in_sigs + (i + 1) * Nt);
   }
   // receivers read u1 at any owned plane (a global ghost plane included, should someone ask for it)
   for (int64_t i = 0; i < sd->Nr; i++) {
      const int64_t ii = sd->out_ixyz[i];
      if (!owns(ii)) continue;
      s.out.push_back(local(ii));
      s.out_rows.push_back(i);
   }
   s.out_reorder.resize(s.out.size());
   for (size_t i = 0; i < s.out.size(); i++) s.out_reorder[i] = (int64_t)i;
   s.u_out.assign(std::max<size_t>(s.out.size() * (size_t)Nt, 1), 0.0);
   // the ssaf vector must be Real-aligned: std::vector<uint8_t> storage is new[]-aligned (16 B), fine for float/double
   pf_simdata &l = s.sd;
   l = *sd;
   (along_z ? l.Nz : l.Nx) = nloc;
   l.Npts = l.Nx * l.Ny * l.Nz;
   l.bn_ixyz = s.bn.data(); l.adj_bn = s.adj.data(); l.K_bn = sd->K_bn ? s.K.data() : nullptr; l.Nb = (int64_t)s.bn.size();
   l.bnl_ixyz = s.bnl.data(); l.mat_bnl = s.matl.data(); l.ssaf_bnl = s.ssaf.data(); l.Nbl = (int64_t)s.bnl.size();
   l.bna_ixyz = s.bna.data(); l.Q_bna = s.Q.data(); l.Nba = (int64_t)s.bna.size();
   l.in_ixyz = s.in.data(); l.in_sigs = s.in_sigs.data(); l.Ns = (int64_t)s.in.size();
   l.out_ixyz = s.out.data(); l.out_reorder = s.out_reorder.data(); l.Nr = (int64_t)s.out.size();
   l.u_out = s.u_out.data();
   l.bn_mask = nullptr; // every engine rebuilds its own mask from its own boundary nodes (as gpu_engine.h:791)
   return nullptr;
}

} // namespace pf_cut
