// absorb_cut_check.cpp -- the chain's merge of the wall absorption maps (pffdtd_amd/csrc/pf_absorb_cut.h over the slabs of pf_slab_cut.h) on a small
// scene built in memory, as a program of its own: tests/test_absorb_cut.py compiles it with the host compiler under the address and
// undefined-behaviour sanitizers and runs it once.  Prints the violated condition on stderr and returns non-zero.
//
// Scene: 13 x 9 x 14 cells, an unsorted list of 180 frequency-dependent nodes, the ABC nodes of the whole interior shell (every interior cell with a
// coordinate 1 or N - 2, the planes next to each cut's ghost planes among them) and a source in every interior plane of both cut axes.  For
// G = 1, 2, 3, both cut axes:
//   * node rows scattered by Slab::bnl_rows and gathered back give the identity, and a gather alone fills every row exactly once;
//   * every ABC node and every source is in exactly one slab's list (the slab that OWNS its plane, never through a ghost plane), with its Q and signal;
//   * the bins added in slab order are the plain sum, and a set's split (the scene's bins to slab 0, zeros to the others) adds up to the same doubles.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "pf_absorb_cut.h"
#include "pf_slab_cut.h"

namespace {

int g_bad = 0;
char g_ctx[128] = "";
void check(bool ok, const char *fmt, ...) {
   if (ok) return;
   g_bad++;
   fprintf(stderr, "absorb_cut_check [%s]: ", g_ctx);
   va_list ap;
   va_start(ap, fmt);
   vfprintf(stderr, fmt, ap);
   va_end(ap);
   fprintf(stderr, "\n");
}

struct Scene {
   static constexpr int64_t Nx = 13, Ny = 9, Nz = 14, Nt = 3;
   std::vector<int64_t> bn, bnl, bna, in, out, reorder;
   std::vector<uint16_t> adj;
   std::vector<int8_t> mat, Q, Mb{3, 11, 5};
   std::vector<float> ssaf;
   std::vector<double> sigs, u_out;
   pf_simdata sd{};
   uint64_t state = 0x9E3779B97F4A7C15ull;
   uint64_t rnd() { state = state * 6364136223846793005ull + 1442695040888963407ull; return state >> 33; }
   int64_t cell(int64_t x, int64_t y, int64_t z) const { return x * Ny * Nz + y * Nz + z; }
   Scene() {
      bnl.resize(180);
      for (auto &v : bnl) v = cell(1 + (int64_t)(rnd() % (Nx - 2)), 1 + (int64_t)(rnd() % (Ny - 2)), 1 + (int64_t)(rnd() % (Nz - 2)));
      bn = bnl;
      adj.assign(bn.size(), 0x15);
      mat.resize(bnl.size());
      for (auto &v : mat) v = (int8_t)(rnd() % 3);
      ssaf.assign(bnl.size(), 1.0f);
      for (int64_t x = 1; x < Nx - 1; x++)
         for (int64_t y = 1; y < Ny - 1; y++)
            for (int64_t z = 1; z < Nz - 1; z++) {
               const int q = (x == 1 || x == Nx - 2) + (y == 1 || y == Ny - 2) + (z == 1 || z == Nz - 2);
               if (q) { bna.push_back(cell(x, y, z)); Q.push_back((int8_t)q); }
            }
      for (int64_t x = 1; x < Nx - 1; x++) in.push_back(cell(x, 4, 2 + x % 3));
      for (int64_t z = 1; z < Nz - 1; z++) in.push_back(cell(2 + z % 3, 5, z));
      for (size_t i = 0; i < in.size(); i++)
         for (int64_t n = 0; n < Nt; n++) sigs.push_back((double)(100 * i + n)); // (a source's row names it)
      out = {cell(7, 4, 8)};
      reorder = {0};
      u_out.assign(out.size() * (size_t)Nt, 0.0);
      sd.bn_ixyz = bn.data(); sd.adj_bn = adj.data(); sd.Nb = (int64_t)bn.size();
      sd.bnl_ixyz = bnl.data(); sd.mat_bnl = mat.data(); sd.ssaf_bnl = ssaf.data(); sd.Nbl = (int64_t)bnl.size();
      sd.bna_ixyz = bna.data(); sd.Q_bna = Q.data(); sd.Nba = (int64_t)bna.size();
      sd.in_ixyz = in.data(); sd.in_sigs = sigs.data(); sd.Ns = (int64_t)in.size();
      sd.out_ixyz = out.data(); sd.out_reorder = reorder.data(); sd.u_out = u_out.data(); sd.Nr = (int64_t)out.size();
      sd.Nt = Nt; sd.Nx = Nx; sd.Ny = Ny; sd.Nz = Nz; sd.Npts = Nx * Ny * Nz;
      sd.Nm = 3; sd.Mb = Mb.data(); sd.NN = 6; sd.real_bytes = 4;
   }
};

void check_chain(Scene &sc, int G, bool along_z) {
   const pf_simdata *sd = &sc.sd;
   std::vector<int64_t> cuts;
   const char *msg = pf_cut::partition(sd, G, true, cuts, along_z);
   check(msg == nullptr, "partition: %s", msg ? msg : "");
   if (msg) return;
   std::vector<pf_cut::Slab> slabs(G);
   for (int g = 0; g < G; g++) {
      msg = pf_cut::cut_slab(sd, cuts, g, G, slabs[g], along_z);
      check(msg == nullptr, "cut_slab %d: %s", g, msg ? msg : "");
      if (msg) return;
   }
   // node rows: scatter + gather = identity; a gather fills every row once
   std::vector<double> x((size_t)sd->Nbl), y((size_t)sd->Nbl, -1.0);
   for (auto &v : x) v = 1.0 + (double)(sc.rnd() % 1000);
   std::vector<int> filled((size_t)sd->Nbl, 0);
   for (int g = 0; g < G; g++) {
      const pf_cut::Slab &s = slabs[g];
      std::vector<double> loc(s.bnl_rows.size(), 0.0);
      pf_cut::scatter_rows(s, x.data(), loc.data());
      for (size_t i = 0; i < loc.size(); i++) check(loc[i] == x[(size_t)s.bnl_rows[i]], "slab %d: local row %zu is not scene row %ld", g, i, (long)s.bnl_rows[i]);
      pf_cut::gather_rows(s, loc.data(), y.data());
      for (int64_t r : s.bnl_rows) filled[(size_t)r]++;
   }
   check(x == y, "gather(scatter(nodes)) != nodes");
   for (int64_t r = 0; r < sd->Nbl; r++) check(filled[(size_t)r] == 1, "node row %ld is filled by %d slabs", (long)r, filled[(size_t)r]);
   // every ABC node and every source: exactly one slab, the owner of its plane, with its Q / its signal
   const int64_t N = along_z ? sc.Nz : sc.Nx;
   auto plane_of = [&](int64_t ii) { return along_z ? ii % sc.Nz : ii / (sc.Ny * sc.Nz); };
   std::vector<int> na((size_t)sd->Nba, 0), ns((size_t)sd->Ns, 0);
   for (int g = 0; g < G; g++) {
      const pf_cut::Slab &s = slabs[g];
      check(s.bna.size() == s.Q.size() && s.in_sigs.size() == s.in.size() * (size_t)sc.Nt, "slab %d: list sizes", g);
      for (size_t i = 0; i < s.bna.size(); i++) {
         const int64_t ii = pf_cut::scene_index(sd, s, along_z, s.bna[i]), p = plane_of(ii);
         check(p >= s.x0 && p < s.x1, "slab %d counts ABC cell %ld of plane %ld, which it does not own ([%ld, %ld))", g, (long)ii, (long)p, (long)s.x0, (long)s.x1);
         bool found = false;
         for (int64_t j = 0; j < sd->Nba; j++) if (sd->bna_ixyz[j] == ii) { na[(size_t)j]++; found = true; check(s.Q[i] == sd->Q_bna[j], "slab %d: Q of ABC cell %ld", g, (long)ii); }
         check(found, "slab %d: ABC cell %ld is none of the scene's", g, (long)ii);
      }
      for (size_t i = 0; i < s.in.size(); i++) {
         const int64_t ii = pf_cut::scene_index(sd, s, along_z, s.in[i]), p = plane_of(ii);
         check(p >= s.x0 && p < s.x1, "slab %d counts the source at %ld of plane %ld, which it does not own", g, (long)ii, (long)p);
         const int64_t j = (int64_t)(s.in_sigs[i * (size_t)sc.Nt] / 100.0);
         check(j >= 0 && j < sd->Ns && sd->in_ixyz[j] == ii, "slab %d: source %zu carries the signal of another cell", g, i);
         if (j >= 0 && j < sd->Ns) ns[(size_t)j]++;
      }
   }
   for (int64_t j = 0; j < sd->Nba; j++) check(na[(size_t)j] == 1, "ABC node %ld (plane %ld of %ld) is counted by %d slabs", (long)j, (long)plane_of(sd->bna_ixyz[j]), (long)N, na[(size_t)j]);
   for (int64_t j = 0; j < sd->Ns; j++) check(ns[(size_t)j] == 1, "source %ld (plane %ld) is counted by %d slabs", (long)j, (long)plane_of(sd->in_ixyz[j]), ns[(size_t)j]);
   // bins: slab order, and a set's split
   const int64_t nb = 7;
   std::vector<std::vector<double>> part((size_t)G, std::vector<double>((size_t)nb));
   std::vector<double> sum((size_t)nb, 0.0), plain((size_t)nb, 0.0);
   for (int g = 0; g < G; g++)
      for (auto &v : part[(size_t)g]) v = 1e-3 * (double)(sc.rnd() % 100000);
   for (int g = 0; g < G; g++) pf_cut::add_bins(sum.data(), part[(size_t)g].data(), nb);
   for (int64_t k = 0; k < nb; k++) { for (int g = 0; g < G; g++) plain[(size_t)k] += part[(size_t)g][(size_t)k]; }
   check(sum == plain, "add_bins in slab order is not the plain sum");
   std::vector<double> again((size_t)nb, 0.0), zeros((size_t)nb, 0.0);
   for (int g = 0; g < G; g++) pf_cut::add_bins(again.data(), g ? zeros.data() : sum.data(), nb);
   check(again == sum, "a set's split does not add up to the same doubles");
}

} // namespace

int main() {
   for (int G : {1, 2, 3})
      for (int along_z = 0; along_z < 2; along_z++) {
         snprintf(g_ctx, sizeof g_ctx, "G=%d cut along %s", G, along_z ? "z" : "x");
         Scene sc;
         check_chain(sc, G, along_z != 0);
      }
   if (g_bad) fprintf(stderr, "absorb_cut_check: %d condition(s) violated\n", g_bad);
   return g_bad ? 1 : 0;
}
