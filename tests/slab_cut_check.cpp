// slab_cut_check.cpp -- the C chain's cut (pffdtd_amd/csrc/pf_slab_cut.h: partition + cut_slab) on a small scene built in memory, as a
// program of its own: tests/test_host.py compiles it with the host compiler under the address and undefined-behaviour sanitizers and
// runs it once.  Prints the violated condition on stderr and returns non-zero.
//
// Scene: 12 x 9 x 14 cells, unsorted lists of a few hundred entries each (every entry interior along x AND z, as the loader demands, so
// that either axis can be cut), two sources, five receivers -- one of them on a global ghost plane of both axes --, ssaf in fp32 and fp64.
// For G = 2, 3, 5, both axes, both split rules:
//   * every list entry lands in exactly one slab, and each slab's arrays (indices, adj, K, mat, ssaf bytes, Q, source rows) are the
//     originals' IN ORDER;
//   * every kept entry is interior to its slab along the cut axis (receivers: in its owned planes), and its local index maps back to
//     the global one;
//   * the slabs' out_rows together are 0 .. Nr-1 exactly once;
//   * the cuts increase strictly, at least two planes apart.
// Scenes of 100 x 9 x 100 cells whose sources leave the balanced split no plane CUT_CLEAR = 8 planes from all of them, or only a few -- a source
// in every interior plane; on every 6th plane (closer together than 2 * CUT_CLEAR); one band of 66 consecutive planes --, each list shuffled
// and with four nodes listed twice, for G = 2, 3, 8: the same conditions, so the slabs' source lists partition the scene's in file order
// (duplicates keep their order) and each signal row travels with its node.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "pf_slab_cut.h"

namespace {

int g_bad = 0;
char g_ctx[128] = "";
void check(bool ok, const char *fmt, ...) {
   if (ok) return;
   g_bad++;
   fprintf(stderr, "slab_cut_check [%s]: ", g_ctx);
   va_list ap;
   va_start(ap, fmt);
   vfprintf(stderr, fmt, ap);
   va_end(ap);
   fprintf(stderr, "\n");
}

struct Scene {
   static constexpr int64_t Nt = 6;
   const int64_t Nx, Ny, Nz;
   std::vector<int64_t> bn, bnl, bna, in, out, reorder;
   std::vector<uint16_t> adj;
   std::vector<int8_t> K, mat, Q, Mb{3, 11, 5};
   std::vector<uint8_t> ssaf;
   std::vector<double> sigs, u_out;
   pf_simdata sd{};
   uint64_t state = 0x9E3779B97F4A7C15ull;
   uint64_t rnd() { state = state * 6364136223846793005ull + 1442695040888963407ull; return state >> 33; }
   int64_t cell(int64_t x, int64_t y, int64_t z) const { return x * Ny * Nz + y * Nz + z; }
   int64_t interior() { return cell(1 + (int64_t)(rnd() % (Nx - 2)), (int64_t)(rnd() % Ny), 1 + (int64_t)(rnd() % (Nz - 2))); }
   enum Sources { TWO, EVERY_PLANE, EVERY_6TH, BAND_66 };
   // node k of a spread list sits in plane p of x AND of z, so either axis can be cut through the same arrangement
   void spread(Sources mode) {
      in.clear();
      const int64_t p0 = mode == EVERY_6TH ? 7 : (mode == BAND_66 ? 17 : 1), p1 = mode == BAND_66 ? 17 + 66 : Nx - 1, dp = mode == EVERY_6TH ? 6 : 1;
      for (int64_t p = p0; p < p1; p += dp) in.push_back(cell(p, 1 + (int64_t)(rnd() % (Ny - 2)), p));
      for (int k = 0; k < 4; k++) in.push_back(in[rnd() % in.size()]); // four nodes a second time
      for (size_t i = in.size() - 1; i > 0; i--) std::swap(in[i], in[rnd() % (i + 1)]); // out of order
   }
   explicit Scene(int real_bytes, Sources mode = TWO, int64_t nx = 12, int64_t ny = 9, int64_t nz = 14) : Nx(nx), Ny(ny), Nz(nz) {
      bn.resize(300); bnl.resize(200); bna.resize(250);
      for (auto *l : {&bn, &bnl, &bna}) for (auto &v : *l) v = interior(); // (random order: unsorted)
      adj.resize(bn.size()); K.resize(bn.size()); mat.resize(bnl.size()); Q.resize(bna.size()); ssaf.resize(bnl.size() * (size_t)real_bytes);
      for (auto &v : adj) v = (uint16_t)rnd();
      for (auto &v : K) v = (int8_t)(rnd() % 7);
      for (auto &v : mat) v = (int8_t)(rnd() % 3);
      for (auto &v : Q) v = (int8_t)(1 + rnd() % 3);
      for (auto &v : ssaf) v = (uint8_t)rnd();
      in = {cell(6, 4, 7), cell(2, 1, 11)};
      if (mode != TWO) spread(mode);
      out = {cell(7, 4, 8), cell(11, 3, 0) /* a global ghost plane of x and of z */, cell(1, 8, 12), cell(5, 0, 1), cell(6, 4, 7)};
      reorder = {0, 1, 2, 3, 4};
      sigs.resize(in.size() * (size_t)Nt);
      for (size_t i = 0; i < sigs.size(); i++) sigs[i] = 0.25 * (double)(i + 1);
      u_out.assign(out.size() * (size_t)Nt, 0.0);
      sd.bn_ixyz = bn.data(); sd.adj_bn = adj.data(); sd.K_bn = K.data(); sd.Nb = (int64_t)bn.size();
      sd.bnl_ixyz = bnl.data(); sd.mat_bnl = mat.data(); sd.ssaf_bnl = ssaf.data(); sd.Nbl = (int64_t)bnl.size();
      sd.bna_ixyz = bna.data(); sd.Q_bna = Q.data(); sd.Nba = (int64_t)bna.size();
      sd.in_ixyz = in.data(); sd.in_sigs = sigs.data(); sd.Ns = (int64_t)in.size();
      sd.out_ixyz = out.data(); sd.out_reorder = reorder.data(); sd.u_out = u_out.data(); sd.Nr = (int64_t)out.size();
      sd.Nt = Nt; sd.Nx = Nx; sd.Ny = Ny; sd.Nz = Nz; sd.Npts = Nx * Ny * Nz;
      sd.Nm = 3; sd.Mb = Mb.data(); sd.NN = 6; sd.real_bytes = real_bytes;
   }
};

// one list of one slab against the scene's: `kept` = the slab's local indices, [p0, p1) = the global planes whose entries it must hold,
// [q0, q1) = the LOCAL planes a kept entry may lie in.  Returns the positions in the global list of the entries kept, in the slab's order.
std::vector<int64_t> check_list(const char *name, const Scene &sc, const pf_cut::Slab &s, bool along_z, const int64_t *global, int64_t n,
                                const std::vector<int64_t> &kept, const int64_t *kept_ptr, int64_t kept_n, int64_t p0, int64_t p1, int64_t q0, int64_t q1,
                                std::vector<int> &seen) {
   const int64_t NzNy = sc.Ny * sc.Nz, nloc = s.xhi - s.xlo;
   std::vector<int64_t> want;
   for (int64_t i = 0; i < n; i++) {
      const int64_t p = along_z ? global[i] % sc.Nz : global[i] / NzNy;
      if (p >= p0 && p < p1) want.push_back(i);
   }
   check(kept_ptr == kept.data() && kept_n == (int64_t)kept.size(), "%s: the slab's pf_simdata does not describe its own array", name);
   check(kept.size() == want.size(), "%s: %zu entries kept, %zu lie in planes [%ld, %ld)", name, kept.size(), want.size(), (long)p0, (long)p1);
   if (kept.size() != want.size()) return {};
   for (size_t j = 0; j < kept.size(); j++) {
      const int64_t l = kept[j];
      const int64_t q = along_z ? l % nloc : l / NzNy;
      const int64_t back = along_z ? (l / nloc) * sc.Nz + l % nloc + s.xlo : l + s.xlo * NzNy;
      check(l >= 0 && l < s.sd.Npts, "%s[%zu]: local index %ld outside the slab's grid", name, j, (long)l);
      check(q >= q0 && q < q1, "%s[%zu]: local plane %ld not in [%ld, %ld)", name, j, (long)q, (long)q0, (long)q1);
      check(back == global[want[j]], "%s[%zu]: maps back to %ld, the list's entry %ld is %ld (order kept?)", name, j, (long)back, (long)want[j], (long)global[want[j]]);
      seen[want[j]]++;
   }
   return want;
}

void check_chain(const Scene &sc, int G, bool along_z, bool even) {
   const pf_simdata *sd = &sc.sd;
   const int64_t N = along_z ? sc.Nz : sc.Nx, Nt = sc.Nt;
   const int rb = sd->real_bytes;
   snprintf(g_ctx, sizeof g_ctx, "fp%d, %ld sources, G = %d, cut along %s, %s split", rb * 8, (long)sd->Ns, G, along_z ? "z" : "x", even ? "even" : "balanced");
   std::vector<int64_t> cuts;
   const char *msg = pf_cut::partition(sd, G, even, cuts, along_z);
   check(!msg, "partition: %s", msg ? msg : "");
   if (msg) return;
   check((int)cuts.size() == G + 1 && cuts[0] == 0 && cuts[G] == N, "cuts do not span [0, %ld]", (long)N);
   for (int g = 0; g < G && (int)cuts.size() == G + 1; g++)
      check(cuts[g + 1] - cuts[g] >= 2, "cut %d at %ld, cut %d at %ld: not two planes apart", g, (long)cuts[g], g + 1, (long)cuts[g + 1]);
   std::vector<int> seen_bn(sd->Nb, 0), seen_bnl(sd->Nbl, 0), seen_bna(sd->Nba, 0), seen_in(sd->Ns, 0), seen_out(sd->Nr, 0), seen_row(sd->Nr, 0);
   for (int g = 0; g < G; g++) {
      pf_cut::Slab s;
      msg = pf_cut::cut_slab(sd, cuts, g, G, s, along_z);
      check(!msg, "cut_slab(%d): %s", g, msg ? msg : "");
      if (msg) continue;
      const int64_t nloc = s.xhi - s.xlo;
      check(s.x0 == cuts[g] && s.x1 == cuts[g + 1] && s.xlo == s.x0 - (g > 0) && s.xhi == s.x1 + (g < G - 1), "slab %d: plane ranges", g);
      check((along_z ? s.sd.Nz : s.sd.Nx) == nloc && (along_z ? s.sd.Nx : s.sd.Nz) == (along_z ? sc.Nx : sc.Nz) && s.sd.Ny == sc.Ny &&
            s.sd.Npts == s.sd.Nx * s.sd.Ny * s.sd.Nz, "slab %d: local dimensions", g);
      const int64_t u0 = std::max<int64_t>(s.x0, 1), u1 = std::min<int64_t>(s.x1, N - 1); // the planes the slab updates
      char name[32];
      auto nm = [&](const char *l) { snprintf(name, sizeof name, "slab %d %s", g, l); return name; };
      std::vector<int64_t> w;
      w = check_list(nm("bn"), sc, s, along_z, sd->bn_ixyz, sd->Nb, s.bn, s.sd.bn_ixyz, s.sd.Nb, u0, u1, 1, nloc - 1, seen_bn);
      check(s.adj.size() == w.size() && s.K.size() == w.size() && s.sd.adj_bn == s.adj.data() && s.sd.K_bn == s.K.data(), "%s: adj / K sizes", name);
      for (size_t j = 0; j < w.size() && j < s.adj.size() && j < s.K.size(); j++)
         check(s.adj[j] == sd->adj_bn[w[j]] && s.K[j] == sd->K_bn[w[j]], "%s[%zu]: adj / K are not entry %ld's", name, j, (long)w[j]);
      w = check_list(nm("bnl"), sc, s, along_z, sd->bnl_ixyz, sd->Nbl, s.bnl, s.sd.bnl_ixyz, s.sd.Nbl, u0, u1, 1, nloc - 1, seen_bnl);
      check(s.matl.size() == w.size() && s.ssaf.size() == w.size() * (size_t)rb && s.sd.mat_bnl == s.matl.data() && s.sd.ssaf_bnl == (void *)s.ssaf.data(), "%s: mat / ssaf sizes", name);
      for (size_t j = 0; j < w.size() && j < s.matl.size() && (j + 1) * (size_t)rb <= s.ssaf.size(); j++)
         check(s.matl[j] == sd->mat_bnl[w[j]] && !memcmp(&s.ssaf[j * (size_t)rb], (const uint8_t *)sd->ssaf_bnl + (size_t)w[j] * rb, (size_t)rb), "%s[%zu]: mat / ssaf are not entry %ld's", name, j, (long)w[j]);
      w = check_list(nm("bna"), sc, s, along_z, sd->bna_ixyz, sd->Nba, s.bna, s.sd.bna_ixyz, s.sd.Nba, u0, u1, 1, nloc - 1, seen_bna);
      check(s.Q.size() == w.size() && s.sd.Q_bna == s.Q.data(), "%s: Q size", name);
      for (size_t j = 0; j < w.size() && j < s.Q.size(); j++) check(s.Q[j] == sd->Q_bna[w[j]], "%s[%zu]: Q is not entry %ld's", name, j, (long)w[j]);
      w = check_list(nm("in"), sc, s, along_z, sd->in_ixyz, sd->Ns, s.in, s.sd.in_ixyz, s.sd.Ns, u0, u1, 1, nloc - 1, seen_in);
      check(s.in_sigs.size() == w.size() * (size_t)Nt && s.sd.in_sigs == s.in_sigs.data(), "%s: source rows' size", name);
      for (size_t j = 0; j < w.size() && (j + 1) * (size_t)Nt <= s.in_sigs.size(); j++)
         check(!memcmp(&s.in_sigs[j * (size_t)Nt], sd->in_sigs + w[j] * Nt, sizeof(double) * (size_t)Nt), "%s[%zu]: the signal is not source %ld's", name, j, (long)w[j]);
      // receivers: at any OWNED plane, a global ghost plane included
      w = check_list(nm("out"), sc, s, along_z, sd->out_ixyz, sd->Nr, s.out, s.sd.out_ixyz, s.sd.Nr, s.x0, s.x1, s.x0 - s.xlo, s.x1 - s.xlo, seen_out);
      check(s.out_rows == w, "%s: out_rows are not the receivers' positions in the scene's list, in order", name);
      check(s.out_reorder.size() == s.out.size() && s.sd.out_reorder == s.out_reorder.data() && s.u_out.size() >= s.out.size() * (size_t)Nt && s.sd.u_out == s.u_out.data(), "%s: out_reorder / u_out", name);
      for (size_t j = 0; j < s.out_reorder.size(); j++) check(s.out_reorder[j] == (int64_t)j, "%s: out_reorder[%zu]", name, j);
      for (int64_t r : s.out_rows) if (r >= 0 && r < sd->Nr) seen_row[r]++; else check(false, "%s: out_row %ld outside 0 .. Nr-1", name, (long)r);
   }
   auto once = [&](const char *l, const std::vector<int> &seen) {
      for (size_t i = 0; i < seen.size(); i++) check(seen[i] == 1, "%s entry %zu landed in %d slabs", l, i, seen[i]);
   };
   once("bn", seen_bn); once("bnl", seen_bnl); once("bna", seen_bna); once("in", seen_in); once("out", seen_out); once("out_rows", seen_row);
}

} // namespace

int main() {
   for (int rb : {4, 8}) {
      const Scene sc(rb);
      for (int G : {2, 3, 5})
         for (bool along_z : {false, true})
            for (bool even : {true, false}) check_chain(sc, G, along_z, even);
   }
   // sources that leave no cut, or hardly any, clear
   for (int rb : {4, 8})
      for (Scene::Sources mode : {Scene::EVERY_PLANE, Scene::EVERY_6TH, Scene::BAND_66}) {
         const Scene sc(rb, mode, 100, 9, 100);
         for (int G : {2, 3, 8})
            for (bool along_z : {false, true})
               for (bool even : {true, false}) check_chain(sc, G, along_z, even);
      }
   // what cannot be cut says so
   const Scene sc(4);
   std::vector<int64_t> cuts;
   snprintf(g_ctx, sizeof g_ctx, "refusals");
   check(pf_cut::partition(&sc.sd, (int)sc.Nx, true, cuts) != nullptr, "partition accepts as many slabs as planes");
   pf_cut::Slab s;
   check(pf_cut::cut_slab(&sc.sd, {0, 1, sc.Nx}, 0, 2, s) != nullptr, "cut_slab accepts a slab that owns the global ghost plane alone");
   return g_bad ? 1 : 0;
}
