// state_cut_check.cpp -- the chain's cut of the canonical state (pffdtd_amd/csrc/pf_state_cut.h: scatter_state + gather_state over the slabs of
// pf_slab_cut.h) on a small scene built in memory, as a program of its own: tests/test_state_cut.py compiles it with the host compiler under the
// address and undefined-behaviour sanitizers and runs it once.  Prints the violated condition on stderr and returns non-zero.
//
// Scene: 12 x 9 x 14 cells, an unsorted list of 200 frequency-dependent nodes of which every fifth repeats an earlier entry (duplicates are
// legal and keep a state each).  For G = 1, 2, 3, 5, both cut axes, fp32 and fp64:
//   * gather(scatter(x)) == x: every byte of the six arrays, through the slabs and back into an empty state;
//   * every global node row lands in exactly one slab, in file order;
//   * each slab's ghost planes hold what its neighbour's owned planes hold.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "pf_slab_cut.h"
#include "pf_state_cut.h"

namespace {

int g_bad = 0;
char g_ctx[128] = "";
void check(bool ok, const char *fmt, ...) {
   if (ok) return;
   g_bad++;
   fprintf(stderr, "state_cut_check [%s]: ", g_ctx);
   va_list ap;
   va_start(ap, fmt);
   vfprintf(stderr, fmt, ap);
   va_end(ap);
   fprintf(stderr, "\n");
}

struct Scene {
   static constexpr int64_t Nx = 12, Ny = 9, Nz = 14, Nt = 4;
   std::vector<int64_t> bn, bnl, in, out, reorder;
   std::vector<uint16_t> adj;
   std::vector<int8_t> mat, Mb{3, 11, 5};
   std::vector<uint8_t> ssaf;
   std::vector<double> sigs, u_out;
   pf_simdata sd{};
   uint64_t state = 0x2545F4914F6CDD1Dull;
   uint64_t rnd() { state = state * 6364136223846793005ull + 1442695040888963407ull; return state >> 33; }
   int64_t cell(int64_t x, int64_t y, int64_t z) const { return x * Ny * Nz + y * Nz + z; }
   int64_t interior() { return cell(1 + (int64_t)(rnd() % (Nx - 2)), (int64_t)(rnd() % Ny), 1 + (int64_t)(rnd() % (Nz - 2))); }
   explicit Scene(int real_bytes) {
      bnl.resize(200);
      for (size_t i = 0; i < bnl.size(); i++) bnl[i] = (i % 5 == 4) ? bnl[rnd() % i] : interior(); // unsorted, with duplicates
      bn = bnl;
      adj.assign(bn.size(), 0x15);
      mat.resize(bnl.size());
      for (auto &v : mat) v = (int8_t)(rnd() % 3);
      ssaf.assign(bnl.size() * (size_t)real_bytes, 0);
      in = {cell(6, 4, 7)};
      out = {cell(7, 4, 8)};
      reorder = {0};
      sigs.assign(in.size() * (size_t)Nt, 1.0);
      u_out.assign(out.size() * (size_t)Nt, 0.0);
      sd.bn_ixyz = bn.data(); sd.adj_bn = adj.data(); sd.Nb = (int64_t)bn.size();
      sd.bnl_ixyz = bnl.data(); sd.mat_bnl = mat.data(); sd.ssaf_bnl = ssaf.data(); sd.Nbl = (int64_t)bnl.size();
      sd.in_ixyz = in.data(); sd.in_sigs = sigs.data(); sd.Ns = (int64_t)in.size();
      sd.out_ixyz = out.data(); sd.out_reorder = reorder.data(); sd.u_out = u_out.data(); sd.Nr = (int64_t)out.size();
      sd.Nt = Nt; sd.Nx = Nx; sd.Ny = Ny; sd.Nz = Nz; sd.Npts = Nx * Ny * Nz;
      sd.Nm = 3; sd.Mb = Mb.data(); sd.NN = 6; sd.real_bytes = real_bytes;
   }
};

// the scene's whole state as six byte arrays
struct Global {
   std::vector<uint8_t> a[6];
   pf_state st{};
   Global(const pf_simdata &sd, Scene *fill) {
      const size_t rb = (size_t)sd.real_bytes;
      const size_t n[6] = {(size_t)sd.Npts * rb, (size_t)sd.Npts * rb, (size_t)sd.Nbl * rb, (size_t)sd.Nbl * rb, (size_t)sd.Nbl * PF_MMB * rb, (size_t)sd.Nbl * PF_MMB * rb};
      for (int k = 0; k < 6; k++) {
         a[k].assign(n[k], 0);
         if (fill) for (auto &v : a[k]) v = (uint8_t)(1 + fill->rnd() % 255); // (never 0: a byte nobody wrote shows)
      }
      st.u_prev = a[0].data(); st.u_cur = a[1].data(); st.u1b = a[2].data(); st.u2b = a[3].data(); st.vh1 = a[4].data(); st.gh1 = a[5].data();
   }
};

// plane p (of the cut axis, LOCAL numbering) of a slab's field as bytes, in file order of the other two axes
std::vector<uint8_t> local_plane(const Scene &sc, const pf_cut::Slab &s, bool along_z, const std::vector<uint8_t> &f, int64_t p) {
   const size_t rb = (size_t)sc.sd.real_bytes;
   std::vector<uint8_t> o;
   if (!along_z) {
      const size_t plane = (size_t)(sc.Ny * sc.Nz) * rb;
      o.assign(f.begin() + (size_t)p * plane, f.begin() + (size_t)(p + 1) * plane);
      return o;
   }
   const int64_t nloc = s.xhi - s.xlo;
   for (int64_t r = 0; r < sc.Nx * sc.Ny; r++) o.insert(o.end(), f.begin() + (size_t)(r * nloc + p) * rb, f.begin() + (size_t)(r * nloc + p + 1) * rb);
   return o;
}

void check_chain(Scene &sc, int G, bool along_z) {
   const pf_simdata *sd = &sc.sd;
   std::vector<int64_t> cuts;
   const char *msg = pf_cut::partition(sd, G, false, cuts, along_z);
   check(msg == nullptr, "partition: %s", msg ? msg : "");
   if (msg) return;
   std::vector<pf_cut::Slab> slabs(G);
   std::vector<pf_cut::LocalState> loc(G);
   Global x(*sd, &sc), y(*sd, nullptr);
   std::vector<int> seen(sd->Nbl, 0);
   for (int g = 0; g < G; g++) {
      msg = pf_cut::cut_slab(sd, cuts, g, G, slabs[g], along_z);
      check(msg == nullptr, "cut_slab %d: %s", g, msg ? msg : "");
      if (msg) return;
      const pf_cut::Slab &s = slabs[g];
      check((int64_t)s.bnl_rows.size() == s.sd.Nbl, "slab %d: %zu rows recorded for %ld local entries", g, s.bnl_rows.size(), (long)s.sd.Nbl);
      for (size_t i = 0; i < s.bnl_rows.size(); i++) {
         const int64_t r = s.bnl_rows[i];
         check(r >= 0 && r < sd->Nbl, "slab %d: row %ld outside the list", g, (long)r);
         if (r < 0 || r >= sd->Nbl) return;
         seen[r]++;
         check(i == 0 || s.bnl_rows[i - 1] < r, "slab %d: rows not in file order at %zu", g, i);
         const int64_t l = s.bnl[i], nloc = s.xhi - s.xlo;
         const int64_t back = along_z ? (l / nloc) * sc.Nz + l % nloc + s.xlo : l + s.xlo * sc.Ny * sc.Nz;
         check(back == sd->bnl_ixyz[r], "slab %d: local entry %zu is cell %ld, row %ld of the scene is %ld", g, i, (long)back, (long)r, (long)sd->bnl_ixyz[r]);
      }
      pf_cut::alloc_state(s, loc[g]);
      pf_cut::scatter_state(sd, &x.st, s, along_z, loc[g]);
   }
   for (int64_t r = 0; r < sd->Nbl; r++) check(seen[r] == 1, "node row %ld lands in %d slabs", (long)r, seen[r]);
   // ghost planes: what the neighbour owns there
   for (int g = 0; g + 1 < G; g++) {
      const pf_cut::Slab &a = slabs[g], &b = slabs[g + 1];
      for (int f = 0; f < 2; f++) {
         const std::vector<uint8_t> &fa = f ? loc[g].u_cur : loc[g].u_prev, &fb = f ? loc[g + 1].u_cur : loc[g + 1].u_prev;
         check(local_plane(sc, a, along_z, fa, a.xhi - 1 - a.xlo) == local_plane(sc, b, along_z, fb, b.x0 - b.xlo), "slab %d's high ghost plane (field %d) is not slab %d's first owned plane", g, f, g + 1);
         check(local_plane(sc, b, along_z, fb, 0) == local_plane(sc, a, along_z, fa, a.x1 - 1 - a.xlo), "slab %d's low ghost plane (field %d) is not slab %d's last owned plane", g + 1, f, g);
      }
   }
   for (int g = 0; g < G; g++) pf_cut::gather_state(sd, loc[g], slabs[g], along_z, &y.st);
   static const char *names[6] = {"u_prev", "u_cur", "u1b", "u2b", "vh1", "gh1"};
   for (int k = 0; k < 6; k++) check(x.a[k] == y.a[k], "gather(scatter(x)) != x in %s", names[k]);
}

} // namespace

int main() {
   for (int rb : {4, 8})
      for (int G : {1, 2, 3, 5})
         for (int along_z = 0; along_z < 2; along_z++) {
            snprintf(g_ctx, sizeof g_ctx, "fp%d G=%d cut along %s", rb * 8, G, along_z ? "z" : "x");
            Scene sc(rb);
            check_chain(sc, G, along_z != 0);
         }
   if (g_bad) fprintf(stderr, "state_cut_check: %d condition(s) violated\n", g_bad);
   return g_bad ? 1 : 0;
}
