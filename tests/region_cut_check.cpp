// region_cut_check.cpp -- a region of the field cut to the slabs of a chain (pffdtd_amd/csrc/pf_region_cut.h: region_check + region_part over the slabs
// of pf_slab_cut.h), as a program of its own: tests/test_region_cut.py compiles it with the host compiler under the address and undefined-behaviour
// sanitizers and runs it once.  Prints the violated condition on stderr and returns non-zero.
//
// Grid: 23 x 7 x 19 cells whose value is their file index.  For G = 1 .. 5 slabs, both cut axes, even cuts and random ones, and 400 random regions
// each (strides 1 .. 4 per axis; whole axes, boxes, regions of thickness 1 -- on the planes x0 and x1 - 1 of every slab too --, regions that miss
// slabs): every slab plays the engine's part on its LOCAL field (the planes it holds, ghost planes included) and writes what region_part tells it
// to where region_part tells it to.  Then
//   * every cell of the dense output was written exactly once, by a slab that OWNS the cell it read;
//   * the output equals the same slicing of the global array;
//   * a part's counts are the counts of its local region, and it lies inside the slab's field.
// And the regions that are not well-formed, or leave the grid, are refused with a message that names the field.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "pf_region_cut.h"

namespace {

int g_bad = 0;
char g_ctx[160] = "";
void check(bool ok, const char *fmt, ...) {
   if (ok) return;
   g_bad++;
   if (g_bad > 40) return;
   fprintf(stderr, "region_cut_check [%s]: ", g_ctx);
   va_list ap;
   va_start(ap, fmt);
   vfprintf(stderr, fmt, ap);
   va_end(ap);
   fprintf(stderr, "\n");
}

constexpr int64_t N[3] = {23, 7, 19};
uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return g_state >> 33; }
int64_t rnd_in(int64_t lo, int64_t hi) { return lo + (int64_t)(rnd() % (uint64_t)(hi - lo)); } // [lo, hi)

// a slab's local field: the planes [xlo, xhi) of the cut axis, file order, values = the global file index
std::vector<int64_t> local_field(const pf_cut::Slab &s, bool along_z) {
   const int64_t nloc = s.xhi - s.xlo;
   std::vector<int64_t> f;
   for (int64_t x = 0; x < (along_z ? N[0] : nloc); x++)
      for (int64_t y = 0; y < N[1]; y++)
         for (int64_t z = 0; z < (along_z ? nloc : N[2]); z++) f.push_back(((x + (along_z ? 0 : s.xlo)) * N[1] + y) * N[2] + z + (along_z ? s.xlo : 0));
   return f;
}

void check_region(const std::vector<pf_cut::Slab> &slabs, const std::vector<std::vector<int64_t>> &fields, bool along_z, const pf_region &r) {
   int64_t rc[3];
   char msg[256] = "";
   const int64_t total = pf_cut::region_check(&r, N, rc, msg, sizeof msg);
   check(total == rc[0] * rc[1] * rc[2] && total > 0, "a good region is refused: %s", msg);
   if (total <= 0) return;
   std::vector<int64_t> out((size_t)total, -1), want;
   for (int64_t x = r.lo[0]; x < r.hi[0]; x += r.stride[0])
      for (int64_t y = r.lo[1]; y < r.hi[1]; y += r.stride[1])
         for (int64_t z = r.lo[2]; z < r.hi[2]; z += r.stride[2]) want.push_back((x * N[1] + y) * N[2] + z);
   check((int64_t)want.size() == total, "counts %ld x %ld x %ld, the slicing has %zu cells", (long)rc[0], (long)rc[1], (long)rc[2], want.size());
   if ((int64_t)want.size() != total) return;
   const int a = along_z ? 2 : 0;
   for (size_t g = 0; g < slabs.size(); g++) {
      const pf_cut::Slab &s = slabs[g];
      const pf_cut::RegionPart p = pf_cut::region_part(r, rc, s, along_z);
      const bool hits = [&] { for (int64_t v = r.lo[a]; v < r.hi[a]; v += r.stride[a]) if (v >= s.x0 && v < s.x1) return true; return false; }();
      check(p.empty == !hits, "slab %zu: part %s, the region %s its owned planes", g, p.empty ? "empty" : "not empty", hits ? "meets" : "misses");
      if (p.empty) continue;
      int64_t lc[3], ln[3] = {N[0], N[1], N[2]};
      ln[a] = s.xhi - s.xlo;
      const int64_t ltotal = pf_cut::region_check(&p.local, ln, lc, msg, sizeof msg);
      check(ltotal > 0, "slab %zu: its local region is refused: %s", g, msg);
      if (ltotal <= 0) continue;
      check(lc[0] == p.counts[0] && lc[1] == p.counts[1] && lc[2] == p.counts[2], "slab %zu: counts of the part differ from its local region's", g);
      check(p.out_pitch == rc[2], "slab %zu: output pitch %ld, the region has %ld cells along z", g, (long)p.out_pitch, (long)rc[2]);
      for (int64_t i = 0; i < lc[0]; i++)
         for (int64_t j = 0; j < lc[1]; j++)
            for (int64_t k = 0; k < lc[2]; k++) {
               const int64_t l[3] = {p.local.lo[0] + i * r.stride[0], p.local.lo[1] + j * r.stride[1], p.local.lo[2] + k * r.stride[2]};
               const int64_t cut = l[a] + s.xlo;
               check(cut >= s.x0 && cut < s.x1, "slab %zu reads plane %ld of the cut axis, it owns [%ld, %ld)", g, (long)cut, (long)s.x0, (long)s.x1);
               const int64_t o = p.out_off + (i * lc[1] + j) * p.out_pitch + k;
               check(o >= 0 && o < total, "slab %zu writes output cell %ld of %ld", g, (long)o, (long)total);
               if (o < 0 || o >= total) return;
               check(out[(size_t)o] == -1, "output cell %ld written twice (slab %zu)", (long)o, g);
               out[(size_t)o] = fields[g][(size_t)((l[0] * ln[1] + l[1]) * ln[2] + l[2])];
            }
   }
   int64_t wrong = 0;
   for (int64_t o = 0; o < total; o++) wrong += out[(size_t)o] != want[(size_t)o];
   check(wrong == 0, "%ld of %ld output cells differ from the slicing of the global array (lo %ld %ld %ld hi %ld %ld %ld stride %ld %ld %ld)", (long)wrong, (long)total,
         (long)r.lo[0], (long)r.lo[1], (long)r.lo[2], (long)r.hi[0], (long)r.hi[1], (long)r.hi[2], (long)r.stride[0], (long)r.stride[1], (long)r.stride[2]);
}

void check_chain(int G, bool along_z, bool even) {
   pf_simdata sd{};
   sd.Nx = N[0]; sd.Ny = N[1]; sd.Nz = N[2]; sd.Npts = N[0] * N[1] * N[2]; sd.Nt = 1; sd.real_bytes = 4;
   const int64_t n = along_z ? N[2] : N[0];
   std::vector<int64_t> cuts;
   if (even) {
      const char *msg = pf_cut::partition(&sd, G, true, cuts, along_z);
      check(msg == nullptr, "partition: %s", msg ? msg : "");
      if (msg) return;
   } else { // random cuts that leave every slab an interior plane
      cuts.assign(G + 1, 0);
      cuts[G] = n;
      for (int g = 1; g < G; g++) cuts[g] = rnd_in(cuts[g - 1] + 2, n - 2 * (G - g) + 1);
   }
   std::vector<pf_cut::Slab> slabs(G);
   std::vector<std::vector<int64_t>> fields(G);
   for (int g = 0; g < G; g++) {
      const char *msg = pf_cut::cut_slab(&sd, cuts, g, G, slabs[g], along_z);
      check(msg == nullptr, "cut_slab %d: %s", g, msg ? msg : "");
      if (msg) return;
      fields[g] = local_field(slabs[g], along_z);
   }
   const int a = along_z ? 2 : 0;
   pf_region whole{{0, 0, 0}, {N[0], N[1], N[2]}, {1, 1, 1}};
   check_region(slabs, fields, along_z, whole);
   for (int g = 0; g < G; g++) // thickness 1 on both sides of every cut, and a strided box that starts on one
      for (int64_t plane : {slabs[g].x0, slabs[g].x1 - 1}) {
         pf_region r = whole;
         r.lo[a] = plane; r.hi[a] = plane + 1;
         check_region(slabs, fields, along_z, r);
         r.hi[a] = n; r.stride[a] = 3; r.stride[1] = 2;
         check_region(slabs, fields, along_z, r);
      }
   for (int t = 0; t < 400; t++) {
      pf_region r;
      for (int b = 0; b < 3; b++) {
         r.lo[b] = rnd_in(0, N[b]);
         r.hi[b] = (rnd() % 4 == 0) ? r.lo[b] + 1 : rnd_in(r.lo[b] + 1, N[b] + 1);
         r.stride[b] = rnd_in(1, 5);
      }
      check_region(slabs, fields, along_z, r);
   }
}

void check_refusals() {
   snprintf(g_ctx, sizeof g_ctx, "refusals");
   const pf_region good{{1, 2, 3}, {20, 6, 19}, {2, 1, 4}};
   int64_t c[3];
   char msg[256];
   check(pf_cut::region_check(&good, N, c, msg, sizeof msg) == 10 * 4 * 4 && c[0] == 10 && c[1] == 4 && c[2] == 4, "counts of a good region: %ld %ld %ld", (long)c[0], (long)c[1], (long)c[2]);
   check(pf_cut::region_counts(&good, nullptr) == 160, "region_counts without a counts array");
   struct Bad { int axis; int64_t lo, hi, stride; const char *names; };
   const Bad bad[] = {{0, -1, 5, 1, "lo[0]"}, {1, 2, 8, 1, "hi[1]"}, {2, 5, 5, 1, "lo[2]"}, {2, 7, 5, 1, "lo[2]"}, {1, 2, 6, 0, "stride[1]"}, {0, 1, 20, -3, "stride[0]"}, {2, 0, 20, 1, "hi[2]"}};
   for (const Bad &b : bad) {
      pf_region r = good;
      r.lo[b.axis] = b.lo; r.hi[b.axis] = b.hi; r.stride[b.axis] = b.stride;
      msg[0] = 0;
      check(pf_cut::region_check(&r, N, c, msg, sizeof msg) < 0, "a bad region (%s) is accepted", b.names);
      check(strstr(msg, b.names) != nullptr, "the refusal '%s' does not name %s", msg, b.names);
   }
   msg[0] = 0;
   check(pf_cut::region_check(nullptr, N, c, msg, sizeof msg) < 0 && strstr(msg, "null"), "a null region: '%s'", msg);
   pf_region r = good; // strides far larger than the grid: one cell per axis, no overflow
   for (int b = 0; b < 3; b++) r.stride[b] = INT64_MAX;
   check(pf_cut::region_check(&r, N, c, msg, sizeof msg) == 1, "strides of INT64_MAX: one cell");
}

} // namespace

int main() {
   for (int G = 1; G <= 5; G++)
      for (int along_z = 0; along_z < 2; along_z++)
         for (int even = 0; even < 2; even++) {
            snprintf(g_ctx, sizeof g_ctx, "G=%d cut along %s, %s cuts", G, along_z ? "z" : "x", even ? "even" : "random");
            check_chain(G, along_z != 0, even != 0);
         }
   check_refusals();
   if (g_bad) fprintf(stderr, "region_cut_check: %d condition(s) violated\n", g_bad);
   return g_bad ? 1 : 0;
}
