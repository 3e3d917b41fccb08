// strip_map_check.cpp -- csrc/pf_strip_map.h against the per-lane rules of pf_wall.h's column-strip bodies, on the CPU (tests/test_strip_map.py builds
// and runs it under the address and undefined-behaviour sanitizers).  The staged strip bodies issue the per-lane form's addresses with another lane
// assignment; what is checked here is that the assignment is a re-ordering and nothing else:
//   * every (row, vector) of a tile is loaded exactly once, from the row the per-lane rule takes it from (wall_body: lsrc), inside the grid;
//   * a (row, vector) is stored exactly when the per-lane store_pencil stores it (own_lane and the owned vectors), and once;
//   * a store instruction is instruction 0 moved on by a whole number of rows (what wall_body's store_map relies on);
//   * what is written to the LDS tile in the rows' order is read back as the pencils: the places agree, stay inside the tile, collide nowhere,
//     and sixteen lanes' 16-byte accesses start in sixteen different bank groups.
// Every violated condition is named on stderr; the exit status is their number (capped).
#include <cstdio>
#include <set>
#include <utility>
#include <vector>
#include "pf_strip_map.h"

static int bad = 0;
#define CHECK(c, ...) do { if (!(c)) { bad++; fprintf(stderr, "FAILED %s: ", #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// ---- the per-lane rules, as wall_body has them ----
static int lsrc_ref(int lc, int NL) {
   int s = lc < 0 ? 0 : (lc > NL - 1 ? NL - 1 : lc);
   if (s == 0) s = 2;
   else if (s == NL - 1) s = NL - 3;
   return s;
}
static bool own_lane_ref(int lane, int lc, int hl, int l1) { return lane >= hl && lane <= 63 - hl && lc < l1; }
static bool vec_stored_ref(int q, int V, int ko0, int ko1) { return (q + 1) * V > ko0 && q * V < ko1; }

struct Side { const char *name; int ko0, ko1; };

static void check_tile(int DP, int V, int NL, int l0, int l1, int hl, int j, const Side &sd) {
   using namespace pf;
   const int NV = DP / V, lt = STRIP_ROWS - 2 * hl, tl0 = strip_row_coord(0, l0, hl, lt, j);
   // loads
   std::vector<int> seen((size_t)STRIP_ROWS * NV, 0);
   for (int i = 0; i < NV; i++)
      for (int lane = 0; lane < STRIP_ROWS; lane++) {
         const int e = strip_elem(i, lane), row = strip_row(e, NV), v = strip_vec(e, NV);
         CHECK(row >= 0 && row < STRIP_ROWS && v >= 0 && v < NV, "element %d -> row %d vector %d", e, row, v);
         if (row < 0 || row >= STRIP_ROWS || v < 0 || v >= NV) continue;
         seen[(size_t)row * NV + v]++;
         const int lc = strip_row_coord(row, l0, hl, lt, j), src = strip_lane_src(lc, NL);
         CHECK(lc == tl0 + row, "row %d: coordinate %d, tile from %d", row, lc, tl0);
         CHECK(src == lsrc_ref(lc, NL), "NL %d lc %d: source row %d, per-lane rule %d", NL, lc, src, lsrc_ref(lc, NL));
         CHECK(src >= 0 && src < NL, "NL %d lc %d: source row %d outside the grid", NL, lc, src);
         // the transpose: element e of the rows' order is vector v of row `row`'s pencil
         CHECK(strip_lds_elem(e) == strip_lds_pencil(row, v, NV), "element %d at %d, lane %d reads vector %d at %d", e, strip_lds_elem(e), row, v, strip_lds_pencil(row, v, NV));
         CHECK(strip_lds_elem(e) >= 0 && strip_lds_elem(e) < strip_lds_vectors(NV), "element %d outside the tile", e);
      }
   for (int r = 0; r < STRIP_ROWS; r++)
      for (int v = 0; v < NV; v++) CHECK(seen[(size_t)r * NV + v] == 1, "row %d vector %d loaded %d times", r, v, seen[(size_t)r * NV + v]);
   // stores
   const int q0 = strip_q0(sd.ko0, V), nvo = strip_nvo(sd.ko0, sd.ko1, V), nown = strip_owned_rows(tl0, hl, l1);
   CHECK(nvo >= 1 && q0 >= 0 && q0 + nvo <= NV, "%s: owned vectors %d .. %d of %d", sd.name, q0, q0 + nvo - 1, NV);
   CHECK(STRIP_ROWS % nvo == 0, "%s: %d owned vectors do not divide a wave", sd.name, nvo);
   std::set<std::pair<int, int>> want, got;
   for (int lane = 0; lane < STRIP_ROWS; lane++)
      for (int q = 0; q < NV; q++)
         if (own_lane_ref(lane, tl0 + lane, hl, l1) && vec_stored_ref(q, V, sd.ko0, sd.ko1)) want.insert({lane, q});
   for (int i = 0; i < nvo; i++)
      for (int lane = 0; lane < STRIP_ROWS; lane++) {
         const int e = strip_elem(i, lane), row = strip_row(e, nvo), q = q0 + strip_vec(e, nvo);
         CHECK(row >= 0 && row < STRIP_ROWS && q >= q0 && q < q0 + nvo, "%s: store element %d -> row %d vector %d", sd.name, e, row, q);
         CHECK(row == strip_row(strip_elem(0, lane), nvo) + i * (STRIP_ROWS / nvo) && q == q0 + strip_vec(strip_elem(0, lane), nvo),
               "%s: store instruction %d lane %d is not instruction 0 moved on by whole rows", sd.name, i, lane);
         CHECK(strip_lds_pencil(row, q, NV) >= 0 && strip_lds_pencil(row, q, NV) < strip_lds_vectors(NV), "%s: row %d vector %d outside the tile", sd.name, row, q);
         if (!strip_row_owned(row, hl, nown)) continue;
         CHECK(got.insert({row, q}).second, "%s: row %d vector %d stored twice", sd.name, row, q);
      }
   CHECK(got == want, "%s NL %d l0 %d l1 %d tile %d: %zu (row, vector) stored, the per-lane form stores %zu", sd.name, NL, l0, l1, j, got.size(), want.size());
   // every lane's pencil in the tile: distinct places; sixteen lanes at a time start in sixteen different 16-byte groups of the banks' 256 bytes
   std::set<int> places;
   for (int lane = 0; lane < STRIP_ROWS; lane++)
      for (int v = 0; v < NV; v++) {
         const int at = strip_lds_pencil(lane, v, NV);
         CHECK(at >= 0 && at < strip_lds_vectors(NV), "lane %d vector %d outside the tile", lane, v);
         CHECK(places.insert(at).second, "lane %d vector %d shares its place", lane, v);
      }
   if (V * 4 == 16) // (fp32: a vector is 16 bytes)
      for (int g = 0; g < STRIP_ROWS; g += 16)
         for (int v = 0; v < NV; v++) {
            std::set<int> groups;
            for (int lane = g; lane < g + 16; lane++) groups.insert(strip_lds_pencil(lane, v, NV) % 16);
            CHECK(groups.size() == 16, "lanes %d .. %d vector %d: %zu bank groups", g, g + 15, v, groups.size());
         }
}

int main() {
   const int DP = 20, V = 4, hl = 3, lt = pf::STRIP_ROWS - 2 * hl;
   const Side sides[2] = {{"low side", 1, 16}, {"high side", DP - 16, DP - 1}}; // wall_body's constant geometry of a margin of 16 cells
   int tiles = 0;
   // lane-axis extents and owned ranges: tiles that start before the grid (l0 - hl < 0), end beyond l1 and beyond the grid, whole and partial last tiles
   const int cases[][3] = {{70, 1, 69}, {70, 2, 68}, {67, 1, 66}, {67, 4, 63}, {64, 1, 63}, {61, 2, 59}, {120, 1, 119}, {1024, 4, 1020}, {1024, 1, 1023}, {9, 1, 8}, {5, 1, 4}};
   for (const auto &c : cases) {
      const int NL = c[0], l0 = c[1], l1 = c[2], nlt = (l1 - l0 + lt - 1) / lt;
      for (int j = 0; j < nlt; j++)
         for (const Side &sd : sides) { check_tile(DP, V, NL, l0, l1, hl, j, sd); tiles++; }
   }
   // the source-row rule over a wide range of coordinates, grid sizes from the smallest a ghost layer allows
   for (int NL = 4; NL <= 80; NL++)
      for (int lc = -70; lc <= NL + 70; lc++) CHECK(pf::strip_lane_src(lc, NL) == lsrc_ref(lc, NL), "NL %d lc %d: %d, per-lane rule %d", NL, lc, pf::strip_lane_src(lc, NL), lsrc_ref(lc, NL));
   // the owned-row count against own_lane, every start and end
   for (int tl0 = -5; tl0 <= 70; tl0++)
      for (int l1 = 0; l1 <= 140; l1++)
         for (int row = 0; row < pf::STRIP_ROWS; row++)
            CHECK(pf::strip_row_owned(row, hl, pf::strip_owned_rows(tl0, hl, l1)) == own_lane_ref(row, tl0 + row, hl, l1), "tile from %d, l1 %d, row %d", tl0, l1, row);
   printf("%d tiles checked\n", tiles);
   return bad > 100 ? 100 : bad;
}
