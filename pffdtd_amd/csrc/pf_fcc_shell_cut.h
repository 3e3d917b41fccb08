// pf_fcc_shell_cut.h -- how the shell of a 13-point blocked pair becomes bricks (pf_brick_fcc.h: k_brick_fcc steps a brick and its halo in
// LDS, `ns` steps per launch).  The shell is every interior cell outside the box the pair kernel advances: two x slabs (whole planes), two
// row strips (the box's planes), two column strips (the box's planes and rows; the right one may be dozens of columns wide) -- each cut
// into owned boxes, regular per slab, small enough that the extended box (owned + `ns` cells of halo, clipped to the interior) fits the
// LDS bound and holds no more frequency-dependent nodes than the kernel's threads carry (Scene::max_nodes <= BRICK_T * BRICK_KN).
// HOST ONLY: the standard library, no device, no engine state -- a pure function of the dimensions, the box, the node / lossy / ABC /
// source lists and `ns`, which returns its refusal as a message ("" = fine); tests/fcc_shell_cut_check.cpp includes this file as it is.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace pf_fcc {

constexpr int BRICK_T = 256; // threads per brick
constexpr int BRICK_KN = 2;  // frequency-dependent nodes a thread carries at most

struct Brick {
   int32_t e0[3], en[3]; // extended box: first cell (x, y, z; >= 1) and extents (ghost cells are never part of it)
   int32_t o0[3], o1[3]; // the cells it owns (stores): [o0, o1)
   uint32_t info_off;    // its first info word
   uint32_t los_off, nlos; // its frequency-dependent nodes
};
struct Node { uint32_t cell, li; }; // cell of the extended box | owned << 31, position in the lossy arrays

// info word of a cell of an extended box: twelve adjacency bits (the oracle's order), node / frequency-dependent flags; air cells: the ABC count
constexpr uint16_t INFO_ADJ = 0x0fff, INFO_NODE = 0x1000, INFO_FD = 0x2000;
constexpr int INFO_Q_SHIFT = 14;

// bytes of LDS a brick of `cells` extended cells needs: the materials' tables (12 branches of four Reals, beta, branch count), three planes
inline size_t lds_bytes(int64_t cells, int nmat, int real_bytes) {
   size_t b = (size_t)nmat * 12 * 4 * (size_t)real_bytes + (size_t)nmat * (size_t)real_bytes + (size_t)nmat * sizeof(int32_t);
   b = (b + 15) & ~(size_t)15;
   return b + 3 * (size_t)cells * (size_t)real_bytes;
}

struct Scene {
   int64_t N[3];           // stored dimensions (x, y, z), ghost shell included
   int64_t sx, sy;         // a cell's index in the lists below: ix * sx + iy * sy + iz
   int32_t box0[3], box1[3]; // the pair kernel's box [box0, box1)
   int64_t Nb; const int64_t *bn; const uint16_t *adj; const int32_t *lossy; // boundary nodes: cell, adjacency bits, place in the lossy arrays or -1
   int64_t Nba; const int64_t *bna; const int8_t *Q;                        // ABC cells and their counts
   int64_t Ns; const int64_t *src;                                          // source cells
   int32_t ns;             // steps per launch (halo cells)
   int32_t real_bytes, nmat;
   size_t lds_max;         // bytes of LDS a brick may take
   int32_t max_nodes;      // frequency-dependent nodes an extended box may hold (<= BRICK_T * BRICK_KN; pf_brick_fcc.h: brick_fcc_kn)
};
struct Cut {
   std::vector<Brick> brk;
   std::vector<uint16_t> info;
   std::vector<Node> los;
   std::vector<int32_t> rest; // boundary nodes (positions in the list) no brick owns: the nodes inside the box
   size_t lds = 0;            // the largest brick's
   int64_t nodes_owned = 0;   // frequency-dependent nodes the bricks own
   int32_t tile[6][3] = {};   // owned box per slab (x lo, x hi, y lo, y hi, z lo, z hi), 0: the slab is empty
};

namespace detail {
struct Slab { int32_t a0[3], a1[3], t[3], n[3]; uint32_t first; };
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
// tiles of the slab whose EXTENDED box holds cell g: fn(tile index within the slab, i[3])
template <typename F> inline void tiles_holding(const Slab &s, const int64_t *N, int ns, const int32_t *g, F &&fn) {
   int lo[3], hi[3];
   for (int d = 0; d < 3; d++) {
      const int a = g[d] - ns - s.a0[d], b = g[d] + ns - s.a0[d];
      if (b < 0) return;
      lo[d] = a < 0 ? 0 : a / s.t[d];
      hi[d] = std::min(b / s.t[d], s.n[d] - 1);
      if (lo[d] > hi[d]) return;
   }
   for (int i = lo[0]; i <= hi[0]; i++) for (int j = lo[1]; j <= hi[1]; j++) for (int k = lo[2]; k <= hi[2]; k++) {
      const int ii[3] = {i, j, k};
      bool in = true;
      for (int d = 0; d < 3 && in; d++) {
         const int o0 = s.a0[d] + ii[d] * s.t[d], o1 = std::min(o0 + s.t[d], s.a1[d]);
         in = g[d] >= std::max(o0 - ns, 1) && g[d] < std::min<int64_t>(o1 + ns, N[d] - 1);
      }
      if (in) fn((uint32_t)((i * s.n[1] + j) * s.n[2] + k), ii);
   }
}
} // namespace detail

inline std::string cut_shell(const Scene &sc, Cut &out) {
   using namespace detail;
   char msg[256];
   out = Cut{};
   const int ns = sc.ns;
   if (ns < 1 || ns > 2) return "bricks take one or two steps per launch";
   if (sc.max_nodes < 1 || sc.max_nodes > BRICK_T * BRICK_KN) return "a brick's threads carry between 1 and BRICK_T * BRICK_KN frequency-dependent nodes";
   for (int d = 0; d < 3; d++)
      if (sc.box0[d] < 2 || sc.box1[d] > sc.N[d] - 2 || sc.box1[d] - sc.box0[d] < 2 * ns + 1) return "the box does not leave a shell on every side";
   auto coords = [&](int64_t c, int32_t *g) { g[0] = (int32_t)(c / sc.sx); g[1] = (int32_t)((c % sc.sx) / sc.sy); g[2] = (int32_t)(c % sc.sy); };
   // a brick recomputes `ns` steps of its halo, and a source is added BETWEEN the steps: none within `ns` cells of a shell cell
   for (int64_t i = 0; i < sc.Ns; i++) {
      int32_t g[3];
      coords(sc.src[i], g);
      for (int d = 0; d < 3; d++)
         if (g[d] < sc.box0[d] + ns || g[d] >= sc.box1[d] - ns) {
            snprintf(msg, sizeof msg, "a source at (%d, %d, %d) lies within %d cells of the shell", g[0], g[1], g[2], ns);
            return msg;
         }
   }
   // (a node on the ABC shell would take the loss before its rigid update, oracle/pf_oracle_impl.inc:296-346: not a brick's business)
   {
      std::vector<int64_t> abc(sc.bna, sc.bna + sc.Nba);
      std::sort(abc.begin(), abc.end());
      for (int64_t i = 0; i < sc.Nb; i++)
         if (std::binary_search(abc.begin(), abc.end(), sc.bn[i])) return "a boundary node on the ABC shell";
   }
   // the six slabs
   Slab slabs[6];
   for (int q = 0; q < 6; q++) {
      Slab &s = slabs[q];
      const int ax = q / 2, hi = q % 2;
      for (int d = 0; d < 3; d++) {
         if (d < ax) { s.a0[d] = sc.box0[d]; s.a1[d] = sc.box1[d]; }
         else if (d == ax) { s.a0[d] = hi ? sc.box1[d] : 1; s.a1[d] = hi ? (int32_t)sc.N[d] - 1 : sc.box0[d]; }
         else { s.a0[d] = 1; s.a1[d] = (int32_t)sc.N[d] - 1; }
         s.t[d] = s.n[d] = 0;
      }
   }
   // Owned boxes: the slab's thin axis in even chunks of at most 12 cells, its two long axes in tiles of 16 x 16 cells -- shorter ones where
   // those need too much LDS or hold too many frequency-dependent nodes (the longer side along z, the unit-stride axis, where z is a long axis)
   static const int cand[5][2] = {{16, 16}, {8, 16}, {8, 8}, {4, 8}, {4, 4}};
   std::vector<uint32_t> cnt;
   for (int q = 0; q < 6; q++) {
      Slab &s = slabs[q];
      const int ax = q / 2;
      if (s.a1[ax] <= s.a0[ax]) continue;
      bool ok = false;
      for (int c = 0; c < 5 && !ok; c++) {
         int64_t cells = 1, ntile = 1;
         for (int d = 0, k = 0; d < 3; d++) {
            const int len = s.a1[d] - s.a0[d];
            if (d == ax) s.t[d] = (int)cdiv(len, cdiv(len, 12));
            else s.t[d] = std::min(cand[c][k++], len);
            s.n[d] = (int)cdiv(len, s.t[d]);
            cells *= std::min<int64_t>(s.t[d] + 2 * ns, sc.N[d] - 2);
            ntile *= s.n[d];
         }
         if (lds_bytes(cells, sc.nmat, sc.real_bytes) > sc.lds_max || ntile >= ((int64_t)1 << 30)) continue;
         cnt.assign((size_t)ntile, 0u);
         uint32_t most = 0;
         for (int64_t i = 0; i < sc.Nb; i++) {
            if (sc.lossy[i] < 0) continue;
            int32_t g[3];
            coords(sc.bn[i], g);
            tiles_holding(s, sc.N, ns, g, [&](uint32_t t, const int *) { most = std::max(most, ++cnt[t]); });
         }
         ok = most <= (uint32_t)sc.max_nodes;
      }
      if (!ok) {
         snprintf(msg, sizeof msg, "no brick size fits the %s %c slab of the shell (%zu bytes of LDS, %d frequency-dependent nodes per brick at most)", q % 2 ? "high" : "low",
                  "xyz"[ax], sc.lds_max, sc.max_nodes);
         return msg;
      }
      for (int d = 0; d < 3; d++) out.tile[q][d] = s.t[d];
   }
   // the bricks
   uint64_t ninfo = 0;
   for (int q = 0; q < 6; q++) {
      Slab &s = slabs[q];
      s.first = (uint32_t)out.brk.size();
      if (s.a1[q / 2] <= s.a0[q / 2]) { s.n[0] = s.n[1] = s.n[2] = 0; s.t[0] = s.t[1] = s.t[2] = 1; continue; }
      for (int i = 0; i < s.n[0]; i++) for (int j = 0; j < s.n[1]; j++) for (int k = 0; k < s.n[2]; k++) {
         const int ii[3] = {i, j, k};
         Brick b{};
         int64_t cells = 1;
         for (int d = 0; d < 3; d++) {
            b.o0[d] = s.a0[d] + ii[d] * s.t[d];
            b.o1[d] = std::min(b.o0[d] + s.t[d], s.a1[d]);
            b.e0[d] = std::max(b.o0[d] - ns, 1);
            b.en[d] = (int32_t)std::min<int64_t>(b.o1[d] + ns, sc.N[d] - 1) - b.e0[d];
            cells *= b.en[d];
         }
         if (ninfo + (uint64_t)cells >= ((uint64_t)1 << 32)) return "the shell's bricks hold more than 2^32 cells";
         b.info_off = (uint32_t)ninfo;
         ninfo += (uint64_t)cells;
         out.lds = std::max(out.lds, lds_bytes(cells, sc.nmat, sc.real_bytes));
         out.brk.push_back(b);
      }
   }
   if (out.brk.empty()) return "the shell is empty";
   out.info.assign((size_t)ninfo, (uint16_t)0);
   auto cell_of = [](const Brick &b, const int32_t *g) {
      return ((uint32_t)(g[0] - b.e0[0]) * (uint32_t)b.en[1] + (uint32_t)(g[1] - b.e0[1])) * (uint32_t)b.en[2] + (uint32_t)(g[2] - b.e0[2]);
   };
   // air cells: the ABC count, taken from the list
   for (int64_t i = 0; i < sc.Nba; i++) {
      int32_t g[3];
      coords(sc.bna[i], g);
      for (const Slab &s : slabs)
         tiles_holding(s, sc.N, ns, g, [&](uint32_t t, const int *) {
            const Brick &b = out.brk[s.first + t];
            out.info[(size_t)b.info_off + cell_of(b, g)] = (uint16_t)(((unsigned)sc.Q[i] & 3u) << INFO_Q_SHIFT);
         });
   }
   // boundary nodes: info words, the bricks' lists of frequency-dependent nodes, the rest list
   std::vector<std::vector<Node>> los(out.brk.size());
   for (int64_t i = 0; i < sc.Nb; i++) {
      int32_t g[3];
      coords(sc.bn[i], g);
      bool in_box = true;
      for (int d = 0; d < 3; d++) in_box = in_box && g[d] >= sc.box0[d] && g[d] < sc.box1[d];
      if (in_box) out.rest.push_back((int32_t)i);
      for (const Slab &s : slabs)
         tiles_holding(s, sc.N, ns, g, [&](uint32_t t, const int *) {
            const Brick &b = out.brk[s.first + t];
            const uint32_t c = cell_of(b, g);
            out.info[(size_t)b.info_off + c] = (uint16_t)((sc.adj[i] & INFO_ADJ) | INFO_NODE | (sc.lossy[i] >= 0 ? INFO_FD : 0));
            if (sc.lossy[i] >= 0) {
               bool own = true;
               for (int d = 0; d < 3; d++) own = own && g[d] >= b.o0[d] && g[d] < b.o1[d];
               los[s.first + t].push_back(Node{c | (own ? 0x80000000u : 0u), (uint32_t)sc.lossy[i]});
               if (own) out.nodes_owned++;
            }
         });
   }
   for (size_t b = 0; b < out.brk.size(); b++) {
      if (los[b].size() > (size_t)sc.max_nodes) return "a brick holds too many frequency-dependent nodes"; // (counted above: never)
      out.brk[b].los_off = (uint32_t)out.los.size();
      out.brk[b].nlos = (uint32_t)los[b].size();
      out.los.insert(out.los.end(), los[b].begin(), los[b].end());
   }
   return "";
}

} // namespace pf_fcc
