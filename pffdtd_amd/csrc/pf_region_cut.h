// pf_region_cut.h -- a region of the scene's field (pffdtd_hip.h: pf_region) checked, counted and cut to the slabs of a chain.
//   region_counts: counts[a] = ceil((hi - lo) / stride) of a well-formed region (lo >= 0, lo < hi, stride >= 1), else a message that names the field;
//   region_check:  the same against a grid's dimensions (hi <= N);
//   region_part:   what slab s OWNS of a region -- the cells whose coordinate along the cut axis (x, or file z: along_z) lies in [x0, x1) -- with
//                  the stride's phase carried across the cut: the part's first cell is the region's first cell at or after x0, not x0 itself.  The
//                  part is given in the slab's LOCAL file coordinates (minus xlo along the cut axis) together with where it lands in the region's
//                  dense output, out[(i * c1 + j) * c2 + k]: cut along x a block of output planes (offset k0 * c1 * c2), cut along file z the
//                  columns [k0, k0 + n) of every output row (offset k0, rows c2 apart).  The parts of all slabs tile the region exactly once.
// HOST ONLY, like pf_slab_cut.h: the public header and the standard library; tests/region_cut_check.cpp includes this file as it is.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "pf_slab_cut.h"

namespace pf_cut {

// returns the number of cells, or -1 and a message (msg may be null)
inline int64_t region_counts(const pf_region *r, int64_t counts[3], char *msg = nullptr, size_t nmsg = 0) {
   const bool tell = msg && nmsg;
   if (!r) { if (tell) snprintf(msg, nmsg, "null pf_region"); return -1; }
   int64_t n = 1;
   for (int a = 0; a < 3; a++) {
      if (r->stride[a] < 1) { if (tell) snprintf(msg, nmsg, "pf_region.stride[%d] = %ld: a stride is at least 1", a, (long)r->stride[a]); return -1; }
      if (r->lo[a] < 0) { if (tell) snprintf(msg, nmsg, "pf_region.lo[%d] = %ld < 0", a, (long)r->lo[a]); return -1; }
      if (r->lo[a] >= r->hi[a]) { if (tell) snprintf(msg, nmsg, "pf_region.lo[%d] = %ld >= hi[%d] = %ld: an empty region", a, (long)r->lo[a], a, (long)r->hi[a]); return -1; }
      const int64_t c = (r->hi[a] - r->lo[a] - 1) / r->stride[a] + 1;
      if (counts) counts[a] = c;
      n *= c;
   }
   return n;
}
inline int64_t region_check(const pf_region *r, const int64_t N[3], int64_t counts[3], char *msg = nullptr, size_t nmsg = 0) {
   const int64_t n = region_counts(r, counts, msg, nmsg);
   if (n < 0) return n;
   for (int a = 0; a < 3; a++)
      if (r->hi[a] > N[a]) {
         if (msg && nmsg) snprintf(msg, nmsg, "pf_region.hi[%d] = %ld > %ld, the grid's size along that axis", a, (long)r->hi[a], (long)N[a]);
         return -1;
      }
   return n;
}

struct RegionPart {
   bool empty = true;
   pf_region local{};              // the part in the slab's local file coordinates
   int64_t counts[3] = {0, 0, 0};  // ... its cells per axis
   int64_t out_off = 0;            // where its first cell lands in the region's dense output (elements)
   int64_t out_pitch = 0;          // elements between two of its rows there (the region's counts[2])
};

// r: region_check(r, the scene's dimensions, rc) done
inline RegionPart region_part(const pf_region &r, const int64_t rc[3], const Slab &s, bool along_z) {
   RegionPart p;
   const int a = along_z ? 2 : 0;
   const int64_t lo = r.lo[a], st = r.stride[a], end = std::min(s.x1, r.hi[a]);
   const int64_t k0 = lo >= s.x0 ? 0 : (s.x0 - lo - 1) / st + 1;  // first index of the region at or after x0
   const int64_t k1 = end > lo ? (end - lo - 1) / st + 1 : 0;   // first index at or after the slab's end (or the region's)
   if (k1 <= k0) return p;
   p.empty = false;
   p.local = r;
   p.local.lo[a] = lo + k0 * st - s.xlo;
   p.local.hi[a] = lo + (k1 - 1) * st + 1 - s.xlo;
   for (int b = 0; b < 3; b++) p.counts[b] = rc[b];
   p.counts[a] = k1 - k0;
   p.out_off = along_z ? k0 : k0 * rc[1] * rc[2];
   p.out_pitch = rc[2];
   return p;
}

} // namespace pf_cut
