// pf_state_cut.h -- the canonical state of a scene (pffdtd_hip.h: pf_state) cut to the slabs of a chain and put together again.
//   scatter_state: a slab receives the planes it HOLDS, [xlo, xhi) of the cut axis, ghost planes included (the edge planes of an interior slab are real data),
//                  and the node rows cut_slab recorded for it (Slab::bnl_rows: the entries it updates, in file order, disjoint between slabs);
//   gather_state:  it returns the planes it OWNS, [x0, x1), and the same rows.
// Cut along x a slab's planes are contiguous in the global arrays; cut along FILE Z (along_z) they are the columns z in [xlo, xhi) of every row.
// HOST ONLY, like pf_slab_cut.h: the public header and the standard library; tests/state_cut_check.cpp includes this file as it is.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "pf_slab_cut.h"

namespace pf_cut {

// a slab's local state: the arrays and the pf_state that names them (Real bytes)
struct LocalState {
   std::vector<uint8_t> u_prev, u_cur, u1b, u2b, vh1, gh1;
   pf_state st{};
};

inline void alloc_state(const Slab &s, LocalState &l) {
   const size_t rb = (size_t)s.sd.real_bytes, np = (size_t)s.sd.Npts * rb, nl = (size_t)s.sd.Nbl * rb;
   l.u_prev.assign(np, 0); l.u_cur.assign(np, 0);
   l.u1b.assign(nl, 0); l.u2b.assign(nl, 0);
   l.vh1.assign(nl * PF_MMB, 0); l.gh1.assign(nl * PF_MMB, 0);
   l.st.u_prev = l.u_prev.data(); l.st.u_cur = l.u_cur.data();
   l.st.u1b = l.u1b.data(); l.st.u2b = l.u2b.data(); l.st.vh1 = l.vh1.data(); l.st.gh1 = l.gh1.data();
}

namespace detail {
// planes [p0, p1) of the cut axis between a global field and the slab's local one (local plane = global plane - s.xlo); to_local: global -> local
inline void move_planes(const pf_simdata *g, const Slab &s, bool along_z, int64_t p0, int64_t p1, uint8_t *glob, uint8_t *loc, bool to_local) {
   const size_t rb = (size_t)g->real_bytes;
   if (p1 <= p0) return;
   if (!along_z) {
      const size_t plane = (size_t)(g->Ny * g->Nz) * rb;
      uint8_t *a = glob + (size_t)p0 * plane, *b = loc + (size_t)(p0 - s.xlo) * plane;
      if (to_local) memcpy(b, a, (size_t)(p1 - p0) * plane); else memcpy(a, b, (size_t)(p1 - p0) * plane);
      return;
   }
   const int64_t rows = g->Nx * g->Ny, nloc = s.xhi - s.xlo;
   const size_t w = (size_t)(p1 - p0) * rb;
   for (int64_t r = 0; r < rows; r++) {
      uint8_t *a = glob + (size_t)(r * g->Nz + p0) * rb, *b = loc + (size_t)(r * nloc + (p0 - s.xlo)) * rb;
      if (to_local) memcpy(b, a, w); else memcpy(a, b, w);
   }
}
// the slab's node rows of one array of `per` Reals per node
inline void move_rows(const pf_simdata *g, const Slab &s, int per, uint8_t *glob, uint8_t *loc, bool to_local) {
   const size_t w = (size_t)per * (size_t)g->real_bytes;
   for (size_t i = 0; i < s.bnl_rows.size(); i++) {
      uint8_t *a = glob + (size_t)s.bnl_rows[i] * w, *b = loc + i * w;
      if (to_local) memcpy(b, a, w); else memcpy(a, b, w);
   }
}
} // namespace detail

// g: the scene's pf_simdata and its state; l: alloc_state(s, l) done
inline void scatter_state(const pf_simdata *g, const pf_state *gs, const Slab &s, bool along_z, LocalState &l) {
   detail::move_planes(g, s, along_z, s.xlo, s.xhi, (uint8_t *)gs->u_prev, l.u_prev.data(), true);
   detail::move_planes(g, s, along_z, s.xlo, s.xhi, (uint8_t *)gs->u_cur, l.u_cur.data(), true);
   if (s.bnl_rows.empty()) return;
   detail::move_rows(g, s, 1, (uint8_t *)gs->u1b, l.u1b.data(), true);
   detail::move_rows(g, s, 1, (uint8_t *)gs->u2b, l.u2b.data(), true);
   detail::move_rows(g, s, PF_MMB, (uint8_t *)gs->vh1, l.vh1.data(), true);
   detail::move_rows(g, s, PF_MMB, (uint8_t *)gs->gh1, l.gh1.data(), true);
}
inline void gather_state(const pf_simdata *g, LocalState &l, const Slab &s, bool along_z, pf_state *gs) {
   detail::move_planes(g, s, along_z, s.x0, s.x1, (uint8_t *)gs->u_prev, l.u_prev.data(), false);
   detail::move_planes(g, s, along_z, s.x0, s.x1, (uint8_t *)gs->u_cur, l.u_cur.data(), false);
   if (s.bnl_rows.empty()) return;
   detail::move_rows(g, s, 1, (uint8_t *)gs->u1b, l.u1b.data(), false);
   detail::move_rows(g, s, 1, (uint8_t *)gs->u2b, l.u2b.data(), false);
   detail::move_rows(g, s, PF_MMB, (uint8_t *)gs->vh1, l.vh1.data(), false);
   detail::move_rows(g, s, PF_MMB, (uint8_t *)gs->gh1, l.gh1.data(), false);
}

} // namespace pf_cut
