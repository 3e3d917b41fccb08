// pf_absorb_cut.h -- the wall absorption maps of a scene (pffdtd_hip.h: pf_absorb) put together from the slabs of a chain and cut to them again.
//   node sums: a slab holds the rows cut_slab recorded for it (Slab::bnl_rows: the lossy entries of the planes it updates, in file order, disjoint
//              between slabs, as pf_state_cut.h's node state); gather_rows / scatter_rows move them to and from the scene's [Nbl] array;
//   bins:      a slab accounts the ABC nodes and sources of cut_slab's lists, which hold the planes it UPDATES -- owned planes only, never a ghost
//              plane -- so every one is counted by exactly one slab and the scene's bins are the slabs' bins added in slab order (add_bins: a fixed
//              order, so the sum is deterministic).  A set gives the scene's bins to slab 0 and zeros to the others: a get straight after it returns
//              the same doubles (x + 0.0 changes no bit).  A chain that goes on from there adds the same terms in another order than the chain in one
//              piece -- ((a0 + a1) + b0) + b1 against (a0 + b0) + (a1 + b1) -- so a RESUMED CHAIN's bins agree with the one-piece chain's to rounding
//              (Nbl * 2^-52 relative), not bit for bit; its node sums, each one slab's own, are bit-equal.  Single engines resume bit for bit.
// HOST ONLY, like pf_slab_cut.h: the public header and the standard library; tests/absorb_cut_check.cpp includes this file as it is.
#pragma once
#include <cstdint>
#include <vector>

#include "pf_slab_cut.h"

namespace pf_cut {

inline void gather_rows(const Slab &s, const double *local, double *scene) {
   for (size_t i = 0; i < s.bnl_rows.size(); i++) scene[s.bnl_rows[i]] = local[i];
}
inline void scatter_rows(const Slab &s, const double *scene, double *local) {
   for (size_t i = 0; i < s.bnl_rows.size(); i++) local[i] = scene[s.bnl_rows[i]];
}
inline void add_bins(double *sum, const double *part, int64_t n) {
   for (int64_t i = 0; i < n; i++) sum[i] += part[i];
}
// the scene's file index of a slab's local index (the inverse of cut_slab's `local`)
inline int64_t scene_index(const pf_simdata *sd, const Slab &s, bool along_z, int64_t local) {
   if (!along_z) return local + s.xlo * sd->Ny * sd->Nz;
   const int64_t nloc = s.xhi - s.xlo;
   return (local / nloc) * sd->Nz + local % nloc + s.xlo;
}

} // namespace pf_cut
