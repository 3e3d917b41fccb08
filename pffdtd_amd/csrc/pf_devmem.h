// pf_devmem.h -- who frees what the engine allocates on the device: one list of owned allocations and the function that frees one.
//   take(p):    p is the owner's from now on (returns p);
//   release(p): frees p and nulls the caller's pointer -- if p is owned.  Null, a pointer never taken (a caller's grid: pf_opts.ext_u0 / ext_u1, the
//               pools of pf_engine_place_grids pass through the same code) and one released before: nothing is freed, and the result says so;
//   the destructor (release_all) frees what is left, each allocation once.
// Roles (u0 / u1, ub[], bufC ...) stay raw pointers that rotate and swap; ownership goes by address and does not follow them.
// HOST ONLY, like pf_slab_cut.h: the standard library, and the free function is handed in; tests/devmem_check.cpp includes this file as it is.
#pragma once
#include <algorithm>
#include <vector>

namespace pf {

class DevMem {
 public:
   typedef void (*FreeFn)(void *);
   explicit DevMem(FreeFn f) : free_(f) {}
   DevMem(const DevMem &) = delete;
   DevMem &operator=(const DevMem &) = delete;
   ~DevMem() { release_all(); }

   template <typename T> T *take(T *p) {
      if (p) owned_.push_back((void *)p);
      return p;
   }
   bool owns(const void *p) const { return p && std::find(owned_.begin(), owned_.end(), p) != owned_.end(); }
   template <typename T> bool release(T *&p) {
      const auto it = std::find(owned_.begin(), owned_.end(), (void *)p);
      if (!p || it == owned_.end()) return false;
      owned_.erase(it);
      free_((void *)p);
      p = nullptr;
      return true;
   }
   // adopt `keep`, release the rest of `pool`, in the pool's order; returns how many were freed (members that are not owned stay as they are)
   template <typename T> int release_rest(const std::vector<T *> &pool, const std::vector<T *> &keep) {
      int n = 0;
      for (T *g : pool)
         if (std::find(keep.begin(), keep.end(), g) == keep.end()) n += release(g) ? 1 : 0;
      return n;
   }
   void release_all() {
      for (void *p : owned_) free_(p);
      owned_.clear();
   }
   size_t size() const { return owned_.size(); }

 private:
   FreeFn free_;
   std::vector<void *> owned_;
};

} // namespace pf
