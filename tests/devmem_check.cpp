// devmem_check.cpp -- the engine's owner of device allocations (pffdtd_amd/csrc/pf_devmem.h) over real malloc'ed blocks and a counting fake free
// function, as a program of its own: tests/test_devmem.py compiles it with the host compiler under the address and undefined-behaviour sanitizers
// and runs it once (a block freed twice or never is the sanitizers' finding as well as this program's).  Prints the violated condition on stderr
// and returns non-zero.
//   * every taken block is freed exactly once: by release, by the destructor, by both in a mix;
//   * release of null, of a pointer never taken and of one released before frees nothing and reports false;
//   * release nulls the caller's pointer;
//   * take, release, take again of the SAME address (an allocator reuses addresses: Engine::upload relies on it);
//   * a pool of six with two foreign members: "adopt two, release the rest" frees the owned members it should, the foreign ones never.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "pf_devmem.h"

namespace {

int g_bad = 0;
void check(bool ok, const char *fmt, ...) {
   if (ok) return;
   g_bad++;
   fprintf(stderr, "devmem_check: ");
   va_list ap;
   va_start(ap, fmt);
   vfprintf(stderr, fmt, ap);
   va_end(ap);
   fprintf(stderr, "\n");
}

std::map<void *, int> g_freed; // address -> how often the fake was handed it
int g_calls = 0;
bool g_really_free = true;
void counting_free(void *p) {
   g_freed[p]++;
   g_calls++;
   if (g_really_free) free(p);
}
void reset() { g_freed.clear(); g_calls = 0; }
int *block() { return (int *)malloc(64); }

void all_freed_once(const std::vector<int *> &blocks, const char *what) {
   for (size_t i = 0; i < blocks.size(); i++) check(g_freed[blocks[i]] == 1, "%s: block %zu freed %d times", what, i, g_freed[blocks[i]]);
   check(g_calls == (int)blocks.size(), "%s: %d calls of the free function for %zu blocks", what, g_calls, blocks.size());
}

void by_destructor() {
   reset();
   std::vector<int *> b;
   {
      pf::DevMem m(counting_free);
      for (int i = 0; i < 5; i++) { int *p = block(); check(m.take(p) == p, "take returns its argument"); b.push_back(p); }
      check(m.take((int *)nullptr) == nullptr && m.size() == 5, "take(null) records nothing");
      for (int *p : b) check(m.owns(p), "owns a taken block");
      check(g_calls == 0, "nothing freed before the destructor");
   }
   all_freed_once(b, "destructor");
}

void by_release_and_mix() {
   reset();
   std::vector<int *> b;
   {
      pf::DevMem m(counting_free);
      for (int i = 0; i < 6; i++) b.push_back(m.take(block()));
      for (int i : {4, 0, 2}) { // out of order
         int *p = b[i];
         check(m.release(p), "release of an owned block reports true");
         check(p == nullptr, "release nulls the caller's pointer");
         check(!m.owns(b[i]) && g_freed[b[i]] == 1, "a released block is freed and no longer owned");
      }
      check(g_calls == 3 && m.size() == 3, "three released, three left");
      m.release_all();
      check(g_calls == 6 && m.size() == 0, "release_all frees what is left");
      m.release_all(); // (and the destructor after it)
   }
   all_freed_once(b, "release + release_all + destructor");
}

void refusals() {
   reset();
   int *foreign = block();
   {
      pf::DevMem m(counting_free);
      int *own = m.take(block()), *null = nullptr, *f = foreign;
      check(!m.release(null) && null == nullptr, "release(null) reports false");
      check(!m.release(f) && f == foreign, "release of a pointer never taken reports false and leaves the pointer");
      check(!m.owns(foreign) && !m.owns(nullptr), "owns: neither a foreign pointer nor null");
      int *again = own, *first = own;
      check(m.release(first), "release of the owned block");
      check(!m.release(again) && again == own, "release of a pointer released before reports false");
      check(g_calls == 1 && g_freed[own] == 1 && g_freed.count(foreign) == 0, "only the owned block was freed, once");
   }
   check(g_calls == 1, "the destructor frees nothing that was released");
   free(foreign);
}

void same_address_again() {
   reset();
   g_really_free = false; // the "allocator" hands the same block out again
   int *p = block();
   {
      pf::DevMem m(counting_free);
      int *a = m.take(p);
      check(m.release(a) && g_freed[p] == 1, "first life freed");
      int *b = m.take(p);
      check(m.owns(p) && m.size() == 1, "taken again at the same address: owned, once");
      check(m.release(b) && g_freed[p] == 2 && !m.owns(p), "second life freed");
      m.take(p);
   }
   check(g_freed[p] == 3 && g_calls == 3, "three lives of one address: three frees (got %d)", g_calls);
   g_really_free = true;
   free(p);
}

void adopt_two_release_the_rest() {
   for (int keep_foreign = 0; keep_foreign < 2; keep_foreign++) {
      reset();
      int *foreign[2] = {block(), block()};
      std::vector<int *> owned;
      {
         pf::DevMem m(counting_free);
         for (int i = 0; i < 4; i++) owned.push_back(m.take(block()));
         const std::vector<int *> pool = {owned[0], foreign[0], owned[1], owned[2], foreign[1], owned[3]};
         // adopt the caller's two (all four owned members go) / adopt two of the owner's (the other two go)
         const std::vector<int *> keep = keep_foreign ? std::vector<int *>{foreign[0], foreign[1]} : std::vector<int *>{owned[1], owned[3]};
         const int n = m.release_rest(pool, keep);
         check(n == (keep_foreign ? 4 : 2) && g_calls == n, "release_rest freed %d blocks (%d calls)", n, g_calls);
         for (int i = 0; i < 4; i++) {
            const bool kept = !keep_foreign && (i == 1 || i == 3);
            check(g_freed[owned[i]] == (kept ? 0 : 1) && m.owns(owned[i]) == kept, "owned member %d: freed %d times, kept %d", i, g_freed[owned[i]], (int)kept);
         }
         check(g_freed.count(foreign[0]) == 0 && g_freed.count(foreign[1]) == 0, "a foreign member was handed to the free function");
      }
      for (int i = 0; i < 4; i++) check(g_freed[owned[i]] == 1, "owned member %d freed %d times in all", i, g_freed[owned[i]]);
      check(g_calls == 4 && g_freed.count(foreign[0]) == 0 && g_freed.count(foreign[1]) == 0, "the foreign members are the caller's to the end");
      foreign[0][0] = 1; foreign[1][15] = 2; // (still the caller's memory: the address sanitizer agrees)
      free(foreign[0]); free(foreign[1]);
   }
}

} // namespace

int main() {
   by_destructor();
   by_release_and_mix();
   refusals();
   same_address_again();
   adopt_two_release_the_rest();
   return g_bad ? 1 : 0;
}
