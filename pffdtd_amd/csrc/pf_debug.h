// pf_debug.h -- development and test switches, 0 in production.  Each PF_DBG_* bit forces an alternative arrangement the engine also
// contains -- an older kernel family, a fallback, one stream instead of two -- so that the tests can pin every path to the oracle and A/B
// measurements can be taken on one box.  INTERNAL: none of this is part of the drop-in boundary.  Round 6: the switches left the public
// pf_opts (include/pffdtd_hip.h); they reach the library through pf_internal_hooks below (exported, declared only here; pffdtd_amd/engine.py
// calls it for its `debug=` / `test_*=` keyword arguments) or the environment variable PFFDTD_DEBUG (a number, OR-ed in).
#pragma once
#include <vector>
#include "pffdtd_hip.h"
// the options as the engines and the chain see them: the public ones + the switches
struct pf_opts_x : pf_opts {
   int32_t debug;              // a mask of PF_DBG_* bits
   int32_t test_drop_exchange; // pf_multi_create: 1 + n = slab 1 misses the ghost planes of step n (the exchange self-check, which then always
                               // covers that step, must notice)
   int32_t test_faults;        // pf_multi_create: fault injection for the first-contact paths of a multi-device box.  1: no peer access between
                               // any two devices; 2: RCCL unusable; 4: the host thread of slab 1 stalls before the barrier of its fourth step
                               // (the watchdog of the others must turn the hang into an error)
};
// The switches of the NEXT pf_engine_create / pf_multi_create / pf_run_sim_devices / pf_slab_wall_scale call of the calling thread (that call
// clears them again).
extern "C" void pf_internal_hooks(int32_t debug, int32_t test_drop_exchange, int32_t test_faults);
pf_opts_x pf__take_hooks(const pf_opts *o); // *o (NULL: the defaults) + the calling thread's pending switches + PFFDTD_DEBUG
int pf__engine_create_x(const pf_simdata *sd, const pf_opts_x *o, pf_engine **out);
int pf__engine_get_region_x(pf_engine *e, int32_t which, const pf_region *r, void *host, int64_t pitch); // pf_engine_get_region with the output's rows `pitch` elements apart (0: dense)
// The region observers: field accumulators, band accumulators, vector band accumulators, decimating recorders and vector decimating recorders.  Their
// kinds (an engine's object and a handle are their kind's alone) and what a message calls their handle types and their chain functions (pf_multi_<name>_*).
namespace pfeng {
enum : int { OBS_ACCUM, OBS_BAND, OBS_VBAND, OBS_DECIM, OBS_VDECIM, OBS_ABSORB };
static const char *const obs_type[6] = {"pf_accum", "pf_bandacc", "pf_vbandacc", "pf_decim", "pf_vdecim", "pf_absorb"};
static const char *const obs_name[6] = {"accum", "bandacc", "vband", "decim", "vdecim", "absorb"};
}
// What the handle types of pffdtd_hip.h share.  An engine's handle: `eng` and the engine's own object `impl`.  A chain's: `chain` and, in the
// derived type's `part`, one engine handle per slab, null where the region misses the slab -- part[g] observes region_part(...).local of slab g; its
// rows land in the caller's arrays at out_off, the region's rows out_pitch and the device rows `cells` (of the whole region) apart.  `count` is kept
// here, by the C ABI; an engine's recorder keeps its own (pf_decim_count asks it).
struct pf_observer {
   pf_engine *eng = nullptr;
   void *impl = nullptr;
   pf_multi *chain = nullptr;
   pf_region region{};
   int64_t rc[3] = {0, 0, 0}, cells = 0; // the region's counts
   int64_t count = 0;
   virtual ~pf_observer() {}
};
struct pf_accum : pf_observer {
   static constexpr int kind = pfeng::OBS_ACCUM;
   std::vector<pf_accum *> part;
   int32_t nchan = 0;
};
struct pf_bandacc : pf_observer { // rows_e = nband * nbin, rows_s = (npre + nband * nsec) * 2 rows of `cells` doubles
   static constexpr int kind = pfeng::OBS_BAND;
   std::vector<pf_bandacc *> part;
   int64_t nbin = 0;
};
struct pf_vbandacc : pf_observer {
   static constexpr int kind = pfeng::OBS_VBAND;
   std::vector<pf_vbandacc *> part;
   int64_t nbin = 0;
};
// A chain's recorder: the slabs' parts advance together, and the chain keeps `count` and `rd` (the next frame a read gives) itself -- its refusals
// are host arithmetic.
struct pf_decim : pf_observer {
   static constexpr int kind = pfeng::OBS_DECIM;
   std::vector<pf_decim *> part;
   int64_t factor = 1, cap = 0, rd = 0;
};
struct pf_vdecim : pf_observer { // frames are [ncomp][cells], acc [ncomp][P][cells]
   static constexpr int kind = pfeng::OBS_VDECIM;
   std::vector<pf_vdecim *> part;
   int64_t factor = 1, cap = 0, rd = 0;
};
// The wall absorption maps (pf_engine_absorb.inc) observe no region: the lossy nodes, the ABC nodes and the sources of the engine.  A chain's: one part
// per slab, every slab (part[g] never null); the chain keeps `primed`, `last` and `count` itself, so a gap in n is refused before any slab is asked.
struct pf_absorb : pf_observer {
   static constexpr int kind = pfeng::OBS_ABSORB;
   std::vector<pf_absorb *> part;
   int32_t nbin = 0;
   bool primed = false;
   int64_t last = -1;
};
// pf_engine_*_get / _set / _read / _get_state / _set_state with the caller's region rows `pitch` and channel / sum / state / frame / acc rows `rowstride`
// doubles apart (0: dense) -- a slab's cells of a chain's arrays; count: as given.  The band accumulators': `a` is a pf_bandacc (scalar) or a pf_vbandacc; the
// recorders': a pf_decim (scalar) or a pf_vdecim.
int pf__engine_accum_get_x(pf_engine *e, pf_accum *a, double *host, int64_t pitch, int64_t chstride);
int pf__engine_accum_set_x(pf_engine *e, pf_accum *a, const double *host, int64_t pitch, int64_t chstride, int64_t count);
int pf__engine_bands_get_x(pf_engine *e, pf_observer *a, bool scalar, double *sums, double *state, int64_t pitch, int64_t rowstride);
int pf__engine_bands_set_x(pf_engine *e, pf_observer *a, bool scalar, const double *sums, const double *state, int64_t pitch, int64_t rowstride, int64_t count);
int pf__engine_rec_read_x(pf_engine *e, pf_observer *a, bool scalar, double *frames, int64_t max_frames, int64_t *first, int64_t *nread, int64_t pitch, int64_t rowstride);
int pf__engine_rec_get_state_x(pf_engine *e, pf_observer *a, bool scalar, double *acc, double *state, int64_t pitch, int64_t rowstride);
int pf__engine_rec_set_state_x(pf_engine *e, pf_observer *a, bool scalar, const double *acc, const double *state, int64_t pitch, int64_t rowstride, int64_t count);
int pf__engine_between_runs(pf_engine *e); // 1: not inside a split-phase step or pass (what pf_engine_accum_add needs)
enum : int {
   PF_DBG_BRANCH_SELECTS = 0x1,       // three-step wall regions: fd_regs' select form (a branch count per lane) even where every material has the same count
   PF_DBG_STORE_UNREAD = 0x2,         // three-step wall regions: u^{n+1} of their cells goes to the scratch grid even where nothing reads it
   PF_DBG_STRIPS_PER_LANE = 0x4,      // three-step column strips with a uniform branch count: every lane loads and stores its own pencil, no staging through LDS (pf_strip_map.h)
   PF_DBG_RUNTIME_NODES = 0x20,      // three-step wall regions: the bodies that read the node words from their blocks, never the ones with a wall profile compiled in
   PF_DBG_LW32 = 0x100,               // 32-lane row segments (0x200: 16-lane, 0x400: 64-lane) instead of the measured choice
   PF_DBG_LW16 = 0x200,
   PF_DBG_LW64 = 0x400,
   PF_DBG_SRC_TILES_SINGLE = 0x40,    // triples: the tiles within reach of a source (and a receiver's tile) step singly, the sources added by k_io (until round 6)
   PF_DBG_EDGE_SEPARATE = 0x80,       // slab triples: the edge planes of the two sides by separate launches (lean kernel, boundary kernel), as in round 5
   PF_DBG_RUNTIME_GEOMETRY = 0x800,   // three-step wall regions: the bodies with run-time pencil geometry, never the ones with it compiled in
   PF_DBG_SWZ_ON = 0x1000,            // store the grid with the file's x and z axes exchanged (0x2000: never; default: decided per scene)
   PF_DBG_SWZ_OFF = 0x2000,
   PF_DBG_SINGLE_STEPS = 0x4000,      // single steps only (no blocked pairs / triples)
   PF_DBG_NO_AUTOTUNE = 0x8000,       // no creation-time measurement: static rules choose the kernel, grids stay as allocated
   PF_DBG_WALLS_BESIDE_BOX = 0x10000, // experiment: a triple's alike wall launches beside k_tb3 instead of before it
   PF_DBG_NO_TRIPLES = 0x20000,       // never three steps per pass (pairs as in round 4)
   PF_DBG_FCC_PAIR_R4 = 0x40000,      // 13-point pairs by the round-4 kernel k_tb2_fcc_x (A/B measurements)
   PF_DBG_THIRD_STEP_LISTS = 0x80000, // the third step of a single domain's triple by the list kernels (round-5 start); no bricks
   PF_DBG_BND_PLAIN_ORDER = 0x100000, // boundary pass in plain workgroup order (no XCD-aware runs)
   PF_DBG_BND_FETCH_ALL = 0x200000,   // ... fetches the neighbours inside the wall too
   PF_DBG_FRAME_GENERIC = 0x400000,   // the frame of the shell (edges, corners) as generic blocks of k_wall2 (round 5) instead of bricks (pf_brick.h)
   PF_DBG_GRAPH = 0x800000,           // replay the single-step loop from a hipGraph (six steps per graph; no faster on this stack)
   PF_DBG_XY_TWO_PLUS_ONE = 0x1000000,// a triple's x / y wall regions take two steps + one instead of three in one pass (k_wall2 NS = 3)
   PF_DBG_STRIPS_SPLIT = 0x2000000,   // wide column strips cut in two (12- + 16-cell pencils)
   PF_DBG_WALLS_ONE_STREAM = 0x4000000, // every launch of a blocked pass on the main stream
   PF_DBG_WALLS_ALL_GENERIC = 0x8000000, // wall regions: every block generic (no alike fast path, no bricks)
   PF_DBG_NO_WALL_REGIONS = 0x10000000, // blocked pairs keep the single-step shell
   PF_DBG_BND_ALL_NODES = 0x20000000, // the boundary-list kernel visits every node (none left to the column-strip kernel)
   PF_DBG_STRIPS_TWO_PLUS_ONE = 0x40000000, // a triple's column strips take two steps + one instead of three in one pass
};
