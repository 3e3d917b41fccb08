// pf_engine.hip -- host side of libpffdtd_hip.so: the C ABI of include/pffdtd_hip.h over the kernels of
// pf_kernels.h.  Replaces the reference's `double run_sim(struct SimData*)` (c_cuda/gpu_engine.h:665-1255,
// c_cuda/cpu_engine.h:52-360) for MI355X.  Not derived from gpu_engine.h: different memory layout (padded
// pitch, engine-built skip-mask), different kernels (2.5D register marching), device-resident source signals
// and receiver ring instead of per-step host traffic, and a split-phase step for overlapped slab exchange.
#include "pf_engine_class.inc"

namespace {
thread_local std::string g_err;
}
std::mutex pf__tune_mu[64]; // creation-time measurements of engines that share a device run one at a time (both precisions)

// internal: lets the other translation units of this library (pf_vox.hip) feed pf_last_error()
extern "C" void pf__set_error(const char *msg) { g_err = msg ? msg : ""; }

// internal (pf_engine.hip, pf_multi.hip): would this scene rather be stored with the file's x and z axes exchanged (Engine::swz)?
// Rooms only -- a box-shaped room (most boundary nodes within a few cells of a grid face) steps in blocked pairs, which exist
// for the file's axis order alone --, when clearly more boundary nodes have their successor ALONG FILE X in the list than
// along file z: those runs become unit-stride runs, the others a row apart.  counts[0..1] = the two run counts.
extern "C" int pf__axis_exchange_pays(const pf_simdata *sd, int64_t *counts) {
   if (counts) counts[0] = counts[1] = 0;
   const int64_t fNx = sd->Nx, fNy = sd->Ny, fNz = sd->Nz;
   if (sd->Nb < 100000 || sd->Npts > ((int64_t)1 << 34) || fNx <= fNz) return 0; // (small scenes: nothing to gain; the bitmap below is Npts / 8 bytes)
   const int64_t NzNy = fNz * fNy;
   std::vector<uint64_t> bits;
   try { bits.assign((size_t)(sd->Npts >> 6) + 1, 0); } catch (const std::bad_alloc &) { return 0; } // (no room for the bitmap: file order; nothing may cross the C ABI)
   int64_t near_face = 0;
   for (int64_t i = 0; i < sd->Nb; i++) {
      const int64_t ii = sd->bn_ixyz[i];
      if (ii < 0 || ii >= sd->Npts) return 0; // (reported by the engine's own checks)
      bits[(size_t)(ii >> 6)] |= (uint64_t)1 << (ii & 63);
      const int64_t fz = ii % fNz, fy = (ii / fNz) % fNy, fx = ii / NzNy;
      const int64_t d = std::min(std::min(std::min(fx, fNx - 1 - fx), std::min(fy, fNy - 1 - fy)), std::min(fz, fNz - 1 - fz));
      near_face += d < 16;
   }
   if (near_face * 10 >= sd->Nb * 8) return 0; // a box-shaped room
   auto has = [&](int64_t ii) { return ii < sd->Npts && ((bits[(size_t)(ii >> 6)] >> (ii & 63)) & 1u) != 0; };
   int64_t run_z = 0, run_x = 0;
   for (int64_t i = 0; i < sd->Nb; i++) {
      const int64_t ii = sd->bn_ixyz[i];
      run_z += has(ii + 1);
      run_x += has(ii + NzNy);
   }
   if (counts) { counts[0] = run_x; counts[1] = run_z; }
   // measured (profiles/r03_reference_configs.jsonl): CTK church 3.46 M / 2.75 M (x / z successors) +12-15 % exchanged, Musikverein
   // 17.2 M / 14.4 M +11 %
   return (double)run_x > 1.1 * (double)run_z && run_x - run_z > sd->Nb / 20;
}


struct pf_engine {
   pfeng::EngineBase *impl;
   std::vector<pf_observer *> observers; // the handles of its region observers still alive (pf_engine_destroy frees those left)
};
pfeng::EngineBase *pf__new_engine_f64(const pf_simdata *sd, const pf_opts_x *o, int *rc); // pf_engine_f64.hip

extern "C" {

const char *pf_last_error(void) { return g_err.c_str(); }
const char *pf_version(void) { return "pffdtd_hip 0.3 (gfx950)"; }

int pf_device_count(void) {
   int n = 0;
   if (hipGetDeviceCount(&n) != hipSuccess) return 0;
   return n;
}

int64_t pf_grid_pitch(int64_t Nz, int32_t real_bytes) {
   if (real_bytes != 4 && real_bytes != 8) return -1;
   return grid_pitch(Nz, real_bytes);
}
size_t pf_grid_bytes(int64_t Nx, int64_t Ny, int64_t Nz, int32_t real_bytes) {
   if (real_bytes != 4 && real_bytes != 8) return 0;
   return (size_t)(Nx * Ny * grid_pitch(Nz, real_bytes)) * (size_t)real_bytes;
}

void pf_opts_default(pf_opts *o) {
   if (!o) return;
   memset(o, 0, sizeof *o);
   o->slab_first = 1;
   o->slab_last = 1;
}

// development / test switches (pf_debug.h): pending for the next create call of this thread
static thread_local int32_t t_hooks[3] = {0, 0, 0};
void pf_internal_hooks(int32_t debug, int32_t test_drop_exchange, int32_t test_faults) {
   t_hooks[0] = debug; t_hooks[1] = test_drop_exchange; t_hooks[2] = test_faults;
}

int pf_engine_create(const pf_simdata *sd, const pf_opts *opts, pf_engine **out) {
   const pf_opts_x o = pf__take_hooks(opts);
   return pf__engine_create_x(sd, &o, out);
}

} // extern "C"

pf_opts_x pf__take_hooks(const pf_opts *opts) {
   pf_opts_x x{};
   if (opts) static_cast<pf_opts &>(x) = *opts; else pf_opts_default(&x);
   x.debug = t_hooks[0]; x.test_drop_exchange = t_hooks[1]; x.test_faults = t_hooks[2];
   t_hooks[0] = t_hooks[1] = t_hooks[2] = 0;
   if (const char *e = getenv("PFFDTD_DEBUG")) x.debug |= (int32_t)strtol(e, nullptr, 0);
   return x;
}

int pf__engine_create_x(const pf_simdata *sd, const pf_opts_x *opts, pf_engine **out) {
   if (!sd || !out || !opts) return set_err(PF_ERR_ARG, "null argument");
   *out = nullptr;
   pf_opts_x o = *opts;
   if (o.layout == PF_LAYOUT_EXCHANGED) o.debug |= PF_DBG_SWZ_ON; // (the engine's own switches: the same two bits the tests force)
   else if (o.layout == PF_LAYOUT_FILE) o.debug |= PF_DBG_SWZ_OFF;
   else if (o.layout != PF_LAYOUT_AUTO) return set_err(PF_ERR_ARG, "pf_opts.layout must be PF_LAYOUT_AUTO, _EXCHANGED or _FILE");
   pfeng::EngineBase *impl = nullptr;
   int rc;
   if (sd->real_bytes == 4) {
      auto *e = new Engine<float>();
      rc = e->init(sd, &o);
      impl = e;
#ifndef PF_DEV_F32_ONLY // (development builds, PFFDTD_DEV_F32=1 in pffdtd_amd/build.py: the fp32 unit alone; never shipped)
   } else if (sd->real_bytes == 8) {
      impl = pf__new_engine_f64(sd, &o, &rc);
#endif
   } else {
      return set_err(PF_ERR_ARG, "real_bytes must be 4 or 8 (got %d)", sd->real_bytes);
   }
   if (rc) { std::string keep = g_err; delete impl; g_err = keep; return rc; }
   *out = new pf_engine{impl, {}};
   return PF_OK;
}

// internal (pf_multi.hip): the region's rows land `pitch` elements apart in `host` -- a slab's columns of a chain's dense output
int pf__engine_get_region_x(pf_engine *e, int32_t which, const pf_region *r, void *host, int64_t pitch) {
   if (!e || !e->impl) return set_err(PF_ERR_ARG, "null engine");
   return e->impl->get_region(which, r, host, pitch);
}

// region observers (pf_debug.h): the handle must be this engine's (a chain's handle, or another engine's, is refused before the engine sees it; one of
// another kind is refused by the engine, which looks its object up by kind)
static int mine(pf_engine *e, const pf_observer *a, int kind, const char *what) {
   if (!e || !e->impl) return set_err(PF_ERR_ARG, "%s: null engine", what);
   if (!a) return set_err(PF_ERR_ARG, "%s: null %s", what, pfeng::obs_type[kind]);
   if (a->eng != e) {
      char chain[64] = "";
      if (a->chain) snprintf(chain, sizeof chain, " (it is a chain's: pf_multi_%s_*)", pfeng::obs_name[kind]);
      return set_err(PF_ERR_ARG, "%s: the %s belongs to another engine%s", what, pfeng::obs_type[kind], chain);
   }
   return PF_OK;
}
// make(&impl): the engine's create call
template <typename T, typename Make> static int create(pf_engine *e, const char *what, const pf_region *r, T **out, Make make) {
   if (!e || !e->impl) return set_err(PF_ERR_ARG, "%s: null engine", what);
   if (!out) return set_err(PF_ERR_ARG, "%s: null out", what);
   *out = nullptr;
   void *impl = nullptr;
   const int rc = make(&impl);
   if (rc) return rc;
   T *a = new T();
   a->eng = e; a->impl = impl; a->region = *r;
   a->cells = pf_cut::region_counts(r, a->rc);
   e->observers.push_back(a);
   *out = a;
   return PF_OK;
}
// the accumulators' add and set: the engine's call, then the count the C ABI keeps
template <typename Add> static int add_counted(pf_engine *e, pf_observer *a, int kind, const char *what, Add add) {
   int rc = mine(e, a, kind, what);
   if (rc || (rc = add())) return rc;
   a->count++;
   return PF_OK;
}
template <typename Set> static int set_counted(pf_engine *e, pf_observer *a, int kind, const char *what, int64_t count, Set set) {
   int rc = mine(e, a, kind, what);
   if (rc) return rc;
   if (count < 0) return set_err(PF_ERR_ARG, "%s: count = %ld < 0", what, (long)count);
   if ((rc = set())) return rc;
   a->count = count;
   return PF_OK;
}
static int destroy(pf_engine *e, pf_observer *a, int kind, const char *what) {
   int rc = mine(e, a, kind, what);
   if (rc || (rc = e->impl->observer_destroy(what, kind, a->impl))) return rc;
   e->observers.erase(std::find(e->observers.begin(), e->observers.end(), a));
   delete a;
   return PF_OK;
}
// (an engine's recorder asks the engine's object; a chain's keeps the two numbers itself)
template <typename T> static void rec_numbers(const T *a, int64_t *count, int64_t *pending) {
   *count = *pending = -1;
   if (!a) return;
   if (a->chain) { *count = a->count; *pending = (a->count + a->factor - 1) / a->factor - a->rd; }
   else if (a->eng && a->eng->impl) a->eng->impl->vdecim_info(T::kind == pfeng::OBS_DECIM, a->impl, count, pending);
}
// a kind with a scalar and a vector form: the public function's name and the handle's kind
#define PF_TWO(scalar, s, v, S, V, fn) const char *what = (scalar) ? "pf_engine_" s "_" fn : "pf_engine_" v "_" fn; const int kind = (scalar) ? pfeng::S : pfeng::V
#define PF_BANDS(scalar, fn) PF_TWO(scalar, "bandacc", "vband", OBS_BAND, OBS_VBAND, fn)
#define PF_REC(scalar, fn) PF_TWO(scalar, "decim", "vdecim", OBS_DECIM, OBS_VDECIM, fn)

// internal (pf_multi.hip): a slab's cells of a chain's arrays
int pf__engine_accum_get_x(pf_engine *e, pf_accum *a, double *host, int64_t pitch, int64_t chstride) {
   const int rc = mine(e, a, pfeng::OBS_ACCUM, "pf_engine_accum_get");
   return rc ? rc : e->impl->accum_get(a->impl, host, pitch, chstride);
}
int pf__engine_accum_set_x(pf_engine *e, pf_accum *a, const double *host, int64_t pitch, int64_t chstride, int64_t count) {
   return set_counted(e, a, pfeng::OBS_ACCUM, "pf_engine_accum_set", count, [&] { return e->impl->accum_set(a->impl, host, pitch, chstride); });
}
int pf__engine_bands_get_x(pf_engine *e, pf_observer *a, bool scalar, double *sums, double *state, int64_t pitch, int64_t rowstride) {
   PF_BANDS(scalar, "get");
   const int rc = mine(e, a, kind, what);
   return rc ? rc : e->impl->vband_get(what, scalar, a->impl, sums, state, pitch, rowstride);
}
int pf__engine_bands_set_x(pf_engine *e, pf_observer *a, bool scalar, const double *sums, const double *state, int64_t pitch, int64_t rowstride, int64_t count) {
   PF_BANDS(scalar, "set");
   return set_counted(e, a, kind, what, count, [&] { return e->impl->vband_set(what, scalar, a->impl, sums, state, pitch, rowstride); });
}
static int bands_add(pf_engine *e, pf_observer *a, bool scalar, int64_t bin) {
   PF_BANDS(scalar, "add");
   return add_counted(e, a, kind, what, [&] { return e->impl->vband_add(what, scalar, a->impl, bin); });
}
int pf__engine_rec_read_x(pf_engine *e, pf_observer *a, bool scalar, double *frames, int64_t max_frames, int64_t *first, int64_t *nread, int64_t pitch, int64_t rowstride) {
   PF_REC(scalar, "read");
   const int rc = mine(e, a, kind, what);
   return rc ? rc : e->impl->vdecim_read(what, scalar, a->impl, frames, max_frames, first, nread, pitch, rowstride);
}
int pf__engine_rec_get_state_x(pf_engine *e, pf_observer *a, bool scalar, double *acc, double *state, int64_t pitch, int64_t rowstride) {
   PF_REC(scalar, "get_state");
   const int rc = mine(e, a, kind, what);
   return rc ? rc : e->impl->vdecim_get_state(what, scalar, a->impl, acc, state, pitch, rowstride);
}
int pf__engine_rec_set_state_x(pf_engine *e, pf_observer *a, bool scalar, const double *acc, const double *state, int64_t pitch, int64_t rowstride, int64_t count) {
   PF_REC(scalar, "set_state");
   const int rc = mine(e, a, kind, what);
   return rc ? rc : e->impl->vdecim_set_state(what, scalar, a->impl, acc, state, pitch, rowstride, count);
}
static int rec_add(pf_engine *e, pf_observer *a, bool scalar) {
   PF_REC(scalar, "add");
   const int rc = mine(e, a, kind, what);
   return rc ? rc : e->impl->vdecim_add(what, scalar, a->impl);
}
#undef PF_REC
#undef PF_BANDS
#undef PF_TWO
int pf__engine_between_runs(pf_engine *e) { return e && e->impl && e->impl->between_runs() ? 1 : 0; }

extern "C" {

void pf_engine_destroy(pf_engine *e) {
   if (!e) return;
   for (pf_observer *a : e->observers) delete a; // (their device memory is the engine's: freed with it)
   delete e->impl;
   delete e;
}

int pf_engine_accum_create(pf_engine *e, const pf_region *r, int32_t nchan, int32_t depth, pf_accum **out) {
   const int rc = create(e, "pf_engine_accum_create", r, out, [&](void **impl) { return e->impl->accum_create(r, nchan, depth, impl); });
   if (rc == PF_OK) (*out)->nchan = nchan;
   return rc;
}
int pf_engine_accum_add(pf_engine *e, pf_accum *a, const double *w) {
   return add_counted(e, a, pfeng::OBS_ACCUM, "pf_engine_accum_add", [&] { return e->impl->accum_add(a->impl, w); });
}
int pf_engine_accum_get(pf_engine *e, pf_accum *a, double *host) { return pf__engine_accum_get_x(e, a, host, 0, 0); }
int pf_engine_accum_set(pf_engine *e, pf_accum *a, const double *host, int64_t count) { return pf__engine_accum_set_x(e, a, host, 0, 0, count); }
int64_t pf_accum_count(const pf_accum *a) { return a ? a->count : -1; }
int pf_engine_accum_destroy(pf_engine *e, pf_accum *a) { return destroy(e, a, pfeng::OBS_ACCUM, "pf_engine_accum_destroy"); }

// the scalar band accumulator is the vector one with the one component 0, the one product (0, 0, 0) and a handle type of its own
int pf_engine_bandacc_create(pf_engine *e, const pf_region *r, int32_t npre, const double *pre_sos, int32_t nband, int32_t nsec, const double *band_sos, int64_t nbin,
                             int32_t depth, pf_bandacc **out) {
   static const int32_t cell[1] = {0}, square[3] = {0, 0, 0};
   const char *what = "pf_engine_bandacc_create";
   const int rc = create(e, what, r, out, [&](void **impl) { return e->impl->vband_create(what, true, r, 1, cell, npre, pre_sos, nband, nsec, band_sos, 1, square, nbin, depth, impl); });
   if (rc == PF_OK) (*out)->nbin = nbin;
   return rc;
}
int pf_engine_bandacc_add(pf_engine *e, pf_bandacc *a, int64_t bin) { return bands_add(e, a, true, bin); }
int pf_engine_bandacc_get(pf_engine *e, pf_bandacc *a, double *sums, double *state) { return pf__engine_bands_get_x(e, a, true, sums, state, 0, 0); }
int pf_engine_bandacc_set(pf_engine *e, pf_bandacc *a, const double *sums, const double *state, int64_t count) { return pf__engine_bands_set_x(e, a, true, sums, state, 0, 0, count); }
int64_t pf_bandacc_count(const pf_bandacc *a) { return a ? a->count : -1; }
int pf_engine_bandacc_destroy(pf_engine *e, pf_bandacc *a) { return destroy(e, a, pfeng::OBS_BAND, "pf_engine_bandacc_destroy"); }

int pf_engine_vband_create(pf_engine *e, const pf_region *r, int32_t ncomp, const int32_t *comp, int32_t npre, const double *pre_sos, int32_t nband, int32_t nsec,
                           const double *band_sos, int32_t nprod, const int32_t *prod, int64_t nbin, int32_t depth, pf_vbandacc **out) {
   const char *what = "pf_engine_vband_create";
   const int rc = create(e, what, r, out,
                         [&](void **impl) { return e->impl->vband_create(what, false, r, ncomp, comp, npre, pre_sos, nband, nsec, band_sos, nprod, prod, nbin, depth, impl); });
   if (rc == PF_OK) (*out)->nbin = nbin;
   return rc;
}
int pf_engine_vband_add(pf_engine *e, pf_vbandacc *a, int64_t bin) { return bands_add(e, a, false, bin); }
int pf_engine_vband_get(pf_engine *e, pf_vbandacc *a, double *sums, double *state) { return pf__engine_bands_get_x(e, a, false, sums, state, 0, 0); }
int pf_engine_vband_set(pf_engine *e, pf_vbandacc *a, const double *sums, const double *state, int64_t count) { return pf__engine_bands_set_x(e, a, false, sums, state, 0, 0, count); }
int64_t pf_vbandacc_count(const pf_vbandacc *a) { return a ? a->count : -1; }
int pf_engine_vband_destroy(pf_engine *e, pf_vbandacc *a) { return destroy(e, a, pfeng::OBS_VBAND, "pf_engine_vband_destroy"); }

// the scalar recorder is the vector recorder with the one component 0 and a handle type of its own
int pf_engine_decim_create(pf_engine *e, const pf_region *r, int32_t npre, const double *pre_sos, int32_t ntap, const double *taps, int32_t factor, int64_t cap,
                           int32_t depth, pf_decim **out) {
   static const int32_t cell[1] = {0};
   const char *what = "pf_engine_decim_create";
   const int rc = create(e, what, r, out, [&](void **impl) { return e->impl->vdecim_create(what, true, r, 1, cell, npre, pre_sos, ntap, taps, factor, cap, depth, impl); });
   if (rc == PF_OK) { (*out)->factor = factor; (*out)->cap = cap; }
   return rc;
}
int pf_engine_decim_add(pf_engine *e, pf_decim *a) { return rec_add(e, a, true); }
int pf_engine_decim_read(pf_engine *e, pf_decim *a, double *frames, int64_t max_frames, int64_t *first, int64_t *nread) {
   return pf__engine_rec_read_x(e, a, true, frames, max_frames, first, nread, 0, 0);
}
int pf_engine_decim_get_state(pf_engine *e, pf_decim *a, double *acc, double *state) { return pf__engine_rec_get_state_x(e, a, true, acc, state, 0, 0); }
int pf_engine_decim_set_state(pf_engine *e, pf_decim *a, const double *acc, const double *state, int64_t count) {
   return pf__engine_rec_set_state_x(e, a, true, acc, state, 0, 0, count);
}
int64_t pf_decim_count(const pf_decim *a) { int64_t c, p; rec_numbers(a, &c, &p); return c; }
int64_t pf_decim_pending(const pf_decim *a) { int64_t c, p; rec_numbers(a, &c, &p); return p; }
int pf_engine_decim_destroy(pf_engine *e, pf_decim *a) { return destroy(e, a, pfeng::OBS_DECIM, "pf_engine_decim_destroy"); }

int pf_engine_vdecim_create(pf_engine *e, const pf_region *r, int32_t ncomp, const int32_t *comp, int32_t npre, const double *pre_sos, int32_t ntap, const double *taps,
                            int32_t factor, int64_t cap, int32_t depth, pf_vdecim **out) {
   const char *what = "pf_engine_vdecim_create";
   const int rc = create(e, what, r, out, [&](void **impl) { return e->impl->vdecim_create(what, false, r, ncomp, comp, npre, pre_sos, ntap, taps, factor, cap, depth, impl); });
   if (rc == PF_OK) { (*out)->factor = factor; (*out)->cap = cap; }
   return rc;
}
int pf_engine_vdecim_add(pf_engine *e, pf_vdecim *a) { return rec_add(e, a, false); }
int pf_engine_vdecim_read(pf_engine *e, pf_vdecim *a, double *frames, int64_t max_frames, int64_t *first, int64_t *nread) {
   return pf__engine_rec_read_x(e, a, false, frames, max_frames, first, nread, 0, 0);
}
int pf_engine_vdecim_get_state(pf_engine *e, pf_vdecim *a, double *acc, double *state) { return pf__engine_rec_get_state_x(e, a, false, acc, state, 0, 0); }
int pf_engine_vdecim_set_state(pf_engine *e, pf_vdecim *a, const double *acc, const double *state, int64_t count) {
   return pf__engine_rec_set_state_x(e, a, false, acc, state, 0, 0, count);
}
int64_t pf_vdecim_count(const pf_vdecim *a) { int64_t c, p; rec_numbers(a, &c, &p); return c; }
int64_t pf_vdecim_pending(const pf_vdecim *a) { int64_t c, p; rec_numbers(a, &c, &p); return p; }
int pf_engine_vdecim_destroy(pf_engine *e, pf_vdecim *a) { return destroy(e, a, pfeng::OBS_VDECIM, "pf_engine_vdecim_destroy"); }

// the wall absorption maps observe no region; the engine's object keeps the count (a priming add accounts nothing)
int pf_engine_absorb_create(pf_engine *e, const double *E, double wall_scale, double abc_scale, double in_scale, int32_t nbin, pf_absorb **out) {
   const char *what = "pf_engine_absorb_create";
   if (!e || !e->impl) return set_err(PF_ERR_ARG, "%s: null engine", what);
   if (!out) return set_err(PF_ERR_ARG, "%s: null out", what);
   *out = nullptr;
   void *impl = nullptr;
   const int rc = e->impl->absorb_create(E, wall_scale, abc_scale, in_scale, nbin, &impl);
   if (rc) return rc;
   pf_absorb *a = new pf_absorb();
   a->eng = e; a->impl = impl; a->nbin = nbin;
   e->observers.push_back(a);
   *out = a;
   return PF_OK;
}
int pf_engine_absorb_add(pf_engine *e, pf_absorb *a, int64_t n, int64_t bin) {
   const int rc = mine(e, a, pfeng::OBS_ABSORB, "pf_engine_absorb_add");
   return rc ? rc : e->impl->absorb_add(a->impl, n, bin);
}
int pf_engine_absorb_get(pf_engine *e, pf_absorb *a, double *nodes, double *mats, double *abc, double *in) {
   const int rc = mine(e, a, pfeng::OBS_ABSORB, "pf_engine_absorb_get");
   return rc ? rc : e->impl->absorb_get(a->impl, nodes, mats, abc, in);
}
int pf_engine_absorb_set(pf_engine *e, pf_absorb *a, const double *nodes, const double *mats, const double *abc, const double *in, int64_t count) {
   const int rc = mine(e, a, pfeng::OBS_ABSORB, "pf_engine_absorb_set");
   return rc ? rc : e->impl->absorb_set(a->impl, nodes, mats, abc, in, count);
}
int64_t pf_absorb_count(const pf_absorb *a) {
   if (!a) return -1;
   if (a->chain) return a->count;
   return a->eng && a->eng->impl ? a->eng->impl->absorb_count(a->impl) : -1;
}
int pf_engine_absorb_destroy(pf_engine *e, pf_absorb *a) { return destroy(e, a, pfeng::OBS_ABSORB, "pf_engine_absorb_destroy"); }

#define PF_NEED(e) if (!(e) || !(e)->impl) return set_err(PF_ERR_ARG, "null engine")

int pf_engine_run(pf_engine *e, int64_t n0, int64_t nsteps) { PF_NEED(e); return e->impl->run(n0, nsteps); }
int pf_engine_step_begin(pf_engine *e, int64_t n) { PF_NEED(e); return e->impl->step_begin(n); }
int pf_engine_halo_ptrs(pf_engine *e, void **send_lo, void **send_hi, void **recv_lo, void **recv_hi, size_t *plane_bytes) {
   PF_NEED(e);
   return e->impl->halo_ptrs(send_lo, send_hi, recv_lo, recv_hi, plane_bytes);
}
int pf_engine_step_end(pf_engine *e, int64_t n) { PF_NEED(e); return e->impl->step_end(n); }
int pf_engine_state_grids(pf_engine *e, void **u_prev, void **u_cur) { PF_NEED(e); return e->impl->state_grids(u_prev, u_cur); }
int pf_engine_layout(pf_engine *e, int64_t *dims, int64_t *pitch, int32_t *exchanged) { PF_NEED(e); return e->impl->layout(dims, pitch, exchanged); }
int pf_engine_set_spares(pf_engine *e, void *g2, void *g3) { PF_NEED(e); return e->impl->set_spares(g2, g3); }
int pf_engine_place_grids(pf_engine *e, void *const *grids, int32_t n, int32_t *idx) { PF_NEED(e); return e->impl->place_grids(grids, n, idx); }
int pf_engine_place_grids5(pf_engine *e, void *const *grids, int32_t n, int32_t *idx) { PF_NEED(e); return e->impl->place_grids5(grids, n, idx); }
void *pf_engine_stream(pf_engine *e, int32_t which) { return (e && e->impl) ? e->impl->stream(which) : nullptr; }
int pf_engine_sync(pf_engine *e) { PF_NEED(e); return e->impl->sync(); }
int pf_engine_flush_outputs(pf_engine *e) { PF_NEED(e); return e->impl->flush(); }
int pf_engine_get_grid(pf_engine *e, int32_t which, void *host) { PF_NEED(e); return e->impl->get_grid(which, host); }
int pf_engine_set_grid(pf_engine *e, int32_t which, const void *host) { PF_NEED(e); return e->impl->set_grid(which, host); }
int64_t pf_region_count(const pf_region *r, int64_t counts[3]) {
   char msg[256];
   const int64_t n = pf_cut::region_counts(r, counts, msg, sizeof msg);
   if (n < 0) set_err(PF_ERR_ARG, "pf_region_count: %s", msg);
   return n;
}
int pf_engine_get_region(pf_engine *e, int32_t which, const pf_region *r, void *host) { PF_NEED(e); return e->impl->get_region(which, r, host, 0); }
int pf_engine_save_state(pf_engine *e, pf_state *st) { PF_NEED(e); return e->impl->save_state(st); }
int pf_engine_load_state(pf_engine *e, const pf_state *st) { PF_NEED(e); return e->impl->load_state(st); }
int pf_engine_timing(pf_engine *e, pf_timing *t, int32_t reset) { PF_NEED(e); return e->impl->timing(t, reset); }
int pf_engine_set_timing(pf_engine *e, int32_t on) { PF_NEED(e); return e->impl->set_timing(on); }
int pf_engine_energy_cfg(pf_engine *e, double h, double c, double Ts, const double *DEF) { PF_NEED(e); if (!DEF) return set_err(PF_ERR_ARG, "null DEF"); return e->impl->energy_cfg(h, c, Ts, DEF); }
int pf_engine_run_energy(pf_engine *e, int64_t n0, int64_t nsteps, double *H_tot, double *E_lost, double *E_in) {
   PF_NEED(e);
   if (!H_tot || !E_lost || !E_in) return set_err(PF_ERR_ARG, "null output array");
   return e->impl->run_energy(n0, nsteps, H_tot, E_lost, E_in);
}

} // extern "C"
