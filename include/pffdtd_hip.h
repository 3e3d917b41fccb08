/*
 * pffdtd_hip.h -- C ABI of the MI355X-native FDTD time-step engine (libpffdtd_hip.so).
 *
 * This is the drop-in boundary for the reference's in-process engine seam
 *
 *     double run_sim(struct SimData *sd);          c_cuda/cpu_engine.h:52, c_cuda/gpu_engine.h:665
 *
 * called from c_cuda/fdtd_main.c:44-53 (load_sim_data -> scale_input -> run_sim ->
 * rescale_output -> write_outputs).  `pf_simdata` is a field-for-field POD mirror of
 * `struct SimData` (c_cuda/fdtd_data.h:38-76); the only additions are `real_bytes`
 * (the reference selects `Real` at compile time with -DPRECISION, c_cuda/fdtd_common.h:44-71;
 * this library carries both precisions and selects at run time) and the widened copies of the
 * `Real` scalars.  Everything is plain pointers and sizes: no C++ or torch types cross this line.
 *
 * All array pointers in pf_simdata are HOST pointers owned by the caller (as in the reference,
 * where load_sim_data mallocs and free_sim_data frees, fdtd_data.h:99,721).  The engine owns
 * only its device state.  Linear indices are in the file layout  ii = ix*Ny*Nz + iy*Nz + iz
 * (cpu_engine.h:180); the engine re-bases them onto its own padded HBM layout internally.
 *
 * Error behaviour: the reference asserts/exits (helper_funcs.h:86-94, gpu_engine.h:192-200);
 * this ABI returns a non-zero pf_status and keeps a message retrievable with pf_last_error().
 */
#ifndef PFFDTD_HIP_H
#define PFFDTD_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_MMB 12 /* max RLC branches per material: MMb, fdtd_data.h:33 */
#define PF_MNM 64 /* max number of materials:      MNm, fdtd_data.h:35 */

/* struct MatQuad (fdtd_data.h:79-84) for Real=float / Real=double */
typedef struct pf_matquad_f32 { float  b, bd, bDh, bFh; } pf_matquad_f32;
typedef struct pf_matquad_f64 { double b, bd, bDh, bFh; } pf_matquad_f64;

/* Mirror of struct SimData (fdtd_data.h:38-76), same field order. */
typedef struct pf_simdata {
   int64_t  *bn_ixyz;     /* [Nb]  boundary node indices */
   int64_t  *bnl_ixyz;    /* [Nbl] lossy boundary node indices */
   int64_t  *bna_ixyz;    /* [Nba] absorbing (ABC) node indices */
   int8_t   *Q_bna;       /* [Nba] 1 face, 2 edge, 3 corner */
   int64_t  *in_ixyz;     /* [Ns]  source nodes */
   int64_t  *out_ixyz;    /* [Nr]  receiver nodes (duplicates allowed) */
   int64_t  *out_reorder; /* [Nr]  row permutation used by write_outputs (fdtd_data.h:941-945) */
   uint16_t *adj_bn;      /* [Nb]  adjacency bits, bit j = neighbour j (fdtd_data.h:532-538) */
   void     *ssaf_bnl;    /* [Nbl] Real: scaled surface-area factors (fdtd_data.h:283-289,608) */
   uint8_t  *bn_mask;     /* [(Npts-1)/8+1] bit ii%8 of byte ii>>3 (fdtd_data.h:567-572); may be NULL:
                             the engine rebuilds its own mask from bn_ixyz (as gpu_engine.h:791 does) */
   int8_t   *mat_bnl;     /* [Nbl] material index of lossy nodes */
   int8_t   *K_bn;        /* [Nb]  popcount(adj_bn); may be NULL (cpu_engine.h:238-240 recomputes it) */
   double   *in_sigs;     /* [Ns*Nt] input signals, row-major (already scaled by scale_input) */
   double   *u_out;       /* [Nr*Nt] receiver outputs, engine row order, written by the engine */
   int64_t   Ns, Nr, Nt, Npts, Nx, Ny, Nz, Nb, Nbl, Nba;
   double    l, l2;
   int8_t    fcc_flag;    /* 0 Cartesian, 1 FCC checkerboard, 2 FCC folded */
   int8_t    NN;          /* 6 | 12 */
   int8_t    Nm;          /* number of materials */
   int8_t   *Mb;          /* [Nm] branches per material */
   void     *mat_quads;   /* [Nm*PF_MMB] pf_matquad_f32 | pf_matquad_f64 */
   void     *mat_beta;    /* [Nm] Real */
   double    infac;       /* input rescaling (scale_input, fdtd_data.h:879-909); not used by the engine */
   double    sl2, lo2, a2, a1; /* the Real-rounded coefficients of fdtd_data.h:186-194, widened exactly */
   int32_t   real_bytes;  /* 4 = float (PRECISION=1), 8 = double (PRECISION=2) */
} pf_simdata;

typedef enum pf_status {
   PF_OK = 0,
   PF_ERR_ARG = 1,      /* bad argument / unsupported configuration */
   PF_ERR_HIP = 2,      /* a HIP runtime call failed */
   PF_ERR_NODEV = 3,    /* no HIP device visible */
   PF_ERR_STATE = 4     /* call sequence violated */
} pf_status;

/* numerics modes */
#define PF_NUM_CPU_EXACT       0 /* operation order and rounding of the reference C CPU engine (cpu_engine.h:174-301,363-405), no
                                    contraction: results are bit-identical to it (the parity target) */
#define PF_NUM_GPU_SAFEGUARDED 2 /* the reference GPU engine's arithmetic for the air and rigid-node updates (fdtd_common.h:44-71,
                                    gpu_engine.h:220-274,288-348): pairwise neighbour sums -- in fp32 rounded TOWARDS ZERO, its
                                    long-run stability safeguard -- then two round-to-nearest FMAs; every kernel family has it: single steps,
                                    7-point blocked pairs with their wall regions, 13-point blocked pairs (round 5) */

typedef struct pf_opts {
   int32_t device;        /* HIP device ordinal */
   int32_t numerics;      /* PF_NUM_* */
   int32_t slab_first;    /* 1 if this grid holds the global ix=0 ghost plane (gpu_engine.h:1030-1032) */
   int32_t slab_last;     /* 1 if this grid holds the global ix=Nx-1 ghost plane (gpu_engine.h:1033-1035) */
   int32_t readout_chunk; /* receiver ring depth in steps before a D2H flush (0 = default) */
   int32_t air_variant;   /* 0 = automatic (measured at creation); 3 = the reference's kernel sequence (flips, air, ABC lists); 4 / 7 =
                             barrier-free marching kernel with virtual ghosts / in-kernel ABC; 25 = lean fused kernel (7-point); 40 =
                             temporally blocked pairs forced (41: their driver only); 42 = 13-point blocked pairs with the shell in bricks
                             (folded FCC, single domain, file order: everything 40 needs, and no source within two cells of the shell);
                             | 256 = separate rigid / branch-ODE kernels */
   int32_t air_chunk;     /* planes marched per workgroup (0 = auto, <0 = that many equal chunks) */
   int32_t timing;        /* 1 = bracket the air kernel with HIP events every step (pf_engine_timing) */
   void   *ext_u0;        /* optional caller-owned DEVICE buffers for the two state grids, each of */
   void   *ext_u1;        /*   pf_grid_bytes() bytes, zero-filled by the caller; NULL = engine allocates */
   int32_t x_global0;     /* global ix of this grid's plane 0 (slabs): only its parity matters, for the FCC
                             checkerboard form (fcc_flag 1) whose existing nodes have even ix+iy+iz */
   int32_t layout;        /* PF_LAYOUT_*: how the engine stores the grid (pf_engine_layout reports it) */
   int32_t energy;        /* 1 = keep what the energy diagnostic needs (explicit Laplacian grid, unfused kernel
                             sequence); then use pf_engine_energy_cfg + pf_engine_run_energy */
   int32_t multi_flags;   /* pf_run_sim_devices / pf_multi_create only: PF_MULTI_* */
   int32_t transport;     /* pf_run_sim_devices / pf_multi_create only: PF_TRANSPORT_* (how ghost planes travel between devices) */
   int32_t verify_exchange; /* same: the first n exchanges are checksummed on both sides (pf_multi_info.exchange_verified) */
   int32_t only_slab;     /* pf_multi_create only: 1 + g = cost model of ONE rank -- the chain is cut as usual but slab g alone is
                             instantiated and receives its own edge planes as ghost planes, through the chosen transport (the
                             physics is wrong, the work and the launches are a rank's); 0 = the whole chain */
   double  wall_scale;    /* pf_multi_create / pf_run_sim_devices: > 0 = cut the chain with the wall planes' weights times this factor (a host that
                             measured it once -- pf_slab_wall_scale -- and wants the same cut in every process); 0 = the compiled-in weights, or the
                             library's own measurement under PF_MULTI_MEASURE_WEIGHTS */
} pf_opts;

#define PF_LAYOUT_AUTO      0 /* decided per scene: rooms whose large surfaces are normal to file z are stored with the file's x and z axes
                               exchanged (single domains: +11-15 % on the two reference rooms; chains: PF_MULTI_CUT_Z) */
#define PF_LAYOUT_EXCHANGED 1 /* always exchanged (a slab of a chain cut along file z: pffdtd_amd/dist.py; no energy diagnostic) */
#define PF_LAYOUT_FILE      2 /* never: the file's own order (x slowest, z unit stride) */

#define PF_TRANSPORT_AUTO 0 /* peer copies where hipDeviceCanAccessPeer says yes for every neighbouring pair, else RCCL, else -- librccl
                               missing, its communicators failing or not returning within PFFDTD_RCCL_INIT_TIMEOUT_S (60) seconds --
                               host-staged copies (pf_multi_info.transport / transport_note say which and why) */
#define PF_TRANSPORT_PEER 1 /* each slab pulls its ghost planes with hipMemcpyPeerAsync on its edge stream (gpu_engine.h:1086-1126
                               uses cudaMemcpyPeerAsync after a full sync); an error without peer access when asked for explicitly */
#define PF_TRANSPORT_RCCL 2 /* ncclSend / ncclRecv of both planes, grouped per slab on its edge stream, one single-process
                               communicator clique over the chain (librccl is loaded at run time); environment PFFDTD_TRANSPORT=
                               peer|rccl|host|auto overrides pf_opts.transport */
#define PF_TRANSPORT_HOST 3 /* the last resort: every slab copies its two edge planes into a pinned bounce buffer on its edge stream and its
                               neighbours copy them out on theirs; the two sides meet on the host (hipEventSynchronize).  Needs nothing
                               from the driver beyond device <-> pinned-host copies.  No counterpart in the reference */

#define PF_MULTI_EVEN_SPLIT  1 /* the reference's Nx/G planes per slab (gpu_engine.h:532-550) instead of the cost-balanced cut */
#define PF_MULTI_ONE_THREAD  2 /* one host thread drives every slab (the reference's arrangement) instead of one thread per slab */
#define PF_MULTI_NO_PAIRS    4 /* never step slabs in temporally blocked pairs */
#define PF_MULTI_FORCE_PAIRS 8 /* ask every slab engine for pairs regardless of its thickness (tests) */
#define PF_MULTI_CUT_Z      16 /* cut the chain along FILE Z instead of x: the slab engines store the grid with the x and z axes
                                  exchanged (pf_engine_layout), what rooms whose large surfaces are normal to z gain 11-15 % from;
                                  chosen automatically for such rooms */
#define PF_MULTI_CUT_X      32 /* never (the reference's arrangement, gpu_engine.h:516-662) */
#define PF_MULTI_MEASURE_WEIGHTS 128 /* measure the wall planes' weights on the scene when the chain is created (pf_slab_wall_scale) instead of
                                  cutting with the compiled-in ones (23 / 5 interior planes per full plane of lossy / rigid nodes).  Opt-in:
                                  on MI355X the measurement reproduces the compiled-in figures where it is clean (factors 0.99-1.05,
                                  profiles/r05_partition_weights.txt) and its own noise -- two engines of one geometry differ by 2-3 %
                                  with the luck of their grid placement -- is larger than their error */
#define PF_MULTI_NO_TRIPLES 64 /* slabs step in pairs at most (round 5: by default a slab whose wall regions fit steps THREE steps per
                                  pass across three split-phase steps, pf_engine_place_grids5) */

typedef struct pf_timing {
   double  air_ms_total;    /* sum of HIP-event durations of the air kernel launches */
   int64_t air_launches;
   double  step_ms_total;   /* sum of HIP-event durations of whole steps (pre .. readout) */
   int64_t steps;
   double  tb2_ms_total;    /* temporal blocking: sum of the two-steps-per-pass kernel's launch durations (included in air_ms_total) */
   int64_t tb2_launches;    /* kernel launches behind tb2_ms_total; 0 when the engine steps one step per pass */
   int64_t tb2_cells;       /* cells one such launch advances by two steps (average over the x ranges of the box) */
   double  tune_ms[3];      /* creation-time measurement of the interior update of one step, ms: lean fused kernel,
                               barrier-free kernel, temporally blocked pair / 2 (0 = not measured) */
   int64_t air_path;        /* what the engine runs: 0 lean, 1 barrier-free (virtual ghosts), 2 blocked pairs, -1 other */
   int64_t tb2_lw;          /* blocked pairs: lanes per row segment of the two-steps-per-pass kernel (64 | 32 | 16), else 0 */
   int64_t tb2_dirty_tiles; /* blocked pairs: tiles of the box that step singly (geometry or a source inside) */
   int64_t place_candidates;/* blocked pairs: grid placements timed at creation (0: none), and the two-steps-per-pass kernel's */
   double  place_ms[3];     /*   ms per launch on the first (as allocated), the chosen (fastest) and the slowest of them */
   int64_t wall_blocks[2];  /* blocked pairs with the shell in pairs too (wall regions, pf_wall.h): blocks of the launches whose pencils
                               are all alike / generic blocks (edges, corners); 0, 0: the shell takes single steps */
   int64_t tb_steps_per_pass; /* steps one launch behind tb2_ms_total advances its cells by: 2 (pairs), 3 (k_tb3, pf_tb3.h), 0: none */
   int64_t wall_bricks;     /* wall regions: bricks of the frame (edges and corners of the shell, stepped in LDS: pf_brick.h); 0: generic blocks */
   int64_t wall_three_steps;/* triples: which wall regions take all three steps in ONE pass (k_wall2<..., NS = 3>): bit 0 the x / y regions, bit 3 the
                               column strips; 0: two steps + one.  Slabs of a chain: bits 4 / 5 -- the slab's low / high x side is the grid's own wall
                               and a region's and the bricks' too (no single steps of its planes) */
   int64_t wall_profile;    /* of the regions in wall_three_steps, which run with the node layout of a plain box wall compiled in (pf_wall.h: wall profiles):
                               bit 0 the x / y regions, bit 3 the column strips; 0: the node words are read from the blocks */
   int64_t wall_uniform_branches; /* of the regions in wall_profile with a frequency-dependent node layer: the branch count their kernels evaluate for every
                               node alike, without a per-node guard (every material of the scene has that many branches: 1 .. 4, 11 or 12);
                               0: the guarded form ran (mixed counts, other counts) or no such region */
   int64_t wall_unread_skipped; /* triples: wall regions (bits as in wall_three_steps) that do not store u^{n+1} of their cells because nothing reads it:
                               no receiver in their cells, no tile or node that steps singly */
   int64_t wall_strips_staged; /* triples: 1 = the column strips' three-step kernel moves its planes through LDS, so that memory sees whole rows
                               (pf_strip_map.h: the bodies with a uniform branch count); 0: every lane loads and stores its own pencil, or no such strips */
   int64_t fcc_shell_bricks;/* air_variant 42: bricks this engine launches per pair (the whole 13-point shell, pf_brick_fcc.h); 0 otherwise */
} pf_timing;

typedef struct pf_engine pf_engine;

/* ---- library-level ---- */
const char *pf_last_error(void);
const char *pf_version(void);
int         pf_device_count(void);
/* bytes of one state grid in the engine's padded HBM layout, and its z pitch in elements */
size_t      pf_grid_bytes(int64_t Nx, int64_t Ny, int64_t Nz, int32_t real_bytes);
int64_t     pf_grid_pitch(int64_t Nz, int32_t real_bytes);
void        pf_opts_default(pf_opts *o);

/* ---- the reference seam: double run_sim(struct SimData*) ---- */
/* Runs all sd->Nt steps, fills sd->u_out (engine row order), returns elapsed seconds (<0 on error; pf_last_error()).
 * Like the reference's GPU engine (gpu_engine.h:680-682) it spreads the grid over EVERY visible device as a chain of
 * Z-slabs along Nx (environment: PFFDTD_NGPUS=n limits it to the first n devices, PFFDTD_DEVICES=0,1,... names the chain). */
double      pf_run_sim(pf_simdata *sd);
/* The same on an explicit chain: slab g on device devices[g]; an id may repeat ("virtual slabs": the whole multi-device
 * code path on one GPU).  One host thread per slab, split-phase steps, ghost planes pulled from the neighbours with
 * peer copies on the edge stream while the interior planes run (replaces gpu_engine.h:516-662,739-823,993-1145).
 * base: options common to all slabs (numerics, air_variant, readout_chunk, multi_flags, transport, ...); NULL = defaults. */
double      pf_run_sim_devices(pf_simdata *sd, int32_t nslabs, const int32_t *devices, const pf_opts *base);
/* The owned plane ranges such a run uses when cut along x: cuts[0..nslabs], slab g owns global planes [cuts[g], cuts[g+1]).
 * pf_slab_partition: with the compiled-in wall-plane weights; _w: those weights times wall_scale. */
int         pf_slab_partition(const pf_simdata *sd, int32_t nslabs, int32_t even_split, int64_t *cuts);
int         pf_slab_partition_w(const pf_simdata *sd, int32_t nslabs, int32_t even_split, double wall_scale, int64_t *cuts);
/* ... and the cut along FILE Z (along_z = 1: what a chain of slabs stored with exchanged axes uses, PF_MULTI_CUT_Z) -- the ONE implementation of
 * the cut: pffdtd_amd/slab.py (one process per GPU under torch.distributed) calls this too.  No device needed. */
int         pf_slab_partition_axis(const pf_simdata *sd, int32_t nslabs, int32_t even_split, double wall_scale, int32_t along_z, int64_t *cuts);
/* Measures that factor for this scene on `device` (round 5): three short one-rank cost models -- an interior rank with Nx / nslabs planes,
 * one with a few planes more, the first rank with its x wall -- give the cost of an interior plane and of the wall; the ratio to what
 * the compiled-in weights predict is returned (<= 0: not measured -- scene too small, fewer than 63 steps --: use 1).  pf_multi_create
 * does this by itself under PF_MULTI_MEASURE_WEIGHTS; hosts with one process per device measure on rank 0 and hand the factor to every
 * rank (pf_opts.wall_scale). */
double      pf_slab_wall_scale(pf_simdata *sd, int32_t nslabs, int32_t device, const pf_opts *base);

/* ---- the same chain as an object (what pf_run_sim_devices does inside): lets a host warm up, time and inspect a
 * multi-device run -- bench.py --gpus N drives this from one plain process, as the reference drives all its GPUs from one
 * (gpu_engine.h:680-682, 993-1145).  One persistent host thread per slab.  sd must outlive the object; receivers land in
 * sd->u_out after every pf_multi_run. */
typedef struct pf_multi pf_multi;
typedef struct pf_multi_info {
   int32_t nslabs;
   int32_t transport;          /* PF_TRANSPORT_PEER | PF_TRANSPORT_RCCL (0: a single slab, nothing travels) */
   int32_t rccl_self;          /* 1: RCCL with one 1-rank communicator per slab (all slabs on one device: tests) */
   int32_t exchange_verified;  /* 1: every checked exchange delivered the senders' planes bit for bit; 0: one did not; -1: none checked */
   int64_t exchanges_checked;  /* exchanges (steps) checksummed so far */
   int32_t exchange_nonzero;   /* 1: at least one checked ghost plane was not all zeros (the check was not vacuous) */
   int32_t cut_along_z;        /* 1: the chain is cut along FILE Z (PF_MULTI_CUT_Z or chosen for the scene); pf_multi_get_slab's ranges are then z ranges */
   int64_t plane_bytes;        /* bytes of one exchanged plane */
   double  last_run_seconds;   /* wall time of the last pf_multi_run */
   char    transport_name[64];
   char    transport_note[256]; /* why this transport: the fallbacks PF_TRANSPORT_AUTO took ("" = its first choice) */
   double  wall_scale;         /* the factor on the wall planes' weights the chain was cut with (1: the compiled-in weights) */
   int32_t wall_measured;      /* 1: that factor was measured at creation (pf_slab_wall_scale) */
} pf_multi_info;
int  pf_multi_create(pf_simdata *sd, int32_t nslabs, const int32_t *devices, const pf_opts *base, pf_multi **out);
/* steps n0 .. n0+nsteps-1 on every slab; returns when all streams have drained and the receiver rows are in sd->u_out.
 * A slab whose host thread does not reach a step barrier within PFFDTD_BARRIER_TIMEOUT_S seconds (a stuck device, a collective that never
 * completes) turns the call into PF_ERR_HIP, pf_last_error() = "slab chain hung ...".  After THAT error the object is beyond repair: the
 * stuck thread may still be inside a driver / RCCL call and cannot be joined, so pf_multi_destroy only detaches the threads and frees
 * nothing -- device grids, pinned buffers and communicators of every slab stay allocated until the process ends.  A host that catches
 * the error should report it and EXIT; retrying in the same process can run out of device memory. */
int  pf_multi_run(pf_multi *m, int64_t n0, int64_t nsteps);
int  pf_multi_get_info(pf_multi *m, pf_multi_info *info);
/* slab g: owned global planes [x0, x1), device, whether it steps in temporally blocked pairs (1) or triples (3), and its engine (for
 * pf_engine_state_grids / pf_engine_timing between runs; do not step it directly) */
int  pf_multi_get_slab(pf_multi *m, int32_t g, int64_t *x0, int64_t *x1, int32_t *device, int32_t *paired, pf_engine **engine);
void pf_multi_destroy(pf_multi *m);

/* ---- one process per device: the plane exchange of a slab engine by native RCCL (replaces cudaMemcpyPeerAsync of gpu_engine.h:1086-1126
 * for a host whose ranks are PROCESSES, e.g. under torch.distributed.run; the chain object above is the one-process form).  Rank 0 obtains
 * the 128-byte id and hands it to every rank by any channel; all ranks then create their communicator together (returns PF_ERR_HIP with
 * pf_last_error() if the rendezvous fails or does not complete within PFFDTD_RCCL_INIT_TIMEOUT_S seconds: fall back to the host's own p2p).
 * pf_rccl_exchange goes between pf_engine_step_begin and pf_engine_step_end: first / last updated plane to rank peer_lo / peer_hi, theirs
 * into the ghost planes (peer < 0: no neighbour there), one ncclGroup on the engine's edge stream; asynchronous. */
typedef struct pf_rccl_comm pf_rccl_comm;
int  pf_rccl_unique_id(void *id128);
int  pf_rccl_comm_create(const void *id128, int32_t nranks, int32_t rank, int32_t device, pf_rccl_comm **out);
int  pf_rccl_exchange(pf_rccl_comm *c, pf_engine *e, int32_t peer_lo, int32_t peer_hi);
void pf_rccl_comm_destroy(pf_rccl_comm *c);

/* ---- engine object (what run_sim does inside, exposed for the Python host, slabs and tests) ---- */
int  pf_engine_create(const pf_simdata *sd, const pf_opts *opts, pf_engine **out);
void pf_engine_destroy(pf_engine *e);
/* steps n0 .. n0+nsteps-1 with no halo exchange (single slab); receivers land in sd->u_out[r*Nt+n] */
int  pf_engine_run(pf_engine *e, int64_t n0, int64_t nsteps);
/* split-phase step for Z-slab runs (gpu_engine.h:993-1145 re-thought): begin enqueues the edge planes +
 * all boundary-node work on the edge stream and the interior planes on the main stream; the caller then
 * exchanges the planes returned by pf_engine_halo_ptrs() (ordered after the edge stream), and end joins
 * the streams and rotates the state pointers. */
int  pf_engine_step_begin(pf_engine *e, int64_t n);
int  pf_engine_halo_ptrs(pf_engine *e, void **send_lo, void **send_hi, void **recv_lo, void **recv_hi,
                         size_t *plane_bytes);
int  pf_engine_step_end(pf_engine *e, int64_t n);
/* Slab engines created on caller-owned grids (pf_opts.ext_u0/ext_u1): hand over two more grids of the same size, so
 * that the engine may advance in temporally blocked pairs (two split-phase steps per pair, the state then cycles
 * through the four grids: pf_engine_halo_ptrs always names the grid being written).  Returns 0 when pairs are on,
 * 1 when this engine keeps stepping singly (scene without a boundary-free box, small y-z cross-section, 13-point,
 * single-domain engine, ...); other values
 * are pf_status errors.  No counterpart in the reference. */
int  pf_engine_set_spares(pf_engine *e, void *grid2, void *grid3);
/* The same with a choice: before its first step a slab engine is offered a pool of n >= 4 zero-filled caller-owned grids
 * (pool[0], pool[1] may be the ext_u0 / ext_u1 it was created on).  The speed of the two-steps-per-pass kernel depends on
 * where its four grids lie relative to each other in physical memory ("grid placement"), so the engine times
 * assignments of pool members to its four roles and adopts the fastest: idx[0], idx[1] = the state grids from now on,
 * idx[2], idx[3] = the spares; the caller may free the others.  An engine that keeps stepping singly (cf.
 * pf_engine_set_spares) picks the pair of the pool its single step is fastest on and says idx = i, j, -1, -1.  Returns a pf_status.
 * THE OFFERED GRIDS MUST BE ALL ZEROS AND ARE ZEROED AGAIN: the search runs real step kernels on them.  Initialise the field
 * (pf_engine_set_grid, device writes) only afterwards; after pf_engine_set_grid the call is refused with PF_ERR_STATE.
 * No counterpart in the reference. */
int  pf_engine_place_grids(pf_engine *e, void *const *pool, int32_t n, int32_t idx[4]);
/* The same with room for TRIPLES (round 5): a slab engine offered n >= 5 grids whose wall regions fit steps three steps per pass
 * across three split-phase steps (k_tb3, pf_tb3.h): idx[0], idx[1] = the state grids, idx[2], idx[3] = the two grids its blocked
 * kernel writes, idx[4] = the grid that holds u^{n+1} where somebody needs it in memory.  idx[4] = -1: pairs (idx[2], idx[3] the
 * spares) or single steps (idx[2] = idx[3] = -1), exactly as pf_engine_place_grids reports them.  No counterpart in the reference. */
int  pf_engine_place_grids5(pf_engine *e, void *const *pool, int32_t n, int32_t idx[5]);
/* Device pointers of the two state grids as they stand between runs (u_prev = u^{n-1}, overwritten by the next step;
 * u_cur = u^n), each pf_grid_bytes() long: the engine's own allocations unless pf_opts.ext_u0 / ext_u1 were given.
 * Lets a host that left the allocation to the engine (which then also chooses WHERE the grids live, see DESIGN.md
 * "placement") initialise or inspect the field on the device.  No counterpart in the reference. */
int  pf_engine_state_grids(pf_engine *e, void **u_prev, void **u_cur);
/* How those grids are laid out: dims[0..2] = planes, rows, columns as STORED, pitch = elements per row (a grid holds
 * dims[0] * dims[1] * pitch elements), exchanged = 1 when the engine stores the file's x and z axes exchanged (unit stride along
 * file x; only engines that own their grids may choose to, see DESIGN.md 5: rooms whose large surfaces are normal to file z).
 * pf_engine_get_grid / _set_grid and every index in pf_simdata stay in file order whatever the storage. */
int  pf_engine_layout(pf_engine *e, int64_t *dims, int64_t *pitch, int32_t *exchanged);
void *pf_engine_stream(pf_engine *e, int32_t which); /* 0 main, 1 edge: hipStream_t */
int  pf_engine_sync(pf_engine *e);
int  pf_engine_flush_outputs(pf_engine *e);          /* ring -> sd->u_out */
/* copy a state grid to/from a host array in FILE layout [Nx*Ny*Nz] Real; which: 0 = u0, 1 = u1.
 * pf_engine_set_grid: the field must be FINITE everywhere, the cells inside the walls included.  In the CPU-exact arithmetic the
 * boundary pass does not fetch a neighbour whose adjacency bit is clear (a cell inside the wall): the reference adds (a2 * 0) * u1
 * there, which is +-0 for a finite u1 and leaves the sum as it is (the sums of the time loop never hold -0), but NaN for an Inf
 * or NaN -- the internal switch PF_DBG_BND_FETCH_ALL (csrc/pf_debug.h) fetches every neighbour, the exact reference behaviour for such fields too. */
int  pf_engine_get_grid(pf_engine *e, int32_t which, void *host);
int  pf_engine_set_grid(pf_engine *e, int32_t which, const void *host);
/* ---- checkpoint and resume: the whole state between two steps n-1 | n, in its canonical form ----
 * Exactly what the reference's run_sim carries across its loop, in the FILE's terms -- independent of how an engine stores it (kernel family,
 * storage layout, one domain or a chain of slabs): a state saved by one of them loads into any other of the same scene and precision and
 * continues bit for bit.  No counterpart in the reference (its run_steps is re-entrant in memory only).
 *   - The step index is the caller's: after a load it continues with pf_engine_run(e, n, ...) / pf_multi_run(m, n, ...).  Receiver rows of the
 *     steps < n are the caller's as well (sd->u_out); both calls flush the receiver ring into sd->u_out first.
 *   - Valid between runs only: PF_ERR_STATE inside a split-phase step or pass (between pf_engine_step_begin and the pf_engine_step_end that ends
 *     a slab's pair or triple), and for an engine created with pf_opts.energy (its sums live with the caller).  PF_ERR_ARG for a null pointer;
 *     with Nbl == 0 the four node arrays may be NULL.
 *   - A load is allowed at any time between runs, also into an engine that has stepped already (a rewind).  Afterwards nothing of what went
 *     before is read again: the engine behaves as a new engine that holds this state.
 *   - Branch slots m >= Mb[mat] are written as 0 by a save and ignored by a load.
 *   - A save materialises the ghost cells of u_cur as pf_engine_get_grid(1) does.  A load into a whole domain does not depend on the ghost cells
 *     or the folded row of either field (the engines re-derive them every step); the edge planes of an interior slab of a chain are real data,
 *     which pf_multi_load_state fills from the global arrays.
 *   - u1b / u2b are the node values the reference carries from step to step (cpu_engine.h:322-325), saved and restored as they are, not
 *     gathered from the fields: in the first two steps after pf_engine_set_grid they differ from them (the reference starts them at zero).
 *   - Device memory: the fields move through a staging buffer of a fixed number of planes where the engine stores the axes exchanged, and by
 *     pitched copies otherwise -- never through a second grid; the node arrays through a device copy of their own size for the call's duration. */
typedef struct pf_state {      /* all HOST pointers, caller-owned; Real = float | double by pf_simdata.real_bytes */
   void *u_prev, *u_cur;       /* [Npts]  u^{n-1}, u^n in FILE order (ix*Ny*Nz + iy*Nz + iz), as pf_engine_get_grid(0 / 1) */
   void *u1b, *u2b;            /* [Nbl]   node values of the last two steps, in the order of sd->bnl_ixyz (cpu_engine.h:322-325) */
   void *vh1, *gh1;            /* [Nbl * PF_MMB]  branch state, [nb * PF_MMB + m] as cpu_engine.h:363-402 */
} pf_state;
int  pf_engine_save_state(pf_engine *e, pf_state *st);
int  pf_engine_load_state(pf_engine *e, const pf_state *st);
/* The same for a chain: the global arrays of the WHOLE scene (the sd given to pf_multi_create).  Every slab saves / loads its part on its own
 * device and host thread; a load leaves the chain ready for pf_multi_run(m, n, ...), and the exchange self-check (pf_opts.verify_exchange)
 * covers the first exchanges after it again.  PF_ERR_STATE for a one-rank cost model (pf_opts.only_slab). */
int  pf_multi_save_state(pf_multi *m, pf_state *st);
int  pf_multi_load_state(pf_multi *m, const pf_state *st);
/* ---- field regions: a plane or a box of the field during a run, without copying the grid ----
 * The data behind the reference's plots (python/fdtd/sim_fdtd.py: gather_slice), which pf_engine_get_grid serves only by a copy of the whole grid.
 * A region is a strided box in FILE coordinates x, y, z: the cells lo[a] + k * stride[a] < hi[a].  `host` receives counts[0] * counts[1] * counts[2]
 * Reals, dense, z fastest: ((i * counts[1] + j) * counts[2] + k).  which: 0 = u^{n-1}, 1 = u^n, as pf_engine_get_grid.
 *   - Every cell -- ghost cells and the folded row included -- holds bit for bit what pf_engine_get_grid(which) gives for it; for a chain, what
 *     pf_multi_save_state writes into u_prev / u_cur.  The ghost shell of u^n is materialised (as pf_engine_get_grid(1) does) only when the region
 *     holds a cell of a face of the grid.
 *   - PF_ERR_ARG, with a message that names the field, for a null pointer, which outside 0 / 1, lo < 0, hi > N, lo >= hi, stride < 1.
 *   - PF_ERR_STATE inside a split-phase step, inside a slab's pair or triple (u^{n+1} is not complete in memory there: a chain whose slabs step in
 *     passes answers it at the steps in between, the caller advances a step and asks again) and for a one-rank cost model (pf_opts.only_slab).
 *     A refusal leaves the engine or chain as it was.
 *   - Works on an engine created with pf_opts.energy.  The receiver ring is not flushed, and nothing a later step reads changes.
 *   - Device memory: ONE staging buffer for the call's duration, no larger than min(the region's bytes, 32 MiB) (csrc/pf_state.h:
 *     PF_REGION_STAGE_BYTES); larger regions move in pieces along their slowest axis -- or, where they are evenly pitched rows of file-order storage
 *     (unit strides, whole columns of y), by one pitched copy without any buffer, as pf_engine_get_grid.  Never a second grid, whatever the layout.
 *   - A chain cuts the region to its slabs (csrc/pf_region_cut.h): every slab copies the part it owns on its own device and host thread into that
 *     part's cells of `host`; a slab the region misses does nothing.
 * pf_region_count: counts[a] = ceil((hi[a] - lo[a]) / stride[a]) (counts may be NULL); returns their product, or < 0 for a region that is not
 * well-formed (pf_last_error says why; hi <= N is the engine's to check).  No counterpart in the reference. */
typedef struct pf_region { int64_t lo[3], hi[3], stride[3]; } pf_region;
int64_t pf_region_count(const pf_region *r, int64_t counts[3]);
int  pf_engine_get_region(pf_engine *e, int32_t which, const pf_region *r, void *host);
int  pf_multi_get_region(pf_multi *m, int32_t which, const pf_region *r, void *host);
/* ---- field accumulators: running sums of a region over the time steps, kept on the device ----
 * What frames cannot give: EVERY step of every cell of a region (a 1024^2 plane over 76 460 steps is 320 GB through the host).  An accumulator
 * belongs to one engine (or chain) and holds, for a region and nchan real channels,
 *        acc[m][cell] += w[m] * (double)u^n[cell]          at every pf_engine_accum_add, in double, on the device
 * -- with w = g(n) cos(2 pi f n Ts), -g(n) sin(2 pi f n Ts) a running DFT of every cell (pffdtd_amd/spectra.py).  16 bytes per cell and channel,
 * whatever the run's length.  No counterpart in the reference.
 *   - The sample is u^n, the field the receivers of step n sample: cell for cell -- ghost cells and the folded row included -- what
 *     pf_engine_get_region(1, ...) gives at the same moment, and the virtual ghost shell is materialised exactly when that call would.  Nothing a
 *     later step reads changes; the receiver ring is not flushed.
 *   - Arithmetic: one multiplication rounded to double, one addition rounded to double per sample and channel, in the order of the calls (no fused
 *     multiply-add): numpy's acc += w * u.astype(float64) gives the same bits.  fp32 denormals of the field are kept.
 *   - depth (1 .. 16, 0 = the default the measurements of profiles/field_spectra.txt chose): so many samples wait in a ring on the device and are
 *     folded into the sums together, which moves 16 * nchan / depth + 2 * sizeof(Real) bytes per sample and cell instead of 16 * nchan +
 *     sizeof(Real).  The order of the additions is the same: the depth never changes a bit of a sum.
 *   - get folds what is pending and copies the sums out, [nchan][cells] doubles, the cells dense in the region's order (z fastest, as
 *     pf_engine_get_region); it resets nothing.  set drops what is pending and replaces the sums (host NULL: zeros) and the count: how a resumed
 *     run continues.  pf_accum_count: the samples added so far, or the count given to set.
 *   - add, get and set are valid between runs only: PF_ERR_STATE under the conditions of pf_engine_get_region.  An engine created with pf_opts.energy
 *     answers.  PF_ERR_ARG, with a message that names the field, for a null pointer, nchan outside 1 .. 256, depth outside 0 .. 16, a region
 *     pf_engine_get_region would refuse, a negative count, and a handle that belongs to another engine or chain.
 *   - Several accumulators per engine are allowed; pf_engine_destroy / pf_multi_destroy free those left (their handles are dead afterwards).
 *   - Device memory, all of it the engine's: nchan * cells doubles (rows padded to an even cell count), depth * cells Reals, depth * nchan doubles.
 *   - A chain gives every slab that owns cells of the region an accumulator over its part (csrc/pf_region_cut.h); add runs on every slab's own
 *     device and host thread.  add is all or nothing: where any slab is inside a pair or a triple no slab's sums or count change, the call
 *     returns PF_ERR_STATE and the chain stays usable -- a chain meant to be sampled at given steps is created with
 *     PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES.  PF_ERR_STATE for a one-rank cost model (pf_opts.only_slab). */
typedef struct pf_accum pf_accum;
int     pf_engine_accum_create (pf_engine *e, const pf_region *r, int32_t nchan, int32_t depth, pf_accum **out);
int     pf_engine_accum_add    (pf_engine *e, pf_accum *a, const double *w);          /* w[nchan] */
int     pf_engine_accum_get    (pf_engine *e, pf_accum *a, double *host);             /* host[nchan][cells] */
int     pf_engine_accum_set    (pf_engine *e, pf_accum *a, const double *host, int64_t count);
int64_t pf_accum_count         (const pf_accum *a);
int     pf_engine_accum_destroy(pf_engine *e, pf_accum *a);
int     pf_multi_accum_create  (pf_multi *m, const pf_region *r, int32_t nchan, int32_t depth, pf_accum **out);
int     pf_multi_accum_add     (pf_multi *m, pf_accum *a, const double *w);
int     pf_multi_accum_get     (pf_multi *m, pf_accum *a, double *host);
int     pf_multi_accum_set     (pf_multi *m, pf_accum *a, const double *host, int64_t count);
int     pf_multi_accum_destroy (pf_multi *m, pf_accum *a);
/* ---- band accumulators: per cell, the sample filtered by second-order sections, squared, summed into time bins -- on the device ----
 * What an energy decay per octave band needs of every cell of an audience plane (EDT, T20 / T30, C50 / C80, D50, strength: pffdtd_amd/decay.py),
 * and what the linear sums above cannot give.  A band accumulator belongs to one engine (or chain) and holds a region, npre shared sections,
 * nband bands of nsec sections each, nbin time bins and a ring of `depth` samples.  No counterpart in the reference.
 *   - A section is five doubles b0 b1 b2 a1 a2 (a0 = 1; scipy's sos rows without their fourth column) with state s1, s2 per cell, transposed
 *     direct form II, every operation rounded to double once, no fused multiply-add, in exactly this association:
 *            y  = b0*x + s1;     s1 = (b1*x - a1*y) + s2;     s2 = b2*x - a2*y
 *     pre_sos[npre][5], band_sos[nband][nsec][5].  npre = nsec = 0: plain squares.
 *   - pf_engine_bandacc_add(a, bin) takes u^n of the region exactly as pf_engine_accum_add does (the same cells, the same ghost-shell rule) and per
 *     cell: x = (double)u through the shared sections in order; per band b, y = x through that band's sections; bin >= 0: E[b][bin] = E[b][bin] + y*y
 *     (one multiplication, one addition); bin == -1: the filters run, nothing is summed.  Samples are applied in the order of the calls: the depth
 *     (1 .. 16, 0 = the default) never changes a bit, and a numpy loop over time written with the three lines above gives the same bits.
 *   - get folds what is pending and copies sums[nband][nbin][cells] and state[npre + nband*nsec][2][cells] out (s1, s2; the shared sections first,
 *     then band 0's, ...), the cells dense in the region's order, z fastest; state may be NULL; nothing is reset.  set drops what is pending and
 *     replaces sums, state (NULL: zeros) and the count: how a resumed run continues.  pf_bandacc_count: the samples added, or the count given to set.
 *   - PF_ERR_STATE as pf_engine_accum_*.  PF_ERR_ARG, with a message that names the field, for a null pointer, nband outside 1 .. 16, npre or nsec
 *     outside 0 .. 8, nbin < 1, depth outside 0 .. 16, a coefficient that is not finite, a region pf_engine_get_region would refuse, bin outside
 *     -1 .. nbin-1, a negative count, and a handle that belongs to another engine or chain.  An engine created with pf_opts.energy answers.
 *   - Several per engine are allowed; pf_engine_destroy / pf_multi_destroy free those left.
 *   - Device memory, all of it the engine's: E nband*nbin rows and state (npre + nband*nsec)*2 rows of doubles (rows padded to an even cell
 *     count), depth * cells Reals, and -- npre > 0 -- depth rows of doubles for the samples after the shared sections.
 *   - A chain: as the field accumulators, one per slab over its part; add is all or nothing. */
typedef struct pf_bandacc pf_bandacc;
int     pf_engine_bandacc_create (pf_engine *e, const pf_region *r, int32_t npre, const double *pre_sos, int32_t nband, int32_t nsec, const double *band_sos,
                                  int64_t nbin, int32_t depth, pf_bandacc **out);
int     pf_engine_bandacc_add    (pf_engine *e, pf_bandacc *a, int64_t bin);
int     pf_engine_bandacc_get    (pf_engine *e, pf_bandacc *a, double *sums, double *state);
int     pf_engine_bandacc_set    (pf_engine *e, pf_bandacc *a, const double *sums, const double *state, int64_t count);
int64_t pf_bandacc_count         (const pf_bandacc *a);
int     pf_engine_bandacc_destroy(pf_engine *e, pf_bandacc *a);
int     pf_multi_bandacc_create  (pf_multi *m, const pf_region *r, int32_t npre, const double *pre_sos, int32_t nband, int32_t nsec, const double *band_sos,
                                  int64_t nbin, int32_t depth, pf_bandacc **out);
int     pf_multi_bandacc_add     (pf_multi *m, pf_bandacc *a, int64_t bin);
int     pf_multi_bandacc_get     (pf_multi *m, pf_bandacc *a, double *sums, double *state);
int     pf_multi_bandacc_set     (pf_multi *m, pf_bandacc *a, const double *sums, const double *state, int64_t count);
int     pf_multi_bandacc_destroy (pf_multi *m, pf_bandacc *a);
/* ---- vector band accumulators: per cell, up to four COMPONENTS of the field filtered, PRODUCTS of two of them summed into time bins -- on the device ----
 * What a quantity that needs the field's direction asks of every cell of an audience plane: the lateral energy fraction LF / LFC of ISO 3382-1 and
 * the sound intensity per band and time bin (pffdtd_amd/directional.py).  A pf_bandacc squares one input; two of them cannot be multiplied after the
 * fact, because the product is formed per sample.  A vector band accumulator belongs to one engine (or chain) and holds a region, ncomp components,
 * npre sections PER COMPONENT, nband bands of nsec sections each (coefficients shared by the components, state per component), nprod products, nbin
 * time bins and a ring of `depth` samples.  No counterpart in the reference.
 *   - comp[ncomp], ncomp 1 .. 4, no value twice.  Component 0 is the cell itself: exactly what pf_engine_bandacc_add samples.  Component a = 1, 2, 3 is
 *     the central difference along FILE x, y, z:   d_a(c) = u^n[c + e_a] - u^n[c - e_a],   ONE subtraction in the field's own precision, rounded once
 *     (numpy: u[hi] - u[lo] in the field's dtype), each operand bit for bit the cell pf_engine_get_region(1, ...) gives for it.  The difference is
 *     kept in the field's precision until the filters widen it.
 *   - A region with a difference component along axis a keeps one cell clear of both faces along a: lo[a] >= 1 and its last cell <= N[a] - 2;
 *     otherwise PF_ERR_ARG names the axis.  The virtual ghost shell is materialised when the region, WIDENED by one cell along its difference axes,
 *     holds a face cell: the pf_engine_get_region rule applied to the cells actually read.
 *   - Components 1 / 2 / 3 are refused by name on fcc_flag != 0: an axis neighbour at +-1 is no node of the checkerboard.  comp = {0} alone works on
 *     every grid.
 *   - Components 4, 5, 6 are the LATTICE DIFFERENCE along FILE x, y, z, on fcc_flag 1 and 2 only (refused by name, comp[k], on fcc_flag == 0).  Eight
 *     of a node's twelve neighbours sit at +-1 along any axis, in four opposite pairs; with the + offsets o0 .. o3, in the order of the 12-point
 *     stencil (synth.FCC_OFFS),
 *         4 (x): (+1,+1,0) (+1,0,+1) (+1,-1,0) (+1,0,-1)     5 (y): (+1,+1,0) (0,+1,+1) (-1,+1,0) (0,+1,-1)     6 (z): (0,+1,+1) (+1,0,+1) (0,-1,+1) (-1,0,+1)
 *         L_a(c) = ((u[c+o0] - u[c-o0]) + (u[c+o1] - u[c-o1])) + ((u[c+o2] - u[c-o2]) + (u[c+o3] - u[c-o3]))          = 8 h du/da + O(h^3)
 *     seven operations in the field's own precision, each rounded once, in exactly this association, no contraction.  Every operand is bit for bit
 *     the cell pf_engine_get_region(1, ...) gives right after the add, in STORED coordinates: on a folded grid (fcc_flag 2) folded ones, the fold row
 *     Ny - 1 holding the copy of row Ny - 2 -- an add whose cells read that row writes it first, from the row of u^n the next step copies again (an
 *     engine whose shell lives in memory otherwise still carries the row of two steps ago there; nothing a later step reads changes).  No parity
 *     logic runs on the device: a hole of a flag-1 grid is computed like any cell, from holes.  On a folded grid the stored +y of a cell with odd
 *     ix + iy + iz is the room's -y (pffdtd_amd/directional.py: fold_coordinates).  The value stays Real until the filters widen it.
 *   - A region with any lattice component keeps one cell clear of ALL SIX faces (every L_a reads neighbours along all three axes); otherwise
 *     PF_ERR_ARG names the first offending axis.  The ghost shell is materialised when the region widened by one cell on every axis holds a face cell.
 *   - pre_sos[ncomp][npre][5] (npre 0 .. 8; a shorter cascade is padded with 1 0 0 0 0), band_sos[nband][nsec][5]; a section and its three lines
 *     exactly as pf_bandacc above: the same association, every operation rounded to double once, no fused multiply-add.  Per component k,
 *     x_k = (double)component runs through pre_sos[k] in order; for every band b, y_k = x_k runs through band_sos[b] with component k's own state.
 *   - prod[nprod][3], nprod 1 .. 10, rows (i, j, mode) with i, j < ncomp.  bin >= 0, mode 0: S[p][b][bin] = S[p][b][bin] + y_i * y_j (one
 *     multiplication, one addition); mode 1: S[p][b][bin] + fabs(y_i * y_j).  bin == -1: the filters run, nothing is summed.  Samples are applied in
 *     the order of the calls: the depth (1 .. 8, 0 = the default) never changes a bit, and a numpy loop over time written with those lines
 *     gives the same bits.
 *   - get folds what is pending and copies sums[nprod][nband][nbin][cells] and state[ncomp][npre + nband*nsec][2][cells] out (per component: its pre
 *     sections first, then band 0's, ...), the cells dense in the region's order, z fastest; state may be NULL; nothing is reset.  set drops what is
 *     pending and replaces sums, state (NULL: zeros) and the count.  pf_vbandacc_count: the samples added, or the count given to set.
 *   - Between runs only, PF_ERR_STATE, an engine created with pf_opts.energy, handles of another engine or chain, several per engine, freeing by
 *     pf_engine_destroy / pf_multi_destroy: all as pf_bandacc.  PF_ERR_ARG, with a message that names the field, also for ncomp outside 1 .. 4, a
 *     comp value outside 0 .. 6, a repeated component, nprod outside 1 .. 10, a product index >= ncomp, a mode outside 0 / 1, a coefficient that is
 *     not finite, depth outside 0 .. 8.
 *   - Device memory, all of it the engine's: nprod*nband*nbin rows of sums and ncomp*(npre + nband*nsec)*2 rows of state (doubles, rows padded to an
 *     even cell count), ncomp * depth * cells Reals, and -- npre > 0 -- ncomp * depth rows of doubles.
 *   - A chain: as the band accumulators, one per slab over its part; add is all or nothing.  A difference across the cut reads the slab's ghost
 *     plane, which between runs holds the neighbour's u^n (the exchange of the step that wrote u^n filled it; pf_multi_load_state fills it).  A
 *     lattice difference beside a cut reads that plane at (y +- 1) and (z +- 1) too: it holds the neighbour's WHOLE plane.  The chain checks the
 *     one-cell rule against the scene's faces, a slab its part against its own planes. */
typedef struct pf_vbandacc pf_vbandacc;
int     pf_engine_vband_create (pf_engine *e, const pf_region *r, int32_t ncomp, const int32_t *comp, int32_t npre, const double *pre_sos, int32_t nband, int32_t nsec,
                                const double *band_sos, int32_t nprod, const int32_t *prod, int64_t nbin, int32_t depth, pf_vbandacc **out);
int     pf_engine_vband_add    (pf_engine *e, pf_vbandacc *a, int64_t bin);
int     pf_engine_vband_get    (pf_engine *e, pf_vbandacc *a, double *sums, double *state);
int     pf_engine_vband_set    (pf_engine *e, pf_vbandacc *a, const double *sums, const double *state, int64_t count);
int64_t pf_vbandacc_count      (const pf_vbandacc *a);
int     pf_engine_vband_destroy(pf_engine *e, pf_vbandacc *a);
int     pf_multi_vband_create  (pf_multi *m, const pf_region *r, int32_t ncomp, const int32_t *comp, int32_t npre, const double *pre_sos, int32_t nband, int32_t nsec,
                                const double *band_sos, int32_t nprod, const int32_t *prod, int64_t nbin, int32_t depth, pf_vbandacc **out);
int     pf_multi_vband_add     (pf_multi *m, pf_vbandacc *a, int64_t bin);
int     pf_multi_vband_get     (pf_multi *m, pf_vbandacc *a, double *sums, double *state);
int     pf_multi_vband_set     (pf_multi *m, pf_vbandacc *a, const double *sums, const double *state, int64_t count);
int     pf_multi_vband_destroy (pf_multi *m, pf_vbandacc *a);
/* ---- decimating recorders: per cell, EVERY sample low-pass filtered by a linear-phase FIR and every D-th output kept -- on the device ----
 * The impulse response of every cell of an audience plane (pffdtd_amd/recordings.py), D times smaller than a receiver per cell and not aliased as
 * raw frames every D steps are.  A decimating recorder belongs to one engine (or chain) and holds a region, npre (0 .. 8) second-order sections,
 * ntap (1 .. 4096) FIR taps h, a factor D (1 .. 64), a frame capacity cap (>= 1) and a ring of `depth` samples (1 .. 16, 0 = the default).
 * P = ceil(ntap / D) outputs are in flight at a time; P > 128 is refused.  No counterpart in the reference.
 *   - pf_engine_decim_add takes u^n of the region exactly as pf_engine_bandacc_add does (the same cut, the same ghost-shell rule); x = (double)u runs
 *     through the npre sections pre_sos[npre][5] by pf_bandacc's three lines, unchanged (state [npre][2][cells]).
 *   - The FIR is evaluated in ARRIVAL order, so the depth never changes a bit and a numpy loop gives the same bits.  For the sample with index n
 *     (the count of adds before it, from 0), with q = ceil(n / D), for every slot p = 0 .. P-1:
 *            m = q + ((p - q) mod P);  k = m*D - n          the output slot p carries, and the tap this sample meets in it
 *            k < ntap:  acc[p] = acc[p] + h[k] * x          the product rounded to double, then the sum: no fused multiply-add
 *            k == 0:    frame m = acc[p];  acc[p] = +0.0
 *     Frame m = sum_k h[k] x[m D - k] over the samples that exist (nothing is added for the time before sample 0); it completes with sample m D.
 *     P D >= ntap, so a slot never carries two outputs.  After `count` samples ceil(count / D) frames have completed.
 *   - Frames live on the device, frame m in row m mod cap.  read folds what is pending and copies the oldest min(max_frames, pending) frames in order
 *     as frames[nread][cells] (the cells dense in the region's order, z fastest), gives the index of the first, and marks them read.  add is refused
 *     with PF_ERR_STATE, nothing changed, when its sample would complete a frame (count % D == 0) while pending == cap.
 *   - get_state folds and copies acc[P][cells] in slot order and state[npre][2][cells] (may be NULL); nothing is reset.  set_state drops pending
 *     samples and unread frames and replaces acc (NULL: zeros), state (NULL: zeros) and the count; the next frame to complete is ceil(count / D).
 *     pf_decim_count: the samples added, or the count given to set_state.  pf_decim_pending: the frames complete and not yet read.
 *   - Between runs only, PF_ERR_STATE, an engine created with pf_opts.energy, handles of another engine or chain, several per engine, freeing by
 *     pf_engine_destroy / pf_multi_destroy: all as pf_bandacc.  PF_ERR_ARG, with a message that names the field, for npre, ntap, factor, P, cap or
 *     depth out of range, a tap or coefficient that is not finite, a null array, max_frames < 0, a negative count.
 *   - Device memory, all of it the engine's: P + cap + 2 npre rows of doubles (rows padded to an even cell count), depth * cells Reals, and
 *     -- npre > 0 -- depth rows of doubles.
 *   - A chain: as the band accumulators, one per slab over its part; add is all or nothing, and a full cap is refused before any slab samples. */
typedef struct pf_decim pf_decim;
int     pf_engine_decim_create   (pf_engine *e, const pf_region *r, int32_t npre, const double *pre_sos, int32_t ntap, const double *taps, int32_t factor,
                                  int64_t cap, int32_t depth, pf_decim **out);
int     pf_engine_decim_add      (pf_engine *e, pf_decim *a);
int     pf_engine_decim_read     (pf_engine *e, pf_decim *a, double *frames, int64_t max_frames, int64_t *first, int64_t *nread);
int     pf_engine_decim_get_state(pf_engine *e, pf_decim *a, double *acc, double *state);
int     pf_engine_decim_set_state(pf_engine *e, pf_decim *a, const double *acc, const double *state, int64_t count);
int64_t pf_decim_count           (const pf_decim *a);
int64_t pf_decim_pending         (const pf_decim *a);
int     pf_engine_decim_destroy  (pf_engine *e, pf_decim *a);
int     pf_multi_decim_create    (pf_multi *m, const pf_region *r, int32_t npre, const double *pre_sos, int32_t ntap, const double *taps, int32_t factor,
                                  int64_t cap, int32_t depth, pf_decim **out);
int     pf_multi_decim_add       (pf_multi *m, pf_decim *a);
int     pf_multi_decim_read      (pf_multi *m, pf_decim *a, double *frames, int64_t max_frames, int64_t *first, int64_t *nread);
int     pf_multi_decim_get_state (pf_multi *m, pf_decim *a, double *acc, double *state);
int     pf_multi_decim_set_state (pf_multi *m, pf_decim *a, const double *acc, const double *state, int64_t count);
int     pf_multi_decim_destroy   (pf_multi *m, pf_decim *a);
/* ---- vector decimating recorders: per cell, up to four COMPONENTS of the field, each low-pass filtered and decimated -- a B-format impulse response ----
 * A pf_decim keeps the pressure only: an omnidirectional microphone at every cell.  A vector decimating recorder keeps the time signal of the
 * pressure gradient beside it (pffdtd_amd/recordings.py: W and a figure-of-eight channel per axis).  It belongs to one engine (or chain) and holds a
 * region, ncomp (1 .. 4) components comp[], npre (0 .. 8) sections PER COMPONENT pre_sos[ncomp][npre][5], ONE FIR taps[ntap] shared by the
 * components, and factor, cap and depth with pf_decim's meaning and limits (P = ceil(ntap / factor) <= 128; depth 0 = the default).  No
 * counterpart in the reference.
 *   - comp[] means what it means to pf_engine_vband_create: 0 the cell, 1 / 2 / 3 the central difference along file x / y / z on fcc_flag == 0,
 *     4 / 5 / 6 the lattice difference on fcc_flag != 0, each formed in the field's own precision in exactly pf_vbandacc's association.  The
 *     refusals are pf_vbandacc's, by name: a repeated component, the wrong kind for the grid, a region not one cell clear of the faces the
 *     component needs.
 *   - add takes u^n at the same moment and under the same ghost-shell and fold-row rules as pf_engine_vband_add.  Component k's sample
 *     x_k = (double)component runs through pre_sos[k] by pf_bandacc's three lines and then through the FIR by pf_decim's lines, in ARRIVAL order
 *     (acc = acc + h[tap] * x, the product and the sum each rounded to double, no fused multiply-add).  The slot and tap arithmetic does not depend
 *     on the component.  Ring depth, cap and the slot group size never change a bit; a numpy loop per component gives the same bits.
 *   - read gives frames[nread][ncomp][cells]; get_state acc[ncomp][P][cells] and state[ncomp][npre][2][cells] (may be NULL); set_state (NULL:
 *     zeros), pf_vdecim_count, pf_vdecim_pending, a full cap refused with PF_ERR_STATE before the cut with nothing changed, PF_ERR_ARG and
 *     PF_ERR_STATE: all as pf_decim.
 *   - Device memory, all of it the engine's: ncomp * (P + cap + 2 npre) rows of doubles (rows padded to an even cell count), ncomp * depth * cells
 *     Reals, and -- npre > 0 -- ncomp * depth rows of doubles.  A 512 x 512 plane with 4 components and P = 98 holds 0.8 GB of acc alone; a create
 *     that does not fit fails with the allocator's error and leaves nothing behind.
 *   - A chain: one per slab over its part, as pf_vbandacc: a difference across the cut reads the slab's ghost plane, and the one-cell rule is checked
 *     against the scene's faces; add is all or nothing, and a full cap and the size of a read are decided before any slab is asked, as pf_decim. */
typedef struct pf_vdecim pf_vdecim;
int     pf_engine_vdecim_create   (pf_engine *e, const pf_region *r, int32_t ncomp, const int32_t *comp, int32_t npre, const double *pre_sos, int32_t ntap, const double *taps,
                                   int32_t factor, int64_t cap, int32_t depth, pf_vdecim **out);
int     pf_engine_vdecim_add      (pf_engine *e, pf_vdecim *a);
int     pf_engine_vdecim_read     (pf_engine *e, pf_vdecim *a, double *frames, int64_t max_frames, int64_t *first, int64_t *nread);
int     pf_engine_vdecim_get_state(pf_engine *e, pf_vdecim *a, double *acc, double *state);
int     pf_engine_vdecim_set_state(pf_engine *e, pf_vdecim *a, const double *acc, const double *state, int64_t count);
int64_t pf_vdecim_count           (const pf_vdecim *a);
int64_t pf_vdecim_pending         (const pf_vdecim *a);
int     pf_engine_vdecim_destroy  (pf_engine *e, pf_vdecim *a);
int     pf_multi_vdecim_create    (pf_multi *m, const pf_region *r, int32_t ncomp, const int32_t *comp, int32_t npre, const double *pre_sos, int32_t ntap, const double *taps,
                                   int32_t factor, int64_t cap, int32_t depth, pf_vdecim **out);
int     pf_multi_vdecim_add       (pf_multi *m, pf_vdecim *a);
int     pf_multi_vdecim_read      (pf_multi *m, pf_vdecim *a, double *frames, int64_t max_frames, int64_t *first, int64_t *nread);
int     pf_multi_vdecim_get_state (pf_multi *m, pf_vdecim *a, double *acc, double *state);
int     pf_multi_vdecim_set_state (pf_multi *m, pf_vdecim *a, const double *acc, const double *state, int64_t count);
int     pf_multi_vdecim_destroy   (pf_multi *m, pf_vdecim *a);
/* ---- wall absorption maps: the energy every step takes out of the room, per wall node, per material and per time bin -- on the device ----
 * Which surface absorbs the energy: the one output that reads the WALLS, not the air.  A pf_absorb belongs to one engine (or chain) and observes no
 * region: its nodes are the scene's frequency-dependent boundary nodes, its ABC nodes and its sources.  Per step n the reference Python engine's
 * terms (python/fdtd/sim_fdtd.py:615-620), with vh the branch currents before and after the step:
 *        wall node i:    wall_scale * ssaf_i * sum_m (vh_old + vh_new)^2_{i,m} * E[mat_i][m]      wall_scale = V_fac * 0.25 * h / l
 *        ABC node j:     abc_scale * 2^-Q_j * Q_j * (u^{n+1}_j - u^{n-1}_j)^2                     abc_scale  = 0.5 * V_fac * h / l
 *        source s:       in_scale * (u^{n+1}_s - u^{n-1}_s) * in_sig_s[n]                         in_scale   = 0.5 * V_fac * h / l2
 * (V_fac: 2 on FCC grids, else 1; E: the second column of the materials' DEF triplets; in_sig: the sample the engine adds, in the field's precision).
 * The wall terms are summed per node over the run and per material into a time bin, the ABC terms ("open boundary") and the source terms ("input")
 * into the same bin.  The sums of a run equal the diagnostic's E_lost and E_in -- on every engine path, every fcc_flag, exchanged-axes storage, slab
 * chains and across a checkpoint.  BROADBAND: the loss is quadratic in the branch currents, so a band's share needs a band-limited source.
 *   - add(n, bin) is called between two steps: n is the index of the engine's NEXT step, the state is (u^{n-1}, u^n).  The first add after create or
 *     set only primes (it copies the branch currents and u^{n-1} at the ABC and source nodes) and accounts nothing.  Every later add needs
 *     n == last + 1 -- a gap means the step's old branch currents are gone: PF_ERR_STATE, the message names both numbers -- and puts step n - 1's
 *     three quantities into `bin`.  One streaming pass over the node lists on the main stream, not waited for; the next step is ordered behind it.
 *   - Arithmetic: double throughout, sums over a node's branches in ascending order, no fused multiply-add, NO floating-point atomics.  The sums
 *     per material have an order fixed by the node order and the node count alone: the same run gives the same bits, and a run resumed from a
 *     checkpoint (get, pf_engine_save_state; pf_engine_load_state, set) the bits of the one-piece run.
 *   - get: nodes[Nbl] in the order of sd->bnl_ixyz, mats[nbin][Nm], abc[nbin], in[nbin]; a NULL array is skipped, nothing is reset.  set replaces the
 *     sums (NULL: zeros) and the count; the next add primes.  pf_absorb_count: the steps accounted so far, or the count given to set.
 *   - add, get and set are valid between runs only (PF_ERR_STATE inside a split-phase step or pass).  PF_ERR_ARG, with a message that names the
 *     field, for a null E, nbin < 1, bin outside 0 .. nbin - 1, n outside 1 .. Nt, a negative count, a handle of another engine, chain or kind.
 *     Scenes without frequency-dependent nodes (Nbl == 0) or without ABC nodes are fine: those rows stay zero.
 *   - Device memory, all of it the engine's: a copy of the branch currents (round_up(Nbl, 64) * 12 Reals), Nbl + nbin * (Nm + 2) doubles, one Real per
 *     ABC node and source, and the partial sums of one sample (Nm doubles per 256 nodes).
 *   - A chain: one per slab on its own device; a slab accounts the nodes of the planes it owns, so every node, ABC node and source is counted once.
 *     nodes are the slabs' rows put together (bit-equal to a single engine's), the bins the slabs' bins added in slab order on the host.  set gives
 *     the bins to slab 0: a chain resumed mid-bin sums that bin in another order than the chain in one piece, so its bins agree to rounding
 *     (Nbl * 2^-52 relative) while its nodes stay bit-equal; only a single engine resumes bit for bit.  add is all or nothing as
 *     pf_multi_accum_add: create the chain with PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES. */
typedef struct pf_absorb pf_absorb;
int     pf_engine_absorb_create (pf_engine *e, const double *E /*[Nm*PF_MMB]*/, double wall_scale, double abc_scale, double in_scale, int32_t nbin, pf_absorb **out);
int     pf_engine_absorb_add    (pf_engine *e, pf_absorb *a, int64_t n, int64_t bin);
int     pf_engine_absorb_get    (pf_engine *e, pf_absorb *a, double *nodes /*[Nbl], FILE order*/, double *mats /*[nbin*Nm]*/, double *abc /*[nbin]*/, double *in /*[nbin]*/);
int     pf_engine_absorb_set    (pf_engine *e, pf_absorb *a, const double *nodes, const double *mats, const double *abc, const double *in, int64_t count); /* null = zero; the next add primes */
int64_t pf_absorb_count         (const pf_absorb *a);   /* steps accounted */
int     pf_engine_absorb_destroy(pf_engine *e, pf_absorb *a);
int     pf_multi_absorb_create  (pf_multi *m, const double *E, double wall_scale, double abc_scale, double in_scale, int32_t nbin, pf_absorb **out);
int     pf_multi_absorb_add     (pf_multi *m, pf_absorb *a, int64_t n, int64_t bin);
int     pf_multi_absorb_get     (pf_multi *m, pf_absorb *a, double *nodes, double *mats, double *abc, double *in);
int     pf_multi_absorb_set     (pf_multi *m, pf_absorb *a, const double *nodes, const double *mats, const double *abc, const double *in, int64_t count);
int     pf_multi_absorb_destroy (pf_multi *m, pf_absorb *a);
int  pf_engine_timing(pf_engine *e, pf_timing *t, int32_t reset);
/* switch the per-launch HIP events of pf_opts.timing on / off between runs (a host times its headline region without them
 * and collects kernel durations in a region of its own) */
int  pf_engine_set_timing(pf_engine *e, int32_t on);

/* ---- energy-conservation diagnostic of the reference Python engine (python/fdtd/sim_fdtd.py:587-620,671-678) ----
 * Needs pf_opts.energy=1 at creation.  DEF = the materials' (D,E,F) triplets, double[Nm*PF_MMB*3] (zero padded),
 * h = grid spacing, c = speed of sound, Ts = time step (sim_consts.h5).  pf_engine_run_energy runs steps like
 * pf_engine_run and fills H_tot[n], E_lost[n+1], E_in[n+1] (arrays of Nt, Nt+1, Nt+1 doubles; E_*[0] must be
 * initialised by the caller).  fcc_flag 0 and 1 only, like the reference. */
int  pf_engine_energy_cfg(pf_engine *e, double h, double c, double Ts, const double *DEF);
int  pf_engine_run_energy(pf_engine *e, int64_t n0, int64_t nsteps, double *H_tot, double *E_lost, double *E_in);

#ifdef __cplusplus
}
#endif
#endif /* PFFDTD_HIP_H */
