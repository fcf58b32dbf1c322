/*
 * lbm_hip.h -- C ABI of the MI355X-native D2Q9-BGK engine (liblbm_hip.so).
 *
 * This is the drop-in boundary that replaces the Poplar Engine the reference
 * host (thorbenlouw/lbm-graphcore main/LbmRunner.cpp) drives.  Plain C types
 * only; no C++ exception crosses it; every call is blocking and non-reentrant
 * per handle.  The caller owns every host buffer; the library owns all device
 * memory, streams, events and the RCCL communicator and keeps no caller
 * pointer after a call returns.
 *
 * Layout at the boundary (unchanged from the reference):
 *   cells      AoS float[ny][nx][9], speed order 0 M,1 E,2 N,3 W,4 S,5 NE,6 NW,7 SW,8 SE
 *              (main/include/LatticeBoltzmannUtils.hpp:20-22, :125-157)
 *   obstacles  uint8[ny][nx], row-major, nonzero = blocked
 *              (main/include/LbmParams.hpp:67-128 stores bool[ny*nx])
 *   av_vels    float[max_iters]  (LbmRunner.cpp:70, stream "<<av_vel")
 * Inside the library the lattice is SoA f[9][ny+2][pitch] with a one-cell
 * ghost ring; the transpose happens in lbm_load_cells / lbm_store, off the
 * timed path.
 *
 * Return codes: 0 on success, a negative LBM_E* value on failure; the message
 * is available from lbm_last_error().
 */
#ifndef LBM_HIP_H
#define LBM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LBM_ABI_VERSION 5

enum {
    LBM_OK = 0,
    LBM_E_INVALID = -1,     /* bad argument / unsupported configuration */
    LBM_E_HIP = -2,         /* HIP runtime error */
    LBM_E_RCCL = -3,        /* RCCL error */
    LBM_E_NOMEM = -4,       /* host or device allocation failed */
    LBM_E_STATE = -5,       /* call out of order (e.g. lbm_run before lbm_load_cells) */
    LBM_E_INTERNAL = -6
};

/* lbm::Params (main/include/LbmParams.hpp:16-65): the 7-line params file. */
typedef struct lbm_params {
    int32_t nx;            /* cells in x (columns) */
    int32_t ny;            /* cells in y (rows) */
    int32_t max_iters;     /* steps per lbm_run */
    int32_t reynolds_dim;
    float density;
    float accel;
    float omega;
} lbm_params;

enum { LBM_TRANSPORT_LOCAL = 0, LBM_TRANSPORT_RCCL = 1 };
/* Step kernels.  SCALAR / VEC4: one time step per launch (VEC4 needs widths
 * that are multiples of 4).  STEP2: fused two-step launches through LDS.
 * STREAM: fused S-step launches (S = steps_per_launch, 2..6, 2..10 with
 * LBM_FLAG_TOLERANCE; default 6, 10 with it) streaming rows through registers; a run of
 * K steps is K / S launches plus, when 2 <= K % S, one fused launch of K % S
 * steps (else K % S one-step launches), single and decomposed domains alike.  RESIDENT: every step of a run in one persistent
 * launch with the lattice held on chip (LDS + registers) -- single
 * sub-domain grids small enough for all of their 64-column tiles to be
 * co-resident (1024x1024 and below on MI355X).  Its tiles hand populations to
 * each other through device memory, so all of them must run at once: the
 * grid is sized to the device's occupancy and launched cooperatively; if it
 * still cannot become co-resident (another kernel holding CUs: the runtime
 * refuses the cooperative launch, or a neighbour hand-off passes its 2 s
 * deadline) the run is repeated on the STEP2 kernel from the run's input
 * lattice -- untouched by the failed launch -- and returns LBM_OK with the
 * same lattice and av_vels; the handle keeps STEP2 afterwards
 * (lbm_kernel_in_use reports it, lbm_numerics reports bitwise) and prints one
 * line to stderr.  No run waits longer than one deadline for this.  PIPELINE: the unfused
 * reference pipeline, one kernel per stage and step (accelerate_flow ->
 * propagate -> rebound -> textbook BGK collision -> av_velocity,
 * main/LbmPoplibs.cpp:225-233) with the conditional accelerate at the start
 * of EVERY step -- for per-stage profiles; its numerics differ from the
 * fused scheme's in the last bits (both pass the reference gate).  AUTO picks the fastest
 * kernel the sub-domain sizes allow; lbm_kernel_in_use reports the choice.
 * LBM_FLAG_ONE_STEP forces one step per launch. */
enum {
    LBM_KERNEL_AUTO = 0,
    LBM_KERNEL_SCALAR = 1,
    LBM_KERNEL_VEC4 = 2,
    LBM_KERNEL_STEP2 = 3,
    LBM_KERNEL_STREAM = 4,
    LBM_KERNEL_RESIDENT = 5,
    LBM_KERNEL_PIPELINE = 6
};

/*
 * Placement of the 2-D block decomposition.
 *   LOCAL: this process owns every sub-domain; sub-domain i lives on device
 *          devices[i % num_devices] (NULL -> device i % visible devices) and
 *          halos move by device copies (peer copies across devices).  With
 *          several sub-domains on one device this is the loop-back mode the
 *          tests use to exercise the multi-GPU path on one GPU.
 *   RCCL:  one process per GPU; this process owns sub-domain `rank` on
 *          devices[0] (or `rank` % visible devices) and halos move with
 *          grouped ncclSend/ncclRecv over xGMI.  rccl_unique_id must hold the
 *          128 bytes from lbm_rccl_unique_id() of rank 0.
 * grid_rows/grid_cols = 0 selects the reference's partitionForIpus rule
 * (main/include/StructuredGridUtils.hpp:472-561) for `parts` sub-domains.
 */
typedef struct lbm_config {
    int32_t parts;          /* number of sub-domains (>= 1) */
    int32_t grid_rows;      /* 0 = choose by rule */
    int32_t grid_cols;      /* 0 = choose by rule */
    int32_t transport;      /* LBM_TRANSPORT_* */
    int32_t rank;           /* RCCL only */
    int32_t world;          /* RCCL only; must equal parts */
    const int32_t *devices; /* optional device list */
    int32_t num_devices;
    const uint8_t *rccl_unique_id; /* 128 bytes, RCCL only */
    int32_t kernel;         /* LBM_KERNEL_* */
    int32_t graph_steps;    /* >0: replay the step loop as hipGraphs of 2*graph_steps steps
                               (single sub-domain without exchange); <0: off; 0: library default */
    int32_t flags;          /* LBM_FLAG_* */
    int32_t steps_per_launch; /* STREAM: time steps fused per launch (2..6; 2..10 with LBM_FLAG_TOLERANCE);
                                 0 = library default: 6 (10 with LBM_FLAG_TOLERANCE), lowered to the
                                 deepest S every sub-domain allows (S cells, 2S across a decomposed
                                 dimension) */
} lbm_config;

/* Route the periodic wrap of undecomposed dimensions through the transport
 * too (send to / receive from itself) instead of writing the ghost ring
 * in-kernel.  Lets one GPU exercise the full exchange path, RCCL included. */
#define LBM_FLAG_FORCE_EXCHANGE 1
/* One time step per launch (no fused two-step kernel). */
#define LBM_FLAG_ONE_STEP 2
/* fp32 tolerance mode of the STREAM kernel (north_star: "within a stated fp32
 * tolerance"): one reciprocal of the density per cell
 * (v_rcp_f32, 1 ulp) shared by u_x and u_y instead of two
 * correctly rounded divisions, the constant divisions by 9 and 36 folded into
 * multiplications, and FMA contraction.  Still IEEE fp32 arithmetic, but no
 * longer bitwise equal to LastChance.cpp:226-262.  Stated tolerance (tested in
 * tests/test_gpu_tolerance.py): every population within 2e-5 relative of the
 * oracle for runs of up to 100 steps (8192^2, 16384^2), and within 2e-3 over
 * the full reference runs (20000-80000 steps on all four reference grids,
 * measured <= 9.0e-4), av_vels within 2e-4 relative over <= 100 steps (2e-3
 * at 8192^2 / 16384^2, where the oracle's own sequential fp32 sum of 67 M+
 * terms drifts by that much) and within 2e-3 over the full runs (measured
 * <= 1.5e-3), and the two-file check.py gate passes
 * on all four grids.  The
 * packed RESIDENT tiles take the same collision (and the D3Q19 engine's
 * two-step passes); the other kernels (one-step remainder launches, STEP2,
 * VEC4, the scalar resident tiles) stay bitwise.
 * lbm_numerics() reports which mode a handle runs. */
#define LBM_FLAG_TOLERANCE 4
/* Per-launch device timing (lbm_profile_summary): every launch is bracketed
 * by a pair of HIP events on its own stream and folded per launch class after
 * each run; hipGraph replay is off.  Costs a few microseconds per launch; off
 * by default.  The counterpart of the reference's engine.printProfileSummary
 * under LbmRunner -d (LbmRunner.cpp:115-122). */
#define LBM_FLAG_PROFILE 8

typedef struct lbm_handle lbm_handle;

/* Sub-domain rectangle in global cell coordinates. */
typedef struct lbm_rect {
    int32_t x0, y0, w, h;
} lbm_rect;

/* ---- host-only helpers (no GPU needed) -------------------------------- */

int32_t lbm_abi_version(void);

/*
 * Reference partition rule, StructuredGridUtils.hpp:472-561 partitionForIpus:
 * parts in {1,2,4,8,16} -> rows x cols (2: by imbalance, 8: 4x2 or 2x4 by
 * imbalance), round-robin row/col allocation (:161-165), rank = row*cols+col
 * (:548).  Writes rows/cols and, if rects != NULL, `parts` rectangles.
 */
int lbm_partition(int32_t nx, int32_t ny, int32_t parts, int32_t grid_rows, int32_t grid_cols,
                  int32_t *rows_out, int32_t *cols_out, lbm_rect *rects);

/*
 * Halo exchange plan (host-only): for each of the 8 directions d (order E, N,
 * W, S, NE, NW, SW, SE = velocities of speeds 1..8) writes 6 ints
 * {dx, dy, nplanes, plane0, plane1, plane2} (unused planes = -1): the
 * populations that leave a sub-domain through side d and land in the
 * neighbour's ghost ring on the opposite side.  Replaces the stitched-halo
 * views of the reference (GraphcoreUtils.hpp:119-127,
 * StructuredGridUtils.hpp:805-851), which copy whole 9-speed cells.
 */
int lbm_halo_plan(int32_t table[48]);

/*
 * The exact, ordered list of transfers one rank's halo exchange posts
 * (host-only; the engine's RCCL exchange iterates the same list inside one
 * ncclGroupStart/End, lbm_engine.hip exchange_posts).  RCCL pairs the
 * messages between two ranks by posting order only, so a checker that pairs
 * every rank's list proves the matching, extent-2 dimensions (one peer on
 * two or more sides) included.  Reference behaviour replaced: the periodic
 * halo slices of StructuredGridUtils.hpp:805-851 / the stitched halos of
 * LbmAoS.cpp:151-160.
 *   op      LBM_XFER_SEND: the halo leaving through side `dir` to `peer`;
 *           LBM_XFER_RECV: ghost side `dir` filled from `peer`;
 *           LBM_XFER_SELF: side `dir` wraps onto this rank (written in place
 *           by the step kernel, nothing posted)
 *   dir     0..7 = E, N, W, S, NE, NW, SW, SE (lbm_halo_plan order)
 *   floats  message length: W1 = the populations leaving through the side
 *           (lbm_halo_plan) x edge length; WG = all 9 populations of the
 *           halo_width outermost rows / columns (halo_width^2 x 9 at corners)
 * halo_mode LBM_HALO_W1 (one-step launches) or LBM_HALO_WG (fused launches,
 * halo_width = steps per launch).  force_exchange as LBM_FLAG_FORCE_EXCHANGE.
 * *n_out = number of entries (at most 24); out may be NULL to query it.
 */
enum { LBM_XFER_SEND = 0, LBM_XFER_RECV = 1, LBM_XFER_SELF = 2 };
enum { LBM_HALO_W1 = 1, LBM_HALO_WG = 2 };
typedef struct lbm_xfer {
    int32_t op, dir, peer, reserved;
    int64_t floats;
} lbm_xfer;
int lbm_exchange_schedule(int32_t nx, int32_t ny, int32_t parts, int32_t grid_rows, int32_t grid_cols, int32_t rank,
                          int32_t halo_mode, int32_t halo_width, int32_t force_exchange, lbm_xfer *out,
                          int32_t max_out, int32_t *n_out);

/* Number of visible HIP devices (0 on a host without GPUs; never fails). */
int32_t lbm_device_count(void);

/* 128-byte RCCL unique id for rank 0 to broadcast (ncclGetUniqueId). */
int lbm_rccl_unique_id(uint8_t out[128]);

/* ---- engine ------------------------------------------------------------ */

/*
 * ≙ Engine(Executable::deserialize(..)) + connectStream(">>obstacles") +
 *   engine.load(device)  (main/LbmRunner.cpp:81-96).
 * Single process driving `num_gpus` devices (LbmRunner's -n), LOCAL transport.
 * obstacles: uint8[ny][nx] (full domain).
 */
int lbm_create(const lbm_params *params, const uint8_t *obstacles, int32_t num_gpus,
               lbm_handle **out);

/* As lbm_create with an explicit placement (see lbm_config). */
int lbm_create_ex(const lbm_params *params, const uint8_t *obstacles, const lbm_config *config,
                  lbm_handle **out);

/*
 * ≙ engine.run(0) with stream ">>cells" (LbmRunner.cpp:86-100):
 * host AoS float[ny][nx][9] (full domain) -> device.  Every process passes
 * the full-domain array; each takes its sub-domain(s).
 */
int lbm_load_cells(lbm_handle *h, const float *cells_aos);

/* Equilibrium initial state on the device (≙ lbm::Cells::initialise,
 * LatticeBoltzmannUtils.hpp:137-157, without a host array). */
int lbm_init_equilibrium(lbm_handle *h);

/*
 * ≙ engine.run(1) (LbmRunner.cpp:102-104; graph program LbmAoS.cpp:349-356):
 * the one-time conditional accelerate of row ny-2, then max_iters fused
 * steps, with av_vels kept on the device.  Blocking.
 */
int lbm_run(lbm_handle *h);

/* `steps` fused steps, optionally preceded by the first accelerate (bench / tests). */
int lbm_run_steps(lbm_handle *h, int32_t steps, int32_t accelerate_first);

/*
 * ≙ engine.run(2) with "<<cells"/"<<av_vel" (LbmRunner.cpp:85-108).
 * cells_aos: full-domain AoS (may be NULL).  In RCCL mode only this rank's
 * sub-domain is written into the full-size array (others untouched).
 * av_vels: float[n_av] for the last lbm_run/lbm_run_steps, each entry
 * sum over ALL ranks of |u| / total free cells (may be NULL).
 */
int lbm_store(lbm_handle *h, float *cells_aos, float *av_vels, int32_t n_av);

/*
 * Per-rank host I/O (one process per GPU at scale: a 16384^2 lattice is
 * 9.66 GB of AoS per copy, so ranks should not each hold the full domain).
 * cells_aos_local: this handle's local sub-domains only, each AoS
 * float[h][w][9] of its lbm_local_rects rectangle, packed one after another
 * in lbm_local_rects order (RCCL: the rank's one rectangle);
 * lbm_local_cells() = the sum of w*h.  Same semantics as lbm_load_cells /
 * lbm_store otherwise (av_vels are still the all-rank values).  A rank-0
 * reader scatters the rectangles (lbm_amd.io.scatter_subdomains) and gathers
 * them back for the .dat writers (gather_subdomains); the reference's
 * single-process LbmRunner (LbmRunner.cpp:67-108) keeps using lbm_load_cells.
 */
int lbm_load_cells_local(lbm_handle *h, const float *cells_aos_local);
int lbm_store_local(lbm_handle *h, float *cells_aos_local, float *av_vels, int32_t n_av);
int64_t lbm_local_cells(lbm_handle *h);

/*
 * Macroscopic fields of the current lattice, computed on the device: the
 * u_x, u_y, |u| and pressure columns of final_state.dat without moving the
 * nine populations to the host (lbm_store + writeResults move 36 B per cell
 * and hold a second AoS lattice on the device; this moves 4 B per cell and
 * requested field).
 * Planar float[ny][nx] each, full domain; any pointer may be NULL (not
 * computed).  RCCL: only this rank's rectangle is written.  Exactly the
 * values lbmhost::writeResults derives from lbm_store's cells
 * (LatticeBoltzmannUtils.hpp:221-281: sequential density sum, correctly
 * rounded divide and sqrt; an obstacle cell gives 0, 0, 0, density * (1.f / 3.f)),
 * bit for bit, whatever kernel or numerics mode advanced the lattice.
 * LBM_E_STATE before lbm_load_cells / lbm_init_equilibrium.
 */
int lbm_store_fields(lbm_handle *h, float *ux, float *uy, float *speed, float *pressure);
/* Local sub-domains only, each float[h][w], packed in lbm_local_rects order. */
int lbm_store_fields_local(lbm_handle *h, float *ux, float *uy, float *speed, float *pressure);
/* Sum over this handle's sub-domains of every cell's density (fp64
 * accumulation of the fp32 per-cell sums) and the largest |u| of its fluid
 * cells (0 when there are none).  Either pointer may be NULL.  Folded in a
 * fixed order: two calls on the same lattice return identical bits. */
int lbm_field_stats(lbm_handle *h, double *mass, float *max_speed);

/* ≙ engine.readTensor("readTimer") (LbmRunner.cpp:133-144):
 * device-event seconds of the last lbm_run / lbm_run_steps. */
int lbm_last_run_seconds(lbm_handle *h, double *seconds);

/* Total non-obstacle cells of the full domain (LastChance.cpp:486-493). */
int64_t lbm_total_free_cells(lbm_handle *h);

/* Local sub-domain rectangles of this handle (LOCAL: all; RCCL: this rank's). */
int lbm_local_rects(lbm_handle *h, lbm_rect *rects, int32_t max_rects, int32_t *n_out);

/* Which step kernel the handle uses (LBM_KERNEL_RESIDENT, _STREAM, _STEP2,
 * _VEC4, _SCALAR or _PIPELINE), and how many time steps one of its launches advances
 * (RESIDENT: all steps of a run -- the last run's count, max_iters before
 * the first run). */
int32_t lbm_kernel_in_use(lbm_handle *h);
int32_t lbm_steps_per_launch(lbm_handle *h);

/* Launches of the last lbm_run / lbm_run_steps: fused (steps_per_launch
 * steps each; RESIDENT: the one persistent launch) and one-step (the
 * remainder of a step count that is not a multiple, or every step in
 * one-step modes).  Lets a test prove which kernel advanced the lattice. */
int lbm_run_stats(lbm_handle *h, int32_t *fused_launches, int32_t *one_step_launches);

/* Read-only view of the stream kernel's work units (strip x segment, one wave
 * each): per local sub-domain (lbm_local_rects order) the interior
 * launch's units in unit index order, then the boundary launch's.  x0, y0, w,
 * h: the cells the unit owns (writes), sub-domain-local, from the same helper
 * the kernel's geometry uses; reads_obstacle: the per-unit flag the kernel
 * reads, copied back from the device (1: the unit runs the copy with obstacle
 * loads and rebound selects, 0: the select-free copy), -1 for every unit of a
 * handle without flags (LBM_STREAM_UOBST=0: every unit runs the first copy).
 * *n_out = number of units; at most max_out entries are written, and out may
 * be NULL to ask for the count.  LBM_E_STATE when the handle's kernel is not
 * the stream kernel, LBM_E_INVALID when h or n_out is NULL.  An additive part
 * of the ABI (LBM_ABI_VERSION unchanged). */
typedef struct lbm_stream_unit {
    int32_t sub;            /* index in lbm_local_rects order */
    int32_t boundary;       /* 0 interior launch, 1 boundary launch */
    int32_t x0, y0, w, h;   /* owned cells, sub-domain-local */
    int32_t reads_obstacle; /* the flag the kernel reads; -1 if the handle has none (LBM_STREAM_UOBST=0) */
} lbm_stream_unit;
int lbm_stream_units(lbm_handle *h, lbm_stream_unit *out, int32_t max_out, int32_t *n_out);

/* Placement probe of lbm_create: the candidate lattice pair kept
 * (-1: no probe ran), how many pairs were timed, and (up to max_ms of) their
 * ms per launch. */
int lbm_placement_probe(lbm_handle *h, int32_t *kept, int32_t *tried, float *ms_per_launch, int32_t max_ms);

/* Launch-class device time accumulated over every run of a handle created
 * with LBM_FLAG_PROFILE (since creation or lbm_profile_reset): one entry per
 * class -- e.g. "stream_steps2d S=10 tolerance", "... interior" / "...
 * boundary" on decomposed grids, "halo exchange WG (RCCL) + unpack",
 * "accelerate_row", "finalize_av", "resident_steps (all steps, one launch)",
 * the pipeline stages, "macroscopic_fields" (lbm_store_fields; lbm_field_stats:
 * "macroscopic_fields stats") -- with its launch count and total / min / max ms
 * between the events around each launch.  *n_out = number of classes; at most
 * max_out entries are written.  LBM_E_STATE without the flag. */
typedef struct lbm_kernel_time {
    char name[64];
    int64_t launches;
    double total_ms, min_ms, max_ms;
} lbm_kernel_time;
int lbm_profile_summary(lbm_handle *h, lbm_kernel_time *out, int32_t max_out, int32_t *n_out);
int lbm_profile_reset(lbm_handle *h);

/* 0: every kernel of the handle is bitwise equal to the CPU oracle; 1: the
 * fused launches run the LBM_FLAG_TOLERANCE collision. */
int32_t lbm_numerics(lbm_handle *h);

/* Debug scan: number of NaN / +-Inf populations in the current
 * lattice of this handle's sub-domains.  With LBM_NAN_CHECK=1 in the
 * environment every lbm_run / lbm_run_steps ends with this scan and fails
 * with LBM_E_INTERNAL when it finds any. */
int lbm_nonfinite_count(lbm_handle *h, int64_t *count);

/* Hash of the library's sources (csrc/, include/) at build time; the Python
 * binding refuses a library whose hash differs from the sources beside it. */
const char *lbm_source_hash(void);

const char *lbm_last_error(lbm_handle *h);

void lbm_destroy(lbm_handle *h);

#ifdef __cplusplus
}
#endif

#endif /* LBM_HIP_H */
