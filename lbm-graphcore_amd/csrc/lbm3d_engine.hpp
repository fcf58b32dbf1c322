// lbm3d_engine.hpp -- declaration of the D3Q19 engine behind the C ABI
// (include/lbm3d_hip.h), shared by its units:
//   lbm3d.hip          the step kernels (one step per launch, two and three
//                      steps per pass) and their launch_* wrappers;
//   lbm3d_engine.hip   create, tuning knobs, allocation, placement probe, the
//                      step loop, ghost exchange, load / store / destroy;
//   lbm3d_fields.hip   macroscopic fields and lattice stats (kernel + host side);
//   lbm3d_forces.hip   momentum-exchange wall forces (kernels + host side);
//   lbm3d_averages.hip time-averaged fields and Reynolds stresses (kernels + host side);
//   lbm3d_gradients.hip vorticity, divergence, strain rate and Q (kernel + host side);
//   lbm3d_stress.hip   strain rate and wall shear from the non-equilibrium moments (kernel + host side);
//   lbm3d_binned.hip   sums over box-shaped bins of the current lattice (kernel + host side);
//   lbm3d_tracers.hip  Lagrangian tracers and point probes (host side; kernels in lbm_tracers.hpp);
//   lbm3d_scalar.hip   passive scalar: a D3Q7 lattice beside the flow lattice (step kernel, host side;
//                      shared parts in lbm_scalar.hpp);
//   lbm3d_transport.hip binned transport sums of the scalar (kernel + host side; terms in lbm_transport.hpp);
//   lbm3d_scalar_walls.hip wall models of the scalar and the per-body wall flux (host side; kernels in
//                      lbm_scalar_walls.hpp);
//   lbm3d_forcing.hip  forcing zones: body force, drag and velocity target on boxes of cells (kernel, host
//                      side; shared parts in lbm_forcing.hpp);
//   lbm3d_sgs.hip      sub-grid model: a local relaxation rate by rescaling the stored non-equilibrium part
//                      (kernel, host side; shared parts in lbm_sgs.hpp);
//   lbm3d_abi.hip      the extern "C" functions and the RCCL posting order.
// The diagnostics units (fields to binned) share their host paths through
// lbm_diag_host.hpp and their cell reads and block fold through lbm_quad.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <array>
#include <string>
#include <utility>
#include <vector>

#include "lbm3d_fields.hpp"
#include "lbm3d_fields_hip.h"
#include "lbm_diag_host.hpp"
#include "lbm_forces.hpp"
#include "lbm_forces_hip.h"

namespace lbm {

namespace avg {
struct State;  // accumulators of a handle that is averaging (lbm_moments.hpp)
}
namespace tracer {
struct State;  // point set of a handle that keeps tracers (lbm_tracers.hpp)
}
namespace scalar {
struct State;  // scalar lattice of a handle that carries a passive scalar (lbm_scalar.hpp)
}
namespace forcing {
struct State;  // zones of a handle that set a forcing zone (lbm_forcing.hpp)
}
namespace sgs {
struct State;  // model of a handle that set a sub-grid model (lbm_sgs.hpp)
}
namespace grad {
struct Grad3Args;  // lbm_gradients.hpp
}
namespace stress {
struct State3;       // near-wall class maps of a handle that asked for strain statistics (lbm3d_stress.hip)
struct Stress3Args;  // lbm_stress.hpp
}

constexpr int Q3 = 19;
constexpr int GZ3 = 3;  // ghost planes each side of every slab lattice (and obst_g)

struct Step3Args {
    const float *fin;        // origin (plane z = 0) of the lattice read
    float *fout;             // origin of the lattice written
    const uint8_t *obst;     // [nzs][ny][nx]
    long long PL, KS;        // plane stride, speed stride (floats)
    int px, nx, ny;
    int z0;                  // first plane of this launch
    float omega, omo, w1, w2;
    float *partials;         // this launch writes partials[block]
};

struct Two3Args {
    const float *fin;   // origin of the lattice read (ghost planes -2, -1, nz, nz + 1 filled)
    float *fout;
    const uint8_t *obst;  // plane 0 of [nz + 6][ny][nx]: three planes of neighbour / periodic images each side
    long long PL, KS;
    int px, nx, ny, nz, seg;
    int z0, zn;           // output planes [z0, zn) of this launch, in segments of seg planes
    float omega, omo, w1, w2;
    float k0, k1, k2;     // tolerance collision: omega / 3, omega / 18, omega / 36
    float *partials;      // [2][nblocks]: |u| of step t+1, then t+2, at blk0 + this launch's block
    int nblocks, blk0;
};

// Launchers of lbm3d.hip.  Each owns its grid; the *_blocks functions give the
// blocks (= |u| partials) of the launch over the same arguments.  A launch
// over no planes enqueues nothing and succeeds.
// One step of `planes` planes from a.z0: step3d, or (pair) step3d_pair<zb, nt>.
int step3d_blocks(int nx, int ny, int planes, bool pair, int zb);
hipError_t launch_step3d(const Step3Args &a, int planes, bool pair, int zb, bool nt, hipStream_t s);
// switch key of the instantiated step3d_two<PD> variants (12 rows, no skip, PD 0 | 1), -1 if none
int two_variant(int th, bool skip, int pd);
// n steps (n = 2, 3) of planes [a.z0, a.zn) in segments of a.seg planes:
// step3d_two<variant> or (tol) its tolerance form; step3d_three<tol, skip>.
int pass3d_blocks(int n, int nx, int ny, int planes, int seg);
hipError_t launch_step3d_two(const Two3Args &a, int variant, bool tol, hipStream_t s);
hipError_t launch_step3d_three(const Two3Args &a, bool tol, bool skip, hipStream_t s);
hipError_t launch_reduce3d(const float *partials, int n, float *av_local, int t, hipStream_t s);
hipError_t launch_init3d(float *base, long long planes, long long KS, long long PL, float c0, float c1, float c2,
                         hipStream_t s);
// AoS [nzs][ny][nx][19] staging <-> lattice interior, n cells
hipError_t launch_aos_to_soa3d(const float *aos, float *f, long long PL, long long KS, int px, int nx, int ny,
                               long long n, hipStream_t s);
hipError_t launch_soa_to_aos3d(const float *f, float *aos, long long PL, long long KS, int px, int nx, int ny,
                               long long n, hipStream_t s);
hipError_t launch_debug_spin(int microseconds, hipStream_t s);  // lbm_kernels.hip

// The ordered posts of one z slab's ghost exchange (RCCL pairs them by
// order inside one ncclGroupStart/End): send up (dir 0, +z) to rank+1, send
// down (dir 1, -z) to rank-1, receive the below ghosts (dir 1) from rank-1,
// receive the above ghosts (dir 0) from rank+1 -- periodic in z.  `floats`
// per message: 5 speed planes for a one-step launch, n whole planes (all 19
// speeds) for an n-step pass.  post_exchange() posts exactly this list;
// lbm3d_exchange_schedule exports it.  (lbm3d_abi.hip)
std::array<lbm_xfer, 4> slab_posts(int rank, int world, long long floats);

struct Slab {
    int id = 0, dev = 0, z0 = 0, nzs = 0;
    float *f[2] = {nullptr, nullptr};  // allocations (ghost plane below first)
    bool f_joint = false;              // f[1] lies in f[0]'s allocation (LBM_LATTICE_PAD)
    float *o[2] = {nullptr, nullptr};  // origins: plane z = 0
    uint8_t *obst = nullptr;
    uint8_t *obst_g = nullptr;   // [nzs + 6][ny][nx]: obst with three image planes each side (two/three-step kernels)
    float *partials = nullptr;
    int nblk_all = 0, nblk_bnd = 0, nblk_int = 0;
    // n-step passes (n = 2, 3; index n - 2): |u| partials [n][nblk] and the blocks of one pass
    float *pass_partials[2] = {nullptr, nullptr};
    int pass_nblk[2] = {0, 0};
    float *av_local = nullptr;
    int av_cap = 0;
    int cur = 0;
    hipStream_t s_comp = nullptr, s_bnd = nullptr, s_comm = nullptr;
    hipEvent_t ev_b = nullptr, ev_i = nullptr, ev_x = nullptr, ev_end = nullptr;
};

// one exchange's four message ends of a slab, as offsets (floats) from the
// origin of the lattice exchanged, and the floats per message
struct Ends3 {
    long long up_src, down_src, ghost_lo, ghost_hi, floats;
};

}  // namespace lbm

struct lbm3d_handle {
    lbm3d_params p{};
    int parts = 1, transport = LBM_TRANSPORT_LOCAL, rank = 0, world = 1;
    int px = 0;
    long long KS = 0, PL = 0;
    bool pair = true;  // column-pair kernel (nx even; LBM3D_PAIR=0 forces the one-cell kernel)
    // tuned at 512^3 (profiles/r01/d3q19/ab_zb_nt.log): 2 planes per block,
    // non-temporal stores (the lattice written now is read a whole step later)
    int zb = 2;        // LBM3D_ZB: planes per block of the pair kernel (1, 2, 4, 8)
    bool nt = true;    // LBM3D_NT: non-temporal output stores
    bool two = true;   // LBM3D_TWO: two steps per pass (step3d_two), single slab or z slabs
    // LBM3D_THREE: three steps per pass (step3d_three), one slab or z slabs of
    // >= 6 planes (needs two);
    // default (-1): both modes since round 4 (with skip3) -- 512^3, skip3 on:
    // tolerance 55.4-55.6 GLUPS, bitwise 51.2-51.3 vs 44.1-45.2 for two-step
    // passes (profiles/r04/d3q19/ab_skip3.log); round 3, skip3 off, had kept
    // bitwise on two-step passes (43.9-44.1 vs 44.6-45.0: the divisions made
    // the third level's recompute VALU-bound)
    int three = -1;
    int seg3 = 64;     // LBM3D_SEG3: z planes per block of the three-step kernel
    int seg = 64;      // LBM3D_SEG: z planes per block of the two-step kernel (32-128 equal within noise at 512^3)
    int th = 12;       // LBM3D_TH: rows (waves) per block of the two-step kernel (12 only since round 3)
    bool skip = false; // LBM3D_SKIP: waves skip the collisions of rows no later level reads (not faster)
    // LBM3D_SKIP3: the same in the three-step pass -- there it pays (default on):
    // the live rows per level (10, 8, 6 of 12) spread over the 4 SIMDs as
    // 3 + 2 + 2 wave-collisions on the busiest SIMD instead of 3 + 3 + 3;
    // 512^3 tolerance 55.4-55.6 vs 45.6-50.0 GLUPS, bitwise 51.2-51.3 vs 43.7-43.9
    bool skip3 = true;
    // LBM3D_PD: input planes in flight in the two-step kernel -- 0 (default): the
    // next plane loaded once level 1 has consumed the current one (44.7 vs
    // 38.6-42.5 GLUPS at 512^3 for 1, profiles/r03/d3q19/ab_pd.log); 1, 2
    int pd = 0;
    long long kspad = 0;  // LBM3D_KSPAD: floats appended to each speed plane (multiple of 64)
    const char *lattice_pad = nullptr;  // LBM_LATTICE_PAD (debug knob)
    bool poison = false;  // LBM_POISON=1: fresh allocations filled with NaN bytes
    int probe_tries = 6;  // LBM3D_PLACEMENT_TRIES: lattice pairs the placement probe times (1 = off)
    long long probe_min_cells = 1LL << 26;  // LBM3D_PROBE_MIN_CELLS: smallest single slab probed
    bool probe_three = true;                 // LBM3D_PROBE_THREE=0: three-step engines skip the probe (A/B)
    bool probe_log = false;  // LBM_PLACEMENT_LOG: print the probe's per-pair times
    // ordering regression knobs (debug only, tests/test_gpu_ordering.py): slab
    // LBM_DEBUG_DELAY_SUB's boundary and interior launches are each preceded
    // by a stall of LBM_DEBUG_DELAY_US on their stream
    int delay_sub = -1, delay_us = 0;
    bool tolerance = false;  // LBM_FLAG_TOLERANCE: the two-step passes use cell3dt (not bitwise)
    std::vector<lbm::Slab> slabs;
    std::vector<int> all_z0, all_nz;
    ncclComm_t comm = nullptr;
    int64_t free_cells = 0;
    bool loaded = false;
    int last_steps = 0;
    int run_three = 0, run_two = 0, run_one = 0;  // passes / one-step launches of the last run_steps (lbm3d_run_stats)
    double last_seconds = 0.0;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    std::string err;
    // momentum-exchange wall forces (lbm_forces_hip.h): one wall list per slab, built at the first force call
    std::vector<lbm::forces::WallList> walls;
    bool walls_built = false;
    int wall_bodies = 0;  // bodies set (0: none)

    // several slabs, or RCCL transport (then even one rank sends its faces to
    // itself through RCCL: the exchange path is testable on one GPU)
    bool multi() const { return parts > 1 || transport == LBM_TRANSPORT_RCCL; }
    float w1() const { return p.density * p.accel / 18.f; }
    float w2() const { return p.density * p.accel / 36.f; }

    // lbm3d_engine.hip
    void read_tuning();
    void create(const lbm3d_params *prm, const uint8_t *obstacles, const lbm_config &cfg);
    void placement_probe();
    void alloc(lbm::Slab &s, const uint8_t *obstacles);
    void fill_fresh(void *ptr, size_t bytes, hipStream_t st) const;
    int blocks_for(int planes) const { return lbm::step3d_blocks(p.nx, p.ny, planes, pair, zb); }
    bool use_pass(int n) const;
    bool use_two() const { return use_pass(2); }
    bool use_three() const { return use_pass(3); }
    std::vector<std::pair<int, int>> pass_ranges(int n, const lbm::Slab &s) const;
    int pass_seg(int n) const { return n == 3 ? seg3 : seg; }
    int pass_blocks(int n, int z0, int zn) const { return lbm::pass3d_blocks(n, p.nx, p.ny, zn - z0, pass_seg(n)); }
    void launch_pass(int n, lbm::Slab &s, int z0, int zn, int blk0, hipStream_t st);
    void reduce_pass(int n, lbm::Slab &s, int t, hipStream_t st);
    void step_pass_multi(int n, int t);
    void step_pass(int n, int t);
    void ensure_av(int n);
    lbm::Slab *local(int id);
    lbm::Ends3 ends(const lbm::Slab &s, int n) const;
    void post_exchange(int l, int n, bool use_comm);
    void exchange(int l, bool use_comm);
    void stall(const lbm::Slab &s, hipStream_t st);
    void wait_x(lbm::Slab &s, hipStream_t st);
    void launch(lbm::Slab &s, int zfirst, int planes, float *partials, hipStream_t st);
    void step_once(int t);
    void sync_all();
    void refresh();
    void run_steps(int steps);
    void init_equilibrium();
    void load_cells(const float *aos);
    void store(float *aos, float *av, int n_av);
    void destroy();
    // lbm3d_fields.hip
    lbm::Box3View box_view(const lbm::Slab &s, int x0, int y0, int z0, int bx, int by, int bz) const;
    lbm::Box3Edit slab_edit(const lbm::Slab &s) const {  // every cell of the slab, writable
        return lbm::Box3Edit{box_view(s, 0, 0, 0, p.nx, p.ny, s.nzs), s.o[s.cur]};
    }
    void check_box(const lbm3d_box &b) const;
    bool slab_planes(const lbm::Slab &s, const lbm3d_box &b, int &zlo, int &zhi) const;
    // where the box's planes from global plane zlo on lie in a packed host array float[b.nz][b.ny][b.nx]
    static lbm::HostSpan box_span(const lbm3d_box &b, int zlo) {
        return lbm::HostSpan{(size_t)(zlo - b.z0) * b.ny * b.nx, (size_t)b.nx};
    }
    void store_fields_box(const lbm3d_box &b, float *const (&host)[5]);
    void field_stats(double *mass, float *max_speed);
    // lbm3d_forces.hip
    std::vector<uint8_t> obst_g_host(const lbm::Slab &s) const;
    void walls_build();
    void walls_release();
    void wall_force(double *fx, double *fy, double *fz, int64_t *links);
    void store_wall_force(float *const (&host)[3]);
    void set_bodies(const int32_t *labels, int32_t nbodies);
    void body_forces(double *fx, double *fy, double *fz, int64_t *links, int32_t nbodies);
    // lbm3d_averages.hip (include/lbm_averages_hip.h)
    lbm::avg::State *averages = nullptr;  // set between avg_begin and avg_end
    void avg_begin(int moments);
    void avg_sample();
    int64_t avg_samples() const;
    void avg_store_sums(double *const *out);
    void avg_store(float *const *out);
    void avg_end();
    // lbm3d_gradients.hip (include/lbm_gradients_hip.h)
    std::vector<float *> grad_faces;  // per slab: face velocity planes, allocated at the first gradient call
    int grad_prepare();
    void grad_release();
    lbm::grad::Grad3Args grad_args(size_t k, int hp, int x0, int y0, int z0, int bx, int by, int bz) const;
    void store_gradients_box(const lbm3d_box &b, float *const *host);
    void gradient_stats(double *sum_w2, double *sum_s2, float *max_w, float *max_div);
    // lbm3d_stress.hip (include/lbm_stress_hip.h)
    lbm::stress::State3 *stress = nullptr;  // built at the first statistics call
    lbm::stress::Stress3Args stress_args(const lbm::Slab &s, int x0, int y0, int z0, int bx, int by, int bz) const;
    void stress_build();
    void stress_release();
    void store_stress_box(const lbm3d_box &b, float *const *host);
    void stress_stats(double *sum_s2, float *max_strain, int64_t *wall_cells, double *sum_wall_strain,
                      float *max_wall_strain);
    // lbm3d_binned.hip (include/lbm_binned_hip.h)
    void store_binned(int bw, int bh, int bd, double *const *out);
    void bin_fluid_cells(int bw, int bh, int bd, int64_t *count);
    // lbm3d_tracers.hip (include/lbm_tracers_hip.h)
    lbm::tracer::State *tracers = nullptr;  // set between tracer_begin and tracer_end
    void tracer_begin(int64_t n, const double *x, const double *y, const double *z);
    int64_t tracer_count() const;
    void tracer_advance(double dt, int scheme);
    void tracer_sample(double *const (&host)[4]);
    void tracer_store(double *const (&host)[3], uint8_t *blocked);
    void tracer_end();
    // lbm3d_scalar.hip (include/lbm_scalar_hip.h)
    lbm::scalar::State *scalars = nullptr;  // set between scalar_begin and scalar_end
    void scalar_begin(float omega_s, const float *phi0);
    void scalar_set_fixed(int64_t n, const int32_t *x, const int32_t *y, const int32_t *z, const float *value);
    void scalar_advance(int steps);
    int64_t scalar_steps();
    void scalar_store(float *phi, float *g);
    void scalar_stats(double *total, float *min, float *max);
    void scalar_end();
    void scalar_buoyancy(float sx, float sy, float sz, float phi_ref);  // include/lbm_thermal_hip.h
    void scalar_store_binned(int bw, int bh, int bd, double *const *out);  // lbm3d_transport.hip; include/lbm_transport_hip.h
    // lbm3d_scalar_walls.hip (include/lbm_scalar_walls_hip.h)
    std::vector<uint8_t> obst_host() const;
    void scalar_set_walls(const int32_t *labels, int32_t nbodies, const int32_t *kind, const float *value);
    void scalar_wall_flux(double *q, int64_t *links);
    void scalar_body_flux(double *q, int64_t *links, int32_t nbodies);
    void scalar_store_wall_flux(float *q);
    void need_whole_domain(const char *what) const;  // lbm3d_scalar.hip: the restrictions of scalar_begin
    // lbm3d_forcing.hip (include/lbm_forcing_hip.h)
    lbm::forcing::State *forcing = nullptr;  // built at the first zone set
    void forcing_set_zone(int zone, int x0, int y0, int z0, int w, int h, int d, const float *const *coef,
                          const float *konst);
    void forcing_clear();
    void forcing_zones(int32_t *n_set, uint32_t *mask) const;
    void forcing_apply(float steps, double *impulse);
    // lbm3d_sgs.hip (include/lbm_sgs_hip.h)
    lbm::sgs::State *sgs = nullptr;  // built at the first model set
    void sgs_set(int mode, float konst, const float *coef);
    void sgs_clear();
    void sgs_apply(float steps, double *stats);
    void sgs_store_nut(float *nut);
};
