// lbm_gradients.hip -- vorticity, divergence, strain rate and the Q criterion
// of the D2Q9 engine on the device (the lbm_* functions of
// include/lbm_gradients_hip.h): central differences of the velocities
// lbm_store_fields gives, without moving a field to the host.  The kernels,
// then the engine's host side.
//
// The first derived quantity that needs a cell's neighbours.  Inside a
// sub-domain they come from the lattice itself; across its four sides they
// come from velocities, never from the lattice's ghost ring (whose content
// depends on the step kernel in use and may be stale): edge_velocities writes
// (ux, uy) of each sub-domain's outermost rows and columns, and side d then
// receives out[OPP_DIR[d]] of nb[d] by a device copy -- the periodic
// self-image is the same path with nb[d] the sub-domain itself.
//
// velocity_gradients: one memory-bound pass over the nine populations of the
// current side of the pair (origin / plane / pitch, either layout).  A wave
// owns a strip of 248 columns and a segment of 32 rows; a lane takes four
// consecutive cells (nine 16-B loads per row, lbm_quad.hpp), keeps
// the velocities of three rows in registers (24 VGPRs) and gets the
// x-neighbours of its outer cells from the adjacent lanes.  Lanes 0 and 63
// and one row each side of the segment only supply neighbours: 256 x 34 cells
// read for 248 x 32 owned, under 10 % redundant.  No LDS but the statistics'
// fold.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "lbm_cell_macro.hpp"
#include "lbm_engine.hpp"
#include "lbm_gradients.hpp"
#include "lbm_gradients_hip.h"
#include "lbm_packed.hpp"
#include "lbm_quad.hpp"

namespace lbm {
namespace grad {

namespace {

struct Row {
    float ux[4], uy[4];
    unsigned blocked;  // bit i: cell i is an obstacle (rows of the lattice only)
};

__device__ __forceinline__ void cell_velocity(const float (&c)[Q], bool blocked, float obst_pressure, float &ux,
                                              float &uy) {
    float rho;
    const CellMacro m = cell_macro<true, false>(c, blocked, obst_pressure, rho);
    ux = m.ux;
    uy = m.uy;
}

// The velocities of cells x .. x + 3 of row y (-1 <= y <= h; x a multiple of
// 4, -4 <= x): lattice cells from their populations, column -1 / w and row
// -1 / h from the edge velocities across that side, anything beyond +0.
__device__ __forceinline__ void load_row(const GradArgs &a, int x, int y, Row &r) {
    const EdgeLayout el{a.w, a.h};
#pragma unroll
    for (int i = 0; i < 4; ++i) r.ux[i] = r.uy[i] = 0.f;
    r.blocked = 0;
    if (y < 0 || y >= a.h) {
        const float *e = a.in + el.off(y < 0 ? DS : DN);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x + i >= 0 && x + i < a.w) {
                r.ux[i] = e[x + i];
                r.uy[i] = e[a.w + x + i];
            }
        return;
    }
    const float *src = a.o + (long long)y * a.pitch + x;
    const uint8_t *ob = a.obst + (long long)y * a.w + x;
    if (x >= 0 && x + 4 <= a.w) {
        float4 v[Q];
        load_quad<Q>(src, a.plane, v);
        const unsigned bits = quad_map_bytes(ob, (a.w & 3) == 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float c[Q];
            quad_cell<Q>(v, i, c);
            const bool blocked = ((bits >> (8 * i)) & 0xffu) != 0;
            if (blocked) r.blocked |= 1u << i;
            cell_velocity(c, blocked, a.obst_pressure, r.ux[i], r.uy[i]);
        }
        return;
    }
    // the quad straddles the west or east border, or holds the ragged tail of the row
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int xc = x + i;
        if (xc == -1 || xc == a.w) {
            const float *e = a.in + el.off(xc < 0 ? DW : DE);
            r.ux[i] = e[y];
            r.uy[i] = e[a.h + y];
        } else if (xc >= 0 && xc < a.w) {
            float c[Q];
            load_cell<Q>(src, a.plane, i, c);
            const bool blocked = ob[i] != 0;
            if (blocked) r.blocked |= 1u << i;
            cell_velocity(c, blocked, a.obst_pressure, r.ux[i], r.uy[i]);
        }
    }
}

}  // namespace

// (ux, uy) of the sub-domain's outermost column / row of each side into
// a.edge_out: item j of 2 h + 2 w runs over sides E, N, W, S in turn.
__global__ __launch_bounds__(BLOCK) void edge_velocities(GradArgs a) {
    const EdgeLayout el{a.w, a.h};
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= 2 * a.h + 2 * a.w) return;
    int d, i;
    if (j < a.h) {
        d = DE, i = j;
    } else if (j < a.h + a.w) {
        d = DN, i = j - a.h;
    } else if (j < 2 * a.h + a.w) {
        d = DW, i = j - a.h - a.w;
    } else {
        d = DS, i = j - 2 * a.h - a.w;
    }
    const int x = d == DE ? a.w - 1 : d == DW ? 0 : i;
    const int y = d == DN ? a.h - 1 : d == DS ? 0 : i;
    const float *src = a.o + (long long)y * a.pitch + x;
    float c[Q];
    load_cell<Q>(src, a.plane, 0, c);
    float ux, uy;
    cell_velocity(c, a.obst[(long long)y * a.w + x] != 0, a.obst_pressure, ux, uy);
    float *e = a.edge_out + el.off(d);
    e[i] = ux;
    e[el.len(d) + i] = uy;
}

// STATS: no field is stored; block b writes its partial sums and maxima over
// the fluid cells it owns (fold_block, lbm_quad.hpp).
template <bool STATS>
__global__ __launch_bounds__(BLOCK) void velocity_gradients(GradArgs a) {
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    double sw2 = 0.0, ss2 = 0.0;
    float mw = 0.f, md = 0.f;
    if (item < (long long)a.strips * a.segs) {  // the same for every lane of the wave
        const int strip = (int)(item % a.strips), seg = (int)(item / a.strips);
        const int x = (strip * GR_OWN_Q + lane - 1) * 4;
        const int y0 = seg * GR_SEG, y1 = min(y0 + GR_SEG, a.h);
        const bool own = lane >= 1 && lane <= GR_OWN_Q && x < a.w;
        Row p, c, n;
        load_row(a, x, y0 - 1, p);
        load_row(a, x, y0, c);
        for (int y = y0; y < y1; ++y) {
            load_row(a, x, y + 1, n);
            // the x-neighbours of the lane's outer cells: the adjacent lanes' inner ones
            // (DPP wave shifts, as the stream kernel's: one v_mov_dpp each, no LDS crossbar)
            const float uw = dpp_from_left(c.ux[3]), vw = dpp_from_left(c.uy[3]);
            const float ue = dpp_from_right(c.ux[0]), ve = dpp_from_right(c.uy[0]);
            if (own) {
                Grad2 g[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    g[i] = gradients2(i < 3 ? c.ux[i + 1] : ue, i > 0 ? c.ux[i - 1] : uw, n.ux[i], p.ux[i],
                                      i < 3 ? c.uy[i + 1] : ve, i > 0 ? c.uy[i - 1] : vw, n.uy[i], p.uy[i]);
                    const bool fluid = x + i < a.w && !((c.blocked >> i) & 1u);
                    if (!fluid) g[i] = Grad2{0.f, 0.f, 0.f, 0.f, 0.f};
                    if (STATS && fluid) {
                        sw2 += (double)g[i].vorticity * (double)g[i].vorticity;
                        ss2 += (double)g[i].s2;
                        mw = fmaxf(mw, fabsf(g[i].vorticity));
                        md = fmaxf(md, fabsf(g[i].divergence));
                    }
                }
                if (!STATS) {
                    const long long so = (long long)y * a.sp + x;  // rows padded to 4 floats: the whole quad fits
                    if (a.out[0])
                        *reinterpret_cast<float4 *>(a.out[0] + so) =
                            make_float4(g[0].vorticity, g[1].vorticity, g[2].vorticity, g[3].vorticity);
                    if (a.out[1])
                        *reinterpret_cast<float4 *>(a.out[1] + so) =
                            make_float4(g[0].divergence, g[1].divergence, g[2].divergence, g[3].divergence);
                    if (a.out[2])
                        *reinterpret_cast<float4 *>(a.out[2] + so) =
                            make_float4(g[0].strain, g[1].strain, g[2].strain, g[3].strain);
                    if (a.out[3]) *reinterpret_cast<float4 *>(a.out[3] + so) = make_float4(g[0].q, g[1].q, g[2].q, g[3].q);
                }
            }
            p = c;
            c = n;
        }
    }
    if (STATS) {
        double s[2] = {sw2, ss2};
        float m[2] = {mw, md};
        fold_block<BLOCK / 64>(s, m, blockIdx.x, gridDim.x, a.sum_part, a.max_part);
    }
}

int gradient_strips(int w) { return ((w + 3) / 4 + GR_OWN_Q - 1) / GR_OWN_Q; }
int gradient_segs(int h) { return (h + GR_SEG - 1) / GR_SEG; }

// blocks of a launch over w x h: also the partials a stats launch writes
int gradient_blocks(int w, int h) {
    const long long items = (long long)gradient_strips(w) * gradient_segs(h);
    return (int)((items + BLOCK / 64 - 1) / (BLOCK / 64));
}

hipError_t launch_edge_velocities(const GradArgs &a, hipStream_t s) {
    const int items = 2 * a.h + 2 * a.w;
    hipLaunchKernelGGL(edge_velocities, dim3((items + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_velocity_gradients(const GradArgs &a, bool stats, hipStream_t s) {
    const int blocks = gradient_blocks(a.w, a.h);
    if (stats)
        hipLaunchKernelGGL(velocity_gradients<true>, dim3(blocks), dim3(BLOCK), 0, s, a);
    else
        hipLaunchKernelGGL(velocity_gradients<false>, dim3(blocks), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

// edge buffers of a handle that asked for gradients: per local sub-domain
// [out | in], EdgeLayout::total() floats each, on the sub-domain's device
struct State {
    std::vector<float *> edge;
};

}  // namespace grad
}  // namespace lbm

// ---- D2Q9 engine: host side ----

using lbm::grad::EdgeLayout;
using lbm::grad::GradArgs;

// Allocates the edge buffers at the first call, then brings the velocities
// across every side of every local sub-domain into its `in` buffer and
// returns the kernel arguments per sub-domain.  Ends synchronised.
std::vector<GradArgs> lbm_handle::grad_prepare() {
    if (transport == LBM_TRANSPORT_RCCL && world > 1)
        throw lbm_failure(LBM_E_INVALID,
                          "velocity gradients are not built for RCCL handles of world size > 1: the neighbours' "
                          "edge velocities live in other processes");
    if (!gradients) {
        auto *st = new grad::State();
        gradients = st;
        st->edge.assign(subs.size(), nullptr);
        for (size_t k = 0; k < subs.size(); ++k) {
            set_device(subs[k]);
            const EdgeLayout el{subs[k].w, subs[k].h};
            HIP_CHECK(hipMalloc(&st->edge[k], sizeof(float) * 2 * (size_t)el.total()));
        }
    }
    std::vector<GradArgs> args(subs.size());
    for (size_t k = 0; k < subs.size(); ++k) {
        const Sub &s = subs[k];
        set_device(s);
        const EdgeLayout el{s.w, s.h};
        GradArgs a{lattice_view(s)};
        a.edge_out = gradients->edge[k];
        a.in = gradients->edge[k] + el.total();
        a.strips = grad::gradient_strips(s.w);
        a.segs = grad::gradient_segs(s.h);
        args[k] = a;
        timed(s, s.s_comp, "edge_velocities", [&] { HIP_CHECK(grad::launch_edge_velocities(a, s.s_comp)); });
    }
    for (const auto &s : subs) {
        set_device(s);
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
    }
    for (size_t k = 0; k < subs.size(); ++k) {
        const Sub &s = subs[k];
        set_device(s);
        const EdgeLayout el{s.w, s.h};
        for (int d = 0; d < 4; ++d) {
            const Sub *src = local_sub(s.nb[d]);
            if (!src) throw lbm_failure(LBM_E_INTERNAL, "missing local neighbour");
            const EdgeLayout sl{src->w, src->h};
            if (sl.len(d) != el.len(d)) throw lbm_failure(LBM_E_INTERNAL, "neighbour edge length mismatch");
            const float *from = gradients->edge[(size_t)(src - subs.data())] + sl.off(OPP_DIR[d]);
            float *to = gradients->edge[k] + el.total() + el.off(d);
            const size_t bytes = sizeof(float) * 2 * (size_t)el.len(d);
            if (src->dev == s.dev)
                HIP_CHECK(hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToDevice, s.s_comp));
            else
                HIP_CHECK(hipMemcpyPeerAsync(to, s.dev, from, src->dev, bytes, s.s_comp));
        }
    }
    for (const auto &s : subs) {
        set_device(s);
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
    }
    return args;
}

void lbm_handle::grad_release() {
    if (!gradients) return;
    for (size_t k = 0; k < gradients->edge.size() && k < subs.size(); ++k)
        if (gradients->edge[k] && hipSetDevice(subs[k].dev) == hipSuccess) (void)hipFree(gradients->edge[k]);
    delete gradients;
    gradients = nullptr;
}

// vorticity, divergence, strain, q of the current lattice into planar host
// arrays (out[LBM_GRAD_*]; layout rules of store_fields).  A NULL entry is
// neither stored nor staged.
void lbm_handle::store_gradients(float *const *out, bool local) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to derive gradients from");
    const int want = count_wanted(out, LBM_GRAD_FIELDS);
    if (want == 0) return;
    sync_all();
    prof_drop();
    std::vector<GradArgs> args = grad_prepare();
    size_t packed = 0;  // local: cells of the sub-domains before this one
    for (size_t k = 0; k < subs.size(); ++k) {
        const Sub &s = subs[k];
        set_device(s);
        GradArgs &a = args[k];
        const PlanarStage stage(want, (size_t)a.sp * s.h);
        for (int i = 0, n = 0; i < LBM_GRAD_FIELDS; ++i)
            if (out[i]) a.out[i] = stage.field(n++);
        timed(s, s.s_comp, "velocity_gradients", [&] { HIP_CHECK(grad::launch_velocity_gradients(a, false, s.s_comp)); });
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        stage.copy_out(out, LBM_GRAD_FIELDS, host_span(s, local, packed), (size_t)a.sp, (size_t)s.w, (size_t)s.h);
        packed += (size_t)s.w * s.h;
    }
    prof_collect();
}

// Sums of vorticity^2 and S:S (fp64) and the largest |vorticity| and
// |divergence| over the local fluid cells, from the kernel's per-block
// partials (BlockPartials, lbm_diag_host.hpp).
void lbm_handle::gradient_stats(double *sum_w2, double *sum_s2, float *max_w, float *max_div) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take statistics of");
    if (!sum_w2 && !sum_s2 && !max_w && !max_div) return;
    sync_all();
    prof_drop();
    std::vector<GradArgs> args = grad_prepare();
    double sum[2] = {0.0, 0.0};  // w2, s2
    float max[2] = {0.f, 0.f};   // |vorticity|, |divergence|
    for (size_t k = 0; k < subs.size(); ++k) {
        const Sub &s = subs[k];
        set_device(s);
        GradArgs &a = args[k];
        const BlockPartials<2, 2> part((size_t)grad::gradient_blocks(s.w, s.h));
        a.sum_part = part.sums();
        a.max_part = part.maxima();
        timed(s, s.s_comp, "velocity_gradients stats",
              [&] { HIP_CHECK(grad::launch_velocity_gradients(a, true, s.s_comp)); });
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        part.fold(sum, max);
    }
    prof_collect();
    if (sum_w2) *sum_w2 = sum[0];
    if (sum_s2) *sum_s2 = sum[1];
    if (max_w) *max_w = max[0];
    if (max_div) *max_div = max[1];
}
