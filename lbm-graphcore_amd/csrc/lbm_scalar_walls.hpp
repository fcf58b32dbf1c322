// lbm_scalar_walls.hpp -- wall models of the passive scalar and the per-body
// wall flux (include/lbm_scalar_walls_hip.h), shared by the D2Q9 engine
// (lbm_scalar_walls.hip, D2Q5) and the D3Q19 engine (lbm3d_scalar_walls.hip,
// D3Q7): the per-cell functions, compiled for the device and for the host from
// one text, the kernels (templates over the number of speeds) and their host
// side.
//
// One wall list covers the whole domain, since the scalar lattice is global:
// forces::WallList (lbm_forces.hpp) with the offset of a wall cell inside a
// scalar plane, its link mask and its index in the planar map, sorted by body
// (row-major inside a body, so a straight wall coalesces; unlabelled cells
// last) and cut into that list's chunks.  Beside it the body of every labelled
// entry and the per-body table (kind, value), which a table-only update
// rewrites without touching the list.
//
// The wall pass: one lane per labelled wall cell, at most Q - 1 loads and
// stores gated by the link bits, plain vector stores, no atomics, no LDS; a
// lane owns its cell.  The flux kernels are those of lbm_forces.hpp with one
// component and the table: the model interface there (populations and mask
// alone) has no way to the body's kind and value, so they are restated here
// over the same list, chunks, partial buffers, fetches and fixed-order folds
// (lanes of a wave by shuffle, a block's waves through LDS, blocks on the
// host; a body's chunks by one wave of a second launch).
//
// Index safety: every offset of the list comes from a cell inside the domain,
// every body index is below nbodies (checked on the host before upload), and
// the kernels touch nothing but list entries i < n.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

#include "lbm_diag_host.hpp"
#include "lbm_forces.hpp"
#include "lbm_scalar.hpp"
#include "lbm_scalar_walls_hip.h"

namespace lbm {
namespace scalar {

#define LBM_HD __host__ __device__ __forceinline__

// ---- the per-cell functions (host and device) ----

// The pass on one wall cell: p its rest population, ks the stride between its populations.
template <int Q>
LBM_HD void wall_apply(float *p, long long ks, unsigned mask, int kind, float v, float w1) {
    if (kind == LBM_SCALAR_WALL_ADIABATIC) return;
    const float m = v * w1;
    const float d = m + m;
#pragma unroll
    for (int k = 1; k < Q; ++k)
        if ((mask >> (k - 1)) & 1u) {
            const float gk = p[k * ks];
            p[k * ks] = kind == LBM_SCALAR_WALL_VALUE ? d - gk : gk + v;
        }
}

// The flux of one wall cell from its stored populations; a population is loaded only where a VALUE link needs it.
template <int Q>
LBM_HD float wall_flux(const float *p, long long ks, unsigned mask, int kind, float v, float w1) {
    const float m = v * w1;
    float t[Q];
#pragma unroll
    for (int k = 1; k < Q; ++k) {
        const bool link = ((mask >> (k - 1)) & 1u) != 0;
        const float gk = (link && kind == LBM_SCALAR_WALL_VALUE) ? p[k * ks] : 0.f;
        const float tv = (gk - m) * 2.f;
        t[k] = !link ? 0.f : kind == LBM_SCALAR_WALL_VALUE ? tv : kind == LBM_SCALAR_WALL_FLUX ? v : 0.f;
    }
    float q = t[1] + t[2];
#pragma unroll
    for (int k = 3; k < Q; ++k) q += t[k];
    return q;
}

// the neighbour of (x, y, z) along moving speed k, periodic: D2Q5 (Q = 5) E N W S, D3Q7 +x -x +y -y +z -z
template <int Q>
inline void wall_neighbour(int k, int &x, int &y, int &z, int nx, int ny, int nz) {
    if (Q == 5) {
        if (k == 1) x = above(x, nx);
        if (k == 2) y = above(y, ny);
        if (k == 3) x = below(x, nx);
        if (k == 4) y = below(y, ny);
    } else {
        if (k == 1) x = above(x, nx);
        if (k == 2) x = below(x, nx);
        if (k == 3) y = above(y, ny);
        if (k == 4) y = below(y, ny);
        if (k == 5) z = above(z, nz);
        if (k == 6) z = below(z, nz);
    }
}

// link mask of cell (x, y, z) of the unpadded map (0 for a fluid cell)
template <int Q>
inline unsigned wall_mask(const uint8_t *obst, int x, int y, int z, int nx, int ny, int nz) {
    if (!obst[((size_t)z * ny + y) * nx + x]) return 0u;
    unsigned m = 0;
    for (int k = 1; k < Q; ++k) {
        int xx = x, yy = y, zz = z;
        wall_neighbour<Q>(k, xx, yy, zz, nx, ny, nz);
        if (!obst[((size_t)zz * ny + yy) * nx + xx]) m |= 1u << (k - 1);
    }
    return m;
}

// ---- what a scalar with walls holds ----

struct BodyRow {
    int kind;
    float value;
};

struct Walls {
    forces::WallList list;      // every wall cell of the domain, in the order described above
    long long nlab = 0;         // the labelled entries: the first nlab of the list
    int nbodies = 0;
    unsigned *body = nullptr;   // [nlab] body of each labelled entry
    BodyRow *tab = nullptr;     // [nbodies]
};

// ---- kernels ----

using forces::WallArgs;
using forces::WBLOCK;

struct FluxArgs {
    WallArgs w;            // o: the current scalar set, ks: its plane stride
    const unsigned *body;  // [nlab]
    const BodyRow *tab;
    long long nlab;
    float w1;
};

template <int Q>
__global__ __launch_bounds__(WBLOCK) void scalar_walls_pass(float *g, long long plane, const long long *off,
                                                            const unsigned *mask, const unsigned *body,
                                                            const BodyRow *tab, long long nlab, float w1) {
    for (long long i = (long long)blockIdx.x * WBLOCK + threadIdx.x; i < nlab; i += (long long)gridDim.x * WBLOCK) {
        const BodyRow r = tab[body[i]];
        wall_apply<Q>(g + off[i], plane, mask[i], r.kind, r.value, w1);
    }
}

template <int Q>
__device__ __forceinline__ float flux_of_entry(const FluxArgs &a, long long i, unsigned m) {
    BodyRow r{LBM_SCALAR_WALL_ADIABATIC, 0.f};
    if (i < a.nlab) r = a.tab[a.body[i]];
    return wall_flux<Q>(a.w.o + a.w.off[i], a.w.ks, m, r.kind, r.value, a.w1);
}

// fixed-order sum over the 64 lanes of a wave: the result is in lane 0
__device__ __forceinline__ void wave_sum1(double &x, long long &links) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        x += __shfl_down(x, d, 64);
        links += __shfl_down(links, d, 64);
    }
}

// per block one partial in the layout WallList::fetch_total reads ([blocks][3] doubles, then the link counts)
template <int Q>
__global__ __launch_bounds__(WBLOCK) void scalar_wall_flux_total(FluxArgs a) {
    double s = 0.0;
    long long links = 0;
    for (long long i = (long long)blockIdx.x * WBLOCK + threadIdx.x; i < a.w.n; i += (long long)gridDim.x * WBLOCK) {
        const unsigned m = a.w.mask[i];
        s += (double)flux_of_entry<Q>(a, i, m);
        links += __popc(m);
    }
    wave_sum1(s, links);
    __shared__ double w[WBLOCK / 64];
    __shared__ long long wl[WBLOCK / 64];
    if ((threadIdx.x & 63) == 0) {
        w[threadIdx.x >> 6] = s;
        wl[threadIdx.x >> 6] = links;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = w[0];
        long long l = wl[0];
        for (int i = 1; i < WBLOCK / 64; ++i) {
            t += w[i];
            l += wl[i];
        }
        a.w.part[3 * blockIdx.x + 0] = t;
        a.w.part[3 * blockIdx.x + 1] = 0.0;
        a.w.part[3 * blockIdx.x + 2] = 0.0;
        a.w.lpart[blockIdx.x] = l;
    }
}

// one wave per chunk: lane l takes cells l, l + 64, ... of the chunk's range (every chunk lies inside a body)
template <int Q>
__global__ __launch_bounds__(WBLOCK) void scalar_wall_flux_chunks(FluxArgs a) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (WBLOCK / 64);
    for (long long c = (long long)blockIdx.x * (WBLOCK / 64) + (threadIdx.x >> 6); c < a.w.nc; c += waves) {
        const unsigned end = a.w.cs[c + 1];
        const unsigned cb = a.w.cbody[c];
        const BodyRow r = a.tab[cb & ~forces::BODY_WHOLE];
        double s = 0.0;
        long long links = 0;
        for (unsigned i = a.w.cs[c] + lane; i < end; i += 64) {
            const unsigned m = a.w.mask[i];
            s += (double)wall_flux<Q>(a.w.o + a.w.off[i], a.w.ks, m, r.kind, r.value, a.w1);
            links += __popc(m);
        }
        wave_sum1(s, links);
        if (lane == 0) {
            const bool whole = (cb & forces::BODY_WHOLE) != 0;
            double *d = whole ? a.w.bsum + 3 * (size_t)(cb & ~forces::BODY_WHOLE) : a.w.csum + 3 * (size_t)c;
            d[0] = s;
            (whole ? a.w.blinks[cb & ~forces::BODY_WHOLE] : a.w.clinks[c]) = links;
        }
    }
}

// one wave per body of several chunks: lane l takes chunk sums l, l + 64, ...
template <int Q>
__global__ __launch_bounds__(WBLOCK) void scalar_wall_flux_fold(FluxArgs a) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (WBLOCK / 64);
    for (long long m = (long long)blockIdx.x * (WBLOCK / 64) + (threadIdx.x >> 6); m < a.w.nm; m += waves) {
        const unsigned b = a.w.mtab[3 * m], end = a.w.mtab[3 * m + 2];
        double s = 0.0;
        long long links = 0;
        for (unsigned c = a.w.mtab[3 * m + 1] + lane; c < end; c += 64) {
            s += a.w.csum[3 * (size_t)c];
            links += a.w.clinks[c];
        }
        wave_sum1(s, links);
        if (lane == 0) {
            a.w.bsum[3 * (size_t)b] = s;
            a.w.blinks[b] = links;
        }
    }
}

// the wall cells scattered into the zeroed planar map a.w.mx
template <int Q>
__global__ __launch_bounds__(WBLOCK) void scalar_wall_flux_map(FluxArgs a) {
    for (long long i = (long long)blockIdx.x * WBLOCK + threadIdx.x; i < a.w.n; i += (long long)gridDim.x * WBLOCK)
        a.w.mx[a.w.cell[i]] = flux_of_entry<Q>(a, i, a.w.mask[i]);
}

// ---- host side both engines share ----

inline void check_table(int32_t nbodies, const int32_t *kind, const float *value) {
    if (nbodies < 1 || !kind || !value) throw lbm_failure(LBM_E_INVALID, "scalar walls need nbodies >= 1, kinds and values");
    for (int32_t b = 0; b < nbodies; ++b) {
        if (kind[b] < LBM_SCALAR_WALL_ADIABATIC || kind[b] > LBM_SCALAR_WALL_FLUX)
            throw lbm_failure(LBM_E_INVALID, "wall kind of body " + std::to_string(b) + " is none of 0, 1, 2");
        if (!std::isfinite(value[b]))
            throw lbm_failure(LBM_E_INVALID, "wall value of body " + std::to_string(b) + " is not finite");
    }
}

inline std::vector<BodyRow> table_of(int32_t nbodies, const int32_t *kind, const float *value) {
    std::vector<BodyRow> t((size_t)nbodies);
    for (int32_t b = 0; b < nbodies; ++b) t[(size_t)b] = BodyRow{kind[b], value[b]};
    return t;
}

// lbm_scalar_set_walls / lbm3d_scalar_set_walls behind the engine's checks; obst() gives the unpadded obstacle
// map of the whole domain and is called only when a list is built.
template <int Q, class ObstFn>
void set_walls(State &s, const int32_t *labels, int32_t nbodies, const int32_t *kind, const float *value,
               ObstFn &&obst) {
    HIP_CHECK(hipSetDevice(s.dev));
    if (!labels) {
        if (nbodies == 0 && !kind && !value) {  // clear
            walls_free(s.walls);
            s.walls = nullptr;
            return;
        }
        if (!s.walls || nbodies < 1 || nbodies != s.walls->nbodies)
            throw lbm_failure(LBM_E_INVALID, "NULL labels: nbodies must equal the count of the walls set (or all be 0 / NULL)");
        check_table(nbodies, kind, value);
        const std::vector<BodyRow> t = table_of(nbodies, kind, value);  // the table alone; the list stays
        HIP_CHECK(hipMemcpy(s.walls->tab, t.data(), sizeof(BodyRow) * t.size(), hipMemcpyHostToDevice));
        return;
    }
    check_table(nbodies, kind, value);
    const Grid &gr = s.grid;
    const long long cells = (long long)gr.nx * gr.ny * gr.nz;
    if (cells > (long long)INT_MAX) throw lbm_failure(LBM_E_INVALID, "domain too large for a scalar wall list");
    const std::vector<uint8_t> ob = obst();
    for (long long c = 0; c < cells; ++c)
        if (ob[(size_t)c] && labels[c] >= nbodies) throw lbm_failure(LBM_E_INVALID, "label >= nbodies on a blocked cell");
    // wall cells row-major, then stably by body (unlabelled last)
    std::vector<unsigned> cell, mask;
    std::vector<int> body;
    for (int z = 0; z < gr.nz; ++z)
        for (int y = 0; y < gr.ny; ++y)
            for (int x = 0; x < gr.nx; ++x) {
                const unsigned m = wall_mask<Q>(ob.data(), x, y, z, gr.nx, gr.ny, gr.nz);
                if (!m) continue;
                const size_t c = ((size_t)z * gr.ny + y) * gr.nx + x;
                cell.push_back((unsigned)c);
                mask.push_back(m);
                body.push_back(labels[c] < 0 ? -1 : labels[c]);
            }
    std::vector<size_t> order(cell.size());
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
        return (unsigned)body[a] < (unsigned)body[b];  // -1 sorts last
    });
    Walls *w = new Walls;
    try {
        w->list.dims = Q == 5 ? 2 : 3;
        std::vector<unsigned> hbody;
        for (size_t i : order) {
            const unsigned c = cell[i];
            const unsigned x = c % (unsigned)gr.nx, row = c / (unsigned)gr.nx;
            w->list.add((long long)row * gr.sp + x, c, mask[i]);
            w->list.h_body.push_back(body[i]);
            if (body[i] >= 0) hbody.push_back((unsigned)body[i]);
        }
        HIP_CHECK(w->list.upload(nbodies));  // already in its order: the stable counting sort there keeps it
        w->nlab = (long long)hbody.size();
        w->nbodies = nbodies;
        if (w->nlab > 0) {
            HIP_CHECK(hipMalloc((void **)&w->body, sizeof(unsigned) * hbody.size()));
            HIP_CHECK(hipMemcpy(w->body, hbody.data(), sizeof(unsigned) * hbody.size(), hipMemcpyHostToDevice));
        }
        const std::vector<BodyRow> t = table_of(nbodies, kind, value);
        HIP_CHECK(hipMalloc((void **)&w->tab, sizeof(BodyRow) * t.size()));
        HIP_CHECK(hipMemcpy(w->tab, t.data(), sizeof(BodyRow) * t.size(), hipMemcpyHostToDevice));
    } catch (...) {
        walls_free(w);
        throw;
    }
    walls_free(s.walls);
    s.walls = w;
}

// the pass on set g of the state (inside advance, between the step and the fixed list)
template <int Q>
hipError_t launch_pass(const State &s, float *g, hipStream_t st) {
    const Walls *w = s.walls;
    if (!w || w->nlab == 0) return hipSuccess;
    hipLaunchKernelGGL(scalar_walls_pass<Q>, dim3(forces::wall_blocks(w->nlab)), dim3(WBLOCK), 0, st, g, s.grid.plane,
                       w->list.off, w->list.mask, w->body, w->tab, w->nlab, s.w1);
    return hipGetLastError();
}

inline FluxArgs flux_args(const State &s) {
    const Walls &w = *s.walls;
    return FluxArgs{w.list.args(s.g[s.cur], s.grid.plane), w.body, w.tab, w.nlab, s.w1};
}

template <int Q, class Around>
void wall_flux_total(const State &s, hipStream_t st, double *q, int64_t *links, Around &&around) {
    double f[3] = {0.0, 0.0, 0.0};
    long long nl = 0;
    if (s.walls && s.walls->list.n > 0) {
        HIP_CHECK(hipSetDevice(s.dev));
        const FluxArgs a = flux_args(s);
        around([&] {
            hipLaunchKernelGGL(scalar_wall_flux_total<Q>, dim3(forces::wall_blocks(a.w.n)), dim3(WBLOCK), 0, st, a);
            HIP_CHECK(hipGetLastError());
        });
        HIP_CHECK(s.walls->list.fetch_total(st, f, nl));  // blocks in order
    }
    if (q) *q = f[0];
    if (links) *links = nl;
}

template <int Q, class Around>
void wall_flux_bodies(const State &s, hipStream_t st, double *q, int64_t *links, int32_t nbodies, Around &&around) {
    if (!s.walls || s.walls->nbodies != nbodies)
        throw lbm_failure(LBM_E_STATE, "scalar body flux: no walls set, or set with another nbodies");
    for (int b = 0; b < nbodies; ++b) {
        if (q) q[b] = 0.0;
        if (links) links[b] = 0;
    }
    const forces::WallList &wl = s.walls->list;
    if (wl.n == 0 || !wl.bpart) return;  // a body without wall cells has no chunk: its sums stay zero
    HIP_CHECK(hipSetDevice(s.dev));
    const FluxArgs a = flux_args(s);
    HIP_CHECK(hipMemsetAsync(wl.bpart, 0, (3 * sizeof(double) + sizeof(long long)) * (size_t)nbodies, st));
    around([&] {
        if (a.w.nc > 0)
            hipLaunchKernelGGL(scalar_wall_flux_chunks<Q>, dim3(forces::body_blocks(a.w.nc)), dim3(WBLOCK), 0, st, a);
        if (a.w.nm > 0)
            hipLaunchKernelGGL(scalar_wall_flux_fold<Q>, dim3(forces::body_blocks(a.w.nm)), dim3(WBLOCK), 0, st, a);
        HIP_CHECK(hipGetLastError());
    });
    HIP_CHECK(wl.fetch_bodies(st, q, nullptr, nullptr, links));
}

// the planar map float[nz][ny][nx]
template <int Q, class Around>
void wall_flux_store(const State &s, hipStream_t st, float *q, Around &&around) {
    if (!q) return;
    const Grid &gr = s.grid;
    const size_t cells = (size_t)gr.nx * gr.ny * gr.nz;
    if (!s.walls || s.walls->list.n == 0) {
        std::fill(q, q + cells, 0.f);
        return;
    }
    HIP_CHECK(hipSetDevice(s.dev));
    FluxArgs a = flux_args(s);
    const PlanarStage stage(1, cells);
    HIP_CHECK(hipMemsetAsync(stage.get(), 0, stage.bytes(), st));
    a.w.mx = stage.field(0);
    around([&] {
        hipLaunchKernelGGL(scalar_wall_flux_map<Q>, dim3(forces::wall_blocks(a.w.n)), dim3(WBLOCK), 0, st, a);
        HIP_CHECK(hipGetLastError());
    });
    HIP_CHECK(hipStreamSynchronize(st));
    float *const host[1] = {q};
    stage.copy_out(host, 1, HostSpan{0, (size_t)gr.nx}, (size_t)gr.nx, (size_t)gr.nx, (size_t)gr.ny * gr.nz);
}

// the *_walls_ref entry points
template <int Q>
int walls_ref(int nx, int ny, int nz, const uint8_t *obst, const int32_t *labels, int32_t nbodies,
              const int32_t *kind, const float *value, float *g, float *q) {
    if (nx < 1 || ny < 1 || nz < 1 || nbodies < 1 || !obst || !labels || !kind || !value || !g) return LBM_E_INVALID;
    const size_t plane = (size_t)nx * ny * nz;
    for (int32_t b = 0; b < nbodies; ++b)
        if (kind[b] < LBM_SCALAR_WALL_ADIABATIC || kind[b] > LBM_SCALAR_WALL_FLUX || !std::isfinite(value[b]))
            return LBM_E_INVALID;
    for (size_t c = 0; c < plane; ++c)
        if (obst[c] && labels[c] >= nbodies) return LBM_E_INVALID;
    const float w1 = Q == 5 ? 1.f / 6.f : 0.125f;
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const size_t c = ((size_t)z * ny + y) * nx + x;
                const unsigned m = wall_mask<Q>(obst, x, y, z, nx, ny, nz);
                const bool on = m != 0 && labels[c] >= 0;
                const int k = on ? kind[labels[c]] : LBM_SCALAR_WALL_ADIABATIC;
                const float v = on ? value[labels[c]] : 0.f;
                wall_apply<Q>(g + c, (long long)plane, m, k, v, w1);
                if (q) q[c] = wall_flux<Q>(g + c, (long long)plane, m, k, v, w1);
            }
    return LBM_OK;
}

#undef LBM_HD

}  // namespace scalar
}  // namespace lbm
