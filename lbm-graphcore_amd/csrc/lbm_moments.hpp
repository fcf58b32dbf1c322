// lbm_moments.hpp -- time-averaged fields on the device
// (include/lbm_averages_hip.h): the accumulate and derive kernels and the
// host side both engines share.  lbm_averages.hip (D2Q9) and
// lbm3d_averages.hip (D3Q19) instantiate them with their lattice's cell
// expressions (lbm_cell_macro.hpp / lbm3d_cell_macro.hpp: the definitions the
// fields kernels compile) and describe their sub-domains / slabs as Parts.
//
// Field order (the enums of the public header): NV velocity components, p,
// then the pairs u_i u_j (i <= j, i outer) and p p.
//
// accumulate_moments is memory-bound: per cell and sample it reads the Q
// populations and the obstacle byte (37 B / 77 B) and reads and writes 8 B of
// every accumulator: 85 B (MEAN) or 149 B (MEAN|SECOND) for D2Q9, 141 B or
// 253 B for D3Q19.  One lane takes four consecutive cells of a row by the
// access path of lbm_quad.hpp: Q 16-B loads, the obstacle word, and per field
// 32 contiguous, 32-B aligned accumulator bytes (two 16-B loads, two 16-B
// stores).  No atomics, no LDS: every accumulator has one owner lane.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <vector>

#include "lbm_diag_host.hpp"
#include "lbm_quad.hpp"

namespace lbm {

int fields_blocks(int w, int h);  // lbm_fields.hip: blocks of a grid-stride launch over w x h cells, four per lane

namespace avg {

constexpr int MAX_FIELDS = 11;
constexpr int AVG_BLOCK = 256;  // 4 wave64s, the fields launch's block

constexpr int first_fields(int nv) { return nv + 1; }
constexpr int all_fields(int nv) { return nv + 1 + nv * (nv + 1) / 2 + 1; }

// Row r of a part is row r % ny of plane r / ny (D2Q9: one plane of h rows).
struct MomentArgs {
    const float *o;        // lattice origin: cell (0, 0) of plane 0, current side of the pair
    const uint8_t *obst;   // uint8[rows][w]
    long long PL, KS;      // plane stride (D2Q9: unused), speed stride (floats)
    int pitch;             // row pitch (floats)
    int w, ny, rows, sp;   // sp = roundup(w, 4): accumulator row pitch (doubles)
    float obst_pressure;   // sample of an obstacle cell's pressure: density * (1/3)
    double *acc;           // [fields][rows][sp]
    long long fstride;     // rows * sp
};

// T: Q, NV and sample(c, blocked, obst_pressure, m): m[0 .. NV-1] = u, m[NV] = p
template <class T, bool SECOND>
__device__ __forceinline__ void add_cell(const float (&m)[T::NV + 1], double *acc, long long fstride) {
    constexpr int NV = T::NV;
    double d[NV + 1];
#pragma unroll
    for (int i = 0; i <= NV; ++i) {
        d[i] = (double)m[i];
        acc[i * fstride] += d[i];
    }
    if (SECOND) {
        int f = NV + 1;
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
            for (int j = i; j < NV; ++j) acc[(f++) * fstride] += d[i] * d[j];
        acc[f * fstride] += d[NV] * d[NV];
    }
}

__device__ __forceinline__ void add_quad(double *p, double v0, double v1, double v2, double v3) {
    double2 lo = reinterpret_cast<double2 *>(p)[0], hi = reinterpret_cast<double2 *>(p)[1];
    lo.x += v0;
    lo.y += v1;
    hi.x += v2;
    hi.y += v3;
    reinterpret_cast<double2 *>(p)[0] = lo;
    reinterpret_cast<double2 *>(p)[1] = hi;
}

template <class T, bool SECOND>
__global__ __launch_bounds__(AVG_BLOCK) void accumulate_moments(MomentArgs a) {
    constexpr int Q = T::Q, NV = T::NV;
    const int qpr = (a.w + 3) >> 2;  // lanes' quads per row
    const long long total = (long long)qpr * a.rows;
    const bool obst_word = (a.w & 3) == 0;  // every quad's four obstacle bytes are one aligned word
    for (long long q = (long long)blockIdx.x * AVG_BLOCK + threadIdx.x; q < total;
         q += (long long)gridDim.x * AVG_BLOCK) {
        const int r = (int)(q / qpr);
        const int x = (int)(q - (long long)r * qpr) << 2;
        const int z = r / a.ny, y = r - z * a.ny;
        const float *src = a.o + z * a.PL + (long long)y * a.pitch + x;
        const uint8_t *ob = a.obst + (long long)r * a.w + x;
        double *acc = a.acc + (long long)r * a.sp + x;
        if (x + 4 <= a.w) {
            float4 v[Q];
            load_quad<Q>(src, a.KS, v);
            const unsigned bits = quad_map_bytes(ob, obst_word);
            double d[4][NV + 1];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float c[Q], m[NV + 1];
                quad_cell<Q>(v, i, c);
                T::sample(c, ((bits >> (8 * i)) & 0xffu) != 0, a.obst_pressure, m);
#pragma unroll
                for (int f = 0; f <= NV; ++f) d[i][f] = (double)m[f];
            }
#pragma unroll
            for (int f = 0; f <= NV; ++f) add_quad(acc + f * a.fstride, d[0][f], d[1][f], d[2][f], d[3][f]);
            if (SECOND) {
                int f = NV + 1;
#pragma unroll
                for (int i = 0; i < NV; ++i)
#pragma unroll
                    for (int j = i; j < NV; ++j)
                        add_quad(acc + (f++) * a.fstride, d[0][i] * d[0][j], d[1][i] * d[1][j], d[2][i] * d[2][j],
                                 d[3][i] * d[3][j]);
                add_quad(acc + f * a.fstride, d[0][NV] * d[0][NV], d[1][NV] * d[1][NV], d[2][NV] * d[2][NV],
                         d[3][NV] * d[3][NV]);
            }
        } else {
            // ragged tail of a row: the last w % 4 cells, one at a time
            for (int i = 0; x + i < a.w; ++i) {
                float c[Q], m[NV + 1];
                load_cell<Q>(src, a.KS, i, c);
                T::sample(c, ob[i] != 0, a.obst_pressure, m);
                add_cell<T, SECOND>(m, acc + i, a.fstride);
            }
        }
    }
}

// Output field f of moment_means: a first moment (ab < 0) S_a / n, or the
// central moment S_ab / n - (S_a / n) (S_b / n); null out: not derived.
struct MeansArgs {
    const double *acc;
    long long fstride;   // doubles per accumulator = floats per staging array (rows * sp)
    double n;            // the sample count
    float *out[MAX_FIELDS];
    int a[MAX_FIELDS], b[MAX_FIELDS], ab[MAX_FIELDS];
};

// four consecutive entries per lane (fstride is a multiple of 4): 16-B loads, one 16-B store per field
// (a template only so that both engines' units may instantiate it)
template <class T>
__global__ __launch_bounds__(AVG_BLOCK) void moment_means(MeansArgs m) {
    const long long quads = m.fstride >> 2;
    for (long long q = (long long)blockIdx.x * AVG_BLOCK + threadIdx.x; q < quads;
         q += (long long)gridDim.x * AVG_BLOCK) {
        const long long e = q << 2;
#pragma unroll 1
        for (int f = 0; f < MAX_FIELDS; ++f) {
            if (!m.out[f]) continue;
            const double2 *sa = reinterpret_cast<const double2 *>(m.acc + m.a[f] * m.fstride + e);
            const double2 a0 = sa[0], a1 = sa[1];
            const double ma[4] = {a0.x / m.n, a0.y / m.n, a1.x / m.n, a1.y / m.n};
            float4 r;
            if (m.ab[f] < 0) {
                r = make_float4((float)ma[0], (float)ma[1], (float)ma[2], (float)ma[3]);
            } else {
                const double2 *sb = reinterpret_cast<const double2 *>(m.acc + m.b[f] * m.fstride + e);
                const double2 *sab = reinterpret_cast<const double2 *>(m.acc + m.ab[f] * m.fstride + e);
                const double2 b0 = sb[0], b1 = sb[1], p0 = sab[0], p1 = sab[1];
                const double mb[4] = {b0.x / m.n, b0.y / m.n, b1.x / m.n, b1.y / m.n};
                const double mp[4] = {p0.x / m.n, p0.y / m.n, p1.x / m.n, p1.y / m.n};
                r = make_float4((float)(mp[0] - ma[0] * mb[0]), (float)(mp[1] - ma[1] * mb[1]),
                                (float)(mp[2] - ma[2] * mb[2]), (float)(mp[3] - ma[3] * mb[3]));
            }
            *reinterpret_cast<float4 *>(m.out[f] + e) = r;
        }
    }
}

// ---- host side ----

// one sub-domain / slab of a handle: rows of w cells, contiguous in the
// caller's full-domain arrays from host_off with a pitch of host_pitch entries
struct Part {
    int dev = 0;
    hipStream_t st = nullptr;  // the part's compute stream
    int w = 0, rows = 0, sp = 0;
    size_t host_off = 0, host_pitch = 0;
    double *acc = nullptr;     // [nf][rows][sp]
    long long fstride() const { return (long long)rows * sp; }
};

struct State {
    int nv = 0;         // velocity components of the engine
    int moments = 0;    // LBM_AVG_MEAN or LBM_AVG_MEAN | LBM_AVG_SECOND
    int nf = 0;         // accumulators per cell
    int64_t n = 0;      // samples taken
    std::vector<Part> parts;

    void release() {
        for (auto &p : parts)
            if (p.acc && hipSetDevice(p.dev) == hipSuccess) (void)hipFree(p.acc);
        parts.clear();
    }
};

// (a, b, ab) accumulator indices of output field f (ab < 0: a first moment)
inline void field_sums(int nv, int f, int &a, int &b, int &ab) {
    a = b = f;
    ab = -1;
    if (f <= nv) return;
    int g = nv + 1;
    for (int i = 0; i < nv; ++i)
        for (int j = i; j < nv; ++j, ++g)
            if (g == f) {
                a = i;
                b = j;
                ab = f;
                return;
            }
    a = b = nv;  // p p
    ab = f;
}

// begin: zeroed accumulators of `moments` for the parts (acc null on entry)
// in the handle's slot.  Invalid moments throw LBM_E_INVALID and leave the
// slot as it was; an allocation failure throws LBM_E_NOMEM and leaves it empty.
inline void begin(State *&slot, int nv, int moments, std::vector<Part> parts) {
    State *old = slot;
    if (moments != 1 && moments != 3) throw lbm_failure(LBM_E_INVALID, "moments must be LBM_AVG_MEAN or LBM_AVG_MEAN | LBM_AVG_SECOND");
    const int nf = moments == 3 ? all_fields(nv) : first_fields(nv);
    if (old && old->moments == moments && old->parts.size() == parts.size()) {
        for (auto &p : old->parts) {
            HIP_CHECK(hipSetDevice(p.dev));
            HIP_CHECK(hipMemsetAsync(p.acc, 0, sizeof(double) * (size_t)nf * (size_t)p.fstride(), p.st));
            HIP_CHECK(hipStreamSynchronize(p.st));
        }
        old->n = 0;
        return;
    }
    if (old) {
        slot = nullptr;
        old->release();
        delete old;
    }
    State *st = new State();
    st->nv = nv;
    st->moments = moments;
    st->nf = nf;
    st->parts = std::move(parts);
    try {
        for (auto &p : st->parts) {
            if ((long long)p.rows * ((p.w + 3) / 4) > (long long)INT_MAX)
                throw lbm_failure(LBM_E_INVALID, "sub-domain too large to average");
            HIP_CHECK(hipSetDevice(p.dev));
            const size_t bytes = sizeof(double) * (size_t)nf * (size_t)p.fstride();
            void *mem = nullptr;
            if (hipMalloc(&mem, bytes) != hipSuccess) {
                (void)hipGetLastError();
                throw lbm_failure(LBM_E_NOMEM, "no device memory for the accumulators of the averages");
            }
            p.acc = static_cast<double *>(mem);
            HIP_CHECK(hipMemsetAsync(p.acc, 0, bytes, p.st));
            HIP_CHECK(hipStreamSynchronize(p.st));
        }
    } catch (...) {
        st->release();
        delete st;
        throw;
    }
    slot = st;
}

template <class T>
hipError_t launch_accumulate(const MomentArgs &a, bool second, hipStream_t s) {
    const int blocks = fields_blocks(a.w, a.rows);
    if (second)
        hipLaunchKernelGGL((accumulate_moments<T, true>), dim3(blocks), dim3(AVG_BLOCK), 0, s, a);
    else
        hipLaunchKernelGGL((accumulate_moments<T, false>), dim3(blocks), dim3(AVG_BLOCK), 0, s, a);
    return hipGetLastError();
}

template <class T>
hipError_t launch_means(const MeansArgs &m, int w, int rows, hipStream_t s) {
    hipLaunchKernelGGL(moment_means<T>, dim3(fields_blocks(w, rows)), dim3(AVG_BLOCK), 0, s, m);
    return hipGetLastError();
}

// which of the nf_all outputs are asked for; throws LBM_E_STATE / LBM_E_INVALID per the contract
template <class P>
int wanted(const State *st, P *const *out) {
    if (!st) throw lbm_failure(LBM_E_STATE, "not averaging: call avg_begin first");
    if (!out) throw lbm_failure(LBM_E_INVALID, "NULL array of output pointers");
    const int all = all_fields(st->nv);
    int want = 0;
    for (int f = 0; f < all; ++f) {
        if (!out[f]) continue;
        if (f >= st->nf) throw lbm_failure(LBM_E_INVALID, "second moments asked of a handle begun with LBM_AVG_MEAN only");
        ++want;
    }
    return want;
}

// the raw sums into the caller's planar double arrays (the handle's streams are idle)
inline void store_sums(const State *st, double *const *out) {
    if (wanted(st, out) == 0) return;
    for (const auto &p : st->parts) {
        HIP_CHECK(hipSetDevice(p.dev));
        for (int f = 0; f < st->nf; ++f)
            if (out[f])
                HIP_CHECK(hipMemcpy2D(out[f] + p.host_off, sizeof(double) * p.host_pitch, p.acc + f * p.fstride(),
                                      sizeof(double) * (size_t)p.sp, sizeof(double) * (size_t)p.w, (size_t)p.rows,
                                      hipMemcpyDeviceToHost));
    }
}

// means and central moments into the caller's planar float arrays; launch(k, part, args) enqueues
// moment_means of part k on its stream
template <class L>
void store_means(const State *st, float *const *out, L &&launch) {
    const int want = wanted(st, out);
    if (want == 0) return;
    if (st->n == 0) throw lbm_failure(LBM_E_STATE, "no samples to average");
    for (size_t k = 0; k < st->parts.size(); ++k) {
        const Part &p = st->parts[k];
        HIP_CHECK(hipSetDevice(p.dev));
        const PlanarStage stage(want, (size_t)p.fstride());
        MeansArgs m{};
        m.acc = p.acc;
        m.fstride = p.fstride();
        m.n = (double)st->n;
        for (int f = 0, i = 0; f < st->nf; ++f) {
            field_sums(st->nv, f, m.a[f], m.b[f], m.ab[f]);
            if (out[f]) m.out[f] = stage.field(i++);
        }
        launch(k, p, m);
        HIP_CHECK(hipStreamSynchronize(p.st));
        stage.copy_out(out, st->nf, HostSpan{p.host_off, p.host_pitch}, (size_t)p.sp, (size_t)p.w, (size_t)p.rows);
    }
}

}  // namespace avg
}  // namespace lbm
