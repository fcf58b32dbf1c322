// lbm_host.hpp -- host-side problem I/O kept from the reference so its gate
// (check/check.py) keeps working unchanged.
//
//   Params::fromFile        main/include/LbmParams.hpp:28-58
//   Obstacles::fromFile     main/include/LbmParams.hpp:92-123 (+ bounds check,
//                           as LastChance.cpp:476-478 does)
//   initialiseCells         main/include/LatticeBoltzmannUtils.hpp:137-157
//   reynoldsNumber          LatticeBoltzmannUtils.hpp:202-205
//   writeAverageVelocities  LatticeBoltzmannUtils.hpp:208-219
//   writeResults            LatticeBoltzmannUtils.hpp:221-281
//   writeResultsFromFields  the same file from lbm_store_fields' planar arrays
//   writeMeanState          the time averages of lbm_avg_store in the same row
//                           format (lbm_runner --mean-every; no reference counterpart)
//   averageVelocity         LastChance.cpp:290-339 (used by compare_lbm)
//   labelBodies, wallForces, writeForces
//                           the momentum-exchange wall forces of
//                           include/lbm_forces_hip.h on the host (lbm_runner
//                           --forces; no reference counterpart)
//   nearWall, neqStrain, writeStressState
//                           the non-equilibrium strain rate of
//                           include/lbm_stress_hip.h on the host (lbm_runner
//                           --stress; no reference counterpart)
//   readTracers, tracerAdvance, tracerBlocked, writeTracers
//                           the tracers of include/lbm_tracers_hip.h on the
//                           host (lbm_runner --tracers; no reference
//                           counterpart): the advance goes through
//                           lbm_tracer_advance_ref, the per-point functions of
//                           the kernels compiled for the host
//   timedStep               main/include/GraphcoreUtils.hpp:130-138
#pragma once

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <numeric>
#include <optional>
#include <string>
#include <vector>

#include "lbm_hip.h"
#include "lbm_tracers_hip.h"

namespace lbmhost {

constexpr unsigned NumSpeeds = 9;

struct Params {
    size_t nx = 0, ny = 0, maxIters = 0, reynolds_dim = 0;
    float density = 0.f, accel = 0.f, omega = 0.f;

    static std::optional<Params> fromFile(const std::string &filename) {
        std::ifstream file(filename);
        if (!file.is_open()) {
            std::cerr << "Could not read parameters from " << filename << std::endl;
            return std::nullopt;
        }
        try {
            std::string line;
            auto u = [&]() -> size_t { std::getline(file, line); return std::stoul(line); };
            auto f = [&]() -> float { std::getline(file, line); return std::stof(line); };
            Params p;
            p.nx = u();
            p.ny = u();
            p.maxIters = u();
            p.reynolds_dim = u();
            p.density = f();
            p.accel = f();
            p.omega = f();
            return p;
        } catch (const std::exception &) {
            std::cerr << "Could not read parameters from " << filename << std::endl;
            return std::nullopt;
        }
    }

    lbm_params abi() const {
        return lbm_params{(int32_t)nx, (int32_t)ny, (int32_t)maxIters, (int32_t)reynolds_dim, density, accel, omega};
    }
};

struct Obstacles {
    size_t nx = 0, ny = 0;
    std::vector<uint8_t> data;  // [ny][nx]

    bool at(size_t x, size_t y) const { return data[y * nx + x] != 0; }

    static std::optional<Obstacles> fromFile(size_t nx, size_t ny, const std::string &filename) {
        std::ifstream file(filename);
        if (!file.is_open()) {
            std::cerr << "Could not read parameters from " << filename << std::endl;
            return std::nullopt;
        }
        Obstacles o;
        o.nx = nx;
        o.ny = ny;
        o.data.assign(nx * ny, 0);
        std::string line;
        while (std::getline(file, line)) {
            int x = 0, y = 0, v = 0;
            const int n = sscanf(line.c_str(), "%d %d %d", &x, &y, &v);
            if (n <= 0) break;  // blank tail ends the list
            if (n != 3 || v != 1) {
                std::cerr << "Malformed line: obstacle must be 1" << std::endl;
                return std::nullopt;
            }
            if (x < 0 || y < 0 || (size_t)x >= nx || (size_t)y >= ny) {
                std::cerr << "obstacle (" << x << "," << y << ") outside the grid" << std::endl;
                return std::nullopt;
            }
            o.data[(size_t)y * nx + (size_t)x] = 1;
        }
        return o;
    }
};

inline std::vector<float> initialiseCells(const Params &p) {
    std::vector<float> c(p.nx * p.ny * NumSpeeds);
    const float w0 = p.density * 4.f / 9.f, w1 = p.density / 9.f, w2 = p.density / 36.f;
    for (size_t i = 0; i < p.nx * p.ny; ++i) {
        float *s = &c[i * NumSpeeds];
        s[0] = w0;
        s[1] = s[2] = s[3] = s[4] = w1;
        s[5] = s[6] = s[7] = s[8] = w2;
    }
    return c;
}

inline float reynoldsNumber(const Params &p, float average_velocity) {
    const float viscosity = 1.f / 6.f * (2.f / p.omega - 1.f);
    return average_velocity * p.reynolds_dim / viscosity;
}

struct Macro {
    float ux, uy, u, pressure;
};

inline Macro macroscopic(const Params &p, const Obstacles &o, const std::vector<float> &cells, size_t ii, size_t jj) {
    const float c_sq = 1.f / 3.f;
    if (o.at(ii, jj)) return Macro{0.f, 0.f, 0.f, p.density * c_sq};
    const float *c = &cells[(ii + jj * p.nx) * NumSpeeds];
    float rho = 0.f;
    for (unsigned k = 0; k < NumSpeeds; ++k) rho += c[k];
    const float ux = (c[1] + c[5] + c[8] - (c[3] + c[6] + c[7])) / rho;
    const float uy = (c[2] + c[5] + c[6] - (c[4] + c[7] + c[8])) / rho;
    return Macro{ux, uy, sqrtf((ux * ux) + (uy * uy)), rho * c_sq};
}

inline float averageVelocity(const Params &p, const Obstacles &o, const std::vector<float> &cells) {
    int tot_cells = 0;
    float tot_u = 0.f;
    for (size_t jj = 0; jj < p.ny; ++jj)
        for (size_t ii = 0; ii < p.nx; ++ii)
            if (!o.at(ii, jj)) {
                tot_u += macroscopic(p, o, cells, ii, jj).u;
                ++tot_cells;
            }
    return tot_u / (float)tot_cells;
}

inline bool writeAverageVelocities(const std::string &filename, const std::vector<float> &av_vels) {
    std::ofstream file(filename);
    if (!file.is_open()) return false;
    for (size_t i = 0; i < av_vels.size(); ++i)
        file << i << ":\t" << std::scientific << std::setprecision(12) << av_vels[i] << "\n";
    return true;
}

// one row of a per-cell .dat file: `ii jj v[0] .. v[n-1] obstacle`
inline void writeCellRow(std::ostream &file, size_t ii, size_t jj, const float *v, int n, bool obstacle) {
    file << ii << " " << jj << std::setprecision(12) << std::scientific;
    for (int k = 0; k < n; ++k) file << " " << v[k];
    file << " " << (int)obstacle << "\n";
}

// one final_state.dat row: `ii jj u_x u_y |u| pressure obstacle`
inline void writeResultsRow(std::ostream &file, size_t ii, size_t jj, const Macro &m, bool obstacle) {
    const float v[4] = {m.ux, m.uy, m.u, m.pressure};
    writeCellRow(file, ii, jj, v, 4, obstacle);
}

inline bool writeResults(const std::string &filename, const Params &p, const Obstacles &o,
                         const std::vector<float> &cells) {
    std::ofstream file(filename);
    if (!file.is_open()) return false;
    for (size_t jj = 0; jj < p.ny; ++jj)
        for (size_t ii = 0; ii < p.nx; ++ii) writeResultsRow(file, ii, jj, macroscopic(p, o, cells, ii, jj), o.at(ii, jj));
    return true;
}

// final_state.dat from the planar float[ny][nx] fields of lbm_store_fields
// (computed on the device: the values macroscopic() derives from the cells)
inline bool writeResultsFromFields(const std::string &filename, const Params &p, const Obstacles &o,
                                   const std::vector<float> &ux, const std::vector<float> &uy,
                                   const std::vector<float> &u, const std::vector<float> &pressure) {
    const size_t n = p.nx * p.ny;
    if (ux.size() != n || uy.size() != n || u.size() != n || pressure.size() != n) return false;
    std::ofstream file(filename);
    if (!file.is_open()) return false;
    for (size_t jj = 0; jj < p.ny; ++jj)
        for (size_t ii = 0; ii < p.nx; ++ii) {
            const size_t i = ii + jj * p.nx;
            writeResultsRow(file, ii, jj, Macro{ux[i], uy[i], u[i], pressure[i]}, o.at(ii, jj));
        }
    return true;
}

// ---- momentum-exchange wall forces (include/lbm_forces_hip.h) ----

// Connected components of the blocked cells: 8-connected, periodic, numbered
// by each body's first cell in row-major order (lio.label_bodies' rule).
// labels[ny][nx], -1 on fluid cells; returns the number of bodies.
inline int32_t labelBodies(const Obstacles &o, std::vector<int32_t> &labels) {
    const size_t n = o.nx * o.ny;
    std::vector<size_t> parent(n);
    std::iota(parent.begin(), parent.end(), (size_t)0);
    auto find = [&](size_t i) {
        while (parent[i] != i) i = parent[i] = parent[parent[i]];
        return i;
    };
    for (size_t y = 0; y < o.ny; ++y)
        for (size_t x = 0; x < o.nx; ++x) {
            if (!o.at(x, y)) continue;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const size_t xx = (x + o.nx + dx) % o.nx, yy = (y + o.ny + dy) % o.ny;
                    if (!o.at(xx, yy)) continue;
                    const size_t a = find(y * o.nx + x), b = find(yy * o.nx + xx);
                    if (a != b) parent[std::max(a, b)] = std::min(a, b);  // the root is the body's first cell
                }
        }
    labels.assign(n, -1);
    int32_t nbodies = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!o.data[i]) continue;
        const size_t r = find(i);
        if (r == i) labels[i] = nbodies++;  // roots come first in row-major order
        else labels[i] = labels[r];
    }
    return nbodies;
}

struct BodyForces {
    std::vector<double> fx, fy;   // per body
    std::vector<int64_t> links;
    double total_fx = 0.0, total_fy = 0.0;
    int64_t total_links = 0;
};

// Per-body and total wall forces of AoS cells: the per-cell fp32 expressions
// of lbm_forces_hip.h, summed in fp64 in row-major order.
inline BodyForces wallForces(const Params &p, const Obstacles &o, const std::vector<float> &cells,
                             const std::vector<int32_t> &labels, int32_t nbodies) {
    static const int ex[9] = {0, 1, 0, -1, 0, 1, -1, -1, 1};
    static const int ey[9] = {0, 0, 1, 0, -1, 1, 1, -1, -1};
    BodyForces r;
    r.fx.assign(nbodies, 0.0);
    r.fy.assign(nbodies, 0.0);
    r.links.assign(nbodies, 0);
    for (size_t y = 0; y < p.ny; ++y)
        for (size_t x = 0; x < p.nx; ++x) {
            if (!o.at(x, y)) continue;
            const float *c = &cells[(x + y * p.nx) * NumSpeeds];
            float t[9];
            int nl = 0;
            for (int j = 1; j < 9; ++j) {
                const bool link = !o.at((x + p.nx + ex[j]) % p.nx, (y + p.ny + ey[j]) % p.ny);
                t[j] = link ? c[j] : 0.f;
                nl += link ? 1 : 0;
            }
            if (!nl) continue;
            const float fx = ((t[3] + t[6] + t[7]) - (t[1] + t[5] + t[8])) * 2.f;
            const float fy = ((t[4] + t[7] + t[8]) - (t[2] + t[5] + t[6])) * 2.f;
            r.total_fx += (double)fx;
            r.total_fy += (double)fy;
            r.total_links += nl;
            const int32_t b = labels[x + y * p.nx];
            if (b >= 0 && b < nbodies) {
                r.fx[b] += (double)fx;
                r.fy[b] += (double)fy;
                r.links[b] += nl;
            }
        }
    return r;
}

// mean_state.dat from the seven planar float[ny][nx] arrays of lbm_avg_store
// (LBM_AVG_* order): `ii jj mean_ux mean_uy mean_pressure c_uxux c_uxuy c_uyuy
// c_pp obstacle`, through the row formatter of final_state.dat
inline bool writeMeanState(const std::string &filename, const Params &p, const Obstacles &o,
                           const std::vector<float> (&f)[7]) {
    const size_t n = p.nx * p.ny;
    for (const auto &a : f)
        if (a.size() != n) return false;
    std::ofstream file(filename);
    if (!file.is_open()) return false;
    for (size_t jj = 0; jj < p.ny; ++jj)
        for (size_t ii = 0; ii < p.nx; ++ii) {
            const size_t i = ii + jj * p.nx;
            const float v[7] = {f[0][i], f[1][i], f[2][i], f[3][i], f[4][i], f[5][i], f[6][i]};
            writeCellRow(file, ii, jj, v, 7, o.at(ii, jj));
        }
    return true;
}

// ---- velocity gradients (include/lbm_gradients_hip.h) ----

// vorticity, divergence, strain, q (LBM_GRAD_* order), planar float[ny][nx]:
// the header's fp32 expressions over macroscopic()'s velocities of the AoS
// cells, periodic central differences, obstacle cells +0.
inline void velocityGradients(const Params &p, const Obstacles &o, const std::vector<float> &cells,
                              std::vector<float> (&f)[4]) {
    const size_t nx = p.nx, ny = p.ny;
    std::vector<float> U(nx * ny), V(nx * ny);
    for (size_t y = 0; y < ny; ++y)
        for (size_t x = 0; x < nx; ++x) {
            const Macro m = macroscopic(p, o, cells, x, y);
            U[x + y * nx] = m.ux;
            V[x + y * nx] = m.uy;
        }
    for (auto &a : f) a.assign(nx * ny, 0.f);
    for (size_t y = 0; y < ny; ++y)
        for (size_t x = 0; x < nx; ++x) {
            if (o.at(x, y)) continue;
            const size_t xe = x + 1 == nx ? 0 : x + 1, xw = x == 0 ? nx - 1 : x - 1;
            const size_t yn = y + 1 == ny ? 0 : y + 1, ys = y == 0 ? ny - 1 : y - 1;
            const float gxx = (U[xe + y * nx] - U[xw + y * nx]) * 0.5f, gxy = (U[x + yn * nx] - U[x + ys * nx]) * 0.5f;
            const float gyx = (V[xe + y * nx] - V[xw + y * nx]) * 0.5f, gyy = (V[x + yn * nx] - V[x + ys * nx]) * 0.5f;
            const float sxy = (gxy + gyx) * 0.5f;
            const float s2 = ((gxx * gxx) + (gyy * gyy)) + ((sxy * sxy) * 2.f);
            const size_t i = x + y * nx;
            f[0][i] = gyx - gxy;
            f[1][i] = gxx + gyy;
            f[2][i] = sqrtf(s2);
            f[3][i] = (((gxx * gxx) + (gyy * gyy)) * -0.5f) - (gxy * gyx);
        }
}

// gradient_state.dat from the four planar float[ny][nx] arrays (LBM_GRAD_*
// order): `ii jj vorticity divergence strain q obstacle`, through the row
// formatter of final_state.dat
inline bool writeGradientState(const std::string &filename, const Params &p, const Obstacles &o,
                               const std::vector<float> (&f)[4]) {
    const size_t n = p.nx * p.ny;
    for (const auto &a : f)
        if (a.size() != n) return false;
    std::ofstream file(filename);
    if (!file.is_open()) return false;
    for (size_t jj = 0; jj < p.ny; ++jj)
        for (size_t ii = 0; ii < p.nx; ++ii) {
            const size_t i = ii + jj * p.nx;
            const float v[4] = {f[0][i], f[1][i], f[2][i], f[3][i]};
            writeCellRow(file, ii, jj, v, 4, o.at(ii, jj));
        }
    return true;
}

// ---- non-equilibrium strain rate (include/lbm_stress_hip.h) ----

// near[ny][nx] = 1 on the fluid cells with a blocked neighbour among the eight (periodic)
inline std::vector<uint8_t> nearWall(const Obstacles &o) {
    std::vector<uint8_t> near(o.nx * o.ny, 0);
    for (size_t y = 0; y < o.ny; ++y)
        for (size_t x = 0; x < o.nx; ++x) {
            if (o.at(x, y)) continue;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx)
                    if ((dx || dy) && o.at((x + o.nx + dx) % o.nx, (y + o.ny + dy) % o.ny)) near[x + y * o.nx] = 1;
        }
    return near;
}

// sxx, sxy, syy, strain (LBM_STRESS_* order), planar float[ny][nx], from the
// non-equilibrium second moment of the stored AoS cells: the header's fp32
// expressions, obstacle cells +0.  false for omega = 1.
inline bool neqStrain(const Params &p, const Obstacles &o, const std::vector<float> &cells,
                      std::vector<float> (&f)[4]) {
    const size_t nx = p.nx, ny = p.ny;
    const float omo = 1.f - p.omega;
    if (omo == 0.f) return false;
    const float coef = (-1.5f * p.omega) / omo;
    for (auto &a : f) a.assign(nx * ny, 0.f);
    for (size_t y = 0; y < ny; ++y)
        for (size_t x = 0; x < nx; ++x) {
            if (o.at(x, y)) continue;
            const size_t i = x + y * nx;
            const float *c = &cells[i * NumSpeeds];
            const Macro m = macroscopic(p, o, cells, x, y);
            float rho = 0.f;
            for (unsigned k = 0; k < NumSpeeds; ++k) rho += c[k];
            const float pxx = ((((c[1] + c[3]) + c[5]) + c[6]) + c[7]) + c[8];
            const float pyy = ((((c[2] + c[4]) + c[5]) + c[6]) + c[7]) + c[8];
            const float pxy = (c[5] + c[7]) - (c[6] + c[8]);
            const float pr = rho * (1.f / 3.f);
            const float nxx = (pxx - pr) - ((rho * m.ux) * m.ux);
            const float nyy = (pyy - pr) - ((rho * m.uy) * m.uy);
            const float nxy = pxy - ((rho * m.ux) * m.uy);
            const float k = coef / rho;
            const float sxx = nxx * k, syy = nyy * k, sxy = nxy * k;
            f[0][i] = sxx;
            f[1][i] = sxy;
            f[2][i] = syy;
            f[3][i] = sqrtf(((sxx * sxx) + (syy * syy)) + ((sxy * sxy) * 2.f));
        }
    return true;
}

// stress_state.dat from the four planar float[ny][nx] arrays (LBM_STRESS_*
// order) and the near-wall map: `ii jj sxx sxy syy strain near_wall obstacle`,
// the values through the row formatter of final_state.dat
inline bool writeStressState(const std::string &filename, const Params &p, const Obstacles &o,
                             const std::vector<float> (&f)[4], const std::vector<uint8_t> &near) {
    const size_t n = p.nx * p.ny;
    for (const auto &a : f)
        if (a.size() != n) return false;
    if (near.size() != n) return false;
    std::ofstream file(filename);
    if (!file.is_open()) return false;
    for (size_t jj = 0; jj < p.ny; ++jj)
        for (size_t ii = 0; ii < p.nx; ++ii) {
            const size_t i = ii + jj * p.nx;
            file << ii << " " << jj << std::setprecision(12) << std::scientific;
            for (int k = 0; k < 4; ++k) file << " " << f[k][i];
            file << " " << (int)near[i] << " " << (int)o.at(ii, jj) << "\n";
        }
    return true;
}

// ---- binned sums (include/lbm_binned_hip.h) ----

// The nine LBM_BIN_* sums and the fluid cells per bin of bw x bh cells, planar
// [nby][nbx]: per bin the fp64 sum, row after row, of (double) of the header's
// fp32 terms over the bin's fluid cells (products formed in fp64).
struct BinnedSums {
    size_t nbx = 0, nby = 0;
    std::vector<double> sum[9];
    std::vector<int64_t> fluid;
};

inline BinnedSums binnedSums(const Params &p, const Obstacles &o, const std::vector<float> &cells, size_t bw,
                             size_t bh) {
    BinnedSums r;
    r.nbx = (p.nx + bw - 1) / bw;
    r.nby = (p.ny + bh - 1) / bh;
    for (auto &a : r.sum) a.assign(r.nbx * r.nby, 0.0);
    r.fluid.assign(r.nbx * r.nby, 0);
    for (size_t y = 0; y < p.ny; ++y)
        for (size_t x = 0; x < p.nx; ++x) {
            if (o.at(x, y)) continue;
            const float *c = &cells[(x + y * p.nx) * NumSpeeds];
            const Macro m = macroscopic(p, o, cells, x, y);
            float rho = 0.f;
            for (unsigned k = 0; k < NumSpeeds; ++k) rho += c[k];
            const float jx = c[1] + c[5] + c[8] - (c[3] + c[6] + c[7]);
            const float jy = c[2] + c[5] + c[6] - (c[4] + c[7] + c[8]);
            const double ux = m.ux, uy = m.uy;
            const double t[9] = {rho, jx, jy, ux, uy, m.u, ux * ux, ux * uy, uy * uy};
            const size_t b = x / bw + (y / bh) * r.nbx;
            for (int k = 0; k < 9; ++k) r.sum[k][b] += t[k];
            ++r.fluid[b];
        }
    return r;
}

// binned_state.dat: `bx by fluid` and the nine sums per bin, by outer
inline bool writeBinnedState(const std::string &filename, const BinnedSums &b) {
    FILE *file = fopen(filename.c_str(), "w");
    if (!file) return false;
    for (size_t by = 0; by < b.nby; ++by)
        for (size_t bx = 0; bx < b.nbx; ++bx) {
            const size_t i = bx + by * b.nbx;
            fprintf(file, "%zu %zu %lld", bx, by, (long long)b.fluid[i]);
            for (const auto &a : b.sum) fprintf(file, " %.12E", a[i]);
            fprintf(file, "\n");
        }
    return fclose(file) == 0;
}

// ---- tracers and point probes (include/lbm_tracers_hip.h) ----

struct Tracers {
    std::vector<double> x, y;
    std::vector<uint8_t> blocked;
};

// one `x y` per line (cell units); every point inside [0, nx) x [0, ny)
inline std::optional<Tracers> readTracers(const std::string &filename, const Params &p) {
    std::ifstream file(filename);
    if (!file.is_open()) {
        std::cerr << "Could not read tracers from " << filename << std::endl;
        return std::nullopt;
    }
    Tracers t;
    std::string line;
    while (std::getline(file, line)) {
        double x = 0.0, y = 0.0;
        const int n = sscanf(line.c_str(), "%lf %lf", &x, &y);
        if (n <= 0) continue;  // blank line
        if (n != 2 || !(x >= 0.0 && x < (double)p.nx) || !(y >= 0.0 && y < (double)p.ny)) {
            std::cerr << "Malformed tracer line (x y inside the grid expected): " << line << std::endl;
            return std::nullopt;
        }
        t.x.push_back(x);
        t.y.push_back(y);
    }
    if (t.x.empty()) {
        std::cerr << "No tracer in " << filename << std::endl;
        return std::nullopt;
    }
    return t;
}

// One advance by dt in the velocity field of the AoS cells: macroscopic()'s
// u_x, u_y as planar arrays, then lbm_tracer_advance_ref.
inline bool tracerAdvance(const Params &p, const Obstacles &o, const std::vector<float> &cells, Tracers &t, double dt,
                          int scheme) {
    std::vector<float> ux(p.nx * p.ny), uy(p.nx * p.ny);
    for (size_t y = 0; y < p.ny; ++y)
        for (size_t x = 0; x < p.nx; ++x) {
            const Macro m = macroscopic(p, o, cells, x, y);
            ux[x + y * p.nx] = m.ux;
            uy[x + y * p.nx] = m.uy;
        }
    return lbm_tracer_advance_ref((int32_t)p.nx, (int32_t)p.ny, ux.data(), uy.data(), (int64_t)t.x.size(), t.x.data(),
                                  t.y.data(), dt, scheme) == LBM_OK;
}

// the header's blocked flag: the nearest cell, floor(c + 0.5) taken to 0 at the extent, is an obstacle
inline void tracerBlocked(const Obstacles &o, Tracers &t) {
    auto nearest = [](double c, size_t n) {
        const size_t i = (size_t)std::floor(c + 0.5);
        return i == n ? (size_t)0 : i;
    };
    t.blocked.resize(t.x.size());
    for (size_t i = 0; i < t.x.size(); ++i) t.blocked[i] = o.at(nearest(t.x[i], o.nx), nearest(t.y[i], o.ny)) ? 1 : 0;
}

// tracers.dat: `id x y blocked` per point, the positions in %.17g (they read back to the same doubles)
inline bool writeTracers(const std::string &filename, const Tracers &t) {
    FILE *file = fopen(filename.c_str(), "w");
    if (!file) return false;
    for (size_t i = 0; i < t.x.size(); ++i) fprintf(file, "%zu %.17g %.17g %d\n", i, t.x[i], t.y[i], (int)t.blocked[i]);
    return fclose(file) == 0;
}

// forces.dat: `body fx fy links` per body, then `total fx fy links`
inline bool writeForces(const std::string &filename, const BodyForces &f) {
    FILE *file = fopen(filename.c_str(), "w");
    if (!file) return false;
    for (size_t b = 0; b < f.fx.size(); ++b)
        fprintf(file, "%zu %.12E %.12E %lld\n", b, f.fx[b], f.fy[b], (long long)f.links[b]);
    fprintf(file, "total %.12E %.12E %lld\n", f.total_fx, f.total_fy, (long long)f.total_links);
    return fclose(file) == 0;
}

template <class F>
double timedStep(const std::string &description, F &&f) {
    std::cerr << std::setw(60) << description;
    const auto tic = std::chrono::high_resolution_clock::now();
    f();
    const auto toc = std::chrono::high_resolution_clock::now();
    const double s = std::chrono::duration<double>(toc - tic).count();
    std::cerr << " took " << std::right << std::setw(12) << std::setprecision(5) << s << "s" << std::endl;
    return s;
}

// Fail loudly on any C-ABI error.
inline void check(int rc, lbm_handle *h, const char *what) {
    if (rc != LBM_OK) {
        std::cerr << what << " failed (" << rc << "): " << lbm_last_error(h) << std::endl;
        std::exit(EXIT_FAILURE);
    }
}

}  // namespace lbmhost
