/*
 * lbm_thermal_hip.h -- Boussinesq buoyancy: the scalar of lbm_scalar_hip.h
 * drives the flow.  An additive part of the C ABI of liblbm_hip.so
 * (LBM_ABI_VERSION unchanged) for both engines; lbm_scalar_hip.h includes it,
 * so a program that carries a scalar has these calls too.  (The declarations
 * stand in a file of their own because the scalar header's list of sixteen
 * symbols is pinned.)
 *
 * The scalar step reads the flow and never writes it.  This is the arrow
 * back: one call adds to every fluid cell of the current flow lattice the
 * momentum
 *
 *     rho0 * s * (phi - phi_ref)
 *
 * rho0 the handle's params.density (the Boussinesq approximation: density
 * varies through this term alone), s an impulse vector (the acceleration per
 * unit of scalar times the number of flow steps it stands for), phi the
 * cell's scalar exactly as lbm_scalar_store gives it: the sequential sum of
 * its own stored g.  The force is an impulse on the stored populations
 * between runs; no step kernel changes, and a run afterwards continues from
 * the kicked lattice exactly as if it had been loaded with load_cells.
 *
 * Definition.  IEEE fp32, every operation rounded separately, as written, no
 * contraction.  Per call, on the host:
 *
 *     kx = density * sx;  ky = density * sy;  (3-D)  kz = density * sz
 *
 * Per fluid cell, D2Q9 (speeds 0 rest, 1 E, 2 N, 3 W, 4 S, 5 NE, 6 NW, 7 SW,
 * 8 SE):
 *
 *     d  = phi - phi_ref;       jx = kx * d;            jy = ky * d
 *     ax = jx * (1.f/3.f);      ay = jy * (1.f/3.f)
 *     f1 += ax;  f3 -= ax;      f2 += ay;  f4 -= ay
 *     bx = jx * (1.f/12.f);     by = jy * (1.f/12.f);   p = bx + by;  q = by - bx
 *     f5 += p;   f7 -= p;       f6 += q;   f8 -= q
 *
 * which is 3 w_k rho0 (c_k . s) d with the D2Q9 weights; f0 is not touched.
 *
 * Per fluid cell, D3Q19 (speed order of lbm3d_hip.h), j_c = k_c * d:
 *
 *     a_c = j_c * (1.f/6.f);    b_c = j_c * (1.f/12.f)          c = x, y, z
 *     f1  += ax;       f2  -= ax          (+x, -x)
 *     f3  += ay;       f4  -= ay          (+y, -y)
 *     f9  += az;       f14 -= az          (+z, -z)
 *     f5  += bx + by;  f6  -= bx + by     (+x+y, -x-y)
 *     f7  += bx - by;  f8  -= bx - by     (+x-y, -x+y)
 *     f10 += bx + bz;  f15 -= bx + bz     (+x+z, -x-z)
 *     f11 += bz - bx;  f16 -= bz - bx     (-x+z, +x-z)
 *     f12 += by + bz;  f17 -= by + bz     (+y+z, -y-z)
 *     f13 += bz - by;  f18 -= bz - by     (-y+z, +y-z)
 *
 * each sum or difference of two b formed once per opposite pair; f0 is not
 * touched.
 *
 * In both: the increment of speed k is exactly the negative of the increment
 * of opp(k), so in exact arithmetic the call adds no mass and exactly
 * (jx, jy[, jz]) of momentum.  An obstacle cell keeps the bits of all its
 * populations (the loaded value is selected, no zero is added).  Ghost cells
 * and pad columns are neither read nor written.  There is NO positivity
 * guard: a large |s (phi - phi_ref)| drives populations negative like any
 * over-strong force; keeping |s| small is the caller's business.
 *
 * Contract.  NULL handle: LBM_E_INVALID.  Before lbm_scalar_begin, or before
 * the flow lattice is loaded: LBM_E_STATE.  A non-finite argument:
 * LBM_E_INVALID, nothing written.  Every component of s equal to zero:
 * LBM_OK, no launch, the lattice keeps its bits.  Otherwise the call follows
 * a synchronisation of the handle's streams, launches once per local
 * sub-domain (slab) on the compute stream of the first, on the owned cells of
 * the CURRENT side of the flow pair, blocks, and leaves the ghost cells to
 * the engine's own mechanism (D2Q9: the ring is rebuilt at the start of the
 * next run; D3Q19: the ghost planes are exchanged as after load_cells).  The
 * scalar lattice, its step count, the fixed list and av_vels are untouched.
 * On an LBM_FLAG_PROFILE handle (D2Q9) the launches are accounted under the
 * class "scalar_buoyancy".  The restrictions are those of scalar_begin.
 *
 * Not built: the kick fused into the scalar step or a flow kernel;
 * second-order (Guo) forcing; a force on the local rho; a heat-flux
 * (Nusselt) reduction; scalars on several devices.
 */
#ifndef LBM_THERMAL_HIP_H
#define LBM_THERMAL_HIP_H

#include <stdint.h>

#include "lbm3d_hip.h"
#include "lbm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int lbm_scalar_buoyancy(lbm_handle *h, float sx, float sy, float phi_ref);
int lbm3d_scalar_buoyancy(lbm3d_handle *h, float sx, float sy, float sz, float phi_ref);

/* Host-only restatements (no GPU, no handle), compiled from the same per-cell
 * function as the kernels: the kick applied in place to AoS cells
 * float[ny][nx][9] (float[nz][ny][nx][19]) from the planar scalar populations
 * g float[5][ny][nx] (float[7][nz][ny][nx]) and the obstacle map.  A NULL
 * array, an extent < 1 or a non-finite number: LBM_E_INVALID, nothing
 * written.  Every component of s zero: LBM_OK, nothing written. */
int lbm_scalar_buoyancy_ref(int32_t nx, int32_t ny, float density, float sx, float sy, float phi_ref,
                            const uint8_t *obst, const float *g, float *cells);
int lbm3d_scalar_buoyancy_ref(int32_t nx, int32_t ny, int32_t nz, float density, float sx, float sy, float sz,
                              float phi_ref, const uint8_t *obst, const float *g, float *cells);

#ifdef __cplusplus
}
#endif

#endif /* LBM_THERMAL_HIP_H */
