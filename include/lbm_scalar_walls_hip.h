/*
 * lbm_scalar_walls_hip.h -- wall models of the passive scalar (a fixed wall
 * value, a fixed wall flux) and the scalar every body hands to the fluid (the
 * heat a cylinder gives off, the heat through a plate).  An additive part of
 * the C ABI of liblbm_hip.so (LBM_ABI_VERSION unchanged) for both engines:
 * the D2Q5 scalar of lbm_hip.h handles and the D3Q7 scalar of lbm3d_hip.h
 * handles (lbm_scalar_hip.h).
 *
 * The scalar step stores in every obstacle cell the populations that hit it,
 * reversed (out_k = p_opp(k)): the zero-flux wall.  The stored g_k of a blocked
 * cell x is what the fluid cell x + e_k pulls in the next step.  A wall model
 * is therefore a pass over the wall cells alone, after the step, that rewrites
 * those stored values link by link, and the scalar handed to the fluid through
 * a link is a cell-local function of the stored scalar lattice -- as the wall
 * force of lbm_forces_hip.h is of the flow lattice.  No step kernel changes
 * and no cell that is no wall cell is read or written: the cost is O(wall
 * cells).
 *
 * Kinds.  LBM_SCALAR_WALL_ADIABATIC (0), LBM_SCALAR_WALL_VALUE (1),
 * LBM_SCALAR_WALL_FLUX (2).
 *
 * Links.  For a blocked cell x and a moving scalar speed k (1..4 in D2Q5: E,
 * N, W, S; 1..6 in D3Q7: +x, -x, +y, -y, +z, -z; the speed order of
 * lbm_scalar_hip.h), link k is set iff cell x + e_k, periodic over the full
 * domain, is not blocked.  A blocked cell with at least one link is a wall
 * cell: the rule of lbm_forces_hip.h on the scalar's speeds.
 *
 * Bodies.  A label map assigns blocked cells to bodies 0 .. nbodies-1, by the
 * rules of lbm_set_bodies: a negative label belongs to no body and the cell
 * stays adiabatic; labels on fluid cells are ignored; a label >= nbodies on a
 * blocked cell is LBM_E_INVALID.  Every body has a kind and an fp32 value v; a
 * kind outside 0..2 or a value that is not finite is LBM_E_INVALID.  After any
 * LBM_E_INVALID the walls set before stay.  The library copies what it needs
 * and keeps no caller pointer.
 *
 * Wall pass.  Inside every step of lbm_scalar_advance, on the new current set,
 * after the step launches and before the fixed list.  IEEE fp32, every
 * operation rounded on its own, no contraction.  For a wall cell of a body
 * (kind, v) and every set link k, with w1 the begin weight of a moving speed
 * (1.f/6.f in D2Q5, 0.125f in D3Q7):
 *     VALUE:  m = v * w1;  d = m + m;  g_k <- d - g_k     (anti-bounce-back: the
 *             wall holds the value v halfway between the wall cell and the fluid cell)
 *     FLUX:   g_k <- g_k + v                              (v: the scalar added per link
 *             and step; positive heats the fluid)
 * ADIABATIC bodies, unset links, g_0 and every cell that is no wall cell of a
 * labelled body keep every bit.  Setting the walls applies nothing; the pass
 * is not idempotent and runs nowhere but inside lbm_scalar_advance.
 *
 * Wall flux.  Per wall cell q = ((t_1 + t_2) + ...) in speed order, with
 *     t_k = (g_k - m) * 2.f  for a set link of a VALUE body,
 *     t_k = v                for a set link of a FLUX body,
 *     t_k = +0.f             for anything else and for unset links,
 * of the STORED populations; every other cell gives +0.  This is the scalar
 * handed to the fluid through the wall cell's links in the step that produced
 * the stored set: it has that meaning only after at least one advance since
 * the walls (or the table) were set, and on cells the fixed list does not
 * overwrite.  Summed over all wall cells it is the change of the total scalar
 * in that step (the step itself conserves the sum).
 *
 * Totals and per-body sums follow lbm_wall_force: fp64 sums of the fp32
 * per-cell values and counts of set link bits, folded in a fixed order without
 * atomics, so two calls on the same state give identical bits.  The total's
 * link count covers every wall cell of the domain, labelled or not; a body's
 * covers its own wall cells.
 *
 * Fixed list.  A cell may be in the fixed list and a wall cell of a body.  The
 * fixed list runs last and wins: such a cell holds the begin state of its
 * fixed value, and its wall flux says nothing about a heat exchange.
 *
 * Lifetime.  lbm_scalar_begin (which replaces the state) and lbm_scalar_end
 * drop the walls.
 *
 * Contract, as in lbm_scalar_hip.h: LBM_E_INVALID for a NULL handle;
 * LBM_E_STATE before lbm_scalar_begin; every call blocks; a flux sample
 * changes no bit of either lattice; set_walls touches neither lattice.  A
 * handle that never sets walls allocates and launches nothing new, and its
 * lbm_scalar_advance is what it was bit for bit.  One list covers the whole
 * domain (the scalar lattice is global), so nothing depends on the handle's
 * decomposition.  On an LBM_FLAG_PROFILE handle (D2Q9) the pass is accounted
 * under the class "scalar_walls", the samples under classes whose names start
 * with "scalar_wall_flux".
 *
 * Not built: wall values or fluxes that vary inside a body (one body per
 * value: a body may be a single cell); walls that are not halfway between the
 * cells; domains of more than 2^31 - 1 cells (LBM_E_INVALID).
 */
#ifndef LBM_SCALAR_WALLS_HIP_H
#define LBM_SCALAR_WALLS_HIP_H

#include <stdint.h>

#include "lbm_forces_hip.h"
#include "lbm_scalar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { LBM_SCALAR_WALL_ADIABATIC = 0, LBM_SCALAR_WALL_VALUE = 1, LBM_SCALAR_WALL_FLUX = 2 };

/* Builds the wall list (cell, link mask, body) from the handle's obstacle map
 * and labels int32[ny][nx], and the per-body table from kind and value (nbodies
 * entries each; nbodies >= 1).  labels == NULL with nbodies equal to the count
 * set before (>= 1) replaces only the table -- a wall value that changes in
 * time, without a rebuild.  (NULL, 0, NULL, NULL) clears the walls.  Anything
 * else with a NULL array: LBM_E_INVALID. */
int lbm_scalar_set_walls(lbm_handle *h, const int32_t *labels, int32_t nbodies, const int32_t *kind,
                         const float *value);

/* The sum of the wall flux over all wall cells and the links of all wall
 * cells; zeros while no walls are set.  Either pointer may be NULL. */
int lbm_scalar_wall_flux(lbm_handle *h, double *q, int64_t *links);

/* Per-body sums into arrays of nbodies entries (either may be NULL).  No
 * walls set, or set with another nbodies: LBM_E_STATE. */
int lbm_scalar_body_flux(lbm_handle *h, double *q, int64_t *links, int32_t nbodies);

/* The per-cell wall flux, planar float[ny][nx], +0 off the walls. */
int lbm_scalar_store_wall_flux(lbm_handle *h, float *q);

/* D3Q19 twins: labels int32[nz][ny][nx], q planar float[nz][ny][nx]. */
int lbm3d_scalar_set_walls(lbm3d_handle *h, const int32_t *labels, int32_t nbodies, const int32_t *kind,
                           const float *value);
int lbm3d_scalar_wall_flux(lbm3d_handle *h, double *q, int64_t *links);
int lbm3d_scalar_body_flux(lbm3d_handle *h, double *q, int64_t *links, int32_t nbodies);
int lbm3d_scalar_store_wall_flux(lbm3d_handle *h, float *q);

/* Host-only restatements (no GPU, no handle), compiled from the same per-cell
 * functions as the kernels: the wall pass applied in place to the planar,
 * unpadded populations g (float[5][ny][nx] / float[7][nz][ny][nx]) over the
 * obstacle map uint8 and the labels int32 of the domain, and, when q is not
 * NULL, the per-cell wall flux of the result (float, the domain's shape).  A
 * NULL array other than q, an extent < 1, nbodies < 1, a bad kind, value or
 * label: LBM_E_INVALID, nothing written. */
int lbm_scalar_walls_ref(int32_t nx, int32_t ny, const uint8_t *obst, const int32_t *labels, int32_t nbodies,
                         const int32_t *kind, const float *value, float *g, float *q);
int lbm3d_scalar_walls_ref(int32_t nx, int32_t ny, int32_t nz, const uint8_t *obst, const int32_t *labels,
                           int32_t nbodies, const int32_t *kind, const float *value, float *g, float *q);

#ifdef __cplusplus
}
#endif

#endif /* LBM_SCALAR_WALLS_HIP_H */
