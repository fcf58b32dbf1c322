/*
 * lbm_forces_hip.h -- the force the fluid puts on the obstacles (drag / lift
 * per body, wall totals), computed on the device from the current lattice by
 * momentum exchange.  An additive part of the C ABI of liblbm_hip.so
 * (LBM_ABI_VERSION unchanged) for both engines: D2Q9 (lbm_hip.h) and D3Q19
 * (lbm3d_hip.h).
 *
 * The step bounces back on obstacle cells (out_k = s_opp(k)), so an obstacle
 * cell's stored populations are the populations that hit it in the last step,
 * already reversed.  The force is therefore a cell-local function of the
 * stored lattice and the static obstacle map; no neighbour's populations are
 * read, no halo is exchanged and no step kernel changes.
 *
 * Definition, D2Q9 (speed order of lbm_hip.h: e1 (+1,0), e2 (0,+1), e3 (-1,0),
 * e4 (0,-1), e5 (+1,+1), e6 (-1,+1), e7 (-1,-1), e8 (+1,-1)).  For a blocked
 * cell x and j = 1..8, link j is set iff cell x + e_j (periodic over the full
 * domain) is not blocked; a blocked cell with at least one link is a wall
 * cell.  With t_j = link_j ? f_j(x) : +0.f, in IEEE fp32, left to right, no
 * contraction:
 *     fx = ((t3 + t6 + t7) - (t1 + t5 + t8)) * 2.f
 *     fy = ((t4 + t7 + t8) - (t2 + t5 + t6)) * 2.f
 * Every other cell gives +0, +0.  D3Q19 (speed order and opposites of
 * lbm3d_hip.h), the same rule over j = 1..18:
 *     fx = ((t2+t6+t8+t11+t15)    - (t1+t5+t7+t10+t16))  * 2.f
 *     fy = ((t4+t6+t7+t13+t17)    - (t3+t5+t8+t12+t18))  * 2.f
 *     fz = ((t14+t15+t16+t17+t18) - (t9+t10+t11+t12+t13)) * 2.f
 * This is the momentum handed to the wall in the step that produced the
 * lattice.
 *
 * Totals: F = fp64 sum over wall cells of the fp32 per-cell values (the
 * convention of lbm_field_stats), links = count of set link bits.  Folded in
 * a fixed order without floating-point atomics: two calls on the same lattice
 * return identical bits.  Totals cover this handle's sub-domains / slabs;
 * RCCL callers add the ranks' values themselves.
 *
 * Bodies: a label map assigns blocked cells to bodies 0 .. nbodies-1.  A
 * negative label belongs to no body (the cell still counts in the totals);
 * labels on fluid cells are ignored; a blocked cell with label >= nbodies, or
 * nbodies <= 0 with non-NULL labels, or NULL labels with nbodies != 0, is
 * LBM_E_INVALID (the bodies set before stay).  set_bodies(h, NULL, 0) clears
 * the bodies.  The library copies what it needs and keeps no caller pointer.
 * body_forces before set_bodies, or with another nbodies, is LBM_E_STATE.
 *
 * Only wall cells are touched: the first force call of a handle builds one
 * compact wall list per sub-domain / slab (cell offset, link mask, body id),
 * and a sample reads O(wall cells) bytes.  A handle that never asks for forces
 * allocates and launches nothing extra.
 *
 * Every call blocks, reads the current lattice and changes no engine state (a
 * run afterwards continues bit-identically); LBM_E_INVALID for a NULL handle,
 * LBM_E_STATE before load_cells / init_equilibrium.  2-D calls on an
 * LBM_FLAG_PROFILE handle are accounted under launch classes whose names
 * start with "wall_force".
 */
#ifndef LBM_FORCES_HIP_H
#define LBM_FORCES_HIP_H

#include <stdint.h>

#include "lbm3d_hip.h"
#include "lbm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Total force on all wall cells of this handle's sub-domains and the number
 * of links.  Any pointer may be NULL. */
int lbm_wall_force(lbm_handle *h, double *fx, double *fy, int64_t *links);

/* Per-cell force, planar float[ny][nx] per component, full domain (+0 on
 * every cell that is no wall cell).  RCCL: this rank's rectangle only, the
 * rest of the arrays is left untouched.  Either pointer may be NULL. */
int lbm_store_wall_force(lbm_handle *h, float *fx, float *fy);

/* labels int32[ny][nx], full domain (see "Bodies" above). */
int lbm_set_bodies(lbm_handle *h, const int32_t *labels, int32_t nbodies);

/* Per-body sums over this handle's sub-domains into arrays of nbodies entries
 * (any may be NULL): fp64 sums of the fp32 per-cell values and link counts,
 * reduced on the device in a fixed order. */
int lbm_body_forces(lbm_handle *h, double *fx, double *fy, int64_t *links, int32_t nbodies);

/* D3Q19 twins: planar float[nz][ny][nx], labels int32[nz][ny][nx]; RCCL:
 * this rank's planes only. */
int lbm3d_wall_force(lbm3d_handle *h, double *fx, double *fy, double *fz, int64_t *links);
int lbm3d_store_wall_force(lbm3d_handle *h, float *fx, float *fy, float *fz);
int lbm3d_set_bodies(lbm3d_handle *h, const int32_t *labels, int32_t nbodies);
int lbm3d_body_forces(lbm3d_handle *h, double *fx, double *fy, double *fz, int64_t *links, int32_t nbodies);

#ifdef __cplusplus
}
#endif

#endif /* LBM_FORCES_HIP_H */
