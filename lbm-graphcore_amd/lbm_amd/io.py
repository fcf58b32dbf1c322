"""Problem I/O, mirroring the reference host (kept on the host in this build).

* Params.from_file      -- lbm::Params::fromFile     main/include/LbmParams.hpp:28-58
* Obstacles.from_file   -- lbm::Obstacles::fromFile  main/include/LbmParams.hpp:92-123
* init_cells            -- lbm::Cells::initialise    main/include/LatticeBoltzmannUtils.hpp:137-157
* write_average_velocities -- writeAverageVelocities  LatticeBoltzmannUtils.hpp:208-219
* write_results         -- writeResults              LatticeBoltzmannUtils.hpp:221-281
* write_results_from_fields -- the same file from planar u_x, u_y, |u|, pressure
                           arrays (Engine.fields(): lbm_store_fields)
* reynolds_number       -- reynoldsNumber            LatticeBoltzmannUtils.hpp:202-205
* macroscopic3d         -- the D3Q19 fields of include/lbm3d_fields_hip.h in fp32 numpy
                           (Engine3D.fields(): lbm3d_store_fields)
* wall_links, wall_force_cells, wall_force (+ ...3d), label_bodies
                        -- the momentum-exchange wall forces of include/lbm_forces_hip.h
                           in fp32 numpy (Engine.wall_force(), .wall_force_field(), .body_forces())
* neq_strain, neq_strain3d, near_wall, near_wall3d, strain_stats
                        -- the non-equilibrium strain rate of include/lbm_stress_hip.h in fp32
                           numpy (Engine.strain_rate(), .strain_stats())
* binned_terms, binned_sums (+ ...3d), bin_reduce, binned_means
                        -- the binned sums of include/lbm_binned_hip.h: the per-cell terms in
                           numpy, math.fsum per bin (Engine.binned(), .profile_y(), .flux_x())
* tracer_interp, tracer_advance, tracer_blocked (+ ...3d), tracer_wrap, read_tracers
                        -- the tracers and point probes of include/lbm_tracers_hip.h in float64
                           numpy (Engine.tracer_sample(), .tracers_advance(), .tracers())
* scalar_init, scalar_step, scalar_phi, scalar_apply_fixed, scalar_stats (+ ...3d)
                        -- the passive scalar of include/lbm_scalar_hip.h in fp32 numpy
                           (Engine.scalar_begin(), .scalar_advance(), .scalar(), .scalar_stats())
* buoyancy_increments, buoyancy_kick (+ ...3d), rayleigh_number
                        -- the Boussinesq kick of include/lbm_thermal_hip.h in fp32 numpy
                           (Engine.scalar_buoyancy(), .run_thermal())

Error behaviour follows the reference: loaders return None (std::nullopt)
and print the reference's message on stderr.  One deliberate strengthening:
an obstacle outside the grid is rejected (the reference indexes out of
bounds; LastChance.cpp:476-478 rejects it too).
"""
from __future__ import annotations

import sys
from dataclasses import dataclass

import numpy as np

Q = 9
C_SQ = np.float32(1.0) / np.float32(3.0)


@dataclass(frozen=True)
class Params:
    nx: int
    ny: int
    max_iters: int
    reynolds_dim: int
    density: float   # fp32 values (stof)
    accel: float
    omega: float

    @staticmethod
    def from_file(filename: str) -> "Params | None":
        """7 lines: nx, ny, maxIters, reynolds_dim (stoul), density, accel, omega (stof)."""
        try:
            with open(filename, "r") as f:
                lines = f.read().split("\n")
        except OSError:
            print(f"Could not read parameters from {filename}", file=sys.stderr)
            return None
        try:
            ints = [int(lines[i].strip().split()[0]) for i in range(4)]
            floats = [float(np.float32(lines[i].strip().split()[0])) for i in range(4, 7)]
        except (IndexError, ValueError):
            print(f"Could not read parameters from {filename}", file=sys.stderr)
            return None
        if any(v < 0 for v in ints):
            print(f"Could not read parameters from {filename}", file=sys.stderr)
            return None
        return Params(ints[0], ints[1], ints[2], ints[3], *floats)

    def with_iters(self, iters: int) -> "Params":
        return Params(self.nx, self.ny, int(iters), self.reynolds_dim, self.density, self.accel, self.omega)


@dataclass(frozen=True)
class Params3D:
    """D3Q19 extension (include/lbm3d_hip.h; no reference counterpart)."""
    nx: int
    ny: int
    nz: int
    max_iters: int
    density: float
    accel: float
    omega: float


def channel_obstacles3d(nx: int, ny: int, nz: int) -> np.ndarray:
    """Wall planes at y = 0 and y = ny-1 (a Poiseuille channel, periodic in x and z)."""
    o = np.zeros((nz, ny, nx), np.uint8)
    o[:, 0, :] = 1
    o[:, -1, :] = 1
    return o


def read_obstacles(nx: int, ny: int, filename: str) -> "np.ndarray | None":
    """`x y 1` lines -> uint8[ny][nx] (LbmParams.hpp:92-123). None on failure."""
    data = np.zeros((ny, nx), np.uint8)
    try:
        f = open(filename, "r")
    except OSError:
        print(f"Could not read parameters from {filename}", file=sys.stderr)
        return None
    with f:
        for line in f:
            parts = line.split()
            if not parts:
                break  # reference: a line sscanf cannot parse ends the read
            try:
                x, y, o = int(parts[0]), int(parts[1]), int(parts[2])
            except (IndexError, ValueError):
                print("Malformed line: obstacle must be 1", file=sys.stderr)
                return None
            if o != 1:
                print("Malformed line: obstacle must be 1", file=sys.stderr)
                return None
            if not (0 <= x < nx and 0 <= y < ny):
                print(f"obstacle ({x},{y}) outside the {nx}x{ny} grid", file=sys.stderr)
                return None
            data[y, x] = 1
    return data


def init_cells(p: Params) -> np.ndarray:
    """Equilibrium at rest, AoS float32[ny][nx][9] (LatticeBoltzmannUtils.hpp:137-157)."""
    d = np.float32(p.density)
    w = np.array([d * np.float32(4.0) / np.float32(9.0)] + [d / np.float32(9.0)] * 4 + [d / np.float32(36.0)] * 4,
                 np.float32)
    return np.broadcast_to(w, (p.ny, p.nx, Q)).copy()


def reynolds_number(p: Params, average_velocity: float) -> float:
    viscosity = np.float32(1.0) / np.float32(6.0) * (np.float32(2.0) / np.float32(p.omega) - np.float32(1.0))
    return float(np.float32(average_velocity) * np.float32(p.reynolds_dim) / viscosity)


def macroscopic(p: Params, obstacles: np.ndarray, cells: np.ndarray):
    """Per-cell (u_x, u_y, |u|, pressure) in fp32 exactly as writeResults computes them."""
    c = cells.astype(np.float32, copy=False)
    rho = np.zeros(c.shape[:2], np.float32)
    for k in range(Q):   # sequential sum, speed order (LatticeBoltzmannUtils.hpp:249-251)
        rho = rho + c[..., k]
    ux = (((c[..., 1] + c[..., 5]) + c[..., 8]) - ((c[..., 3] + c[..., 6]) + c[..., 7])) / rho
    uy = (((c[..., 2] + c[..., 5]) + c[..., 6]) - ((c[..., 4] + c[..., 7]) + c[..., 8])) / rho
    u = np.sqrt(ux * ux + uy * uy, dtype=np.float32)
    pressure = rho * C_SQ
    ob = obstacles.astype(bool)
    ux = np.where(ob, np.float32(0), ux)
    uy = np.where(ob, np.float32(0), uy)
    u = np.where(ob, np.float32(0), u)
    pressure = np.where(ob, np.float32(p.density) * C_SQ, pressure).astype(np.float32)
    return ux, uy, u, pressure


def macroscopic3d(p: Params3D, obstacles: np.ndarray, cells: np.ndarray):
    """Per-cell (u_x, u_y, u_z, |u|, pressure), float32[nz][ny][nx] each, of the AoS D3Q19
    cells float32[nz][ny][nx][19] in fp32 exactly as include/lbm3d_fields_hip.h defines
    them (the expressions of oracle/lbm_oracle3d.c cell3d, sums sequential in the written
    order); an obstacle cell gives +0, +0, +0, +0, density / 3."""
    c = cells.astype(np.float32, copy=False)

    def seq(*ks):
        acc = c[..., ks[0]]
        for k in ks[1:]:
            acc = acc + c[..., k]
        return acc

    with np.errstate(divide="ignore", invalid="ignore"):
        rho = seq(*range(19))
        ux = (seq(1, 5, 7, 10, 16) - seq(2, 6, 8, 11, 15)) / rho
        uy = (seq(3, 5, 8, 12, 18) - seq(4, 6, 7, 13, 17)) / rho
        uz = (seq(9, 10, 11, 12, 13) - seq(14, 15, 16, 17, 18)) / rho
        u = np.sqrt(ux * ux + uy * uy + uz * uz, dtype=np.float32)
    pressure = rho * C_SQ
    ob = np.asarray(obstacles).reshape(rho.shape).astype(bool)
    zero = np.float32(0)
    ux, uy, uz, u = (np.where(ob, zero, f).astype(np.float32) for f in (ux, uy, uz, u))
    pressure = np.where(ob, np.float32(p.density) * C_SQ, pressure).astype(np.float32)
    return ux, uy, uz, u, pressure


# ---- momentum-exchange wall forces (include/lbm_forces_hip.h) ----

# speed vectors (x, y[, z]) in the speed order of lbm_hip.h / lbm3d_hip.h
E2 = ((0, 0), (1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))
E3 = ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (1, 1, 0), (-1, -1, 0), (1, -1, 0), (-1, 1, 0),
      (0, 0, 1), (1, 0, 1), (-1, 0, 1), (0, 1, 1), (0, -1, 1),
      (0, 0, -1), (-1, 0, -1), (1, 0, -1), (0, -1, -1), (0, 1, -1))


def _links(obstacles, vectors):
    ob = np.asarray(obstacles) != 0
    axes = tuple(range(ob.ndim))
    mask = np.zeros(ob.shape, np.uint32)
    for j, e in enumerate(vectors[1:]):
        # neighbour x + e_j, periodic: rolled[x] = ob[x + e]; array axes are (z,) y, x
        nb = np.roll(ob, tuple(-c for c in reversed(e)), axes)
        mask |= np.where(ob & ~nb, np.uint32(1 << j), np.uint32(0))
    return mask


def wall_links(obstacles) -> np.ndarray:
    """uint32[ny][nx]: bit j-1 set iff the cell is blocked and its neighbour along e_j
    (periodic) is not -- link j of include/lbm_forces_hip.h.  Non-zero = wall cell."""
    return _links(np.asarray(obstacles).reshape(np.shape(obstacles)[-2:]), E2)


def wall_links3d(obstacles) -> np.ndarray:
    """uint32[nz][ny][nx] link masks of the D3Q19 lattice (bits 0..17)."""
    return _links(obstacles, E3)


def _gated(links, cells):
    """t_j = link_j ? f_j : +0.f for every speed j (index 0 unused)."""
    c = np.asarray(cells, np.float32)
    zero = np.float32(0)
    return [None] + [np.where((links >> np.uint32(j - 1)) & np.uint32(1), c[..., j], zero).astype(np.float32)
                     for j in range(1, c.shape[-1])]


def _seq(t, *ks):
    acc = t[ks[0]]
    for k in ks[1:]:
        acc = acc + t[k]
    return acc


def wall_force_cells(obstacles, cells):
    """Per-cell (fx, fy), float32[ny][nx] each: the momentum-exchange force on every wall
    cell in fp32 exactly as include/lbm_forces_hip.h defines it, +0 elsewhere."""
    links = wall_links(obstacles)
    t = _gated(links, np.asarray(cells, np.float32).reshape(links.shape + (Q,)))
    two = np.float32(2)
    fx = (_seq(t, 3, 6, 7) - _seq(t, 1, 5, 8)) * two
    fy = (_seq(t, 4, 7, 8) - _seq(t, 2, 5, 6)) * two
    return fx.astype(np.float32), fy.astype(np.float32)


def wall_force_cells3d(obstacles, cells):
    """Per-cell (fx, fy, fz), float32[nz][ny][nx] each, of the D3Q19 lattice."""
    links = wall_links3d(obstacles)
    t = _gated(links, np.asarray(cells, np.float32).reshape(links.shape + (19,)))
    two = np.float32(2)
    fx = (_seq(t, 2, 6, 8, 11, 15) - _seq(t, 1, 5, 7, 10, 16)) * two
    fy = (_seq(t, 4, 6, 7, 13, 17) - _seq(t, 3, 5, 8, 12, 18)) * two
    fz = (_seq(t, 14, 15, 16, 17, 18) - _seq(t, 9, 10, 11, 12, 13)) * two
    return fx.astype(np.float32), fy.astype(np.float32), fz.astype(np.float32)


def _totals(links, comps, labels, nbodies):
    nlinks = np.zeros(links.shape, np.int64)
    for j in range(18):
        nlinks += (links >> np.uint32(j)) & np.uint32(1)
    total = tuple(float(np.sum(c, dtype=np.float64)) for c in comps) + (int(nlinks.sum()),)
    if labels is None:
        return total
    lab = np.asarray(labels).reshape(links.shape)
    if nbodies <= 0 or (lab[links != 0] >= nbodies).any():
        raise ValueError("labels of wall cells must be < nbodies (negative: no body)")
    sel = (links != 0) & (lab >= 0)
    bodies = tuple(np.bincount(lab[sel], weights=c[sel].astype(np.float64), minlength=nbodies) for c in comps)
    bodies += (np.bincount(lab[sel], weights=nlinks[sel], minlength=nbodies).astype(np.int64),)
    return total, bodies


def wall_force(obstacles, cells, labels=None, nbodies=0):
    """(fx, fy, links): the fp64 sums of wall_force_cells over all wall cells and the
    number of links.  With labels (int[ny][nx]; negative = no body) also the per-body
    sums: ((fx, fy, links), (fx[nbodies], fy[nbodies], links[nbodies]))."""
    return _totals(wall_links(obstacles), wall_force_cells(obstacles, cells), labels, nbodies)


def wall_force3d(obstacles, cells, labels=None, nbodies=0):
    """(fx, fy, fz, links) of the D3Q19 lattice; with labels also the per-body sums."""
    return _totals(wall_links3d(obstacles), wall_force_cells3d(obstacles, cells), labels, nbodies)


def label_bodies(obstacles):
    """(labels int32, nbodies): the connected components of the blocked cells, periodic,
    8-connected in 2-D and 26-connected in 3-D (cells that touch by a corner are one
    body), numbered by each body's first cell in row-major order; fluid cells get -1."""
    ob = np.asarray(obstacles) != 0
    axes = tuple(range(ob.ndim))
    n = int(ob.sum())
    labels = np.full(ob.shape, -1, np.int32)
    if n == 0:
        return labels, 0
    ids = np.full(ob.shape, -1, np.int64)
    ids[ob] = np.arange(n)            # row-major rank among the blocked cells
    shifts = [s for s in np.ndindex(*(3,) * ob.ndim) if any(c != 1 for c in s)]
    pairs = []
    for s in shifts:
        nb = np.roll(ids, tuple(1 - c for c in s), axes)[ob]
        pairs.append((np.nonzero(nb >= 0)[0], nb[nb >= 0]))
    lab = np.arange(n)
    while True:   # smallest rank of the neighbourhood, then pointer jumping, until nothing moves
        new = lab.copy()
        for me, other in pairs:
            new[me] = np.minimum(new[me], lab[other])   # each cell once per direction
        while True:
            jump = new[new]
            if np.array_equal(jump, new):
                break
            new = jump
        if np.array_equal(new, lab):
            break
        lab = new
    roots, inv = np.unique(lab, return_inverse=True)   # roots ascend: first cells in row-major order
    labels[ob] = inv.astype(np.int32)
    return labels, int(roots.size)


# ---- time averages: the definition of include/lbm_averages_hip.h in numpy ----

def _moment_pairs(nv):
    """(a, b) of the second-moment sums after the nv + 1 first moments: the velocity
    pairs u_i u_j (i <= j, i outer), then p p -- the order of the header's enums."""
    return [(i, j) for i in range(nv) for j in range(i, nv)] + [(nv, nv)]


def moment_sums(samples, second: bool = True):
    """The fp64 sums Engine.avg_sums() returns.  samples: a sequence of samples in time
    order, each a sequence of float32 arrays (ux, uy[, uz], pressure) as fields() gives
    them.  Returns the list [S_ux, S_uy, (S_uz,) S_p] and, with `second`, the sums of
    products in the header's order: S += (double)a, S_ab += (double)a * (double)b."""
    samples = [[np.asarray(f, np.float32).astype(np.float64) for f in s] for s in samples]
    first = len(samples[0])
    pairs = _moment_pairs(first - 1) if second else []
    sums = [np.zeros(samples[0][0].shape, np.float64) for _ in range(first + len(pairs))]
    for s in samples:
        for k in range(first):
            sums[k] += s[k]
        for k, (a, b) in enumerate(pairs):
            sums[first + k] += s[a] * s[b]
    return sums


def moment_means(sums, n: int):
    """The float32 arrays Engine.mean_fields() returns from the sums of n samples: the
    means (float)(S_a / n), then (if the sums hold them) the central second moments
    (float)(S_ab / n - (S_a / n) * (S_b / n)), every operation in fp64 in that order."""
    sums = [np.asarray(s, np.float64) for s in sums]
    nv = {3: 2, 7: 2, 4: 3, 11: 3}[len(sums)]
    first, dn = nv + 1, np.float64(n)
    out = [(s / dn).astype(np.float32) for s in sums[:first]]
    if len(sums) > first:
        for k, (a, b) in enumerate(_moment_pairs(nv)):
            out.append((sums[first + k] / dn - (sums[a] / dn) * (sums[b] / dn)).astype(np.float32))
    return out


# ---- velocity gradients: the definition of include/lbm_gradients_hip.h in numpy ----

def _central(f, axis):
    """(f[+1] - f[-1]) * 0.5f along `axis`, periodic, in fp32."""
    return ((np.roll(f, -1, axis) - np.roll(f, 1, axis)) * np.float32(0.5)).astype(np.float32)


def velocity_gradients(ux, uy, obstacles):
    """{"vorticity", "divergence", "strain", "q", "s2"}: float32[ny][nx] each, from the
    planar velocities fields() gives -- central periodic differences, every operation in
    fp32 in the order include/lbm_gradients_hip.h writes, obstacle cells +0.  ("s2" = S:S
    is not a field of the C ABI: gradient_stats sums it.)"""
    u, v = (np.asarray(f, np.float32) for f in (ux, uy))
    half, two = np.float32(0.5), np.float32(2)
    gxx, gxy = _central(u, 1), _central(u, 0)
    gyx, gyy = _central(v, 1), _central(v, 0)
    sxy = (gxy + gyx) * half
    diag = (gxx * gxx) + (gyy * gyy)
    s2 = diag + ((sxy * sxy) * two)
    out = {"vorticity": gyx - gxy, "divergence": gxx + gyy, "strain": np.sqrt(s2, dtype=np.float32),
           "q": (diag * np.float32(-0.5)) - (gxy * gyx), "s2": s2}
    ob = np.asarray(obstacles).reshape(u.shape).astype(bool)
    return {k: np.where(ob, np.float32(0), f).astype(np.float32) for k, f in out.items()}


def velocity_gradients3d(ux, uy, uz, obstacles):
    """{"wx", "wy", "wz", "vorticity", "divergence", "strain", "q", "s2"}:
    float32[nz][ny][nx] each, the D3Q19 definition of include/lbm_gradients_hip.h."""
    u, v, w = (np.asarray(f, np.float32) for f in (ux, uy, uz))
    half, two = np.float32(0.5), np.float32(2)
    gxx, gxy, gxz = _central(u, 2), _central(u, 1), _central(u, 0)
    gyx, gyy, gyz = _central(v, 2), _central(v, 1), _central(v, 0)
    gzx, gzy, gzz = _central(w, 2), _central(w, 1), _central(w, 0)
    wx, wy, wz = gzy - gyz, gxz - gzx, gyx - gxy
    sxy, sxz, syz = (gxy + gyx) * half, (gxz + gzx) * half, (gyz + gzy) * half
    diag = ((gxx * gxx) + (gyy * gyy)) + (gzz * gzz)
    s2 = diag + ((((sxy * sxy) + (sxz * sxz)) + (syz * syz)) * two)
    out = {"wx": wx, "wy": wy, "wz": wz,
           "vorticity": np.sqrt(((wx * wx) + (wy * wy)) + (wz * wz), dtype=np.float32),
           "divergence": (gxx + gyy) + gzz, "strain": np.sqrt(s2, dtype=np.float32),
           "q": (diag * np.float32(-0.5)) - (((gxy * gyx) + (gxz * gzx)) + (gyz * gzy)), "s2": s2}
    ob = np.asarray(obstacles).reshape(u.shape).astype(bool)
    return {k: np.where(ob, np.float32(0), f).astype(np.float32) for k, f in out.items()}


def gradient_stats(fields, obstacles):
    """(sum_w2, sum_s2, max_w, max_div) over the fluid cells of the dict
    velocity_gradients / velocity_gradients3d returns: the sums of (double)vorticity^2
    (3-D: ((double)wx*wx + (double)wy*wy) + (double)wz*wz) and of (double)s2 by math.fsum,
    the maxima of |vorticity| and |divergence| as float32."""
    import math
    fluid = ~np.asarray(obstacles).reshape(fields["s2"].shape).astype(bool)
    d = {k: np.asarray(f, np.float32)[fluid].astype(np.float64) for k, f in fields.items()}
    if "wx" in d:
        w2 = (d["wx"] * d["wx"] + d["wy"] * d["wy"]) + d["wz"] * d["wz"]
    else:
        w2 = d["vorticity"] * d["vorticity"]
    if not fluid.any():
        return 0.0, 0.0, np.float32(0), np.float32(0)
    return (math.fsum(w2.tolist()), math.fsum(d["s2"].tolist()),
            np.float32(np.abs(d["vorticity"]).max()), np.float32(np.abs(d["divergence"]).max()))


def read_gradient_state(filename: str, nx: int, ny: int):
    """gradient_state.dat (`x y vorticity divergence strain q obstacle`, y outer) back into
    {"vorticity", "divergence", "strain", "q"}: float32[ny][nx], and "obstacle": uint8."""
    t = np.loadtxt(filename, dtype=np.float64).reshape(ny, nx, 7)
    out = {n: t[..., 2 + i].astype(np.float32) for i, n in enumerate(("vorticity", "divergence", "strain", "q"))}
    out["obstacle"] = t[..., 6].astype(np.uint8)
    return out


# ---- non-equilibrium strain rate: the definition of include/lbm_stress_hip.h in numpy ----

def _neq_coef(omega):
    omega = np.float32(omega)
    omo = np.float32(1) - omega
    if omo == 0:
        raise ValueError("omega = 1: the post-collision lattice carries no non-equilibrium part")
    return (np.float32(-1.5) * omega) / omo


def _neq_finish(n, rho, coef, ob):
    """s_ab = n_ab * (coef / rho), "s2", "strain"; obstacle cells +0.  `n` maps a component
    name to n_ab, diagonal components first (names with two equal letters)."""
    k = coef / rho
    s = {name: v * k for name, v in n.items()}
    diag = [s[a] * s[a] for a in s if a[1] == a[2]]
    off = [s[a] * s[a] for a in s if a[1] != a[2]]
    d, o = diag[0], off[0]
    for t in diag[1:]:
        d = d + t
    for t in off[1:]:
        o = o + t
    s["s2"] = d + (o * np.float32(2))
    s["strain"] = np.sqrt(s["s2"], dtype=np.float32)
    return {name: np.where(ob, np.float32(0), f).astype(np.float32) for name, f in s.items()}


def neq_strain(cells, obstacles, omega):
    """{"sxx", "sxy", "syy", "strain", "s2"}: float32[ny][nx] each, the strain rate from
    the non-equilibrium second moment of the stored (post-collision) AoS cells
    float32[ny][nx][9] -- every operation in fp32 in the order include/lbm_stress_hip.h
    writes, obstacle cells +0.  ("s2" = S:S is not a field of the C ABI: strain_stats sums it.)"""
    c = np.asarray(cells, np.float32)
    ob = np.asarray(obstacles).reshape(c.shape[:-1]).astype(bool)
    coef = _neq_coef(omega)
    t = [c[..., k] for k in range(Q)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rho = _seq(t, *range(Q))
        ux = (_seq(t, 1, 5, 8) - _seq(t, 3, 6, 7)) / rho
        uy = (_seq(t, 2, 5, 6) - _seq(t, 4, 7, 8)) / rho
        p = rho * C_SQ
        n = {"sxx": (_seq(t, 1, 3, 5, 6, 7, 8) - p) - ((rho * ux) * ux),
             "syy": (_seq(t, 2, 4, 5, 6, 7, 8) - p) - ((rho * uy) * uy),
             "sxy": ((t[5] + t[7]) - (t[6] + t[8])) - ((rho * ux) * uy)}
        return _neq_finish(n, rho, coef, ob)


def neq_strain3d(cells, obstacles, omega):
    """{"sxx", "syy", "szz", "sxy", "sxz", "syz", "strain", "s2"}: float32[nz][ny][nx] each,
    the D3Q19 definition of include/lbm_stress_hip.h from the AoS cells float32[nz][ny][nx][19]."""
    c = np.asarray(cells, np.float32)
    ob = np.asarray(obstacles).reshape(c.shape[:-1]).astype(bool)
    coef = _neq_coef(omega)
    t = [c[..., k] for k in range(19)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rho = _seq(t, *range(19))
        ux = (_seq(t, 1, 5, 7, 10, 16) - _seq(t, 2, 6, 8, 11, 15)) / rho
        uy = (_seq(t, 3, 5, 8, 12, 18) - _seq(t, 4, 6, 7, 13, 17)) / rho
        uz = (_seq(t, 9, 10, 11, 12, 13) - _seq(t, 14, 15, 16, 17, 18)) / rho
        p = rho * C_SQ
        n = {"sxx": (_seq(t, 1, 2, 5, 6, 7, 8, 10, 11, 15, 16) - p) - ((rho * ux) * ux),
             "syy": (_seq(t, 3, 4, 5, 6, 7, 8, 12, 13, 17, 18) - p) - ((rho * uy) * uy),
             "szz": (_seq(t, *range(9, 19)) - p) - ((rho * uz) * uz),
             "sxy": ((t[5] + t[6]) - (t[7] + t[8])) - ((rho * ux) * uy),
             "sxz": ((t[10] + t[15]) - (t[11] + t[16])) - ((rho * ux) * uz),
             "syz": ((t[12] + t[17]) - (t[13] + t[18])) - ((rho * uy) * uz)}
        return _neq_finish(n, rho, coef, ob)


def _near_wall(obstacles, vectors):
    ob = np.asarray(obstacles) != 0
    axes = tuple(range(ob.ndim))
    near = np.zeros(ob.shape, bool)
    for e in vectors[1:]:
        near |= np.roll(ob, tuple(-c for c in reversed(e)), axes)   # rolled[x] = ob[x + e], periodic
    return near & ~ob


def near_wall(obstacles) -> np.ndarray:
    """bool[ny][nx]: the fluid cells with at least one blocked neighbour among the 8 of the
    D2Q9 lattice, periodic over the full domain (include/lbm_stress_hip.h)."""
    return _near_wall(np.asarray(obstacles).reshape(np.shape(obstacles)[-2:]), E2)


def near_wall3d(obstacles) -> np.ndarray:
    """bool[nz][ny][nx]: the same over the 18 neighbours of the D3Q19 lattice."""
    return _near_wall(obstacles, E3)


def strain_stats(fields, obstacles, near):
    """(sum_s2, max_strain, wall_cells, sum_wall_strain, max_wall_strain) of the dict
    neq_strain / neq_strain3d returns: over the fluid cells the sum of (double)s2 by
    math.fsum and the largest strain, over the near-wall cells `near` their number, the
    sum of (double)strain by math.fsum and the largest strain (float32; 0 over no cell)."""
    import math
    shape = fields["s2"].shape
    fluid = ~np.asarray(obstacles).reshape(shape).astype(bool)
    near = np.asarray(near).reshape(shape).astype(bool) & fluid
    s2 = np.asarray(fields["s2"], np.float32)[fluid].astype(np.float64)
    strain = np.asarray(fields["strain"], np.float32)
    sw = strain[near]
    return (math.fsum(s2.tolist()), np.float32(strain[fluid].max() if fluid.any() else 0), int(near.sum()),
            math.fsum(sw.astype(np.float64).tolist()), np.float32(sw.max() if sw.size else 0))


def read_stress_state(filename: str, nx: int, ny: int):
    """stress_state.dat (`x y sxx sxy syy strain near_wall obstacle`, y outer) back into
    {"sxx", "sxy", "syy", "strain"}: float32[ny][nx], and "near_wall", "obstacle": uint8."""
    t = np.loadtxt(filename, dtype=np.float64).reshape(ny, nx, 8)
    out = {n: t[..., 2 + i].astype(np.float32) for i, n in enumerate(("sxx", "sxy", "syy", "strain"))}
    out["near_wall"] = t[..., 6].astype(np.uint8)
    out["obstacle"] = t[..., 7].astype(np.uint8)
    return out


# ---- binned sums (include/lbm_binned_hip.h) ----

# index order of LBM_BIN_* / LBM3D_BIN_*
BIN_FIELDS = ("rho", "jx", "jy", "ux", "uy", "speed", "uxux", "uxuy", "uyuy")
BIN_FIELDS3D = ("rho", "jx", "jy", "jz", "ux", "uy", "uz", "speed",
                "uxux", "uxuy", "uxuz", "uyuy", "uyuz", "uzuz")


def _bin_products(t, names):
    for a in range(len(names)):
        for b in range(a, len(names)):
            t[names[a] + names[b]] = t[names[a]] * t[names[b]]   # float64: exact


def binned_terms(p: Params, obstacles: np.ndarray, cells: np.ndarray):
    """{name: float64[ny][nx]} of the per-cell terms the D2Q9 binned sums add, in
    BIN_FIELDS order: (double) of macroscopic()'s fp32 ux, uy, speed, of its sequential
    fp32 density and of the fp32 numerators jx, jy it divides by the density, and the
    fp64 products of the velocities.  +0 on obstacle cells."""
    c = cells.astype(np.float32, copy=False)
    ux, uy, u, _ = macroscopic(p, obstacles, cells)
    rho = np.zeros(c.shape[:2], np.float32)
    for k in range(Q):
        rho = rho + c[..., k]
    jx = ((c[..., 1] + c[..., 5]) + c[..., 8]) - ((c[..., 3] + c[..., 6]) + c[..., 7])
    jy = ((c[..., 2] + c[..., 5]) + c[..., 6]) - ((c[..., 4] + c[..., 7]) + c[..., 8])
    fluid = ~np.asarray(obstacles).reshape(rho.shape).astype(bool)
    t = {n: np.where(fluid, f, np.float32(0)).astype(np.float64)
         for n, f in (("rho", rho), ("jx", jx), ("jy", jy), ("ux", ux), ("uy", uy), ("speed", u))}
    _bin_products(t, ("ux", "uy"))
    return {n: t[n] for n in BIN_FIELDS}


def binned_terms3d(p: Params3D, obstacles: np.ndarray, cells: np.ndarray):
    """The same for D3Q19: {name: float64[nz][ny][nx]} in BIN_FIELDS3D order, from
    macroscopic3d()'s values."""
    c = cells.astype(np.float32, copy=False)

    def seq(*ks):
        acc = c[..., ks[0]]
        for k in ks[1:]:
            acc = acc + c[..., k]
        return acc

    ux, uy, uz, u, _ = macroscopic3d(p, obstacles, cells)
    rho = seq(*range(19))
    jx = seq(1, 5, 7, 10, 16) - seq(2, 6, 8, 11, 15)
    jy = seq(3, 5, 8, 12, 18) - seq(4, 6, 7, 13, 17)
    jz = seq(9, 10, 11, 12, 13) - seq(14, 15, 16, 17, 18)
    fluid = ~np.asarray(obstacles).reshape(rho.shape).astype(bool)
    t = {n: np.where(fluid, f, np.float32(0)).astype(np.float64)
         for n, f in (("rho", rho), ("jx", jx), ("jy", jy), ("jz", jz), ("ux", ux), ("uy", uy), ("uz", uz),
                      ("speed", u))}
    _bin_products(t, ("ux", "uy", "uz"))
    return {n: t[n] for n in BIN_FIELDS3D}


def bin_reduce(a: np.ndarray, bins, exact: bool = True) -> np.ndarray:
    """Sum `a` over the cells of each bin.  bins = (bw, bh[, bd]) in cells along x, y[, z];
    `a` is indexed [[z]][y][x].  Bins tile the array from its first cell and the last one
    along an axis may be ragged.  exact: math.fsum per bin (the exactly rounded sum of
    float64 terms, from +0.0: a sum of value zero is +0.0 whatever the signs of its zero
    terms); otherwise numpy's sum in a's own type (integer counts)."""
    import math
    a = np.asarray(a)
    sizes = tuple(int(b) for b in bins)[::-1]        # slowest axis first, as a's
    if len(sizes) != a.ndim or any(b < 1 for b in sizes):
        raise ValueError("one bin size >= 1 per axis")
    counts = tuple(-(-n // b) for n, b in zip(a.shape, sizes))
    out = np.zeros(counts, np.float64 if exact else a.dtype)
    if all(b == 1 for b in sizes):                    # one-cell bins: the cell itself
        out[...] = a
        return out + 0.0 if exact else out
    for idx in np.ndindex(*counts):
        block = a[tuple(slice(i * b, (i + 1) * b) for i, b in zip(idx, sizes))]
        out[idx] = math.fsum(block.ravel().tolist()) + 0.0 if exact else block.sum()
    return out


def _binned(terms, obstacles, bins):
    out = {n: bin_reduce(t, bins) for n, t in terms.items()}
    shape = next(iter(terms.values())).shape
    fluid = (~np.asarray(obstacles).reshape(shape).astype(bool)).astype(np.int64)
    out["fluid"] = bin_reduce(fluid, bins, exact=False)
    return out


def binned_sums(p: Params, obstacles: np.ndarray, cells: np.ndarray, bw: int, bh: int):
    """The definition of lbm_store_binned restated: {name: float64[nby][nbx]} for the
    BIN_FIELDS -- per bin the exactly rounded sum (math.fsum) of binned_terms() over its
    fluid cells, +0 over none -- and "fluid": int64, the fluid cells per bin."""
    return _binned(binned_terms(p, obstacles, cells), obstacles, (bw, bh))


def binned_sums3d(p: Params3D, obstacles: np.ndarray, cells: np.ndarray, bw: int, bh: int, bd: int):
    """The same for D3Q19 (lbm3d_store_binned): float64[nbz][nby][nbx] per BIN_FIELDS3D
    name, and "fluid"."""
    return _binned(binned_terms3d(p, obstacles, cells), obstacles, (bw, bh, bd))


def binned_means(sums):
    """{name: sum / fluid} of a dict binned_sums / Engine.binned returns (0 where a bin
    holds no fluid cell); "fluid" is passed through."""
    fluid = np.asarray(sums["fluid"])
    out = {}
    for n, s in sums.items():
        if n == "fluid":
            out[n] = fluid
            continue
        s = np.asarray(s, np.float64)
        out[n] = np.divide(s, fluid, out=np.zeros_like(s), where=fluid != 0)
    return out


def read_binned_state(filename: str, nbx: int, nby: int):
    """binned_state.dat (`bx by fluid` and the nine BIN_FIELDS sums, by outer) back into
    {name: float64[nby][nbx]} and "fluid": int64."""
    t = np.loadtxt(filename, dtype=np.float64).reshape(nby, nbx, 3 + len(BIN_FIELDS))
    out = {n: t[..., 3 + i].copy() for i, n in enumerate(BIN_FIELDS)}
    out["fluid"] = t[..., 2].astype(np.int64)
    return out


# ---- Lagrangian tracers and point probes (include/lbm_tracers_hip.h) ----
# float64 numpy restatements of the header's definition: every operation is one
# numpy ufunc, so each is rounded once, in the header's order.

TRACER_SCHEMES = {"euler": 0, "heun": 1}


def tracer_wrap(v, n: int) -> np.ndarray:
    """wrap(v, n): v - n * floor(v / n), and 0 wherever that is not in [0, n) (NaN, Inf)."""
    v = np.asarray(v, np.float64)
    n = np.float64(n)
    with np.errstate(all="ignore"):
        r = v - n * np.floor(v / n)
    return np.where((r >= 0.0) & (r < n), r, np.float64(0.0))


def _tracer_split(x, n: int):
    x = np.asarray(x, np.float64)
    i0 = np.floor(x).astype(np.int64)
    t = x - i0.astype(np.float64)
    i1 = np.where(i0 + 1 == n, 0, i0 + 1)
    return i0, i1, t


def _tracer_lerp(a, b, t):
    with np.errstate(all="ignore"):
        return a + t * (b - a)


def tracer_interp(field, x, y) -> np.ndarray:
    """The [ny][nx] field (fp32 values, widened to float64) interpolated bilinearly at the
    points (x, y) in cell units, periodic: lbm_tracer_sample / lbm_tracer_sample_ref."""
    f = np.asarray(field).astype(np.float64)
    ny, nx = f.shape
    i0, i1, tx = _tracer_split(x, nx)
    j0, j1, ty = _tracer_split(y, ny)
    lo = _tracer_lerp(f[j0, i0], f[j0, i1], tx)
    hi = _tracer_lerp(f[j1, i0], f[j1, i1], tx)
    return _tracer_lerp(lo, hi, ty)


def tracer_interp3d(field, x, y, z) -> np.ndarray:
    """The same for a [nz][ny][nx] field: along x first, then y, then z."""
    f = np.asarray(field).astype(np.float64)
    nz, ny, nx = f.shape
    i0, i1, tx = _tracer_split(x, nx)
    j0, j1, ty = _tracer_split(y, ny)
    k0, k1, tz = _tracer_split(z, nz)
    planes = []
    for k in (k0, k1):
        lo = _tracer_lerp(f[k, j0, i0], f[k, j0, i1], tx)
        hi = _tracer_lerp(f[k, j1, i0], f[k, j1, i1], tx)
        planes.append(_tracer_lerp(lo, hi, ty))
    return _tracer_lerp(planes[0], planes[1], tz)


def _tracer_scheme(scheme) -> int:
    if isinstance(scheme, str):
        if scheme not in TRACER_SCHEMES:
            raise ValueError(f"scheme is one of {tuple(TRACER_SCHEMES)}; got {scheme!r}")
        return TRACER_SCHEMES[scheme]
    if int(scheme) not in TRACER_SCHEMES.values():
        raise ValueError(f"scheme is one of {tuple(TRACER_SCHEMES)} (0, 1); got {scheme!r}")
    return int(scheme)


def _tracer_advance(fields, interp, pos, dt, scheme):
    heun = _tracer_scheme(scheme) == 1
    dt = np.float64(dt)
    extent = np.shape(fields[0])[::-1]                    # (nx, ny[, nz])
    pos = [np.asarray(c, np.float64) for c in pos]
    with np.errstate(all="ignore"):
        k1 = [interp(f, *pos) for f in fields]
        if not heun:
            return tuple(tracer_wrap(c + dt * k, n) for c, k, n in zip(pos, k1, extent))
        mid = [tracer_wrap(c + dt * k, n) for c, k, n in zip(pos, k1, extent)]
        k2 = [interp(f, *mid) for f in fields]
        half = np.float64(0.5) * dt
        return tuple(tracer_wrap(c + half * (a + b), n) for c, a, b, n in zip(pos, k1, k2, extent))


def tracer_advance(ux, uy, x, y, dt, scheme="heun"):
    """(x', y') after one advance by dt in the frozen [ny][nx] velocity fields ux, uy
    (lbm_tracer_advance / lbm_tracer_advance_ref); scheme "euler" / "heun" or 0 / 1."""
    return _tracer_advance((ux, uy), tracer_interp, (x, y), dt, scheme)


def tracer_advance3d(ux, uy, uz, x, y, z, dt, scheme="heun"):
    """(x', y', z') for [nz][ny][nx] fields (lbm3d_tracer_advance / _ref)."""
    return _tracer_advance((ux, uy, uz), tracer_interp3d, (x, y, z), dt, scheme)


def _tracer_nearest(x, n: int):
    i = np.floor(np.asarray(x, np.float64) + np.float64(0.5)).astype(np.int64)
    return np.where(i == n, 0, i)


def tracer_blocked(obstacles, x, y) -> np.ndarray:
    """uint8[n]: 1 where the nearest cell of the point is an obstacle (lbm_tracer_store)."""
    o = np.asarray(obstacles)
    ny, nx = o.shape
    return (o[_tracer_nearest(y, ny), _tracer_nearest(x, nx)] != 0).astype(np.uint8)


def tracer_blocked3d(obstacles, x, y, z) -> np.ndarray:
    o = np.asarray(obstacles)
    nz, ny, nx = o.shape
    return (o[_tracer_nearest(z, nz), _tracer_nearest(y, ny), _tracer_nearest(x, nx)] != 0).astype(np.uint8)


def read_tracers(filename: str):
    """tracers.dat (`id x y blocked`, positions in %.17g) -> (x, y float64[n], blocked uint8[n]);
    the positions through float() of the text: the runner's doubles, bit for bit."""
    x, y, b = [], [], []
    with open(filename, "r") as f:
        for line in f:
            t = line.split()
            if not t:
                continue
            x.append(float(t[1]))
            y.append(float(t[2]))
            b.append(int(t[3]))
    return np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(b, np.uint8)


# ---- passive scalar (include/lbm_scalar_hip.h) ----
#
# The header's definition in fp32 numpy, one ufunc per operation so that every
# operation is rounded on its own.  Populations are planar float32[5][ny][nx]
# (D2Q5) or float32[7][nz][ny][nx] (D3Q7).  The tables below are read at call
# time: a test plants an error by replacing one.

SCALAR_W = (np.float32(1) / np.float32(3), np.float32(1) / np.float32(6))     # begin / equilibrium weights: rest, moving
SCALAR_W3D = (np.float32(0.25), np.float32(0.125))
SCALAR_OPP = (0, 3, 4, 1, 2)
SCALAR_OPP3D = (0, 2, 1, 4, 3, 6, 5)
# per moving speed: (velocity component, array axis it moves along, sign)
SCALAR_SPEEDS = ((0, 1, +1), (1, 0, +1), (0, 1, -1), (1, 0, -1))                          # E N W S
SCALAR_SPEEDS3D = ((0, 2, +1), (0, 2, -1), (1, 1, +1), (1, 1, -1), (2, 0, +1), (2, 0, -1))   # +x -x +y -y +z -z


def scalar_diffusivity(omega_s, dims: int = 2) -> float:
    """D = (1 / omega_s - 1/2) / 3 (2-D) or / 4 (3-D)."""
    return (1.0 / float(omega_s) - 0.5) / (3.0 if dims == 2 else 4.0)


def _scalar_init(phi0, w, q):
    phi0 = np.ascontiguousarray(phi0, np.float32)
    moving = phi0 * w[1]
    return np.stack([phi0 * w[0]] + [moving] * (q - 1))


def scalar_init(phi0) -> np.ndarray:
    """float32[5][ny][nx]: the begin state of phi0 (lbm_scalar_begin)."""
    return _scalar_init(phi0, SCALAR_W, 5)


def scalar_init3d(phi0) -> np.ndarray:
    """float32[7][nz][ny][nx]: lbm3d_scalar_begin."""
    return _scalar_init(phi0, SCALAR_W3D, 7)


def scalar_phi(g) -> np.ndarray:
    """phi of every cell: the populations summed in speed order (either lattice)."""
    g = np.asarray(g, np.float32)
    phi = g[0]
    for k in range(1, g.shape[0]):
        phi = phi + g[k]
    return phi


scalar_phi3d = scalar_phi


def _scalar_step(g, u, obst, omega_s, w, opp, speeds, c):
    g = np.asarray(g, np.float32)
    u = [np.asarray(a, np.float32) for a in u]
    om, c = np.float32(omega_s), np.float32(c)
    # p_k: what arrives along speed k, from the periodic neighbour against it
    p = [g[0]] + [np.roll(g[k + 1], sign, axis=axis) for k, (_, axis, sign) in enumerate(speeds)]
    phi = p[0]
    for k in range(1, len(p)):
        phi = phi + p[k]
    t = phi * w[1]
    a = [t * (c * uc) for uc in u]
    e = [phi * w[0]] + [(t + a[comp]) if sign > 0 else (t - a[comp]) for comp, _, sign in speeds]
    blocked = np.asarray(obst) != 0
    return np.stack([np.where(blocked, p[opp[k]], p[k] + om * (e[k] - p[k])) for k in range(len(p))])


def scalar_step(g, ux, uy, obst, omega_s) -> np.ndarray:
    """One D2Q5 step over the frozen velocity field (lbm_scalar_advance(1) without the fixed list /
    lbm_scalar_step_ref): ux, uy float32[ny][nx] as Engine.fields() gives them, obst [ny][nx]."""
    return _scalar_step(g, (ux, uy), obst, omega_s, SCALAR_W, SCALAR_OPP, SCALAR_SPEEDS, 3)


def scalar_step3d(g, ux, uy, uz, obst, omega_s) -> np.ndarray:
    """One D3Q7 step (lbm3d_scalar_advance(1) / lbm3d_scalar_step_ref)."""
    return _scalar_step(g, (ux, uy, uz), obst, omega_s, SCALAR_W3D, SCALAR_OPP3D, SCALAR_SPEEDS3D, 4)


def _scalar_apply_fixed(g, idx, value, w):
    g = np.array(g, np.float32)
    value = np.asarray(value, np.float32).reshape(-1)
    g[(0,) + idx] = value * w[0]
    moving = value * w[1]
    for k in range(1, g.shape[0]):
        g[(k,) + idx] = moving
    return g


def scalar_apply_fixed(g, x, y, value) -> np.ndarray:
    """A copy of g with the listed cells set to the begin state of `value` (lbm_scalar_set_fixed)."""
    return _scalar_apply_fixed(g, (np.asarray(y, np.int64), np.asarray(x, np.int64)), value, SCALAR_W)


def scalar_apply_fixed3d(g, x, y, z, value) -> np.ndarray:
    return _scalar_apply_fixed(g, (np.asarray(z, np.int64), np.asarray(y, np.int64), np.asarray(x, np.int64)), value,
                               SCALAR_W3D)


def scalar_stats(g, obst):
    """(total, min, max) of lbm_scalar_stats: the float64 sum of every cell's float32 phi (math.fsum:
    the exact sum, which the device's fold approaches within its bound) and the extremes over the
    fluid cells (+inf, -inf when there is none).  Either lattice.  Non-finite scalars as the header
    states them: a NaN phi of a fluid cell is left out of the extremes (fmaxf drops it), infinities
    take part; the total is the IEEE sum, NaN with a NaN anywhere or with infinities of both signs."""
    import math
    phi = scalar_phi(g)
    fluid = phi[np.asarray(obst) == 0]
    terms = phi.astype(np.float64).ravel()
    if np.isfinite(terms).all():
        total = math.fsum(terms.tolist())
    else:
        with np.errstate(invalid="ignore"):
            total = float(np.sum(terms))     # NaN, or the one infinity the non-finite terms share
    return total, np.float32(np.fmin.reduce(fluid, initial=np.inf)), np.float32(np.fmax.reduce(fluid, initial=-np.inf))


scalar_stats3d = scalar_stats


# ---- Boussinesq buoyancy (include/lbm_thermal_hip.h) ----
#
# The kick of the scalar on the flow in fp32 numpy, one ufunc per operation.  The
# tables are read at call time: a test plants an error by replacing one.

KICK_W = (np.float32(1) / np.float32(3), np.float32(1) / np.float32(12))      # 3 w_k of D2Q9: axis, diagonal speeds
KICK_W3D = (np.float32(1) / np.float32(6), np.float32(1) / np.float32(12))    # of D3Q19
# per opposite pair (plus speed, minus speed, terms of the increment): one term (component,) takes the axis
# weight, two terms ((sign, component), (sign, component)) are diagonal-weight products added in that order
KICK_PAIRS = ((1, 3, (0,)), (2, 4, (1,)), (5, 7, ((+1, 0), (+1, 1))), (6, 8, ((+1, 1), (-1, 0))))
KICK_PAIRS3D = ((1, 2, (0,)), (3, 4, (1,)), (9, 14, (2,)),
                (5, 6, ((+1, 0), (+1, 1))), (7, 8, ((+1, 0), (-1, 1))),
                (10, 15, ((+1, 0), (+1, 2))), (11, 16, ((+1, 2), (-1, 0))),
                (12, 17, ((+1, 1), (+1, 2))), (13, 18, ((+1, 2), (-1, 1))))


def _buoyancy_increments(phi, density, s, phi_ref, w, pairs, q):
    phi = np.asarray(phi, np.float32)
    d = phi - np.float32(phi_ref)
    return _pair_increments([(np.float32(density) * np.float32(c)) * d for c in s], w, pairs, q)


def _pair_increments(j, w, pairs, q):
    """[None, d1 .. d(q-1)] of the momentum j = [jx, jy[, jz]] (float32 arrays): the part the buoyancy and the
    forcing zones share."""
    a = [jc * w[0] for jc in j]
    b = [jc * w[1] for jc in j]
    inc = [None] * q
    for plus, minus, terms in pairs:
        if len(terms) == 1:
            v = a[terms[0]]
        else:
            (s1, c1), (s2, c2) = terms
            assert s1 > 0
            v = (b[c1] + b[c2]) if s2 > 0 else (b[c1] - b[c2])
        inc[plus], inc[minus] = v, -v
    return inc


def buoyancy_increments(phi, density, s, phi_ref=0.0):
    """[None, d1 .. d8]: what lbm_scalar_buoyancy adds to speed k of a fluid cell whose scalar is phi
    (float32 arrays of phi's shape; the rest speed gets nothing): 3 w_k density (c_k . s) (phi - phi_ref),
    the increment of opp(k) the exact negative of that of k."""
    if len(s) != 2:
        raise ValueError("s = (sx, sy)")
    return _buoyancy_increments(phi, density, s, phi_ref, KICK_W, KICK_PAIRS, 9)


def buoyancy_increments3d(phi, density, s, phi_ref=0.0):
    """[None, d1 .. d18] of lbm3d_scalar_buoyancy."""
    if len(s) != 3:
        raise ValueError("s = (sx, sy, sz)")
    return _buoyancy_increments(phi, density, s, phi_ref, KICK_W3D, KICK_PAIRS3D, 19)


def _buoyancy_kick(cells, g, obst, inc_of, s, q):
    cells = np.array(cells, np.float32)
    if cells.shape[-1] != q or np.asarray(g).shape[1:] != cells.shape[:-1]:
        raise ValueError("cells AoS [...][q] and g planar [qs][...] of one domain")
    if all(np.float32(c) == 0 for c in s):
        return cells                     # no launch: every bit stays (x + 0 would turn a -0 into +0)
    inc = inc_of(scalar_phi(g))
    fluid = np.asarray(obst).reshape(cells.shape[:-1]) == 0
    for k in range(1, q):
        cells[..., k] = np.where(fluid, cells[..., k] + inc[k], cells[..., k])
    return cells


def buoyancy_kick(cells, g, obst, density, s, phi_ref=0.0) -> np.ndarray:
    """A kicked copy of the AoS cells float32[ny][nx][9]: lbm_scalar_buoyancy(s, phi_ref) on a handle of
    that density whose scalar populations are g (float32[5][ny][nx]).  Obstacle cells keep their bits."""
    return _buoyancy_kick(cells, g, obst, lambda phi: buoyancy_increments(phi, density, s, phi_ref), s, 9)


def buoyancy_kick3d(cells, g, obst, density, s, phi_ref=0.0) -> np.ndarray:
    """lbm3d_scalar_buoyancy: cells float32[nz][ny][nx][19], g float32[7][nz][ny][nx]."""
    return _buoyancy_kick(cells, g, obst, lambda phi: buoyancy_increments3d(phi, density, s, phi_ref), s, 19)


def rayleigh_number(accel, dphi, height, omega, omega_s, dims: int = 2) -> float:
    """Ra = accel dphi height^3 / (nu D): accel the buoyancy acceleration per unit of scalar and step,
    dphi the scalar difference across `height` cells, nu = (1 / omega - 1/2) / 3 and D the scalar's
    diffusivity (scalar_diffusivity)."""
    nu = (1.0 / float(omega) - 0.5) / 3.0
    return float(accel) * float(dphi) * float(height) ** 3 / (nu * scalar_diffusivity(omega_s, dims))


# ---- forcing zones (include/lbm_forcing_hip.h) ----
#
# One zone applied to AoS cells in fp32 numpy, one ufunc per operation.  The pair tables are the
# buoyancy's (KICK_W, KICK_PAIRS); they, the momentum tables and forcing_momentum are read at call
# time: a test plants an error by replacing one.

# per component (speeds added, speeds subtracted), each group summed left to right: cell_momentum / cell3_momentum
FORCING_J = (((1, 5, 8), (3, 6, 7)), ((2, 5, 6), (4, 7, 8)))
FORCING_J3D = (((1, 5, 7, 10, 16), (2, 6, 8, 11, 15)), ((3, 5, 8, 12, 18), (4, 6, 7, 13, 17)),
               ((9, 10, 11, 12, 13), (14, 15, 16, 17, 18)))


def forcing_momentum(l, rho, ut, j, g):
    """m = (l * ((rho * ut) - j)) + (rho * g): what a zone adds to one momentum component of a cell."""
    return (l * ((rho * ut) - j)) + (rho * g)


def _forcing_kick(cells, obst, box, coef, n, dims, w, pairs, jtable):
    q = 9 if dims == 2 else 19
    cells = np.array(cells, np.float32)
    if cells.ndim != dims + 1 or cells.shape[-1] != q or np.asarray(obst).shape != cells.shape[:-1]:
        raise ValueError("cells AoS [...][q] and obst [...] of one domain")
    box = [int(v) for v in box]
    if len(box) != 2 * dims or len(coef) != 1 + 2 * dims:
        raise ValueError("box = (x0, y0[, z0], w, h[, d]) and coef = (lam, ut.., f..)")
    origin, ext = box[:dims][::-1], box[dims:][::-1]                           # slowest axis first
    if any(e < 1 or o < 0 or o + e > s for o, e, s in zip(origin, ext, cells.shape)):
        raise ValueError("the box is not empty and lies inside the domain")
    n = np.float32(n)
    if not (np.isfinite(n) and n >= 0):
        raise ValueError("n is finite and not negative")
    k = [np.broadcast_to(np.asarray(c, np.float32), ext) for c in coef]
    if not all(np.isfinite(c).all() for c in k) or (k[0] < 0).any():
        raise ValueError("finite coefficients and lam >= 0")
    terms = np.zeros(tuple(ext) + (dims,), np.float32)
    if n == 0:
        return cells, terms                       # no launch: every bit stays
    sl = tuple(slice(o, o + e) for o, e in zip(origin, ext))
    c = cells[sl]                                 # a view: the box is kicked in place in the copy
    with np.errstate(all="ignore"):               # hard states: Inf and NaN under obstacles are selected away
        l = np.minimum(n * k[0], np.float32(1))
        g = [n * k[1 + dims + i] for i in range(dims)]
        idle = (np.asarray(obst)[sl] != 0) | ((l == 0) & np.logical_and.reduce([gi == 0 for gi in g]))
        rho = c[..., 0]
        for i in range(1, q):
            rho = rho + c[..., i]
        m = []
        for i, (plus, minus) in enumerate(jtable):
            a = c[..., plus[0]]
            for s in plus[1:]:
                a = a + c[..., s]
            b = c[..., minus[0]]
            for s in minus[1:]:
                b = b + c[..., s]
            m.append(forcing_momentum(l, rho, k[1 + i], a - b, g[i]))
        inc = _pair_increments(m, w, pairs, q)
        for s in range(1, q):
            c[..., s] = np.where(idle, c[..., s], c[..., s] + inc[s])
        for i in range(dims):
            terms[..., i] = np.where(idle, np.float32(0), m[i])
    return cells, terms


def forcing_kick(cells, obst, box, coef, n):
    """(kicked copy of the AoS cells float32[ny][nx][9], terms float32[h][w][2]): one forcing zone applied once,
    lbm_forcing_apply(n) on a handle whose only zone is box = (x0, y0, w, h) with coef = (lam, utx, uty, fx, fy),
    each a number or an array [h][w].  terms holds (mx, my) of every cell of the box, zeros where it is idle
    (obstacle, or no drag and no force); their sum is the impulse.  Idle cells keep their bits."""
    return _forcing_kick(cells, obst, box, coef, n, 2, KICK_W, KICK_PAIRS, FORCING_J)


def forcing_kick3d(cells, obst, box, coef, n):
    """lbm3d_forcing_apply: cells float32[nz][ny][nx][19], box = (x0, y0, z0, w, h, d),
    coef = (lam, utx, uty, utz, fx, fy, fz), arrays [d][h][w], terms float32[d][h][w][3]."""
    return _forcing_kick(cells, obst, box, coef, n, 3, KICK_W3D, KICK_PAIRS3D, FORCING_J3D)


# ---- sub-grid model (include/lbm_sgs_hip.h) ----
#
# One application on AoS cells in fp32 numpy, one ufunc per operation.  SGS_SMAG_K, SGS_RESCALED[3D] and
# sgs_factor are read at call time: a test plants an error by replacing one.

SGS_MODES = {"smagorinsky": 1, "omega": 2}
SGS_SMAG_K = np.float32(25.455844)                       # 18 sqrt 2
SGS_RESCALED = tuple(range(9))                           # the speeds an application rescales: all of them
SGS_RESCALED3D = tuple(range(19))
# (first speed, second speed, weight: 1 axis / 2 diagonal, velocity along the first from (ux, uy[, uz]))
SGS_PAIRS = ((1, 3, 1, lambda u: u[0]), (2, 4, 1, lambda u: u[1]),
             (5, 7, 2, lambda u: u[0] + u[1]), (6, 8, 2, lambda u: (-u[0]) + u[1]))
SGS_PAIRS3D = ((1, 2, 1, lambda u: u[0]), (3, 4, 1, lambda u: u[1]), (5, 6, 2, lambda u: u[0] + u[1]),
               (7, 8, 2, lambda u: u[0] - u[1]), (9, 14, 1, lambda u: u[2]), (10, 15, 2, lambda u: u[0] + u[2]),
               (11, 16, 2, lambda u: (-u[0]) + u[2]), (12, 17, 2, lambda u: u[1] + u[2]),
               (13, 18, 2, lambda u: (-u[1]) + u[2]))
# second moment of q: the diagonal sums (sequential) and the off-diagonal ((a + b) - (c + d))
SGS_MOMENT = (((1, 3, 5, 6, 7, 8), (2, 4, 5, 6, 7, 8)), ((5, 7, 6, 8),))
SGS_MOMENT3D = (((1, 2, 5, 6, 7, 8, 10, 11, 15, 16), (3, 4, 5, 6, 7, 8, 12, 13, 17, 18), tuple(range(9, 19))),
                ((5, 6, 7, 8), (10, 15, 11, 16), (12, 17, 13, 18)))


def sgs_factor(omega0, omega_eff, omo):
    """d = (w0 - w_eff) / (1 - w0): the share of its stored non-equilibrium part a cell gains."""
    return (omega0 - omega_eff) / omo


def sgs_mode(mode) -> int:
    m = SGS_MODES.get(mode, mode) if isinstance(mode, str) else mode
    if m not in (1, 2):
        raise ValueError(f"mode is one of {sorted(SGS_MODES)} (or 1, 2)")
    return int(m)


def _sgs_filter(cells, obst, omega, mode, coef, n, dims, with_idle=False):
    q9, pairs, moment, rescaled = ((9, SGS_PAIRS, SGS_MOMENT, SGS_RESCALED) if dims == 2
                                   else (19, SGS_PAIRS3D, SGS_MOMENT3D, SGS_RESCALED3D))
    cells = np.array(cells, np.float32)
    shape = cells.shape[:-1]
    if cells.ndim != dims + 1 or cells.shape[-1] != q9 or np.asarray(obst).shape != shape:
        raise ValueError("cells AoS [...][q] and obst [...] of one domain")
    mode = sgs_mode(mode)
    f32 = np.float32
    w0, n = f32(omega), f32(n)
    if not (np.isfinite(w0) and 0 < w0 < 2) or f32(1) - w0 == 0:
        raise ValueError("omega lies in (0, 2) and is not 1")
    if not (np.isfinite(n) and n >= 0):
        raise ValueError("n is finite and not negative")
    if np.ndim(coef) != 0 and np.shape(coef) != shape:
        raise ValueError(f"a coefficient array has the domain's shape {shape}")
    k = np.broadcast_to(np.asarray(coef, np.float32), shape)
    if not np.isfinite(k).all() or (k < 0).any() or (mode == 2 and not ((k > 0) & (k < 2)).all()):
        raise ValueError("finite coefficients: Cs >= 0, or a rate in (0, 2)")
    nut = np.zeros(shape, np.float32)
    if n == 0:                                     # no launch: every bit stays
        return (cells, nut, np.ones(shape, bool)) if with_idle else (cells, nut)
    omo, tau0 = f32(1) - w0, f32(1) / w0
    nu0 = (tau0 - f32(0.5)) / f32(3)
    t = [cells[..., i] for i in range(q9)]
    with np.errstate(all="ignore"):                # hard states: Inf and NaN under obstacles are selected away
        if dims == 2:
            rho = _seq([f32(0)] + t, *range(q9 + 1))
            u = [(_seq(t, *a) - _seq(t, *b)) / rho for a, b in FORCING_J]
            usq = (u[0] * u[0]) + (u[1] * u[1])
            lw = ((f32(4) / f32(9)) * rho, rho / f32(9), rho / f32(36))
        else:
            rho = _seq(t, *range(q9))
            u = [(_seq(t, *a) - _seq(t, *b)) / rho for a, b in FORCING_J3D]
            usq = ((u[0] * u[0]) + (u[1] * u[1])) + (u[2] * u[2])
            lw = (rho / f32(3), rho / f32(18), rho / f32(36))
        csq = f32(1) - (usq * f32(1.5))
        two3 = f32(2) / f32(3)
        q = [None] * q9
        q[0] = t[0] - (lw[0] * csq)
        for a, b, wi, vel in pairs:
            v = vel(u)
            q[a] = t[a] - (lw[wi] * (((f32(4.5) * v) * (two3 + v)) + csq))
            q[b] = t[b] - (lw[wi] * (((f32(-4.5) * v) * (two3 - v)) + csq))
        diag = [_seq(q, *ks) for ks in moment[0]]
        off = [(q[a] + q[b]) - (q[c] + q[d]) for a, b, c, d in moment[1]]
        p2 = _seq([x * x for x in diag], *range(len(diag))) + (_seq([x * x for x in off], *range(len(off))) * f32(2))
        pim = np.sqrt(p2, dtype=np.float32) / np.abs(omo)
        if mode == 1:
            a = (SGS_SMAG_K * n) * (k * k)
            tau = f32(0.5) * (tau0 + np.sqrt((tau0 * tau0) + ((a * pim) / rho), dtype=np.float32))
            off_cell = k == 0
        else:
            nu1 = ((f32(1) / k) - f32(0.5)) / f32(3)
            tau = (f32(3) * (nu0 + (n * (nu1 - nu0)))) + f32(0.5)
            tau = np.broadcast_to(tau, shape)
            off_cell = k == w0
            we = f32(1) / tau
            if not ((we > 0) & (we < 2)).all():
                raise ValueError("the rate an application ends with lies in (0, 2)")
        we = f32(1) / tau
        d = sgs_factor(w0, we, omo)
        idle = (np.asarray(obst) != 0) | off_cell | (d == 0)
        nut = np.where(idle, f32(0), (tau - tau0) / f32(3)).astype(np.float32)
        for i in rescaled:
            cells[..., i] = np.where(idle, t[i], t[i] + (d * q[i]))
    return (cells, nut, idle) if with_idle else (cells, nut)


def sgs_filter(cells, obst, omega, mode, coef, n=1.0, with_idle=False):
    """(filtered copy of the AoS cells float32[ny][nx][9], nut float32[ny][nx]): one lbm_sgs_apply(n) on a
    lattice that was collided with `omega`, mode "smagorinsky" (coef = Cs) or "omega" (coef = the rate wanted),
    coef a number or an array [ny][nx].  nut is nu_add of every cell, 0 where it is idle (obstacle, Cs = 0 or
    rate = omega, or a factor d of exactly 0); idle cells keep their bits.  with_idle=True appends the bool
    map of the idle cells."""
    return _sgs_filter(cells, obst, omega, mode, coef, n, 2, with_idle)


def sgs_filter3d(cells, obst, omega, mode, coef, n=1.0, with_idle=False):
    """lbm3d_sgs_apply: cells float32[nz][ny][nx][19], coef a number or an array [nz][ny][nx]."""
    return _sgs_filter(cells, obst, omega, mode, coef, n, 3, with_idle)


def sgs_stats(nut, idle):
    """(cells, sum, max) as lbm_sgs_apply's stats give them, from the nut and the idle map of an application
    (with_idle=True): the cells that were not idle, the float64 sum of their nu_add and the larger of 0 and
    their largest nu_add."""
    live = ~np.asarray(idle, bool)
    v = np.asarray(nut, np.float32)[live]
    return int(live.sum()), float(np.sum(v.astype(np.float64))), float(np.fmax.reduce(v, initial=np.float32(0)))


# ---- scalar transport sums (include/lbm_transport_hip.h) ----
#
# The face fluxes in fp32 numpy (one subtraction), the other terms in float64 as
# the header widens them.  The tables are read at call time.

# index order of LBM_SBIN_* / LBM3D_SBIN_*
SBIN_FIELDS = ("phi", "phiphi", "uxphi", "uyphi", "fx", "fy")
SBIN_FIELDS3D = ("phi", "phiphi", "uxphi", "uyphi", "uzphi", "fx", "fy", "fz")
# per axis x, y[, z]: (speed that leaves the cell across the face, speed the neighbour sends back, array axis)
SCALAR_FACES = ((1, 3, 1), (2, 4, 0))
SCALAR_FACES3D = ((1, 2, 2), (3, 4, 1), (5, 6, 0))


def _scalar_face_flux(g, faces):
    g = np.asarray(g, np.float32)
    return tuple(g[out] - np.roll(g[back], -1, axis=axis) for out, back, axis in faces)


def scalar_face_flux(g):
    """(FX, FY) float32[ny][nx]: what crosses the face on the high side of each cell in the next scalar
    step, FX[y][x] = g1[y][x] - g3[y][x+1], FY[y][x] = g2[y][x] - g4[y+1][x], periodic.  The budget
    phi' - phi = FX[x-1] - FX[x] + FY[y-1] - FY[y] holds up to fp32 rounding off the fixed list."""
    return _scalar_face_flux(g, SCALAR_FACES)


def scalar_face_flux3d(g):
    """(FX, FY, FZ) float32[nz][ny][nx]: g1 - g2[x+1], g3 - g4[y+1], g5 - g6[z+1]."""
    return _scalar_face_flux(g, SCALAR_FACES3D)


def _scalar_terms(g, u, obst, faces, names):
    phi = scalar_phi(g).astype(np.float64)
    fluid = np.asarray(obst).reshape(phi.shape) == 0
    zero = np.float64(0)
    t = [np.where(fluid, phi, zero), np.where(fluid, phi * phi, zero)]
    t += [np.where(fluid, np.asarray(c, np.float32).astype(np.float64) * phi, zero) for c in u]
    t += [f.astype(np.float64) for f in _scalar_face_flux(g, faces)]
    return dict(zip(names, t))


def scalar_terms(g, ux, uy, obst):
    """{name: float64[ny][nx]} of the per-cell terms the transport sums add, in SBIN_FIELDS order: phi,
    phi^2 and u phi over the fluid cells (+0 on obstacles; phi the fp32 sum of the cell's populations,
    ux, uy as Engine.fields() gives them, every product in float64, where it is exact), and the fp32 face
    fluxes of every cell.  lbm_scalar_terms_ref gives the same bits."""
    return _scalar_terms(g, (ux, uy), obst, SCALAR_FACES, SBIN_FIELDS)


def scalar_terms3d(g, ux, uy, uz, obst):
    """The same for D3Q7 beside D3Q19: {name: float64[nz][ny][nx]} in SBIN_FIELDS3D order."""
    return _scalar_terms(g, (ux, uy, uz), obst, SCALAR_FACES3D, SBIN_FIELDS3D)


def scalar_binned_sums(g, ux, uy, obst, bw: int, bh: int):
    """The definition of lbm_scalar_store_binned restated: {name: float64[nby][nbx]} for the SBIN_FIELDS
    -- per bin the exactly rounded sum (math.fsum) of scalar_terms(), from +0 -- and "fluid"."""
    return _binned(scalar_terms(g, ux, uy, obst), obst, (bw, bh))


def scalar_binned_sums3d(g, ux, uy, uz, obst, bw: int, bh: int, bd: int):
    """lbm3d_scalar_store_binned: float64[nbz][nby][nbx] per SBIN_FIELDS3D name, and "fluid"."""
    return _binned(scalar_terms3d(g, ux, uy, uz, obst), obst, (bw, bh, bd))


def nusselt_number(flux_sum, area, diffusivity, dphi, height):
    """The flux through a section of `area` faces (a plane sum of a face flux) over what pure conduction
    carries across a layer `height` cells thick with the scalar difference dphi: area D dphi / height.
    The fixed list overwrites with equilibrium, which puts the effective wall off the node (its place
    depends on omega_s), so `height` is the caller's and results are best quoted against a conduction
    run of the same set-up."""
    return np.asarray(flux_sum, np.float64) / (float(area) * float(diffusivity) * float(dphi) / float(height))


def read_transport_state(filename: str, nbx: int, nby: int):
    """transport_state.dat (`bx by fluid` and the six SBIN_FIELDS sums in %.17g, bx fastest) back into
    {name: float64[nby][nbx]} and "fluid": int64."""
    out = {n: np.zeros((nby, nbx), np.float64) for n in SBIN_FIELDS}
    out["fluid"] = np.zeros((nby, nbx), np.int64)
    with open(filename, "r") as f:
        for line in f:
            t = line.split()
            if t:
                bx, by = int(t[0]), int(t[1])
                out["fluid"][by, bx] = int(t[2])
                for i, n in enumerate(SBIN_FIELDS):
                    out[n][by, bx] = float(t[3 + i])
    return out


# ---- scalar wall models and the wall flux (include/lbm_scalar_walls_hip.h) ----
#
# The header's definition in fp32 numpy, one ufunc per operation.  The tables and
# the two one-line functions are read at call time: a test plants an error by
# replacing one.

WALL_ADIABATIC, WALL_VALUE, WALL_FLUX = 0, 1, 2
# vectors (x, y[, z]) of the scalar speeds, in the speed order of lbm_scalar_hip.h
SCALAR_E = ((0, 0), (1, 0), (0, 1), (-1, 0), (0, -1))
SCALAR_E3D = ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))


def scalar_wall_links(obstacles) -> np.ndarray:
    """uint32[ny][nx]: bit k-1 set iff the cell is blocked and its neighbour along scalar speed k
    (E, N, W, S; periodic) is not -- link k of include/lbm_scalar_walls_hip.h.  Non-zero = wall cell."""
    return _links(np.asarray(obstacles).reshape(np.shape(obstacles)[-2:]), SCALAR_E)


def scalar_wall_links3d(obstacles) -> np.ndarray:
    """uint32[nz][ny][nx] link masks of the D3Q7 lattice (bits 0..5: +x -x +y -y +z -z)."""
    return _links(obstacles, SCALAR_E3D)


def _wall_reflect(m, gk):
    """g_k of a fixed-value wall: d - g_k with d = m + m (anti-bounce-back)."""
    d = m + m
    return d - gk


def _wall_handed(m, gk):
    """What a fixed-value link hands to the fluid: (g_k - m) * 2."""
    return (gk - m) * np.float32(2)


def _wall_table(links, obst, labels, kinds, values):
    """Per cell: (kind, value) of its body where it is a wall cell of a labelled body, else (0, +0)."""
    kinds = np.asarray(kinds, np.int32).reshape(-1)
    values = np.asarray(values, np.float32).reshape(-1)
    lab = np.asarray(labels).reshape(links.shape)
    nb = kinds.size
    if nb < 1 or values.size != nb or ((kinds < 0) | (kinds > 2)).any() or not np.isfinite(values).all():
        raise ValueError("one kind in 0..2 and one finite value per body, at least one body")
    if (lab[np.asarray(obst).reshape(links.shape) != 0] >= nb).any():
        raise ValueError("labels of blocked cells must be < nbodies (negative: no body)")
    on = (links != 0) & (lab >= 0)
    idx = np.where(on, lab, 0)
    return np.where(on, kinds[idx], 0), np.where(on, values[idx], np.float32(0)).astype(np.float32)


def _scalar_apply_walls(g, obst, labels, kinds, values, links, w):
    g = np.array(g, np.float32)
    kind, v = _wall_table(links, obst, labels, kinds, values)
    m = v * w[1]
    for k in range(1, g.shape[0]):
        link = ((links >> np.uint32(k - 1)) & np.uint32(1)) != 0
        gk = g[k].copy()
        g[k] = np.where(link & (kind == WALL_VALUE), _wall_reflect(m, gk),
                        np.where(link & (kind == WALL_FLUX), gk + v, gk))
    return g


def scalar_apply_walls(g, obst, labels, kinds, values) -> np.ndarray:
    """A copy of g float32[5][ny][nx] after the wall pass of lbm_scalar_advance: on every set link of
    a wall cell of body b (labels int[ny][nx], negative = no body) g_k <- 2 v w1 - g_k for kinds[b] = 1
    (fixed value v = values[b]) or g_k <- g_k + v for kinds[b] = 2 (fixed flux); everything else keeps
    its bits.  lbm_scalar_walls_ref gives the same bits."""
    return _scalar_apply_walls(g, obst, labels, kinds, values, scalar_wall_links(obst), SCALAR_W)


def scalar_apply_walls3d(g, obst, labels, kinds, values) -> np.ndarray:
    """The D3Q7 twin: g float32[7][nz][ny][nx]."""
    return _scalar_apply_walls(g, obst, labels, kinds, values, scalar_wall_links3d(obst), SCALAR_W3D)


def _scalar_wall_flux_cells(g, obst, labels, kinds, values, links, w):
    g = np.asarray(g, np.float32)
    kind, v = _wall_table(links, obst, labels, kinds, values)
    m = v * w[1]
    zero = np.float32(0)
    t = [None]
    for k in range(1, g.shape[0]):
        link = ((links >> np.uint32(k - 1)) & np.uint32(1)) != 0
        t.append(np.where(link & (kind == WALL_VALUE), _wall_handed(m, g[k]),
                          np.where(link & (kind == WALL_FLUX), v, zero)).astype(np.float32))
    return _seq(t, *range(1, g.shape[0])).astype(np.float32)


def scalar_wall_flux_cells(g, obst, labels, kinds, values) -> np.ndarray:
    """float32[ny][nx]: per wall cell the scalar its links handed to the fluid in the step (and pass)
    that produced g, exactly as include/lbm_scalar_walls_hip.h defines it; +0 elsewhere."""
    return _scalar_wall_flux_cells(g, obst, labels, kinds, values, scalar_wall_links(obst), SCALAR_W)


def scalar_wall_flux_cells3d(g, obst, labels, kinds, values) -> np.ndarray:
    return _scalar_wall_flux_cells(g, obst, labels, kinds, values, scalar_wall_links3d(obst), SCALAR_W3D)


def scalar_wall_flux(g, obst, labels, kinds, values):
    """((q, links), (q[nbodies], links[nbodies])): the fp64 sums of scalar_wall_flux_cells over all
    wall cells with the links of all wall cells, and the per-body sums."""
    links = scalar_wall_links(obst)
    return _totals(links, (_scalar_wall_flux_cells(g, obst, labels, kinds, values, links, SCALAR_W),), labels,
                   np.asarray(kinds).size)


def scalar_wall_flux3d(g, obst, labels, kinds, values):
    links = scalar_wall_links3d(obst)
    return _totals(links, (_scalar_wall_flux_cells(g, obst, labels, kinds, values, links, SCALAR_W3D),), labels,
                   np.asarray(kinds).size)


def read_wall_flux(filename: str):
    """wall_flux.dat (`body kind value q links` per line) -> (kind int32[n], value float32[n],
    q float64[n], links int64[n]) in body order."""
    rows = [line.split() for line in open(filename, "r") if line.split()]
    rows.sort(key=lambda t: int(t[0]))
    return (np.array([int(t[1]) for t in rows], np.int32), np.array([np.float32(t[2]) for t in rows], np.float32),
            np.array([float(t[3]) for t in rows], np.float64), np.array([int(t[4]) for t in rows], np.int64))


def read_scalar_state(filename: str, nx: int, ny: int) -> np.ndarray:
    """scalar_state.dat (`x y phi` per cell, phi in %.9g) -> float32[ny][nx]."""
    phi = np.zeros((ny, nx), np.float32)
    with open(filename, "r") as f:
        for line in f:
            t = line.split()
            if t:
                phi[int(t[1]), int(t[0])] = np.float32(t[2])
    return phi


def write_average_velocities(filename: str, av_vels) -> bool:
    """`i:\\t%.12e` per step (iostream scientific, precision 12)."""
    try:
        with open(filename, "w") as f:
            f.write("".join(f"{i}:\t{float(v):.12e}\n" for i, v in enumerate(np.asarray(av_vels, np.float32))))
        return True
    except OSError:
        return False


def write_results(filename: str, p: Params, obstacles: np.ndarray, cells: np.ndarray) -> bool:
    """final_state.dat: `ii jj u_x u_y |u| pressure obstacle`, jj outer, ii inner."""
    return write_results_from_fields(filename, p, obstacles, *macroscopic(p, obstacles, cells))


def write_results_from_fields(filename: str, p: Params, obstacles: np.ndarray, ux, uy, speed, pressure) -> bool:
    """final_state.dat from the planar float32[ny][nx] fields (macroscopic(), or
    Engine.fields() computed on the device): the bytes write_results writes."""
    fields = [np.asarray(f, np.float32).reshape(p.ny, p.nx) for f in (ux, uy, speed, pressure)]
    jj, ii = np.meshgrid(np.arange(p.ny), np.arange(p.nx), indexing="ij")
    cols = [ii.ravel(), jj.ravel()] + [f.ravel() for f in fields] + [np.asarray(obstacles).ravel().astype(int)]
    try:
        with open(filename, "w") as f:
            f.writelines(f"{a} {b} {c:.12e} {d:.12e} {e:.12e} {g:.12e} {h}\n"
                         for a, b, c, d, e, g, h in zip(*[col.tolist() for col in cols]))
        return True
    except OSError:
        return False


# ---- one process per GPU: rank-0 scatter / gather of sub-domain AoS blocks ----
#
# With lbm_load_cells_local / lbm_store_local (include/lbm_hip.h) a rank only
# holds its own rectangle of the lattice (16384^2 is 9.66 GB of AoS per full
# copy).  Rank 0 keeps the full-domain array the reference's loaders and .dat
# writers use (LbmRunner.cpp:67-113) and moves the blocks over a
# torch.distributed process group (gloo: host tensors).

def scatter_subdomains(full, rects, group=None):
    """Rank 0: full AoS float32[ny][nx][9]; every rank: returns its block
    full[y0:y0+h, x0:x0+w] (rects[rank], e.g. from lbm_partition)."""
    import torch
    import torch.distributed as dist
    rank = dist.get_rank(group)
    x0, y0, w, h = rects[rank]
    if rank == 0:
        for r, (rx, ry, rw, rh) in enumerate(rects):
            if r == 0:
                continue
            blk = np.ascontiguousarray(full[ry:ry + rh, rx:rx + rw], dtype=np.float32)
            dist.send(torch.from_numpy(blk), dst=r, group=group)
        return np.ascontiguousarray(full[y0:y0 + h, x0:x0 + w], dtype=np.float32)
    buf = torch.empty((h, w, 9), dtype=torch.float32)
    dist.recv(buf, src=0, group=group)
    return buf.numpy()


def gather_subdomains(block, rects, nx, ny, group=None):
    """Every rank passes its block (rects[rank]); rank 0 returns the full AoS
    float32[ny][nx][9], the others None."""
    import torch
    import torch.distributed as dist
    rank = dist.get_rank(group)
    if rank != 0:
        dist.send(torch.from_numpy(np.ascontiguousarray(block, dtype=np.float32)), dst=0, group=group)
        return None
    full = np.empty((ny, nx, 9), np.float32)
    x0, y0, w, h = rects[0]
    full[y0:y0 + h, x0:x0 + w] = block
    for r, (rx, ry, rw, rh) in enumerate(rects):
        if r == 0:
            continue
        buf = torch.empty((rh, rw, 9), dtype=torch.float32)
        dist.recv(buf, src=r, group=group)
        full[ry:ry + rh, rx:rx + rw] = buf.numpy()
    return full
