"""Every clamped launch of the D3Q19 engine's scalar and wall kernels past its clamp, on one slab
(devices=[0]); the 3-D twin of tests/test_gpu_launch_caps.py.  tests/caps_cases.py has the clamps and the
boxes, tests/test_launch_caps_host.py guards them on the CPU and lists every clamped launch in csrc/.

Bar: bitwise against the restatements of tests/test_gpu_scalar3d.py, test_gpu_thermal3d.py,
test_gpu_forces3d.py, test_gpu_scalar_walls3d.py, test_gpu_stress3d.py and test_gpu_gradients3d.py; sums
within the fold bounds those tests state.  No tolerance is new.

  8 x 512 x 130, 5 x 512 x 130   scalar_step3d and scalar_buoyancy3d: slab_grid is 1 x 128 x 128 blocks,
                                 planes 128 and 129 are a second trip of the plane loop (whole quads; one
                                 quad and a one-cell ragged lane)
  5 x 262200 x 1                 more rows than 4 x 65535: gridDim.y is clamped and rows 262140 .. 262199
                                 are a second trip of the row loop of scalar_step3d, scalar_buoyancy3d,
                                 macroscopic_fields3d and neq_strain3d.  velocity_gradients3d has no row
                                 loop and refuses a grid past 65535 blocks in y; its blocks hold 16 rows, so
                                 this box (16 388 blocks) is not refused and is pinned bitwise
  5 x 1048561 x 1                one row more than 65535 gradient blocks: the refusal and its message
  16 x 512 x 260, 17 x 511 x 261 scalar_phi<7> and scalar_stats<7>: 8320 whole blocks; a ragged last block
                                 and pad columns
  128 x 128 x 130                obstacles at all-even coordinates and one ball: wall_force_total / _map and
                                 the scalar wall pass and flux over 2 trips, the chunk kernels over 9
"""
from __future__ import annotations

import math

import numpy as np
import pytest

import caps_cases as cc
from lbm_amd import io as lio
from oracle import oracle
from test_gpu_forces import assert_sum

pytestmark = pytest.mark.gpu

OMEGA_S = 1.3
VEL = ("ux", "uy", "uz")
S3, PHI_REF = (0.004, -0.003, 0.002), 1.4


def _fold_bound(terms):
    """a sum of n terms folded in fp64 lies within 2 (n - 1) 2^-53 sum|term| of the exact sum."""
    t = np.abs(np.asarray(terms, np.float64)).ravel()
    return 2.0 * (t.size - 1) * 2.0 ** -53 * math.fsum(t.tolist())


def _state(box, seed, obstacles=0.1):
    """(p, obst, cells0, phi0): random obstacles (no channel walls: the box is periodic), a 25 % perturbed
    equilibrium from uniform float32 draws, phi0 in [1, 2)."""
    nx, ny, nz = box
    rng = np.random.default_rng(seed)
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.002, 1.85)
    obst = (rng.random((nz, ny, nx), dtype=np.float32) < obstacles).astype(np.uint8)
    one = oracle.init_cells3d(lio.Params3D(1, 1, 1, 0, 0.1, 0.002, 1.85)).reshape(19)
    cells = (one * (np.float32(0.875) + np.float32(0.25) * rng.random((nz, ny, nx, 19), dtype=np.float32))).astype(np.float32)
    phi0 = (1 + rng.random((nz, ny, nx), dtype=np.float32)).astype(np.float32)
    return p, obst, cells, phi0


def _slab_where(box):
    gx, gy, gz = cc.slab_grid(*box)

    def where(z, y, x):
        return (f"plane {z}: trip {z // gz} of the plane loop of block z = {z % gz}; row {y}: trip "
                f"{y // (gy * cc.S3Y)} of the row loop of block y = {y // cc.S3Y % gy}, wave {y % cc.S3Y}; "
                f"lane {x // 4 % cc.S3X}, cell {x % 4}")
    return where


def _step_and_kick(gpu_lib, box, seed):
    """scalar_advance(2) and the kick on a one-slab box, bitwise; returns nothing."""
    p, obst, cells0, phi0 = _state(box, seed)
    last = cc.slab_last_trip_mask(*box)
    assert last.any() and not last.all() and obst[last].any() and (obst[last] == 0).any()
    where = _slab_where(box)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        assert e.local_slabs() == [(0, box[2])]
        e.load_cells(cells0)
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        f = e.fields(VEL)
        g0 = lio.scalar_init3d(phi0)
        g = g0
        for _ in range(2):
            g = lio.scalar_step3d(g, f["ux"], f["uy"], f["uz"], obst, OMEGA_S)
        e.scalar_advance(2)
        got = e.scalar(populations=True)[1]
        for k in range(7):
            cc.assert_touched(g[k], g0[k], last, f"g[{k}]")
        cc.assert_same_bits(got, g, f"{box} scalar_step3d over advance(2)", lambda k, z, y, x: where(z, y, x) + f", speed {k}")
        e.scalar_buoyancy(S3, PHI_REF)
        kicked = e.store()[0]
    want = lio.buoyancy_kick3d(cells0, g, obst, p.density, S3, PHI_REF)
    cc.assert_touched(want, cells0, last[..., None], "kick")
    cc.assert_same_bits(kicked, want, f"{box} scalar_buoyancy3d", lambda z, y, x, k: where(z, y, x) + f", speed {k}")
    return p, obst, cells0, last, where


@pytest.mark.parametrize("box", cc.BOXES_STRIDED, ids=lambda b: "x".join(map(str, b)))
def test_strided_planes__scalar_step3d_scalar_buoyancy3d_plane_trip2_of_2(gpu_lib, box):
    assert cc.slab_grid(*box) == (1, 128, 128)
    _step_and_kick(gpu_lib, box, 130 + box[0])


def test_strided_rows__scalar_step3d_buoyancy3d_fields3d_strain3d_row_trip2_of_2__gradients3d_not_refused(gpu_lib):
    box = cc.BOX_ROWS
    assert cc.slab_grid(*box) == (1, cc.GRID_YZ_MAX, 1)
    p, obst, cells0, last, where = _step_and_kick(gpu_lib, box, 262200)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(cells0)
        # the fields launch clamps gridDim.y as the scalar launches do (the scalar step above read its velocities)
        ref = lio.macroscopic3d(p, obst, cells0)
        got = e.fields()
        for name, r in zip(got, ref):
            cc.assert_touched(r, np.zeros_like(r), last, name)
            cc.assert_same_bits(got[name], r, f"fields {name}", where)
        # the strain rate from the non-equilibrium moments: the same grid rule
        ref = lio.neq_strain3d(cells0, obst, p.omega)
        got = e.strain_rate()
        for name in e._STRESS_FIELDS:
            cc.assert_touched(ref[name], np.zeros_like(ref[name]), last, name)
            cc.assert_same_bits(got[name], ref[name], f"strain_rate {name}", where)
        # the gradients: 16 rows per block, 16 388 blocks in y -- below the 65535 the launch refuses beyond
        assert -(-box[1] // 16) < cc.GRID_YZ_MAX
        f = e.fields(VEL)
        ref = lio.velocity_gradients3d(f["ux"], f["uy"], f["uz"], obst)
        got = e.gradients()
        for name in e._GRAD_FIELDS:
            cc.assert_same_bits(got[name], ref[name], f"gradients {name}", where)


def test_refusal__velocity_gradients3d_grid_past_65535_row_blocks(gpu_lib):
    nx, ny, nz = cc.BOX_REFUSED
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.002, 1.85)
    with gpu_lib.Engine3D(p, np.zeros((nz, ny, nx), np.uint8), devices=[0]) as e:
        e.init_equilibrium()
        for call in (lambda: e.gradients(("q",)), e.gradient_stats):
            with pytest.raises(gpu_lib.LbmError, match=r"launch_velocity_gradients3d\(.*\): invalid argument") as err:
                call()
            assert err.value.code == gpu_lib.LBM_E_HIP
        ux = e.fields(("ux",))["ux"]                                       # the handle goes on working
        assert ux.shape == (nz, ny, nx) and np.isfinite(ux).all()


@pytest.mark.parametrize("box", [cc.BOX_FLAT, cc.BOX_FLAT_RAGGED], ids=lambda b: "x".join(map(str, b)))
def test_flat__scalar_phi7_scalar_stats7_trip2_of_2(gpu_lib, box):
    nx, ny, nz = box
    rng = np.random.default_rng(nx)
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.002, 1.85)
    obst = (rng.random((nz, ny, nx), dtype=np.float32) < 0.1).astype(np.uint8)
    phi0 = (rng.random((nz, ny, nx), dtype=np.float32) - np.float32(0.5)).astype(np.float32)      # both signs
    obst[-1, -1, -3:] = 0
    phi0[-1, -1, -2] = 2.0                                                  # the extremes lie in the last trip
    phi0[-1, -1, -3] = -2.0
    plane = cc.plane_trips(nx, ny * nz)
    region = cc.region_trips(nx * ny * nz)
    assert plane.trips == 2 and region.trips == 2
    sp = -(-nx // 4) * 4
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.scalar_begin(phi0, omega_s=OMEGA_S)                               # no lattice: everything but advance works
        phi, got = e.scalar(populations=True)
        total, lo, hi = e.scalar_stats()
        again = e.scalar_stats()
    g = lio.scalar_init3d(phi0)
    cc.assert_same_bits(got, g, f"{box} begin")
    ref = lio.scalar_phi(g)
    in_last = cc.plane_last_trip_mask((nz, ny, nx))
    cc.assert_touched(ref, np.zeros_like(ref), in_last, "phi")
    cc.assert_same_bits(phi, ref, f"{box} scalar_phi<7>", lambda z, y, x: plane.describe((z * ny + y) * sp + x))
    want, wlo, whi = lio.scalar_stats(g, obst)
    bound = _fold_bound(ref)
    print(f"{box}: total {total!r} exact {want!r} diff {abs(total - want):.3e} bound {bound:.3e}; [{lo!r}, {hi!r}]")
    assert abs(total - want) <= bound
    assert np.float32(lo) == wlo and np.float32(hi) == whi
    last = cc.region_last_trip_mask((nz, ny, nx))
    fluid = obst == 0
    assert ref[fluid & last].max() > ref[fluid & ~last].max() and ref[fluid & last].min() < ref[fluid & ~last].min()
    assert float(np.abs(ref[last]).astype(np.float64).sum()) > 1e6 * bound
    assert np.float64(again[0]).view(np.uint64) == np.float64(total).view(np.uint64) and again[1:] == (lo, hi)


# ------------------------------------------------------------------ walls ----

@pytest.fixture(scope="module")
def walls3d():
    nx, ny, nz = cc.WALLS3D
    obst, balls = cc.walls3d_obstacles()
    labels, nbodies = cc.one_cell_labels(obst, balls)
    p, _, cells, phi0 = _state(cc.WALLS3D, 128, obstacles=0.0)
    for a in (obst, labels, cells, phi0):
        a.setflags(write=False)
    return p, obst, balls, labels, nbodies, cells, phi0


def _links_count(links, n):
    nl = np.zeros(links.shape, np.int64)
    for j in range(n):
        nl += (links >> np.uint32(j)) & np.uint32(1)
    return nl


def test_wall_forces3d__wall_force_total_map_trip2_of_2_chunks_trip9_of_9(gpu_lib, walls3d):
    p, obst, balls, labels, nbodies, cells0, _ = walls3d
    links = lio.wall_links3d(obst)
    wall = links != 0
    nl = _links_count(links, 18)
    wt = cc.wall_trips(int(wall.sum()))
    per_body = np.bincount(labels[wall], minlength=nbodies)
    chunks = -(-per_body // cc.BODY_CHUNK)
    ct = cc.chunk_trips(int(chunks.sum()))
    assert wt.trips == 2 and wt.idle_lanes > 0 and ct.trips == 9 and chunks[0] > 1
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(cells0)
        e.run_steps(1)
        cells = e.store()[0]
        ref = lio.wall_force_cells3d(obst, cells)
        last = cc.wall_last_trip_mask(links)
        got = e.wall_force_field()
        for name, g_, r in zip("xyz", got, ref):
            cc.assert_touched(r, np.zeros_like(r), last, f"f{name}")
            cc.assert_same_bits(g_, r, f"wall_force_field f{name}")
        total = e.wall_force()
        for name, v, comp in zip("xyz", total, ref):
            assert_sum(v, comp[wall], f"total f{name}")
        assert total[-1] == int(nl.sum())
        e.set_bodies(labels, nbodies)
        got = e.wall_force_field()
        for name, g_, r in zip("xyz", got, ref):
            cc.assert_same_bits(g_, r, f"wall_force_field f{name}, sorted by body")
        total_b = e.wall_force()
        for name, v, comp in zip("xyz", total_b, ref):
            assert_sum(v, comp[wall], f"total f{name}, sorted by body")
        bodies = e.body_forces()
        again = e.body_forces()
    sel = wall & (labels >= 0)
    one = per_body == 1
    first_chunk = np.cumsum(chunks) - chunks
    in_last_trip = one & (first_chunk >= ct.last_start)
    assert in_last_trip.any()
    for c, (name, got_b, comp) in enumerate(zip("xyz", bodies, ref)):
        assert np.array_equal(got_b.view(np.uint64), again[c].view(np.uint64))
        want = np.zeros(nbodies, np.float64)
        want[labels[sel]] = comp[sel].astype(np.float64)
        assert (want[in_last_trip] != 0).any()
        bad = one & (got_b.view(np.uint64) != want.view(np.uint64))           # a one-cell body: its cell, exactly
        assert not bad.any(), (name, int(bad.sum()), ct.describe(first_chunk[np.flatnonzero(bad)[0]]))
        assert_sum(float(got_b[0]), comp[wall & (labels == 0)], f"ball f{name}")
    assert np.array_equal(bodies[-1], np.bincount(labels[sel], weights=nl[sel], minlength=nbodies).astype(np.int64))


def test_scalar_walls3d__scalar_walls_pass_flux_total_map_trip2_of_2_flux_chunks_trip9_of_9(gpu_lib, walls3d):
    p, obst, balls, labels, nbodies, cells0, phi0 = walls3d
    rng = np.random.default_rng(9)
    kinds = (np.arange(nbodies) % 3).astype(np.int32)
    kinds[0] = lio.WALL_VALUE
    values = (np.where(kinds == lio.WALL_FLUX, 0.02, 1.5) * rng.normal(size=nbodies)).astype(np.float32)
    links = lio.scalar_wall_links3d(obst)
    wall = links != 0
    nl = _links_count(links, 6)
    wt = cc.wall_trips(int(wall.sum()))
    assert wt.trips == 2 and wt.idle_lanes > 0
    last = cc.wall_last_trip_mask(links, labels, nbodies)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(cells0)
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        e.scalar_walls(labels, kinds, values)
        f = e.fields(VEL)
        g = lio.scalar_init3d(phi0)
        for _ in range(2):
            stepped = lio.scalar_step3d(g, f["ux"], f["uy"], f["uz"], obst, OMEGA_S)
            g = lio.scalar_apply_walls3d(stepped, obst, labels, kinds, values)
        e.scalar_advance(2)
        got = e.scalar(populations=True)[1]
        assert set(kinds[labels[last]]) == {0, 1, 2}
        assert ((cc.bits(g) != cc.bits(stepped)).any(axis=0) & last).any()
        cc.assert_same_bits(got, g, "scalar_walls over advance(2)")
        cells = lio.scalar_wall_flux_cells3d(g, obst, labels, kinds, values)
        cc.assert_touched(cells, np.zeros_like(cells), last, "flux map")
        cc.assert_same_bits(e.scalar_wall_flux_field(), cells, "scalar_wall_flux_field")
        q, n = e.scalar_wall_flux()
        exact = math.fsum(cells[wall].astype(np.float64).tolist())
        bound = _fold_bound(cells[wall])
        print(f"wall flux {q!r} exact {exact!r} diff {abs(q - exact):.3e} bound {bound:.3e}")
        assert n == int(nl.sum()) and abs(q - exact) <= bound
        qb, nb = e.scalar_body_flux()
    sel = wall & (labels >= 0)
    per_body = np.bincount(labels[sel], minlength=nbodies)
    one = per_body == 1
    want = np.zeros(nbodies, np.float64)
    want[labels[sel]] = cells[sel].astype(np.float64)
    bad = one & (qb.view(np.uint64) != want.view(np.uint64))
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:4].tolist())
    assert np.array_equal(nb, np.bincount(labels[sel], weights=nl[sel], minlength=nbodies).astype(np.int64))
    t = cells[wall & (labels == 0)]
    assert per_body[0] > cc.BODY_CHUNK and abs(qb[0] - math.fsum(t.astype(np.float64).tolist())) <= _fold_bound(t)
    assert cc.chunk_trips(cc.chunk_count(per_body)).trips == 9
