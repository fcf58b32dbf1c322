"""Every clamped grid-stride launch of the D2Q9 engine past its clamp, at its product value
(tests/caps_cases.py has the clamps and shapes; tests/test_launch_caps_host.py guards them on the CPU and
lists every clamped launch in csrc/ with its case or the reason it has none).

Bar: what the small tests of each kernel assert, on a shape whose last trip of the stride loop is
partial -- bitwise (uint32 / uint64 patterns) against the numpy restatement that kernel's own test uses,
sums within the fold bound that test states.  No tolerance is new.  Each test also asserts that its
reference changed cells of the last trip, so no comparison is of untouched memory, and every failure
names the trip, block and lane of the first differing cell.

  the large handle, 4098 x 2047 (2 098 175 quads: a second trip of 1023 quads of the last row, ending on
  the ragged two-cell quad and the periodic wrap in x and y; block 3 of it has one idle lane)
      macroscopic_fields and its stats form, count_nonfinite (8 trips), accumulate_moments and
      moment_means, scalar_step with its cross-lane moves, scalar_fixed (short list, one trip),
      scalar_phi (5 trips), scalar_stats (4 trips), scalar_buoyancy and the run that continues from it
  2 097 473 tracers on 37 x 19        advance (both schemes), sample, flag: a second trip of 321 tracers
  1100 x 1000, 275 000 isolated wall cells and two rings
      wall_force_total / _map (2 trips), wall_force_chunks (9 trips of 32 768 waves) and _fold_chunks,
      scalar_walls_pass, scalar_wall_flux_total / _map / _chunks / _fold
"""
from __future__ import annotations

import math

import numpy as np
import pytest

import caps_cases as cc
from lbm_amd import io as lio
from test_gpu_forces import assert_sum
from tracer_util import seeds

pytestmark = pytest.mark.gpu

NX, NY = cc.BIG_NX, cc.BIG_NY
OMEGA_S = 1.3
FIELDS = ("ux", "uy", "speed", "pressure")


def _quad_where(y, x, *rest):
    return cc.quad_where(NX, NY, y, x)


def _fold_bound(terms):
    """a sum of n terms folded in fp64 lies within 2 (n - 1) 2^-53 sum|term| of the exact sum."""
    t = np.abs(np.asarray(terms, np.float64)).ravel()
    return 2.0 * (t.size - 1) * 2.0 ** -53 * math.fsum(t.tolist())


# ------------------------------------------------------- the large handle ----

@pytest.fixture(scope="module")
def big():
    """(p, obst, cells0, phi0, last): the state of the large handle, built once from cheap numpy and left
    unchanged.  About 10 % obstacles, some of them in the last row; a 25 % perturbed equilibrium (uniform,
    float32 draws); phi0 in [1, 2) with a bump in the last rows; `last` the cells of the quad launches'
    second trip.  Cell (NY - 1, 1001) of that trip is fluid and the fastest of the domain."""
    rng = np.random.default_rng(4098)
    p = lio.Params(NX, NY, 4, 10, 0.1, 0.005, 1.85)
    obst = (rng.random((NY, NX), dtype=np.float32) < 0.1).astype(np.uint8)
    last = cc.quad_last_trip_mask(NX, NY)
    obst[NY - 1, [8, 9, NX - 2]] = 1                     # the first quad of the second trip, the ragged quad
    obst[NY - 1, 1000:1004] = 0
    obst[NY - 5:NY, 2000:2009] = 0
    cells = lio.init_cells(p) * (np.float32(0.875) + np.float32(0.25) * rng.random((NY, NX, 9), dtype=np.float32))
    cells = cells.astype(np.float32)
    cells[NY - 1, 1001, 1] *= np.float32(4)              # the largest |u| lies in the second trip
    phi0 = (1 + rng.random((NY, NX), dtype=np.float32)).astype(np.float32)
    phi0[NY - 5:NY, 2000:2009] += np.float32(3)          # the largest phi lies in every kernel's last trip
    assert obst[last].any() and (obst[last] == 0).any() and 0.09 < obst.mean() < 0.11
    for a in (obst, cells, phi0, last):
        a.setflags(write=False)
    return p, obst, cells, phi0, last


def _fixed_list():
    """A short fixed list: the first and the last cell of the second trip among them."""
    x = np.array([0, 8, NX - 1, 1002, 77, NX - 1], np.int32)
    y = np.array([0, NY - 1, NY - 1, NY - 1, 1000, 0], np.int32)
    return x, y, np.array([3.0, 3.25, 3.5, 3.75, 4.0, 4.25], np.float32)


def test_fields_and_stats__macroscopic_fields_trip2_of_2(gpu_lib, big):
    p, obst, cells0, _, last = big
    ref = lio.macroscopic(p, obst, cells0)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        got = e.fields()
        mass, umax = e.field_stats()
        again = e.field_stats()
    assert tuple(got) == FIELDS
    for name, r in zip(FIELDS, ref):
        cc.assert_touched(r, np.zeros_like(r), last, name)             # fields() hands out zeroed arrays
        cc.assert_same_bits(got[name], r, f"fields {name}", _quad_where)
    # the statistics, within the bound tests/test_gpu_fields.py states; the second trip is folded in
    rho32 = np.zeros((NY, NX), np.float32)
    for k in range(9):
        rho32 = rho32 + cells0[..., k]
    n = NX * NY
    mass_ref = float(rho32.astype(np.float64).sum())
    bound = 2 * (n - 1) * 2.0 ** -53 * mass_ref
    print(f"mass {mass!r} ref {mass_ref!r} diff {abs(mass - mass_ref):.3e} bound {bound:.3e}; max |u| {umax!r}")
    assert abs(mass - mass_ref) <= bound
    assert float(rho32[last].astype(np.float64).sum()) > 100 * bound    # dropping the second trip would show
    fluid = obst == 0
    speed = ref[2]
    assert cc.bits(np.float32(umax)) == cc.bits(np.max(speed[fluid]))
    assert np.max(speed[fluid & last]) > np.max(speed[fluid & ~last])   # and it comes from the second trip
    assert np.float64(again[0]).view(np.uint64) == np.float64(mass).view(np.uint64) and again[1] == umax


def test_nonfinite_count__count_nonfinite_trip8_of_8(gpu_lib, big):
    p, obst, cells0, _, _ = big
    t = cc.nonfinite_trips(NX * NY)
    cells = cells0.copy()
    flat = cells.reshape(-1, 9)
    planted = {0: (0,), 5000: (1, 2), t.last_start - 1: (3,), t.last_start: (4, 5, 6), t.units - 1: (7, 8),
               t.units - 300: (0,)}
    for i, (cell, ks) in enumerate(planted.items()):
        flat[cell, list(ks)] = (np.nan, np.inf, -np.inf)[i % 3]
    in_last = sum(len(ks) for cell, ks in planted.items() if cell >= t.last_start)
    total = sum(len(ks) for ks in planted.values())
    assert t.trips == 8 and 0 < in_last < total
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        assert e.nonfinite_count() == 0
        e.load_cells(cells)
        assert e.nonfinite_count() == total, (total, in_last, t.describe(t.units - 1))


@pytest.mark.parametrize("second", [False, True], ids=["mean", "mean_second"])
def test_averages__accumulate_moments_moment_means_trip2_of_2(gpu_lib, big, second):
    p, obst, cells0, _, last = big
    first = ("ux", "uy", "pressure")
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.avg_begin(second=second)
        samples = []
        for steps in (0, 1):                                            # two samples, one per lattice of the pair
            if steps:
                e.run_steps(steps)
            e.avg_sample()
            f = e.fields(first)
            samples.append([f[k] for k in first])
        assert e.avg_samples == 2
        names = e._AVG_FIELDS if second else e._AVG_FIELDS[:3]
        ref = lio.moment_sums(samples, second)
        means = lio.moment_means(ref, 2)
        assert len(ref) == len(names)
        assert (cc.bits(samples[0][0]) != cc.bits(samples[1][0]))[last].any()   # the step moved the second trip
        for name, r, m in zip(names, ref, means):
            cc.assert_touched(r, np.zeros_like(r), last, name)
            got = e.avg_sums((name,))[name]
            cc.assert_same_bits(got, r, f"avg_sums {name}", _quad_where)
            got = e.mean_fields((name,))[name]
            cc.assert_touched(m, np.zeros_like(m), last, name)
            cc.assert_same_bits(got, m, f"mean_fields {name}", _quad_where)


def test_scalar__scalar_step_trip2_of_2_scalar_phi_trip5_of_5_scalar_stats_trip4_of_4(gpu_lib, big):
    p, obst, cells0, phi0, last = big
    fixed = _fixed_list()
    where_g = lambda k, y, x: cc.quad_where(NX, NY, y, x) + f", speed {k}"
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        g0 = lio.scalar_init(phi0)
        e.scalar_fix(*fixed)
        g = lio.scalar_apply_fixed(g0, *fixed)
        e.run_steps(2, accelerate_first=True)
        f = e.fields(("ux", "uy"))
        for _ in range(2):
            g = lio.scalar_apply_fixed(lio.scalar_step(g, f["ux"], f["uy"], obst, OMEGA_S), *fixed)
        e.scalar_advance(2)
        assert e.scalar_steps == 2
        phi, got = e.scalar(populations=True)
        total, lo, hi = e.scalar_stats()
        again = e.scalar_stats()
    for k in range(5):
        cc.assert_touched(g[k], g0[k], last, f"g[{k}]")
    cc.assert_same_bits(got, g, "scalar populations after advance(2)", where_g)
    # scalar_phi: one entry of the padded plane per lane
    plane = cc.plane_trips(NX, NY)
    sp = -(-NX // 4) * 4
    phi_ref = lio.scalar_phi(g)
    cc.assert_touched(phi_ref, np.zeros_like(phi_ref), cc.plane_last_trip_mask((NY, NX)), "phi")
    cc.assert_same_bits(phi, phi_ref, "scalar()", lambda y, x: plane.describe(y * sp + x))
    held = lio.scalar_phi(lio.scalar_init(fixed[2].reshape(1, -1)))[0]
    assert np.array_equal(cc.bits(phi[fixed[1], fixed[0]]), cc.bits(held))
    # scalar_stats: extremes exact, sum within the fold bound of tests/test_gpu_scalar.py
    want, wlo, whi = lio.scalar_stats(g, obst)
    bound = _fold_bound(phi_ref)
    print(f"scalar total {total!r} exact {want!r} diff {abs(total - want):.3e} bound {bound:.3e}; [{lo!r}, {hi!r}]")
    assert abs(total - want) <= bound
    assert np.float32(lo) == wlo and np.float32(hi) == whi
    fluid = obst == 0
    in_last = cc.region_last_trip_mask((NY, NX))
    assert phi_ref[fluid & in_last].max() > phi_ref[fluid & ~in_last].max()     # the maximum comes from trip 4
    assert float(np.abs(phi_ref[in_last]).astype(np.float64).sum()) > 1e6 * bound
    assert np.float64(again[0]).view(np.uint64) == np.float64(total).view(np.uint64) and again[1:] == (lo, hi)


def test_buoyancy__scalar_buoyancy_trip2_of_2_and_the_run_after(gpu_lib, big):
    p, obst, cells0, phi0, last = big
    s, phi_ref = (0.004, -0.003), 1.4
    where_c = lambda y, x, k: cc.quad_where(NX, NY, y, x) + f", speed {k}"
    with gpu_lib.Engine(p, obst) as a:
        a.load_cells(cells0)
        a.scalar_begin(phi0, omega_s=OMEGA_S)
        a.run_steps(1, accelerate_first=True)
        a.scalar_advance(1)
        before = a.store(n_av=0)[0]
        g = a.scalar(populations=True)[1]
        a.scalar_buoyancy(s, phi_ref)
        kicked = a.store(n_av=0)[0]
        want = lio.buoyancy_kick(before, g, obst, p.density, s, phi_ref)
        cc.assert_touched(want, before, last[..., None], "kick")
        cc.assert_same_bits(kicked, want, "scalar_buoyancy", where_c)
        blocked = obst != 0
        assert np.array_equal(cc.bits(kicked[blocked]), cc.bits(before[blocked]))
        assert np.array_equal(cc.bits(a.scalar(populations=True)[1]), cc.bits(g))
        del before, want, g
        # the run continues as a second handle does that loaded the kicked cells
        a.run_steps(1)
        cells_a, av_a = a.store(n_av=1)
    with gpu_lib.Engine(p, obst) as b:
        b.load_cells(kicked)
        b.run_steps(1)
        cells_b, av_b = b.store(n_av=1)
    cc.assert_touched(cells_b, kicked, last[..., None], "the step after the kick")
    cc.assert_same_bits(cells_a, cells_b, "one step after the kick", where_c)
    assert np.array_equal(cc.bits(av_a), cc.bits(av_b))


# ---------------------------------------------------------------- tracers ----

@pytest.fixture(scope="module")
def tracer_problem():
    nx, ny = cc.TRACER_GRID
    rng = np.random.default_rng(37)
    p = lio.Params(nx, ny, 8, 10, 0.1, 0.005, 1.85)
    obst = (rng.random((ny, nx)) < 0.1).astype(np.uint8)
    obst[0, 0] = obst[ny - 1, nx - 1] = 1
    cells = (lio.init_cells(p) * (1 + 0.05 * rng.standard_normal((ny, nx, 9)))).astype(np.float32)
    x, y = seeds(np.random.default_rng(5), (nx, ny), cc.TRACER_PERIOD)
    reps = -(-cc.TRACER_COUNT // cc.TRACER_PERIOD)
    tile = lambda a: np.tile(a, reps)[:cc.TRACER_COUNT]
    return p, obst, cells, x, y, tile


@pytest.mark.parametrize("scheme", ["euler", "heun"])
def test_tracers__advance_sample_flag_trip2_of_2(gpu_lib, tracer_problem, scheme):
    p, obst, cells0, x0, y0, tile = tracer_problem
    t = cc.tracer_trips()
    where = lambda i: t.describe(i) + f", the image of tracer {i % cc.TRACER_PERIOD}"
    assert t.trips == 2 and t.last_count == 321
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.tracers_begin(tile(x0), tile(y0))
        assert e.tracer_count == cc.TRACER_COUNT
        x, y = x0, y0
        for n in (3, 2):
            e.run_steps(n, accelerate_first=n == 3)
            f = e.fields(("ux", "uy", "pressure"))
            x, y = lio.tracer_advance(f["ux"], f["uy"], x, y, float(n), scheme)   # the first 4099, by tracer_util's route
            e.tracers_advance(n, scheme)
            got = e.tracers()
            for c, want in (("x", x), ("y", y)):
                cc.assert_same_bits(got[c], tile(want), f"{scheme} advance({n}) {c}", where)
            cc.assert_same_bits(got["blocked"], tile(lio.tracer_blocked(obst, x, y)), f"{scheme} flag", where)
            s = e.tracer_sample()
            for name in ("ux", "uy", "pressure"):
                cc.assert_same_bits(s[name], tile(lio.tracer_interp(f[name], x, y)), f"{scheme} sample {name}", where)
    moved = cc.bits(tile(x)) != cc.bits(tile(x0))
    assert moved[t.last_start:].any() and lio.tracer_blocked(obst, x, y).any()


# ------------------------------------------------------------------ walls ----

@pytest.fixture(scope="module")
def walls_problem():
    nx, ny = cc.WALLS_NX, cc.WALLS_NY
    rng = np.random.default_rng(1100)
    p = lio.Params(nx, ny, 4, 10, 0.1, 0.005, 1.85)
    obst, rings = cc.walls2d_obstacles()
    labels, nbodies = cc.one_cell_labels(obst, rings)
    cells = (lio.init_cells(p) * (np.float32(0.875) + np.float32(0.25) * rng.random((ny, nx, 9), dtype=np.float32)))
    cells = cells.astype(np.float32)
    phi0 = (1 + rng.random((ny, nx), dtype=np.float32)).astype(np.float32)
    for a in (obst, labels, cells, phi0):
        a.setflags(write=False)
    return p, obst, rings, labels, nbodies, cells, phi0


def test_wall_forces__wall_force_total_map_trip2_of_2_chunks_trip9_of_9(gpu_lib, walls_problem):
    p, obst, rings, labels, nbodies, cells0, _ = walls_problem
    links = lio.wall_links(obst)
    wall = links != 0
    nl = np.zeros(links.shape, np.int64)
    for j in range(8):
        nl += (links >> np.uint32(j)) & np.uint32(1)
    wt = cc.wall_trips(int(wall.sum()))
    per_body = np.bincount(labels[wall], minlength=nbodies)
    ct = cc.chunk_trips(cc.chunk_count(per_body))
    assert wt.trips == 2 and ct.trips == 9
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.run_steps(1, accelerate_first=True)
        cells = e.store(n_av=0)[0]
        ref = lio.wall_force_cells(obst, cells)
        # row-major list: the map and the total
        order = cc.wall_list_order(links)
        rank = np.zeros(links.size, np.int64)
        rank[order] = np.arange(order.size)
        where = lambda y, x: wt.describe(rank[y * p.nx + x]) if wall[y, x] else "no wall cell"
        last = cc.wall_last_trip_mask(links)
        got = e.wall_force_field()
        for name, g_, r in zip("xy", got, ref):
            cc.assert_touched(r, np.zeros_like(r), last, f"f{name}")
            cc.assert_same_bits(g_, r, f"wall_force_field f{name}", where)
        total = e.wall_force()
        for name, v, comp in zip("xy", total, ref):
            assert_sum(v, comp[wall], f"total f{name}")
            assert abs(float(comp[last].astype(np.float64).sum())) > 0
        assert total[-1] == int(nl.sum())
        # the list sorted by body: the map and the total again, then the per-body sums
        e.set_bodies(labels, nbodies)
        order_b = cc.wall_list_order(links, labels, nbodies)
        assert (order_b != order).any()                          # the rings moved to the front of the list
        got = e.wall_force_field()
        for name, g_, r in zip("xy", got, ref):
            cc.assert_same_bits(g_, r, f"wall_force_field f{name}, sorted by body")
        total_b = e.wall_force()
        for name, v, comp in zip("xy", total_b, ref):
            assert_sum(v, comp[wall], f"total f{name}, sorted by body")
        assert total_b[-1] == total[-1]
        bodies = e.body_forces()
        again = e.body_forces()
    sel = wall & (labels >= 0)
    one = per_body == 1                                       # a one-cell body's sum is its cell's value, exactly
    chunks = -(-per_body // cc.BODY_CHUNK)
    first_chunk = np.cumsum(chunks) - chunks                  # chunks are laid out body after body
    where_b = lambda b: f"body {b}, " + ct.describe(first_chunk[b])
    in_last_trip = one & (first_chunk >= ct.last_start)
    assert in_last_trip.any() and (chunks[:len(rings)] > 1).all()
    for c, (name, got_b, comp) in enumerate(zip("xy", bodies, ref)):
        assert np.array_equal(got_b.view(np.uint64), again[c].view(np.uint64))
        want = np.zeros(nbodies, np.float64)
        want[labels[sel]] = comp[sel].astype(np.float64)      # (the rings: whichever cell came last; not compared)
        assert (want[in_last_trip] != 0).any()
        bad = one & (got_b.view(np.uint64) != want.view(np.uint64))
        assert not bad.any(), (name, int(bad.sum()), where_b(int(np.flatnonzero(bad)[0])))
        for r in range(len(rings)):
            assert_sum(float(got_b[r]), comp[wall & (labels == r)], f"ring {r} f{name}")
    assert np.array_equal(bodies[-1], np.bincount(labels[sel], weights=nl[sel], minlength=nbodies).astype(np.int64))
    assert int(one.sum()) > cc.BODY_MAX_BLOCKS * 4


def test_scalar_walls__scalar_walls_pass_flux_total_map_trip2_of_2_flux_chunks_trip9_of_9(gpu_lib, walls_problem):
    p, obst, rings, labels, nbodies, cells0, phi0 = walls_problem
    rng = np.random.default_rng(7)
    kinds = (np.arange(nbodies) % 3).astype(np.int32)                   # adiabatic, value, flux in turn
    kinds[:2] = (lio.WALL_VALUE, lio.WALL_FLUX)
    values = (np.where(kinds == lio.WALL_FLUX, 0.02, 1.5) * rng.normal(size=nbodies)).astype(np.float32)
    links = lio.scalar_wall_links(obst)
    wall = links != 0
    nl = np.zeros(links.shape, np.int64)
    for k in range(4):
        nl += (links >> np.uint32(k)) & np.uint32(1)
    wt = cc.wall_trips(int(wall.sum()))
    assert wt.trips == 2 and wt.idle_lanes > 0
    order = cc.wall_list_order(links, labels, nbodies)
    rank = np.zeros(links.size, np.int64)
    rank[order] = np.arange(order.size)
    where = lambda y, x: wt.describe(rank[y * p.nx + x]) if wall[y, x] else "no wall cell"
    last = cc.wall_last_trip_mask(links, labels, nbodies)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        e.scalar_walls(labels, kinds, values)
        e.run_steps(1, accelerate_first=True)
        f = e.fields(("ux", "uy"))
        g = lio.scalar_init(phi0)
        for _ in range(2):
            stepped = lio.scalar_step(g, f["ux"], f["uy"], obst, OMEGA_S)
            g = lio.scalar_apply_walls(stepped, obst, labels, kinds, values)
        e.scalar_advance(2)
        got = e.scalar(populations=True)[1]
        assert set(kinds[labels[last]]) == {0, 1, 2}
        assert ((cc.bits(g) != cc.bits(stepped)).any(axis=0) & last).any()          # the pass acted in its last trip
        cc.assert_same_bits(got, g, "scalar_walls over advance(2)", lambda k, y, x: where(y, x) + f", speed {k}")
        # the flux: map, total, per body
        cells = lio.scalar_wall_flux_cells(g, obst, labels, kinds, values)
        cc.assert_touched(cells, np.zeros_like(cells), last, "flux map")
        cc.assert_same_bits(e.scalar_wall_flux_field(), cells, "scalar_wall_flux_field", where)
        q, n = e.scalar_wall_flux()
        exact = math.fsum(cells[wall].astype(np.float64).tolist())
        bound = _fold_bound(cells[wall])
        print(f"wall flux {q!r} exact {exact!r} diff {abs(q - exact):.3e} bound {bound:.3e}")
        assert n == int(nl.sum()) and abs(q - exact) <= bound
        assert abs(float(cells[last].astype(np.float64).sum())) > 1e3 * bound
        qb, nb = e.scalar_body_flux()
        qb2, nb2 = e.scalar_body_flux()
    assert np.array_equal(qb.view(np.uint64), qb2.view(np.uint64)) and np.array_equal(nb, nb2)
    sel = wall & (labels >= 0)
    per_body = np.bincount(labels[sel], minlength=nbodies)
    one = per_body == 1
    want = np.zeros(nbodies, np.float64)
    want[labels[sel]] = cells[sel].astype(np.float64)
    bad = one & (qb.view(np.uint64) != want.view(np.uint64))                        # one-cell bodies: exact
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:4].tolist())
    assert np.array_equal(nb, np.bincount(labels[sel], weights=nl[sel], minlength=nbodies).astype(np.int64))
    for r in range(len(rings)):
        t = cells[wall & (labels == r)]
        assert per_body[r] > cc.BODY_CHUNK
        assert abs(qb[r] - math.fsum(t.astype(np.float64).tolist())) <= _fold_bound(t), r
    assert cc.chunk_trips(cc.chunk_count(per_body)).trips == 9
