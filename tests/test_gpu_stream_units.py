"""The stream kernel's two unit copies and the per-unit flags that choose
between them (csrc/lbm_stream2.hip stream_steps2d / stream2d_flags,
csrc/lbm_split.hip build_args), seen through lbm_stream_units.

A work unit (strip x segment) whose load window holds no obstacle byte runs
the select-free copy (OBST = false), every other unit the copy with obstacle
loads and rebound selects.  The suite's other stream tests scatter 3-5 %
obstacles (every unit flagged) or none (no unit flagged next to a flagged
one), and the big grids carry walls many cells thick, so a flag that scanned
a row or a column too few would go unnoticed.  Here:

  a. the flag contract, on maps of a few lone cells: a unit with an obstacle
     within S - 1 cells of its owned rectangle is flagged (correctness), a unit
     whose load window holds none is not (performance);
  b. one lone obstacle swept across unit seams, periodic seams, the ragged last
     strip and sub-domain borders: bitwise against the oracle (tolerance forms:
     within TOL_POP, and bitwise equal to the same handle without flags);
  c. the dispatch order, the flags and the 16-column strip widths change no
     lattice value (and the order no |u| sum);
  d. the tolerance LP forms S = 7..10 with segments shorter than 2S rows;
  e. a lone obstacle swept across a tile seam of the other kernels (the packed
     resident kernel has the same wave-uniform shortcut);
  and, on the CPU, that the perturbed state makes every swept position visible.

Problem family of a-c: 384 x 64, LBM_STREAM_HS = 16: four strips (the last
ragged) x four segments in every form.  The populations are the rest
equilibrium times (1 + 0.05 N(0, 1)): on the rest equilibrium itself rebound
and collision both return their input and a missed obstacle would not show.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from conftest import load_problem
from lbm_amd import io as lio
from oracle import oracle

NX, NY, HS = 384, 64, 16
P = lio.Params(NX, NY, 0, 10, 0.1, 0.02, 1.7)
TOL_POP = 2e-5  # tests/test_gpu_tolerance.py: max |f_gpu - f_oracle| / |f_oracle| over every population

# name -> (S, tolerance, LBM_STREAM_CFG or None for the default form)
FORMS = {
    "bitwise-S4-plain": (4, False, "0"), "bitwise-S5-plain": (5, False, "0"), "bitwise-S6-LP": (6, False, None),
    "bitwise-S6-plain": (6, False, "0"),
    "tolerance-S6": (6, True, None), "tolerance-S8": (8, True, None), "tolerance-S10": (10, True, None),
}
# the flag contract also runs the depths no sweep uses
CONTRACT_FORMS = dict(FORMS, **{
    "bitwise-S2-plain": (2, False, "0"), "bitwise-S3-plain": (3, False, "0"),
    "tolerance-S7": (7, True, None), "tolerance-S9": (9, True, None),
})
DECOMPS = {"single": dict(), "1x2": dict(parts=2, grid=(1, 2)), "2x1": dict(parts=2, grid=(2, 1)),
           "2x2": dict(parts=4, grid=(2, 2))}

gpu = pytest.mark.gpu


def _rel(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))


@functools.lru_cache(maxsize=None)
def perturbed_cells(nx=NX, ny=NY, seed=20):
    p = lio.Params(nx, ny, 0, 10, 0.1, 0.02, 1.7)
    rng = np.random.default_rng(seed)
    cells = (lio.init_cells(p) * (1 + 0.05 * rng.standard_normal((ny, nx, 9)))).astype(np.float32)
    cells.setflags(write=False)
    return cells


def lone(x, y, nx=NX, ny=NY):
    obst = np.zeros((ny, nx), np.uint8)
    obst[y % ny, x % nx] = 1
    return obst


def random_cells_map(seed, n=8):
    """n lone obstacle cells, uniformly random: about one per two units of the single domain."""
    rng = np.random.default_rng(seed)
    obst = np.zeros((NY, NX), np.uint8)
    obst.reshape(-1)[rng.choice(NX * NY, n, replace=False)] = 1
    return obst


def set_form(monkeypatch, form, hs=HS):
    S, tol, cfg = CONTRACT_FORMS[form]
    monkeypatch.setenv("LBM_STREAM_HS", str(hs))
    if cfg is not None:
        monkeypatch.setenv("LBM_STREAM_CFG", cfg)
    return S, tol


def engine(native, obst, form, p=P, **kw):
    S, tol, _ = CONTRACT_FORMS[form]
    flags = kw.pop("flags", 0) | (native.FLAG_TOLERANCE if tol else 0)
    e = native.Engine(p, obst, devices=[0], kernel=native.KERNEL_STREAM, steps_per_launch=S, flags=flags, **kw)
    assert e.kernel_in_use() == "stream" and e.steps_per_launch() == S
    assert e.numerics() == ("tolerance" if tol else "bitwise")
    return e


def global_units(e):
    """[(boundary, gx0, gy0, w, h, flag, sub)] with each unit's rectangle moved to its sub-domain's origin."""
    rects = e.local_rects()
    return [(b, rects[s][0] + x0, rects[s][1] + y0, w, h, f, s) for (s, b, x0, y0, w, h, f) in e.stream_units()]


def any_obstacle(obst, x0, x1, y0, y1):
    """Any obstacle in columns [x0, x1) x rows [y0, y1) of the periodic global map."""
    ny, nx = obst.shape
    xs = np.arange(x0, min(x1, x0 + nx)) % nx
    ys = np.arange(y0, min(y1, y0 + ny)) % ny
    return bool(obst[np.ix_(ys, xs)].any())


def inside(u, x, y, grow=0):
    _, gx0, gy0, w, h, _, _ = u
    return (x - (gx0 - grow)) % NX < w + 2 * grow and (y - (gy0 - grow)) % NY < h + 2 * grow


# ------------------------------------------------------- a. flag contract ----

@gpu
@pytest.mark.parametrize("form", list(CONTRACT_FORMS))
def test_unit_flag_contract(gpu_lib, debug_knobs, form, monkeypatch):
    """Units tile every sub-domain once; reads_obstacle is 1 wherever an
    obstacle lies within S - 1 cells of the owned rectangle, and 0 wherever the
    unit's load window holds none.

    The window (stream2d_geo / stream2d_load): rows yo0 - S .. yo1 + S - 1,
    128 columns from (xo0 - S) & ~1, so inside [xo0 - S - 1, xo0 + 128 - S].
    One case the window's plain statement misses: the obstacle map's rows are
    w + 2 og bytes (og = S + 2) and the loads do not clamp their column to
    it, so window columns x >= w + og of a sub-domain's last strips fall on
    the NEXT row's bytes, columns x - (w + 2 og) from -og on (its ghost ring
    and first cells).  Those lanes lie S + 2 or more columns past the
    sub-domain, outside every owned cell's dependency cone, so what they read
    changes no result; it can set the flag of such a strip, and the clean
    region asserted here includes it."""
    S, _ = set_form(monkeypatch, form)
    seen = {0: set(), 1: set()}
    for dname, kw in DECOMPS.items():
        for seed in (1, 2, 3):
            obst = random_cells_map(seed)
            with engine(gpu_lib, obst, form, **kw) as e:
                rects = e.local_rects()
                units = e.stream_units()
            cover = [np.zeros((h, w), np.int32) for (_, _, w, h) in rects]
            for (s, b, x0, y0, w, h, f) in units:
                assert w > 0 and h > 0 and b in (0, 1) and f in (0, 1), (dname, seed, (s, b, x0, y0, w, h, f))
                cover[s][y0:y0 + h, x0:x0 + w] += 1
                sx, sy, sw, _ = rects[s]
                gx0, gy0 = sx + x0, sy + y0
                where = (form, dname, seed, (s, b, x0, y0, w, h))
                if any_obstacle(obst, gx0 - (S - 1), gx0 + w + S - 1, gy0 - (S - 1), gy0 + h + S - 1):
                    assert f == 1, ("obstacle within S - 1 of the owned cells, flag clear", where)
                clean = not any_obstacle(obst, gx0 - (S + 1), gx0 + 128 - S + 1, gy0 - S, gy0 + h + S)
                over = x0 + 128 - S - (sw + 2 * (S + 2))  # last next-row column the window reaches
                if over >= -(S + 2):
                    clean = clean and not any_obstacle(obst, sx - (S + 2), sx + over + 1, gy0 - S + 1, gy0 + h + S + 1)
                if clean:
                    assert f == 0, ("no obstacle in the load window, flag set", where)
                seen[b].add(f)
            for c in cover:
                assert (c == 1).all(), (form, dname, seed)
    assert seen[0] == {0, 1} and seen[1] == {0, 1}, seen


@gpu
def test_unit_flags_off_and_errors(gpu_lib, debug_knobs, monkeypatch):
    """LBM_STREAM_UOBST=0: no flags, every unit reports -1; a handle on another
    kernel answers LBM_E_STATE, NULL arguments LBM_E_INVALID."""
    set_form(monkeypatch, "bitwise-S6-LP")
    obst = random_cells_map(1)
    with engine(gpu_lib, obst, "bitwise-S6-LP") as e:
        with_flags = e.stream_units()
        n = ctypes.c_int32()
        assert gpu_lib.load_library().lbm_stream_units(e._h, None, 0, None) == gpu_lib.LBM_E_INVALID
        assert gpu_lib.load_library().lbm_stream_units(None, None, 0, ctypes.byref(n)) == gpu_lib.LBM_E_INVALID
    monkeypatch.setenv("LBM_STREAM_UOBST", "0")
    for kw in (dict(), dict(parts=4, grid=(2, 2))):
        with engine(gpu_lib, obst, "bitwise-S6-LP", **kw) as e:
            units = e.stream_units()
        assert units and all(u[6] == -1 for u in units)
        if not kw:
            assert [u[:6] for u in units] == [u[:6] for u in with_flags]
    with gpu_lib.Engine(P, obst, devices=[0], kernel=gpu_lib.KERNEL_STEP2) as e:
        with pytest.raises(gpu_lib.LbmError) as ei:
            e.stream_units()
    assert ei.value.code == gpu_lib.LBM_E_STATE


# ------------------------------------------------ b. lone-obstacle sweeps ----

def seams(units):
    """Strip and segment starts of a single-domain unit list."""
    return sorted({u[1] for u in units}), sorted({u[2] for u in units})


def sweep_positions(kind, S, xs, ys):
    """Obstacle positions of one sweep, as (d, x, y): d = signed distance from
    the seam (d >= 0: the cell d past it; at the periodic seams the seam is the
    wrap, so d = x or x - NX, likewise y)."""
    D = range(-(2 * S + 2), 2 * S + 3)
    xseam, yseam, xrag = xs[1], ys[2], xs[-1]
    ymid, xmid = ys[1] + (ys[2] - ys[1]) // 2, xs[0] + (xs[1] - xs[0]) // 2
    E = range(-(S + 1), S + 1)  # x in [0, S] and [nx - S - 1, nx - 1], likewise y
    return {
        "x": [(d, xseam + d, ymid) for d in D],
        "y": [(d, xmid + (d & 1), yseam + d) for d in D],  # both columns of a lane's pair
        "diag": [(d, xseam + d, yseam + d) for d in D],
        "antidiag": [(d, xseam + d, yseam - 1 - d) for d in D],
        "ragged": [(d, xrag + d, ymid) for d in D],
        "periodic-x": [(d, d % NX, ymid) for d in E],
        "periodic-y": [(d, xmid + (d & 1), d % NY) for d in E],
        # through the periodic corner: (k, k) .. (nx - 1 - k, ny - 1 - k), and (k, ny - 1 - k) .. (nx - 1 - k, k)
        "periodic-diag": [(d, d % NX, d % NY) for d in E],
        "periodic-antidiag": [(d, d % NX, (-1 - d) % NY) for d in E],
    }[kind]


def ring_overlap(a, la, b, lb, n):
    """[a, a + la) and [b, b + lb) intersect on a ring of n cells."""
    return (b - a) % n < la or (a - b) % n < lb


def check_sweep_units(units, x, y, where):
    """The sweep reaches both copies: the unit that owns the obstacle is
    flagged, and a unit next to it (touching the owner, corners included) is
    not."""
    owner = [u for u in units if inside(u, x, y)]
    assert len(owner) == 1 and owner[0][5] == 1, (where, owner)
    _, ox, oy, ow_, oh, _, _ = owner[0]
    near = [u for u in units if u is not owner[0] and ring_overlap(ox - 1, ow_ + 2, u[1], u[3], NX) and
            ring_overlap(oy - 1, oh + 2, u[2], u[4], NY)]
    assert any(u[5] == 0 for u in near), (where, near)


def run_lone(native, form, obst, steps, stats, monkeypatch, where, on_units=check_sweep_units, **kw):
    """One engine on `obst`: every step count in `steps` from the perturbed
    state, checked against the oracle (bitwise forms: bitwise; tolerance forms:
    TOL_POP, and bitwise equal to the same configuration without unit flags)."""
    S, tol, _ = CONTRACT_FORMS[form]
    cells0 = perturbed_cells()
    out = {}
    for flags_on in ((True, False) if tol else (True,)):
        if not flags_on:
            monkeypatch.setenv("LBM_STREAM_UOBST", "0")
        try:
            with engine(native, obst, form, **kw) as e:
                if flags_on:
                    units = global_units(e)
                for n in steps:
                    e.load_cells(cells0)
                    e.run_steps(n, accelerate_first=True)
                    assert e.run_stats() == stats(n), (where, n)
                    out[flags_on, n] = e.store(n_av=n)
        finally:
            if not flags_on:
                monkeypatch.delenv("LBM_STREAM_UOBST")
    for n in steps:
        ref, ref_av = oracle.run(P, obst, n, cells0)
        cells, av = out[True, n]
        if tol:
            assert _rel(cells, ref) < TOL_POP, (where, n)
            assert np.array_equal(cells, out[False, n][0]), ("flags change the tolerance lattice", where, n)
        else:
            assert np.array_equal(cells, ref), (where, n)
            np.testing.assert_allclose(av, ref_av, rtol=1e-5, err_msg=str((where, n)))
    (y,), (x,) = np.nonzero(obst)
    on_units(units, int(x), int(y), where)


def fused_stats(S):
    # a remainder of r >= 2 steps is one more fused launch, r = 1 a one-step launch
    return lambda n: (n // S + (n % S >= 2), 1 if n % S == 1 else 0)


@gpu
@pytest.mark.parametrize("kind", ["x", "y", "diag", "antidiag", "ragged", "periodic-x", "periodic-y", "periodic-diag",
                                  "periodic-antidiag"])
@pytest.mark.parametrize("form", list(FORMS))
def test_lone_obstacle_sweep(gpu_lib, debug_knobs, form, kind, monkeypatch):
    """One obstacle cell at every signed distance d in [-(2S + 2), 2S + 2] from
    a unit seam (positions from stream_units; at the periodic seams d in
    [-(S + 1), S], along x, along y and along both diagonals through the
    corner), 2S - 1 steps = one fused S-step
    launch plus a fused (S - 1)-step remainder on the same flags; at the
    distances where the flag of the unit across the seam flips (+-(S - 2) ..
    +-(S + 1)) also S + 2 steps (the shortest fused remainder) and 2S + 1 (a
    one-step remainder from the other side of the lattice pair)."""
    S, _ = set_form(monkeypatch, form)
    with engine(gpu_lib, np.zeros((NY, NX), np.uint8), form) as e:
        units = e.stream_units()
    assert len(units) == 16 and all(u[6] == 0 and u[1] == 0 for u in units)
    xs, ys = seams(global_units_of(units))
    assert len(xs) == 4 and len(ys) == 4 and NX - xs[-1] < xs[1] - xs[0]  # the last strip is ragged
    flip = {s * k for s in (-1, 1) for k in (S - 2, S - 1, S, S + 1)}
    for d, x, y in sweep_positions(kind, S, xs, ys):
        steps = (2 * S - 1, S + 2, 2 * S + 1) if d in flip else (2 * S - 1,)
        run_lone(gpu_lib, form, lone(x, y), steps, fused_stats(S), monkeypatch, (form, kind, d, x % NX, y % NY))


def global_units_of(units):
    """Single domain: the sub-domain's origin is the global one."""
    return [(b, x0, y0, w, h, f, s) for (s, b, x0, y0, w, h, f) in units]


@gpu
@pytest.mark.parametrize("decomp,force", [("1x2", False), ("2x1", False), ("1x2", True)])
@pytest.mark.parametrize("form", ["bitwise-S6-LP", "tolerance-S10"])
def test_lone_obstacle_across_subdomain_border(gpu_lib, debug_knobs, form, decomp, force, monkeypatch):
    """The obstacle moves from 2S + 2 cells inside one sub-domain to 2S + 2
    inside the other (1x2: across x = 192 at a mid-segment row; 2x1: across
    y = 32 at a mid-strip column): the neighbour's obstacle reaches a unit's
    flag only through the obstacle map's ghost ring.  Once more with every
    wrap through the transport.

    That the sweep reaches both copies is shown per sweep here (at S = 10 and
    16-row segments every unit touching the owner can be flagged): the owner
    is always flagged, and the unit just across the border from the obstacle
    is clean at some distances and flagged at others."""
    S, _ = set_form(monkeypatch, form)
    kw = dict(DECOMPS[decomp])
    if force:
        kw["flags"] = gpu_lib.FLAG_FORCE_EXCHANGE
    across = set()
    for d in range(-(2 * S + 2), 2 * S + 3):
        x, y = (NX // 2 + d, 8) if decomp == "1x2" else (58 + (d & 1), NY // 2 + d)
        far = NX // 2 - (d >= 0) if decomp == "1x2" else NY // 2 - (d >= 0)  # first cell of the other sub-domain

        def on_units(units, ox, oy, where):
            owner = [u for u in units if inside(u, ox, oy)]
            assert len(owner) == 1 and owner[0][5] == 1, (where, owner)
            other = [u for u in units if inside(u, *((far, oy) if decomp == "1x2" else (ox, far)))]
            assert len(other) == 1 and other[0][6] != owner[0][6] and other[0][0] == 1, (where, other)
            across.add(other[0][5])

        run_lone(gpu_lib, form, lone(x, y), (2 * S - 1,), fused_stats(S), monkeypatch, (form, decomp, force, d),
                 on_units=on_units, **kw)
    assert across == {0, 1}


# ------------------------------------------------ c. order and flag knobs ----

def reordered(units):
    """The dispatch order differs from the unit order: in some launch (one
    sub-domain's interior or boundary units), inside one of the eight
    contiguous slot ranges the units are cut into (the first n % 8 ranges one
    unit longer; lbm_split.hip build_args moves each range's flagged units to
    its front), a clean unit precedes a flagged one."""
    launches = {}
    for (s, b, _, _, _, _, f) in units:
        launches.setdefault((s, b), []).append(f)
    for fl in launches.values():
        q, r = divmod(len(fl), 8)
        t0 = 0
        for x in range(8):
            rng = fl[t0:t0 + q + (x < r)]
            t0 += len(rng)
            if 0 in rng and 1 in rng[rng.index(0):]:
                return True
    return False


@gpu
@pytest.mark.parametrize("decomp", ["single", "2x2"])
@pytest.mark.parametrize("form", ["bitwise-S5-plain", "bitwise-S6-LP", "tolerance-S10"])
def test_order_flag_and_width_knobs(gpu_lib, debug_knobs, form, decomp, monkeypatch):
    """On a map where flagged and clean units sit side by side: the dispatch
    order changes neither the lattice nor any |u| sum (partials and flags are
    indexed by unit); without flags the lattice is the same and the sums differ
    by their order inside a lane only; the other strip width changes no
    lattice value.

    Four-row segments here: the dispatch order only moves units inside one of
    a launch's eight slot ranges, and with the family's 16-row segments those
    hold two units (single domain) or one (2x2), so the default order was the
    unit order on every contract map and LBM_STREAM_ORDER=0 showed nothing.
    That each knob took effect is asserted from stream_units()."""
    S, tol = set_form(monkeypatch, form, hs=4)
    obst = random_cells_map(2)
    cells0 = perturbed_cells()
    steps = 2 * S - 1

    def run(**env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        try:
            with engine(gpu_lib, obst, form, **DECOMPS[decomp]) as e:
                units = e.stream_units()
                e.load_cells(cells0)
                e.run_steps(steps, accelerate_first=True)
                return (*e.store(n_av=steps), units)
        finally:
            for k in env:
                monkeypatch.delenv(k)

    cells, av, units = run()
    assert {u[6] for u in units} == {0, 1}
    assert reordered(units), "the default dispatch order is the unit order on this map: ORDER=0 would show nothing"
    ref, ref_av = oracle.run(P, obst, steps, cells0)
    if tol:
        assert _rel(cells, ref) < TOL_POP
    else:
        assert np.array_equal(cells, ref)
        np.testing.assert_allclose(av, ref_av, rtol=1e-5)
    c, a, _ = run(LBM_STREAM_ORDER="0")
    assert np.array_equal(c, cells) and np.array_equal(a, av)
    c, a, u = run(LBM_STREAM_UOBST="0")
    assert {v[6] for v in u} == {-1}
    assert np.array_equal(c, cells)
    np.testing.assert_allclose(a, av, rtol=1e-5)
    default_ow16 = (tol and S <= 8) or S <= 5  # lbm_split.hip stream_split
    c, a, u = run(LBM_STREAM_OW16="0" if default_ow16 else "1")
    assert {v[6] for v in u} == {0, 1}
    wide, narrow = (units, u) if default_ow16 else (u, units)  # the knob took effect: 16-column widths or not
    assert max(v[4] for v in wide) % 16 == 0 and max(v[4] for v in narrow) % 16 != 0
    assert np.array_equal(c, cells)  # bitwise forms: cells == oracle, above


# --------------------------------- d. short segments, tolerance LP forms ----

@functools.lru_cache(maxsize=None)
def whole_segment_lattice(S, n):
    """The tolerance lattice after n steps of the 128x256 problem, single
    domain, one segment per strip; checked against the oracle once."""
    from lbm_amd import native
    p, obst = load_problem("128x256", iters=n)
    cells0 = lio.init_cells(p)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("LBM_DEBUG_KNOBS", "1")
        mp.setenv("LBM_STREAM_HS", "100000")
        with native.Engine(p, obst, devices=[0], kernel=native.KERNEL_STREAM, steps_per_launch=S,
                           flags=native.FLAG_TOLERANCE) as e:
            assert e.steps_per_launch() == S and e.numerics() == "tolerance"
            e.load_cells(cells0)
            e.run_steps(n, accelerate_first=True)
            whole = e.store(n_av=n)[0]
    assert _rel(whole, oracle.run(p, obst, n, cells0)[0]) < TOL_POP
    whole.setflags(write=False)
    return whole


@gpu
@pytest.mark.parametrize("hs", [1, 7, 100000])
@pytest.mark.parametrize("S", [7, 8, 9, 10])
def test_tolerance_lp_segments(gpu_lib, debug_knobs, S, hs, monkeypatch):
    """tests/test_gpu_parity.py test_stream_segments_bitwise for the tolerance
    LP forms S = 7..10: segments of one row, seven rows (< 2S) and the whole
    sub-domain give the same lattice bit for bit, single domain and 2x2
    loop-back, with and without a one-step remainder, within TOL_POP of the
    oracle."""
    p, obst = load_problem("128x256", iters=2 * S + 3)
    cells0 = lio.init_cells(p)

    def run(n, hs_, **kw):
        monkeypatch.setenv("LBM_STREAM_HS", str(hs_))
        with gpu_lib.Engine(p, obst, devices=[0], kernel=gpu_lib.KERNEL_STREAM, steps_per_launch=S,
                            flags=gpu_lib.FLAG_TOLERANCE, **kw) as e:
            assert e.kernel_in_use() == "stream" and e.steps_per_launch() == S and e.numerics() == "tolerance"
            e.load_cells(cells0)
            e.run_steps(n, accelerate_first=True)
            return e.store(n_av=n)[0]

    for n in (2 * S + 2, 2 * S + 3):
        for kw in (dict(), dict(parts=4, grid=(2, 2))):
            assert np.array_equal(run(n, hs, **kw), whole_segment_lattice(S, n)), (S, hs, n, kw)


# ------------------------------------- e. a lone obstacle in the other kernels ----

OTHER = {
    # mode -> (engine options, knobs, tile width, tile height)
    "resident-v1": (dict(kernel="RESIDENT"), {"LBM_RES_V": "1", "LBM_RES_TH": "8"}, 64, 8),
    "resident-v2": (dict(kernel="RESIDENT"), {"LBM_RES_V": "2", "LBM_RES_TH": "8"}, 128, 8),
    "step2-tile0": (dict(kernel="STEP2"), {"LBM_TILE2": "0"}, 64, 8),
    "step2-tile1": (dict(kernel="STEP2"), {"LBM_TILE2": "1"}, 64, 8),
    "vec4": (dict(kernel="VEC4", one_step=True), {}, 64, 8),
    "scalar": (dict(kernel="SCALAR", one_step=True), {}, 64, 8),
    "pipeline": (dict(kernel="PIPELINE"), {}, 64, 8),
}


@gpu
@pytest.mark.parametrize("mode", list(OTHER))
def test_other_kernels_lone_obstacle(gpu_lib, debug_knobs, mode, monkeypatch):
    """The packed resident kernel hands collide2u / collide2t a wave-uniform
    any_obst as the stream kernel does (lbm_resident.hip); the scalar resident
    tiles, the two-step, one-step and pipeline kernels have no such shortcut,
    and for them this is a lone-obstacle parity run, which the suite lacked
    too.  One obstacle cell at d in [-3, 3] around the first tile seam in x
    and in y (the tile of each mode as listed above), and around x = 128 and
    y = 16, which are seams of every tile shape up to 128 x 16 should the
    listed one not be the one in use; 256 x 32 perturbed cells, 5 steps,
    bitwise against the oracle (the pipeline against its own)."""
    opts, env, tw, th = OTHER[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nx, ny, steps = 256, 32, 5
    p = lio.Params(nx, ny, steps, 10, 0.1, 0.02, 1.7)
    cells0 = perturbed_cells(nx, ny, 21)
    kw = dict(kernel=getattr(gpu_lib, "KERNEL_" + opts["kernel"]),
              flags=gpu_lib.FLAG_ONE_STEP if opts.get("one_step") else 0)
    ref_run = oracle.pipe_run if mode == "pipeline" else oracle.run
    for d in range(-3, 4):
        for x, y in {(tw + d, th // 2), (tw // 2, th + d), (128 + d, 5), (37, 16 + d)}:
            obst = lone(x, y, nx, ny)
            with gpu_lib.Engine(p, obst, devices=[0], **kw) as e:
                assert e.kernel_in_use() == opts["kernel"].lower()
                e.load_cells(cells0)
                e.run_steps(steps, accelerate_first=True)
                cells, av = e.store(n_av=steps)
            ref, ref_av = ref_run(p, obst, steps, cells0)
            assert np.array_equal(cells, ref), (mode, d, x, y)
            np.testing.assert_allclose(av, ref_av, rtol=1e-5, err_msg=str((mode, d, x, y)))


# ------------------------------------------------ sensitivity (CPU only) ----

def test_lone_obstacle_is_observable():
    """The perturbed state makes a lone obstacle visible wherever a sweep puts
    it: after S steps the oracle's lattice with the obstacle differs from the
    obstacle-free one in a cell 1..S away (max-norm) -- a cell some other
    unit's halo would have to get right.  S = 6, the positions of an x sweep
    around column 116 (the first strip seam of the default form) and of a y
    sweep around row 32."""
    S = 6
    cells0 = perturbed_cells()
    free, _ = oracle.run(P, np.zeros((NY, NX), np.uint8), S, cells0)
    yy, xx = np.mgrid[0:NY, 0:NX]
    for d in range(-(2 * S + 2), 2 * S + 3):
        for x, y in ((116 + d, 24), (58, 32 + d), (d % NX, d % NY)):
            x, y = x % NX, y % NY
            with_obst, _ = oracle.run(P, lone(x, y), S, cells0)
            dx, dy = np.abs(xx - x), np.abs(yy - y)
            dist = np.maximum(np.minimum(dx, NX - dx), np.minimum(dy, NY - dy))
            ring = (dist >= 1) & (dist <= S)
            assert (with_obst != free).any(axis=2)[ring].any(), (x, y)
            assert not (with_obst != free).any(axis=2)[dist > S].any(), (x, y)  # and nothing travels faster
