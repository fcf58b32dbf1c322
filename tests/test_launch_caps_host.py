"""The clamp guard of the launch-clamp tests (tests/caps_cases.py, tests/test_gpu_launch_caps.py,
tests/test_gpu_launch_caps3d.py), on the CPU.

1. The clamps tests/caps_cases.py assumes are read out of csrc/ by regex and must equal what it
   states: raising one fails here and does not silently leave a GPU test inside a single trip.
2. Every shape exceeds its clamp, ends on a partial trip (a block with inactive lanes; for the chunk
   kernels, whose unit is a wave, a block with inactive waves) and is no more than twice the size it
   needs.  The 3-D box of more than 4 x 65535 rows is exempt from the last: it is there for gridDim.y.
3. The comparison the GPU modules share is fed one wrong bit in a cell of the last trip and must name
   that cell, its trip, block and lane.

Every launch in csrc/ whose grid is clamped, and the case that crosses the clamp:

  macroscopic_fields, moment sums / means, scalar_step, scalar_buoyancy  (fields_blocks, 8192 blocks of
      256 quads)                          4098 x 2047: test_gpu_launch_caps.py, the large handle
  count_nonfinite (4096 blocks of 256 cells)                       the same handle, nonfinite_count()
  scalar_phi, scalar_stats (scalar::blocks_for)                    the same handle; 3-D: 16 x 512 x 260
  scalar_fixed (scalar::blocks_for)       NO CASE: a second trip needs a fixed list of more than
      2 097 152 distinct cells, which set_fixed checks and sorts on the host; the kernel is the flat
      loop of scalar_phi with a 64-bit counter, and the large handle runs it with a short list
  advance / sample / flag tracers (tracers::blocks_for)            2 097 473 tracers on 37 x 19
  wall_force_total / _map, scalar_walls_pass, scalar_wall_flux_total / _map (wall_blocks, 1024 blocks)
                                          1100 x 1000 and 128 x 128 x 130, obstacles at even coordinates
  wall_force_chunks, scalar_wall_flux_chunks (body_blocks, 8192 blocks of four waves)   the same maps
      with every isolated cell a body of its own: more than 32 768 chunks
  wall_force_fold_chunks, scalar_wall_flux_fold (body_blocks)      NO CASE: a second trip needs more than
      32 768 bodies of several chunks (more than 512 wall cells) each, about 16 M wall cells
  scalar_step3d, scalar_buoyancy3d (slab_grid: 16384 blocks aimed for, gridDim.y at most 65535)
                                          8 x 512 x 130, 5 x 512 x 130, 5 x 262200 x 1
  macroscopic_fields3d, neq_strain3d (the same grid rule)          tests/test_gpu_fields3d.py
      (test_fields3d_grid_strides_bitwise) and the 5 x 262200 x 1 box
  velocity_gradients3d                    no stride loop: a grid past 65535 blocks (of 16 rows) in y is refused.
      5 x 262200 x 1 is 16 388 blocks and runs, pinned bitwise; 5 x 1048561 x 1 pins the refusal

Not clamped (the grid covers every unit, no stride loop): the step kernels, binned_sums / fold_bins and
their 3-D and transport forms (scalar_binned, scalar_binned3d), neq_strain, velocity_gradients,
edge_velocities, the layout conversions and the halo kernels.
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import caps_cases as cc
from lbm_amd import io as lio

CSRC = Path(__file__).resolve().parents[1] / "lbm-graphcore_amd" / "csrc"

# (file, regex with one group per value, the values caps_cases.py assumes)
CLAMPS = {
    "FIELDS_MAX_BLOCKS": ("lbm_fields.hip", r"constexpr int FIELDS_MAX_BLOCKS = (\d+);", (cc.FIELDS_MAX_BLOCKS,)),
    "BLOCK": ("lbm_layout.hpp", r"constexpr int BLOCK = (\d+);", (cc.BLOCK,)),
    "AVG_BLOCK": ("lbm_moments.hpp", r"constexpr int AVG_BLOCK = (\d+);", (cc.BLOCK,)),
    "scalar::BLOCK": ("lbm_scalar.hpp", r"constexpr int BLOCK = (\d+);", (cc.SCALAR_BLOCK,)),
    "scalar::MAX_BLOCKS": ("lbm_scalar.hpp", r"constexpr int MAX_BLOCKS = (\d+);", (cc.SCALAR_MAX_BLOCKS,)),
    "tracers::BLOCK": ("lbm_tracers.hpp", r"constexpr int BLOCK = (\d+);", (cc.TRACER_BLOCK,)),
    "tracers::MAX_BLOCKS": ("lbm_tracers.hpp", r"constexpr int MAX_BLOCKS = (\d+);", (cc.TRACER_MAX_BLOCKS,)),
    "WBLOCK": ("lbm_forces.hpp", r"constexpr int WBLOCK = (\d+);", (cc.WBLOCK,)),
    "WALL_MAX_BLOCKS": ("lbm_forces.hpp", r"constexpr int WALL_MAX_BLOCKS = (\d+);", (cc.WALL_MAX_BLOCKS,)),
    "BODY_MAX_BLOCKS": ("lbm_forces.hpp", r"constexpr int BODY_MAX_BLOCKS = (\d+);", (cc.BODY_MAX_BLOCKS,)),
    "BODY_CHUNK": ("lbm_forces.hpp", r"constexpr unsigned BODY_CHUNK = (\d+);", (cc.BODY_CHUNK,)),
    "S3X / S3Y": ("lbm3d_scalar.hip", r"constexpr int S3X = (\d+), S3Y = (\d+);", (cc.S3X, cc.S3Y)),
    "S3_TARGET_BLOCKS": ("lbm3d_scalar.hip", r"constexpr int S3_TARGET_BLOCKS = (\d+);", (cc.S3_TARGET_BLOCKS,)),
    "slab_grid gridDim.y": ("lbm3d_scalar.hip", r"\(long long\)a\.by \+ S3Y - 1\) / S3Y, (\d+)\);", (cc.GRID_YZ_MAX,)),
    "G3X / G3Y": ("lbm_gradients.hpp", r"constexpr int G3X = (\d+), G3Y = (\d+);", (cc.G3X, cc.G3Y)),
    "count_nonfinite": ("lbm_kernels.hip", r"blocks = \(unsigned\)std::min<long long>\((\d+), \(n \+ BLOCK - 1\) / BLOCK\);",
                        (cc.NONFINITE_MAX_BLOCKS,)),
}


def read_clamp(name, root=CSRC):
    fname, pattern, _ = CLAMPS[name]
    found = re.findall(pattern, (Path(root) / fname).read_text())
    assert len(found) == 1, f"{name}: {len(found)} matches of {pattern!r} in {fname}"
    return tuple(int(v) for v in (found[0] if isinstance(found[0], tuple) else (found[0],)))


def check_clamps(root=CSRC):
    for name, (_, _, want) in CLAMPS.items():
        got = read_clamp(name, root)
        assert got == want, (f"{name} is {got} in csrc/ and {want} in tests/caps_cases.py: the shapes of the "
                             f"launch-clamp tests were chosen for {want}; choose them anew")


@pytest.mark.parametrize("name", sorted(CLAMPS))
def test_clamp_is_what_the_shapes_assume(name):
    assert read_clamp(name) == CLAMPS[name][2], name


def test_an_edited_clamp_fails_the_guard(tmp_path):
    """Every constant raised in a scratch copy of its file: the guard names it."""
    for name, (fname, pattern, want) in CLAMPS.items():
        text = (CSRC / fname).read_text()
        m = re.search(pattern, text)
        raised = text[:m.start(1)] + str(2 * int(m.group(1))) + text[m.end(1):]
        root = tmp_path / name.replace(" ", "_").replace("/", "_").replace(":", "_")
        root.mkdir()
        for other in {f for f, _, _ in CLAMPS.values()}:
            (root / other).write_text(raised if other == fname else (CSRC / other).read_text())
        with pytest.raises(AssertionError, match=re.escape(name)):
            check_clamps(root)
    check_clamps()


def test_the_blocks_functions_still_clamp_as_assumed():
    """The launch-side expressions the Trips model restates."""
    text = {f: (CSRC / f).read_text() for f in ("lbm_fields.hip", "lbm_scalar.hpp", "lbm_tracers.hpp", "lbm_forces.hpp")}
    assert "std::min<long long>(FIELDS_MAX_BLOCKS, (quads + BLOCK - 1) / BLOCK)" in text["lbm_fields.hip"]
    for f in ("lbm_scalar.hpp", "lbm_tracers.hpp"):
        assert "b > MAX_BLOCKS ? MAX_BLOCKS : b" in text[f], f
    assert "b > WALL_MAX_BLOCKS ? WALL_MAX_BLOCKS : b" in text["lbm_forces.hpp"]
    assert "b > BODY_MAX_BLOCKS ? BODY_MAX_BLOCKS : b" in text["lbm_forces.hpp"]
    assert "(long long)waves + WBLOCK / 64 - 1) / (WBLOCK / 64)" in text["lbm_forces.hpp"]


# ---------------------------------------------------------------- the shapes ----

def _walls2d():
    obst, discs = cc.walls2d_obstacles()
    links = lio.wall_links(obst)
    labels, nbodies = cc.one_cell_labels(obst, discs)
    return obst, discs, links, labels, nbodies


def _flat_cases():
    """{id: (Trips, units a launch needs to cross the clamp with one unit)} of every flat launch."""
    nx, ny = cc.BIG_NX, cc.BIG_NY
    cases = {
        "quads 4098x2047": cc.quad_trips(nx, ny),
        "scalar_phi 4098x2047": cc.plane_trips(nx, ny),
        "scalar_stats 4098x2047": cc.region_trips(nx * ny),
        "count_nonfinite 4098x2047": cc.nonfinite_trips(nx * ny),
        "tracers": cc.tracer_trips(),
        "scalar_phi 16x512x260": cc.plane_trips(cc.BOX_FLAT[0], cc.BOX_FLAT[1] * cc.BOX_FLAT[2]),
        "scalar_stats 16x512x260": cc.region_trips(int(np.prod(cc.BOX_FLAT))),
        "scalar_phi 17x511x261": cc.plane_trips(cc.BOX_FLAT_RAGGED[0], cc.BOX_FLAT_RAGGED[1] * cc.BOX_FLAT_RAGGED[2]),
        "scalar_stats 17x511x261": cc.region_trips(int(np.prod(cc.BOX_FLAT_RAGGED))),
    }
    _, discs, links, labels, nbodies = _walls2d()
    nwall = int((links != 0).sum())
    cases["wall cells 1100x1000"] = cc.wall_trips(nwall)
    per_body = np.bincount(labels[links != 0], minlength=nbodies)
    cases["chunks 1100x1000"] = cc.chunk_trips(cc.chunk_count(per_body))
    slinks = lio.scalar_wall_links(_walls2d()[0])                       # the scalar's list: the four axis links
    cases["scalar wall cells 1100x1000"] = cc.wall_trips(int((slinks != 0).sum()))
    per_body = np.bincount(labels[slinks != 0], minlength=nbodies)
    cases["scalar chunks 1100x1000"] = cc.chunk_trips(cc.chunk_count(per_body))
    obst3, balls = cc.walls3d_obstacles()
    links3 = lio.wall_links3d(obst3)
    labels3, nbodies3 = cc.one_cell_labels(obst3, balls)
    cases["wall cells 128x128x130"] = cc.wall_trips(int((links3 != 0).sum()))
    per_body = np.bincount(labels3[links3 != 0], minlength=nbodies3)
    cases["chunks 128x128x130"] = cc.chunk_trips(cc.chunk_count(per_body))
    slinks3 = lio.scalar_wall_links3d(obst3)
    cases["scalar wall cells 128x128x130"] = cc.wall_trips(int((slinks3 != 0).sum()))
    per_body = np.bincount(labels3[slinks3 != 0], minlength=nbodies3)
    cases["scalar chunks 128x128x130"] = cc.chunk_trips(cc.chunk_count(per_body))
    return cases


FLAT = _flat_cases()
# the size each shape is allowed: twice what crosses its clamp.  The scalar plane and the region of the large
# handle ride on the quad launch's shape (four cells per quad: five and four trips), and count_nonfinite on it too;
# the chunk launches ride on the wall maps, whose size the 262 144 wall cells of the per-cell launches set (a
# one-cell body is one chunk: seven and nine trips).
RIDES_ALONG = ("scalar_phi 4098x2047", "scalar_stats 4098x2047", "count_nonfinite 4098x2047", "chunks 1100x1000",
               "chunks 128x128x130", "scalar chunks 1100x1000", "scalar chunks 128x128x130")
# 16 x 512 x 260 is 8320 whole blocks of either launch: its last trip is partial by whole blocks (128 of 8192
# work) and no block of it has an inactive lane.  17 x 511 x 261 is there for the ragged block.
WHOLE_BLOCKS = ("scalar_phi 16x512x260", "scalar_stats 16x512x260")


@pytest.mark.parametrize("name", sorted(FLAT))
def test_flat_shape_crosses_its_clamp_on_a_partial_trip(name):
    t = FLAT[name]
    assert t.wanted > t.max_blocks and t.trips >= 2, (name, t)
    assert 0 < t.last_count < t.span, (name, t.last_count)
    if name in WHOLE_BLOCKS:
        assert t.idle_lanes == 0 and -(-t.last_count // t.lanes) < t.max_blocks
    else:
        assert t.idle_lanes > 0, f"{name}: the last trip fills its last block"
    if name not in RIDES_ALONG:
        assert t.units <= 2 * (t.span + 1), f"{name}: {t.units} units, {t.span + 1} cross the clamp"
    print(f"{name}: {t.units} units, {t.wanted} blocks wanted of {t.max_blocks}, {t.trips} trips, "
          f"last trip {t.last_count} units, {t.idle_lanes} idle lanes")


def test_the_large_handle_is_the_shape_the_issue_names():
    t = cc.quad_trips(cc.BIG_NX, cc.BIG_NY)
    assert (-(-cc.BIG_NX // 4), t.units, t.wanted, t.trips, t.last_count) == (1025, 2_098_175, 8196, 2, 1023)
    assert t.where(t.units - 1) == (1, 3, 254) and t.idle_lanes == 1          # block 3 has one idle lane
    mask = cc.quad_last_trip_mask(cc.BIG_NX, cc.BIG_NY)
    # the second trip: 1023 quads of the last row, ending on the ragged two-cell quad and the wrap in x and y
    assert not mask[:-1].any() and mask[-1, 8:].all() and not mask[-1, :8].any() and cc.BIG_NX % 4 == 2
    assert int(mask.sum()) == 4 * 1022 + 2
    assert cc.plane_trips(cc.BIG_NX, cc.BIG_NY).trips == 5 and cc.region_trips(cc.BIG_NX * cc.BIG_NY).trips == 4
    assert cc.plane_trips(cc.BIG_NX, cc.BIG_NY).units == 2047 * 4100
    assert cc.nonfinite_trips(cc.BIG_NX * cc.BIG_NY).trips == 8


def test_the_wall_shapes():
    obst, discs, links, labels, nbodies = _walls2d()
    lone = cc.lattice_obstacles((cc.WALLS_NY, cc.WALLS_NX)) != 0
    assert int(lone.sum()) == 275_000
    for d in discs:
        ring = int(((links != 0) & d).sum())
        assert cc.BODY_CHUNK < ring < 5000, ring                      # a body of several chunks
    outside = lone & ~discs[0] & ~discs[1]
    assert (links[outside] != 0).all() and (links[outside] == 0xFF).mean() > 0.97   # isolated: all eight links
    assert nbodies == 2 + int(outside.sum()) and labels.max() == nbodies - 1
    last = cc.wall_last_trip_mask(links, labels, nbodies)
    assert last.any() and last.sum() == cc.wall_trips(int((links != 0).sum())).last_count
    o3 = cc.lattice_obstacles(cc.WALLS3D[::-1])
    assert int(o3.sum()) == 266_240 and o3.shape == (130, 128, 128)
    obst3, balls = cc.walls3d_obstacles()
    shell = int(((lio.wall_links3d(obst3) != 0) & balls[0]).sum())
    assert cc.BODY_CHUNK < shell < 2000, shell                         # a body of several chunks


@pytest.mark.parametrize("box", cc.BOXES_STRIDED)
def test_strided_boxes_stride_over_planes(box):
    nx, ny, nz = box
    gx, gy, gz = cc.slab_grid(nx, ny, nz)
    assert (gx, gy, gz) == (1, 128, 128)
    assert gz < nz <= 2 * gz and nz % gz != 0                         # planes 128 and 129 are strided
    assert gx * gy * gz == cc.S3_TARGET_BLOCKS
    m = cc.slab_last_trip_mask(nx, ny, nz)
    assert m[128:].all() and not m[:128].any()
    # a partial block in x: lanes 2 .. 63 (8 wide) or 2 .. 63 with a one-cell ragged lane 1 (5 wide) are idle
    assert -(-nx // 4) < cc.S3X


def test_refused_box_is_one_row_past_the_gradient_grid():
    nx, ny, nz = cc.BOX_REFUSED
    assert -(-ny // cc.G3Y) == cc.GRID_YZ_MAX + 1 and -(-(ny - 1) // cc.G3Y) == cc.GRID_YZ_MAX
    assert -(-cc.BOX_ROWS[1] // cc.G3Y) <= cc.GRID_YZ_MAX                # the rows box is not refused
    text = (CSRC / "lbm3d_gradients.hip").read_text()
    assert "if (g.y > 65535u || g.z > 65535u) return hipErrorInvalidValue;" in text
    assert "(unsigned)((a.by + G3Y - 1) / G3Y)" in text


def test_rows_box_strides_over_rows():
    nx, ny, nz = cc.BOX_ROWS
    gx, gy, gz = cc.slab_grid(nx, ny, nz)
    assert -(-ny // cc.S3Y) > cc.GRID_YZ_MAX and (gx, gy, gz) == (1, cc.GRID_YZ_MAX, 1)
    first_strided = gy * cc.S3Y
    assert first_strided < ny < 2 * first_strided
    assert (ny - first_strided) % cc.S3Y != 0 or ny - first_strided < first_strided   # the second trip is partial
    m = cc.slab_last_trip_mask(nx, ny, nz)
    assert m[0, first_strided:].all() and not m[0, :first_strided].any()


# ------------------------------------------------------------ planted error ----

def _flip(a, idx, bit=1):
    b = a.copy()
    cc.bits(b)[idx] ^= bit
    return b


def test_planted_bit_in_the_last_trip_is_reported_with_its_lane():
    nx, ny = 134, 70                                                     # the helper, on a small stand-in first
    ref = np.random.default_rng(1).random((ny, nx)).astype(np.float32)
    assert cc.first_difference(ref, ref.copy()) is None
    msg = cc.first_difference(_flip(ref, (69, 133)), ref, lambda y, x: cc.quad_where(nx, ny, y, x))
    assert "first at (69, 133)" in msg and "1 values differ" in msg and "cell 1 of the quad" in msg
    # the large handle's shape: one wrong low bit in the last cell of the second trip, and in its first
    nx, ny = cc.BIG_NX, cc.BIG_NY
    ref = np.zeros((ny, nx), np.float32)
    mask = cc.quad_last_trip_mask(nx, ny)
    ys, xs = np.nonzero(mask)
    for y, x, lane in ((ys[-1], xs[-1], "block 3, lane 254"), (ys[0], xs[0], "block 0, lane 0")):
        with pytest.raises(AssertionError) as err:
            cc.assert_same_bits(_flip(ref, (y, x)), ref, "planted", lambda yy, xx: cc.quad_where(nx, ny, yy, xx))
        text = str(err.value)
        assert f"first at ({y}, {x})" in text and "trip 1 of 2" in text and lane in text, text
    # a cell of the first trip is reported as such
    msg = cc.first_difference(_flip(ref, (5, 5)), ref, lambda yy, xx: cc.quad_where(nx, ny, yy, xx))
    assert "trip 0 of 2" in msg
    # fp64 values, NaN payloads and a flat list
    t = cc.tracer_trips()
    a = np.zeros(cc.TRACER_COUNT)
    msg = cc.first_difference(_flip(a, (cc.TRACER_COUNT - 1,)), a, lambda i: t.describe(i))
    assert f"first at ({cc.TRACER_COUNT - 1},)" in msg and "trip 1 of 2, block 1, lane 64 " in msg
    nan = np.array([np.nan, 1.0], np.float32)
    other = _flip(nan, (0,))
    assert np.isnan(other[0]) and cc.first_difference(other, nan) is not None
    assert cc.first_difference(other, nan, nan_as_one=True) is None
    assert cc.first_difference(np.array([1.0, np.nan], np.float32), nan, nan_as_one=True) is not None
    # assert_touched refuses a reference that left the last trip alone
    with pytest.raises(AssertionError):
        cc.assert_touched(ref, ref.copy(), mask, "untouched")
    cc.assert_touched(_flip(ref, (ys[3], xs[3])), ref, mask, "touched")
