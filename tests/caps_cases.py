"""What the launch-clamp tests share (tests/test_launch_caps_host.py, tests/test_gpu_launch_caps.py,
tests/test_gpu_launch_caps3d.py): the clamps of the grid-stride launches as the tests assume them, the
smallest shapes that cross each clamp at its product value, which cells or list entries of each shape
fall into the last (partial) trip, and the bit comparison that names the trip, block and lane of the
first cell that differs.

A "trip" is one pass of a kernel's stride loop: trip t of a flat launch covers the units
[t * span, (t + 1) * span) with span = max_blocks * lanes per block.  The unit is a quad of four cells
of a row (fields, averages, scalar step, kick), a cell of the padded scalar plane or of a region
(scalar_phi, scalar_stats), a list entry (fixed cells, tracers, wall cells) or a chunk of a body's wall
cells (one wave per chunk).  tests/test_launch_caps_host.py reads the constants out of csrc/ and fails
when one of them no longer equals what is written here or when a shape no longer crosses its clamp.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

# ---- the clamps (csrc/), as the shapes below assume them ----

BLOCK = 256                   # lbm_layout.hpp: the block of the fields, averages, scalar step and kick launches
FIELDS_MAX_BLOCKS = 8192      # lbm_fields.hip: fields_blocks(), used by all four
NONFINITE_MAX_BLOCKS = 4096   # lbm_kernels.hip: launch_count_nonfinite, one cell per lane
SCALAR_BLOCK = 256            # lbm_scalar.hpp scalar::BLOCK
SCALAR_MAX_BLOCKS = 8192      # scalar::MAX_BLOCKS: scalar_phi, scalar_stats, scalar_fixed
TRACER_BLOCK = 256            # lbm_tracers.hpp tracers::BLOCK
TRACER_MAX_BLOCKS = 8192      # tracers::MAX_BLOCKS: advance, sample, flag
WBLOCK = 256                  # lbm_forces.hpp: four waves
WALL_MAX_BLOCKS = 1024        # wall-force total and map, scalar wall pass, wall-flux total and map
BODY_MAX_BLOCKS = 8192        # the chunk kernels: one wave per chunk
BODY_CHUNK = 512              # most wall cells of a chunk
S3X, S3Y = 64, 4              # lbm3d_scalar.hip: a block is 64 lanes along x times 4 rows
S3_TARGET_BLOCKS = 16384      # blocks a 3-D scalar launch aims for: planes beyond are strided over
GRID_YZ_MAX = 65535           # the hardware's gridDim.y / .z, to which slab_grid clamps
G3X, G3Y = 16, 16             # lbm_gradients.hpp: rows of a velocity_gradients3d block (no row loop: a refusal beyond)
WAVE = 64


@dataclass(frozen=True)
class Trips:
    """A flat grid-stride launch over `units` units, `lanes` per block, at most `max_blocks` blocks."""
    units: int
    lanes: int
    max_blocks: int

    @property
    def wanted(self):          # blocks the launch would take without the clamp
        return -(-self.units // self.lanes)

    @property
    def span(self):            # units of one full trip
        return self.max_blocks * self.lanes

    @property
    def trips(self):
        return -(-self.units // self.span)

    @property
    def last_start(self):      # first unit of the last trip
        return (self.trips - 1) * self.span

    @property
    def last_count(self):
        return self.units - self.last_start

    @property
    def idle_lanes(self):      # inactive lanes of the last trip's last working block
        return -self.last_count % self.lanes

    def where(self, unit):
        """(trip, block, lane) that handles `unit`."""
        trip, r = divmod(int(unit), self.span)
        return trip, r // self.lanes, r % self.lanes

    def describe(self, unit):
        t, b, l = self.where(unit)
        return f"unit {int(unit)}: trip {t} of {self.trips}, block {b}, lane {l} (wave {l // WAVE}, lane {l % WAVE})"


# ---- 2-D: the large handle ----

BIG_NX, BIG_NY = 4098, 2047


def quad_trips(nx, ny):
    """fields / averages / scalar_step / scalar_buoyancy over an nx x ny sub-domain: one quad per lane."""
    return Trips(-(-nx // 4) * ny, BLOCK, FIELDS_MAX_BLOCKS)


def plane_trips(nx, rows):
    """scalar_phi over the padded plane of `rows` rows."""
    return Trips(rows * (-(-nx // 4) * 4), SCALAR_BLOCK, SCALAR_MAX_BLOCKS)


def region_trips(cells):
    """scalar_stats over the cells of one region."""
    return Trips(cells, SCALAR_BLOCK, SCALAR_MAX_BLOCKS)


def nonfinite_trips(cells):
    """count_nonfinite over the cells of one sub-domain."""
    return Trips(cells, BLOCK, NONFINITE_MAX_BLOCKS)


def quad_last_trip_mask(nx, ny):
    """bool[ny][nx]: the cells whose quad falls into the last trip of a quad launch."""
    t = quad_trips(nx, ny)
    qpr = -(-nx // 4)
    q = np.arange(ny, dtype=np.int64)[:, None] * qpr + (np.arange(nx, dtype=np.int64) // 4)[None, :]
    return q >= t.last_start


def quad_where(nx, ny, y, x):
    """Trip, block and lane of cell (y, x) in a quad launch."""
    t = quad_trips(nx, ny)
    return t.describe(int(y) * -(-nx // 4) + int(x) // 4) + f", cell {int(x) % 4} of the quad"


def plane_last_trip_mask(shape):
    """bool[...][nx]: the cells of an unpadded array of this shape that scalar_phi's last trip writes."""
    nx = shape[-1]
    rows = int(np.prod(shape[:-1]))
    t = plane_trips(nx, rows)
    sp = -(-nx // 4) * 4
    i = np.arange(rows, dtype=np.int64)[:, None] * sp + np.arange(nx, dtype=np.int64)[None, :]
    return (i >= t.last_start).reshape(shape)


def region_last_trip_mask(shape):
    """bool of this shape: the cells scalar_stats' last trip reads (a region is unpadded, row-major)."""
    n = int(np.prod(shape))
    return (np.arange(n, dtype=np.int64) >= region_trips(n).last_start).reshape(shape)


# ---- tracers ----

TRACER_GRID = (37, 19)
TRACER_PERIOD = 4099                      # tracer i starts where tracer i % 4099 starts
TRACER_COUNT = 2_097_152 + 321


def tracer_trips(n=TRACER_COUNT):
    return Trips(n, TRACER_BLOCK, TRACER_MAX_BLOCKS)


# ---- walls ----

WALLS_NX, WALLS_NY = 1100, 1000
WALLS3D = (128, 128, 130)                 # nx, ny, nz


def lattice_obstacles(shape):
    """uint8 of this shape: blocked wherever every coordinate is even -- isolated wall cells, each
    with all its neighbours fluid (the extents are even, so the periodic images are isolated too)."""
    assert all(n % 2 == 0 for n in shape)
    ob = np.ones(shape, bool)
    for axis, n in enumerate(shape):
        sel = (np.arange(n) % 2 == 0).reshape([-1 if a == axis else 1 for a in range(len(shape))])
        ob = ob & sel
    return ob.astype(np.uint8)


def walls2d_obstacles():
    """The isolated cells of lattice_obstacles plus two discs drawn as rings three cells thick (a few
    thousand wall cells each: bodies of several chunks).  Rings, because a filled disc with that many wall
    cells swallows so many isolated cells that fewer than 262 144 wall cells are left.  Returns
    (obst uint8[ny][nx], ring masks)."""
    obst = lattice_obstacles((WALLS_NY, WALLS_NX))
    yy, xx = np.mgrid[0:WALLS_NY, 0:WALLS_NX]
    d2 = lambda cx, cy: (xx - cx) ** 2 + (yy - cy) ** 2
    discs = [(d2(cx, cy) <= (r + 1.5) ** 2) & (d2(cx, cy) >= (r - 1.5) ** 2)
             for cx, cy, r in ((300, 300, 250), (800, 650, 180))]
    for d in discs:
        obst[d] = 1
    return obst, discs


def walls3d_obstacles():
    """The isolated cells of the 128 x 128 x 130 box (266 240 of them, which would fill whole blocks: 1040
    times 256) plus one solid ball of radius 8, a body of several chunks that makes the last block ragged.
    Returns (obst uint8[nz][ny][nx], [ball mask])."""
    nx, ny, nz = WALLS3D
    obst = lattice_obstacles((nz, ny, nx))
    zz, yy, xx = np.mgrid[0:nz, 0:ny, 0:nx]
    ball = (xx - 40) ** 2 + (yy - 70) ** 2 + (zz - 100) ** 2 <= 64
    obst[ball] = 1
    return obst, [ball]


def one_cell_labels(obst, solids=()):
    """(labels int32, nbodies): every blocked cell outside `solids` a body of its own, numbered in
    row-major order after the solids, each of which is one body (0, 1, ...)."""
    blocked = np.asarray(obst) != 0
    labels = np.full(blocked.shape, -1, np.int32)
    lone = blocked.copy()
    for b, m in enumerate(solids):
        labels[m] = b
        lone &= ~m
    n = int(lone.sum())
    labels[lone] = len(solids) + np.arange(n, dtype=np.int32)
    return labels, len(solids) + n


def wall_trips(nwall):
    """The per-wall-cell launches: one list entry per lane."""
    return Trips(nwall, WBLOCK, WALL_MAX_BLOCKS)


def chunk_count(cells_per_body):
    """Chunks of a body list: every body with wall cells is cut into chunks of at most BODY_CHUNK."""
    c = np.asarray(cells_per_body, np.int64)
    return int((-(-c[c > 0] // BODY_CHUNK)).sum())


def chunk_trips(nchunks):
    """The chunk kernels: one wave per chunk, so the unit is a chunk and a block holds four."""
    return Trips(nchunks, WBLOCK // WAVE, BODY_MAX_BLOCKS)


def wall_list_order(links, labels=None, nbodies=0):
    """Flat map indices of the wall cells in the order of the device list: row-major, and with bodies
    set stably sorted by body, unlabelled cells last."""
    cells = np.flatnonzero(np.asarray(links).ravel() != 0)
    if labels is None:
        return cells
    lab = np.asarray(labels).ravel()[cells].astype(np.int64)
    lab = np.where((lab < 0) | (lab >= nbodies), nbodies, lab)
    return cells[np.argsort(lab, kind="stable")]


def wall_last_trip_mask(links, labels=None, nbodies=0):
    """bool of links' shape: the wall cells the last trip of a per-wall-cell launch handles."""
    order = wall_list_order(links, labels, nbodies)
    mask = np.zeros(np.asarray(links).size, bool)
    mask[order[wall_trips(order.size).last_start:]] = True
    return mask.reshape(np.asarray(links).shape)


# ---- 3-D: slab_grid of lbm3d_scalar.hip ----

BOXES_STRIDED = [(8, 512, 130), (5, 512, 130)]     # nx, ny, nz: whole quads; one quad and a one-cell ragged tail
BOX_ROWS = (5, 262200, 1)                          # more rows than 4 x 65535
BOX_REFUSED = (5, G3Y * GRID_YZ_MAX + 1, 1)        # one row more than velocity_gradients3d's grid can cover
BOX_FLAT = (16, 512, 260)                          # scalar_phi<7> / scalar_stats<7>: 8320 whole blocks
BOX_FLAT_RAGGED = (17, 511, 261)                   # the same launches with a ragged last block and pad columns


def slab_grid(nx, ny, nz):
    """(gx, gy, gz) of scalar_step3d / scalar_buoyancy3d over a one-slab box."""
    cpl = 4 if nx >= 4 else 1                      # box_view: a full-row box at least 4 cells wide goes by quads
    lanes = -(-nx // cpl)
    gx = -(-lanes // S3X)
    gy = min(-(-ny // S3Y), GRID_YZ_MAX)
    gz = max(1, min(min(nz, GRID_YZ_MAX), S3_TARGET_BLOCKS // (gx * gy)))
    return gx, gy, gz


def slab_last_trip_mask(nx, ny, nz):
    """bool[nz][ny][nx]: the cells a block reaches only in the last trip of its plane or row loop."""
    gx, gy, gz = slab_grid(nx, ny, nz)
    z0 = (nz - 1) // gz * gz
    y0 = (ny - 1) // (gy * S3Y) * (gy * S3Y)
    m = np.zeros((nz, ny, nx), bool)
    if z0 > 0:
        m[z0:] = True
    if y0 > 0:
        m[:, y0:] = True
    return m


# ---- the comparison ----

def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def first_difference(got, ref, where=None, nan_as_one=False):
    """None when got and ref hold the same bits, else a message naming the first differing element
    (row-major) and, through where(*index), the trip, block and lane that produced it.  nan_as_one: a NaN
    matches a NaN whatever its payload (the positions must agree)."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return f"shape / dtype {got.shape} {got.dtype} against {ref.shape} {ref.dtype}"
    bad = bits(got) != bits(ref)
    if nan_as_one and got.dtype.kind == "f":
        bad &= ~(np.isnan(got) & np.isnan(ref))
    flat = bad.ravel()
    at = int(np.argmax(flat))
    if not flat[at]:
        return None
    idx = tuple(int(v) for v in np.unravel_index(at, got.shape))
    msg = f"{int(np.count_nonzero(flat))} values differ, first at {idx}: got {got[idx]!r} ({int(bits(got)[idx]):#x}) " \
          f"want {ref[idx]!r} ({int(bits(ref)[idx]):#x})"
    if where is not None:
        msg += "; " + where(*idx)
    return msg


def assert_same_bits(got, ref, what="", where=None, nan_as_one=False):
    msg = first_difference(got, ref, where, nan_as_one)
    assert msg is None, f"{what}: {msg}"


def assert_touched(after, before, mask, what=""):
    """The reference changed cells of the last trip: the comparison is not of untouched memory."""
    changed = (bits(after) != bits(before)) & mask
    assert changed.any(), f"{what}: no cell of the last trip differs from its begin state"
