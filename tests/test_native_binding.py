"""CPU-only checks of the ctypes binding's own logic (lbm_amd/native.py), no GPU call.

The public methods of Engine / Engine3D are driven on instances made with
object.__new__ whose library is a small fake: it records every call (name and,
per argument, the scalar value or whether the pointer is NULL), returns LBM_OK,
fills the out-parameters the binding reads back (counts, the rect list, the
local cell count) and fills packed output buffers with a running index.

* Chunk schedule of every *_history / run_* method: the run_steps arguments, the
  running totals, one lbm_store per chunk on D2Q9 (none for binned_history),
  accelerate_first on the first chunk only, validation before any call, the
  empty returns of steps == 0.
* Field selection: a subset lands in its header-order slots, an unknown or a
  repeated name is refused before any call, the defaults.
* The per-rect split of the *_local methods and the box outputs.
* Every exported symbol has its signature declared (real library, no GPU call).
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from lbm_amd import native

CARG = type(ctypes.byref(ctypes.c_int()))
RECTS = [(0, 0, 3, 2), (3, 0, 5, 4)]          # (x0, y0, w, h): 3x2 and 5x4
LOCAL_CELLS = sum(w * h for _, _, w, h in RECTS)
POINTS = 3


def _fill(ptr, values):
    np.ctypeslib.as_array(ptr, shape=(len(values),))[:] = values


class FakeLib:
    def __init__(self):
        self.calls = []          # (name, [described argument, ...])
        self.av = 0              # running value written into lbm_store's av_vels

    @staticmethod
    def describe(a):
        if a is None:
            return None
        if isinstance(a, ctypes.c_void_p):
            return "handle"
        if isinstance(a, (bool, int, float)):
            return a
        if isinstance(a, ctypes.Array):
            if issubclass(a._type_, ctypes._Pointer):
                return tuple("ptr" if p else None for p in a)
            return "ptr"
        if isinstance(a, ctypes._Pointer):
            return "ptr" if a else None
        if isinstance(a, CARG):
            o = a._obj
            if isinstance(o, native.Box3D):
                return ("box", o.x0, o.y0, o.z0, o.nx, o.ny, o.nz)
            return "ref"
        raise TypeError(f"unexpected argument {a!r}")

    def __getattr__(self, name):
        if not name.startswith("lbm"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, [self.describe(a) for a in args]))
            return self.fill(name, args)
        return call

    def fill(self, name, args):
        if name == "lbm_local_rects":
            _, rects, cap, n = args
            n._obj.value = len(RECTS)
            if rects is not None:
                for i, r in enumerate(RECTS[:cap]):
                    rects[i] = native.Rect(*r)
        elif name == "lbm_local_cells":
            return LOCAL_CELLS
        elif name.endswith("tracer_count"):
            args[1]._obj.value = POINTS
        elif name == "lbm_store":
            _, _, av, n_av = args
            _fill(av, np.arange(self.av, self.av + n_av))
            self.av += n_av
        elif name == "lbm_store_local":
            if args[1] is not None:
                _fill(args[1], np.arange(LOCAL_CELLS * native.Q))
        elif name in ("lbm_store_fields_local", "lbm_store_gradients_local", "lbm_store_stress_local"):
            slots = args[1:] if name == "lbm_store_fields_local" else list(args[1])
            for i, p in enumerate(slots):
                if p:
                    _fill(p, 1000 * i + np.arange(LOCAL_CELLS))
        elif name.endswith("last_error"):
            return b""
        elif name.endswith("destroy"):
            return None
        return native.LBM_OK

    def named(self, *names):
        return [(n, a) for n, a in self.calls if n in names]


def engine2d():
    e = object.__new__(native.Engine)
    e.params = native.Params(7, 5, 10, 10, 0.1, 0.005, 1.85)
    e._h = ctypes.c_void_p(1)
    e._L = FakeLib()
    return e


def engine3d():
    e = object.__new__(native.Engine3D)
    e.params = native.Params3D(8, 9, 10, 10, 0.1, 0.001, 1.85)
    e._h = ctypes.c_void_p(1)
    e._L = FakeLib()
    return e


ENGINES = {2: engine2d, 3: engine3d}
BINS = {2: (4, 4), 3: (4, 4, 4)}
BIN_SHAPE = {2: (2, 2), 3: (3, 3, 2)}           # ceil(extent / 4), slowest axis first


# ---------------------------------------------------------------------------------------------
# chunk schedule

def _steps_of_samples(r):
    return [s[0] for s in r[0]]


def _steps_of_list(r):
    return [s[0] for s in r]


def _steps_of_dict(r):
    assert r["step"].dtype == np.int64
    return list(r["step"])


# (dim, method) -> (call(e, steps, every, **kw), the library call of the sample, steps of the result or None,
#                   av_vels of the result or None)
HISTORY = {
    (2, "force_history"): (lambda e, s, k, **kw: e.force_history(s, k, **kw), "lbm_wall_force",
                           _steps_of_samples, lambda r: r[1]),
    (2, "gradient_history"): (lambda e, s, k, **kw: e.gradient_history(s, k, **kw), "lbm_gradient_stats",
                              _steps_of_samples, lambda r: r[1]),
    (2, "strain_history"): (lambda e, s, k, **kw: e.strain_history(s, k, **kw), "lbm_stress_stats",
                            _steps_of_samples, lambda r: r[1]),
    (2, "run_averaged"): (lambda e, s, k, **kw: e.run_averaged(s, k, **kw), "lbm_avg_sample", None, lambda r: r),
    (2, "binned_history"): (lambda e, s, k, **kw: e.binned_history(s, k, *BINS[2], **kw), "lbm_store_binned",
                            _steps_of_dict, None),
    (2, "run_traced"): (lambda e, s, k, **kw: e.run_traced(s, k, **kw), "lbm_tracer_advance", None, lambda r: r),
    (2, "probe_history"): (lambda e, s, k, **kw: e.probe_history(s, k, **kw), "lbm_tracer_sample",
                           _steps_of_dict, None),
    (3, "gradient_history"): (lambda e, s, k, **kw: e.gradient_history(s, k, **kw), "lbm3d_gradient_stats",
                              _steps_of_list, None),
    (3, "strain_history"): (lambda e, s, k, **kw: e.strain_history(s, k, **kw), "lbm3d_stress_stats",
                            _steps_of_list, None),
    (3, "run_averaged"): (lambda e, s, k, **kw: e.run_averaged(s, k, **kw), "lbm3d_avg_sample", None, None),
    (3, "binned_history"): (lambda e, s, k, **kw: e.binned_history(s, k, *BINS[3], **kw), "lbm3d_store_binned",
                            _steps_of_dict, None),
    (3, "run_traced"): (lambda e, s, k, **kw: e.run_traced(s, k, **kw), "lbm3d_tracer_advance", None, lambda r: r),
    (3, "probe_history"): (lambda e, s, k, **kw: e.probe_history(s, k, **kw), "lbm3d_tracer_sample",
                           _steps_of_dict, None),
}
HISTORY_IDS = [f"{m}{d}d" for d, m in HISTORY]
SCHEDULE = [((0, 3), []), ((2, 5), [2]), ((6, 3), [3, 3]), ((7, 3), [3, 3, 1])]


@pytest.mark.parametrize("key", list(HISTORY), ids=HISTORY_IDS)
@pytest.mark.parametrize("steps_every,chunks", SCHEDULE, ids=[f"{s}by{k}" for (s, k), _ in SCHEDULE])
def test_chunk_schedule(key, steps_every, chunks):
    dim, method = key
    call, sample, steps_of, av_of = HISTORY[key]
    e = ENGINES[dim]()
    r = call(e, *steps_every)
    run, store = ("lbm_run_steps", "lbm_store") if dim == 2 else ("lbm3d_run_steps", "lbm3d_store")
    got = e._L.named(run, store, sample)
    stores = dim == 2 and method != "binned_history"
    totals = list(np.cumsum(chunks))
    # run_steps, then store, then the sample, chunk by chunk
    assert [n for n, _ in got] == ([run] + ([store] if stores else []) + [sample]) * len(chunks)
    assert [a[1] for n, a in got if n == run] == chunks
    if dim == 2:
        assert [a[2] for n, a in got if n == run] == [0] * len(chunks)
        # one lbm_store per chunk with NULL cells and n_av = the chunk, except binned_history
        assert [a[1:] for n, a in got if n == store] == ([[None, "ptr", c] for c in chunks] if stores else [])
    if steps_of is not None:
        assert steps_of(r) == totals
    if av_of is not None:
        av = av_of(r)
        assert av.dtype == np.float32 and av.shape == ((sum(chunks),) if dim == 2 else (0,))
        assert np.array_equal(av, np.arange(av.size))          # each chunk's values, copied, in order
    if method == "run_traced":
        assert [a[1] for n, a in got if n == sample] == [float(c) for c in chunks]   # dt = the chunk's steps
    if (dim, method) == (3, "run_averaged"):
        assert r is None


@pytest.mark.parametrize("key", [k for k in HISTORY if k[0] == 2 and k[1] != "binned_history"],
                         ids=lambda k: k[1])
def test_accelerate_first_is_set_on_the_first_chunk_only(key):
    e = engine2d()
    HISTORY[key][0](e, 7, 3, accelerate_first=True)
    assert [a[1:] for _, a in e._L.named("lbm_run_steps")] == [[3, 1], [3, 0], [1, 0]]


@pytest.mark.parametrize("key", list(HISTORY), ids=HISTORY_IDS)
@pytest.mark.parametrize("steps,every", [(-1, 1), (1, 0)])
def test_bad_schedule_is_refused_before_any_library_call(key, steps, every):
    e = ENGINES[key[0]]()
    with pytest.raises(ValueError):
        HISTORY[key][0](e, steps, every)
    assert e._L.calls == []


@pytest.mark.parametrize("method", ["run_traced", "probe_history"])
def test_accelerate_first_is_refused_on_d3q19(method):
    e = engine3d()
    with pytest.raises(ValueError):
        HISTORY[(3, method)][0](e, 6, 3, accelerate_first=True)
    assert e._L.named("lbm3d_run_steps") == []


def test_empty_returns_of_zero_steps():
    e = engine2d()
    for m in ("force_history", "gradient_history", "strain_history"):
        samples, av = getattr(e, m)(0, 3)
        assert samples == [] and av.dtype == np.float32 and av.shape == (0,)
    for m in ("run_averaged", "run_traced"):
        av = getattr(e, m)(0, 3)
        assert isinstance(av, np.ndarray) and av.dtype == np.float32 and av.shape == (0,)
    e3 = engine3d()
    assert e3.gradient_history(0, 3) == [] and e3.strain_history(0, 3) == []
    assert e3.run_averaged(0, 3) is None
    av = e3.run_traced(0, 3)
    assert isinstance(av, np.ndarray) and av.dtype == np.float32 and av.shape == (0,)
    for dim, eng, names, points in ((2, e, native.BIN_FIELDS, native.TRACER_FIELDS),
                                    (3, e3, native.BIN_FIELDS3D, native.TRACER_FIELDS3D)):
        b = eng.binned_history(0, 3, *BINS[dim])
        assert set(b) == set(names) | {"step", "fluid"}
        for n in names:
            assert b[n].dtype == np.float64 and b[n].shape == (0,) + BIN_SHAPE[dim]
        assert b["step"].dtype == np.int64 and b["step"].shape == (0,)
        assert b["fluid"].dtype == np.int64 and b["fluid"].shape == BIN_SHAPE[dim]
        p = eng.probe_history(0, 3)
        assert set(p) == set(points) | {"step"}
        for n in points:
            assert p[n].dtype == np.float64 and p[n].shape == (0, POINTS)
        assert p["step"].dtype == np.int64 and p["step"].shape == (0,)
        assert eng._L.named("lbm_run_steps", "lbm3d_run_steps", "lbm_store", "lbm3d_store") == []


# ---------------------------------------------------------------------------------------------
# selection

# (dim, method) -> (call(e, **kw), names in header order, library call, dtype)
SELECT = {}
for _dim, _pre, _f, _g, _s, _b, _a, _t in (
        (2, "lbm_", native.FIELDS, native.GRAD_FIELDS, native.STRESS_FIELDS, native.BIN_FIELDS, native.AVG_FIELDS,
         native.TRACER_FIELDS),
        (3, "lbm3d_", native.FIELDS3D, native.GRAD_FIELDS3D, native.STRESS_FIELDS3D, native.BIN_FIELDS3D,
         native.AVG_FIELDS3D, native.TRACER_FIELDS3D)):
    SELECT[(_dim, "fields")] = (lambda e, **kw: e.fields(**kw), _f, _pre + "store_fields", np.float32)
    SELECT[(_dim, "gradients")] = (lambda e, **kw: e.gradients(**kw), _g, _pre + "store_gradients", np.float32)
    SELECT[(_dim, "strain_rate")] = (lambda e, **kw: e.strain_rate(**kw), _s, _pre + "store_stress", np.float32)
    SELECT[(_dim, "binned")] = (lambda e, _d=_dim, **kw: e.binned(*BINS[_d], **kw), _b, _pre + "store_binned",
                                np.float64)
    SELECT[(_dim, "avg_sums")] = (lambda e, **kw: e.avg_sums(**kw), _a, _pre + "avg_store_sums", np.float64)
    SELECT[(_dim, "mean_fields")] = (lambda e, **kw: e.mean_fields(**kw), _a, _pre + "avg_store", np.float32)
    SELECT[(_dim, "tracer_sample")] = (lambda e, **kw: e.tracer_sample(**kw), _t, _pre + "tracer_sample", np.float64)
SELECT_IDS = [f"{m}{d}d" for d, m in SELECT]


def _slots(e, fn, count):
    """The NULL / non-NULL pattern of the one `fn` call's output slots: its pointer table, or its
    last `count` positional arguments."""
    (_, args), = e._L.named(fn)
    tables = [a for a in args if isinstance(a, tuple) and a[:1] != ("box",)]
    if tables:
        (t,) = tables
        assert len(t) == count
        return list(t)
    return args[-count:]


@pytest.mark.parametrize("key", list(SELECT), ids=SELECT_IDS)
def test_a_subset_lands_in_its_header_order_slots(key):
    call, names, fn, dtype = SELECT[key]
    e = ENGINES[key[0]]()
    out = call(e, which=(names[-1], names[1]))
    want = [None] * len(names)
    want[1] = want[-1] = "ptr"
    assert _slots(e, fn, len(names)) == want
    got = {k: v for k, v in out.items() if k != "fluid"}
    assert set(got) == {names[1], names[-1]} and all(v.dtype == dtype for v in got.values())


@pytest.mark.parametrize("key", list(SELECT), ids=SELECT_IDS)
def test_the_default_selects_every_slot(key):
    call, names, fn, _ = SELECT[key]
    e = ENGINES[key[0]]()
    out = call(e)
    assert _slots(e, fn, len(names)) == ["ptr"] * len(names)
    assert set(out) - {"fluid"} == set(names)


@pytest.mark.parametrize("key", list(SELECT), ids=SELECT_IDS)
def test_an_unknown_or_repeated_name_is_refused_before_any_library_call(key):
    call, names, _, _ = SELECT[key]
    e = ENGINES[key[0]]()
    for which in ((names[0], "no_such_field"), (names[1], names[0], names[1])):
        with pytest.raises(ValueError, match=names[0]):          # the message names the allowed set
            call(e, which=which)
    assert e._L.calls == []


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("method,fn", [("avg_sums", "avg_store_sums"), ("mean_fields", "avg_store")])
def test_the_average_default_is_what_avg_begin_began(dim, method, fn):
    names = native.AVG_FIELDS if dim == 2 else native.AVG_FIELDS3D
    fn = ("lbm_" if dim == 2 else "lbm3d_") + fn
    e = ENGINES[dim]()
    e.avg_begin(second=False)
    assert e._L.calls[-1][1][1] == native.AVG_MEAN
    out = getattr(e, method)()
    first = dim + 1                                              # ux, uy[, uz], pressure
    assert _slots(e, fn, len(names)) == ["ptr"] * first + [None] * (len(names) - first)
    assert tuple(out) == names[:first]
    e = ENGINES[dim]()
    e.avg_begin()
    assert e._L.calls[-1][1][1] == native.AVG_MEAN | native.AVG_SECOND
    assert set(getattr(e, method)()) == set(names)


# ---------------------------------------------------------------------------------------------
# per-rect split, boxes

def _rect_slices(width=1):
    out, off = [], 0
    for _, _, w, h in RECTS:
        out.append((off, w, h))
        off += w * h * width
    return out


@pytest.mark.parametrize("method,names", [("fields_local", native.FIELDS), ("gradients_local", native.GRAD_FIELDS),
                                          ("strain_rate_local", native.STRESS_FIELDS)])
def test_local_diagnostics_split_the_packed_arrays_per_rect(method, names):
    e = engine2d()
    which = (names[-1], names[1])
    out = getattr(e, method)(which=which)
    assert len(out) == len(RECTS)
    for d, (off, w, h) in zip(out, _rect_slices()):
        assert set(d) == set(which)
        for f in which:
            assert d[f].dtype == np.float32 and d[f].shape == (h, w)
            assert np.array_equal(d[f], (1000 * names.index(f) + off + np.arange(w * h)).reshape(h, w))
    assert len(getattr(e, method)()[0]) == len(names)


def test_store_local_splits_the_packed_cells_per_rect():
    e = engine2d()
    blocks, av = e.store_local(n_av=4)
    assert av.shape == (4,) and av.dtype == np.float32 and len(blocks) == len(RECTS)
    for b, (off, w, h) in zip(blocks, _rect_slices(native.Q)):
        assert b.dtype == np.float32 and b.shape == (h, w, native.Q)
        assert np.array_equal(b, (off + np.arange(w * h * native.Q)).reshape(h, w, native.Q))
    blocks, av = e.store_local(cells=False, n_av=2)
    assert blocks is None and av.shape == (2,)
    assert e._L.calls[-1] == ("lbm_store_local", ["handle", None, "ptr", 2])


@pytest.mark.parametrize("method,fn,names", [("fields_box", "lbm3d_store_fields_box", native.FIELDS3D),
                                             ("gradients_box", "lbm3d_store_gradients_box", native.GRAD_FIELDS3D),
                                             ("strain_rate_box", "lbm3d_store_stress_box", native.STRESS_FIELDS3D)])
def test_box_methods_pass_the_box_and_shape_their_outputs(method, fn, names):
    e = engine3d()
    out = getattr(e, method)(1, 2, 3, 4, 5, 6)
    assert set(out) == set(names)
    assert all(a.shape == (6, 5, 4) and a.dtype == np.float32 for a in out.values())
    (_, args), = e._L.named(fn)
    assert args[1] == ("box", 1, 2, 3, 4, 5, 6)
    assert _slots(e, fn, len(names)) == ["ptr"] * len(names)
    e = engine3d()
    out = getattr(e, method)(1, 2, 3, 4, 5, 6, which=(names[-1], names[1]))
    want = [None] * len(names)
    want[1] = want[-1] = "ptr"
    assert _slots(e, fn, len(names)) == want and set(out) == {names[1], names[-1]}


# ---------------------------------------------------------------------------------------------
# signatures

def test_every_exported_symbol_has_its_signature_declared():
    L = native.load_library()
    lists = [getattr(native, n) for n in dir(native) if n.startswith("EXPORTED")]
    assert len(lists) >= 9
    for name in sum(lists, []):
        assert getattr(L, name).argtypes is not None, name
