"""Host-side mirror of instant-distance's public API over the MI355X engine.

Same names, argument meaning and error behaviour as the reference
(/root/reference/instant-distance/src/lib.rs; Python flavour follows
/root/reference/instant-distance-py/src/lib.rs):

    Builder  (core/lib.rs:23-113)     Heuristic (core/lib.rs:115-128)
    Hnsw     (core/lib.rs:194-397)    HnswMap   (core/lib.rs:131-173)
    Search   (core/lib.rs:560-574)    Item / MapItem (core/lib.rs:399-413, 175-191)
    PointId  (core/types.rs:241-253)  -> plain int (u32)

`Point::distance` (core/lib.rs:780-782) is arbitrary user code in the reference and
cannot run on a GPU; here a point is an f32 vector and the distance is one of the two
the reference itself ships: squared L2 (FloatArray, the default) or L2 with sqrt
(the Point of tests/all.rs and examples/colors.rs) — `Builder.metric()`.  METRIC_COSINE (not in the reference) is
squared L2 over rows and queries the engine normalises itself, reported as 1 - cos; METRIC_DOT (not in the reference either) is
squared L2 over rows the engine gives one more coordinate, reported as -q.x; the host copies stay the caller's rows.

All compute goes through the C ABI (include/idist.h); there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import itertools
import secrets
from dataclasses import dataclass
from typing import Any, Iterator, Sequence

import numpy as np

from . import _capi
from ._capi import INVALID, M, M2, METRIC_COSINE, METRIC_DOT, METRIC_L2, METRIC_L2SQ, RUNG_EXACT, RUNG_NONE, TIES_DROP, TIES_STRICT

PointId = int


def _lib():
    return _capi.lib()


@dataclass
class Heuristic:
    """core/lib.rs:115-128"""
    extend_candidates: bool = False
    keep_pruned: bool = True


class Builder:
    """Parameters for building the `Hnsw` (core/lib.rs:23-113)."""

    def __init__(self):
        c = _lib().default_config()
        self._ef_search = int(c.ef_search)              # core/lib.rs:104
        self._ef_construction = int(c.ef_construction)  # :105
        self._heuristic: Heuristic | None = Heuristic() # :106
        self._ml = float(c.ml)                          # :107
        self._seed = secrets.randbits(64)               # :108 rand::random()
        self._metric = METRIC_L2SQ
        self._max_batch = 0
        self._device = 0
        self._progress = None
        self._tie_policy = TIES_STRICT
        self._tie_capacity = 0
        self._dot_bound = 0.0

    @classmethod
    def default(cls) -> "Builder":
        return cls()

    # -- reference setters (core/lib.rs:35-68) --
    def ef_construction(self, ef_construction: int) -> "Builder":
        self._ef_construction = int(ef_construction)
        return self

    def ef_search(self, ef: int) -> "Builder":
        self._ef_search = int(ef)      # does NOT touch ef_construction (code, not the doc comment)
        return self

    def select_heuristic(self, params: Heuristic | None) -> "Builder":
        self._heuristic = params
        return self

    def ml(self, ml: float) -> "Builder":
        self._ml = float(np.float32(ml))
        return self

    def seed(self, seed: int) -> "Builder":
        self._seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        return self

    def progress(self, bar) -> "Builder":
        """Builder::progress (core/lib.rs:70-75, `indicatif` feature): track the construction.  `bar` is a
        callable `bar(done, total, layer)` — the bar's position, length and the layer named in its message
        (`layer` is None outside the per-layer loop) — called from a watcher thread while the build runs and
        once more when it is finished (`bar.finish()`, :332-334)."""
        self._progress = bar
        return self

    # -- additions of this engine --
    def metric(self, metric: int) -> "Builder":
        """METRIC_L2SQ (FloatArray, py/lib.rs:378-421), METRIC_L2 (tests/all.rs:93-97) or METRIC_COSINE: the cosine distance
        1 - cos, defined as the METRIC_L2SQ index over the rows normalised by `normalize()`'s arithmetic (the engine does it where
        the rows reach the device, and to every query), with distances reported as half the squared L2 distance of the
        normalised vectors.  `points`, `Item.point` and `__getitem__` keep the caller's rows; rows without a positive finite norm
        (zero, NaN, inf) take part unchanged.
        METRIC_DOT: the inner product, nearest = largest q.x, defined as the METRIC_L2SQ index over the rows `augment_dot()`
        returns — every row gets the extra coordinate sqrt(S - |x|^2), S the bound `dot_bound()` sets or the largest squared norm
        of the rows, every query a trailing 0 — with distances reported as 0.5 * (d - (|q|^2 + S)), approximately -q.x.  The
        error of a reported distance is of the order eps * (|q|^2 + S), not eps * |q.x|: one row with a giant norm coarsens all
        the others.  `points`, `Item.point` and `__getitem__` keep the caller's dim-wide rows; rows with a NaN / inf squared
        norm get the extra coordinate 0."""
        self._metric = int(metric)
        return self

    def dot_bound(self, bound: float) -> "Builder":
        """METRIC_DOT only: the bound S on the squared norms of the rows (finite, >= every finite row's; 0 = the default, derive it
        from the rows).  Indexes that are searched as one (PartitionedHnsw) or compared with each other need the same S;
        `Hnsw.info().dot_bound` reports the one in use."""
        self._dot_bound = float(np.float32(bound))
        return self

    def tie_policy(self, policy: int) -> "Builder":
        """TIES_STRICT (default): results are the reference's whatever the number of un-expanded candidates exactly at
        the furthest distance (the tie region grows, then spills to HBM; IdistError(6) only reaches callers of the
        device-pointer API, whose next launch has the room).  TIES_DROP: keep the 64 nearest, go on
        (mass-duplicate data; deterministic, flagged in build_stats().tie_overflow / Search.tie_overflowed())."""
        self._tie_policy = int(policy)
        return self

    def tie_capacity(self, n: int) -> "Builder":
        """Entries of the LDS tie region behind `nearest` (0 = 64, at most 4096).  Strict builds / searches enlarge it
        by themselves and spill to HBM beyond 4096, so this only pre-sizes it for data with masses of exactly equal
        distances (dense integer grids)."""
        self._tie_capacity = int(n)
        return self

    def max_batch(self, k: int) -> "Builder":
        """1 = strictly sequential insertion (deterministic contract); 0 = default."""
        self._max_batch = int(k)
        return self

    def device(self, device: int) -> "Builder":
        self._device = int(device)
        return self

    def into_parts(self):
        """core/lib.rs:87-98"""
        return (self._ef_search, self._ef_construction, self._ml, self._seed)

    def _config(self) -> _capi.Config:
        c = _lib().default_config()
        c.ef_search = self._ef_search
        c.ef_construction = self._ef_construction
        c.ml = self._ml
        c.has_heuristic = 0 if self._heuristic is None else 1
        c.extend_candidates = int(bool(self._heuristic and self._heuristic.extend_candidates))
        c.keep_pruned = int(bool(self._heuristic.keep_pruned)) if self._heuristic else 1
        c.metric = self._metric
        c.max_batch = self._max_batch
        c.tie_policy = self._tie_policy
        c.tie_capacity = self._tie_capacity
        c.dot_bound = self._dot_bound
        return c

    def build(self, points, values: Sequence[Any]) -> "HnswMap":
        """Builder::build (core/lib.rs:78-80)."""
        return HnswMap._new(points, values, self)

    def build_hnsw(self, points) -> tuple["Hnsw", list[PointId]]:
        """Builder::build_hnsw (core/lib.rs:83-85): (index, original index -> PointId)."""
        return Hnsw._new(points, self)


class _BuildWatch:
    """Arms an idist_progress for the build call of this thread and polls it from a watcher thread."""

    def __init__(self, bar, period: float = 0.05):
        self.bar, self.period, self.h, self._stop, self._thr = bar, period, None, None, None

    def __enter__(self):
        if self.bar is None:
            return self
        import threading

        L = _lib()
        h = C.c_void_p()
        L.check(L.idist_progress_new(C.byref(h)))
        self.h = h
        L.check(L.idist_progress_watch_next_build(h))
        self._stop = threading.Event()

        def poll():
            last = None
            while not self._stop.wait(self.period):
                cur = self._read()
                if cur != last and cur[1]:
                    self.bar(*cur)
                    last = cur

        self._thr = threading.Thread(target=poll, daemon=True)
        self._thr.start()
        return self

    def _read(self):
        d, t, l = C.c_uint64(0), C.c_uint64(0), C.c_int32(-1)
        _lib().idist_progress_get(self.h, C.byref(d), C.byref(t), C.byref(l))
        return int(d.value), int(t.value), (int(l.value) if l.value >= 0 else None)

    def __exit__(self, et, ev, tb):
        if self.h is None:
            return False
        self._stop.set()
        self._thr.join()
        _lib().idist_progress_watch_next_build(None)     # disarm if the build call never consumed it
        if et is None:
            self.bar(*self._read())                       # finish: done == total
        _lib().idist_progress_free(self.h)
        self.h = None
        return False


class Search:
    """Reusable search scratch, `Search::default()` (core/lib.rs:560-574, 767-778).

    After `Hnsw.search(point, search)` it holds that query's results and is an
    iterator over them like the binding's Search (py/lib.rs:177-208)."""

    def __init__(self, slots: int = 0):
        self._slots = slots
        self._ctx = None
        self._owner = None
        self._items: list = []
        self._cur = 0

    def _bind(self, hnsw: "Hnsw"):
        if self._owner is not hnsw:
            self._release()
            ctx = C.c_void_p()
            _lib().check(_lib().idist_search_ctx_new(hnsw._h, self._slots, C.byref(ctx)))
            self._ctx = ctx
            self._owner = hnsw
        return self._ctx

    def _release(self):
        if self._ctx is not None:
            _lib().idist_search_ctx_free(self._ctx)
            self._ctx = None
            self._owner = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def reserve(self, hnsw: "Hnsw", slots: int):
        """Back `slots` query slots now (idist_search_ctx_reserve): later launches up to that width never synchronise
        the device to grow the context."""
        _lib().check(_lib().idist_search_ctx_reserve(self._bind(hnsw), int(slots)))

    def allowed_kernel_ms(self) -> tuple[float, float, float]:
        """HIP-event time (ms) of the select passes, the pending-list passes and the exact step (scan + merge) of the last
        `search_allowed` through this Search; the rungs' own search kernels are in `kernel_times_ms`."""
        a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
        _lib().check(_lib().idist_search_ctx_allowed_kernel_ms(self._ctx, C.byref(a), C.byref(b), C.byref(c)))
        return float(a.value), float(b.value), float(c.value)

    def attr_bitmap_ms(self) -> float:
        """HIP-event time (ms) of the bitmap kernel of the last `search_where` / `search_range_where` through this Search."""
        ms = C.c_float(0)
        _lib().check(_lib().idist_search_ctx_attr_bitmap_ms(self._ctx, C.byref(ms)))
        return float(ms.value)

    def range_kernel_ms(self) -> tuple[float, float, float]:
        """HIP-event time (ms) of the select passes (limits, within-prefixes, offsets, copies, pending lists), the exact step's two
        scans and the sort of the last `search_range` through this Search; the rungs' own search kernels are in `kernel_times_ms`."""
        a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
        _lib().check(_lib().idist_search_ctx_range_kernel_ms(self._ctx, C.byref(a), C.byref(b), C.byref(c)))
        return float(a.value), float(b.value), float(c.value)

    def kernel_times_ms(self, last: int = 64) -> np.ndarray:
        """HIP-event durations of the most recent search kernels launched through this Search."""
        out = np.zeros(last, dtype=np.float32)
        n = C.c_uint32(0)
        _lib().check(_lib().idist_search_ctx_kernel_times(self._ctx, _capi.f32p(out), last, C.byref(n)))
        return out[: n.value]

    def tie_overflowed(self) -> bool:
        """TIES_DROP only: did a search through this Search exceed the tie capacity since the last call?"""
        out = C.c_int32(0)
        _lib().check(_lib().idist_search_ctx_tie_overflowed(self._ctx, C.byref(out)))
        return bool(out.value)

    def filter_counts(self, reset: bool = True) -> tuple[int, int]:
        """(candidates the walk's reject filter examined, f32 rows it spared) over this Search's launches since the last reset —
        diagnostics; results never depend on the filter.  Synchronise first."""
        if self._ctx is None:
            return 0, 0
        a, b = C.c_uint64(0), C.c_uint64(0)
        _lib().check(_lib().idist_search_ctx_filter_counts(self._ctx, C.byref(a), C.byref(b), 1 if reset else 0))
        return int(a.value), int(b.value)

    def filter_principal_counts(self, reset: bool = True) -> tuple[int, int]:
        """The part of `filter_counts()` that was read from the 64-byte principal rows (`Hnsw.info().filter_format`): queries the
        index's basis does not fit are served from the identity rows in the same launch.  Its own reset.  Synchronise first."""
        if self._ctx is None:
            return 0, 0
        a, b = C.c_uint64(0), C.c_uint64(0)
        _lib().check(_lib().idist_search_ctx_filter_principal_counts(self._ctx, C.byref(a), C.byref(b), 1 if reset else 0))
        return int(a.value), int(b.value)

    def filter_inline_counts(self, reset: bool = True) -> tuple[int, int]:
        """(4096-byte blocks of principal rows stored with the adjacency that the walks requested, blocks they tested) — indexes with
        `Hnsw.info().filter_inline_bytes` only.  Its own reset.  Synchronise first."""
        if self._ctx is None:
            return 0, 0
        a, b = C.c_uint64(0), C.c_uint64(0)
        _lib().check(_lib().idist_search_ctx_filter_inline_counts(self._ctx, C.byref(a), C.byref(b), 1 if reset else 0))
        return int(a.value), int(b.value)

    def check_status(self):
        """Raise if a device-side guard tripped during the launches so far (after a stream sync)."""
        _lib().check(_lib().idist_search_ctx_status(self._ctx))

    def __iter__(self):
        return self

    def __next__(self):
        if self._cur >= len(self._items):
            raise StopIteration
        it = self._items[self._cur]
        self._cur += 1
        return it

    def __len__(self):
        return len(self._items)


@dataclass
class Item:
    """core/lib.rs:399-413"""
    distance: float
    pid: PointId
    point: np.ndarray


@dataclass
class MapItem:
    """core/lib.rs:175-191"""
    distance: float
    pid: PointId
    point: np.ndarray
    value: Any


@dataclass
class BatchResult:
    pid: np.ndarray       # [nq, ef_search] uint32, INVALID padded
    distance: np.ndarray  # [nq, ef_search] float32, +inf padded
    count: np.ndarray     # [nq]
    counters: np.ndarray | None  # [nq, 3] {n_dist, n_exp0, n_expU}


@dataclass
class AllowedResult:
    """`Hnsw.search_allowed`: every query holds exactly min(k, allowed points) results."""
    pid: np.ndarray       # [nq, k] uint32, INVALID padded
    distance: np.ndarray  # [nq, k] float32, +inf padded
    count: np.ndarray     # [nq]
    rung: np.ndarray      # [nq] the rung of the ef ladder that answered the query, RUNG_EXACT (the scan of the allowed rows) or RUNG_NONE
    counters: np.ndarray | None  # [nq, 3] {n_dist, n_exp0, n_expU} summed over the rungs the query ran


@dataclass
class GroupedResult(AllowedResult):
    """`Hnsw.search_grouped`: an `AllowedResult` whose rows hold pairwise distinct groups, each represented by its nearest member."""
    group: np.ndarray     # [nq, k] uint32, the group of every result; 0 padded


@dataclass
class RangeResult:
    """`Hnsw.search_range`: query q owns the entries [lims[q], lims[q + 1]) of `pid` and `distance`, nearest first."""
    lims: np.ndarray      # [nq + 1] uint64, lims[0] = 0
    pid: np.ndarray       # [lims[nq]] uint32
    distance: np.ndarray  # [lims[nq]] float32, as the metric reports them
    rung: np.ndarray      # [nq] the rung of the ef ladder that answered the query, RUNG_EXACT (the scan of every row) or RUNG_NONE
    counters: np.ndarray | None  # [nq, 3] {n_dist, n_exp0, n_expU} summed over the rungs the query ran


def allowed_bitmap(allowed, n: int) -> np.ndarray:
    """The allowed set of `search_allowed` as the ABI takes it: (n + 31) // 32 u32 words, bit pid % 32 of word pid // 32.  `allowed`: a
    bool array of length n in PointId order, or an integer array of PointIds (duplicates are harmless)."""
    a = np.asarray(allowed)
    if a.dtype == np.bool_:
        if a.shape != (n,):
            raise ValueError(f"a bool `allowed` must have one entry per point: shape ({n},), got {a.shape}")
        mask = a
    else:
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise TypeError("`allowed` is a bool mask of length n or an integer array of PointIds")
        ids = a.astype(np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= n):
            raise IndexError(f"`allowed` names a PointId outside [0, {n})")
        mask = np.zeros(n, dtype=bool)
        mask[ids] = True
    words = (n + 31) // 32
    padded = np.zeros(words * 32, dtype=np.uint8)
    padded[:n] = mask
    return np.ascontiguousarray(np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32))


def allowed_bitmaps(sets, n: int) -> np.ndarray:
    """The allowed sets of `search_allowed_sets` as the ABI takes them: uint32 [n_sets][(n + 31) // 32].  `sets`: a ready bitmap of that
    shape and dtype, a 2-D bool array [n_sets][n], or a sequence whose entries follow `allowed_bitmap`'s rules (bool masks of length
    n, integer arrays of PointIds)."""
    words = (n + 31) // 32
    if isinstance(sets, np.ndarray) and sets.ndim == 2 and sets.dtype == np.uint32:
        if sets.shape[1] != words:
            raise ValueError(f"a uint32 `sets` is a bitmap of shape (n_sets, {words}), got {sets.shape}")
        return np.ascontiguousarray(sets)
    if isinstance(sets, np.ndarray) and sets.dtype == np.bool_:
        if sets.ndim != 2 or sets.shape[1] != n:
            raise ValueError(f"a bool `sets` must have one row per set and one entry per point: shape (n_sets, {n}), got {sets.shape}")
    elif isinstance(sets, np.ndarray) and sets.ndim != 2 and sets.dtype != object:
        raise ValueError("`sets` is a sequence of sets, a 2-D bool array or a uint32 bitmap [n_sets][words]")
    out = np.zeros((len(sets), words), dtype=np.uint32)
    for i, a in enumerate(sets):
        out[i] = allowed_bitmap(a, n)
    return out


def _set_of(set_of, n_sets: int, nq: int):
    """`set_of` of the several-sets calls as the ABI takes it: uint32 [nq], or None (query q uses set q) when it is None."""
    if set_of is None:
        if n_sets != nq:
            raise ValueError(f"set_of=None means one set per query: {n_sets} sets for {nq} queries")
        return None
    so = np.asarray(set_of)
    if so.size and not np.issubdtype(so.dtype, np.integer):
        raise TypeError("`set_of` is an integer array of set indices, one per query")
    if so.shape != (nq,):
        raise ValueError(f"`set_of` must have one entry per query: shape ({nq},), got {so.shape}")
    if so.size and (so.min() < 0 or so.max() >= n_sets):
        raise IndexError(f"`set_of` names a set outside [0, {n_sets})")
    return np.ascontiguousarray(so.astype(np.uint32))


def _as_u32(x, what: str) -> np.ndarray:
    """integers as the ABI's uint32, shape kept; anything outside [0, 2**32) raises instead of wrapping"""
    a = np.asarray(x)
    if a.dtype == object:                                  # Python ints beyond int64
        flat = [v for v in a.reshape(-1)]
        if not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in flat):
            raise TypeError(f"`{what}` holds integers")
        if any(not 0 <= int(v) <= 0xFFFFFFFF for v in flat):
            raise ValueError(f"`{what}` holds a value outside the uint32 range [0, 2**32)")
        return np.array([int(v) for v in flat], dtype=np.uint32).reshape(a.shape)
    if a.size and (a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer)):
        raise TypeError(f"`{what}` holds integers, got {a.dtype}")
    if a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
        raise ValueError(f"`{what}` holds a value outside the uint32 range [0, 2**32)")
    return a.astype(np.uint32)


def _conditions(lo, hi, nq: int) -> tuple[np.ndarray, np.ndarray, int]:
    """The intervals of a `search_where` call as the ABI takes them: (lo, hi, n_cond).  `lo` / `hi`: scalars (one condition for the
    batch) or arrays of nq (one per query; a scalar next to an array is repeated); hi=None means equality."""
    lo_a = _as_u32(lo, "lo")
    hi_a = lo_a if hi is None else _as_u32(hi, "hi")
    for a, what in ((lo_a, "lo"), (hi_a, "hi")):
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != nq):
            raise ValueError(f"`{what}` is one integer or an array of nq = {nq}, got shape {a.shape}")
    if lo_a.ndim == 0 and hi_a.ndim == 0:
        return lo_a.reshape(1).copy(), hi_a.reshape(1).copy(), 1
    return (np.ascontiguousarray(np.broadcast_to(lo_a, (nq,))), np.ascontiguousarray(np.broadcast_to(hi_a, (nq,))), nq)


class Attr:
    """One uint32 per point, on the device next to the rows (idist_attr): what `search_where` / `search_range_where` compare a
    query's interval with.  Made by `Hnsw.attributes` / `PartitionedHnsw.attributes` and bound to that index: any other raises
    IdistError.  Immutable; `values` keeps the host copy."""

    def __init__(self, handle, owner, values: np.ndarray):
        self._h = handle
        self._owner = owner           # (kept alive: the handle names it)
        self.values = values

    def __len__(self):
        return self.values.shape[0]

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None:
                _lib().idist_attr_free(self._h)
                self._h = None
        except Exception:
            pass


def _attr_values(values, n: int) -> np.ndarray:
    v = _as_u32(values, "values")
    if v.shape != (n,):
        raise ValueError(f"`values` must have one entry per point: shape ({n},), got {v.shape}")
    return np.ascontiguousarray(v)


class AttrTable(Attr):
    """Several uint32 columns per point on the device (idist_attr_new_columns): what `search_match` / `search_range_match` evaluate
    a query's condition over.  Made by `attribute_table`.  `names`: the columns in order; `columns`: name -> the uint32 host copy
    [n]; `values`: column 0, the one `search_where` / `search_range_where` read when they are given a table."""

    def __init__(self, handle, owner, names: list, cols: np.ndarray):
        super().__init__(handle, owner, cols[0] if len(names) else np.zeros(cols.shape[1], np.uint32))
        self.names = list(names)
        self.n_cols = len(self.names)
        self.columns = {name: cols[i] for i, name in enumerate(self.names)}
        self._n = int(cols.shape[1])

    def __len__(self):
        return self._n


def _table_columns(columns, n: int) -> tuple[list, np.ndarray]:
    """`columns` of `attribute_table` as (names, uint32 [n_cols][n], column after column): a dict name -> integer array [n], or an
    integer array [n, n_cols] whose columns are named "0", "1", ...; the checks of `attributes()` per column."""
    if isinstance(columns, dict):
        names = list(columns)
        if not all(isinstance(name, str) for name in names):
            raise TypeError("the columns of an attribute table are named by strings")
        cols = [_attr_values(columns[name], n) for name in names]
        return names, (np.ascontiguousarray(np.stack(cols)) if cols else np.zeros((0, n), np.uint32))
    a = _as_u32(columns, "columns")
    if a.ndim != 2 or a.shape[0] != n:
        raise ValueError(f"`columns` is a dict of arrays [{n}] or one array [{n}, n_cols], got shape {a.shape}")
    return [str(i) for i in range(a.shape[1])], np.ascontiguousarray(a.T)


class AnyOf:
    """The OR of conjunctions in a `search_match` condition: AnyOf(d1, d2, ...) with every d a dict as `search_match` takes it.
    AnyOf() is FALSE; a plain dict d is AnyOf(d); {} is TRUE."""

    def __init__(self, *conjunctions):
        if not all(isinstance(d, dict) for d in conjunctions):
            raise TypeError("AnyOf takes dicts: column name -> an int, a (lo, hi) tuple or a list / set / array of values")
        self.conjunctions = tuple(conjunctions)

    def __repr__(self):
        return "AnyOf(" + ", ".join(repr(d) for d in self.conjunctions) + ")"


MAX_CONJUNCTIONS = 4096      # of one condition, after its membership lists have been multiplied out


def _is_int(x) -> bool:
    return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))


def _u32_scalar(x, what: str) -> int:
    if not _is_int(x):
        raise TypeError(f"`{what}` is an integer, got {type(x).__name__}")
    if not 0 <= int(x) <= 0xFFFFFFFF:
        raise ValueError(f"`{what}` = {x} is outside the uint32 range [0, 2**32)")
    return int(x)


def _intervals(spec, name) -> list[tuple[int, int]]:
    """what a column of a conjunction maps to, as intervals: an int (equality), a (lo, hi) tuple, or a list / set / integer array
    (membership: sorted, duplicates dropped, runs of consecutive values merged)"""
    if _is_int(spec):
        v = _u32_scalar(spec, name)
        return [(v, v)]
    if isinstance(spec, tuple):
        if len(spec) != 2:
            raise ValueError(f"column {name!r}: an interval is a tuple (lo, hi); a list or set is a membership test")
        return [(_u32_scalar(spec[0], f"{name} lo"), _u32_scalar(spec[1], f"{name} hi"))]
    if isinstance(spec, (list, set, frozenset, np.ndarray)):
        a = _as_u32(list(spec) if not isinstance(spec, np.ndarray) else spec, name)
        if a.ndim != 1:
            raise ValueError(f"column {name!r}: a membership test is a flat list of values, got shape {a.shape}")
        u = np.unique(a).astype(np.int64)
        if u.size == 0:
            return []
        cut = np.flatnonzero(np.diff(u) > 1)
        first, last = np.concatenate(([0], cut + 1)), np.concatenate((cut, [u.size - 1]))
        return [(int(u[i]), int(u[j])) for i, j in zip(first, last)]
    raise TypeError(f"column {name!r}: an int, a (lo, hi) tuple or a list / set / array of values, got {type(spec).__name__}")


def encode_conds(conds, names, nq: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """The conditions of `search_match` as idist_attr_conds takes them: (clauses uint32 [m, 3] of (col, lo, hi), and_lims, or_lims,
    n_cond).  `conds`: one dict / AnyOf for the batch (n_cond 1) or a list / tuple of nq of them; `names`: the table's column names in
    order.  A dict is one conjunction, column name -> an int (equality), a (lo, hi) tuple, or a list / set / integer array
    (membership, as merged intervals); several memberships in one dict expand to their Cartesian product, at most MAX_CONJUNCTIONS
    conjunctions per condition.  A pure function of its arguments: no index, no device."""
    col_of = {name: i for i, name in enumerate(names)}
    if isinstance(conds, (dict, AnyOf)):
        per_query, n_cond = [conds], 1
    elif isinstance(conds, (list, tuple)):
        if len(conds) != nq:
            raise ValueError(f"`conds` is one dict / AnyOf for the batch or a list of nq = {nq} of them, got {len(conds)}")
        per_query, n_cond = list(conds), nq
    else:
        raise TypeError(f"`conds` is a dict, an AnyOf or a list of them, got {type(conds).__name__}")
    clauses, and_lims, or_lims = [], [0], [0]
    done = {}                                              # the same object again (a list that repeats a few conditions): encoded once
    for cond in per_query:
        if id(cond) not in done:
            if not isinstance(cond, (dict, AnyOf)):
                raise TypeError(f"a condition is a dict or an AnyOf, got {type(cond).__name__}")
            conjs = []
            for d in (cond,) if isinstance(cond, dict) else cond.conjunctions:
                cols, lists, count = [], [], 1
                for name, spec in d.items():
                    if name not in col_of:
                        raise KeyError(name)
                    cols.append(col_of[name])
                    lists.append(_intervals(spec, name))
                    count *= len(lists[-1])
                if len(conjs) + count > MAX_CONJUNCTIONS:
                    raise ValueError(f"a condition expands to more than {MAX_CONJUNCTIONS} conjunctions")
                conjs += [[(c, lo, hi) for c, (lo, hi) in zip(cols, pick)] for pick in itertools.product(*lists)]
            done[id(cond)] = conjs
        for conj in done[id(cond)]:
            clauses += conj
            and_lims.append(len(clauses))
        or_lims.append(len(and_lims) - 1)
    if max(len(clauses), len(and_lims)) > 0xFFFFFFFF:
        raise ValueError("the conditions of one call hold at most 2**32 - 1 clauses")
    return (np.array(clauses, dtype=np.uint32).reshape(-1, 3), np.array(and_lims, dtype=np.uint32), np.array(or_lims, dtype=np.uint32), n_cond)


def _conds_arg(table: "AttrTable", conds, nq: int):
    """(the idist_attr_conds of a call, the arrays it points into)"""
    if not isinstance(table, AttrTable):
        raise TypeError("`table` is an AttrTable (attribute_table); for an Attr use search_where")
    clauses, and_lims, or_lims, n_cond = encode_conds(conds, table.names, nq)
    keep = (clauses, and_lims, or_lims)
    return _capi.AttrConds(_capi.u32p(clauses), _capi.u32p(and_lims), _capi.u32p(or_lims), n_cond), keep


def _group_column(table: "Attr", by) -> int:
    """The column of `table` a `search_grouped` call collapses by: `by` names a column of an `AttrTable`; by=None takes the only
    column of a one-column `Attr`."""
    if not isinstance(table, Attr):
        raise TypeError("`table` is an AttrTable (attribute_table) or a one-column Attr (attributes)")
    names = table.names if isinstance(table, AttrTable) else None
    if by is None:
        if names is not None and len(names) != 1:
            raise ValueError(f"by=None needs a one-column attribute; name one of the table's columns: {names}")
        return 0
    if names is None or by not in names:
        raise KeyError(f"no column {by!r}: the table has {names if names is not None else 'one unnamed column (by=None)'}")
    return names.index(by)


def normalize(points, device: int = 0, return_norm2: bool = False):
    """x / sqrt(s(x)) per row, s = the canonical squared-L2 distance of the row to the origin (idist_normalize_batch): the rows a
    METRIC_COSINE index holds for `points`, bit for bit — an METRIC_L2SQ index over `normalize(points)` searched with
    `normalize(queries)` returns the same ids and twice the distances.  Rows whose sqrt(s) is not a positive finite number come
    back unchanged.  `return_norm2`: also s per row."""
    pts = _as_points(points)
    out = np.empty_like(pts)
    s = np.empty(pts.shape[0], dtype=np.float32) if return_norm2 else None
    L = _lib()
    L.check(L.idist_normalize_batch(_capi.f32p(pts), pts.shape[0], max(pts.shape[1], 1), _capi.f32p(out),
                                    _capi.f32p(s) if return_norm2 else None, int(device)))
    return (out, s) if return_norm2 else out


def augment_dot(points, bound: float = 0.0, device: int = 0, return_norm2: bool = False):
    """The rows a METRIC_DOT index holds for `points`, bit for bit (idist_dot_augment_batch): [n, dim + 1] rows (x, sqrt(S - s(x))),
    s = the canonical squared-L2 distance of the row to the origin, S = `bound` or, when that is 0, the largest finite s.  Returns
    (rows, S) — or (rows, S, s) with `return_norm2`.  A METRIC_L2SQ index over these rows, searched with the queries given a
    trailing 0, returns the ids of the METRIC_DOT index; its distances d map to 0.5 * (d - (s(q) + S)).  A bound below a row's
    squared norm, negative or not finite raises IdistError."""
    pts = _as_points(points)
    n, dim = pts.shape
    out = np.empty((n, max(dim, 1) + 1), dtype=np.float32)
    s = np.empty(n, dtype=np.float32)
    S = C.c_float(0.0)
    L = _lib()
    L.check(L.idist_dot_augment_batch(_capi.f32p(pts), n, max(dim, 1), float(np.float32(bound)), _capi.f32p(out), _capi.f32p(s),
                                      C.byref(S), int(device)))
    S = np.float32(S.value)
    return (out, S, s) if return_norm2 else (out, S)


def _as_points(points) -> np.ndarray:
    pts = np.ascontiguousarray(points, dtype=np.float32)
    if pts.ndim == 1:
        pts = pts.reshape(0, 1) if pts.size == 0 else pts.reshape(1, -1)
    if pts.ndim != 2:
        raise TypeError("points must be an [n, dim] array of f32")
    return pts


# -- the restricted and range searches: what `Hnsw`, `HnswMap` and `PartitionedHnsw` share --
def _queries(queries, info) -> np.ndarray:
    """The queries of a search call as the ABI takes them, f32 [nq, dim]; `info`: the index's IndexInfo / PartitionedInfo."""
    q = _as_points(queries)
    if q.shape[0] and info.n and q.shape[1] != info.dim:
        raise TypeError(f"query dim {q.shape[1]} != index dim {info.dim}")
    return q


def _radius(radius, nq: int) -> np.ndarray:
    """`radius` of a range call as the ABI takes it: f32 [1] (one for the batch) or [nq]."""
    rad = np.ascontiguousarray(np.asarray(radius, dtype=np.float32).reshape(-1))
    if rad.size != 1 and rad.size != nq:
        raise ValueError(f"`radius` is one float or an array of nq = {nq}, got {rad.size}")
    return rad


def _topk_outputs(nq: int, k: int, rung_shape: tuple, counters: bool) -> tuple:
    """The fields of an `AllowedResult`, in order, as a top-k call hands them to C; `rung_shape`: (nq,), or (nq, n_parts) of a
    partitioned index."""
    return (np.full((nq, k), INVALID, dtype=np.uint32), np.full((nq, k), np.inf, dtype=np.float32), np.zeros(nq, dtype=np.uint32),
            np.full(rung_shape, RUNG_NONE, dtype=np.uint32), np.zeros((nq, 3), dtype=np.uint32) if counters else None)


def _topk_pointers(pid, dist, cnt, rung, ctr) -> tuple:
    return _capi.u32p(pid), _capi.f32p(dist), _capi.u32p(cnt), _capi.u32p(rung), _capi.u32p(ctr) if ctr is not None else None


def _range_outputs(nq: int, rung_shape: tuple, counters: bool) -> tuple:
    """(lims, rung, counters) as a range call hands them to C; `pid` and `distance` follow from `_range_fetch`."""
    return (np.zeros(nq + 1, dtype=np.uint64), np.full(rung_shape, RUNG_NONE, dtype=np.uint32),
            np.zeros((nq, 3), dtype=np.uint32) if counters else None)


def _range_fetch(fetch, handle, lims, rung, ctr) -> RangeResult:
    """The results the range call before it left behind `handle`, sized by `lims`; called for an empty total too."""
    total = int(lims[-1])
    pid = np.zeros(total, dtype=np.uint32)
    dist = np.zeros(total, dtype=np.float32)
    _lib().check(fetch(handle, _capi.u32p(pid), _capi.f32p(dist)))
    return RangeResult(lims, pid, dist, rung, ctr)


def _rows(r, item) -> list[list]:
    """`item(distance, id)` of every result of an `AllowedResult` / `BatchResult`: one row per query, nearest first."""
    return [[item(float(r.distance[i, j]), int(r.pid[i, j])) for j in range(int(r.count[i]))] for i in range(r.pid.shape[0])]


def _range_rows(r: RangeResult, item) -> list[list]:
    """`item(distance, id)` of every result of a `RangeResult`: one row per query, nearest first."""
    return [[item(float(r.distance[j]), int(r.pid[j])) for j in range(int(r.lims[i]), int(r.lims[i + 1]))] for i in range(len(r.lims) - 1)]


# A restriction is what narrows a search to some of the points.  A form knows its validation and the ctypes arguments it becomes
# (`args(n, nq)`, which also keeps what they point into alive for as long as the form lives), its `attr` (whose handle follows the
# leading handles of the call, or None) and whether there is `nothing` to do (read after `args`).
class _Everything:
    """no restriction: `search_range`"""
    attr = None
    nothing = False

    def args(self, n: int, nq: int) -> tuple:
        return ()


class _Sets:
    """one allowed set per query: (bits, n_sets, set_of)"""
    attr = None

    def __init__(self, sets, set_of):
        self.sets, self.set_of = sets, set_of

    def args(self, n: int, nq: int) -> tuple:
        bits = allowed_bitmaps(self.sets, n)
        so = _set_of(self.set_of, bits.shape[0], nq)
        self._keep = (bits, so)
        self.nothing = bits.shape[0] == 0 and nq == 0    # only then: sets with no queries still reach C, as every other form does
        return _capi.u32p(bits), bits.shape[0], _capi.u32p(so) if so is not None else None


class _Where:
    """an interval of an `Attr` per query: (lo, hi, n_cond)"""
    nothing = False

    def __init__(self, attr, lo, hi):
        self.attr, self.lo, self.hi = attr, lo, hi

    def args(self, n: int, nq: int) -> tuple:
        lo, hi, n_cond = _conditions(self.lo, self.hi, nq)
        self._keep = (lo, hi)
        return _capi.u32p(lo), _capi.u32p(hi), n_cond


class _Match:
    """a condition over the columns of an `AttrTable` per query: (idist_attr_conds *,)"""
    nothing = False

    def __init__(self, table, conds):
        self.attr, self.conds = table, conds

    def args(self, n: int, nq: int) -> tuple:
        self._keep = _conds_arg(self.attr, self.conds, nq)    # (the struct, the arrays it points into): encoded once
        return (C.byref(self._keep[0]),)


class _RestrictedSearch:
    """The two drivers behind the restricted and range searches of `Hnsw` and `PartitionedHnsw`.  The index class supplies what
    differs: `_SEARCH`, the C symbol per (range?, restriction form); `_FETCH`, the symbol that fetches a range call's results;
    `_lead(search)`, the handles that lead every call — the last one is the handle the fetch reads from; `_rung_shape(nq, info)`.
    Every symbol takes: leading handles, [attr,] queries, nq, [radius, n_radius,] restriction, (k, max_rungs | max_rungs, max_total),
    outputs.  Arguments are judged in the order queries, radius, restriction."""

    def _topk(self, queries, restriction, k: int, max_rungs: int, counters: bool, search=None) -> AllowedResult:
        info = self.info()
        q = _queries(queries, info)
        nq, k = q.shape[0], max(int(k), 0)                  # a negative k is clamped: for the shapes, and for C
        rargs = restriction.args(int(info.n), nq)
        out = _topk_outputs(nq, k, self._rung_shape(nq, info), counters)
        if not restriction.nothing:                         # (only `_Sets` ever has: the other forms reach C with no queries too,
            L = _lib()                                      #  where the attribute is checked against the index)
            lead = self._lead(search)
            attr = () if restriction.attr is None else (restriction.attr._h,)
            L.check(getattr(L, self._SEARCH[False, type(restriction)])(*lead, *attr, _capi.f32p(q), nq, *rargs, k, int(max_rungs),
                                                                       *_topk_pointers(*out)))
        return AllowedResult(*out)

    def _range(self, queries, radius, restriction, max_rungs: int, max_total: int, counters: bool, search=None) -> RangeResult:
        info = self.info()
        q = _queries(queries, info)
        nq = q.shape[0]
        rad = _radius(radius, nq)
        rargs = restriction.args(int(info.n), nq)
        lims, rung, ctr = _range_outputs(nq, self._rung_shape(nq, info), counters)
        if restriction.nothing:
            return RangeResult(lims, np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float32), rung, ctr)
        L = _lib()
        lead = self._lead(search)
        attr = () if restriction.attr is None else (restriction.attr._h,)
        L.check(getattr(L, self._SEARCH[True, type(restriction)])(*lead, *attr, _capi.f32p(q), nq, _capi.f32p(rad), int(rad.size), *rargs,
                                                                  int(max_rungs), int(max_total), _capi.u64p(lims), _capi.u32p(rung),
                                                                  _capi.u32p(ctr) if counters else None))
        return _range_fetch(getattr(L, self._FETCH), lead[-1], lims, rung, ctr)

    def _grouped(self, queries, table, by, conds, k: int, max_rungs: int, counters: bool, search=None) -> GroupedResult:
        """`_topk` collapsed by a column (`_GROUPED`: leading handles, attr, group_col, queries, nq, conds or NULL, k, max_rungs,
        the outputs of `_topk` with the groups behind the distances).  Arguments are judged in the order queries, by, conds."""
        info = self.info()
        q = _queries(queries, info)
        nq, k = q.shape[0], max(int(k), 0)
        col = _group_column(table, by)
        match = None if conds is None else _Match(table, conds)      # (lives through the call: it owns what its argument points into)
        rargs = (None,) if match is None else match.args(int(info.n), nq)
        pid, dist, cnt, rung, ctr = _topk_outputs(nq, k, self._rung_shape(nq, info), counters)
        group = np.zeros((nq, k), dtype=np.uint32)
        L = _lib()
        L.check(getattr(L, self._GROUPED)(*self._lead(search), table._h, col, _capi.f32p(q), nq, *rargs, k, int(max_rungs), _capi.u32p(pid),
                                          _capi.f32p(dist), _capi.u32p(group), _capi.u32p(cnt), _capi.u32p(rung),
                                          _capi.u32p(ctr) if ctr is not None else None))
        return GroupedResult(pid, dist, cnt, rung, ctr, group)


def _or_fresh(search: "Search | None") -> "Search":
    """search=None of the `where` / `match` calls: a Search of the call's own (the sets and range calls require one)"""
    return search if search is not None else Search()


class Hnsw(_RestrictedSearch):
    """core/lib.rs:194-397.  Owns the points in PointId order and the device index."""

    def __init__(self, handle, points: np.ndarray, ef_search: int):
        self._h = handle
        self.points = points          # [n, dim] in PointId order (Index<PointId>, core/types.rs:269-275)
        self._ef_search = ef_search

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None:
                _lib().idist_index_free(self._h)
                self._h = None
        except Exception:
            pass

    @staticmethod
    def builder() -> Builder:
        return Builder()

    # -- construction --
    @classmethod
    def _new(cls, points, builder: Builder) -> tuple["Hnsw", list[PointId]]:
        """Hnsw::new (core/lib.rs:209-345): shuffle on the host, build on the GPU."""
        pts = _as_points(points)
        n, dim = pts.shape
        L = _lib()
        out_pid = np.zeros(max(n, 1), dtype=np.uint32)
        order = np.zeros(max(n, 1), dtype=np.uint32)
        L.check(L.idist_permutation(C.c_uint64(builder._seed), n, _capi.u32p(out_pid), _capi.u32p(order)))
        ordered = np.ascontiguousarray(pts[order[:n]]) if n else pts.reshape(0, max(dim, 1))
        h = cls.from_ordered_points(ordered, builder)
        return h, [int(x) for x in out_pid[:n]]

    @classmethod
    def from_ordered_points(cls, points_in_pid_order, builder: Builder | None = None) -> "Hnsw":
        """Build from points that already are in PointId order (no shuffle)."""
        builder = builder or Builder()
        pts = _as_points(points_in_pid_order)
        n, dim = pts.shape
        cfg = builder._config()
        h = C.c_void_p()
        L = _lib()
        with _BuildWatch(builder._progress):
            L.check(L.idist_index_build(_capi.f32p(pts), n, max(dim, 1), C.byref(cfg), builder._device, C.byref(h)))
        return cls(h, pts, builder._ef_search)

    @classmethod
    def from_device_points(cls, d_points_ptr: int, n: int, dim: int, builder: Builder | None = None,
                           host_points: np.ndarray | None = None) -> "Hnsw":
        """Build from points already resident in HBM (row-major n x dim f32, PointId order)."""
        builder = builder or Builder()
        if host_points is not None and (tuple(host_points.shape) != (n, dim) or host_points.dtype != np.float32):
            raise ValueError(f"host_points must be the same {n} x {dim} float32 rows that sit on the device, got {host_points.dtype} {host_points.shape}")
        cfg = builder._config()
        h = C.c_void_p()
        L = _lib()
        with _BuildWatch(builder._progress):
            L.check(L.idist_index_build_device(C.c_void_p(d_points_ptr), n, dim, C.byref(cfg), builder._device, C.byref(h)))
        pts = host_points if host_points is not None else np.zeros((n, 0), dtype=np.float32)
        return cls(h, pts, builder._ef_search)

    @classmethod
    def from_parts(cls, points_in_pid_order, zero, layers, builder: Builder | None = None) -> "Hnsw":
        """Adopt the fields of `struct Hnsw` (core/lib.rs:194-199): points, zero, layers."""
        builder = builder or Builder()
        pts = _as_points(points_in_pid_order)
        n, dim = pts.shape
        zero = np.ascontiguousarray(zero, dtype=np.uint32).reshape(n, M2)
        layers = [np.ascontiguousarray(l, dtype=np.uint32).reshape(-1, M) for l in layers]
        ptrs = (C.POINTER(C.c_uint32) * max(len(layers), 1))(*[_capi.u32p(l) for l in layers])
        lens = np.array([l.shape[0] for l in layers] + [0], dtype=np.uint32)
        cfg = builder._config()
        h = C.c_void_p()
        L = _lib()
        L.check(L.idist_index_import(_capi.f32p(pts), n, max(dim, 1), C.byref(cfg), _capi.u32p(zero), ptrs,
                                     _capi.u32p(lens), len(layers), builder._device, C.byref(h)))
        return cls(h, pts, builder._ef_search)

    # -- introspection --
    def info(self) -> _capi.IndexInfo:
        info = _capi.IndexInfo()
        _lib().check(_lib().idist_index_get_info(self._h, C.byref(info)))
        return info

    def into_parts(self):
        """(zero [n,64], layers [[len,32], ...]) copied back from the device."""
        info = self.info()
        zero = np.zeros((info.n, M2), dtype=np.uint32)
        layers = [np.zeros((info.layer_len[l], M), dtype=np.uint32) for l in range(info.n_upper)]
        ptrs = (C.POINTER(C.c_uint32) * max(len(layers), 1))(*[_capi.u32p(l) for l in layers])
        _lib().check(_lib().idist_index_export(self._h, _capi.u32p(zero), ptrs))
        return zero, layers

    def build_stats(self) -> _capi.BuildStats:
        st = _capi.BuildStats()
        _lib().check(_lib().idist_index_build_stats(self._h, C.byref(st)))
        return st

    def set_ef_search(self, ef: int):
        _lib().check(_lib().idist_index_set_ef_search(self._h, int(ef)))
        self._ef_search = int(ef)

    def __len__(self):
        return self.points.shape[0]

    def __getitem__(self, pid: PointId) -> np.ndarray:
        return self.points[pid]

    def iter(self) -> Iterator[tuple[PointId, np.ndarray]]:
        """core/lib.rs:386-391"""
        return ((i, p) for i, p in enumerate(self.points))

    # -- search --
    def search_batch(self, queries, search: Search, counters: bool = False) -> BatchResult:
        """Hnsw::search (core/lib.rs:352-383) for many queries in one launch."""
        q = _as_points(queries)
        dim = self.info().dim     # (the host copy of the points is optional: device-built / replicated indexes)
        if q.shape[0] and len(self) and q.shape[1] != dim:
            raise TypeError(f"query dim {q.shape[1]} != index dim {dim}")
        nq = q.shape[0]
        ef = self._ef_search
        pid = np.full((nq, ef), INVALID, dtype=np.uint32)
        dist = np.full((nq, ef), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        ctr = np.zeros((nq, 3), dtype=np.uint32) if counters else None
        if nq:
            ctx = search._bind(self)
            L = _lib()
            L.check(L.idist_search_batch(self._h, ctx, _capi.f32p(q), nq, _capi.u32p(pid), _capi.f32p(dist),
                                         _capi.u32p(cnt), _capi.u32p(ctr) if counters else None))
        return BatchResult(pid, dist, cnt, ctr)

    # what `_RestrictedSearch` asks of the index class
    _SEARCH = {(False, _Sets): "idist_search_batch_allowed_sets",
               (False, _Where): "idist_search_batch_attr",
               (False, _Match): "idist_search_batch_match",
               (True, _Everything): "idist_search_batch_range",
               (True, _Sets): "idist_search_batch_range_allowed_sets",
               (True, _Where): "idist_search_batch_range_attr",
               (True, _Match): "idist_search_batch_range_match"}
    _FETCH = "idist_search_ctx_range_fetch"

    def _lead(self, search: Search) -> tuple:
        return self._h, search._bind(self)

    def _rung_shape(self, nq: int, info) -> tuple:
        return (nq,)

    def search_allowed(self, queries, allowed, k: int, search: Search, max_rungs: int = -1, counters: bool = False) -> AllowedResult:
        """The k nearest among the points of `allowed` (idist_search_batch_allowed; 1 <= k <= ef_search): `Hnsw::search` at
        ef_search, 4 ef_search, ... 4096, filtered — the first rung that holds k allowed points answers — and an exact scan of the
        allowed rows when the set is too small for the ladder or the ladder ends.  `allowed`: a bool array of length n in PointId
        order or an integer array of PointIds, one set for the whole batch.  `max_rungs`: -1 the whole ladder, m only its first m
        rungs, 0 the exact scan alone (the ground truth for recall).  A query that climbs the whole ladder costs about 1.3 searches
        at ef_search 4096 plus a scan of the allowed rows."""
        info = self.info()
        q = _queries(queries, info)
        bits = allowed_bitmap(allowed, int(info.n))
        nq, k = q.shape[0], max(int(k), 0)                  # a negative k is clamped: for the shapes, and for C
        out = _topk_outputs(nq, k, (nq,), counters)
        L = _lib()
        # one bitmap and no set_of: a symbol of its own; always binds and calls C, with no queries too
        L.check(L.idist_search_batch_allowed(self._h, search._bind(self), _capi.f32p(q), nq, _capi.u32p(bits), k, int(max_rungs),
                                             *_topk_pointers(*out)))
        return AllowedResult(*out)

    def search_range(self, queries, radius, search: Search, max_rungs: int = -1, max_total: int = 64 * 2**20,
                     counters: bool = False) -> RangeResult:
        """Every point within `radius` of each query (idist_search_batch_range): `Hnsw::search` at ef_search, 4 ef_search, ... 4096
        while a rung's list is full and wholly within the radius — the first list that is not answers with its within-prefix — and an
        exact scan of every row where the ladder ends.  `radius`: a float for the batch or an array of one per query, compared with the
        distances the metric reports (`<=`); NaN is refused.  `max_rungs`: -1 the whole ladder, m only its first m rungs, 0 the exact
        scan alone (the ground truth for recall).  `max_total` bounds the number of results of the whole batch: beyond it the call
        raises instead of truncating (the default, 64 Mi results = 512 MB of keys on the device, is a choice, not a measurement)."""
        return self._range(queries, radius, _Everything(), max_rungs, max_total, counters, search)

    def search_range_allowed(self, queries, radius, allowed, search: Search, max_rungs: int = -1, max_total: int = 64 * 2**20,
                             counters: bool = False) -> RangeResult:
        """Every point of `allowed` within `radius` of each query: `search_range_allowed_sets` with one set for the whole batch.
        `allowed`: a bool array of length n or an integer array of PointIds (`allowed_bitmap`'s rules), or a ready uint32 bitmap of
        shape (1, (n + 31) // 32)."""
        a = allowed
        if not (isinstance(a, np.ndarray) and a.ndim == 2 and a.dtype == np.uint32):    # (a ready bitmap: this class only)
            a = allowed_bitmap(a, int(self.info().n))[None, :]
        nq = _as_points(queries).shape[0]
        return self.search_range_allowed_sets(queries, radius, a, np.zeros(nq, dtype=np.uint32), search, max_rungs, max_total, counters)

    def search_range_allowed_sets(self, queries, radius, sets, set_of, search: Search, max_rungs: int = -1, max_total: int = 64 * 2**20,
                                  counters: bool = False) -> RangeResult:
        """`search_range` restricted to one allowed set per query (idist_search_batch_range_allowed_sets): every point of
        sets[set_of[q]] within radius[q].  The rungs are `search_range`'s, each answer filtered by the query's set — saturation is
        judged on the unrestricted list — but a query runs rung r only while ef_search * 4**r < 2 |set| (a longer list costs more than
        the exact step); where its rungs end, an exact scan of the set's rows answers.  `radius`, `max_rungs`, `max_total`: as
        `search_range`, `max_total` bounding the restricted total; `sets`, `set_of`: as `search_allowed_sets`."""
        return self._range(queries, radius, _Sets(sets, set_of), max_rungs, max_total, counters, search)

    def search_allowed_sets(self, queries, sets, set_of, k: int, search: Search, max_rungs: int = -1, counters: bool = False) -> AllowedResult:
        """`search_allowed` with several allowed sets in one call, one per query (idist_search_batch_allowed_sets): row q is exactly
        what `search_allowed(queries[q], sets[set_of[q]], k, ...)` returns.  `sets`: a sequence of bool masks or of PointId arrays
        (`allowed_bitmap`'s rules), a 2-D bool array [n_sets][n] or a ready uint32 bitmap [n_sets][(n + 31) // 32].  `set_of`: the set
        index of every query; None: query q uses set q (one set per query).  Queries start on the rung their own set's size calls
        for; the exact step reads n / 8 bytes of its set's bitmap per query on top of the allowed rows."""
        return self._topk(queries, _Sets(sets, set_of), k, max_rungs, counters, search)

    def attributes(self, values) -> Attr:
        """One uint32 per point (a tenant id, a category, a day number), in PointId order — the order of a bool `allowed` mask —
        copied to the index's device once (idist_attr_new) for `search_where` / `search_range_where`.  Values outside uint32
        raise."""
        v = _attr_values(values, int(self.info().n))
        h = C.c_void_p()
        L = _lib()
        L.check(L.idist_attr_new(self._h, _capi.u32p(v), C.byref(h)))
        return Attr(h, self, v)

    def search_where(self, queries, attr: Attr, lo, hi=None, k: int = 10, search: Search | None = None, max_rungs: int = -1,
                     counters: bool = False) -> AllowedResult:
        """The k nearest among the points whose attribute lies in the query's interval: lo <= attr <= hi, unsigned
        (idist_search_batch_attr).  `lo` / `hi`: one integer for the batch or an array of one per query; hi=None means equality;
        lo > hi is the empty set.  Row q is exactly what `search_allowed_sets` returns for the mask
        `(attr.values >= lo[q]) & (attr.values <= hi[q])` — but the masks are made on the device from the attribute that already
        lives there: nothing of the size of n is computed on the host or uploaded."""
        return self._topk(queries, _Where(attr, lo, hi), k, max_rungs, counters, _or_fresh(search))

    def search_range_where(self, queries, radius, attr: Attr, lo, hi=None, search: Search | None = None, max_rungs: int = -1,
                           max_total: int = 64 * 2**20, counters: bool = False) -> RangeResult:
        """Every point within `radius` whose attribute lies in the query's interval (idist_search_batch_range_attr): row q is
        exactly what `search_range_allowed_sets` returns for the mask of `search_where`; `radius`, `max_rungs`, `max_total` as in
        `search_range`, `lo` / `hi` as in `search_where`."""
        return self._range(queries, radius, _Where(attr, lo, hi), max_rungs, max_total, counters, _or_fresh(search))

    def attribute_table(self, columns) -> AttrTable:
        """Several uint32 columns per point (tenant, category, day ...), in PointId order, copied to the index's device once
        (idist_attr_new_columns) for `search_match` / `search_range_match`.  `columns`: a dict name -> integer array [n], or an
        integer array [n, n_cols] whose columns are named "0", "1", ...; the checks of `attributes()`."""
        names, cols = _table_columns(columns, int(self.info().n))
        h = C.c_void_p()
        L = _lib()
        L.check(L.idist_attr_new_columns(self._h, _capi.u32p(cols), len(names), C.byref(h)))
        return AttrTable(h, self, names, cols)

    def search_match(self, queries, table: AttrTable, conds, k: int = 10, search: Search | None = None, max_rungs: int = -1,
                     counters: bool = False) -> AllowedResult:
        """The k nearest among the points that satisfy the query's condition over the table's columns (idist_search_batch_match).
        `conds`: one condition for the batch or a list of one per query.  A condition is a dict — one conjunction, column name ->
        an int (equality), a (lo, hi) tuple (an interval, unsigned, lo > hi empty) or a list / set / integer array (membership) —
        or `AnyOf(d1, d2, ...)`, the OR of such dicts; {} is TRUE, AnyOf() FALSE.  Row q is exactly what `search_allowed_sets`
        returns for the mask of its condition, but the masks are made on the device from the columns that already live there."""
        return self._topk(queries, _Match(table, conds), k, max_rungs, counters, _or_fresh(search))

    def search_range_match(self, queries, radius, table: AttrTable, conds, search: Search | None = None, max_rungs: int = -1,
                           max_total: int = 64 * 2**20, counters: bool = False) -> RangeResult:
        """Every point within `radius` that satisfies the query's condition (idist_search_batch_range_match): row q is exactly what
        `search_range_allowed_sets` returns for the mask of its condition; `radius`, `max_rungs`, `max_total` as in `search_range`,
        `conds` as in `search_match`."""
        return self._range(queries, radius, _Match(table, conds), max_rungs, max_total, counters, _or_fresh(search))

    _GROUPED = "idist_search_batch_grouped"

    def search_grouped(self, queries, table: Attr, by, k: int = 10, conds=None, search: Search | None = None, max_rungs: int = -1,
                       counters: bool = False) -> GroupedResult:
        """The nearest point of each of the k nearest groups (idist_search_batch_grouped): rows are chunks of documents, the answer
        is the k nearest documents, each represented by its nearest chunk.  `by`: the column of the `AttrTable` that holds a point's
        group — every uint32 is a legal group — or None for a one-column `Attr`.  `conds`: None, or a `search_match` condition
        over the same table ("tenant = 7, one hit per document").  The rungs are `search_match`'s, each list collapsed to the first
        allowed entry of every group; the first rung that holds k groups answers, and where the ladder ends an exact step does —
        `max_rungs=0` is the ground truth.  `.group[q, i]` is the group of result i; when every point is its own group the result
        is `search_match`'s."""
        return self._grouped(queries, table, by, conds, k, max_rungs, counters, _or_fresh(search))

    def search_batch_device(self, search: Search, d_queries: int, nq: int, d_pid: int, d_dist: int, d_count: int,
                            d_counters: int = 0, stream: int = 0):
        """Device-pointer variant: inputs/outputs stay in HBM, enqueued on `stream` without a sync."""
        ctx = search._bind(self)
        L = _lib()
        L.check(L.idist_search_batch_device(self._h, ctx, C.c_void_p(d_queries), nq, C.c_void_p(d_pid), C.c_void_p(d_dist),
                                            C.c_void_p(d_count), C.c_void_p(d_counters) if d_counters else None,
                                            C.c_void_p(stream) if stream else None))

    # -- several GPUs of one node (single process; the multi-process flavour is dist.py) --
    def replicate(self, devices: Sequence[int], rccl: bool = False) -> list["Hnsw"]:
        """One copy of this index per entry of `devices`, device to device over xGMI: peer copies from the root
        (idist_replicate) or, `rccl=True`, one RCCL broadcast per buffer (idist_replicate_rccl; its wall time is left in
        `self.last_replicate_seconds`).  The replicas share this index's host copy of the points (`Item.point` works on
        every replica)."""
        devs = (C.c_int32 * max(len(devices), 1))(*[int(d) for d in devices])
        outs = (C.c_void_p * max(len(devices), 1))()
        if rccl:
            secs = C.c_double(0.0)
            _lib().check(_lib().idist_replicate_rccl(self._h, devs, len(devices), outs, C.byref(secs)))
            self.last_replicate_seconds = secs.value
        else:
            _lib().check(_lib().idist_replicate(self._h, devs, len(devices), outs))
        return [Hnsw(C.c_void_p(outs[i]), self.points, self._ef_search) for i in range(len(devices))]

    @staticmethod
    def search_batch_sharded(replicas: Sequence["Hnsw"], searches: Sequence[Search], queries, counters: bool = False) -> BatchResult:
        """Hnsw::search for a batch block-partitioned over (replica, Search) pairs — one GPU each, one host
        thread each, no collective (idist_search_batch_sharded).  Identical to `search_batch` on one replica."""
        if not replicas or len(replicas) != len(searches):
            raise ValueError("need one Search per replica")
        q = _as_points(queries)
        nq = q.shape[0]
        ef = replicas[0]._ef_search
        pid = np.full((nq, ef), INVALID, dtype=np.uint32)
        dist = np.full((nq, ef), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        ctr = np.zeros((nq, 3), dtype=np.uint32) if counters else None
        k = len(replicas)
        hs = (C.c_void_p * k)(*[r._h for r in replicas])
        cs = (C.c_void_p * k)(*[s._bind(r) for r, s in zip(replicas, searches)])
        L = _lib()
        L.check(L.idist_search_batch_sharded(hs, cs, k, _capi.f32p(q), nq, _capi.u32p(pid), _capi.f32p(dist), _capi.u32p(cnt),
                                             _capi.u32p(ctr) if counters else None))
        return BatchResult(pid, dist, cnt, ctr)

    def search(self, point, search: Search) -> Search:
        """Search the index for the points nearest to `point` (core/lib.rs:352-383).

        Returns `search`, now an iterator over <= ef_search `Item`s, nearest first."""
        r = self.search_batch(np.asarray(point, dtype=np.float32).reshape(1, -1), search)
        c = int(r.count[0])
        search._items = [Item(float(r.distance[0, i]), int(r.pid[0, i]), self.points[int(r.pid[0, i])]) for i in range(c)]
        search._cur = 0
        return search

    def get(self, i: int, search: Search) -> Item | None:
        """core/lib.rs:393-396"""
        return search._items[i] if 0 <= i < len(search._items) else None

    def distances(self, queries, ids) -> np.ndarray:
        """Point::distance over id lists (the gather-L2 kernel on its own)."""
        q = _as_points(queries)
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(q.shape[0], -1)
        out = np.zeros(ids.shape, dtype=np.float32)
        L = _lib()
        L.check(L.idist_distance_batch(self._h, _capi.f32p(q), q.shape[0], _capi.u32p(ids), ids.shape[1], _capi.f32p(out)))
        return out

    def filter_bounds(self, queries, ids) -> np.ndarray:
        """The walk's reject filter over id lists: a lower bound of every distance, from the compact copy of the rows alone
        (0 where there is none) — idist_filter_bound_batch.  METRIC_DOT: the bounds are reported like the distances (a lower bound of
        what `distances` returns); "no bound" is the trivial -(|q|^2 + S) / 2."""
        q = _as_points(queries)
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(q.shape[0], -1)
        out = np.zeros(ids.shape, dtype=np.float32)
        L = _lib()
        L.check(L.idist_filter_bound_batch(self._h, _capi.f32p(q), q.shape[0], _capi.u32p(ids), ids.shape[1], _capi.f32p(out)))
        return out

    def bruteforce(self, queries, k: int):
        """Exact k-NN by exhaustive scan (the check in tests/all.rs:60-67)."""
        q = _as_points(queries)
        pid = np.zeros((q.shape[0], k), dtype=np.uint32)
        dist = np.zeros((q.shape[0], k), dtype=np.float32)
        L = _lib()
        L.check(L.idist_bruteforce(self._h, _capi.f32p(q), q.shape[0], k, _capi.u32p(pid), _capi.f32p(dist)))
        return pid, dist


class HnswMap:
    """core/lib.rs:131-173"""

    def __init__(self, hnsw: Hnsw, values: list):
        self.hnsw = hnsw
        self.values = values

    @classmethod
    def _new(cls, points, values: Sequence[Any], builder: Builder) -> "HnswMap":
        hnsw, ids = Hnsw._new(points, builder)
        # values re-ordered by PointId (core/lib.rs:144-149); too few values is a panic there (:148)
        if len(values) < len(ids):
            raise IndexError("values.len() < points.len() (core/lib.rs:148 panics)")
        new = [None] * len(ids)
        for src, pid in enumerate(ids):
            new[pid] = values[src]
        return cls(hnsw, new)

    def search(self, point, search: Search) -> Search:
        """core/lib.rs:154-162"""
        self.hnsw.search(point, search)
        search._items = [MapItem(it.distance, it.pid, it.point, self.values[it.pid]) for it in search._items]
        return search

    def search_allowed(self, queries, allowed, k: int, search: Search, max_rungs: int = -1) -> list[list[MapItem]]:
        """`Hnsw.search_allowed` with the values: per query its min(k, allowed points) results as `MapItem`s, nearest first."""
        return self._items(self.hnsw.search_allowed(queries, allowed, k, search, max_rungs))

    def _item(self, distance: float, pid: PointId) -> MapItem:
        return MapItem(distance, pid, self.hnsw.points[pid], self.values[pid])

    def _items(self, r: AllowedResult) -> list[list[MapItem]]:
        return _rows(r, self._item)

    def search_range(self, queries, radius, search: Search, max_rungs: int = -1, max_total: int = 64 * 2**20) -> list[list[MapItem]]:
        """`Hnsw.search_range` with the values: per query every result within its radius as `MapItem`s, nearest first."""
        return self._range_items(self.hnsw.search_range(queries, radius, search, max_rungs, max_total))

    def _range_items(self, r: RangeResult) -> list[list[MapItem]]:
        return _range_rows(r, self._item)

    def search_range_allowed(self, queries, radius, allowed, search: Search, max_rungs: int = -1,
                             max_total: int = 64 * 2**20) -> list[list[MapItem]]:
        """`Hnsw.search_range_allowed` with the values: per query every allowed result within its radius as `MapItem`s, nearest first."""
        return self._range_items(self.hnsw.search_range_allowed(queries, radius, allowed, search, max_rungs, max_total))

    def search_range_allowed_sets(self, queries, radius, sets, set_of, search: Search, max_rungs: int = -1,
                                  max_total: int = 64 * 2**20) -> list[list[MapItem]]:
        """`Hnsw.search_range_allowed_sets` with the values: per query every result of its set within its radius as `MapItem`s."""
        return self._range_items(self.hnsw.search_range_allowed_sets(queries, radius, sets, set_of, search, max_rungs, max_total))

    def search_allowed_sets(self, queries, sets, set_of, k: int, search: Search, max_rungs: int = -1) -> list[list[MapItem]]:
        """`Hnsw.search_allowed_sets` with the values: per query its min(k, points of its set) results as `MapItem`s, nearest first."""
        return self._items(self.hnsw.search_allowed_sets(queries, sets, set_of, k, search, max_rungs))

    def attributes(self, values) -> Attr:
        """`Hnsw.attributes`: one uint32 per point in PointId order (the order of `self.values`)."""
        return self.hnsw.attributes(values)

    def search_where(self, queries, attr: Attr, lo, hi=None, k: int = 10, search: Search | None = None,
                     max_rungs: int = -1) -> list[list[MapItem]]:
        """`Hnsw.search_where` with the values: per query its results as `MapItem`s, nearest first."""
        return self._items(self.hnsw.search_where(queries, attr, lo, hi, k, search, max_rungs))

    def search_range_where(self, queries, radius, attr: Attr, lo, hi=None, search: Search | None = None, max_rungs: int = -1,
                           max_total: int = 64 * 2**20) -> list[list[MapItem]]:
        """`Hnsw.search_range_where` with the values: per query every result of its interval within its radius as `MapItem`s."""
        return self._range_items(self.hnsw.search_range_where(queries, radius, attr, lo, hi, search, max_rungs, max_total))

    def attribute_table(self, columns) -> AttrTable:
        """`Hnsw.attribute_table`: the columns in PointId order (the order of `self.values`)."""
        return self.hnsw.attribute_table(columns)

    def search_match(self, queries, table: AttrTable, conds, k: int = 10, search: Search | None = None,
                     max_rungs: int = -1) -> list[list[MapItem]]:
        """`Hnsw.search_match` with the values: per query its results as `MapItem`s, nearest first."""
        return self._items(self.hnsw.search_match(queries, table, conds, k, search, max_rungs))

    def search_range_match(self, queries, radius, table: AttrTable, conds, search: Search | None = None, max_rungs: int = -1,
                           max_total: int = 64 * 2**20) -> list[list[MapItem]]:
        """`Hnsw.search_range_match` with the values: per query every result of its condition within its radius as `MapItem`s."""
        return self._range_items(self.hnsw.search_range_match(queries, radius, table, conds, search, max_rungs, max_total))

    def search_grouped(self, queries, table: Attr, by, k: int = 10, conds=None, search: Search | None = None,
                       max_rungs: int = -1) -> list[list[MapItem]]:
        """`Hnsw.search_grouped` with the values: per query the nearest member of each of its groups as `MapItem`s, nearest first."""
        return self._items(self.hnsw.search_grouped(queries, table, by, k, conds, search, max_rungs))

    def iter(self):
        return self.hnsw.iter()

    def get(self, i: int, search: Search):
        return search._items[i] if 0 <= i < len(search._items) else None
