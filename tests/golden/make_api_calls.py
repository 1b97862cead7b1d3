"""The call transcript of the Python layer (tests/golden/api_calls.txt; run: python tests/golden/make_api_calls.py [--root DIR]).

One table of calls to `Hnsw`, `HnswMap` and `PartitionedHnsw`, constructed directly around dummy handles over a recording stand-in
for the loaded library: no engine, no device.  Every C call the layer makes becomes one text line — symbol, scalars, and per array
dtype / shape / contiguity / crc32 of its bytes as C would read them — followed by a digest of what the method returned, or by the
refusal it raised.  What the layer hands to C and what it makes of the answer is thereby pinned byte for byte.

The committed file is recorded from the commit BEFORE a change of the layer (`--root` names a checkout of it) and
tests/test_api_calls.py replays the same table against the tree under test: the golden never comes from the code it judges.  A new
method adds cases at the END of `table()`, recorded from the commit that introduced it.

Not recorded: `check` (the stand-in always succeeds) and the `*_free` calls, which follow the garbage collector, not the call."""
import argparse
import ctypes as C
import dataclasses
import gc
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "api_calls.txt")

N, DIM, EF, PARTS = 70, 3, 8, (40, 30)            # three bitmap words, the last ragged; two parts
H_INDEX, H_MAP, H_PART0, H_PART1, H_PARTITIONED = 0x10, 0x11, 0x20, 0x21, 0x30
N_OF = {H_INDEX: N, H_MAP: N, H_PART0: PARTS[0], H_PART1: PARTS[1]}


def crc(data: bytes) -> str:
    return f"{zlib.crc32(data):08x}"


def describe(a) -> str:
    if a is None:
        return "-"
    return f"{a.dtype}{list(a.shape)}{'C' if a.flags.c_contiguous else 'strided'}:{crc(np.ascontiguousarray(a).tobytes())}"


class Recorder:
    """Stands in for `_capi.Lib`: every attribute is a C symbol that records its call, answers the few calls the layer reads an
    answer from, and returns success."""

    def __init__(self):
        self.lines: list[str] = []
        self.arrays: dict[int, np.ndarray] = {}     # data address -> the array a pointer argument was made from
        self.handles = 0x100

    def install(self, _capi, setattr_):
        """`setattr_(object, name, value)`: monkeypatch.setattr in the test, plain setattr (undone by the caller) in the generator"""
        setattr_(_capi, "_singleton", self)
        for name in ("f32p", "u32p", "u64p"):
            setattr_(_capi, name, self._pointer(getattr(_capi, name)))

    def _pointer(self, make):
        def wrapped(a):
            self.arrays[a.ctypes.data] = a
            return make(a)
        return wrapped

    def _array(self, p):
        return self.arrays[C.cast(p, C.c_void_p).value]

    def _show(self, arg) -> str:
        if arg is None:
            return "-"
        if isinstance(arg, (bool, int, float)):
            return repr(arg)
        if isinstance(arg, C._Pointer):
            return describe(self._array(arg))
        if isinstance(arg, C.c_void_p):
            return f"h{arg.value:#x}"
        if type(arg).__name__ == "CArgObject":      # byref(...)
            obj = arg._obj
            if type(obj).__name__ == "AttrConds":
                return (f"&conds(n_cond={obj.n_cond} clauses={describe(self._array(obj.clauses))} "
                        f"and_lims={describe(self._array(obj.and_lims))} or_lims={describe(self._array(obj.or_lims))})")
            return "&" + type(obj).__name__
        raise TypeError(f"a C argument of type {type(arg).__name__} is not described")

    def _new_handle(self, ref):
        self.handles += 1
        ref._obj.value = self.handles

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*args):
            if name.endswith("_free"):
                return None
            self.lines.append("  " + " ".join([name] + [self._show(a) for a in args]))
            self._answer(name, args)
            return 0
        return call

    def check(self, status):
        assert status == 0

    def _answer(self, name, args):
        if name == "idist_index_get_info":
            info = args[1]._obj
            info.n, info.dim, info.ef_search = N_OF[args[0].value], DIM, EF
        elif name == "idist_partitioned_get_info":
            info = args[1]._obj
            info.n_parts, info.dim, info.ef_search, info.n = len(PARTS), DIM, EF, N
            info.base[0], info.base[1], info.base[2] = 0, PARTS[0], N
        elif name == "idist_search_ctx_new" or "_attr_new" in name:
            self._new_handle(args[-1])
        elif name.endswith("_range_fetch"):
            self._fill(self._array(args[-2]), self._array(args[-1]))
        elif "search_batch" in name:
            u64 = [self._array(a) for a in args if isinstance(a, C._Pointer) and self._array(a).dtype == np.uint64]
            if u64:                                  # a range call: query q owns two results
                u64[0][:] = 2 * np.arange(u64[0].shape[0], dtype=np.uint64)
            else:                                    # top-k: (pid, dist, cnt[, rung], ctr) end the argument list
                last = 4 if name in ("idist_search_batch", "idist_partitioned_search_batch") else 5
                pid, dist, cnt = (self._array(a) for a in args[-last:-last + 3])
                self._fill(pid, dist)
                cnt[:] = min(pid.shape[1], 2)

    @staticmethod
    def _fill(pid, dist):
        idx = np.arange(pid.size, dtype=np.int64).reshape(pid.shape)
        pid[...] = (7 * idx + 3) % N
        dist[...] = idx * 0.25


def digest(r) -> str:
    """what a method returned, as one line"""
    if dataclasses.is_dataclass(r):                  # AllowedResult / RangeResult: arrays or None
        return type(r).__name__ + " " + " ".join(f"{f.name}={describe(getattr(r, f.name))}" for f in dataclasses.fields(r))
    if hasattr(r, "_items"):                         # a Search after `search()`
        return "Search " + digest(r._items)
    if isinstance(r, list) and r and not isinstance(r[0], list):
        return f"{type(r[0]).__name__} x {len(r)} " + crc(repr(_items(r)).encode())
    if isinstance(r, list):
        return f"rows {[len(row) for row in r]} " + crc(repr([_items(row) for row in r]).encode())
    raise TypeError(f"a result of type {type(r).__name__} is not described")


def _items(row):
    return [(type(it).__name__, it.distance, it.pid, it.point.tobytes().hex(), getattr(it, "value", None)) for it in row]


def table(ida):
    """(name, call) pairs; `call(env)` runs one case.  `env`: h / m / p the three indexes, S() a fresh Search, q[nq] the queries."""
    AnyOf = ida.AnyOf
    u32 = np.uint32
    ids = [np.array([0, 5, 69]), np.array([64, 65], dtype=np.int64), np.arange(0, 70, 7)]
    mask2 = np.zeros((2, N), dtype=bool)
    mask2[0, ::3] = True
    mask2[1, 33:] = True
    ready = np.array([[0xFFFFFFFF, 0, 0x3F], [1, 2, 3], [0, 0, 0]], dtype=u32)
    none0 = np.zeros((0, 3), dtype=u32)
    mask1 = np.arange(N) % 2 == 0
    vals = (np.arange(N) * 37 % 11).astype(np.int64)
    cols = {"tenant": np.arange(N) % 4, "day": np.arange(N) * 3 % 50}
    rad3 = np.array([0.5, 1.0, 2.0])
    c1 = {"tenant": 2}
    c2 = AnyOf({"tenant": [0, 1, 3], "day": (5, 20)}, {"day": {7, 8, 9, 30}})
    per_q = [c1, c2, c1]
    t = []

    def case(name, call):
        t.append((name, call))

    # -- Hnsw: top-k over sets
    for nq in (0, 1, 3):
        for k in (-1, 0, 5):
            case(f"hnsw.allowed_sets nq={nq} k={k}", lambda e, nq=nq, k=k: e.h.search_allowed_sets(e.q[nq], ready[:nq], None, k, e.S(), counters=(k == 5)))
    case("hnsw.allowed_sets list set_of", lambda e: e.h.search_allowed_sets(e.q[3], ids, [2, 0, 2], 5, e.S(), 2))
    case("hnsw.allowed_sets bool set_of", lambda e: e.h.search_allowed_sets(e.q[3], mask2, np.array([1, 1, 0], dtype=np.int16), 5, e.S(), max_rungs=0, counters=True))
    case("hnsw.allowed_sets no sets, set_of given, nq=0", lambda e: e.h.search_allowed_sets(e.q[0], none0, np.zeros(0, dtype=u32), 5, e.S()))
    case("hnsw.allowed_sets sets, nq=0", lambda e: e.h.search_allowed_sets(e.q[0], ready, np.zeros(0, dtype=u32), 5, e.S()))
    case("hnsw.allowed nq=3", lambda e: e.h.search_allowed(e.q[3], mask1, 5, e.S(), counters=True))
    case("hnsw.allowed nq=0 k=-1", lambda e: e.h.search_allowed(e.q[0], ids[0], -1, e.S(), 3))
    # -- Hnsw: range
    case("hnsw.range scalar", lambda e: e.h.search_range(e.q[3], 1.5, e.S()))
    case("hnsw.range array", lambda e: e.h.search_range(e.q[3], rad3, e.S(), 2, 1000, True))
    case("hnsw.range nq=0", lambda e: e.h.search_range(e.q[0], 1.0, e.S()))
    case("hnsw.range_allowed mask", lambda e: e.h.search_range_allowed(e.q[3], rad3, mask1, e.S(), counters=True))
    case("hnsw.range_allowed ready", lambda e: e.h.search_range_allowed(e.q[1], 2.0, ready[1:2], e.S(), 1, 99))
    case("hnsw.range_allowed_sets list", lambda e: e.h.search_range_allowed_sets(e.q[3], 1.0, ids, None, e.S()))
    case("hnsw.range_allowed_sets bool set_of", lambda e: e.h.search_range_allowed_sets(e.q[3], rad3, mask2, [0, 1, 0], e.S(), 0, 77, True))
    case("hnsw.range_allowed_sets nothing", lambda e: e.h.search_range_allowed_sets(e.q[0], 1.0, none0, None, e.S(), counters=True))
    case("hnsw.range_allowed_sets sets, nq=0", lambda e: e.h.search_range_allowed_sets(e.q[0], 1.0, ready, np.zeros(0, dtype=u32), e.S()))
    # -- Hnsw: intervals
    case("hnsw.where scalars, search omitted", lambda e: e.h.search_where(e.q[3], e.attr, 2, 5))
    case("hnsw.where arrays, search given", lambda e: e.h.search_where(e.q[3], e.attr, [0, 3, 9], np.array([4, 3, 2**32 - 1], dtype=np.uint64), 5, e.S(), 2, True))
    case("hnsw.where scalar next to array", lambda e: e.h.search_where(e.q[3], e.attr, 1, [4, 5, 6], k=-1))
    case("hnsw.where hi=None nq=1 k=0", lambda e: e.h.search_where(e.q[1], e.attr, 7, k=0))
    case("hnsw.where nq=0", lambda e: e.h.search_where(e.q[0], e.attr, 7))
    case("hnsw.where on a table", lambda e: e.h.search_where(e.q[1], e.table, [3]))
    case("hnsw.range_where", lambda e: e.h.search_range_where(e.q[3], rad3, e.attr, [0, 3, 9], 10, e.S(), 1, 50, True))
    case("hnsw.range_where hi=None, search omitted", lambda e: e.h.search_range_where(e.q[3], 1.0, e.attr, 4))
    case("hnsw.range_where nq=0", lambda e: e.h.search_range_where(e.q[0], 1.0, e.attr, 4, 9))
    # -- Hnsw: conditions
    case("hnsw.match dict", lambda e: e.h.search_match(e.q[3], e.table, c1))
    case("hnsw.match AnyOf, search given", lambda e: e.h.search_match(e.q[3], e.table, c2, 5, e.S(), 2, True))
    case("hnsw.match per query k=-1", lambda e: e.h.search_match(e.q[3], e.table, per_q, k=-1))
    case("hnsw.match {} nq=1", lambda e: e.h.search_match(e.q[1], e.table, {}, k=0))
    case("hnsw.match AnyOf() nq=0", lambda e: e.h.search_match(e.q[0], e.table, AnyOf()))
    case("hnsw.range_match", lambda e: e.h.search_range_match(e.q[3], rad3, e.table, per_q, e.S(), 1, 50, True))
    case("hnsw.range_match {}, search omitted", lambda e: e.h.search_range_match(e.q[3], 1.0, e.table, {}))
    case("hnsw.range_match AnyOf() nq=0", lambda e: e.h.search_range_match(e.q[0], 1.0, e.table, AnyOf()))

    def one_search_two_calls(e):
        s = e.S()
        e.h.search_where(e.q[1], e.attr, 1, 2, 5, s)
        return e.h.search_range_match(e.q[1], 1.0, e.table, c1, s)
    case("hnsw: one Search binds once", one_search_two_calls)
    # -- HnswMap
    case("map.search", lambda e: e.m.search(e.q[1][0], e.S()))
    case("map.allowed", lambda e: e.m.search_allowed(e.q[3], mask1, 5, e.S()))
    case("map.allowed_sets", lambda e: e.m.search_allowed_sets(e.q[3], ids, None, 1, e.S(), 2))
    case("map.range", lambda e: e.m.search_range(e.q[3], rad3, e.S()))
    case("map.range_allowed", lambda e: e.m.search_range_allowed(e.q[3], 1.0, ids[2], e.S(), 1))
    case("map.range_allowed_sets", lambda e: e.m.search_range_allowed_sets(e.q[3], 1.0, mask2, [1, 0, 1], e.S(), 1, 64))
    case("map.where", lambda e: e.m.search_where(e.q[3], e.m_attr, 2, 5, 5))
    case("map.where nq=0", lambda e: e.m.search_where(e.q[0], e.m_attr, 2))
    case("map.range_where", lambda e: e.m.search_range_where(e.q[3], 1.0, e.m_attr, 2, None, e.S()))
    case("map.match", lambda e: e.m.search_match(e.q[3], e.m_table, c2, 5, e.S()))
    case("map.range_match", lambda e: e.m.search_range_match(e.q[1], 1.0, e.m_table, c1))
    # -- PartitionedHnsw
    for nq in (0, 1, 3):
        for k in (-1, 5):
            case(f"part.allowed_sets nq={nq} k={k}", lambda e, nq=nq, k=k: e.p.search_allowed_sets(e.q[nq], ready[:nq], None, k, counters=(nq == 3)))
    case("part.allowed_sets list set_of k=0", lambda e: e.p.search_allowed_sets(e.q[3], ids, (2, 0, 2), 0, 2))
    case("part.allowed_sets bool set_of", lambda e: e.p.search_allowed_sets(e.q[3], mask2, np.array([1, 1, 0]), 5, max_rungs=0))
    case("part.allowed_sets sets, nq=0", lambda e: e.p.search_allowed_sets(e.q[0], ready, [], 5))
    case("part.allowed", lambda e: e.p.search_allowed(e.q[3], ids[2], 5, 1, True))
    case("part.search", lambda e: e.p.search(e.q[1][0]))
    case("part.search_one_allowed", lambda e: e.p.search_one_allowed(e.q[1][0], mask1, 5))
    case("part.range scalar", lambda e: e.p.search_range(e.q[3], 1.5))
    case("part.range array", lambda e: e.p.search_range(e.q[3], rad3, 2, 1000, True))
    case("part.range nq=0", lambda e: e.p.search_range(e.q[0], 1.0))
    case("part.search_one_range", lambda e: e.p.search_one_range(e.q[1][0], 2))
    case("part.range_allowed", lambda e: e.p.search_range_allowed(e.q[3], rad3, mask1, counters=True))
    case("part.range_allowed_sets", lambda e: e.p.search_range_allowed_sets(e.q[3], 1.0, ids, None, 1, 55))
    case("part.range_allowed_sets set_of", lambda e: e.p.search_range_allowed_sets(e.q[3], rad3, ready, [2, 2, 1], counters=True))
    case("part.range_allowed_sets nothing", lambda e: e.p.search_range_allowed_sets(e.q[0], 1.0, none0, None))
    case("part.where scalars", lambda e: e.p.search_where(e.q[3], e.p_attr, 2, 5))
    case("part.where arrays", lambda e: e.p.search_where(e.q[3], e.p_attr, [0, 3, 9], 9, 5, 2, True))
    case("part.where hi=None nq=0 k=-1", lambda e: e.p.search_where(e.q[0], e.p_attr, 7, k=-1))
    case("part.range_where", lambda e: e.p.search_range_where(e.q[3], rad3, e.p_attr, 1, [4, 5, 6], 1, 50, True))
    case("part.range_where nq=0", lambda e: e.p.search_range_where(e.q[0], 1.0, e.p_attr, 4))
    case("part.match dict", lambda e: e.p.search_match(e.q[3], e.p_table, c1))
    case("part.match per query", lambda e: e.p.search_match(e.q[3], e.p_table, per_q, 5, 2, True))
    case("part.match AnyOf() nq=0 k=0", lambda e: e.p.search_match(e.q[0], e.p_table, AnyOf(), 0))
    case("part.range_match", lambda e: e.p.search_range_match(e.q[3], rad3, e.p_table, c2, 1, 50, True))
    case("part.range_match {} nq=1", lambda e: e.p.search_range_match(e.q[1], 1.0, e.p_table, {}))
    # -- refusals
    bad_q = np.zeros((2, DIM + 1), dtype=np.float32)
    case("refuse: query dim, sets", lambda e: e.h.search_allowed_sets(bad_q, ready[:2], None, 5, e.S()))
    case("refuse: query dim, allowed", lambda e: e.h.search_allowed(bad_q, mask1, 5, e.S()))
    case("refuse: query dim, range", lambda e: e.h.search_range(bad_q, 1.0, e.S()))
    case("refuse: query dim, where", lambda e: e.h.search_where(bad_q, e.attr, 1))
    case("refuse: query dim, range_match", lambda e: e.h.search_range_match(bad_q, 1.0, e.table, c1))
    case("refuse: query dim, map", lambda e: e.m.search_range_where(bad_q, 1.0, e.m_attr, 1))
    case("refuse: query dim, part sets", lambda e: e.p.search_allowed_sets(bad_q, ready[:2], None, 5))
    case("refuse: query dim, part range", lambda e: e.p.search_range(bad_q, 1.0))
    case("refuse: query dim, part match", lambda e: e.p.search_match(bad_q, e.p_table, c1))
    case("refuse: radius length", lambda e: e.h.search_range(e.q[3], [1.0, 2.0], e.S()))
    case("refuse: radius length, range_where", lambda e: e.h.search_range_where(e.q[3], [1.0, 2.0], e.attr, 1))
    case("refuse: radius length, part range_sets", lambda e: e.p.search_range_allowed_sets(e.q[3], np.zeros(0), ready, None))
    case("refuse: radius length, part range_match", lambda e: e.p.search_range_match(e.q[3], [1.0, 2.0], e.p_table, c1))
    case("refuse: set_of float", lambda e: e.h.search_allowed_sets(e.q[3], ready, [0.0, 1.0, 2.0], 5, e.S()))
    case("refuse: set_of shape", lambda e: e.h.search_range_allowed_sets(e.q[3], 1.0, ready, [0, 1], e.S()))
    case("refuse: set_of out of range", lambda e: e.p.search_allowed_sets(e.q[3], ready, [0, 1, 3], 5))
    case("refuse: set_of negative", lambda e: e.p.search_range_allowed_sets(e.q[3], 1.0, ready, [0, -1, 2]))
    case("refuse: set_of None, n_sets != nq", lambda e: e.h.search_allowed_sets(e.q[1], ready, None, 5, e.S()))
    case("refuse: set_of None, n_sets != nq, part", lambda e: e.p.search_allowed_sets(e.q[1], ready, None, 5))
    case("refuse: set_of None, n_sets != nq, part range", lambda e: e.p.search_range_allowed_sets(e.q[0], 1.0, ready, None))
    case("refuse: bitmap words", lambda e: e.h.search_allowed_sets(e.q[1], ready[:1, :2], None, 5, e.S()))
    case("refuse: PointId out of range", lambda e: e.p.search_allowed(e.q[1], [70], 5))
    case("refuse: lo length", lambda e: e.h.search_where(e.q[3], e.attr, [1, 2]))
    case("refuse: lo beyond u32", lambda e: e.h.search_range_where(e.q[3], 1.0, e.attr, 2**32))
    case("refuse: hi negative, part", lambda e: e.p.search_where(e.q[3], e.p_attr, 1, -1))
    case("refuse: unknown column", lambda e: e.h.search_match(e.q[3], e.table, {"colour": 1}))
    case("refuse: unknown column, part range", lambda e: e.p.search_range_match(e.q[3], 1.0, e.p_table, {"colour": 1}))
    case("refuse: match on an Attr", lambda e: e.h.search_match(e.q[3], e.attr, c1))
    case("refuse: conds length", lambda e: e.p.search_match(e.q[3], e.p_table, [c1, c2]))
    case("refuse: query dim before radius", lambda e: e.h.search_range_allowed_sets(bad_q, [1.0, 2.0, 3.0], ready, [0, 9], e.S()))
    case("refuse: query dim before radius, part", lambda e: e.p.search_range_where(bad_q, [1.0, 2.0, 3.0], e.p_attr, 2**32))
    case("refuse: radius before sets", lambda e: e.h.search_range_allowed_sets(e.q[3], [1.0, 2.0], ready[:, :2], [0, 9], e.S()))
    case("refuse: radius before sets, part", lambda e: e.p.search_range_allowed_sets(e.q[3], [1.0, 2.0], ready, [0, 9]))
    case("refuse: radius before conds", lambda e: e.h.search_range_match(e.q[3], [1.0, 2.0], e.table, {"colour": 1}))
    case("refuse: sets before set_of", lambda e: e.h.search_allowed_sets(e.q[3], ready[:, :2], [0, 9], 5, e.S()))
    return t, vals, cols


class Env:
    pass


def transcript(ida, setattr_) -> str:
    """Run the table against the package `ida` with the recorder installed through `setattr_`; the text of tests/golden/api_calls.txt."""
    from instant_distance_amd import _capi

    rec = Recorder()
    rec.install(_capi, setattr_)
    e = Env()
    owners = []
    try:
        points = (np.arange(N * DIM, dtype=np.float32).reshape(N, DIM) * 0.25).astype(np.float32)
        cases, vals, cols = table(ida)
        rec.lines.append("# setup")
        e.h = ida.Hnsw(C.c_void_p(H_INDEX), points, EF)
        e.m = ida.HnswMap(ida.Hnsw(C.c_void_p(H_MAP), points, EF), [f"v{i}" for i in range(N)])
        e.p = ida.PartitionedHnsw(C.c_void_p(H_PARTITIONED), [ida.Hnsw(C.c_void_p(H_PART0), points[:PARTS[0]], EF),
                                                               ida.Hnsw(C.c_void_p(H_PART1), points[PARTS[0]:], EF)])
        e.attr, e.table = e.h.attributes(vals), e.h.attribute_table(cols)
        e.m_attr, e.m_table = e.m.attributes(vals), e.m.attribute_table(cols)
        e.p_attr, e.p_table = e.p.attributes(vals), e.p.attribute_table(cols)
        owners += [e.h, e.m.hnsw, e.p, *e.p.parts, e.attr, e.table, e.m_attr, e.m_table, e.p_attr, e.p_table]
        e.S = ida.Search
        e.q = {0: np.zeros((0, DIM), dtype=np.float32), 1: np.array([[0.5, 1.0, 1.5]]),
               3: np.arange(3 * DIM, dtype=np.float64).reshape(3, DIM) / 8}
        for name, call in cases:
            rec.lines.append("# " + name)
            rec.arrays.clear()
            try:
                rec.lines.append("  = " + digest(call(e)))
            except Exception as err:  # noqa: BLE001 - a refusal is part of the transcript
                rec.lines.append(f"  raises {type(err).__name__}: {err}")
    finally:
        # no dummy handle may outlive the recorder: a __del__ after it is gone would hand the handle to a real library
        for o in owners:
            o._h = None
        del e
        gc.collect()
    return "\n".join(rec.lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(HERE)), help="the checkout whose package is recorded")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import instant_distance_amd as ida
    from instant_distance_amd import _capi

    assert os.path.abspath(ida.__file__).startswith(os.path.abspath(args.root)), ida.__file__
    saved = []

    def setattr_(obj, name, value):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    try:
        text = transcript(ida, setattr_)
    finally:
        for obj, name, value in reversed(saved):
            setattr(obj, name, value)
    with open(args.out, "w") as f:
        f.write(text)
    print(args.out, "written:", text.count("\n"), "lines from", os.path.abspath(args.root))


if __name__ == "__main__":
    main()
