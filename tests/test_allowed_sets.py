"""Restricted search with several allowed sets per call, one per query (idist_search_batch_allowed_sets, include/idist.h; DESIGN.md
section 4.8).

Row q of the call is DEFINED as row 0 of the single-set call for query q alone with its own set, so everything is compared exactly
(ids, counts, rungs and counters with array_equal, distances as bit patterns) and the expected arrays are rows of the oracle model
of tests/test_allowed.py — row q of `model(mask[set_of[q]], k, max_rungs)` — or, where a test says so, of the single-set entry point,
which that file pins to the oracle.  They never come from the new call.  Every case runs on the CPU emulator and (-m gpu) on the
MI355X."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params
from test_allowed import LDS_R_END, Case, allowed_sets, check, ladder, lds_case, lds_rung0_refused, main_case, small_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 0xFFFFFFFF
NONE, EXACT = 254, 255


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


def S(kind, emu, gpu):
    return gpu if kind == "gpu" else emu


# ---- the definition, row by row ----------------------------------------------------------------------------------------------------
def rows_of(models, set_of):
    """row q of models[set_of[q]], for each of the model's six arrays"""
    return tuple(np.array([models[s][i][q] for q, s in enumerate(set_of)], dtype=models[0][i].dtype) for i in range(6))


def start_rung(c, mask, k, max_rungs=-1):
    """the start rule of the definition: the first step of a query restricted to `mask` (a rung index, EXACT or NONE)"""
    E = ladder(c.ef)
    E = E[:max_rungs] if max_rungs >= 0 else E
    a, n = int(mask.sum()), len(c.pts)
    if a == 0 or n == 0 or c.ef == 0:
        return NONE
    if a <= k:
        return EXACT
    return next((r for r, e in enumerate(E) if e * a >= k * n), EXACT)


class Row:
    """Case.model — the very code — on a one-query view of a case: what the definition says about query i alone (a model call for
    the whole batch per query would cost nq^2)."""
    model = Case.model

    def __init__(self, c, i):
        self.c, self.i = c, i
        self.oracle, self.pts, self.q, self.ef, self.metric = c.oracle, c.pts, c.q[i:i + 1], c.ef, c.metric

    def rung(self, ef):
        r, i = self.c.rung(ef), self.i
        return SimpleNamespace(pid=r.pid[i:i + 1], count=r.count[i:i + 1], dist=r.dist[i:i + 1], counters=r.counters[i:i + 1])


def same(a, b, what=""):
    assert np.array_equal(a.rung, b.rung), f"{what}: rungs"
    assert np.array_equal(a.count, b.count), f"{what}: counts"
    assert np.array_equal(a.pid, b.pid), f"{what}: ids"
    assert np.array_equal(pc.bits(a.distance), pc.bits(b.distance)), f"{what}: distance bits"
    if a.counters is not None and b.counters is not None:
        assert np.array_equal(a.counters, b.counters), f"{what}: counters"


def take(r, sel):
    return SimpleNamespace(pid=r.pid[sel], distance=r.distance[sel], count=r.count[sel], rung=r.rung[sel],
                           counters=None if r.counters is None else r.counters[sel])


# ---- 1. mixed sets: every path in one call -------------------------------------------------------------------------------------------
def test_mixed_sets_every_path(eng, oracle):
    ida, kind = eng
    from instant_distance_amd.api import allowed_bitmap

    c, k = main_case(oracle, kind)
    h, s = c.hnsw(ida), ida.Search()
    n, nq = len(c.pts), len(c.q)
    masks = list(allowed_sets(c, k).values())
    assert len(masks) == 8
    bits = np.stack([allowed_bitmap(m, n) for m in masks])
    assert bits.shape == (8, (n + 31) // 32) and bits.dtype == np.uint32
    rungs, causes = set(), set()
    for max_rungs in (-1, 2, 0):
        models = [c.model(m, k, max_rungs) for m in masks]
        starts = np.array([start_rung(c, m, k, max_rungs) for m in masks])
        for shift in range(8):
            set_of = (np.arange(nq) + shift) % 8
            want = rows_of(models, set_of)
            if max_rungs != 0:                          # queries of ONE call start on different rungs
                assert len({int(r) for r in starts[set_of] if r < NONE}) >= 2
            print("max_rungs", max_rungs, "shift", shift, "rungs", dict(zip(*[x.tolist() for x in np.unique(want[3], return_counts=True)])))
            got = h.search_allowed_sets(c.q, bits, set_of, k, s, max_rungs=max_rungs, counters=True)
            check(got, want, f"max_rungs {max_rungs}, shift {shift}")
            rungs |= set(want[3].tolist())
            causes |= set(want[5].tolist())
    # the calls together reach every path: rung 0, a late rung, the exact step by each of its three causes, nothing to find
    assert 0 in rungs and any(2 <= r < NONE for r in rungs) and NONE in rungs and EXACT in rungs
    assert {"small", "start", "ended"} <= causes


# ---- 2. identities -----------------------------------------------------------------------------------------------------------------
def test_one_set_is_search_allowed(eng, oracle):
    ida, kind = eng
    c, k = main_case(oracle, kind)
    h = c.hnsw(ida)
    mask = allowed_sets(c, k)["x0>q80"]
    for max_rungs in (-1, 2):
        a = h.search_allowed_sets(c.q, [mask], np.zeros(len(c.q), np.int64), k, ida.Search(), max_rungs=max_rungs, counters=True)
        b = h.search_allowed(c.q, mask, k, ida.Search(), max_rungs=max_rungs, counters=True)
        check(b, c.model(mask, k, max_rungs), "the single-set call")
        same(a, b, f"max_rungs {max_rungs}")
        assert len(set(b.rung.tolist())) > 1


def test_one_set_per_query(eng, oracle):
    ida, kind = eng
    c, k = main_case(oracle, kind)
    h = c.hnsw(ida)
    n, nq = len(c.pts), len(c.q)
    rng = np.random.default_rng(21)
    shares = np.array([1.0, 0.3, 0.02, 0.0])[np.arange(nq) % 4]
    masks = rng.random((nq, n)) < shares[:, None]
    want = tuple(np.concatenate(x) for x in zip(*[Row(c, q).model(masks[q], k) for q in range(nq)]))
    assert {0, NONE} <= set(want[3].tolist()) and len(set(want[3].tolist())) >= 4
    check(h.search_allowed_sets(c.q, masks, None, k, ida.Search(), counters=True), want, "2-D bool array")
    # the same sets as a sequence of id arrays
    ids = [np.flatnonzero(m) for m in masks]
    check(h.search_allowed_sets(c.q, ids, None, k, ida.Search()), want, "id arrays")


def test_all_ones_is_search_batch(eng, oracle):
    ida, kind = eng
    c, _ = main_case(oracle, kind)
    h = c.hnsw(ida)
    nq = len(c.q)
    a = h.search_allowed_sets(c.q, np.ones((3, len(c.pts)), bool), np.arange(nq) % 3, c.ef, ida.Search(), counters=True)
    b = h.search_batch(c.q, ida.Search(), counters=True)
    assert np.all(a.rung == 0)
    assert np.array_equal(a.pid, b.pid) and np.array_equal(a.count, b.count) and np.array_equal(a.counters, b.counters)
    assert np.array_equal(pc.bits(a.distance), pc.bits(b.distance))


# ---- 3. the exact step straight from the bitmap ----------------------------------------------------------------------------------------
def scan_masks(n, seed):
    """a 40 % random set (partly filled windows: ids carry over from batch to batch); all ones (every window a full batch); a
    clustered set, bits in the first 5 % of the ids only (most segments empty); a set whose only members sit in the last, partial
    word; an empty set"""
    rng = np.random.default_rng(seed)
    clustered = np.zeros(n, bool)
    clustered[: max(n // 20, 1)] = rng.random(max(n // 20, 1)) < 0.7
    clustered[0] = True
    last = np.zeros(n, bool)
    last[(n - 1) // 32 * 32:] = True
    return [rng.random(n) < 0.4, np.ones(n, bool), clustered, last, np.zeros(n, bool)]


def check_bruteforce(ida, c, masks, set_of, got, k):
    """for each non-empty set: its queries' rows == bruteforce on an index over pts[ids], the ids mapped back"""
    for si, mask in enumerate(masks):
        ids = np.flatnonzero(mask).astype(np.uint32)
        sel = np.flatnonzero(np.asarray(set_of) == si)
        if not len(ids) or not len(sel):
            continue
        only = ida.Hnsw.from_parts(c.pts[ids], np.full((len(ids), 64), INVALID, np.uint32), [], ida.Builder())
        kk = min(k, len(ids))
        bp, bd = only.bruteforce(c.q[sel], kk)
        assert np.all(got.rung[sel] == EXACT) and np.all(got.count[sel] == kk)
        assert np.array_equal(got.pid[sel, :kk], ids[bp]) and np.array_equal(pc.bits(got.distance[sel, :kk]), pc.bits(bd)), f"set {si}"
        assert np.all(got.pid[sel, kk:] == INVALID) and np.all(np.isposinf(got.distance[sel, kk:]))


def test_scan_bits_does_not_depend_on_the_segments(eng, oracle, monkeypatch):
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    c, k = main_case(oracle, kind)
    h = c.hnsw(ida)
    nq = len(c.q)
    masks = scan_masks(len(c.pts), 31)
    models = [c.model(m, k, max_rungs=0) for m in masks]
    set_of = np.arange(nq) % 5
    want = rows_of(models, set_of)
    assert set(want[3].tolist()) == {EXACT, NONE} and set(want[2].tolist()) == {0, k}
    for seg in ("1", "3", "64"):
        monkeypatch.setenv("IDIST_ALLOWED_SEGMENTS", seg)          # (sampled when the context is made)
        got = h.search_allowed_sets(c.q, masks, set_of, k, ida.Search(), max_rungs=0, counters=True)
        check(got, want, f"{seg} segments")
        check(h.search_allowed_sets(c.q[:3], masks, set_of[:3], k, ida.Search(), max_rungs=0), tuple(x[:3] for x in want),
              f"{seg} segments, 3 queries")
    check_bruteforce(ida, c, masks, set_of, got, k)


def test_scan_bits_edges(eng, oracle, monkeypatch):
    """n no multiple of 32 or 64, EVERY padding bit of every set set, straight through the ABI"""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    from instant_distance_amd import _capi
    from instant_distance_amd.api import allowed_bitmap

    n, dim, ef, k, nq = S(kind, 205, 1037), 5, 8, 3, 13
    rng = np.random.default_rng(12)
    c = Case(oracle, rng.random((n, dim), dtype=np.float32), rng.random((nq, dim), dtype=np.float32), ef)
    h = c.hnsw(ida)
    masks = scan_masks(n, 32) + [np.zeros(n, bool)]                   # the sixth set: padding bits only
    assert n % 32 and masks[3].sum() == n % 32
    beyond = np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
    dirty = np.stack([allowed_bitmap(m, n) for m in masks])
    dirty[:, -1] |= beyond
    keep = dirty.copy()
    set_of = (np.arange(nq) % 6).astype(np.uint32)

    def raw(s, q, so, max_rungs):
        L = _capi.lib()
        m = len(q)
        pid, dist = np.zeros((m, k), np.uint32), np.zeros((m, k), np.float32)
        cnt, rung, ctr = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros((m, 3), np.uint32)
        L.check(L.idist_search_batch_allowed_sets(h._h, s._bind(h), _capi.f32p(q), m, _capi.u32p(dirty), 6, _capi.u32p(so), k, max_rungs,
                                                  _capi.u32p(pid), _capi.f32p(dist), _capi.u32p(cnt), _capi.u32p(rung), _capi.u32p(ctr)))
        return ida.AllowedResult(pid, dist, cnt, rung, ctr)

    for max_rungs in (0, -1):
        want = rows_of([c.model(m, k, max_rungs) for m in masks], set_of)
        for seg in ("1", "3", "64"):
            monkeypatch.setenv("IDIST_ALLOWED_SEGMENTS", seg)
            got = raw(ida.Search(), c.q, set_of, max_rungs)
            check(got, want, f"max_rungs {max_rungs}, {seg} segments")
            check(raw(ida.Search(), c.q[:3], set_of[:3], max_rungs), tuple(x[:3] for x in want), f"max_rungs {max_rungs}, {seg} segments, 3 queries")
        pad = np.flatnonzero(set_of >= 4)                              # the empty set and the set of padding bits only
        assert np.all(got.rung[pad] == NONE) and np.all(got.count[pad] == 0) and np.all(got.pid[pad] == INVALID)
        assert np.all(np.isposinf(got.distance[pad]))
        if max_rungs == 0:
            check_bruteforce(ida, c, masks, set_of, got, k)
    assert np.array_equal(dirty, keep)                                # the caller's buffer is not written


# ---- 4. the metrics ------------------------------------------------------------------------------------------------------------------
def test_metric_l2(eng, oracle):
    ida, kind = eng
    c = small_case(oracle, kind, 1)
    k = S(kind, 4, 8)
    h, s = c.hnsw(ida), ida.Search()
    rng = np.random.default_rng(8)
    masks = [rng.random(len(c.pts)) < share for share in (1.0, 0.2, 0.03)]
    set_of = rng.integers(0, 3, len(c.q))
    for max_rungs in (-1, 0):
        want = rows_of([c.model(m, k, max_rungs) for m in masks], set_of)
        check(h.search_allowed_sets(c.q, masks, set_of, k, s, max_rungs=max_rungs, counters=True), want, f"max_rungs {max_rungs}")


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_metric_rows_are_the_single_set_call(eng, oracle, metric):
    """three sets mixed in one call on a cosine / DOT index: row by row the single-set call on the same index for that query's set
    (tests/test_allowed.py pins that call to the definition, distances through the metric's report included)"""
    ida, kind = eng
    n, dim, ef, nq = S(kind, (300, 7, 8, 12), (5000, 24, 16, 300))
    rng = np.random.default_rng(11)
    raw = rng.random((n, dim), dtype=np.float32) - np.float32(0.3)
    q = rng.random((nq, dim), dtype=np.float32) - np.float32(0.3)
    k = S(kind, 4, 8)
    if metric == "cosine":
        rows, qt = ida.normalize(raw), ida.normalize(q)
        builder = ida.Builder().metric(ida.METRIC_COSINE)
    else:
        rows, _ = ida.augment_dot(raw)
        qt = np.ascontiguousarray(np.concatenate([q, np.zeros((len(q), 1), np.float32)], axis=1))
        builder = ida.Builder().metric(ida.METRIC_DOT)
    c = Case(oracle, rows, qt, ef)                                      # the L2SQ graph over the transformed rows IS the metric's
    h_m = ida.Hnsw.from_parts(raw, c.zero, c.layers, builder.ef_search(ef))
    rng = np.random.default_rng(9)
    masks = [rng.random(n) < share for share in (1.0, 0.2, 0.03)]
    set_of = np.arange(nq) % 3
    seen = set()
    for max_rungs in (-1, 0):
        got = h_m.search_allowed_sets(q, masks, set_of, k, ida.Search(), max_rungs=max_rungs, counters=True)
        for si, mask in enumerate(masks):
            one = h_m.search_allowed(q, mask, k, ida.Search(), max_rungs=max_rungs, counters=True)
            sel = np.flatnonzero(set_of == si)
            same(take(got, sel), take(one, sel), f"{metric}, max_rungs {max_rungs}, set {si}")
            seen |= set(one.rung[sel].tolist())
    assert EXACT in seen and len(seen) >= 3


# ---- 5. strict ties --------------------------------------------------------------------------------------------------------------------
def test_tie_overflow_never_escapes(eng, oracle):
    """the dense integer grid and the ONE-entry tie region of tests/test_allowed.py, two sets in one call: the rungs' launches
    overflow the region, the call searches the rung again itself and returns the model's arrays"""
    ida, kind = eng
    rng = np.random.default_rng(3000002)
    n, ef, k = S(kind, 420, 12000), 8, 4
    pts = pc.gen_points(rng, n, 3, "grid")
    q = np.ascontiguousarray(pts[: S(kind, 12, 600)] + np.float32(0.25))
    c = Case(oracle, pts, q, ef, metric=1, ef_construction=S(kind, 8, 64))
    rng = np.random.default_rng(4)
    masks = [rng.random(n) < 0.15, rng.random(n) < 0.6]
    set_of = np.arange(len(q)) % 2
    want = rows_of([c.model(m, k) for m in masks], set_of)
    assert len({r for r in want[3].tolist() if r < NONE}) >= 2                     # the ladder climbs
    h = c.hnsw(ida, ida.Builder().tie_capacity(1))
    check(h.search_allowed_sets(q, masks, set_of, k, ida.Search(), counters=True), want)


# ---- 6. arguments ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(eng):
    ida, kind = eng
    from instant_distance_amd import _capi

    rng = np.random.default_rng(1)
    pts = rng.random((50, 4), dtype=np.float32)
    h, s = ida.Hnsw.from_ordered_points(pts, ida.Builder().ef_search(10)), ida.Search()
    q, sets = pts[:3], np.ones((2, 50), bool)
    so = np.array([0, 1, 0])
    L = _capi.lib()
    bits = np.full((2, 2), 0xFFFFFFFF, np.uint32)
    pid, dist, cnt = np.zeros((3, 5), np.uint32), np.zeros((3, 5), np.float32), np.zeros(3, np.uint32)

    def status(n_sets, set_of, k=5, max_rungs=-1):
        return L.idist_search_batch_allowed_sets(h._h, s._bind(h), _capi.f32p(q), 3, _capi.u32p(bits), n_sets,
                                                 None if set_of is None else _capi.u32p(np.asarray(set_of, np.uint32)), k, max_rungs,
                                                 _capi.u32p(pid), _capi.f32p(dist), _capi.u32p(cnt), None, None)

    assert status(2, [0, 1, 0]) == 0 and np.all(cnt == 5)               # out_rung and out_counters may be NULL
    assert status(0, [0, 0, 0]) == 1                                    # no set
    assert status(2, None) == 1                                         # one set per query needs n_sets == nq
    assert status(2, [0, 1, 2]) == 1 and b"query 2" in L.idist_last_error()
    assert status(2, [0, 1, 0], k=0) == 1 and status(2, [0, 1, 0], k=11) == 1 and status(2, [0, 1, 0], max_rungs=-2) == 1
    # the Python layer
    for k, max_rungs in ((0, -1), (11, -1), (5, -2)):
        with pytest.raises(ida.IdistError) as e:
            h.search_allowed_sets(q, sets, so, k, s, max_rungs=max_rungs)
        assert e.value.status == 1
    with pytest.raises(IndexError):
        h.search_allowed_sets(q, sets, [0, 1, 2], 5, s)                 # a set index out of range
    with pytest.raises(IndexError):
        h.search_allowed_sets(q, [np.array([3, 50])], [0, 0, 0], 5, s)  # an id out of range
    with pytest.raises(ValueError):
        h.search_allowed_sets(q, sets, None, 5, s)                      # 2 sets for 3 queries
    with pytest.raises(ValueError):
        h.search_allowed_sets(q, sets, [0, 1], 5, s)                    # set_of: one entry per query
    with pytest.raises(ValueError):
        h.search_allowed_sets(q, np.ones((2, 49), bool), so, 5, s)
    with pytest.raises(ValueError):
        h.search_allowed_sets(q, np.zeros((2, 3), np.uint32), so, 5, s)  # a ready bitmap of the wrong width
    with pytest.raises(ValueError):
        h.search_allowed_sets(q, np.ones(50, bool), so, 5, s)           # one mask is not a sequence of sets
    with pytest.raises(TypeError):
        h.search_allowed_sets(q, sets, np.array([0.0, 1.0, 0.0]), 5, s)
    with pytest.raises(TypeError):
        h.search_allowed_sets(q[:, :3], sets, so, 5, s)
    assert np.all(h.search_allowed_sets(q, sets, so, 10, s).count == 10)            # k == ef_search is legal
    assert np.all(h.search_allowed_sets(q, bits, so, 5, s).count == 5)              # a ready uint32 bitmap (padding bits set)
    r0 = h.search_allowed_sets(np.zeros((0, 4), np.float32), sets, np.zeros(0, np.int64), 5, s, counters=True)
    assert r0.pid.shape == (0, 5) and r0.distance.shape == (0, 5) and r0.count.shape == (0,) and r0.rung.shape == (0,)
    assert r0.counters.shape == (0, 3)


def test_no_points(eng):
    ida, kind = eng
    h = ida.Hnsw.from_ordered_points(np.zeros((0, 4), np.float32), ida.Builder())
    r = h.search_allowed_sets(np.zeros((3, 4), np.float32), np.zeros((2, 0), bool), [0, 1, 1], 5, ida.Search(), counters=True)
    assert np.all(r.rung == NONE) and np.all(r.count == 0) and np.all(r.pid == INVALID) and np.all(r.counters == 0)


# ---- 7. HnswMap ----------------------------------------------------------------------------------------------------------------------------
def test_hnsw_map(eng):
    ida, kind = eng
    rng = np.random.default_rng(2)
    pts = rng.random((120, 5), dtype=np.float32)
    values = [f"v{i}" for i in range(120)]
    m = ida.Builder().seed(7).ef_search(12).build(pts, values)
    masks = [rng.random(120) < 0.3, rng.random(120) < 0.04]
    set_of = [0, 1, 1, 0]
    q = rng.random((4, 5), dtype=np.float32)
    items = m.search_allowed_sets(q, masks, set_of, 6, ida.Search())
    r = m.hnsw.search_allowed_sets(q, masks, set_of, 6, ida.Search())
    assert len(items) == 4
    for i, row in enumerate(items):
        mask = masks[set_of[i]]
        assert [it.pid for it in row] == r.pid[i, : r.count[i]].tolist() and len(row) == min(6, int(mask.sum()))
        assert all(mask[it.pid] and it.value == m.values[it.pid] and np.array_equal(it.point, m.hnsw[it.pid]) for it in row)
        assert all(values[int(np.flatnonzero((pts == it.point).all(axis=1))[0])] == it.value for it in row)


# ---- 8. a rung that does not fit a wave's LDS ends the ladder (the shape and its arithmetic: tests/test_allowed.py) ----------------------
def test_lds_short_rung_ends_the_ladder(eng, oracle):
    """three sets in one call: queries pending behind rung 1, queries WAITING for rung 2 (the refused one) and queries answered on
    rung 0 — the call returns what max_rungs = 2 defines"""
    ida, kind = eng
    c, k, masks = lds_case(oracle)
    masks = masks + [np.ones(len(c.pts), bool)]
    set_of = np.arange(len(c.q)) % 3
    assert start_rung(c, masks[1], k) == LDS_R_END and start_rung(c, masks[0], k) == 0
    want = rows_of([c.model(m, k, max_rungs=LDS_R_END) for m in masks], set_of)
    print("rungs", want[3].tolist(), "causes", want[5].tolist())
    seen = set(zip(want[3].tolist(), want[5].tolist()))
    assert (EXACT, "ended") in seen and (EXACT, "start") in seen and (0, "") in seen
    check(c.hnsw(ida).search_allowed_sets(c.q, masks, set_of, k, ida.Search(), counters=True), want, "the whole ladder")
    lds_rung0_refused(ida, c, lambda hb: hb.search_allowed_sets(c.q, masks, set_of, k, ida.Search()))


# ---- 9. the C++ mirror -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_host_cpp_allowed_sets(tmp_path):
    """host/instant_distance.hpp's Hnsw::search_allowed_sets, compiled against libidist.so and run (tests/host/allowed_sets.cpp
    checks two sets in one call against the single-set call and a scan of its own)"""
    from instant_distance_amd import _capi

    csrc = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "allowed_sets")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "instant-distance_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "allowed_sets.cpp"), "-o", exe, "-L", csrc, "-lidist", "-Wl,-rpath," + csrc])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "allowed_sets ok" in out.stdout
