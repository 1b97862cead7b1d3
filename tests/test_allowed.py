"""Restricted search (idist_search_batch_allowed, include/idist.h): the k nearest among an allowed subset.

The answer is DEFINED through what is already exact — `Hnsw::search` at ef_search, 4 ef_search, ... 4096, filtered by the allowed
set, and `bruteforce` over the allowed rows where the ladder does not apply or ends — so everything here is compared exactly: ids,
order, counts, rungs and counters with array_equal, distances as bit patterns.  The expected arrays come from a small model in this
file (the oracle at each rung's ef_search, a numpy filter, the oracle's brute force over the allowed rows), never from the code
under test.  Every case runs on the CPU emulator and (-m gpu) on the MI355X."""
import atexit
import os
import subprocess

import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 0xFFFFFFFF
INF_BITS = 0x7F800000
MAX_EF = 4096
NONE, EXACT = 254, 255
HALF = np.float32(0.5)


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


def S(kind, emu, gpu):
    return gpu if kind == "gpu" else emu


# ---- the definition, restated --------------------------------------------------------------------------------------------
def ladder(ef):
    out = [ef]
    while out[-1] < MAX_EF:
        out.append(min(4 * out[-1], MAX_EF))
    return out


class Case:
    """One data set: points, queries, the oracle's graph and — computed once, shared by every test that needs them — the oracle's
    search of ALL queries at every ef_search of the ladder (what a rung returns for a query does not depend on who else is pending)."""

    def __init__(self, oracle, pts, q, ef, metric=0, ef_construction=100):
        self.oracle, self.pts, self.q, self.ef, self.metric = oracle, pts, q, ef, metric
        self.oix = oracle.Index.build(pts, oracle.default_config(metric=metric, ef_search=ef, ef_construction=ef_construction), threads=8)
        self.zero, self.layers = self.oix.zero, self.oix.layers
        self._rungs = {}

    def rung(self, ef):
        if ef not in self._rungs:
            self.oix.set_ef_search(ef)
            self._rungs[ef] = self.oix.search(self.q, threads=8)
            self.oix.set_ef_search(self.ef)
        return self._rungs[ef]

    def hnsw(self, ida, builder=None):
        b = builder or ida.Builder()
        return ida.Hnsw.from_parts(self.pts, self.zero, self.layers, b.metric(self.metric).ef_search(self.ef))

    def model(self, mask, k, max_rungs=-1):
        """(pid, distance bits, count, rung, counters, cause): cause[q] says why a query was answered exactly."""
        n, nq = len(self.pts), len(self.q)
        ids = np.flatnonzero(mask).astype(np.uint32)
        pid = np.full((nq, k), INVALID, np.uint32)
        bits = np.full((nq, k), INF_BITS, np.uint32)
        count, rung, ctr = np.zeros(nq, np.uint32), np.full(nq, NONE, np.uint32), np.zeros((nq, 3), np.uint32)
        cause = np.full(nq, "", dtype=object)
        if n == 0 or self.ef == 0 or len(ids) == 0:
            return pid, bits, count, rung, ctr, cause
        E = ladder(self.ef)
        if max_rungs >= 0:
            E = E[:max_rungs]
        pending, why = np.arange(nq), "small"
        if len(ids) > k:
            r0 = next((r for r, e in enumerate(E) if e * len(ids) >= k * n), None)
            why = "start"
            if r0 is not None:
                why = "ended"
                for r in range(r0, len(E)):
                    if not len(pending):
                        break
                    res, still = self.rung(E[r]), []
                    for qi in pending:
                        lst = res.pid[qi, : res.count[qi]]
                        ctr[qi] += res.counters[qi]
                        sel = np.flatnonzero(mask[lst])[:k]
                        if len(sel) == k:
                            pid[qi], bits[qi], count[qi], rung[qi] = lst[sel], pc.bits(res.dist[qi, sel]), k, r
                        else:
                            still.append(qi)
                    pending = np.array(still, dtype=np.int64)
        if len(pending):
            kk = min(k, len(ids))
            bp, bd = self.oracle.bruteforce(self.pts[ids], self.q[pending], kk, metric=self.metric, threads=8)
            pid[pending, :kk], bits[pending, :kk] = ids[bp], pc.bits(bd)
            count[pending], rung[pending], cause[pending] = kk, EXACT, why
        return pid, bits, count, rung, ctr, cause


def check(got, want, what=""):
    w_pid, w_bits, w_cnt, w_rung, w_ctr, _ = want
    assert np.array_equal(got.rung, w_rung), f"{what}: rungs {np.unique(got.rung, return_counts=True)} != {np.unique(w_rung, return_counts=True)}"
    assert np.array_equal(got.count, w_cnt), f"{what}: counts"
    assert np.array_equal(got.pid, w_pid), f"{what}: ids"
    assert np.array_equal(pc.bits(got.distance), w_bits), f"{what}: distance bits"
    if got.counters is not None:
        assert np.array_equal(got.counters, w_ctr), f"{what}: counters"


_CASES = {}
atexit.register(_CASES.clear)      # (the oracle's handles go before the interpreter takes its library apart)


def main_case(oracle, kind):
    """emu: 600 x 12-d, ef_search 8, k 5, 40 queries; gpu: 8000 x 32-d, ef_search 16, k 10, 600 queries (above the 512-query
    crossover: the first rungs run the wide walk, later ones the narrow walks)"""
    if kind not in _CASES:
        n, dim, ef, nq, seed = S(kind, (600, 12, 8, 40, 1), (8000, 32, 16, 600, 2))
        rng = np.random.default_rng(seed)
        _CASES[kind] = Case(oracle, rng.random((n, dim), dtype=np.float32), rng.random((nq, dim), dtype=np.float32), ef)
    return _CASES[kind], S(kind, 5, 10)


def allowed_sets(c, k):
    n, x0 = len(c.pts), c.pts[:, 0]
    rng = np.random.default_rng(77)
    every = np.zeros(n, bool)
    every[:: n // (k + 1)] = True
    exactly_k = np.zeros(n, bool)
    exactly_k[rng.choice(n, k, replace=False)] = True
    return {"all": np.ones(n, bool), "half": rng.random(n) < 0.5, "5%": rng.random(n) < 0.05,
            "x0>q80": x0 > np.quantile(x0, 0.8), "x0>q95": x0 > np.quantile(x0, 0.95), "every": every, "exactly k": exactly_k,
            "empty": np.zeros(n, bool)}


# ---- 1. the ladder, the start rule, the exact step: every path ---------------------------------------------------------------
def test_allowed_sets(eng, oracle):
    ida, kind = eng
    c, k = main_case(oracle, kind)
    h, s = c.hnsw(ida), ida.Search()
    rungs, causes = set(), set()
    for name, mask in allowed_sets(c, k).items():
        want = c.model(mask, k)
        print(name, "rungs", dict(zip(*[x.tolist() for x in np.unique(want[3], return_counts=True)])))
        check(h.search_allowed(c.q, mask, k, s, counters=True), want, name)
        assert np.array_equal(want[2], np.full(len(c.q), min(k, int(mask.sum()))))           # every query: min(k, |A|) results
        rungs |= set(want[3].tolist())
        causes |= set(want[5].tolist())
        if name == "x0>q80":                                                                 # the ladder ended
            want2 = c.model(mask, k, max_rungs=2)
            check(h.search_allowed(c.q, mask, k, s, max_rungs=2, counters=True), want2, name + ", two rungs")
            causes |= set(want2[5].tolist())
            assert len(set(want2[3].tolist())) > 1
        if name == "5%":                                                                     # no permitted rung expects k hits
            want2 = c.model(mask, k, max_rungs=2)
            check(h.search_allowed(c.q, mask, k, s, max_rungs=2, counters=True), want2, name + ", two rungs")
            assert set(want2[5].tolist()) == {"start"}
            causes |= {"start"}
        if mask.any():                                                                       # no rung: the restricted brute force
            want0 = c.model(mask, k, max_rungs=0)
            assert np.all(want0[3] == EXACT)
            check(h.search_allowed(c.q, mask, k, s, max_rungs=0), want0, name + ", no rung")
    # one run reaches every path: rung 0, a late rung, the exact step by each of its three causes, nothing to find
    assert 0 in rungs and any(2 <= r < NONE for r in rungs) and NONE in rungs
    assert {"small", "start", "ended"} <= causes


def test_all_ones_is_search_batch(eng, oracle):
    ida, kind = eng
    c, _ = main_case(oracle, kind)
    h, s = c.hnsw(ida), ida.Search()
    a = h.search_allowed(c.q, np.ones(len(c.pts), bool), c.ef, s, counters=True)
    b = h.search_batch(c.q, ida.Search(), counters=True)
    assert np.all(a.rung == 0)
    assert np.array_equal(a.pid, b.pid) and np.array_equal(a.count, b.count) and np.array_equal(a.counters, b.counters)
    assert np.array_equal(pc.bits(a.distance), pc.bits(b.distance))


# ---- 2. the exact step ---------------------------------------------------------------------------------------------------------
def test_exact_is_bruteforce_over_the_allowed_rows(eng, oracle):
    ida, kind = eng
    c, k = main_case(oracle, kind)
    h = c.hnsw(ida)
    rng = np.random.default_rng(5)
    for share in (0.3, 0.01):
        mask = rng.random(len(c.pts)) < share
        ids = np.flatnonzero(mask).astype(np.uint32)
        only = ida.Hnsw.from_parts(c.pts[ids], np.full((len(ids), 64), INVALID, np.uint32), [], ida.Builder())
        kk = min(k, len(ids))
        bp, bd = only.bruteforce(c.q, kk)
        got = h.search_allowed(c.q, mask, k, ida.Search(), max_rungs=0)
        assert np.all(got.rung == EXACT) and np.all(got.count == kk)
        assert np.array_equal(got.pid[:, :kk], ids[bp]) and np.array_equal(pc.bits(got.distance[:, :kk]), pc.bits(bd))
        assert np.all(got.pid[:, kk:] == INVALID) and np.all(np.isposinf(got.distance[:, kk:]))


def test_exact_does_not_depend_on_the_segments(eng, oracle, monkeypatch):
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    c, k = main_case(oracle, kind)
    h = c.hnsw(ida)
    mask = np.random.default_rng(6).random(len(c.pts)) < 0.4
    want = c.model(mask, k, max_rungs=0)
    for seg in ("1", "3", "64"):
        monkeypatch.setenv("IDIST_ALLOWED_SEGMENTS", seg)          # (sampled when the context is made)
        check(h.search_allowed(c.q, mask, k, ida.Search(), max_rungs=0, counters=True), want, f"{seg} segments")
        check(h.search_allowed(c.q[:3], mask, k, ida.Search(), max_rungs=0), tuple(x[:3] for x in want), f"{seg} segments, 3 queries")


# ---- 3. the metrics ------------------------------------------------------------------------------------------------------------
def small_case(oracle, kind, metric, seed=11):
    n, dim, ef, nq = S(kind, (300, 7, 8, 12), (5000, 24, 16, 300))
    rng = np.random.default_rng(seed)
    return Case(oracle, rng.random((n, dim), dtype=np.float32), rng.random((nq, dim), dtype=np.float32), ef, metric)


def test_metric_l2(eng, oracle):
    ida, kind = eng
    c = small_case(oracle, kind, 1)
    k = S(kind, 4, 8)
    h, s = c.hnsw(ida), ida.Search()
    rng = np.random.default_rng(8)
    for share in (1.0, 0.2, 0.03):
        mask = rng.random(len(c.pts)) < share
        check(h.search_allowed(c.q, mask, k, s, counters=True), c.model(mask, k), f"share {share}")


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_metric_by_definition(eng, oracle, metric):
    """the call on the metric index == the call on the L2SQ index over the transformed rows with the query transformed the same way;
    distances 0.5f * d / 0.5f * (d - t) in numpy f32, bit for bit"""
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
        rows, Sb = ida.augment_dot(raw)
        qt = np.ascontiguousarray(np.concatenate([q, np.zeros((len(q), 1), np.float32)], axis=1))
        sq = ida.augment_dot(q, return_norm2=True)[2]
        t = (sq + np.float32(Sb)).astype(np.float32)
        builder = ida.Builder().metric(ida.METRIC_DOT)
    c = Case(oracle, rows, qt, ef)                                      # the L2SQ graph over the transformed rows IS the metric's
    h_l2 = c.hnsw(ida)
    h_m = ida.Hnsw.from_parts(raw, c.zero, c.layers, builder.ef_search(ef))
    rng = np.random.default_rng(9)
    seen = set()
    for share, max_rungs in ((1.0, -1), (0.2, -1), (0.03, -1), (0.2, 0)):
        mask = rng.random(len(raw)) < share
        a = h_m.search_allowed(q, mask, k, ida.Search(), max_rungs=max_rungs, counters=True)
        b = h_l2.search_allowed(qt, mask, k, ida.Search(), max_rungs=max_rungs, counters=True)
        check(b, c.model(mask, k, max_rungs), f"l2sq side, share {share}")
        assert np.array_equal(a.pid, b.pid) and np.array_equal(a.count, b.count) and np.array_equal(a.rung, b.rung)
        assert np.array_equal(a.counters, b.counters)
        with np.errstate(all="ignore"):
            d = HALF * b.distance if metric == "cosine" else np.where(np.isposinf(b.distance), b.distance, HALF * (b.distance - t[:, None]))
        assert d.dtype == np.float32 and np.array_equal(pc.bits(a.distance), pc.bits(d))
        seen |= set(a.rung.tolist())
    assert EXACT in seen and len(seen) >= 3


# ---- 4. the bitmap's edges -------------------------------------------------------------------------------------------------------
def test_bitmap_edges(eng, oracle):
    ida, kind = eng
    from instant_distance_amd import _capi
    from instant_distance_amd.api import allowed_bitmap

    n, dim, ef, k = S(kind, 205, 1037), 5, 8, 3                        # n is no multiple of 32
    rng = np.random.default_rng(12)
    c = Case(oracle, rng.random((n, dim), dtype=np.float32), rng.random((9, dim), dtype=np.float32), ef)
    h, s = c.hnsw(ida), ida.Search()
    mask = rng.random(n) < 0.3
    mask[n - 1] = True                                                 # the last point, in the partial word
    want = c.model(mask, k)
    check(h.search_allowed(c.q, mask, k, s, counters=True), want, "bool mask")
    # an id array, with duplicates, in any order
    ids = np.flatnonzero(mask)
    ids = rng.permutation(np.concatenate([ids, ids[:7], ids[-3:]]))
    check(h.search_allowed(c.q, ids, k, s, counters=True), want, "id array")
    # set bits beyond n are ignored: straight through the ABI with every padding bit set, and an "allowed set" of padding bits only
    bits = allowed_bitmap(mask, n)
    assert bits.shape == ((n + 31) // 32,)
    L = _capi.lib()

    def raw(words, q):
        nq = len(q)
        pid, dist = np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.float32)
        cnt, rung, ctr = np.zeros(nq, np.uint32), np.zeros(nq, np.uint32), np.zeros((nq, 3), np.uint32)
        L.check(L.idist_search_batch_allowed(h._h, s._bind(h), _capi.f32p(q), nq, _capi.u32p(words), k, -1, _capi.u32p(pid),
                                             _capi.f32p(dist), _capi.u32p(cnt), _capi.u32p(rung), _capi.u32p(ctr)))
        return ida.AllowedResult(pid, dist, cnt, rung, ctr)

    beyond = np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
    dirty = bits.copy()
    dirty[-1] |= beyond
    check(raw(dirty, c.q), want, "padding bits set")
    only_padding = np.zeros_like(bits)
    only_padding[-1] = beyond
    r = raw(only_padding, c.q)
    assert np.all(r.rung == NONE) and np.all(r.count == 0) and np.all(r.pid == INVALID) and np.all(np.isposinf(r.distance))
    # nq 0 and 1
    r0 = h.search_allowed(np.zeros((0, dim), np.float32), mask, k, s, counters=True)
    assert r0.pid.shape == (0, k) and r0.count.shape == (0,) and r0.rung.shape == (0,) and r0.counters.shape == (0, 3)
    check(h.search_allowed(c.q[4:5], mask, k, s, counters=True), tuple(x[4:5] for x in want), "one query")
    check(h.search_allowed(c.q[4], mask, k, s), tuple(x[4:5] for x in want), "one query, 1-d")
    # out_rung and out_counters are optional
    pid, dist, cnt = np.zeros((9, k), np.uint32), np.zeros((9, k), np.float32), np.zeros(9, np.uint32)
    L.check(L.idist_search_batch_allowed(h._h, s._bind(h), _capi.f32p(c.q), 9, _capi.u32p(bits), k, -1, _capi.u32p(pid), _capi.f32p(dist),
                                         _capi.u32p(cnt), None, None))
    assert np.array_equal(pid, want[0]) and np.array_equal(pc.bits(dist), want[1]) and np.array_equal(cnt, want[2])


def test_no_points(eng):
    ida, kind = eng
    h = ida.Hnsw.from_ordered_points(np.zeros((0, 4), np.float32), ida.Builder())
    r = h.search_allowed(np.zeros((3, 4), np.float32), np.zeros(0, bool), 5, ida.Search(), counters=True)
    assert np.all(r.rung == NONE) and np.all(r.count == 0) and np.all(r.pid == INVALID) and np.all(r.counters == 0)


# ---- 5. strict ties ------------------------------------------------------------------------------------------------------------
def test_tie_overflow_never_escapes(eng, oracle):
    """Dense integer grid (test_parity's recipe) and a ONE-entry tie region: the rungs' launches overflow it, the call searches the
    rung again with the larger region itself and returns the model's arrays — through at least one escalating rung."""
    ida, kind = eng
    rng = np.random.default_rng(3000002)
    n, ef, k = S(kind, 420, 12000), 8, 4
    pts = pc.gen_points(rng, n, 3, "grid")
    q = np.ascontiguousarray(pts[: S(kind, 12, 600)] + np.float32(0.25))
    c = Case(oracle, pts, q, ef, metric=1, ef_construction=S(kind, 8, 64))
    mask = np.random.default_rng(4).random(n) < 0.15
    want = c.model(mask, k)
    assert len({r for r in want[3].tolist() if r < NONE}) >= 2                     # the ladder climbs
    h = c.hnsw(ida, ida.Builder().tie_capacity(1))
    check(h.search_allowed(q, mask, k, ida.Search(), counters=True), want)
    first = ladder(ef)[min(r for r in want[3].tolist() if r < NONE)]               # the first rung's launch does overflow that region
    hd = ida.Hnsw.from_parts(pts, c.zero, c.layers, ida.Builder().metric(1).ef_search(first).tie_capacity(1).tie_policy(ida.TIES_DROP))
    sd = ida.Search()
    hd.search_batch(q, sd)
    assert sd.tie_overflowed()


# ---- 6. arguments ----------------------------------------------------------------------------------------------------------------
def test_argument_errors(eng):
    ida, kind = eng
    rng = np.random.default_rng(1)
    pts = rng.random((50, 4), dtype=np.float32)
    h, s = ida.Hnsw.from_ordered_points(pts, ida.Builder().ef_search(10)), ida.Search()
    q, mask = pts[:3], np.ones(50, bool)
    for k, max_rungs in ((0, -1), (11, -1), (5, -2)):
        with pytest.raises(ida.IdistError) as e:
            h.search_allowed(q, mask, k, s, max_rungs=max_rungs)
        assert e.value.status == 1
    with pytest.raises(ValueError):
        h.search_allowed(q, np.ones(49, bool), 5, s)
    with pytest.raises(IndexError):
        h.search_allowed(q, np.array([3, 50]), 5, s)
    with pytest.raises(TypeError):
        h.search_allowed(q[:, :3], mask, 5, s)
    assert np.all(h.search_allowed(q, mask, 10, s).count == 10)                     # k == ef_search is legal


# ---- 7. HnswMap ----------------------------------------------------------------------------------------------------------------
def test_hnsw_map(eng):
    ida, kind = eng
    rng = np.random.default_rng(2)
    pts = rng.random((120, 5), dtype=np.float32)
    values = [f"v{i}" for i in range(120)]
    m = ida.Builder().seed(7).ef_search(12).build(pts, values)
    mask = rng.random(120) < 0.3
    q = rng.random((4, 5), dtype=np.float32)
    items = m.search_allowed(q, mask, 6, ida.Search())
    r = m.hnsw.search_allowed(q, mask, 6, ida.Search())
    assert len(items) == 4
    for i, row in enumerate(items):
        assert [it.pid for it in row] == r.pid[i, : r.count[i]].tolist() and len(row) == 6
        assert all(mask[it.pid] and it.value == m.values[it.pid] and np.array_equal(it.point, m.hnsw[it.pid]) for it in row)
        assert all(values[int(np.flatnonzero((pts == it.point).all(axis=1))[0])] == it.value for it in row)


# ---- 8. a rung that does not fit a wave's LDS ends the ladder ------------------------------------------------------------------------
# The walk's LDS per wave (smem_bytes, idist_kernels.hpp): 4 stride + 8 wcap + 512 + 1056 (QuadCtl) + 4 (2048 Bloom + 64 dirty words)
# = 4 stride + 8 wcap + 10016 bytes, wcap = ef + 64 + 64 (ties) + 8; refused beyond 65536.  dim 13200 is stride 13200 = 52800 B (no
# on-chip set fits 40 KiB next to it: every rung is the bitmap walk), so on the ladder 16, 64, 256, ...
#   ef  16: 52800 + 8 * 152 + 10016 = 64032   launches
#   ef  64: 52800 + 8 * 200 + 10016 = 64416   launches
#   ef 256: 52800 + 8 * 392 + 10016 = 65952   refused: rung 2 ends the ladder, as max_rungs = 2 would
LDS_DIM, LDS_EF, LDS_R_END = 13200, 16, 2
LDS_MESSAGE = "of LDS per wave (> 64 KiB)"


def lds_points():
    """256 x 13200-d and 8 queries, the same for both engines (the arithmetic above has no small version): eight coordinates carry
    the geometry, the others a hundredth of it, so that a set can be near some queries and far from others"""
    rng = np.random.default_rng(41)
    scale = np.full(LDS_DIM, 0.01, np.float32)
    scale[:8] = 1.0
    return rng.random((256, LDS_DIM), dtype=np.float32) * scale, rng.random((8, LDS_DIM), dtype=np.float32) * scale


def lds_case(oracle):
    """(the case, k, two allowed sets: the fifth of the points farthest from query 0 — starts on rung 0, query 0 for one is still
    pending behind rung 1 — and eight points — its start rule names rung 2, the refused one)"""
    if "lds" not in _CASES:
        _CASES["lds"] = Case(oracle, *lds_points(), LDS_EF)
    c = _CASES["lds"]
    d0 = ((c.pts[:, :8] - c.q[0, :8]) ** 2).sum(axis=1)
    few = np.zeros(len(c.pts), bool)
    few[np.random.default_rng(42).choice(len(c.pts), 8, replace=False)] = True
    return c, 3, [d0 >= np.sort(d0)[-51], few]


def lds_rung0_refused(ida, c, call):
    """ef_search = the refused rung's: `call(h)` fails as search_batch does, with its message"""
    h = ida.Hnsw.from_parts(c.pts, c.zero, c.layers, ida.Builder().ef_search(ladder(LDS_EF)[LDS_R_END]))
    with pytest.raises(ida.IdistError) as e0:
        h.search_batch(c.q, ida.Search())
    with pytest.raises(ida.IdistError) as e1:
        call(h)
    assert LDS_MESSAGE in e0.value.message and "dim/ef_search need" in e0.value.message
    assert (e1.value.status, e1.value.message) == (e0.value.status, e0.value.message)


def test_lds_short_rung_ends_the_ladder(eng, oracle):
    ida, kind = eng
    c, k, masks = lds_case(oracle)
    h = c.hnsw(ida)
    seen = set()
    for i, mask in enumerate(masks):
        want = c.model(mask, k, max_rungs=LDS_R_END)
        print("set", i, "rungs", want[3].tolist(), "causes", want[5].tolist())
        check(h.search_allowed(c.q, mask, k, ida.Search(), counters=True), want, f"set {i}, the whole ladder")
        seen |= set(zip(want[3].tolist(), want[5].tolist()))
    assert (EXACT, "ended") in seen and (EXACT, "start") in seen and any(r < LDS_R_END for r, _ in seen)
    assert next(r for r, e in enumerate(ladder(LDS_EF)) if e * int(masks[1].sum()) >= k * len(c.pts)) == LDS_R_END   # (the small set's first rung)
    lds_rung0_refused(ida, c, lambda hb: hb.search_allowed(c.q, masks[0], k, ida.Search()))


# ---- 9. the C++ mirror -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_host_cpp_allowed(tmp_path):
    """host/instant_distance.hpp's Hnsw::search_allowed, compiled against libidist.so and run (tests/host/allowed.cpp checks it
    against a scan of its own)"""
    from instant_distance_amd import _capi

    csrc = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "allowed")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "instant-distance_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "allowed.cpp"), "-o", exe, "-L", csrc, "-lidist", "-Wl,-rpath," + csrc])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "allowed ok" in out.stdout
