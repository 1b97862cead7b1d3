"""Range search (idist_search_batch_range, include/idist.h): every point within a radius.

The answer is DEFINED through what is already exact — `Hnsw::search` at ef_search, 4 ef_search, ... 4096 while a rung's list is full
and wholly within the radius, and an exhaustive scan where that ladder ends — so everything here is compared exactly: lims, ids, order,
rungs and counters with array_equal, distances as bit patterns.  The expected arrays come from a small model in this file (the
oracle's search at each rung's ef_search, the oracle's brute force over all rows, the metrics' reports in numpy), never from the code
under test.  Every case runs on the CPU emulator and (-m gpu) on the MI355X."""
import atexit

import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params
from test_allowed import LDS_EF, LDS_R_END, Case, ladder, lds_points, lds_rung0_refused
from test_cosine import halved, np_normalize
from test_dot import np_augment, np_norms, np_queries, reported

NONE, EXACT = 254, 255
NAN_BITS = 0x7FC00000


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


def S(kind, emu, gpu):
    return gpu if kind == "gpu" else emu


# ---- the definition, restated --------------------------------------------------------------------------------------------
class RCase:
    """One data set under one metric.  Cosine and DOT are reductions onto squared L2 over transformed rows (numpy, the oracle's norms):
    the oracle's graph and searches over those rows give the RAW distances, `report` what the metric reports for them."""

    def __init__(self, oracle, raw, q, ef, metric="l2sq"):
        self.raw, self.q, self.ef, self.mname = np.ascontiguousarray(raw), np.ascontiguousarray(q), ef, metric
        km = 0
        if metric == "cosine":
            rows, qt = np_normalize(oracle, raw)[0], np_normalize(oracle, q)[0]
        elif metric == "dot":
            rows, self.Sb, _ = np_augment(oracle, raw)
            qt, self.sq = np_queries(q), np_norms(oracle, q)
        else:
            rows, qt, km = self.raw, self.q, (1 if metric == "l2" else 0)
        self.c = Case(oracle, rows, qt, ef, metric=km)
        n = len(rows)
        bp, bd = oracle.bruteforce(rows, qt, n, metric=km, threads=8)
        b = np.where(np.isnan(bd), np.uint32(NAN_BITS), pc.bits(bd))             # OrderedFloat: every NaN is the same, and the greatest
        order = np.stack([np.lexsort((bp[i], b[i])) for i in range(len(qt))]) if len(qt) else np.zeros((0, n), np.int64)
        self.all_pid = np.take_along_axis(bp, order, axis=1)                     # every row, by (raw distance bits, id)
        self.all_d = np.take_along_axis(np.ascontiguousarray(bd, dtype=np.float32), order, axis=1)
        self.all_rep = np.stack([self.report(self.all_d[i], i) for i in range(len(qt))]) if len(qt) else self.all_d

    def report(self, d, qi):
        d = np.ascontiguousarray(d, dtype=np.float32)
        if self.mname == "cosine":
            return halved(d).view(np.float32)
        if self.mname == "dot":
            return reported(d[None, :], self.sq[qi:qi + 1], self.Sb)[0].view(np.float32)
        return d

    def hnsw(self, ida, builder=None):
        code = {"l2sq": ida.METRIC_L2SQ, "l2": ida.METRIC_L2, "cosine": ida.METRIC_COSINE, "dot": ida.METRIC_DOT}[self.mname]
        b = builder or ida.Builder()
        return ida.Hnsw.from_parts(self.raw, self.c.zero, self.c.layers, b.metric(code).ef_search(self.ef))

    def model(self, radii, max_rungs=-1, queries=None):
        """(lims, pid, reported distance bits, rung, counters) by the definition"""
        qs = range(len(self.q)) if queries is None else queries
        rad = np.broadcast_to(np.asarray(radii, dtype=np.float32), (len(qs),))
        E = ladder(self.ef)
        if max_rungs >= 0:
            E = E[:max_rungs]
        pids, reps, rung, ctr = [], [], np.full(len(qs), NONE, np.uint32), np.zeros((len(qs), 3), np.uint32)
        for i, qi in enumerate(qs):
            r = rad[i]
            for ri, e in enumerate(E):
                res = self.c.rung(e)
                cnt = int(res.count[qi])
                ctr[i] += res.counters[qi]
                rep = self.report(res.dist[qi, :cnt], qi)
                with np.errstate(invalid="ignore"):
                    w = rep <= r
                if cnt == e and w.all():
                    continue                                                     # saturated: the next rung
                pre = cnt if w.all() else int(np.argmin(w))
                pids.append(res.pid[qi, :pre])
                reps.append(rep[:pre])
                rung[i] = ri
                break
            else:
                with np.errstate(invalid="ignore"):
                    w = self.all_rep[qi] <= r
                pids.append(self.all_pid[qi][w])
                reps.append(self.all_rep[qi][w])
                rung[i] = EXACT
        lims = np.concatenate([[0], np.cumsum([len(p) for p in pids])]).astype(np.uint64)
        pid = np.concatenate(pids).astype(np.uint32) if pids else np.zeros(0, np.uint32)
        rep = np.concatenate(reps).astype(np.float32) if reps else np.zeros(0, np.float32)
        return lims, pid, pc.bits(rep), rung, ctr


def check(got, want, what=""):
    w_lims, w_pid, w_bits, w_rung, w_ctr = want
    assert np.array_equal(got.rung, w_rung), f"{what}: rungs {np.unique(got.rung, return_counts=True)} != {np.unique(w_rung, return_counts=True)}"
    assert got.lims.dtype == np.uint64 and np.array_equal(got.lims, w_lims), f"{what}: lims"
    assert np.array_equal(got.pid, w_pid), f"{what}: ids"
    assert np.array_equal(pc.bits(got.distance), w_bits), f"{what}: distance bits"
    if got.counters is not None:
        assert np.array_equal(got.counters, w_ctr), f"{what}: counters"


_CASES = {}
atexit.register(_CASES.clear)      # (the oracle's handles go before the interpreter takes its library apart)

KINDS = ["below", 0, "ef-1", "ef", "ef+1", "4ef", "n/2", "inf", "neg", "zero", "negzero", "big"]


def main_case(oracle, kind):
    """emu: 600 x 12-d, ef_search 8, 40 queries (ladder 8, 32, 128, 512, 2048, 4096); gpu: 8000 x 32-d, ef_search 16, 600 queries
    (above the 512-query crossover; ladder 16, 64, 256, 1024, 4096).  The queries whose radius will be 0 / -0.0 are stored rows."""
    if kind not in _CASES:
        n, dim, ef, nq, seed = S(kind, (600, 12, 8, 40, 1), (8000, 32, 16, 600, 2))
        rng = np.random.default_rng(seed)
        pts, q = rng.random((n, dim), dtype=np.float32), rng.random((nq, dim), dtype=np.float32)
        for j in (KINDS.index("zero"), KINDS.index("negzero")):
            q[j::len(KINDS)] = pts[rng.choice(n, len(q[j::len(KINDS)]), replace=False)]
        _CASES[kind] = RCase(oracle, pts, q, ef)
    return _CASES[kind]


def radii_of(rc, kinds=KINDS):
    """one radius per query, taken from the exhaustive reported distances of that query"""
    n, ef, D = len(rc.raw), rc.ef, rc.all_rep
    at = {"ef-1": ef - 1, "ef": ef, "ef+1": ef + 1, "4ef": 4 * ef, "n/2": n // 2, "big": (5 * n) // 8}    # big: 5000 of 8000, no power of two
    out = np.zeros(len(rc.q), np.float32)
    for qi in range(len(rc.q)):
        k = kinds[qi % len(kinds)]
        if k == "below":
            out[qi] = np.nextafter(D[qi, 0], np.float32(-np.inf))
        elif k == "inf":
            out[qi] = np.inf
        elif k == "neg":
            out[qi] = -1.0 if rc.mname != "dot" else np.nextafter(D[qi, 0], np.float32(-np.inf)) - np.float32(1.0)
        elif k == "zero":
            out[qi] = 0.0
        elif k == "negzero":
            out[qi] = -0.0
        else:
            out[qi] = D[qi, at.get(k, k)]                             # exactly a reported value: `<=` is inclusive
    return out


def counts(want):
    return np.diff(want[0].astype(np.int64))


# ---- 1. per-query radii: every path ------------------------------------------------------------------------------------------
def test_per_query_radii(eng, oracle):
    ida, kind = eng
    rc = main_case(oracle, kind)
    h, s = rc.hnsw(ida), ida.Search()
    rad = radii_of(rc)
    want = rc.model(rad)
    print("rungs", dict(zip(*[x.tolist() for x in np.unique(want[3], return_counts=True)])))
    check(h.search_range(rc.q, rad, s, counters=True), want, "whole ladder")
    c, nk = counts(want), len(KINDS)
    assert np.all(c[KINDS.index("below")::nk] == 0) and np.all(want[3][KINDS.index("below")::nk] == 0)       # count 0 is an answer, on rung 0
    assert np.all(c[KINDS.index("neg")::nk] == 0)
    cx = counts(rc.model(rad, max_rungs=0))                            # (exhaustively: a rung's list may miss the nearest point)
    assert np.all(cx[KINDS.index(0)::nk] >= 1)                         # `<=` is inclusive
    assert np.all(cx[KINDS.index("zero")::nk] >= 1) and np.all(cx[KINDS.index("negzero")::nk] >= 1)         # 0 <= -0.0
    seen = set(want[3].tolist())
    if kind == "emu":                                                  # 600 points never saturate a rung of 2048: exact by max_rungs
        want2 = rc.model(rad, max_rungs=2)
        check(h.search_range(rc.q, rad, s, max_rungs=2, counters=True), want2, "two rungs")
        seen |= set(want2[3].tolist())
    assert 0 in seen and len({r for r in seen if 0 < r < NONE}) >= 2 and EXACT in seen


# ---- 2. one shared radius ------------------------------------------------------------------------------------------------------
def test_shared_radius(eng, oracle):
    ida, kind = eng
    rc = main_case(oracle, kind)
    r = np.float32(np.median(rc.all_rep))                              # the median pairwise distance
    want = rc.model(r)
    got = rc.hnsw(ida).search_range(rc.q, float(r), ida.Search(), counters=True)
    check(got, want, "shared radius")
    check(rc.hnsw(ida).search_range(rc.q, np.array([r]), ida.Search()), want, "shared radius, array of one")
    assert counts(want).min() > rc.ef


# ---- 3. max_rungs ----------------------------------------------------------------------------------------------------------------
def test_max_rungs(eng, oracle):
    ida, kind = eng
    rc = main_case(oracle, kind)
    h, s = rc.hnsw(ida), ida.Search()
    rad = radii_of(rc)
    for m in (0, 1, 2, -1):
        want = rc.model(rad, max_rungs=m)
        got = h.search_range(rc.q, rad, s, max_rungs=m, counters=True)
        check(got, want, f"max_rungs {m}")
        assert set(want[3].tolist()) <= set(range(m if m >= 0 else 8)) | {EXACT}
        if m == 0:                                                     # the exhaustive answer, for every query
            assert np.all(got.rung == EXACT) and np.all(got.counters == 0)
            for qi in range(len(rc.q)):
                with np.errstate(invalid="ignore"):
                    ids = rc.all_pid[qi][rc.all_rep[qi] <= rad[qi]]
                assert np.array_equal(got.pid[int(got.lims[qi]):int(got.lims[qi + 1])], ids)


# ---- 4. the metrics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2sq", "l2", "cosine", "dot"])
def test_metrics(eng, oracle, metric):
    """radii exactly on reported values; DOT with one large-norm row, so the bound S is large and the report rounds"""
    ida, kind = eng
    n, dim, ef, nq = S(kind, (300, 7, 8, 24), (3000, 24, 16, 120))
    rng = np.random.default_rng(11)
    raw = rng.random((n, dim), dtype=np.float32) - np.float32(0.3)
    q = rng.random((nq, dim), dtype=np.float32) - np.float32(0.3)
    if metric == "dot":
        raw[n // 3] *= np.float32(37.0)
    rc = RCase(oracle, raw, q, ef, metric)
    kinds = ["below", 0, "ef-1", "ef", "ef+1", "4ef", "n/2", "inf", "neg"]
    rad = radii_of(rc, kinds)
    if metric == "dot":
        assert (rad[np.isfinite(rad)] < 0).any()                       # negative radii are meaningful here
        exact = 0.5 * (rc.all_d.astype(np.float64) - (rc.sq.astype(np.float64)[:, None] + float(rc.Sb)))
        assert (rc.all_rep.astype(np.float64) != exact).any()          # the report does round: the f32 steps matter
    h, s = rc.hnsw(ida), ida.Search()
    seen = set()
    for m in (-1, 2, 0):
        want = rc.model(rad, max_rungs=m)
        check(h.search_range(q, rad, s, max_rungs=m, counters=True), want, f"{metric}, max_rungs {m}")
        seen |= set(want[3].tolist())
    assert EXACT in seen and len(seen) >= 3
    c = counts(rc.model(rad, max_rungs=0))
    assert np.all(c[1::len(kinds)] >= 1) and np.all(c[0::len(kinds)] == 0)


# ---- 5. the exact step does not depend on the segments ---------------------------------------------------------------------------
def test_exact_does_not_depend_on_the_segments(eng, oracle, monkeypatch):
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    rc = main_case(oracle, kind)
    h = rc.hnsw(ida)
    rad = radii_of(rc)
    want = rc.model(rad, max_rungs=0)
    for seg in ("1", "3", "64"):
        monkeypatch.setenv("IDIST_RANGE_SEGMENTS", seg)               # (sampled when the context is made)
        check(h.search_range(rc.q, rad, ida.Search(), max_rungs=0, counters=True), want, f"{seg} segments")
    monkeypatch.setenv("IDIST_RANGE_SEGMENTS", "3")
    check(h.search_range(rc.q[:3], rad[:3], ida.Search(), max_rungs=0), rc.model(rad[:3], 0, queries=range(3)), "3 segments, 3 queries")


# ---- 6. list lengths through the sort ---------------------------------------------------------------------------------------------
def lengths_radii(rc, lens):
    rad = np.zeros(len(rc.q), np.float32)
    for qi in range(len(rc.q)):
        L = lens[qi % len(lens)]
        rad[qi] = np.nextafter(rc.all_rep[qi, 0], np.float32(-np.inf)) if L == 0 else rc.all_rep[qi, L - 1]
    return rad


def test_list_lengths(eng, oracle):
    ida, kind = eng
    rc = main_case(oracle, kind)
    n = len(rc.raw)
    lens = [0, 1, 63, 64, 65, n] + S(kind, [129, 257], [2049, 4097, 5000])
    rad = lengths_radii(rc, lens)
    want = rc.model(rad, max_rungs=0)
    assert set(lens) <= set(counts(want).tolist())
    check(rc.hnsw(ida).search_range(rc.q, rad, ida.Search(), max_rungs=0), want, "lengths")


def test_sort_does_not_depend_on_the_chunk(eng, oracle, monkeypatch):
    """a small LDS chunk sends every list longer than it through the global-memory strides of the sort"""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    rc = main_case(oracle, kind)
    n = len(rc.raw)
    lens = [0, 1, 127, 128, 129, 255, 256, 257, 300, 511, 513, n // 2 + 1, n - 1, n]
    rad = lengths_radii(rc, lens)
    want = rc.model(rad, max_rungs=0)
    assert set(lens) <= set(counts(want).tolist())
    nq = S(kind, len(rc.q), 60)                                        # (gpu: a tenth of the batch is enough for every length)
    for chunk in ("128", "256"):
        monkeypatch.setenv("IDIST_RANGE_SORT_CHUNK", chunk)
        check(rc.hnsw(ida).search_range(rc.q[:nq], rad[:nq], ida.Search(), max_rungs=0), rc.model(rad[:nq], 0, queries=range(nq)), f"chunk {chunk}")


# ---- 7. refusals and bounds ------------------------------------------------------------------------------------------------------
def test_refusals_and_bounds(eng, oracle):
    ida, kind = eng
    from instant_distance_amd import _capi

    rc = main_case(oracle, kind)
    h, s = rc.hnsw(ida), ida.Search()
    q, nq = rc.q[:12], 12
    rad = radii_of(rc)[:nq].copy()
    L = _capi.lib()
    lims, rung = np.zeros(nq + 1, np.uint64), np.zeros(nq, np.uint32)

    def call(radius, n_radius, max_rungs=-1, max_total=1 << 40, queries=q, out_lims=lims, n=nq):
        return L.idist_search_batch_range(h._h, s._bind(h), _capi.f32p(queries) if queries is not None else None, n,
                                          _capi.f32p(radius) if radius is not None else None, n_radius, max_rungs, max_total,
                                          _capi.u64p(out_lims) if out_lims is not None else None, _capi.u32p(rung), None)

    pid, dist = np.zeros(8, np.uint32), np.zeros(8, np.float32)
    assert L.idist_search_ctx_range_fetch(s._bind(h), _capi.u32p(pid), _capi.f32p(dist)) == 1          # fetch before any call
    bad = rad.copy()
    bad[7] = np.nan
    assert call(bad, nq) == 1 and b"query 7" in L.idist_last_error()
    with pytest.raises(ida.IdistError) as e:
        h.search_range(q, bad, s)
    assert e.value.status == 1 and "query 7" in str(e.value)
    assert call(np.array([np.nan], np.float32), 1) == 1 and b"NaN" in L.idist_last_error()
    assert call(rad, 5) == 1 and call(rad, 0) == 1                                                    # n_radius not in {1, nq}
    with pytest.raises(ValueError):
        h.search_range(q, rad[:5], s)
    assert call(rad, nq, max_rungs=-2) == 1
    assert call(None, nq) == 1 and call(rad, nq, queries=None) == 1 and call(rad, nq, out_lims=None) == 1
    assert L.idist_search_ctx_range_fetch(s._bind(h), _capi.u32p(pid), _capi.f32p(dist)) == 1          # a refused call leaves nothing to fetch
    # max_total: one below the true total is an error that says what was known, the exact total succeeds
    want = rc.model(rad, queries=range(nq))
    total = int(want[0][-1])
    assert total > 0
    assert call(rad, nq, max_total=total - 1) == 1
    msg = L.idist_last_error().decode()
    assert "max_total" in msg and str(total - 1) in msg and str(total) in msg        # (more than total - 1 and at most total were known)
    assert L.idist_search_ctx_range_fetch(s._bind(h), _capi.u32p(pid), _capi.f32p(dist)) == 1          # ... and holds nothing
    with pytest.raises(ida.IdistError):
        h.search_range(q, rad, s, max_total=total - 1)
    with pytest.raises(ida.IdistError):
        h.search_range(q, rad, s, max_rungs=0, max_total=int(rc.model(rad, 0, queries=range(nq))[0][-1]) - 1)
    check(h.search_range(q, rad, s, max_total=total, counters=True), want, "max_total == the total")
    # the results are handed out once
    assert call(rad, nq) == 0 and int(lims[nq]) == total and lims[0] == 0
    pid, dist = np.zeros(total, np.uint32), np.zeros(total, np.float32)
    assert L.idist_search_ctx_range_fetch(s._bind(h), _capi.u32p(pid), _capi.f32p(dist)) == 0
    assert np.array_equal(pid, want[1]) and np.array_equal(pc.bits(dist), want[2])
    assert L.idist_search_ctx_range_fetch(s._bind(h), _capi.u32p(pid), _capi.f32p(dist)) == 1
    # nq = 0
    r0 = h.search_range(np.zeros((0, q.shape[1]), np.float32), 1.0, s, counters=True)
    assert np.array_equal(r0.lims, np.zeros(1, np.uint64)) and r0.pid.shape == (0,) and r0.rung.shape == (0,) and r0.counters.shape == (0, 3)
    # ef_search = 0, and no points: nothing to find
    h0 = ida.Hnsw.from_parts(rc.raw, rc.c.zero, rc.c.layers, ida.Builder().ef_search(0))
    r = h0.search_range(q, np.inf, ida.Search(), counters=True)
    assert np.all(r.lims == 0) and np.all(r.rung == NONE) and np.all(r.counters == 0) and r.pid.shape == (0,)
    he = ida.Hnsw.from_ordered_points(np.zeros((0, 4), np.float32), ida.Builder())
    r = he.search_range(np.zeros((3, 4), np.float32), np.inf, ida.Search())
    assert np.all(r.lims == 0) and np.all(r.rung == NONE)


# ---- 8. HnswMap ----------------------------------------------------------------------------------------------------------------
def test_hnsw_map(eng):
    ida, kind = eng
    rng = np.random.default_rng(2)
    pts = rng.random((120, 5), dtype=np.float32)
    values = [f"v{i}" for i in range(120)]
    m = ida.Builder().seed(7).ef_search(12).build(pts, values)
    q = rng.random((4, 5), dtype=np.float32)
    rad = np.array([0.05, 0.2, 0.4, 10.0], np.float32)
    items = m.search_range(q, rad, ida.Search())
    r = m.hnsw.search_range(q, rad, ida.Search())
    assert len(items) == 4 and len(items[3]) == 120 and len(items[1]) >= 1
    for i, row in enumerate(items):
        lo, hi = int(r.lims[i]), int(r.lims[i + 1])
        assert [it.pid for it in row] == r.pid[lo:hi].tolist()
        assert [np.float32(it.distance) for it in row] == r.distance[lo:hi].tolist() and all(it.distance <= rad[i] for it in row)
        assert all(it.value == m.values[it.pid] and np.array_equal(it.point, m.hnsw[it.pid]) for it in row)
        assert all(values[int(np.flatnonzero((pts == it.point).all(axis=1))[0])] == it.value for it in row)


# ---- 9. the staging is reused ----------------------------------------------------------------------------------------------------
def test_second_call_on_the_same_context(eng, oracle):
    ida, kind = eng
    rc = main_case(oracle, kind)
    h, s = rc.hnsw(ida), ida.Search()
    check(h.search_range(rc.q, np.inf, s, max_rungs=0), rc.model(np.inf, max_rungs=0), "everything")       # nq * n results
    rad = radii_of(rc)
    check(h.search_range(rc.q, rad, s, counters=True), rc.model(rad), "then the per-query radii")
    sub = range(3, 11)
    check(h.search_range(rc.q[3:11], rad[3:11], s, max_rungs=1, counters=True), rc.model(rad[3:11], 1, queries=sub), "then eight queries")
    a, b, c = s.range_kernel_ms()
    assert a >= 0 and b >= 0 and c >= 0


# ---- 10. NaN and +-inf in a query ------------------------------------------------------------------------------------------------
def test_non_finite_queries(eng, oracle):
    ida, kind = eng
    n, dim, ef = S(kind, 400, 1500), 6, 8
    rng = np.random.default_rng(21)
    pts, q = rng.random((n, dim), dtype=np.float32), rng.random((8, dim), dtype=np.float32)
    q[0, 2], q[1, 0], q[2, 5], q[3, 1], q[4, 4], q[5, 3] = np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf
    rc = RCase(oracle, pts, q, ef)
    rad = np.array([np.inf, np.inf, np.inf, 1.0, 1.0, 1.0, np.inf, 0.5], np.float32)
    h = rc.hnsw(ida)
    for m in (-1, 0):
        want = rc.model(rad, max_rungs=m)
        c = counts(want)
        assert c[0] == 0 and c[3] == 0 and c[4] == 0 and c[5] == 0        # a NaN distance is never within; inf is not <= 1
        assert c[1] > 0 and c[2] > 0 and c[6] > 0                         # inf <= inf
        got = h.search_range(q, rad, ida.Search(), max_rungs=m, counters=True)
        check(got, want, f"max_rungs {m}")
        assert np.all(np.isposinf(got.distance[int(got.lims[1]):int(got.lims[3])]))
    assert counts(rc.model(rad, 0))[1] == n


# ---- 11. a rung that does not fit a wave's LDS ends the ladder (the shape and its arithmetic: tests/test_allowed.py) ---------------
def test_lds_short_rung_ends_the_ladder(eng, oracle):
    """radii that hold more than the 64 results of rung 1 leave their queries pending when rung 2 is refused: the call returns what
    max_rungs = 2 defines"""
    ida, kind = eng
    if "lds" not in _CASES:
        _CASES["lds"] = RCase(oracle, *lds_points(), LDS_EF)
    rc = _CASES["lds"]
    rad = radii_of(rc, ["below", "ef", "4ef", "n/2", "inf", 0, "ef+1", "big"])
    want = rc.model(rad, max_rungs=LDS_R_END)
    print("rungs", want[3].tolist(), "counts", counts(want).tolist())
    assert {0, 1, EXACT} <= set(want[3].tolist()) and counts(want)[want[3] == EXACT].min() > ladder(LDS_EF)[LDS_R_END - 1]
    check(rc.hnsw(ida).search_range(rc.q, rad, ida.Search(), counters=True), want, "the whole ladder")
    lds_rung0_refused(ida, rc.c, lambda hb: hb.search_range(rc.q, rad, ida.Search()))
