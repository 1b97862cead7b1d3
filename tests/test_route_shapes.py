"""Routed search (idist_route.hpp) at the shapes its kernels have regimes for: more than eight centroids (the
second pass of route_kernel, its clamp and a partly filled last pass), every chain geometry of the centroid distance (kdim below 8, the
four-element tail, the zero padding, the dims the indexes use), exact ties and NaN in the order of the parts, more parts than a capped
lists grid has workgroups, an ef_search above one wave in the scatter, and CU-capped grids — each against a model: the route against
the oracle's canonical distance to the centroids, nprobe = n_parts against the unrouted call bit for bit, smaller nprobe against the
numpy merge of the routed parts' own search rows.  Every index is made of tiny parts: the same `Hnsw` may be a part many times, so 64
parts cost three small indexes and an empty one.  Every case runs on the emulator and the MI355X."""
import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params
from test_cus_knob import settings as cus_settings
from test_cus_knob import under
from test_dot import np_norms, np_queries, reported

INVALID, INF_BITS, NAN_BITS = 0xFFFFFFFF, 0x7F800000, 0x7FC00000
L2SQ, COSINE, DOT = 0, 2, 4
EF = 8
SIZES = [6, 3, 9]                   # the three distinct parts
ZERO_Q, NAN_Q = 3, 5                # the query that IS centroid 1, the query with a NaN coordinate
NAN_PART = 11                       # the part whose centroid has a NaN coordinate (n_parts > 12)


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


class Setting:
    pass


def setting(ida, oracle, dim, P, lattice, metric=L2SQ, nq=70):
    """Part p is empty when p % 5 == 2 and distinct[p % 3] otherwise.  Planted: centroid 9 = centroid 1 and centroid P - 1 =
    centroid 0 (n_parts > 9: exact ties, one of them across the eight-centroid pass), a NaN in centroid 11 (n_parts > 12), query 3
    equal to centroid 1 (distance 0, and with n_parts > 9 a tie at the head of its route), a NaN in query 5."""
    rng = np.random.default_rng([dim, P, int(lattice), metric])
    draw = lambda *shape: (rng.integers(-4, 5, shape) if lattice else rng.standard_normal(shape)).astype(np.float32)   # noqa: E731
    rows = [draw(m, dim) for m in SIZES]
    allrows, S = np.concatenate(rows), 0.0
    q = draw(nq, dim)
    q[NAN_Q, 0] = np.nan
    if metric == COSINE:
        space, qp = ida.normalize(allrows), ida.normalize(q)
    elif metric == DOT:
        (space, S), qp = ida.augment_dot(allrows), np_queries(q)
    else:
        space, qp = allrows, q
    kdim = space.shape[1]
    cuts = np.concatenate([[0], np.cumsum(SIZES)])
    srows = [np.ascontiguousarray(space[cuts[t]: cuts[t + 1]]) for t in range(3)]
    mk = lambda: ida.Builder().metric(metric).ef_search(EF).dot_bound(float(S)) if metric == DOT else ida.Builder().metric(metric).ef_search(EF)   # noqa: E731
    if metric == L2SQ:
        distinct = [ida.Hnsw.from_ordered_points(r, ida.Builder().ef_search(EF)) for r in rows]
        twins = distinct                         # the parts search the rows they hold: they are their own models
    else:
        distinct, twins = [], []
        for r, s in zip(rows, srows):            # one graph for the part and its L2SQ twin over the search-space rows
            o = oracle.Index.build(s, oracle.default_config(metric=0, ef_search=EF), threads=1)
            distinct.append(ida.Hnsw.from_parts(r, o.zero, o.layers, mk()))
            twins.append(ida.Hnsw.from_parts(s, o.zero, o.layers, ida.Builder().ef_search(EF)))
    empty = ida.Hnsw.from_ordered_points(np.zeros((0, dim), np.float32), mk())
    kind = [-1 if p % 5 == 2 else p % 3 for p in range(P)]
    cent = draw(P, kdim)
    cent[1 % P] = qp[ZERO_Q]
    if P > 9:
        cent[9], cent[P - 1] = cent[1], cent[0]
    if P > 12:
        cent[NAN_PART, 0] = np.nan
    s = Setting()
    s.ph = ida.PartitionedHnsw.from_hnsws([empty if t < 0 else distinct[t] for t in kind])
    s.ph.set_centroids(cent)
    s.keep = (distinct, twins, empty)
    s.kind, s.twins, s.cent, s.q, s.qp, s.P, s.nq, s.metric, s.S = kind, twins, cent, q, qp, P, nq, metric, S
    s.live = [p for p in range(P) if kind[p] >= 0]
    s.base = np.concatenate([[0], np.cumsum([0 if t < 0 else SIZES[t] for t in kind])])
    # the parts of every query in the reference's `Candidate` order: distance (all NaN equal and greatest), then the part
    s.keys = []
    for row in qp:
        d = [oracle.distance(row, cent[p], 0) for p in s.live]
        s.keys.append(sorted((NAN_BITS if np.isnan(x) else int(pc.bits(x).ravel()[0]), p) for x, p in zip(d, s.live)))
    s.sq = np_norms(oracle, q) if metric == DOT else None
    return s


def expected_route(s, nprobe):
    route = np.full((s.nq, nprobe), INVALID, np.uint32)
    for i, keys in enumerate(s.keys):
        route[i, : min(nprobe, len(keys))] = [p for _, p in keys[:nprobe]]
    return route


def check_inputs(s, nprobe, route):
    """the planted cases are in the data: a tie decides a route, the NaN centroid comes after every finite one, the NaN query takes
    the lowest non-empty parts"""
    assert route[NAN_Q].tolist() == (s.live + [INVALID] * s.P)[:nprobe]
    assert s.keys[ZERO_Q][0] == (0, 1 % s.P)
    if s.P > 9:
        finite = [i for i in range(s.nq) if i != NAN_Q]
        assert any(len({b for b, _ in s.keys[i][: nprobe + 1]}) < len(s.keys[i][: nprobe + 1]) for i in finite)
        assert s.keys[ZERO_Q][:2] == [(0, 1), (0, 9)] and route[ZERO_Q, 0] == 1
    if s.P > 12:
        for i in finite:
            assert s.keys[i][-1] == (NAN_BITS, NAN_PART) and s.keys[i][-2][0] < NAN_BITS
            at = np.flatnonzero(route[i] == NAN_PART)
            assert len(at) == (nprobe >= len(s.live)) and np.all(at == len(s.live) - 1)


def expected_rows(ida, s, route, ef=EF):
    """the numpy merge, by (raw distance bits, global id), of the routed parts' own search rows; counters summed"""
    res = [t.search_batch(s.qp, ida.Search(), counters=True) for t in s.twins]
    nq = len(s.qp)
    pid, bits = np.full((nq, ef), INVALID, np.uint32), np.full((nq, ef), INF_BITS, np.uint32)
    cnt, ctr = np.zeros(nq, np.uint32), np.zeros((nq, 3), np.uint32)
    for i in range(nq):
        ps = [int(p) for p in route[i] if p != INVALID]
        rs = [res[s.kind[p]] for p in ps]
        gid = np.concatenate([r.pid[i, : r.count[i]].astype(np.uint64) + np.uint64(s.base[p]) for r, p in zip(rs, ps)])
        d = np.concatenate([pc.bits(r.distance)[i, : r.count[i]] for r in rs])
        o = np.lexsort((gid, d))[:ef]
        pid[i, : len(o)], bits[i, : len(o)], cnt[i] = gid[o], d[o], len(o)
        ctr[i] = sum(r.counters[i].astype(np.uint32) for r in rs)
    return pid, bits, cnt, ctr


def check_identity(s):
    full = s.ph.search_batch(s.q, counters=True)
    got = s.ph.search_batch(s.q, counters=True, nprobe=s.P, routes=True)
    assert np.array_equal(got.pid, full.pid) and np.array_equal(pc.bits(got.distance), pc.bits(full.distance))
    assert np.array_equal(got.count, full.count) and np.array_equal(got.counters, full.counters)
    return got


def check_rows(ida, s, nprobe, got, ef=EF):
    pid, bits, cnt, ctr = expected_rows(ida, s, got.route, ef)
    want = {L2SQ: lambda: bits, COSINE: lambda: pc.bits(np.float32(0.5) * bits.view(np.float32)),
            DOT: lambda: reported(bits.view(np.float32), s.sq, s.S)}[s.metric]()
    assert np.array_equal(got.pid, pid) and np.array_equal(got.count, cnt), nprobe
    assert np.array_equal(got.counters, ctr) and np.array_equal(pc.bits(got.distance), want), nprobe
    shared = [len(set(s.kind[p] for p in r if p != INVALID)) < np.count_nonzero(r != INVALID) for r in got.route]
    return any(shared)                           # some query merged two copies of one part: every distance of it tied across parts


def check_setting(ida, s, rows):
    for nprobe in sorted({1, min(3, s.P), s.P}):
        route = expected_route(s, nprobe)
        check_inputs(s, nprobe, route)
        got = check_identity(s) if nprobe == s.P else s.ph.search_batch(s.q, counters=True, nprobe=nprobe, routes=True)
        assert np.array_equal(got.route, route), nprobe
        if rows and nprobe < s.P:
            tied = check_rows(ida, s, nprobe, got)
            assert tied or nprobe == 1


# kdim below 8 (no full step of the eight chains), the four-element tail (dp & 7 == 4) with and without padding, one and many steps,
# the dims the indexes are compiled for; 20 parts: three passes of eight, the last partly filled
DIMS = [1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 20, 33, 128, 300]
ROWS = {(20, 64, True), (300, 20, False), (5, 20, False)}
SETTINGS = [(d, 20, False) for d in DIMS] + [(20, 64, True), (20, 64, False), (6, 9, True), (44, 8, False), (16, 1, False), (768, 17, False)]


@pytest.mark.parametrize("dim,P,lattice", SETTINGS)
def test_route(eng, oracle, dim, P, lattice):
    ida, _ = eng
    s = setting(ida, oracle, dim, P, lattice, nq=10 if dim == 768 else 70)
    check_setting(ida, s, (dim, P, lattice) in ROWS)


@pytest.mark.parametrize("metric", [COSINE, DOT])
def test_route_metric(eng, oracle, metric):
    """centroids and queries in the space the walk searches: normalised queries, kdim = dim + 1 for DOT"""
    ida, _ = eng
    s = setting(ida, oracle, 20, 20, False, metric)
    assert s.cent.shape[1] == 20 + (metric == DOT)
    check_setting(ida, s, True)


def test_wide_rows_through_the_scatter(eng, oracle):
    """ef_search 100: a staged row is more than one wave wide (route_scatter_kernel's `i += 64`); 64 queries are exactly one batch of
    route_lists_kernel"""
    ida, _ = eng
    ef, dim, nq = 100, 12, 64
    rng = np.random.default_rng(12)
    centers = rng.standard_normal((3, dim)) * 2
    rows = [(c + rng.standard_normal((150, dim))).astype(np.float32) for c in centers]
    s = Setting()
    s.twins = []
    for r in rows:
        o = oracle.Index.build(r, oracle.default_config(metric=0, ef_search=ef), threads=1)
        s.twins.append(ida.Hnsw.from_parts(r, o.zero, o.layers, ida.Builder().ef_search(ef)))
    s.kind, s.base, s.P, s.metric = [0, 1, 2], np.array([0, 150, 300, 450]), 3, L2SQ
    s.q = s.qp = (centers[rng.integers(0, 3, nq)] + rng.standard_normal((nq, dim))).astype(np.float32)
    cent = np.stack([r.mean(axis=0) for r in rows]).astype(np.float32)
    s.ph = ida.PartitionedHnsw.from_hnsws(s.twins)
    s.ph.set_centroids(cent)
    keys = [sorted((int(pc.bits(oracle.distance(row, cent[p], 0)).ravel()[0]), p) for p in range(3)) for row in s.q]
    got = check_identity(s)
    assert np.array_equal(got.route, np.array([[p for _, p in k] for k in keys], np.uint32))
    assert np.all(got.count == ef)
    for nprobe in (1, 2):
        got = s.ph.search_batch(s.q, counters=True, nprobe=nprobe, routes=True)
        assert np.array_equal(got.route, np.array([[p for _, p in k[:nprobe]] for k in keys], np.uint32))
        check_rows(ida, s, nprobe, got, ef)
        assert np.all(got.count > 64)


def test_grid_caps(eng, oracle, monkeypatch):
    """IDIST_CUS = 1 and 3 on the GPU (test build), 256 under the emulator, against the model and not run against run.  At one CU the
    route grid is 32 workgroups for 70 queries, the lists grid 32 for 64 parts and the scatter has 210 dense rows for 32 workgroups.
    The count is sampled when an index is made, so the indexes are made under the setting."""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    for cus in cus_settings(kind):
        if cus is None:
            continue                             # unset: test_route's own (20, 64, lattice) case
        under(monkeypatch, cus)
        s = setting(ida, oracle, 20, 64, True)
        route = expected_route(s, 3)
        check_inputs(s, 3, route)
        assert np.count_nonzero(route != INVALID) == 210
        got = s.ph.search_batch(s.q, counters=True, nprobe=3, routes=True)
        assert np.array_equal(got.route, route), cus
        assert check_rows(ida, s, 3, got), cus


def test_all_parts_empty(eng):
    ida, _ = eng
    empty = ida.Hnsw.from_ordered_points(np.zeros((0, 6), np.float32), ida.Builder().ef_search(EF))
    ph = ida.PartitionedHnsw.from_hnsws([empty] * 3)
    ph.set_centroids(np.ones((3, 6), np.float32))
    q = np.random.default_rng(0).standard_normal((9, 6)).astype(np.float32)
    for nprobe in (1, 3):
        r = ph.search_batch(q, counters=True, nprobe=nprobe, routes=True)
        assert np.all(r.count == 0) and np.all(r.counters == 0) and np.all(r.pid == INVALID)
        assert r.route.shape == (9, nprobe) and np.all(r.route == INVALID)
