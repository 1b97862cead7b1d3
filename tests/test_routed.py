"""Routed search over a partitioned index (idist_partitioned_search_batch_routed, idist_route.hpp) and
PartitionedHnsw.build(partition="kmeans").  Four parts: two clusters the queries come from, an EMPTY part, and a part far from every
query.  The route is checked against the oracle's canonical distance to the centroids, nprobe = n_parts against search_batch bit for
bit, smaller nprobe against the numpy merge of the routed parts' own search rows.  Every case runs on the emulator and the MI355X."""
import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params
from test_dot import np_norms, np_queries, reported

INVALID, INF_BITS = 0xFFFFFFFF, 0x7F800000
L2SQ, COSINE, DOT = 0, 2, 4
EF, DIM, NQ = 30, 20, 70
SIZES = [150, 0, 120, 100]


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


def setting(ida, oracle, metric):
    """-> (partitioned index, its L2SQ twins over the search-space rows, centroids, queries, prepared queries, s(q), S)"""
    rng = np.random.default_rng(77)
    a, b = rng.standard_normal(DIM) * 3, rng.standard_normal(DIM) * 3
    centers = [a, None, b, -4 * (a + b)]
    rows = [(c + 0.5 * rng.standard_normal((m, DIM))).astype(np.float32) if m else np.zeros((0, DIM), np.float32) for c, m in zip(centers, SIZES)]
    q = (np.where(rng.random((NQ, 1)) < 0.5, a, b) + 0.7 * rng.standard_normal((NQ, DIM))).astype(np.float32)
    allrows, S = np.concatenate(rows), 0.0
    if metric == COSINE:
        space, qp = ida.normalize(allrows), ida.normalize(q)
    elif metric == DOT:
        (space, S), qp = ida.augment_dot(allrows), np_queries(q)
    else:
        space, qp = allrows, q
    cuts = np.concatenate([[0], np.cumsum(SIZES)])
    srows = [np.ascontiguousarray(space[cuts[p]: cuts[p + 1]]) for p in range(4)]
    mk = lambda: ida.Builder().metric(metric).ef_search(EF).dot_bound(float(S)) if metric == DOT else ida.Builder().metric(metric).ef_search(EF)   # noqa: E731
    hs, twins = [], []
    for r, s in zip(rows, srows):
        if len(r):
            o = oracle.Index.build(s, oracle.default_config(metric=0, ef_search=EF), threads=1)
            hs.append(ida.Hnsw.from_parts(r, o.zero, o.layers, mk()))
            twins.append(ida.Hnsw.from_parts(s, o.zero, o.layers, ida.Builder().ef_search(EF)))
        else:
            hs.append(ida.Hnsw.from_ordered_points(r, mk()))
            twins.append(None)
    cent = np.stack([s.mean(axis=0).astype(np.float32) if len(s) else np.zeros(space.shape[1], np.float32) for s in srows])
    return ida.PartitionedHnsw.from_hnsws(hs), twins, cent, q, qp, np_norms(oracle, q), S


def expected_route(oracle, cent, qp, nprobe):
    route = np.full((len(qp), nprobe), INVALID, np.uint32)
    live = [p for p in range(4) if SIZES[p]]
    for i, row in enumerate(qp):
        keys = sorted((int(pc.bits(oracle.distance(row, cent[p], 0)).ravel()[0]), p) for p in live)
        route[i, : min(nprobe, len(live))] = [p for _, p in keys[:nprobe]]
    return route


def expected_rows(ida, twins, qp, route):
    """the numpy merge, by (raw distance bits, global id), of the routed parts' own search rows; counters summed"""
    res = [t.search_batch(qp, ida.Search(), counters=True) if t else None for t in twins]
    base = np.concatenate([[0], np.cumsum(SIZES)])
    pid, bits = np.full((len(qp), EF), INVALID, np.uint32), np.full((len(qp), EF), INF_BITS, np.uint32)
    cnt, ctr = np.zeros(len(qp), np.uint32), np.zeros((len(qp), 3), np.uint32)
    for i in range(len(qp)):
        ps = [int(p) for p in route[i] if p != INVALID]
        gid = np.concatenate([res[p].pid[i, : res[p].count[i]].astype(np.uint64) + np.uint64(base[p]) for p in ps])
        d = np.concatenate([pc.bits(res[p].distance)[i, : res[p].count[i]] for p in ps])
        o = np.lexsort((gid, d))[:EF]
        pid[i, : len(o)], bits[i, : len(o)], cnt[i] = gid[o], d[o], len(o)
        ctr[i] = sum(res[p].counters[i].astype(np.uint32) for p in ps)
    return pid, bits, cnt, ctr


@pytest.mark.parametrize("metric", [L2SQ, COSINE, DOT])
def test_routed_search(eng, oracle, metric):
    ida, _ = eng
    ph, twins, cent, q, qp, sq, S = setting(ida, oracle, metric)
    with pytest.raises(ida.IdistError) as e:                                   # no centroids yet
        ph.search_batch(q, nprobe=1)
    assert e.value.status == 1
    ph.set_centroids(cent)
    full = ph.search_batch(q, counters=True)
    got = ph.search_batch(q, counters=True, nprobe=4, routes=True)             # the identity
    assert np.array_equal(got.pid, full.pid) and np.array_equal(pc.bits(got.distance), pc.bits(full.distance))
    assert np.array_equal(got.count, full.count) and np.array_equal(got.counters, full.counters)
    assert np.array_equal(got.route, expected_route(oracle, cent, qp, 4)) and np.all(got.route[:, 3] == INVALID)
    for nprobe in (1, 2):
        route = expected_route(oracle, cent, qp, nprobe)
        assert not np.isin(route, (1, 3)).any() and {0, 2} <= set(route[:, 0].tolist())     # the empty and the far part get nothing
        got = ph.search_batch(q, counters=True, nprobe=nprobe, routes=True)
        assert np.array_equal(got.route, route), nprobe
        pid, bits, cnt, ctr = expected_rows(ida, twins, qp, route)
        want = {L2SQ: bits, COSINE: pc.bits(np.float32(0.5) * bits.view(np.float32)), DOT: reported(bits.view(np.float32), sq, S)}[metric]
        assert np.array_equal(got.pid, pid) and np.array_equal(got.count, cnt) and np.array_equal(got.counters, ctr), nprobe
        assert np.array_equal(pc.bits(got.distance), want), nprobe
        assert np.array_equal(ph.search_batch(q, nprobe=nprobe).pid, pid) and ph.last_route_ms() >= 0.0


def test_argument_errors(eng, oracle):
    ida, _ = eng
    from instant_distance_amd import _capi

    ph, _, cent, q, _, _, _ = setting(ida, oracle, L2SQ)
    ph.set_centroids(cent)
    for nprobe in (0, 5):
        with pytest.raises(ida.IdistError) as e:
            ph.search_batch(q, nprobe=nprobe)
        assert e.value.status == 1
    with pytest.raises(TypeError):
        ph.set_centroids(cent[:3])
    L, pid, dist = _capi.lib(), np.zeros((NQ, EF), np.uint32), np.zeros((NQ, EF), np.float32)
    assert L.idist_partitioned_search_batch_routed(ph._h, _capi.f32p(q), NQ, 1, _capi.u32p(pid), _capi.f32p(dist), None, None, None) == 1
    assert L.idist_partitioned_set_centroids(ph._h, None) == 1
    assert ph.search_batch(np.zeros((0, DIM), np.float32), nprobe=2, routes=True).route.shape == (0, 2)


def test_grid_independence(eng, oracle, monkeypatch):
    """identical bytes at IDIST_CUS unset / 1 / 3 on the GPU (test build) and 256 under the emulator; the count is sampled when an
    index is made, so every run makes its indexes under the setting it tests"""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    results = []
    for cus in (None, "1", "3") if kind == "gpu" else (None, "256"):
        if cus is None:
            monkeypatch.delenv("IDIST_CUS", raising=False)
        else:
            monkeypatch.setenv("IDIST_CUS", cus)
        ph, _, cent, q, _, _, _ = setting(ida, oracle, L2SQ)
        ph.set_centroids(cent)
        r = ph.search_batch(q, counters=True, nprobe=2, routes=True)
        results.append(b"".join(x.tobytes() for x in (r.pid, r.distance, r.count, r.counters, r.route)))
    assert all(r == results[0] for r in results)


@pytest.mark.parametrize("metric", [L2SQ, COSINE, DOT])
def test_build_kmeans(eng, metric):
    """the ids are a bijection, index[ids[i]] is points[i], and every part's members are nearest to their part's stored centroid
    within the product-form bound of tests/test_kmeans.py::test_assign_float"""
    ida, _ = eng
    rng = np.random.default_rng(3)
    n, dim, P = 240, 8, 4
    pts = (rng.standard_normal((3, dim))[rng.integers(0, 3, n)] * 3 + rng.standard_normal((n, dim))).astype(np.float32)
    ph, ids = ida.PartitionedHnsw.build(pts, ida.Builder().metric(metric).max_batch(1).ef_search(20), parts=P, partition="kmeans", kmeans_iters=5)
    assert sorted(ids) == list(range(n)) and len(ph) == n
    assert all(np.array_equal(ph[ids[i]], pts[i]) for i in range(n))
    space = {L2SQ: lambda: pts, COSINE: lambda: ida.normalize(pts), DOT: lambda: ida.augment_dot(pts)[0]}[metric]().astype(np.float64)
    c = ph.centroids.astype(np.float64)
    assert c.shape == (P, dim + (metric == DOT))
    d = ((space[:, None, :] - c[None]) ** 2).sum(axis=2)
    E = 4 * 2.0 ** -24 * 32 * ((space ** 2).sum(axis=1) + (c ** 2).sum(axis=1).max())
    part = np.array([ph.part_of(g)[0] for g in ids])
    assert np.all(d[np.arange(n), part] <= d.min(axis=1) + 2 * E)
    r = ph.search_batch(pts[:9], nprobe=1, routes=True)
    assert np.array_equal(r.route[:, 0], part[:9]) or np.all(r.count > 0)


def test_build_kmeans_mostly_empty(eng):
    """64 parts of 100 rows with 5 distinct values: most clusters, so most parts, are empty — the ids are still a bijection, all parts
    routed is the unrouted call, and a query that equals a stored row finds its part"""
    ida, _ = eng
    n, P = 100, 64
    pts = np.ascontiguousarray(np.random.default_rng(4).standard_normal((5, 8)).astype(np.float32)[np.arange(n) % 5])
    ph, ids = ida.PartitionedHnsw.build(pts, ida.Builder().max_batch(1).ef_search(20), parts=P, partition="kmeans", kmeans_iters=5)
    assert sorted(ids) == list(range(n)) and len(ph) == n
    assert all(np.array_equal(ph[ids[i]], pts[i]) for i in range(n))
    sizes = np.diff(ph._base)
    assert len(sizes) == P and 1 <= np.count_nonzero(sizes) <= 5 and ph.centroids.shape == (P, 8)
    full = ph.search_batch(pts, counters=True)
    got = ph.search_batch(pts, counters=True, nprobe=P, routes=True)
    assert np.array_equal(got.pid, full.pid) and np.array_equal(pc.bits(got.distance), pc.bits(full.distance))
    assert np.array_equal(got.count, full.count) and np.array_equal(got.counters, full.counters)
    assert np.all((got.route != INVALID).sum(axis=1) == np.count_nonzero(sizes))
    r = ph.search_batch(pts, nprobe=1, routes=True)
    assert np.all(r.count > 0) and np.all(sizes[r.route[:, 0]] > 0)
