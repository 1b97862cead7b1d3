"""Diverse search over a partitioned index (idist_partitioned_search_batch_mmr, include/idist.h; idist_mmr_pool.hpp, DESIGN.md section
8.1): the selection of test_mmr.py over the MERGED list, the pair distances between rows that live in different parts.

The candidate list always comes from `PartitionedHnsw.search_batch` on the same object and the rows from the test's own concatenated
array; the expected selection is test_mmr's plain greedy loop.  Everything is compared with array_equal, distances as bit patterns.
Every case runs on the CPU emulator and (-m gpu) on the MI355X."""
import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params
from test_mmr import INVALID, KF, LAMS, check, expected, lattice_columns

_CASES = {}


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    return engine_loader(request.param), request.param


def cuts(n):
    """four parts of unequal size: a large one, a tiny one of 3 points (most queries take no pool entry from it), an empty one, the rest"""
    return [0, n // 3, n // 3 + 3, n // 3 + 3, n]


def case(oracle, dim, n=2000, nq=24, metric=0, lattice=True, bounds=None):
    """points, queries and the oracle's graph of every part (cosine: some graph over the rows), made once per shape"""
    bounds = bounds or cuts(n)
    key = (dim, n, nq, metric, lattice, tuple(bounds))
    if key not in _CASES:
        rng = np.random.default_rng(dim + n)
        draw = (lambda r: rng.integers(-4, 5, (r, dim)).astype(np.float32)) if lattice else (lambda r: rng.random((r, dim), dtype=np.float32))
        pts, q = draw(n), draw(nq)
        graphs = []
        for lo, hi in zip(bounds, bounds[1:]):
            o = oracle.Index.build(pts[lo:hi], oracle.default_config(metric=metric, ef_search=100), threads=8) if hi > lo else None
            graphs.append((o.zero, o.layers) if o else (np.zeros((0, 64), np.uint32), []))
        _CASES[key] = (pts, q, bounds, graphs)
    return _CASES[key]


def hnsws(ida, pts, bounds, graphs, metric=0, device=lambda p: 0):
    mk = lambda p: ida.Builder().metric(metric).ef_search(100).dot_bound(1024.0 if metric == ida.METRIC_DOT else 0.0).device(device(p))   # noqa: E731
    return [ida.Hnsw.from_parts(pts[lo:hi], z, l, mk(p)) for p, (lo, hi, (z, l)) in enumerate(zip(bounds, bounds[1:], graphs))]


@pytest.mark.parametrize("dim,chunk", [(300, None), (300, 5), (44, None)])
def test_lattice_exact_against_f64(eng, oracle, dim, chunk, monkeypatch):
    """integer coordinates in [-4, 4] (every distance and score exact, many scores equal), n = 2000 in parts of 666, 3, 0 and 1331 points,
    24 queries on a grid smaller than the batch (IDIST_CUS=1); 300-d: the tile and the global kernel by the test knob, 44-d: the global
    kernel on a runtime geometry.  chunk 5: four full chunks of queries and a ragged one — the same answer"""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    monkeypatch.setenv("IDIST_CUS", "1")
    if chunk:
        monkeypatch.setenv("IDIST_MMR_CHUNK", str(chunk))
    pts, q, bounds, graphs = case(oracle, dim)
    hs = hnsws(ida, pts, bounds, graphs)
    base = None
    for knob in ("tile", "global") if dim == 300 else ("global",):
        monkeypatch.setenv("IDIST_MMR", knob)            # (sampled when the parts' contexts are made)
        ph = ida.PartitionedHnsw.from_hnsws(hs)
        base = base if base is not None else ph.search_batch(q, counters=True)
        assert np.any(base.pid[:, :33] < bounds[1]) and np.any(base.pid[:, :33] >= bounds[3])       # pools span parts
        for i, (k, fetch) in enumerate(KF):
            lam = LAMS[(i + dim) % 4]
            got = ph.search_mmr(q, k, lam, fetch, counters=True)
            check(got, expected(base, k, fetch, lam, np.float64, lattice_columns(pts)), f"dim {dim}, k {k}, fetch {fetch}, lam {lam}, {knob}")
            assert np.array_equal(got.counters, base.counters)
        assert min(ph.last_mmr_ms()) >= 0.0


def test_one_part_is_the_identity(eng, oracle):
    ida, kind = eng
    pts, q, bounds, graphs = case(oracle, 300, n=600, bounds=[0, 600])
    h = hnsws(ida, pts, bounds, graphs)[0]
    a, b = ida.PartitionedHnsw.from_hnsws([h]).search_mmr(q, 10, 0.5, 64, counters=True), h.search_mmr(q, 10, 0.5, 64, counters=True)
    check(a, (b.pids, b.ranks, pc.bits(b.distances), b.counts), "one part")
    assert np.array_equal(a.counters, b.counters)


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_lam_1_is_search_batch(eng, oracle, metric):
    ida, kind = eng
    pts, q, bounds, graphs = case(oracle, 300, n=600, nq=16, metric=0 if metric == 2 else metric, lattice=False)
    ph = ida.PartitionedHnsw.from_hnsws(hnsws(ida, pts, bounds, graphs, metric))
    base, got = ph.search_batch(q, counters=True), ph.search_mmr(q, 10, 1.0, 40, counters=True)
    assert np.array_equal(got.pids, base.pid[:, :10]) and np.array_equal(pc.bits(got.distances), pc.bits(base.distance[:, :10]))
    assert np.array_equal(got.ranks, np.tile(np.arange(10, dtype=np.uint32), (16, 1))) and np.all(got.counts == 10)
    assert np.array_equal(got.counters, base.counters)


@pytest.mark.parametrize("dim", [300, 44])
@pytest.mark.parametrize("metric", [0, 1])
def test_float_rows_in_f32(eng, oracle, dim, metric, monkeypatch):
    """float data, the loop in np.float32 in the stated operation order.  The pair distances come from Hnsw.distances (the canonical
    path): of the owning part for two rows of one part, of an index over the concatenated rows for a cross-part pair — a chain or fold
    in the pool path that is not idist_distance_batch's fails here"""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    pts, q, bounds, graphs = case(oracle, dim, n=600, nq=8, metric=metric, lattice=False)
    hs = hnsws(ida, pts, bounds, graphs, metric)
    whole = ida.Hnsw.from_parts(pts, np.full((600, 64), INVALID, np.uint32), [], ida.Builder().metric(metric))
    base = ida.PartitionedHnsw.from_hnsws(hs).search_batch(q)
    pool = base.pid[:, :33]
    assert np.all(base.count >= 33)
    rows, ids = pool.reshape(-1), np.repeat(pool, 33, axis=0)
    pair = whole.distances(pts[rows], ids)                         # [q * 33 + s][i] = D(s, i) = D(i, s)
    for h, lo, hi in zip(hs, bounds, bounds[1:]):
        if hi > lo:
            inside = ((rows >= lo) & (rows < hi))[:, None] & (ids >= lo) & (ids < hi)
            pair = np.where(inside, h.distances(pts[rows], np.where(inside, ids - lo, INVALID).astype(np.uint32)), pair)
    pair = pair.reshape(8, 33, 33)
    for knob in ("tile", "global") if dim == 300 else ("global",):
        monkeypatch.setenv("IDIST_MMR", knob)
        ph = ida.PartitionedHnsw.from_hnsws(hs)
        for lam in (0.25, 0.7):
            want = expected(base, 10, 33, lam, np.float32, lambda qi, ids: (lambda s: pair[qi, s]))
            check(ph.search_mmr(q, 10, lam, 33), want, f"dim {dim}, metric {metric}, lam {lam}, IDIST_MMR={knob}")


def test_cosine_is_l2sq_over_normalised_rows(eng, oracle):
    """every part normalises its own rows: the same selection as the L2SQ parts over normalize(points), distances x 0.5f"""
    ida, kind = eng
    pts, q, bounds, graphs = case(oracle, 300, n=600, nq=16, lattice=False)
    pc_ = ida.PartitionedHnsw.from_hnsws(hnsws(ida, pts, bounds, graphs, ida.METRIC_COSINE))
    pl = ida.PartitionedHnsw.from_hnsws(hnsws(ida, ida.normalize(pts), bounds, graphs))
    a, b = pc_.search_mmr(q, 10, 0.5, 64), pl.search_mmr(ida.normalize(q), 10, 0.5, 64)
    check(a, (b.pids, b.ranks, pc.bits(np.float32(0.5) * b.distances), b.counts), "cosine")
    assert not np.array_equal(a.ranks, np.tile(np.arange(10, dtype=np.uint32), (16, 1)))       # the pair term decided something


@pytest.mark.parametrize("dim", [300, 44])
def test_fewer_points_than_ef(eng, oracle, dim):
    """N = 50 < ef_search over parts of 16, 3, 0 and 31 points: count < fetch and count < k, the padding"""
    ida, kind = eng
    pts, q, bounds, graphs = case(oracle, dim, n=50, nq=8)
    ph = ida.PartitionedHnsw.from_hnsws(hnsws(ida, pts, bounds, graphs))
    got = ph.search_mmr(q, 60, 0.25, 100)
    assert got.counts.max() <= 50 < 60 and np.all(got.pids[:, 50:] == INVALID) and np.all(np.isposinf(got.distances[:, 50:]))
    check(got, expected(ph.search_batch(q), 60, 100, 0.25, np.float64, lattice_columns(pts)), f"dim {dim}, N 50")


def test_arguments(eng, oracle):
    ida, kind = eng
    pts, q, bounds, graphs = case(oracle, 44, n=50, nq=8)
    ph = ida.PartitionedHnsw.from_hnsws(hnsws(ida, pts, bounds, graphs))
    for kw in (dict(lam=float("nan")), dict(lam=-0.1), dict(lam=1.5), dict(k=0), dict(k=11, fetch=10), dict(fetch=101)):
        with pytest.raises(ida.IdistError) as e:
            ph.search_mmr(q[:2], **kw)
        assert e.value.status == 1, kw                  # IDIST_ERR_INVALID_ARG
    with pytest.raises(ida.IdistError) as e:
        ida.PartitionedHnsw.from_hnsws(hnsws(ida, pts, bounds, graphs, ida.METRIC_DOT)).search_mmr(q[:2])
    assert e.value.status == 4 and "inner product" in e.value.message      # IDIST_ERR_UNSUPPORTED
    assert ph.search_mmr(np.zeros((0, 44), np.float32), 5).pids.shape == (0, 5)


@pytest.mark.gpu
def test_two_devices_gpu(engine_loader, oracle):
    """parts away from the merge device: the list by peer copy, the packed rows, the peer copy into the pool"""
    ida = engine_loader("gpu")
    from instant_distance_amd import _capi

    if _capi.lib().device_count() < 2:
        pytest.skip("needs two GPUs")
    pts, q, bounds, graphs = case(oracle, 300)
    ph = ida.PartitionedHnsw.from_hnsws(hnsws(ida, pts, bounds, graphs, device=lambda p: p % 2))
    check(ph.search_mmr(q, 10, 0.5, 100), expected(ph.search_batch(q), 10, 100, 0.5, np.float64, lattice_columns(pts)), "two devices")
