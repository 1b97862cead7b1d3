"""Diverse search (idist_search_batch_mmr, include/idist.h): maximal marginal relevance over the list of
`Hnsw::search`, selected on the device.

The candidate list always comes from `search_batch` on the same index and the rows from the test's own array; the expected selection
is the plain greedy loop below, in f64 on an integer lattice (every distance and score is then an exact integer or a multiple of
1/4 in f32 too) and in f32 in the stated operation order on float data.  Everything is compared with array_equal, distances as bit
patterns.  Every case runs on the CPU emulator and (-m gpu) on the MI355X."""
import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params

INVALID = 0xFFFFFFFF
LAMS = (0.0, 0.25, 0.5, 0.75)
TILE_CAP = {128: 256, 300: 128, 768: 128}          # 32 * rows per group of mmr_tile_kernel; the other dims run mmr_global_kernel
KF = ((1, 1), (10, 100), (10, 33), (37, 37))


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    return engine_loader(request.param), request.param


_CASES = {}


def case(oracle, dim, n=2000, nq=64, ef=100, metric=0, lattice=True):
    """points, queries and the oracle's graph over them, made once per shape"""
    key = (dim, n, nq, ef, metric, lattice)
    if key not in _CASES:
        rng = np.random.default_rng(dim + n)
        draw = (lambda r: rng.integers(-4, 5, (r, dim)).astype(np.float32)) if lattice else (lambda r: rng.random((r, dim), dtype=np.float32))
        pts, q = draw(n), draw(nq)
        oix = oracle.Index.build(pts, oracle.default_config(metric=metric, ef_search=ef), threads=8)
        _CASES[key] = (pts, q, oix.zero, oix.layers)
    return _CASES[key]


def greedy(d, column, k, fetch, lam, ft):
    """the definition: d [count] raw distances of the list, column(s) the raw pair distances of every position to position s;
    arithmetic in `ft`, one rounding per operation -> the selected positions"""
    m = min(len(d), fetch)
    lam, d = ft(lam), d[:m].astype(ft)
    mu, sel, mi, free = ft(1) - lam, [0][:m], np.full(m, np.inf, ft), np.arange(m) > 0
    while len(sel) < min(k, m):
        col = column(sel[-1])[:m].astype(ft)
        mi = np.where(col < mi, col, mi)
        score = lam * d if lam == 1 else (lam * d) - (mu * mi)
        cand = np.flatnonzero(free)
        s = cand[np.argmin(score[cand])]             # the first minimum: ties go to the lower position
        sel.append(int(s))
        free[s] = False
    return sel


def expected(base, k, fetch, lam, ft, column_of):
    """the outputs of search_mmr from `base` = search_batch's result; column_of(q, ids) -> column(s) of query q's pool"""
    nq = len(base.count)
    pid, rank = np.full((nq, k), INVALID, np.uint32), np.full((nq, k), INVALID, np.uint32)
    bits, cnt = np.full((nq, k), 0x7F800000, np.uint32), np.zeros(nq, np.uint32)
    for q in range(nq):
        c = int(base.count[q])
        sel = greedy(base.distance[q, :c], column_of(q, base.pid[q, :c]), k, fetch, lam, ft)
        cnt[q] = len(sel)
        pid[q, :len(sel)], rank[q, :len(sel)], bits[q, :len(sel)] = base.pid[q, sel], sel, pc.bits(base.distance[q, sel])
    return pid, rank, bits, cnt


def check(got, want, what):
    for name, g, w in zip(("counts", "ranks", "ids", "distance bits"), (got.counts, got.ranks, got.pids, pc.bits(got.distances)),
                          (want[3], want[1], want[0], want[2])):
        assert np.array_equal(g, w), f"{what}: {name}"


def lattice_columns(pts):
    p64 = pts.astype(np.float64)
    return lambda q, ids: (lambda s: ((p64[ids] - p64[ids[s]]) ** 2).sum(axis=1))


def lattice_runs(dim):
    """(k, fetch, lam) at ef_search 100: every (k, fetch) of KF with one lam, (10, 100) with all four; the tile's cap and cap + 1 need a
    larger ef_search: test_tile_cap_and_beyond"""
    return [(k, f, LAMS[(i + dim) % 4]) for i, (k, f) in enumerate(KF)] + [(10, 100, lam) for lam in LAMS]


@pytest.mark.parametrize("dim", [300, 128, 768, 44, 20])
def test_lattice_exact_against_f64(eng, oracle, dim):
    """integer coordinates in [-4, 4]: every L2SQ distance is an integer < 2^24, every score exact — and many scores are equal, which
    pins the tie rule.  n = 2000, nq = 64 (more queries than the emulator's grid has workgroups), ef_search 100."""
    ida, kind = eng
    pts, q, zero, layers = case(oracle, dim)
    h = ida.Hnsw.from_parts(pts, zero, layers, ida.Builder().ef_search(100))
    base = h.search_batch(q, ida.Search(), counters=True)
    s = ida.Search()
    for k, fetch, lam in lattice_runs(dim):
        got = h.search_mmr(q, k, lam, fetch, s, counters=True)
        check(got, expected(base, k, fetch, lam, np.float64, lattice_columns(pts)), f"dim {dim}, k {k}, fetch {fetch}, lam {lam}")
        assert np.array_equal(got.counters, base.counters)
    assert s.mmr_kernel_ms() >= 0.0


@pytest.mark.parametrize("dim,ef", [(300, 130), (128, 260), (768, 130)])
def test_tile_cap_and_beyond(eng, oracle, dim, ef, monkeypatch):
    """fetch at the tile's cap, every slot of the tile live (the tile kernel by the test knob, and whatever the policy picks), and one
    above it (the global kernel), at an ef_search that allows both"""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    pts, q, zero, layers = case(oracle, dim, nq=8, ef=ef)
    h = ida.Hnsw.from_parts(pts, zero, layers, ida.Builder().ef_search(ef))
    base = h.search_batch(q, ida.Search())
    for knob, fetch in (("tile", TILE_CAP[dim]), ("policy", TILE_CAP[dim]), ("policy", TILE_CAP[dim] + 1)):
        monkeypatch.setenv("IDIST_MMR", knob)          # (anything but tile / global leaves the choice to plan_mmr)
        want = expected(base, 10, fetch, 0.5, np.float64, lattice_columns(pts))
        check(h.search_mmr(q, 10, 0.5, fetch, ida.Search()), want, f"dim {dim}, fetch {fetch}, IDIST_MMR={knob}")


@pytest.mark.parametrize("dim", [300, 44])
def test_fewer_points_than_ef(eng, oracle, dim):
    """n = 50 < ef_search: count < fetch and count < k, the padding"""
    ida, kind = eng
    pts, q, zero, layers = case(oracle, dim, n=50, nq=8)
    h = ida.Hnsw.from_parts(pts, zero, layers, ida.Builder().ef_search(100))
    base = h.search_batch(q, ida.Search())
    got = h.search_mmr(q, 60, 0.25, 100)
    assert got.counts.max() <= 50 < 60 and np.all(got.pids[:, 50:] == INVALID) and np.all(np.isposinf(got.distances[:, 50:]))
    check(got, expected(base, 60, 100, 0.25, np.float64, lattice_columns(pts)), f"dim {dim}, n 50")


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_lam_1_is_search_batch(eng, oracle, metric):
    ida, kind = eng
    pts, q, zero, layers = case(oracle, 300, n=600, nq=16, metric=0 if metric == 2 else metric, lattice=False)
    h = ida.Hnsw.from_parts(pts, zero, layers, ida.Builder().metric(metric).ef_search(100))   # (cosine: some graph over the rows)
    base = h.search_batch(q, ida.Search(), counters=True)
    got = h.search_mmr(q, 10, 1.0, 40, counters=True)
    assert np.array_equal(got.pids, base.pid[:, :10]) and np.array_equal(pc.bits(got.distances), pc.bits(base.distance[:, :10]))
    assert np.array_equal(got.ranks, np.tile(np.arange(10, dtype=np.uint32), (16, 1))) and np.all(got.counts == 10)
    assert np.array_equal(got.counters, base.counters)


@pytest.mark.parametrize("dim", [300, 44])
@pytest.mark.parametrize("metric", [0, 1])
def test_float_rows_in_f32(eng, oracle, dim, metric, monkeypatch):
    """float data: the pair distances from Hnsw.distances (the canonical path), the loop in np.float32 in the stated operation order —
    on the GPU the test that fails if a score is fused into an fma, or a chain or fold of a kernel is not idist_distance_batch's.
    Every kernel the geometry has runs it, by the test knob: at 300-d the tile (a partly filled slot) and the global kernel"""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    pts, q, zero, layers = case(oracle, dim, n=600, nq=8, metric=metric, lattice=False)
    h = ida.Hnsw.from_parts(pts, zero, layers, ida.Builder().metric(metric).ef_search(100))
    base = h.search_batch(q, ida.Search())
    pool = base.pid[:, :33]
    assert np.all(base.count >= 33)
    pair = h.distances(pts[pool.reshape(-1)], np.repeat(pool, 33, axis=0)).reshape(8, 33, 33)   # [q][s][i] = D(s, i) = D(i, s)
    for lam in (0.25, 0.7):
        want = expected(base, 10, 33, lam, np.float32, lambda qi, ids: (lambda s: pair[qi, s]))
        for knob in ("tile", "global") if dim in TILE_CAP else ("global",):
            monkeypatch.setenv("IDIST_MMR", knob)      # (sampled when the context is made)
            check(h.search_mmr(q, 10, lam, 33, ida.Search()), want, f"dim {dim}, metric {metric}, lam {lam}, IDIST_MMR={knob}")


def test_cosine_is_l2sq_over_normalised_rows(eng, oracle):
    ida, kind = eng
    pts, q, _, _ = case(oracle, 300, n=600, nq=16, lattice=False)
    rows, nq_ = ida.normalize(pts), ida.normalize(q)
    oix = oracle.Index.build(rows, oracle.default_config(metric=0, ef_search=100), threads=8)
    hc = ida.Hnsw.from_parts(pts, oix.zero, oix.layers, ida.Builder().metric(ida.METRIC_COSINE).ef_search(100))
    hl = ida.Hnsw.from_parts(rows, oix.zero, oix.layers, ida.Builder().ef_search(100))
    a, b = hc.search_mmr(q, 10, 0.5, 64), hl.search_mmr(nq_, 10, 0.5, 64)
    assert np.array_equal(a.pids, b.pids) and np.array_equal(a.ranks, b.ranks) and np.array_equal(a.counts, b.counts)
    assert np.array_equal(pc.bits(a.distances), pc.bits(np.float32(0.5) * b.distances))
    assert not np.array_equal(a.ranks, np.tile(np.arange(10, dtype=np.uint32), (16, 1)))       # the pair term decided something


@pytest.mark.parametrize("dim", [300, 128, 768])
def test_tile_against_global(eng, oracle, dim, monkeypatch):
    """both kernels under the test knob, on a grid smaller than the batch (IDIST_CUS=1), on every run of the lattice test — whatever the
    policy makes of it, the tile kernel runs k = m = 1, a partly filled slot (fetch 33, 37) and every lam: equal to each other and to
    the definition.  24 of the lattice test's queries: at one CU the tile's grid is 1 or 2 workgroups, the global kernel's 16"""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    monkeypatch.setenv("IDIST_CUS", "1")
    pts, q, zero, layers = case(oracle, dim)
    q = q[:24]
    h = ida.Hnsw.from_parts(pts, zero, layers, ida.Builder().ef_search(100))
    base = h.search_batch(q, ida.Search())
    ctx = {}
    for knob in ("tile", "global"):
        monkeypatch.setenv("IDIST_MMR", knob)
        ctx[knob] = ida.Search()                       # (the knob is sampled when the context is made)
    for k, fetch, lam in lattice_runs(dim):
        want = expected(base, k, fetch, lam, np.float64, lattice_columns(pts))
        for knob in ("tile", "global"):
            check(h.search_mmr(q, k, lam, fetch, ctx[knob]), want, f"dim {dim}, k {k}, fetch {fetch}, lam {lam}, IDIST_MMR={knob}")
    monkeypatch.setenv("IDIST_MMR", "tile")
    with pytest.raises(ida.IdistError):                # no quiet fall-back: the tile kernel has no such pool
        ida.Hnsw.from_parts(pts, zero, layers, ida.Builder().ef_search(300)).search_mmr(q[:2], 10, 0.5, 300, ida.Search())


def test_arguments(eng, oracle):
    ida, kind = eng
    pts, q, zero, layers = case(oracle, 20)
    h = ida.Hnsw.from_parts(pts, zero, layers, ida.Builder().ef_search(100))
    for kw in (dict(lam=float("nan")), dict(lam=-0.1), dict(lam=1.5), dict(k=0), dict(k=11, fetch=10), dict(fetch=101)):
        with pytest.raises(ida.IdistError) as e:
            h.search_mmr(q[:2], **kw)
        assert e.value.status == 1, kw                  # IDIST_ERR_INVALID_ARG
    hd = ida.Hnsw.from_parts(pts, zero, layers, ida.Builder().metric(ida.METRIC_DOT).ef_search(100))
    with pytest.raises(ida.IdistError) as e:
        hd.search_mmr(q[:2])
    assert e.value.status == 4 and "inner product" in e.value.message      # IDIST_ERR_UNSUPPORTED
    m = ida.HnswMap(h, [str(i) for i in range(len(pts))]).search_mmr(q[:2], 5, 0.5)
    r = h.search_mmr(q[:2], 5, 0.5)
    assert [[it.pid for it in row] for row in m] == r.pids.tolist() and m[0][0].value == str(r.pids[0, 0])
