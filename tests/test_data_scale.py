"""Every distance path on data far from magnitude 1.

The data is always `ldexp(gen_points(...), s)` with the queries scaled by the same s: a power of two makes every f32 operation an
exact rescaling until something under- or overflows, so the oracle's answer at s is its answer at 0 with the distances `ldexp`-ed
(asserted here on the oracle alone, for the scales at which nothing saturates) — and the product has to follow the oracle bit for
bit at EVERY scale: where its own constants (the reject filter's lattice step and its square, the `+ 1e-30f` floors and the
`product_form_eps(K) * (|a|^2 + |b|^2)` margins of the MFMA filters, the row norms behind METRIC_DOT) become denormal, zero or inf long before the
canonical distances do.

  normal            s = -40, +40, +60         nothing saturates; the reject filter must still be at work
  denormal lattice  s = -56 ... -59, -62      the square of the lattice step is a denormal f32 (or 0): the filter may switch
                                              itself off there, it must not reject what `Search::push` accepts
  partly saturated  16-d uniform at s = +63   ~4 % of the squared distances are +inf
                    16-d uniform at s = -70   the squared distances are denormals of ~1300 quanta
Fully saturated data (all +inf / all 0: s = +64, -80) is nothing but ties; only the distance kernel sees it here."""
import numpy as np
import pytest

import parity_cases as pc
import test_allowed
import test_dot
from engines import engine_params
from test_filter import WALKS

NORMAL = (-40, 40, 60)
DENORMAL = (-56, -57, -58, -59, -62)
PARTLY = (63, -70)                   # 16-d uniform only
FOUR_WAVES = next(env for name, env in pc.SEARCH_VARIANTS if name == "four waves per query, quotient set")


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    return engine_loader(request.param), request.param


def per_engine(emu, gpu):
    """parameter tuples that differ by engine: ("emu", ...) for each of `emu`, ("gpu", ...) with the gpu mark for each of `gpu`"""
    e, g = engine_params()
    return [pytest.param(*e.values, *c, marks=e.marks) for c in emu] + [pytest.param(*g.values, *c, marks=g.marks) for c in gpu]


def S(kind, emu, gpu):
    return emu if kind == "emu" else gpu


def empty_graph(ida, pts, metric=0):
    """an index without edges: enough for the pair kernels and the brute force"""
    return ida.Hnsw.from_parts(pts, np.full((len(pts), 64), pc.INVALID, np.uint32), [], ida.Builder().metric(metric))


def scaled_distance(d0, s, metric):
    """what the canonical distance becomes when both points are multiplied by 2^s (nothing saturating)"""
    return np.ldexp(d0, s if metric else 2 * s).astype(np.float32)


# ---- a. the distance kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 16, 300])
@pytest.mark.parametrize("metric", [0, 1])
def test_distance_batch_at_scale(eng, oracle, dim, metric):
    """idist_distance_batch == FloatArray::distance, bit for bit, while the terms and the result of the chain go denormal, to 0
    and to +inf.  (No ties to worry about here: the fully saturated scales are fair.)"""
    ida, kind = eng
    n, nq, n_ids = S(kind, 60, 1000), S(kind, 4, 8), S(kind, 40, 200)
    rng = np.random.default_rng(300 + dim)
    pts0, q0 = pc.gen_points(rng, n, dim), pc.gen_points(rng, nq, dim)
    ids = rng.integers(0, n, size=(nq, n_ids)).astype(np.uint32)
    ids[0, 3] = pc.INVALID
    ids[-1, -1] = pc.INVALID

    def oracle_pairs(pts, q):
        return np.array([[oracle.distance(q[i], pts[j], metric) if j != pc.INVALID else np.inf for j in ids[i]]
                         for i in range(nq)], dtype=np.float32)

    want0 = oracle_pairs(pts0, q0)
    classes = set()
    for s in NORMAL + DENORMAL + PARTLY + (64, -80):
        pts, q = np.ldexp(pts0, s).astype(np.float32), np.ldexp(q0, s).astype(np.float32)
        want = oracle_pairs(pts, q)
        if s in NORMAL:                                  # the inputs are what the module's docstring says: an exact rescaling
            assert np.array_equal(pc.bits(want), pc.bits(scaled_distance(want0, s, metric))), s
        got = empty_graph(ida, pts, metric).distances(q, ids)
        bad = pc.bits(got) != pc.bits(want)
        assert not bad.any(), (s, int(bad.sum()), got[bad][:4], want[bad][:4])
        real = want[ids != pc.INVALID]
        tiny = np.finfo(np.float32).tiny
        classes |= {"inf"} if np.isposinf(real).any() else set()
        classes |= {"zero"} if (real == 0).any() else set()
        classes |= {"denormal"} if ((real > 0) & (real < tiny)).any() else set()
    # the scales reach what they are here for (metric 1 takes the root: its results stay normal longer)
    assert {"inf", "zero"} <= classes and (metric == 1 or "denormal" in classes)


# ---- b. the filter's bound -------------------------------------------------------------------------------------------------
def check_filter_bound(ida, oracle, kind, pts, q, metric, tight, own=False):
    """the assertions of test_filter_bound_never_exceeds_the_canonical_distance (own: column 5 pairs query i with point i)"""
    rng = np.random.default_rng(5)
    n, nq, dim = len(pts), len(q), pts.shape[1]
    n_ids = S(kind, 70, 500)
    h = empty_graph(ida, pts, metric)
    ids = rng.integers(0, n, size=(nq, n_ids)).astype(np.uint32)
    ids[0, 1] = pc.INVALID
    ids[2, :4] = [0, 1, 2, 3]
    if own:
        ids[:, 5] = np.arange(nq)
    bound = h.filter_bounds(q, ids)
    dist = h.distances(q, ids)
    d0 = np.array([oracle.distance(q[0], pts[j], metric) if j != pc.INVALID else np.inf for j in ids[0]], dtype=np.float32)
    assert np.array_equal(pc.bits(dist[0]), pc.bits(d0))
    assert np.all(np.isfinite(bound)) and np.all(bound >= 0)
    ok = ~np.isnan(dist)
    over = ok & (bound > dist)
    with np.errstate(all="ignore"):
        body = bound[4:].astype(np.float64) / np.maximum(dist[4:].astype(np.float64), 1e-300)
    print(f"dim {dim}: {100.0 * over.sum() / ok.sum():.1f} % of the bounds exceed the distance, median bound / distance {np.median(body):.4f}")
    assert not over.any(), (int(over.sum()), int(ok.sum()), bound[over][:4], dist[over][:4])
    assert bound[0, 1] == 0
    if tight:
        assert np.median(body) > (0.5 if dim < 64 else 0.8), float(np.median(body))
    return bound, dist


@pytest.mark.parametrize("dim,metric,s", [(d, m, s) for d, m in ((16, 0), (128, 1), (300, 0)) for s in NORMAL + DENORMAL]
                         + [(16, 0, s) for s in PARTLY])
def test_filter_bound_at_scale(eng, oracle, dim, metric, s):
    """idist_filter_bound_batch never exceeds idist_distance_batch — also where the square of the lattice step is a denormal with a
    handful of significant bits (s = -57 ... -59: it used to exceed it for EVERY pair) — and stays as tight as at scale 0 where
    nothing saturates.  At the denormal scales validity is all that is asked: the filter may be off (a bound of 0)."""
    ida, kind = eng
    rng = np.random.default_rng(77 + dim)
    n, nq = S(kind, 300, 4000), S(kind, 6, 64)
    pts = pc.gen_points(rng, n, dim, "uniform", s)
    q = pc.gen_points(rng, nq, dim, "uniform", s)
    q[1] = q[1] * np.float32(5.0) - np.ldexp(np.float32(3.0), s)           # far outside the lattice
    check_filter_bound(ida, oracle, kind, pts, q, metric, tight=s in NORMAL)


@pytest.mark.parametrize("offset", [4096.0, -4096.0])
@pytest.mark.parametrize("dim,metric", [(16, 0), (300, 1)])
def test_filter_bound_far_from_the_origin(eng, oracle, dim, metric, offset):
    """data 4096 spreads away from the origin: the f32 coordinates are coarser (2^-12 / 2^-11) than the lattice's sub-steps (2^-16)"""
    ida, kind = eng
    rng = np.random.default_rng(91 + dim)
    n, nq = S(kind, 300, 4000), S(kind, 6, 64)
    pts = (pc.gen_points(rng, n, dim) + np.float32(offset)).astype(np.float32)
    q = (pc.gen_points(rng, nq, dim) + np.float32(offset)).astype(np.float32)
    q[1] = (q[1] - np.float32(offset)) * np.float32(5.0) - np.float32(3.0) + np.float32(offset)
    check_filter_bound(ida, oracle, kind, pts, q, metric, tight=False)


def test_filter_bound_huge_spread(eng, oracle):
    """3-d data spread over 2^80: the square of the lattice step is no finite f32 and almost every squared distance is +inf — but a
    query one ulp from a stored row has a finite one, which inf * I "bounds" by +inf.  (Three coordinates: with twelve or more the
    query's own lattice error overflows as well and hides it.)"""
    ida, kind = eng
    rng = np.random.default_rng(80)
    n, nq = S(kind, 300, 4000), S(kind, 6, 64)
    pts = pc.gen_points(rng, n, 3, "uniform", 80)
    q = np.nextafter(pts[:nq], np.float32(np.inf))
    _, dist = check_filter_bound(ida, oracle, kind, pts, q, 0, tight=False, own=True)
    assert np.all(np.isfinite(dist[:, 5])) and np.all(dist[:, 5] > 0) and np.mean(np.isposinf(dist)) > 0.9


# ---- c. the walks ----------------------------------------------------------------------------------------------------------
def filtered_walks(ida, h, q, want, monkeypatch):
    """every WALKS layout with the filter on and off against `want`; returns (seen, rejected) summed over the filtered runs"""
    total = [0, 0]
    for name, env in WALKS:
        for flt in ("1", "0"):
            with pc.search_variant(env), monkeypatch.context() as m:
                m.setenv("IDIST_FILTER", flt)
                srch = ida.Search()
                got = h.search_batch(q, srch, counters=True)
                seen, rejected = srch.filter_counts()
            pc.check_search_result(got, want)
            if flt == "0":
                assert seen == 0, name
            else:
                total[0] += seen
                total[1] += rejected
                assert rejected <= seen <= int(want.counters[:, 0].sum()), name
    return total


def check_search_at_scale(ida, oracle, kind, monkeypatch, dim, kind_, metric, s):
    n, nq, ef = S(kind, 260, 4000), S(kind, 12, 600), S(kind, 12, 100)
    threads = S(kind, 1, 8)
    cfg = oracle.default_config(metric=metric, ef_search=ef, ef_construction=S(kind, 16, 100))

    def data(scale):
        rng = np.random.default_rng(2000 + dim)
        pts = pc.gen_points(rng, n, dim, kind_, scale)
        q = pc.gen_points(rng, nq, dim, kind_, scale)
        q[0] = pts[n // 2]
        return pts, q

    pts, q = data(s)
    oix = oracle.Index.build(pts, cfg, threads=threads)
    want = oix.search(q, threads=threads)
    b = ida.Builder().metric(metric).ef_search(ef)
    h = ida.Hnsw.from_parts(pts, oix.zero, oix.layers, b)
    pc.check_search_result(h.search_batch(q, ida.Search(), counters=True), want)        # the product, as it ships
    pc.use_test_build(monkeypatch)                     # (the walk knobs and the filter's counters exist in the test build only)
    total = filtered_walks(ida, h, q, want, monkeypatch)
    with pc.search_variant(FOUR_WAVES):
        pc.check_search_result(h.search_batch(q, ida.Search(), counters=True), want)
    if s not in NORMAL:
        return
    # nothing saturates: on the same graph the oracle's answer is its answer at scale 0, rescaled — and the filter is as much at
    # work as there (the shares are printed side by side; their equality is expected, not asserted)
    pts0, q0 = data(0)
    want0 = oracle.Index.from_arrays(pts0, oix.zero, oix.layers, cfg).search(q0, threads=threads)
    assert np.array_equal(want.pid, want0.pid) and np.array_equal(want.count, want0.count)
    assert np.array_equal(want.counters, want0.counters)
    assert np.array_equal(pc.bits(want.dist), pc.bits(scaled_distance(want0.dist, s, metric)))
    total0 = filtered_walks(ida, ida.Hnsw.from_parts(pts0, oix.zero, oix.layers, b), q0, want0, monkeypatch)
    print(f"{dim}-d {kind_} metric {metric}: rejected {total[1]} of {total[0]} ({100.0 * total[1] / max(total[0], 1):.2f} %) at s = {s}, "
          f"{total0[1]} of {total0[0]} ({100.0 * total0[1] / max(total0[0], 1):.2f} %) at s = 0")
    assert total[0] > 0
    assert total[1] > 0.3 * total[0], total            # test_filter's threshold: the filter is not simply off away from 1


@pytest.mark.parametrize("dim,kind_,metric,s",
                         [(d, "uniform", m, s) for d, m in ((300, 0), (128, 1), (16, 0)) for s in NORMAL + DENORMAL]
                         + [(d, "lowrank", 0, s) for d in (300, 128) for s in NORMAL + (-58,)]      # (low-rank rows: one denormal scale)
                         + [(16, "uniform", 0, s) for s in PARTLY])
def test_search_at_scale(eng, oracle, monkeypatch, dim, kind_, metric, s):
    """The oracle builds and searches at scale s; the product imports the graph and returns the same counts, ids, distance bits and
    work counters: as it ships, through every filtered on-chip walk with the filter on and off, and four waves per query."""
    ida, kind = eng
    check_search_at_scale(ida, oracle, kind, monkeypatch, dim, kind_, metric, s)


@pytest.mark.gpu
@pytest.mark.parametrize("s", [-58, 60])
def test_search_at_scale_768d_gpu(engine_loader, oracle, monkeypatch, s):
    """rows beyond the thin tile: one fat wave per SIMD, filtered at s = +60 and — the lattice step being out of range — not at -58"""
    check_search_at_scale(engine_loader("gpu"), oracle, "gpu", monkeypatch, 768, "lowrank", 0, s)


# ---- d. the exact build ------------------------------------------------------------------------------------------------------
BUILDS = [v for v in pc.BUILD_VARIANTS if v[1] in ({}, {"IDIST_BUILD_QUAD": "0", "IDIST_BUILD_FILTER": "1"},
                                                   {"IDIST_BUILD_QUAD": "0", "IDIST_BUILD_FILTER": "0"},
                                                   {"IDIST_BUILD_A2": "tile", "IDIST_BUILD_NO_FAST": "1"})]


@pytest.mark.parametrize("kind,n,dim,s", per_engine([(100, 300, -58), (100, 300, 60), (130, 16, -58), (130, 16, 60), (130, 16, 63)],
                                                   [(1500, 300, -58), (1500, 300, 60), (1500, 128, -58), (1500, 128, 60), (1500, 16, 63)]))
def test_exact_build_at_scale(engine_loader, oracle, kind, n, dim, s):
    """Sequential builds are the oracle's, byte for byte (layers and counters): the default (its selections on the MFMA Gram matrix,
    whose eps floor dominates everything at s = -58), descents with and without the reject filter (bound-form log entries), and
    the reference-order kernels."""
    ida = engine_loader(kind)
    assert len(BUILDS) == 4
    pc.check_build_exact(ida, oracle, n, dim, ef_construction=S(kind, 16, 100), seed=1000 + dim + s, variants=BUILDS, scale=s)


# ---- e. the brute force ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,s", [(300, -58), (300, 60), (16, -58), (16, 60), (16, 63)])
def test_bruteforce_at_scale(eng, oracle, monkeypatch, dim, s):
    """the scan kernel and the f32-MFMA filter + canonical re-rank against the oracle's brute force: the filter's floors
    (+ 1e-30f) and slack are absolute, the data is not"""
    ida, kind = eng
    rng = np.random.default_rng(400 + dim)
    n, nq, k = S(kind, 300, 20000), S(kind, 130, 600), 10
    pts = pc.gen_points(rng, n, dim, "uniform", s)
    q = pc.gen_points(rng, nq, dim, "uniform", s)
    q[:3] = pts[[5, 17, n - 1]]
    pc.use_test_build(monkeypatch)                     # (IDIST_BRUTEFORCE / IDIST_BF_SAMPLE exist in the test build only)
    h = empty_graph(ida, pts)
    op, od = oracle.bruteforce(pts, q, k, threads=S(kind, 4, 8))
    for path in ("scan", "mfma"):
        monkeypatch.setenv("IDIST_BRUTEFORCE", path)
        monkeypatch.setenv("IDIST_BF_SAMPLE", str(S(kind, 64, 4096)))
        p, d = h.bruteforce(q, k)
        assert np.array_equal(p, op) and np.array_equal(pc.bits(d), pc.bits(od)), path


# ---- f. the other metrics and the restricted search, one case each -----------------------------------------------------------
def test_dot_search_at_scale(eng, oracle):
    """METRIC_DOT at s = -58: the row norms are ~1e-33, the extra coordinate sqrt(S - s(x)) ~1e-16 beside coordinates of ~1e-18"""
    ida, kind = eng
    test_dot.check_dot_search(ida, oracle, kind, S(kind, 150, 4000), 300, S(kind, 12, 100), S(kind, 20, 600), scale=-58)


def test_search_allowed_at_scale(eng, oracle):
    """the ef ladder and the exact scan of a restricted search at s = -58, against test_allowed's model"""
    ida, kind = eng
    n, nq, ef, k = S(kind, (260, 12, 12, 5), (4000, 600, 16, 10))
    rng = np.random.default_rng(58)
    c = test_allowed.Case(oracle, pc.gen_points(rng, n, 300, "uniform", -58), pc.gen_points(rng, nq, 300, "uniform", -58), ef,
                          ef_construction=S(kind, 16, 100))
    h, srch = c.hnsw(ida), ida.Search()
    few = np.zeros(n, bool)
    few[rng.choice(n, (30 * n) // 260, replace=False)] = True
    most = rng.random(n) < 0.8
    want = c.model(few, k, max_rungs=1)                 # ef_search * |A| < k * n: no rung expects k hits — the exact scan
    assert np.all(want[3] == test_allowed.EXACT)
    test_allowed.check(h.search_allowed(c.q, few, k, srch, max_rungs=1, counters=True), want, "30 of 260")
    test_allowed.check(h.search_allowed(c.q, few, k, srch, counters=True), c.model(few, k), "30 of 260, the whole ladder")
    want = c.model(most, k)
    assert np.mean(want[3] == 0) > 0.5                  # answered by the first rung
    test_allowed.check(h.search_allowed(c.q, most, k, srch, counters=True), want, "four in five")


@pytest.mark.parametrize("s", [-40, 40])
def test_normalize_at_scale(eng, s):
    """cosine rows are normalised before the lattice is fitted: the scale is gone once normalize() is exact in it"""
    ida, kind = eng
    rng = np.random.default_rng(8)
    x = rng.standard_normal((S(kind, 21, 1003), 300)).astype(np.float32)
    assert np.array_equal(pc.bits(ida.normalize(np.ldexp(x, s).astype(np.float32))), pc.bits(ida.normalize(x)))
