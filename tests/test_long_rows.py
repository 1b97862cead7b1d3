"""The product-form filters on long, structured rows.

Two filters decide what the canonical distance ever gets to see, both on |a|^2 + |b|^2 - 2 a.b with the sums accumulated in f32 over
the K stored floats of a row: the Gram filter of the build (build_select_mfma_kernel) and the filter of the wide-batch brute force
(mfma_dist_kernel / kth_threshold_kernel / rerank_kernel).  On random data the roundings of such a chain cancel and its error stays
near sqrt(K) u (u = 2^-24); on rows whose coordinates repeat they all go one way for as long as the partial sum stays in one binade,
and the error grows like K u: the worst case the margins are derived for (product_form_eps, idist_mfma.hpp).  The data here is built
to reach it.  With h = 2^(ceil(log2 K) - 25), half an ulp of the top binade of a sum of K terms of ~1:

  two levels   the queries are all ones; one group of points has every coordinate 1 + h (1 - 2^-6), the other 1 + h (1 + 2^-6).  In
               the top binade every step of q.p drops the first group's excess and doubles the second's: the nearer group looks
               farther by ~K h, the farther one nearer.  A threshold with a slack of 1e-4 (|q|^2 + max |p|^2), which the brute force
               had, returns the WRONG neighbours from K = 8192 on — no overflow, no error; the emulator and the MI355X alike
               (profiles/mfma_slack_ab.json)
  levels       parity_cases.gen_points(kind="levels"): every row one level 1 + h (1 + t), t in +-1/8, on both sides of the half ulp
  quantised    every coordinate drawn from a table of 16 such levels (de-quantised embeddings)
  translated   uniform data moved by +-4096 (|mean| >> spread): the norms dwarf the distances

Everything is compared with the oracle: ids with array_equal, distances as bit patterns.  Every case runs on the CPU emulator — which
models v_mfma_f32_32x32x2_f32 as a k-ordered fma chain — and (-m gpu) on the MI355X, at the same tiny shapes."""
import functools

import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params
from test_data_scale import check_filter_bound, empty_graph

SAMPLE = 64                       # IDIST_BF_SAMPLE: the threshold of a query comes from points 0 .. 63


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    return engine_loader(request.param), request.param


def both_paths(ida, h, monkeypatch, q, k, want, what=""):
    """the scan kernel and the MFMA filter + canonical re-rank, each against the oracle's (ids, distances)"""
    op, od = want
    monkeypatch.setenv("IDIST_BF_SAMPLE", str(SAMPLE))
    for path in ("scan", "mfma"):
        monkeypatch.setenv("IDIST_BRUTEFORCE", path)
        p, d = h.bruteforce(q, k)
        assert np.array_equal(p, op), (what, path, "ids", p[0], op[0], d[0], od[0])
        assert np.array_equal(pc.bits(d), pc.bits(od)), (what, path, "distance bits", d[0], od[0])


# ---- a. two levels -----------------------------------------------------------------------------------------------------------
def two_level_rows(K, n, mirror):
    """(points, queries, near, far): points 0 .. SAMPLE-1 at the farther level and the others at the nearer one — mirror: the other
    way round"""
    h = pc.half_ulp(K)
    near = np.float32(1.0 + h * (1.0 - 2.0 ** -6))
    far = np.float32(1.0 + h * (1.0 + 2.0 ** -6))
    assert float(near) == 1.0 + h * (1.0 - 2.0 ** -6) and float(far) == 1.0 + h * (1.0 + 2.0 ** -6)      # both exact in f32
    pts = np.empty((n, K), np.float32)
    pts[:SAMPLE] = near if mirror else far
    pts[SAMPLE:] = far if mirror else near
    return pts, np.ones((2, K), np.float32), near, far


def fma_chain(x, y, K):
    """sum of K equal terms x * y as an f32 fma chain: the product in f64 (exact), one f32 rounding per step.  The terms being equal,
    the order of the sum is irrelevant.  (x, y: arrays, one chain per element.)"""
    prod = np.asarray(x, np.float64) * np.asarray(y, np.float64)
    acc = np.zeros(prod.shape, np.float32)
    for _ in range(K):
        acc = (acc.astype(np.float64) + prod).astype(np.float32)       # (exact in f64: < 53 bits between the sum's top and the product's end)
    return acc


@functools.lru_cache(maxsize=None)
def product_form_error(K):
    """plain numpy: (|product form - f64 distance| of the nearer and of the farther group, 1e-4 (|q|^2 + max |p|^2))"""
    _, _, near, far = two_level_rows(K, SAMPLE + 1, False)
    lv = np.array([near, far], np.float32)
    one = np.ones(2, np.float32)
    qn, pn, dot = fma_chain(one, one, K), fma_chain(lv, lv, K), fma_chain(one, lv, K)
    assert qn[0] == K
    form = (qn + pn).astype(np.float32) - np.float32(2.0) * dot          # f32 throughout; not clamped at 0
    exact = K * (lv.astype(np.float64) - 1.0) ** 2
    assert exact[0] < exact[1]
    return np.abs(form.astype(np.float64) - exact), 1e-4 * (float(qn[0]) + float(pn.max()))


def check_two_level_inputs(K):
    """the data is as hard as it is meant to be: from K = 8192 both groups' product forms are off by more than the slack the brute
    force had (1.94 > 1.64 at 8192, 7.75 > 3.28 at 16384: the nearer group too large, the farther too small)"""
    err, old_slack = product_form_error(K)
    print(f"K {K}: product form off by {err[0]:.4g} (nearer group) and {err[1]:.4g} (farther), 1e-4 (|q|^2 + max |p|^2) = {old_slack:.4g}")
    if K >= 8192:
        assert err.min() > old_slack, (K, err, old_slack)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("mirror", [False, True], ids=["sample_farther", "sample_nearer"])
@pytest.mark.parametrize("K", [1024, 8192, 16384])
def test_bruteforce_on_two_level_rows(eng, oracle, monkeypatch, K, mirror, metric):
    """sample_farther: the sample looks nearer than it is and the true neighbours, all outside it, farther — a slack below twice the
    product form's error loses every one of them.  sample_nearer: the threshold errs the generous way; every point is a candidate
    (a longer list than this one would overflow into the scan fallback)."""
    ida, kind = eng
    n, k = 192, 10
    check_two_level_inputs(K)
    pts, q, _, _ = two_level_rows(K, n, mirror)
    want = oracle.bruteforce(pts, q, k, metric=metric)
    first = 0 if mirror else SAMPLE                                     # equal rows: the id decides
    assert np.array_equal(want[0], np.tile(np.arange(first, first + k, dtype=np.uint32), (2, 1)))
    assert mirror or want[0].min() >= SAMPLE                            # every true neighbour lies outside the sample
    pc.use_test_build(monkeypatch)                                      # (IDIST_BRUTEFORCE / IDIST_BF_SAMPLE exist in the test build only)
    h = empty_graph(ida, pts, metric)
    assert h.info().row_stride == K
    both_paths(ida, h, monkeypatch, q, k, want, f"K {K}")


def test_partitioned_bruteforce_on_two_level_rows(eng, oracle, monkeypatch):
    """PartitionedHnsw.bruteforce runs the same filter in every part: two parts of 144 points, each with its own farther sample"""
    ida, kind = eng
    K, k = 8192, 10
    check_two_level_inputs(K)
    part, q, _, _ = two_level_rows(K, 144, False)
    pts = np.concatenate([part, part])
    want = oracle.bruteforce(pts, q, k)
    assert np.array_equal(want[0], np.tile(np.arange(SAMPLE, SAMPLE + k, dtype=np.uint32), (2, 1)))
    pc.use_test_build(monkeypatch)
    ph = ida.PartitionedHnsw.from_hnsws([empty_graph(ida, part), empty_graph(ida, part)])
    both_paths(ida, ph, monkeypatch, q, k, want, "two parts")


# ---- b. a seeded sweep ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(16))
@pytest.mark.parametrize("K", [2048, 8192])
def test_bruteforce_on_constant_rows(eng, oracle, monkeypatch, K, seed):
    """every row and every query one level, repeated; the levels distinct and on both sides of the half ulp"""
    ida, kind = eng
    rng = np.random.default_rng(100 * K + seed)
    n, nq, k = (128 if K == 2048 else 192), 6, 10                       # (2048: there are 129 such levels)
    pts, q = pc.gen_points(rng, n, K, "levels"), pc.gen_points(rng, nq, K, "levels")
    lv = pts[:, 0].astype(np.float64) - 1.0
    assert np.all(pts == pts[:, :1]) and len(np.unique(lv)) == n
    h_ulp = pc.half_ulp(K)
    assert lv.min() >= 0.875 * h_ulp and lv.max() <= 1.125 * h_ulp and (lv < h_ulp).sum() > n // 4 and (lv > h_ulp).sum() > n // 4
    pc.use_test_build(monkeypatch)
    both_paths(ida, empty_graph(ida, pts), monkeypatch, q, k, oracle.bruteforce(pts, q, k), f"K {K} seed {seed}")


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("K", [2048, 8192])
def test_bruteforce_on_quantised_rows(eng, oracle, monkeypatch, K, seed):
    """every coordinate one of 16 levels: rows that are not constant, on data that still sits on a few values"""
    ida, kind = eng
    rng = np.random.default_rng(200 * K + seed)
    n, nq, k = 192, 6, 10
    table = pc.levels_table(rng, 16, K)
    pts, q = table[rng.integers(0, 16, size=(n, K))], table[rng.integers(0, 16, size=(nq, K))]
    pc.use_test_build(monkeypatch)
    both_paths(ida, empty_graph(ida, pts), monkeypatch, q, k, oracle.bruteforce(pts, q, k), f"K {K} seed {seed}")


# ---- c. far from the origin ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [4096.0, -4096.0])
def test_bruteforce_far_from_the_origin(eng, oracle, monkeypatch, offset):
    """300-d uniform data 4096 spreads away from the origin (as test_filter_bound_far_from_the_origin): the norms are ~5e9, the
    distances ~50, so the product form says next to nothing and the MFMA filter keeps every point.  At these sizes the lists hold them;
    a call may as well answer through the overflow fallback, and which route it took cannot be observed from outside: what is
    asserted is exactness, for both paths."""
    ida, kind = eng
    rng = np.random.default_rng(4096)
    n, nq, dim = 300, 6, 300
    pts = (pc.gen_points(rng, n, dim) + np.float32(offset)).astype(np.float32)
    q = (pc.gen_points(rng, nq, dim) + np.float32(offset)).astype(np.float32)
    q[0] = pts[n - 1]
    pc.use_test_build(monkeypatch)
    h = empty_graph(ida, pts)
    for k in (1, 10, 70):
        both_paths(ida, h, monkeypatch, q, k, oracle.bruteforce(pts, q, k), f"k {k}")


# ---- d. the Gram filter of the build ---------------------------------------------------------------------------------------------
GRAM_BUILDS = [v for v in pc.BUILD_VARIANTS if v[1] in ({}, {"IDIST_BUILD_A2": "tile", "IDIST_BUILD_NO_FAST": "1"}, {"IDIST_BUILD_A2": "tile"})]


def test_exact_build_on_constant_rows(eng, oracle):
    """2048-d, the longest rows of this family the build accepts (64 KiB of LDS per wave): the default build — its selections through
    the MFMA Gram matrix and eps = product_form_eps(K) (|ci|^2 + |cj|^2) — and the LDS-tile selections, in the reference's order and
    not, give the oracle's layers and counters"""
    ida, kind = eng
    assert len(GRAM_BUILDS) == 3
    pc.check_build_exact(ida, oracle, 120, 2048, kind="levels", ef_construction=16, seed=2048, variants=GRAM_BUILDS)


def test_levels_kind_leaves_the_other_kinds_alone():
    """gen_points: the new kind draws from its own branch only (first values of the existing kinds, as they were before it)"""
    def first(kind):
        return pc.gen_points(np.random.default_rng(7), 3, 5, kind)[0, :2]
    assert np.array_equal(pc.bits(first("uniform")), pc.bits(np.random.default_rng(7).random((3, 5), dtype=np.float32)[0, :2]))
    assert np.array_equal(first("grid"), np.random.default_rng(7).integers(0, 6, size=(3, 5)).astype(np.float32)[0, :2])
    lv = pc.gen_points(np.random.default_rng(7), 40, 2048, "levels")
    assert lv.dtype == np.float32 and lv.shape == (40, 2048) and lv.flags.c_contiguous and np.all(lv == lv[:, :1])
    assert len(np.unique(lv[:, 0])) == 40


# ---- e. the reject filter's bound ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ["constant", "jitter", "moved"])
@pytest.mark.parametrize("dim", [128, 300, 768, 1024, 1600])
def test_filter_bound_on_constant_rows(eng, oracle, dim, rows):
    """idist_filter_bound_batch never exceeds idist_distance_batch on constant rows, on constant rows with a jitter of 1e-4 and on
    constant rows moved by +1000 (where a geometry has no filter the bound is 0 and the check holds as well)"""
    ida, kind = eng
    rng = np.random.default_rng(dim)
    n, nq = 300, 6

    def data(m):
        x = pc.gen_points(rng, m, dim, "levels")
        if rows == "jitter":
            x = (x + np.float32(1e-4) * rng.standard_normal(x.shape).astype(np.float32)).astype(np.float32)
        if rows == "moved":
            x = (x + np.float32(1000.0)).astype(np.float32)
        return x

    check_filter_bound(ida, oracle, kind, data(n), data(nq), 0, tight=False)
