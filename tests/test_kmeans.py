"""k-means on the GPU (idist_kmeans_assign / _update / idist_kmeans, idist_kmeans.hpp; include/idist.h has the definitions).  Assign is
checked exactly on integer-lattice data, where every f32 product and sum is exact, and within the derived product-form bound on float
data; update exactly on the lattice and within the bound its fixed summation order gives; idist_kmeans bit for bit against the loop
over the two steps.  Every case runs on the CPU emulator and (-m gpu) on the MI355X."""
import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params

U = 2.0 ** -24


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


def lattice(n, dim, k, seed=0):
    """integer rows and centroids in [-8, 8]; centroid 1 repeats centroid 0 and the last repeats the middle one (ties)"""
    rng = np.random.default_rng([n, dim, k, seed])
    x = rng.integers(-8, 9, (n, dim)).astype(np.float32)
    c = rng.integers(-8, 9, (k, dim)).astype(np.float32)
    if k > 1:
        c[1] = c[0]
        c[k - 1] = c[k // 2]
    return x, c


def d64(x, c):
    x, c = x.astype(np.float64), c.astype(np.float64)
    return ((x[:, None, :] - c[None, :, :]) ** 2).sum(axis=2)


# the 128-row tile edge, the 32-float K chunk edge, the accumulator boundary at 32 centroids, both centroid stagings (dim <= 160 / beyond)
ASSIGN_SHAPES = [(1, 1, 1), (127, 31, 2), (128, 32, 33), (129, 33, 64), (257, 100, 33), (257, 1, 64), (129, 100, 2), (130, 170, 40)]


# centroids staged per chunk (dim > 160) with both accumulators over six row tiles; both sides of the staging boundary (dim 160 with
# its 64 centroids resident, 161 not); k = 32 exactly (the second accumulator skipped) and k = 33, 17 beyond the boundary; one tiny
ASSIGN_SHAPES += [(700, 200, 64), (385, 161, 33), (300, 160, 64), (513, 192, 17), (260, 164, 32), (5, 5, 5)]


@pytest.mark.parametrize("n,dim,k", ASSIGN_SHAPES)
def test_assign_exact(eng, n, dim, k):
    ida, _ = eng
    x, c = lattice(n, dim, k)
    assign, counts = ida.kmeans_assign(x, c)
    want = d64(x, c).argmin(axis=1)                       # numpy's argmin: the first minimum, i.e. ties to the lower j
    assert np.array_equal(assign, want), (n, dim, k)
    assert np.array_equal(counts, np.bincount(want, minlength=k))


def test_assign_float(eng):
    """d64(x_i, c_a(i)) <= min_j d64(x_i, c_j) + 2 E_i, E_i = product_form_eps(K) (|x_i|^2 + max |c|^2) with K = dim rounded up to the
    chunk: each of the two compared d~ lies within E of its true value (idist_mfma.hpp).  The NaN row gets i mod k."""
    ida, _ = eng
    n, dim, k = 300, 300, 7
    rng = np.random.default_rng(5)
    x, c = rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((k, dim)).astype(np.float32)
    x[201, 17] = np.nan
    assign, counts = ida.kmeans_assign(x, c)
    assert assign[201] == 201 % k and counts.sum() == n
    fin = np.arange(n) != 201
    d = d64(x[fin], c)
    E = 4 * U * 320 * ((x[fin].astype(np.float64) ** 2).sum(axis=1) + (c.astype(np.float64) ** 2).sum(axis=1).max())
    got = d[np.arange(fin.sum()), assign[fin]]
    print("worst excess / bound:", ((got - d.min(axis=1)) / (2 * E)).max())
    assert np.all(got <= d.min(axis=1) + 2 * E)


def scan64(x, c):
    """include/idist.h's definition written out in f64 with IEEE inf and NaN: d~ = (|x|^2 + |c|^2) - 2 x.c, then the strict `<` scan
    from j = 0 — a NaN at j = 0 is never beaten, a NaN elsewhere never taken.  On the lattice every finite term is exact in f32 too."""
    x, c = x.astype(np.float64), c.astype(np.float64)
    with np.errstate(all="ignore"):
        d = ((x ** 2).sum(axis=1)[:, None] + (c ** 2).sum(axis=1)[None, :]) - 2.0 * (x[:, None, :] * c[None, :, :]).sum(axis=2)
    a, best = np.zeros(len(x), np.int64), d[:, 0].copy()
    for j in range(1, len(c)):
        m = d[:, j] < best
        a[m], best[m] = j, d[m, j]
    return a


@pytest.mark.parametrize("dim,k,j,value", [(40, 9, 0, np.nan), (40, 9, 3, np.nan), (40, 40, 35, np.nan), (200, 9, 3, np.inf),
                                           (40, 9, 0, np.inf), (40, 9, 0, -np.inf)])
def test_assign_nonfinite_centroid(eng, dim, k, j, value):
    """one coordinate of centroid j is NaN or infinite: its d~ is NaN wherever 0 * inf or inf - inf occurs and +inf elsewhere, the
    other centroids' are untouched.  At j = 0 the NaN rows stay with it; at j > 0 it receives nothing."""
    ida, _ = eng
    x, c = lattice(200, dim, k)
    if j:
        c[j] = x[7]                                       # while it is finite the centroid has a row of its own
    clean = scan64(x, c)
    assert np.array_equal(ida.kmeans_assign(x, c)[0], clean)
    c[j, 2] = value
    want = scan64(x, c)
    if j == 0:
        assert np.any(want != clean) and np.any(want == 0)
    else:
        assert not np.any(want == j) and np.any(clean == j)
    assign, counts = ida.kmeans_assign(x, c)
    assert np.array_equal(assign, want), (dim, k, j, value)
    assert np.array_equal(counts, np.bincount(want, minlength=k))


def test_overflowing_rows(eng):
    """a row whose |x|^2 overflows although every element is finite, and a row with -inf: both get i mod k, and the update counts
    them as members without summing them — the rest stays within test_update_float's bound (one chunk) and test_assign_float's"""
    ida, _ = eng
    n, dim, k = 130, 12, 7
    rng = np.random.default_rng(21)
    x, c = rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((k, dim)).astype(np.float32)
    x[5] *= np.float32(1e20)
    x[77, 4] = -np.inf
    assert np.all(np.isfinite(x[5])) and (x[5].astype(np.float64) ** 2).sum() > 2 * float(np.finfo(np.float32).max)
    assign, counts = ida.kmeans_assign(x, c)
    assert assign[5] == 5 % k and assign[77] == 77 % k
    assert counts.sum() == n and np.array_equal(counts, np.bincount(assign, minlength=k))
    ok = ~np.isin(np.arange(n), (5, 77))
    d = d64(x[ok], c)
    E = 4 * U * 32 * ((x[ok].astype(np.float64) ** 2).sum(axis=1) + (c.astype(np.float64) ** 2).sum(axis=1).max())
    assert np.all(d[np.arange(ok.sum()), assign[ok]] <= d.min(axis=1) + 2 * E)
    got, ucounts = ida.kmeans_update(x, assign, np.zeros((k, dim), np.float32))
    assert np.array_equal(ucounts, counts)
    for j in range(k):
        m = (assign == j) & ok
        assert m.any() and m.sum() == counts[j] - (j == 5 % k) - (j == 77 % k)
        xs = x[m].astype(np.float64)
        bound = (1024 + 1 + 2) * U * np.abs(xs).sum(axis=0) / m.sum()
        assert np.all(np.abs(got[j] - xs.sum(axis=0) / m.sum()) <= bound)


# ... and a column tile of 64 exactly full and one column over (dim 64, 65, 128, 129), n exactly one and two chunks, one row
@pytest.mark.parametrize("n,dim,k", [(129, 33, 5), (1025, 3, 4), (2100, 70, 64),
                                     (1024, 64, 64), (1025, 65, 64), (2048, 128, 7), (2049, 129, 33), (3, 1, 1)])
def test_update_exact(eng, n, dim, k):
    """lattice rows: the sums are exact, so the centroid is the one rounded division; n = chunk + 1 and three chunks; cluster k - 1 is
    empty (where k > 1) and keeps its centroid"""
    ida, _ = eng
    from instant_distance_amd import _capi

    assert _capi.KMEANS_CHUNK == 1024
    x, c = lattice(n, dim, k)
    assign = np.random.default_rng(n).integers(0, max(k - 1, 1), n).astype(np.uint32)
    got, counts = ida.kmeans_update(x, assign, c)
    want = c.copy()
    for j in range(max(k - 1, 1)):
        m = assign == j
        if m.any():
            want[j] = np.float32(x[m].astype(np.float64).sum(axis=0) / m.sum())
    assert np.array_equal(pc.bits(got), pc.bits(want)) and np.array_equal(counts, np.bincount(assign, minlength=k))


def test_update_float(eng):
    """|c - c64| <= (CHUNK + ceil(n / CHUNK) + 2) u sum|x| / count: a term passes through at most CHUNK additions inside its chunk and
    ceil(n / CHUNK) across them, the division and the conversion of the count add two roundings.  A row with an infinite norm is a
    member that is not summed."""
    ida, _ = eng
    n, dim, k = 2300, 20, 3
    rng = np.random.default_rng(9)
    x, c = rng.standard_normal((n, dim)).astype(np.float32), np.zeros((k, dim), np.float32)
    x[7, 3] = np.inf
    assign = rng.integers(0, k, n).astype(np.uint32)
    got, counts = ida.kmeans_update(x, assign, c)
    assert np.array_equal(counts, np.bincount(assign, minlength=k))
    ok = np.arange(n) != 7
    for j in range(k):
        m = (assign == j) & ok
        xs = x[m].astype(np.float64)
        bound = (1024 + 3 + 2) * U * np.abs(xs).sum(axis=0) / m.sum()
        assert np.all(np.abs(got[j] - xs.sum(axis=0) / m.sum()) <= bound)


def python_loop(ida, x, k, iters):
    n = len(x)
    c = x[(np.arange(k, dtype=np.uint64) * np.uint64(n) // np.uint64(k)).astype(np.int64)].copy()
    prev, run = None, 0
    for _ in range(iters):
        a, _ = ida.kmeans_assign(x, c)
        if prev is not None and np.array_equal(a, prev):
            break
        c, _ = ida.kmeans_update(x, a, c)
        prev, run = a, run + 1
    a, counts = ida.kmeans_assign(x, c)
    return c, a, counts, run


def blobs(n, dim, k, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((k, dim))[rng.integers(0, k, n)] * 4 + rng.standard_normal((n, dim))).astype(np.float32)


@pytest.mark.parametrize("n,dim,k,iters", [(1300, 12, 5, 20), (200, 40, 64, 2), (300, 8, 3, 0)])
def test_kmeans_is_the_loop(eng, n, dim, k, iters):
    """centroids, assign, counts and the number of updates, bit for bit; iters = 0 returns the initial rows: floor(j n / k)"""
    ida, _ = eng
    x = blobs(n, dim, k, n)
    cen, assign, counts, run = ida.kmeans(x, k, iters, return_iters=True)
    w_cen, w_assign, w_counts, w_run = python_loop(ida, x, k, iters)
    assert run == w_run and np.array_equal(pc.bits(cen), pc.bits(w_cen)) and np.array_equal(assign, w_assign) and np.array_equal(counts, w_counts)
    if iters == 0:
        assert np.array_equal(cen, x[[0, 100, 200]])
    else:
        assert 1 <= run <= iters


def test_grid_independence(eng, monkeypatch):
    """the same bytes at IDIST_CUS unset / 1 / 3 on the GPU (test build) and 256 under the emulator, as tests/test_cus_knob.py"""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    x = blobs(2500, 70, 9, 3)
    results = []
    for cus in (None, "1", "3") if kind == "gpu" else (None, "256"):
        if cus is None:
            monkeypatch.delenv("IDIST_CUS", raising=False)
        else:
            monkeypatch.setenv("IDIST_CUS", cus)
        cen, assign, counts = ida.kmeans(x, 9, 4)
        results.append(pc.bits(cen).tobytes() + assign.tobytes() + counts.tobytes())
        if cus is None:
            first = cen, assign, counts
    assert all(r == results[0] for r in results)
    # ... and the runs are anchored to a model: the assignment belongs to the centroids returned, within test_assign_float's bound
    cen, assign, counts = first
    again, acounts = ida.kmeans_assign(x, cen)
    assert np.array_equal(assign, again) and np.array_equal(counts, acounts) and np.array_equal(counts, np.bincount(assign, minlength=9))
    d = d64(x, cen)
    E = 4 * U * 96 * ((x.astype(np.float64) ** 2).sum(axis=1) + (cen.astype(np.float64) ** 2).sum(axis=1).max())
    assert np.all(d[np.arange(len(x)), assign] <= d.min(axis=1) + 2 * E)


def test_argument_errors(eng):
    ida, _ = eng
    x = np.zeros((10, 4), np.float32)
    for k in (0, 65, 11):
        with pytest.raises(ida.IdistError) as e:
            ida.kmeans(x, k)
        assert e.value.status == 1
    with pytest.raises(ida.IdistError):
        ida.kmeans_update(x, np.full(10, 3, np.uint32), x[:3])
