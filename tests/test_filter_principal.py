"""The reject filter's second table (csrc/idist_capi.hip filter_principal_ensure): 64-byte rows of 56 coordinates in
a principal basis, read by thin search walks of indexes whose sample says it pays.  Whatever the format — the policy's, or either one
forced through the test build's IDIST_FILTER_BASIS — ids, order, counts, distance bits and {n_dist, n_exp0, n_expU} are the oracle's;
the bound stays a bound; the choice is a function of the index alone."""
import os
import subprocess

import numpy as np
import pytest

import engines
import parity_cases as pc
from engines import engine_params
from test_filter import ON_CHIP, WALKS, S, _data

NONE, IDENTITY, PRINCIPAL = 0, 1, 2


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    return engine_loader(request.param), request.param


def data(rng, kind_, n, dim):
    if kind_ == "latent64":              # low rank, but more latent dimensions than the 56 a principal row keeps
        z = rng.standard_normal((n, 64)).astype(np.float32)
        a = rng.standard_normal((64, dim)).astype(np.float32)
        x = z @ a + 0.05 * rng.standard_normal((n, dim)).astype(np.float32)
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    if kind_ == "offset":                # centring: low-rank rows far from the origin
        return (pc.gen_points(rng, n, dim, "lowrank") + np.float32(7.0)).astype(np.float32)
    if kind_ == "nonfinite":
        a = pc.gen_points(rng, n, dim, "lowrank")
        for val in (np.nan, np.inf, -np.inf):
            rows = rng.choice(n, size=max(1, n // 25), replace=False)
            a[rows, rng.integers(0, dim, size=len(rows))] = val
        return a
    return _data(rng, kind_, n, dim)


def points_and_queries(rng, kind_, n, nq, dim, scale=0):
    """ONE draw, split: `gen_points(..., "lowrank")` draws its 8 x dim latent map per call, so queries drawn by a second call would lie
    in another subspace than the rows — queries from the data's own distribution are what a principal basis is made for."""
    a = pc.gen_points(rng, n + nq, dim, kind_, scale) if scale else data(rng, kind_, n + nq, dim)
    return np.ascontiguousarray(a[:n]), np.ascontiguousarray(a[n:])


def canon(a):
    """all NaNs are one value (x86 makes 0xFFC00000 out of inf - inf, the GPU stores 0x7FC00000); everything else bit for bit"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def check(got, want, nonfinite=False):
    if not nonfinite:
        return pc.check_search_result(got, want)
    assert np.array_equal(got.count, want.count) and np.array_equal(got.pid, want.pid)
    assert np.array_equal(canon(got.distance), canon(want.dist))
    assert np.array_equal(got.counters, want.counters)


CASES = [(300, "lowrank", 0, 0), (128, "lowrank", 1, 0), (200, "lowrank", 0, 0), (300, "latent64", 1, 0), (300, "offset", 0, 0),
         (300, "outliers", 1, 0), (128, "constant", 0, 0), (128, "grid", 0, 0), (300, "nonfinite", 0, 0), (300, "lowrank", 1, 40)]


@pytest.mark.parametrize("dim,kind_,metric,n_fixed", CASES)
def test_same_answers_in_either_format(eng, oracle, monkeypatch, dim, kind_, metric, n_fixed):
    """n_fixed = 40: fewer rows than the basis has directions."""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    rng = np.random.default_rng(3000 + dim + metric)
    n, ef = n_fixed or S(kind, 260, 20000), 12 if n_fixed else S(kind, 12, 100)    # (`nearest` must fill up for the filter to start)
    pts, q = points_and_queries(rng, kind_, n, S(kind, 12, 600), dim)
    q[0] = pts[n // 2]                                                  # a stored point
    q[1] = pts[1] * np.float32(3.0) + np.float32(11.0)                  # far outside the lattice
    cfg = oracle.default_config(metric=metric, ef_search=ef, ef_construction=S(kind, 16, 100))
    oix = oracle.Index.build(pts, cfg, threads=S(kind, 1, 8))
    want = oix.search(q, threads=S(kind, 1, 8))
    h = ida.Hnsw.from_parts(pts, oix.zero, oix.layers, ida.Builder().metric(metric).ef_search(ef))
    total = {"principal": [0, 0], "identity": [0, 0]}
    on_principal_rows = [0, 0]              # of total["principal"]: what the walks read from the 64-byte rows themselves
    for name, env in WALKS:
        for basis, flt in (("principal", "1"), ("identity", "1"), ("principal", "0")):
            with pc.search_variant(env), monkeypatch.context() as m:
                m.setenv("IDIST_FILTER", flt)
                m.setenv("IDIST_FILTER_BASIS", basis)
                srch = ida.Search()
                got = h.search_batch(q, srch, counters=True)
                seen, rejected = srch.filter_counts()
                p_seen, p_rejected = srch.filter_principal_counts()
            check(got, want, kind_ == "nonfinite")
            assert p_seen <= seen and p_rejected <= rejected and p_rejected <= p_seen
            if basis == "identity":
                assert (p_seen, p_rejected) == (0, 0), name
            elif flt == "1":
                on_principal_rows[0] += p_seen
                on_principal_rows[1] += p_rejected
            if flt == "0":
                assert seen == 0, name
            else:
                total[basis][0] += seen
                total[basis][1] += rejected
                assert rejected <= seen
                # (NaN distances all tie: a walk whose tie region overflows is run again with a larger one, and the filter's counts
                #  include the abandoned pass while the work counters are the final pass's)
                assert kind_ == "nonfinite" or seen <= int(want.counters[:, 0].sum())
    info = h.info()
    assert info.filter_bytes == n * ((info.row_stride + 8 + 63) // 64 * 64) and info.filter_principal_bytes == n * 64
    assert info.filter_format in (IDENTITY, PRINCIPAL)
    if kind_ == "constant":
        assert total["principal"][1] == 0 and total["identity"][1] == 0     # every distance is 0: nothing can be rejected
    elif not n_fixed:                       # (40 rows: the zero layer is complete, the entry's expansion visits everything before `nearest` is full)
        assert total["principal"][0] > 0 and total["identity"][0] > 0
    if kind_ == "lowrank" and not n_fixed:
        assert total["principal"][1] > 0.3 * total["principal"][0], total   # test_filter.py's own floor, principal format forced
        # ... and it is the principal rows that do it: the queries come from the rows' distribution (all but q[1], the far one), so
        # their walks read the 64-byte table, and the floor holds on that table alone
        assert on_principal_rows[0] > 0.75 * total["principal"][0], (on_principal_rows, total)
        assert on_principal_rows[1] > 0.3 * on_principal_rows[0], on_principal_rows


BOUND_CASES = [(300, "lowrank", 0), (128, "uniform", 1), (300, "outliers", 0), (200, "offset", 1), (128, "grid", 0), (300, "nonfinite", 0),
               (496, "lowrank", 0)]


@pytest.mark.parametrize("dim,kind_,metric", BOUND_CASES)
def test_principal_bound_never_exceeds_the_canonical_distance(eng, oracle, monkeypatch, dim, kind_, metric):
    """test_filter.py's bound test on the eligible geometries among its data kinds, principal format forced."""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    monkeypatch.setenv("IDIST_FILTER_BASIS", "principal")
    rng = np.random.default_rng(177 + dim)
    n, nq, n_ids = S(kind, 300, 20000), S(kind, 6, 64), S(kind, 70, 2000)
    base = "lowrank" if kind_ == "nonfinite" else kind_
    pts, q = points_and_queries(rng, base, n, nq, dim)
    q[1] = q[1] * np.float32(5.0) - np.float32(3.0)                       # far outside the lattice
    mean = pts.mean(axis=0, dtype=np.float64)
    q[4] = (mean + 5.0 * (pts[7] - mean)).astype(np.float32)              # far outside the lattice but INSIDE the basis' span: clamped there
    if kind_ == "nonfinite":
        pts[rng.choice(n, 6, replace=False), rng.integers(0, dim, 6)] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf]
        q[2, 3], q[3, 0] = np.nan, np.inf
    zero = np.full((n, 64), pc.INVALID, dtype=np.uint32)
    h = ida.Hnsw.from_parts(pts, zero, [], ida.Builder().metric(metric))
    ids = rng.integers(0, n, size=(nq, n_ids)).astype(np.uint32)
    ids[0, 1] = pc.INVALID
    ids[2, :4] = [0, 1, 2, 3]
    bound = h.filter_bounds(q, ids)
    assert h.info().filter_principal_bytes == n * 64                      # (the bound came from the principal rows)
    dist = h.distances(q, ids)
    assert np.all(np.isfinite(bound)) and np.all(bound >= 0)
    ok = ~np.isnan(dist)
    assert np.all(bound[ok] <= dist[ok]), float(np.max(bound[ok] - dist[ok]))
    assert bound[0, 1] == 0
    monkeypatch.setenv("IDIST_FILTER_BASIS", "identity")
    other = h.filter_bounds(q, ids)
    assert np.all(other[ok] <= dist[ok]) and not np.array_equal(other, bound)
    if base == "lowrank":
        # the in-distribution queries (5 on) and the far one inside the span (4) got their bounds from the principal rows: they differ
        # from the identity rows' almost everywhere (a query the basis does not fit would get the identity bound, bit for bit)
        live = ok[4:] & (ids[4:] != pc.INVALID)
        assert np.mean((other[4:] != bound[4:])[live]) > 0.9
        assert np.mean(other[4] != bound[4]) > 0.9
    if kind_ == "lowrank" and dim == 300:
        body = bound[5:] / np.maximum(dist[5:], np.float32(1e-30))
        assert np.median(body) > 0.8, float(np.median(body))


def _format_after_a_search(ida, pts, zero, layers, ef=20, metric=0):
    h = ida.Hnsw.from_parts(pts, zero, layers, ida.Builder().metric(metric).ef_search(ef))
    assert h.info().filter_format == NONE                                 # the tables are made on first use
    q = pts[:: max(1, len(pts) // 8)][:8].copy()
    with pc.search_variant(ON_CHIP):
        srch = ida.Search()
        got = h.search_batch(q, srch)
        seen, _ = srch.filter_counts()
    return h, got, seen


def test_policy_is_a_function_of_the_index(eng, oracle, monkeypatch):
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    monkeypatch.delenv("IDIST_FILTER_BASIS", raising=False)
    rng = np.random.default_rng(9)
    n = S(kind, 300, 20000)
    empty = lambda rows: np.full((rows, 64), pc.INVALID, dtype=np.uint32)   # noqa: E731  (format and policy need no graph)
    low = pc.gen_points(rng, n, 300, "lowrank")
    h, _, seen = _format_after_a_search(ida, low, empty(n), [])
    info = h.info()
    assert info.filter_format == PRINCIPAL and info.filter_principal_bytes == n * 64 and info.filter_bytes == n * 320
    h2, _, _ = _format_after_a_search(ida, low, empty(n), [])
    assert h2.info().filter_format == PRINCIPAL                           # the same points, the same choice
    hu, _, _ = _format_after_a_search(ida, pc.gen_points(rng, n, 300, "uniform"), empty(n), [])
    info = hu.info()
    assert info.filter_format == IDENTITY and info.filter_principal_bytes == 0 and info.filter_bytes == n * 320   # turned down: freed
    # a forced format that cannot be served is an error: the uniform index freed its principal table before the knob was set
    from instant_distance_amd import _capi
    monkeypatch.setenv("IDIST_FILTER_BASIS", "principal")
    with pc.search_variant(ON_CHIP), pytest.raises(_capi.IdistError):
        hu.search_batch(low[:8].copy(), ida.Search())
    monkeypatch.delenv("IDIST_FILTER_BASIS")
    for dim in (64, 768):                                                 # ineligible geometries: short rows, the fat walk
        m = S(kind, 120, 3000)
        hi, _, _ = _format_after_a_search(ida, pc.gen_points(rng, m, dim, "lowrank"), empty(m), [])
        info = hi.info()
        assert info.filter_format == IDENTITY and info.filter_principal_bytes == 0, dim


def test_import_and_replica_answer_identically(eng, oracle, monkeypatch):
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    monkeypatch.delenv("IDIST_FILTER_BASIS", raising=False)
    rng = np.random.default_rng(10)
    n, ef = S(kind, 260, 20000), S(kind, 12, 100)
    pts, q = points_and_queries(rng, "lowrank", n, S(kind, 12, 600), 300)
    cfg = oracle.default_config(ef_search=ef, ef_construction=S(kind, 16, 100))
    oix = oracle.Index.build(pts, cfg, threads=S(kind, 1, 8))
    want = oix.search(q, threads=S(kind, 1, 8))
    h = ida.Hnsw.from_parts(pts, oix.zero, oix.layers, ida.Builder().ef_search(ef))
    rep = h.replicate([0])[0]
    out = []
    for x in (h, rep):
        with pc.search_variant(ON_CHIP):
            srch = ida.Search()
            got = x.search_batch(q, srch, counters=True)
            out.append(srch.filter_counts() + srch.filter_principal_counts())
        pc.check_search_result(got, want)
        assert x.info().filter_format == PRINCIPAL
    assert out[0] == out[1] and out[0][1] > 0.3 * out[0][0], out          # the same table, bit for bit: the same rejections
    assert out[0][2] >= 0.99 * out[0][0] and out[0][3] >= 0.99 * out[0][1], out   # ... on the principal rows (in-distribution queries: all but
                                                                                   #     the odd one beyond twice the rows' 99th percentile)


@pytest.mark.parametrize("s,available", [(-40, True), (60, True), (-50, False)])
def test_principal_format_at_scale(eng, oracle, monkeypatch, s, available):
    """Coordinates times 2^s: inside the lattice's step range [2^-58, 2^60] the principal rows serve and the answers are the oracle's;
    beyond it (2^-50: a step of ~2^-64) the index has no compact rows at all and the answers are still the oracle's."""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    monkeypatch.setenv("IDIST_FILTER_BASIS", "principal")
    rng = np.random.default_rng(500 + s)
    n, ef = S(kind, 260, 20000), S(kind, 12, 100)
    pts, q = points_and_queries(rng, "lowrank", n, S(kind, 12, 600), 300, s)
    q[0] = pts[n // 2]
    cfg = oracle.default_config(ef_search=ef, ef_construction=S(kind, 16, 100))
    oix = oracle.Index.build(pts, cfg, threads=S(kind, 1, 8))
    want = oix.search(q, threads=S(kind, 1, 8))
    h = ida.Hnsw.from_parts(pts, oix.zero, oix.layers, ida.Builder().ef_search(ef))
    with pc.search_variant(ON_CHIP):
        srch = ida.Search()
        got = h.search_batch(q, srch, counters=True)
        seen, rejected = srch.filter_counts()
    pc.check_search_result(got, want)
    info = h.info()
    if available:
        assert info.filter_principal_bytes == n * 64 and rejected > 0.3 * seen > 0, (seen, rejected)
    else:
        assert info.filter_format == NONE and info.filter_principal_bytes == 0 and seen == 0


def test_basis_routine_alone(tmp_path):
    """tests/host/basis.cpp links the basis routine alone (csrc/idist_basis.hpp, host code): on a 2048 x 300 low-rank sample, the same
    with non-finite entries, a constant sample, a 20-row sample and extreme scales, |B B^T - I|_inf <= 1e-6 after the rounding to
    f32, s >= 1 bounds the largest singular value, and two calls agree bit for bit."""
    exe = str(tmp_path / "basis")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(engines.ROOT, "tests", "host", "basis.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "basis ok" in out.stdout, out.stdout + out.stderr
