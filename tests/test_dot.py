"""Inner product (IDIST_METRIC_DOT, include/idist.h).

A DOT index over rows X of `dim` coordinates is DEFINED as the squared-L2 index over the rows X~ of kdim = dim + 1 coordinates:
s(x) = the canonical squared-L2 distance of x to the origin over its dim coordinates, S = the given bound or the largest finite
s, x~ = (x, sqrtf(S - s(x))) (0 for rows whose s is NaN / inf), searched with q~ = (q, 0), and every distance d is reported as
0.5f * (d - (s(q) + S)).  So everything here but section 7 is exact: expected values come from numpy and the oracle's L2SQ paths
over X~ — never from the code under test; ids, counts and counters are compared with array_equal, rows and distances as bit
patterns.  Section 7 checks the MEANING (largest float64 inner product) within a derived tolerance.  Every case runs on the CPU
emulator and (-m gpu) on the MI355X."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params
from test_cosine import DIMS, DeviceMem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 0xFFFFFFFF
INF_BITS = 0x7F800000
HALF = np.float32(0.5)


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


def S(kind, emu, gpu):
    return gpu if kind == "gpu" else emu


# ---- the definition, restated in numpy ----------------------------------------------------------------------------------
def np_norms(oracle, x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    origin = np.zeros(x.shape[1], dtype=np.float32)
    return np.array([oracle.distance(row, origin, 0) for row in x], dtype=np.float32)


def np_augment(oracle, x, bound=0.0):
    """steps 1-4: (x~ [n, dim + 1], S, s)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    s = np_norms(oracle, x)
    fin = np.isfinite(s)
    if bound > 0:
        Sb = np.float32(bound)
    else:
        Sb = s[fin].max() if fin.any() else np.float32(0.0)
    e = np.zeros(len(x), dtype=np.float32)
    diff = Sb - s[fin]
    assert diff.dtype == np.float32 and np.all(diff >= 0)
    e[fin] = np.sqrt(diff)
    out = np.concatenate([x, e[:, None]], axis=1)
    assert out.dtype == np.float32
    return np.ascontiguousarray(out), np.float32(Sb), s


def np_queries(q):
    q = np.ascontiguousarray(q, dtype=np.float32)
    return np.ascontiguousarray(np.concatenate([q, np.zeros((len(q), 1), np.float32)], axis=1))


def reported(d, sq, Sb):
    """step 6 as bit patterns: d [nq, w] canonical L2SQ distances, sq [nq] = s(q)"""
    d = np.ascontiguousarray(d, dtype=np.float32)
    t = (np.asarray(sq, np.float32) + np.float32(Sb)).astype(np.float32)
    with np.errstate(all="ignore"):
        r = HALF * (d - t[:, None])
    assert r.dtype == np.float32
    keep = np.isnan(d) | np.isposinf(d)
    return pc.bits(np.where(keep, d, r))


def scaled_rows(rng, n, dim, kind="normal"):
    """rows whose lengths spread over 2^-3 .. 2^3"""
    x = rng.standard_normal((n, dim)).astype(np.float32) if kind == "normal" else pc.gen_points(rng, n, dim)
    return np.ascontiguousarray(x * np.exp2(rng.uniform(-3, 3, size=(n, 1))).astype(np.float32))


def dot_builder(ida, ef=100):
    return ida.Builder().metric(ida.METRIC_DOT).ef_search(ef)


def f32_bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


# ---- 1. the augmentation alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_augment_kernel(eng, oracle, dim):
    ida, kind = eng
    from instant_distance_amd import _capi

    rng = np.random.default_rng(200 + dim)
    n = S(kind, 21, 1003)                       # not a multiple of the eight rows a wave takes at a time
    x = scaled_rows(rng, n, dim)
    keep = x.copy()
    want, want_S, want_s = np_augment(oracle, x)
    got, got_S, s = ida.augment_dot(x, return_norm2=True)
    assert np.array_equal(x, keep)
    assert got.shape == (n, dim + 1) and got.dtype == np.float32
    assert np.array_equal(pc.bits(s), pc.bits(want_s))
    assert f32_bits(got_S) == f32_bits(want_S) == int(pc.bits(want_s).max())
    assert np.array_equal(pc.bits(got), pc.bits(want))
    assert (got[:, dim] == 0).sum() >= 1 and got[np.argmax(want_s), dim] == 0       # the maximal row: e = 0
    rows_only, S_only = ida.augment_dot(x)
    assert np.array_equal(pc.bits(rows_only), pc.bits(want)) and f32_bits(S_only) == f32_bits(want_S)
    # a given bound above the maximum
    big = np.float32(want_S) * np.float32(2.5) + np.float32(1.0)
    want2, want2_S, _ = np_augment(oracle, x, big)
    got2, got2_S = ida.augment_dot(x, bound=big)
    assert f32_bits(got2_S) == f32_bits(big) == f32_bits(want2_S)
    assert np.array_equal(pc.bits(got2), pc.bits(want2)) and np.all(got2[:, dim] > 0)
    # the maximum itself is a valid bound and gives the derived rows
    got3, got3_S = ida.augment_dot(x, bound=want_S)
    assert np.array_equal(pc.bits(got3), pc.bits(want)) and f32_bits(got3_S) == f32_bits(want_S)
    # out_rows NULL: only the norms and the bound
    L, f = _capi.lib(), _capi.f32p
    s2, Sc = np.zeros(n, np.float32), C.c_float(-1.0)
    L.check(L.idist_dot_augment_batch(f(x), n, dim, 0.0, None, f(s2), C.byref(Sc), 0))
    assert np.array_equal(pc.bits(s2), pc.bits(want_s)) and f32_bits(Sc.value) == f32_bits(want_S)
    Sc = C.c_float(-1.0)
    L.check(L.idist_dot_augment_batch(f(x), n, dim, 0.0, None, None, C.byref(Sc), 0))
    assert f32_bits(Sc.value) == f32_bits(want_S)
    assert np.array_equal(x, keep)


@pytest.mark.parametrize("dim", [5, 300])
def test_augment_kernel_past_the_grid(eng, oracle, dim):
    """more rows than the waves of dot_norms_kernel take in one trip (eight each); at dim 300 on the GPU also more elements than the
    lanes of dot_augment_rows_kernel's grid.  1009 distinct rows, row i of the batch = row i % 1009, the model over the 1009 (the
    bound S is the maximum over them); the bit rule of test_augment_kernel"""
    # caps: min(ceil(n / 8), n_cu * 32) waves of eight rows, launch_dot_norms; min(ceil(n * stride / 256), 65536) workgroups of 256
    # elements, dot_augment_device (idist_capi.hip)
    from engines import cu_count
    ida, kind = eng
    m = 1009
    n = 8 * cu_count(kind) * 32 + 37
    rng = np.random.default_rng(250 + dim)
    base = scaled_rows(rng, m, dim)
    rows = np.arange(n) % m
    if kind == "emu":                           # (fewer rows than the 1009: the model over the rows that are there)
        base, rows = np.ascontiguousarray(base[:n]), np.arange(n)
    x = np.ascontiguousarray(base[rows])
    want, want_S, want_s = np_augment(oracle, base)
    got, got_S, s = ida.augment_dot(x, return_norm2=True)
    assert got.shape == (n, dim + 1) and f32_bits(got_S) == f32_bits(want_S)
    assert np.array_equal(pc.bits(s), pc.bits(want_s[rows]))
    assert np.array_equal(pc.bits(got), pc.bits(want[rows]))


@pytest.mark.parametrize("dim", [1, 5, 12, 300])
def test_augment_special_rows(eng, oracle, dim):
    """a zero row, a NaN row, inf rows, a row whose s overflows, denormals whose s underflows, and the maximal row"""
    ida, kind = eng
    rng = np.random.default_rng(17 + dim)
    x = rng.standard_normal((13, dim)).astype(np.float32)
    x[1] = 0.0
    x[3, dim // 2] = np.nan
    x[4, dim - 1] = np.inf
    x[6] = np.float32(3.0e19) * np.sign(x[6])                               # s = dim * 9e38 > f32 max
    x[8] = np.float32(1.0e-39) * x[8]                                       # every square underflows to 0
    x[9, 0] = -np.inf
    x[11] = np.float32(64.0) * np.sign(x[11])                               # the maximal finite row
    keep = x.copy()
    want, want_S, want_s = np_augment(oracle, x)
    got, got_S, s = ida.augment_dot(x, return_norm2=True)
    assert np.array_equal(pc.bits(x), pc.bits(keep))
    nan = np.isnan(want_s)
    assert list(np.flatnonzero(nan)) == [3] and np.array_equal(np.isnan(s), nan)
    assert np.array_equal(pc.bits(s[~nan]), pc.bits(want_s[~nan]))
    assert np.isposinf(s[[4, 6, 9]]).all() and s[1] == 0 and s[8] == 0
    assert f32_bits(got_S) == f32_bits(want_S) == f32_bits(want_s[11])       # NaN / inf rows do not enter the bound
    assert np.array_equal(pc.bits(got), pc.bits(want))
    assert np.all(got[[3, 4, 6, 9, 11], dim] == 0)                           # not finite: e = 0; the maximal row: e = 0
    assert f32_bits(got[1, dim]) == f32_bits(np.sqrt(np.float32(want_S))) == f32_bits(got[8, dim])
    # nothing finite at all: S = 0
    bad = x[[3, 4, 6, 9]]
    g, Sb = ida.augment_dot(bad)
    assert f32_bits(Sb) == 0 and np.all(g[:, dim] == 0) and np.array_equal(pc.bits(g[:, :dim]), pc.bits(bad))


def test_augment_refusals(eng, oracle):
    ida, kind = eng
    from instant_distance_amd import _capi

    rng = np.random.default_rng(3)
    x = scaled_rows(rng, 37, 9)
    s = np_norms(oracle, x)
    worst = int(np.argmax(s))
    below = np.nextafter(s[worst], np.float32(0.0))
    with pytest.raises(ida.IdistError) as e:
        ida.augment_dot(x, bound=below)                                      # one ulp too small
    assert e.value.status == 1 and f"row {worst}" in e.value.message
    for bad in (np.inf, np.nan, -1.0, -np.inf):
        with pytest.raises(ida.IdistError) as e:
            ida.augment_dot(x, bound=bad)
        assert e.value.status == 1
    # an inf row does not make a bound too small
    y = x.copy()
    y[5, 2] = np.inf
    rows, Sb = ida.augment_dot(y, bound=s[worst])
    assert f32_bits(Sb) == f32_bits(s[worst]) and rows[5, 9] == 0
    L, f = _capi.lib(), _capi.f32p
    out = np.zeros((37, 10), np.float32)
    assert L.idist_dot_augment_batch(f(x), 37, 0, 0.0, f(out), None, None, 0) == 1
    assert L.idist_dot_augment_batch(f(x), 37, 65536, 0.0, None, None, None, 0) == 1
    assert L.idist_dot_augment_batch(None, 37, 9, 0.0, f(out), None, None, 0) == 1
    Sc = C.c_float(-1.0)
    assert L.idist_dot_augment_batch(f(x), 0, 9, 0.0, f(out), None, C.byref(Sc), 0) == 0 and Sc.value == 0.0   # n = 0
    r0, S0 = ida.augment_dot(np.zeros((0, 5), np.float32))
    assert r0.shape == (0, 6) and S0 == 0


# ---- 2. import and search -----------------------------------------------------------------------------------------------
_GRAPHS = {}


def dot_graph(oracle, n, dim, seed=11, scale=0):
    """raw rows (times 2^scale), x~, S and the oracle's L2SQ graph over x~ (cached: ef_search does not enter a build)"""
    key = (n, dim, seed, scale)
    if key not in _GRAPHS:
        rng = np.random.default_rng(seed)
        x = np.ldexp(scaled_rows(rng, n, dim, "uniform"), scale).astype(np.float32)
        xa, Sb, _ = np_augment(oracle, x)
        o = oracle.Index.build(xa, oracle.default_config(metric=0), threads=8 if n > 1000 else 1)
        _GRAPHS.clear()
        _GRAPHS[key] = (x, xa, Sb, o.zero, o.layers)
    return _GRAPHS[key]


def check_dot_search(ida, oracle, kind, n, dim, ef, wide, scale=0):
    x, xa, Sb, zero, layers = dot_graph(oracle, n, dim, scale=scale)
    oix = oracle.Index.from_arrays(xa, zero, layers, oracle.default_config(metric=0, ef_search=ef))
    h = ida.Hnsw.from_parts(x, zero, layers, dot_builder(ida, ef))          # raw rows: the import augments
    info = h.info()
    assert info.metric == ida.METRIC_DOT == 4 and info.dim == dim and f32_bits(info.dot_bound) == f32_bits(Sb)
    rng = np.random.default_rng(1000 * dim + ef)
    search = ida.Search()
    for nq in (7, wide, 1):
        q = np.ldexp(scaled_rows(rng, nq, dim, "uniform"), scale).astype(np.float32)
        if nq > 2:
            q[1] = x[min(5, n - 1)] * np.float32(4.0)
        keep = q.copy()
        want = oix.search(np_queries(q), threads=8)
        search.filter_counts()                                               # reset
        got = h.search_batch(q, search, counters=True)
        assert np.array_equal(q, keep)
        assert np.array_equal(got.count, want.count)
        assert np.array_equal(got.pid, want.pid)
        assert np.array_equal(got.counters, want.counters)
        assert np.array_equal(pc.bits(got.distance), reported(want.dist, np_norms(oracle, q), Sb))
        # nearest first still holds for what is reported
        c = int(got.count[0])
        assert np.all(np.diff(got.distance[0, :c]) >= 0)
        if kind == "gpu" and nq >= 1024 and n >= 20000:
            examined, rejected = search.filter_counts()
            print(f"dim {dim} ef {ef} nq {nq}: filter examined {examined}, rejected {rejected} "
                  f"({100.0 * rejected / max(examined, 1):.1f} %)")
            assert examined > 0                                              # the filtered wide walk is the kernel that ran
    return h


@pytest.mark.parametrize("ef", [100, 37])
@pytest.mark.parametrize("dim", [300, 127])
def test_search_parity(eng, oracle, dim, ef):
    """300-d rows (kdim 301: a runtime geometry) and 127-d rows (kdim 128: a compiled one).  On the GPU the wide batch has to run
    the filtered wide walk: long rows take it at every size, 512-byte rows once the rows outgrow the L2's reach (32 MB: 65536 rows —
    launch_search's policy), hence the 70000."""
    ida, kind = eng
    check_dot_search(ida, oracle, kind, S(kind, 150, 20000 if dim == 300 else 70000), dim, ef, S(kind, 20, 2048))


def test_search_device_pointers(eng, oracle):
    """idist_search_batch_device: the caller's dim-wide device queries are read, never written; results as the host-pointer call's"""
    ida, kind = eng
    n, dim, ef, nq = S(kind, 150, 20000), 127, 37, S(kind, 9, 600)
    x, xa, Sb, zero, layers = dot_graph(oracle, n, dim)
    oix = oracle.Index.from_arrays(xa, zero, layers, oracle.default_config(metric=0, ef_search=ef))
    h = ida.Hnsw.from_parts(x, zero, layers, dot_builder(ida, ef))
    q = scaled_rows(np.random.default_rng(5), nq, dim, "uniform")
    want = oix.search(np_queries(q), threads=8)
    mem = DeviceMem(kind)
    try:
        o_pid, o_dist = np.zeros((nq, ef), np.uint32), np.zeros((nq, ef), np.float32)
        o_cnt, o_ctr = np.zeros(nq, np.uint32), np.zeros((nq, 3), np.uint32)
        d_q = mem.up(q.copy())
        d = [mem.up(a) for a in (o_pid, o_dist, o_cnt, o_ctr)]
        s = ida.Search()
        h.search_batch_device(s, d_q, nq, d[0], d[1], d[2], d[3])
        got = [mem.down(p, like).copy() for p, like in zip(d, (o_pid, o_dist, o_cnt, o_ctr))]
        s.check_status()
        assert np.array_equal(pc.bits(mem.down(d_q, q)), pc.bits(q))
    finally:
        mem.free()
    assert np.array_equal(got[0], want.pid) and np.array_equal(got[2], want.count) and np.array_equal(got[3], want.counters)
    assert np.array_equal(pc.bits(got[1]), reported(want.dist, np_norms(oracle, q), Sb))


# ---- 3. build -----------------------------------------------------------------------------------------------------------
def test_build_parity(eng, oracle):
    ida, kind = eng
    n, dim, seed = S(kind, 200, 6000), S(kind, 6, 32), 4321
    rng = np.random.default_rng(8)
    x = scaled_rows(rng, n, dim)
    keep = x.copy()
    b = ida.Builder().metric(ida.METRIC_DOT).max_batch(1).seed(seed)
    h, ids = b.build_hnsw(x)
    assert np.array_equal(pc.bits(x), pc.bits(keep))
    out_pid, order = oracle.permutation(seed, n)
    assert ids == [int(p) for p in out_pid]
    raw = np.ascontiguousarray(x[order])
    xa, Sb, _ = np_augment(oracle, raw)                                     # S is a maximum: the shuffle does not change it
    oix = oracle.Index.build(xa, oracle.default_config(metric=0), threads=1)
    zero, layers = h.into_parts()
    assert np.array_equal(zero, oix.zero) and len(layers) == len(oix.layers)
    assert all(np.array_equal(a, o) for a, o in zip(layers, oix.layers))
    st = h.build_stats()
    assert st.n_dist == oix.build_counters.n_dist
    assert st.n_exp0 == oix.build_counters.n_exp0 and st.n_expU == oix.build_counters.n_expU
    assert h.info().dim == dim and f32_bits(h.info().dot_bound) == f32_bits(Sb)
    # the host copies are the caller's dim-wide rows
    assert h.points.shape == (n, dim)
    assert all(np.array_equal(pc.bits(h[ids[i]]), pc.bits(x[i])) for i in range(0, n, max(1, n // 40)))
    q = scaled_rows(rng, 1, dim)[0]
    items = list(h.search(q, ida.Search()))
    want = oix.search(np_queries(q[None, :]))
    assert [it.pid for it in items] == list(want.pid[0, : want.count[0]])
    assert all(np.array_equal(pc.bits(it.point), pc.bits(raw[it.pid])) for it in items)
    assert np.array_equal(pc.bits(np.array([it.distance for it in items], np.float32)),
                          reported(want.dist[:, : want.count[0]], np_norms(oracle, q[None, :]), Sb)[0])
    # a given bound: the same build over the rows augmented with it
    big = np.float32(Sb) * np.float32(3.0)
    hb = ida.Hnsw.from_ordered_points(raw, ida.Builder().metric(ida.METRIC_DOT).max_batch(1).dot_bound(big))
    ob = oracle.Index.build(np_augment(oracle, raw, big)[0], oracle.default_config(metric=0), threads=1)
    zb, lb = hb.into_parts()
    assert f32_bits(hb.info().dot_bound) == f32_bits(big)
    assert np.array_equal(zb, ob.zero) and all(np.array_equal(a, o) for a, o in zip(lb, ob.layers))
    # ... and one that is too small is refused, naming a row
    with pytest.raises(ida.IdistError) as e:
        ida.Hnsw.from_ordered_points(raw, ida.Builder().metric(ida.METRIC_DOT).dot_bound(np.float32(Sb) * np.float32(0.5)))
    assert e.value.status == 1 and "row" in e.value.message
    # rows already in HBM: the caller's device buffer is read, not written
    mem = DeviceMem(kind)
    try:
        d_x = mem.up(raw.copy())
        hd = ida.Hnsw.from_device_points(d_x, n, dim, ida.Builder().metric(ida.METRIC_DOT).max_batch(1))
        zd, ld = hd.into_parts()
        assert np.array_equal(pc.bits(mem.down(d_x, raw)), pc.bits(raw))
    finally:
        mem.free()
    assert np.array_equal(zd, oix.zero) and all(np.array_equal(a, o) for a, o in zip(ld, oix.layers))


def test_concurrent_build_is_searched_as_its_own_graph(eng, oracle):
    """the default (concurrent) schedule: whatever graph it made, the search over it is the oracle's over the same graph and X~"""
    ida, kind = eng
    n, dim, ef = S(kind, 300, 8000), S(kind, 9, 63), 50
    rng = np.random.default_rng(9)
    x = scaled_rows(rng, n, dim)
    h = ida.Hnsw.from_ordered_points(x, dot_builder(ida, ef))
    zero, layers = h.into_parts()
    xa, Sb, _ = np_augment(oracle, x)
    oix = oracle.Index.from_arrays(xa, zero, layers, oracle.default_config(metric=0, ef_search=ef))
    q = scaled_rows(rng, S(kind, 12, 1500), dim)
    want = oix.search(np_queries(q), threads=8)
    got = h.search_batch(q, ida.Search(), counters=True)
    assert np.array_equal(got.pid, want.pid) and np.array_equal(got.count, want.count)
    assert np.array_equal(got.counters, want.counters)
    assert np.array_equal(pc.bits(got.distance), reported(want.dist, np_norms(oracle, q), Sb))


# ---- 4. the distance entry points ---------------------------------------------------------------------------------------
def scan_only(ida, rows, builder):
    """an index that can only be scanned (no graph)"""
    return ida.Hnsw.from_parts(rows, np.full((len(rows), 64), INVALID, np.uint32), [], builder)


@pytest.mark.parametrize("dim", [5, 63, 300])
def test_distances_and_filter_bounds(eng, oracle, dim):
    ida, kind = eng
    rng = np.random.default_rng(dim)
    n, nq, n_ids = S(kind, 90, 3000), 5, 70
    x, q = scaled_rows(rng, n, dim), scaled_rows(rng, nq, dim)
    h = scan_only(ida, x, dot_builder(ida))
    ids = rng.integers(0, n, size=(nq, n_ids)).astype(np.uint32)
    ids[0, 3] = INVALID
    ids[-1, -1] = INVALID
    xa, Sb, _ = np_augment(oracle, x)
    qa, sq = np_queries(q), np_norms(oracle, q)
    raw = np.array([[oracle.distance(qa[i], xa[j], 0) if j != INVALID else np.inf for j in ids[i]] for i in range(nq)], np.float32)
    got = h.distances(q, ids)
    assert np.array_equal(pc.bits(got), reported(raw, sq, Sb))
    assert np.isposinf(got[0, 3]) and np.isposinf(got[-1, -1])
    # the formula's meaning, loosely here (section 7 does it properly): -q.x
    ok = ids != INVALID
    ip = np.einsum("qd,qid->qi", q.astype(np.float64), x.astype(np.float64)[np.where(ok, ids, 0)])
    assert np.allclose(got[ok], -ip[ok], rtol=0, atol=1e-4 * float(Sb + sq.max()))
    lb = h.filter_bounds(q, ids)
    assert np.all(lb <= got)
    # "no bound" is the trivial bound -t / 2, and no bound is below it
    t = (sq + Sb).astype(np.float32)
    trivial = (HALF * (np.float32(0.0) - t)).astype(np.float32)
    assert np.all(lb >= trivial[:, None])
    assert f32_bits(lb[0, 3]) == f32_bits(trivial[0]) and f32_bits(lb[-1, -1]) == f32_bits(trivial[-1])


def check_bruteforce(ida, oracle, n, dim, nq, k, seed):
    rng = np.random.default_rng(seed)
    x, q = scaled_rows(rng, n, dim), scaled_rows(rng, nq, dim)
    h = scan_only(ida, x, dot_builder(ida))
    xa, Sb, _ = np_augment(oracle, x)
    opid, odist = oracle.bruteforce(xa, np_queries(q), k, metric=0, threads=8)
    pid, dist = h.bruteforce(q, k)
    assert np.array_equal(pid, opid)
    assert np.array_equal(pc.bits(dist), reported(odist, np_norms(oracle, q), Sb))


def test_bruteforce(eng, oracle):
    ida, kind = eng
    check_bruteforce(ida, oracle, S(kind, 220, 5000), S(kind, 10, 47), S(kind, 6, 100), 10, 1)


@pytest.mark.gpu
def test_bruteforce_mfma_gpu(engine_loader, oracle):
    """nq >= 256 and n >= 16384: the MFMA filter + canonical re-rank"""
    ida = engine_loader("gpu")
    check_bruteforce(ida, oracle, 20000, 63, 300, 10, 2)


def mfma_bruteforce_knobs(monkeypatch):
    """every brute force takes the MFMA filter + canonical re-rank, whatever its size; a sample of 64 rows sets the thresholds"""
    pc.use_test_build(monkeypatch)                     # (both knobs exist in the test build only)
    monkeypatch.setenv("IDIST_BRUTEFORCE", "mfma")
    monkeypatch.setenv("IDIST_BF_SAMPLE", "64")


def test_bruteforce_mfma_path(eng, oracle, monkeypatch):
    """The MFMA path at a size the emulator runs too: n = 300 and nq = 130 are no multiples of its tiles, dim = 20 makes a 21-wide
    row with tail and remainder, and with n below the smallest candidate capacity (1024) no list can overflow, so the call cannot
    fall back to the scan."""
    ida, kind = eng
    mfma_bruteforce_knobs(monkeypatch)
    check_bruteforce(ida, oracle, 300, 20, 130, 10, 3)


def test_partitioned_bruteforce_mfma_path(eng, oracle, monkeypatch):
    """the parts' MFMA brute force leaves the distances raw: they are reported once, after the merge"""
    ida, kind = eng
    mfma_bruteforce_knobs(monkeypatch)
    rng = np.random.default_rng(6)
    x, q = scaled_rows(rng, 420, 20), scaled_rows(rng, 70, 20)
    xa, Sb, _ = np_augment(oracle, x)                                       # the bound of the WHOLE set
    b = dot_builder(ida).dot_bound(Sb)
    ph = ida.PartitionedHnsw.from_hnsws([scan_only(ida, np.ascontiguousarray(r), b) for r in (x[:150], x[150:])])
    opid, odist = oracle.bruteforce(xa, np_queries(q), 10, metric=0, threads=8)
    pid, dist = ph.bruteforce(q, 10)
    assert np.array_equal(pid, opid)
    assert np.array_equal(pc.bits(dist), reported(odist, np_norms(oracle, q), Sb))


# ---- 5. replicas and imports --------------------------------------------------------------------------------------------
def test_replicas_answer_as_the_root(eng, oracle):
    ida, kind = eng
    from instant_distance_amd import _capi

    n, dim, ef = S(kind, 150, 20000), 127, 37
    x, xa, Sb, zero, layers = dot_graph(oracle, n, dim)
    oix = oracle.Index.from_arrays(xa, zero, layers, oracle.default_config(metric=0, ef_search=ef))
    h = ida.Hnsw.from_parts(x, zero, layers, dot_builder(ida, ef))
    q = scaled_rows(np.random.default_rng(3), S(kind, 24, 1200), dim, "uniform")
    want = oix.search(np_queries(q), threads=8)
    want_bits = reported(want.dist, np_norms(oracle, q), Sb)

    def check(got):
        assert np.array_equal(got.pid, want.pid) and np.array_equal(got.count, want.count)
        assert np.array_equal(got.counters, want.counters)
        assert np.array_equal(pc.bits(got.distance), want_bits)

    check(h.search_batch(q, ida.Search(), counters=True))
    ids = np.random.default_rng(4).integers(0, n, size=(len(q), 16)).astype(np.uint32)
    for rccl in (False, True):
        try:
            (rep,) = h.replicate([0], rccl=rccl)
        except ida.IdistError as e:
            if rccl and e.status == 4:
                pytest.skip("librccl is missing")
            raise
        info = rep.info()
        assert info.metric == ida.METRIC_DOT and info.dim == dim and f32_bits(info.dot_bound) == f32_bits(Sb)
        check(rep.search_batch(q, ida.Search(), counters=True))
        check(ida.Hnsw.search_batch_sharded([h, rep], [ida.Search(), ida.Search()], q, counters=True))
        # the exact distances of a replica's rows: a second augmentation (or a lost S) would show here
        assert np.array_equal(pc.bits(rep.distances(q, ids)), pc.bits(h.distances(q, ids)))


def test_alloc_needs_the_bound(eng):
    """idist_index_alloc makes a replication target: its rows arrive augmented, so the S they were made with must come along"""
    ida, kind = eng
    from instant_distance_amd import _capi

    L = _capi.lib()
    cfg = dot_builder(ida)._config()
    assert cfg.dot_bound == 0.0
    h = C.c_void_p()
    lens = np.zeros(1, np.uint32)
    assert L.idist_index_alloc(10, 5, C.byref(cfg), _capi.u32p(lens), 0, 0, C.byref(h)) == 1 and not h.value
    cfg.dot_bound = 2.5
    L.check(L.idist_index_alloc(10, 5, C.byref(cfg), _capi.u32p(lens), 0, 0, C.byref(h)))
    t = ida.Hnsw(h, np.zeros((10, 0), np.float32), 100)
    info = t.info()
    assert info.dim == 5 and info.dot_bound == 2.5 and info.row_stride >= 6
    # other metrics ignore the field
    cfg2 = ida.Builder()._config()
    cfg2.dot_bound = 7.0
    h2 = C.c_void_p()
    L.check(L.idist_index_alloc(10, 5, C.byref(cfg2), _capi.u32p(lens), 0, 0, C.byref(h2)))
    assert ida.Hnsw(h2, np.zeros((10, 0), np.float32), 100).info().dot_bound == 0.0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, emu_so, q):
    try:
        import torch.distributed as dist

        sys.path.insert(0, ROOT)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import instant_distance_amd as ida
        from instant_distance_amd import _capi
        from instant_distance_amd import dist as idd

        _capi._singleton = _capi.Lib(emu_so)          # test-only engine swap (no GPU here)
        rng = np.random.default_rng(0)
        n, dim, nq = 260, 12, 31
        pts = (rng.standard_normal((n, dim)) * np.exp2(rng.uniform(-3, 3, size=(n, 1)))).astype(np.float32)
        queries = rng.standard_normal((nq, dim)).astype(np.float32)
        # the source's bound is GIVEN and larger than the rows' maximum: a replica that derived its own would hold other rows
        mk = lambda: ida.Builder().metric(ida.METRIC_DOT).max_batch(1).ef_search(40)   # noqa: E731
        hnsw = ida.Hnsw.from_ordered_points(pts, mk().dot_bound(4096.0)) if rank == 0 else None
        hnsw = idd.replicate_index(hnsw, mk(), src=0)
        lo, hi = idd.shard_range(nq, rank, world)
        r = hnsw.search_batch(queries[lo:hi], ida.Search(), counters=True)
        zero, layers = hnsw.into_parts()
        info = hnsw.info()
        q.put((rank, lo, hi, r.pid, r.distance, r.count, zero, float(info.dot_bound), int(info.dim), int(info.metric)))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # noqa: BLE001
        import traceback

        q.put((rank, "error", traceback.format_exc() + str(e)))


@pytest.mark.timeout(600)
def test_replicate_over_gloo_world2(oracle):
    """the host transport of dist.replicate_index: the receiving rank re-imports the caller's rows with the SOURCE's S"""
    import torch.multiprocessing as mp

    import engines

    emu_so = engines.build_emu()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, emu_so, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=500) for _ in procs]
    for p in procs:
        p.join(60)
    for g in got:
        assert g[1] != "error", g[2]
    got.sort(key=lambda g: g[0])
    rng = np.random.default_rng(0)
    pts = (rng.standard_normal((260, 12)) * np.exp2(rng.uniform(-3, 3, size=(260, 1)))).astype(np.float32)
    queries = rng.standard_normal((31, 12)).astype(np.float32)
    xa, Sb, s = np_augment(oracle, pts, 4096.0)
    assert s.max() < 4096.0
    oix = oracle.Index.build(xa, oracle.default_config(ef_search=40))
    want = oix.search(np_queries(queries))
    for g in got:
        assert np.array_equal(g[6], oix.zero) and g[7] == 4096.0 and g[8] == 12 and g[9] == 4
    pid = np.concatenate([g[3] for g in got])
    dist_ = np.concatenate([g[4] for g in got])
    cnt = np.concatenate([g[5] for g in got])
    assert np.array_equal(pid, want.pid) and np.array_equal(cnt, want.count)
    assert np.array_equal(pc.bits(dist_), reported(want.dist, np_norms(oracle, queries), Sb))


# ---- 6. partitioned -----------------------------------------------------------------------------------------------------
def merge_lists(res, sizes, ef):
    """numpy: per query the (distance bits, global id) pairs of the parts' results, lexsorted, cut, padded"""
    base = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    nq = len(res[0].count)
    o_pid = np.full((nq, ef), INVALID, np.uint32)
    o_bits = np.full((nq, ef), INF_BITS, np.uint32)
    o_cnt = np.zeros(nq, np.uint32)
    for qi in range(nq):
        gids = np.concatenate([r.pid[qi, : r.count[qi]].astype(np.uint64) + b for r, b in zip(res, base)])
        bits = np.concatenate([pc.bits(r.dist)[qi, : r.count[qi]] for r in res])
        order = np.lexsort((gids, bits))[:ef]
        o_pid[qi, : len(order)], o_bits[qi, : len(order)], o_cnt[qi] = gids[order].astype(np.uint32), bits[order], len(order)
    o_ctr = np.stack([r.counters for r in res]).sum(axis=0, dtype=np.uint32)
    return o_pid, o_bits, o_cnt, o_ctr


@pytest.mark.parametrize("P", [1, 3])
def test_partitioned(eng, oracle, P):
    ida, kind = eng
    n, dim, ef = S(kind, 330, 12000), S(kind, 6, 63), 37
    rng = np.random.default_rng(40 + P)
    x = scaled_rows(rng, n, dim)
    xa, Sb, _ = np_augment(oracle, x)                                       # the bound of the WHOLE set
    cuts = [0] + [int(n * (p + 1) * (p + 2) / (P * (P + 1))) for p in range(P)]
    rows = [np.ascontiguousarray(x[cuts[p]: cuts[p + 1]]) for p in range(P)]
    rows_a = [np.ascontiguousarray(xa[cuts[p]: cuts[p + 1]]) for p in range(P)]
    oixs = [oracle.Index.build(r, oracle.default_config(metric=0, ef_search=ef), threads=8) for r in rows_a]
    hs = [ida.Hnsw.from_parts(r, o.zero, o.layers, dot_builder(ida, ef).dot_bound(Sb)) for r, o in zip(rows, oixs)]
    ph = ida.PartitionedHnsw.from_hnsws(hs)
    assert ph.info().metric == ida.METRIC_DOT and ph.info().dim == dim
    for nq in (7, S(kind, 40, 1500)):
        q = scaled_rows(rng, nq, dim)
        qa, sq = np_queries(q), np_norms(oracle, q)
        w_pid, w_bits, w_cnt, w_ctr = merge_lists([o.search(qa, threads=8) for o in oixs], [len(r) for r in rows], ef)
        got = ph.search_batch(q, counters=True)
        assert np.array_equal(got.count, w_cnt) and np.array_equal(got.pid, w_pid) and np.array_equal(got.counters, w_ctr)
        assert np.array_equal(pc.bits(got.distance), reported(w_bits.view(np.float32), sq, Sb))   # reported AFTER the merge
    # exact search over all parts
    opid, odist = oracle.bruteforce(xa, qa, 10, metric=0, threads=8)
    pid, dist = ph.bruteforce(q, 10)
    assert np.array_equal(pid, opid) and np.array_equal(pc.bits(dist), reported(odist, sq, Sb))
    # a DOT part next to a squared-L2 part
    other = ida.Hnsw.from_parts(rows[0], oixs[0].zero, oixs[0].layers, ida.Builder().ef_search(ef))
    with pytest.raises(ida.IdistError) as e:
        ida.PartitionedHnsw.from_hnsws([hs[0], other])
    assert e.value.status == 1


def test_partitioned_build_shares_the_bound(eng, oracle):
    ida, kind = eng
    n, dim, ef, P = S(kind, 240, 9000), S(kind, 7, 31), 30, 3
    rng = np.random.default_rng(77)
    x = scaled_rows(rng, n, dim)
    x[n - 3] = np.float32(64.0) * np.sign(x[n - 3])                         # the largest norm sits in the LAST part
    _, Sb, s = np_augment(oracle, x)
    assert int(np.argmax(s)) == n - 3
    ph, ids = ida.PartitionedHnsw.build(x, dot_builder(ida, ef).seed(5), parts=P)
    assert [f32_bits(p.info().dot_bound) for p in ph.parts] == [f32_bits(Sb)] * P
    assert all(p.info().dim == dim for p in ph.parts)
    # searched as one: the numpy merge of the oracle's searches of every part's own graph over its rows of X~
    from instant_distance_amd.dist import shard_range

    oixs, sizes = [], []
    for p, part in enumerate(ph.parts):
        zero, layers = part.into_parts()
        pa = np_augment(oracle, part.points, Sb)[0]                         # part.points: the part's rows in ITS PointId order
        oixs.append(oracle.Index.from_arrays(pa, zero, layers, oracle.default_config(metric=0, ef_search=ef)))
        lo, hi = shard_range(n, p, P)
        sizes.append(hi - lo)
    q = scaled_rows(rng, S(kind, 9, 1100), dim)
    qa, sq = np_queries(q), np_norms(oracle, q)
    w_pid, w_bits, w_cnt, w_ctr = merge_lists([o.search(qa, threads=8) for o in oixs], sizes, ef)
    got = ph.search_batch(q, counters=True)
    assert np.array_equal(got.count, w_cnt) and np.array_equal(got.pid, w_pid) and np.array_equal(got.counters, w_ctr)
    assert np.array_equal(pc.bits(got.distance), reported(w_bits.view(np.float32), sq, Sb))
    # parts with different bounds are refused, and the message names the part
    a = scan_only(ida, x[:50], dot_builder(ida, ef).dot_bound(Sb))
    b = scan_only(ida, x[50:100], dot_builder(ida, ef).dot_bound(Sb))
    c = scan_only(ida, x[100:150], dot_builder(ida, ef))                    # derives its own, smaller bound
    assert f32_bits(c.info().dot_bound) != f32_bits(Sb)
    with pytest.raises(ida.IdistError) as e:
        ida.PartitionedHnsw.from_hnsws([a, b, c])
    assert e.value.status == 1 and "part 2" in e.value.message


# ---- 7. meaning, independent of the definition: float64 -----------------------------------------------------------------
def check_mips(q, x, pid, dist, Sb, dim, k):
    """every returned id has a float64 inner product >= the k-th largest minus tol, every distance is within tol of -q.x;
    tol = 4 (dim/8 + 12) 2^-24 (|q|^2 + S) per query: relative error (steps + folds) u on the sums of squares, three roundings
    in e, a factor 2 for comparing two candidates.  No query is left out.  Returns the largest error / tol seen."""
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    ip = q64 @ x64.T
    kth = -np.sort(-ip, axis=1)[:, k - 1]
    tol = 4.0 * (dim / 8.0 + 12.0) * 2.0 ** -24 * ((q64 * q64).sum(axis=1) + float(Sb))
    got_ip = np.take_along_axis(ip, pid.astype(np.int64), axis=1)
    assert np.all(got_ip >= (kth - tol)[:, None])
    err = np.abs(dist.astype(np.float64) + got_ip)
    assert np.all(err <= tol[:, None]), (err / tol[:, None]).max()
    return float((err / tol[:, None]).max())


@pytest.mark.parametrize("dim", [3, 32, 300, 768])
def test_is_the_inner_product(eng, oracle, dim):
    ida, kind = eng
    rng = np.random.default_rng(dim)
    n, nq, k = S(kind, 500, 2000), S(kind, 60, 400), 10
    x = (rng.standard_normal((n, dim)) * np.exp2(rng.uniform(-3, 3, size=(n, 1)))).astype(np.float32)
    q = (rng.standard_normal((nq, dim)) * np.exp2(rng.uniform(-3, 3, size=(nq, 1)))).astype(np.float32)
    h = scan_only(ida, x, dot_builder(ida))
    Sb = np.float32(h.info().dot_bound)
    pid, dist = h.bruteforce(q, k)
    worst = check_mips(q, x, pid, dist, Sb, dim, k)
    print(f"dim {dim}: max |d + q.x| / tol = {worst:.4f}")
    if kind == "emu":
        # the reference alone passes the same assertion: the oracle's L2SQ brute force over X~, reported by the formula
        xa, So, _ = np_augment(oracle, x)
        opid, odist = oracle.bruteforce(xa, np_queries(q), k, metric=0, threads=8)
        orep = reported(odist, np_norms(oracle, q), So).view(np.float32)
        print(f"dim {dim}: oracle alone {check_mips(q, x, opid, orep, So, dim, k):.4f}")
    # not L2 in disguise: the nearest row by inner product is not the nearest row by distance
    l2 = scan_only(ida, x, ida.Builder())
    l2pid, _ = l2.bruteforce(q, 1)
    differ = float((l2pid[:, 0] != pid[:, 0]).mean())
    print(f"dim {dim}: DOT top-1 != L2SQ top-1 for {100 * differ:.1f} % of the queries")
    assert differ > 0.25, differ


# ---- 8. info and refusals -----------------------------------------------------------------------------------------------
def test_info_and_refusals(eng, oracle):
    ida, kind = eng
    rng = np.random.default_rng(1)
    x = scaled_rows(rng, 40, 5)
    _, Sb, _ = np_augment(oracle, x)
    h = scan_only(ida, x, dot_builder(ida))
    info = h.info()
    assert info.dim == 5 and info.metric == 4 and info.n == 40 and f32_bits(info.dot_bound) == f32_bits(Sb)
    assert info.row_stride >= 6
    assert scan_only(ida, x, ida.Builder()).info().dot_bound == 0.0
    assert scan_only(ida, x, ida.Builder().metric(ida.METRIC_COSINE).dot_bound(3.0)).info().dot_bound == 0.0
    # a query of another dimension (kdim included)
    for d in (4, 6):
        with pytest.raises(TypeError):
            h.search_batch(np.zeros((2, d), np.float32), ida.Search())
    # metric 3 stays unassigned
    with pytest.raises(ida.IdistError) as e:
        scan_only(ida, x, ida.Builder().metric(3))
    assert e.value.status == 1
    # dim 65536 is one too many for kdim; 65535 is the limit (refused before anything is read)
    from instant_distance_amd import _capi

    L = _capi.lib()
    cfg = dot_builder(ida)._config()
    hh = C.c_void_p()
    one = np.zeros(65536, np.float32)
    assert L.idist_index_build(_capi.f32p(one), 1, 65536, C.byref(cfg), 0, C.byref(hh)) == 1 and not hh.value
    assert b"65535" in L.idist_last_error()
    # a bound that is negative or not finite
    for bad in (-1.0, np.inf, np.nan):
        with pytest.raises(ida.IdistError) as e:
            scan_only(ida, x, dot_builder(ida).dot_bound(bad))
        assert e.value.status == 1
