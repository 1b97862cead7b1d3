"""Cosine distance (IDIST_METRIC_COSINE, include/idist.h).

A cosine index over rows X is DEFINED as the squared-L2 index over the normalised rows X^ (s = the canonical squared-L2 distance
to the origin, r = sqrt(s), x^ = x / r, all f32 and correctly rounded; x^ = x where r is not a positive finite number), searched
with q^, with every reported distance multiplied by 0.5f.  So everything here is exact: expected values come from the oracle's
L2SQ paths and numpy, never from the code under test; ids, counts and counters are compared with array_equal, distances and
rows as bit patterns.  Every case runs on the CPU emulator and (-m gpu) on the MI355X."""
import ctypes as C

import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params

INVALID = 0xFFFFFFFF
INF_BITS = 0x7F800000
HALF = np.float32(0.5)


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


def S(kind, emu, gpu):
    return gpu if kind == "gpu" else emu


def np_normalize(oracle, x):
    """steps 1-3 of the definition in numpy: (x^, s), s from the oracle's canonical distance to the origin"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    origin = np.zeros(x.shape[1], dtype=np.float32)
    s = np.array([oracle.distance(row, origin, 0) for row in x], dtype=np.float32)
    with np.errstate(all="ignore"):
        r = np.sqrt(s)
        assert r.dtype == np.float32
        ok = np.isfinite(r) & (r > 0)
        out = x.copy()
        out[ok] = x[ok] / r[ok][:, None]
    assert out.dtype == np.float32
    return out, s


def scaled_rows(rng, n, dim, kind="normal"):
    """rows whose lengths spread over 2^-3 .. 2^3: nothing about them is normalised already"""
    x = rng.standard_normal((n, dim)).astype(np.float32) if kind == "normal" else pc.gen_points(rng, n, dim)
    return np.ascontiguousarray(x * np.exp2(rng.uniform(-3, 3, size=(n, 1))).astype(np.float32))


def halved(d):
    return pc.bits(np.ascontiguousarray(d, dtype=np.float32) * HALF)


def cosine_builder(ida, ef=100):
    return ida.Builder().metric(ida.METRIC_COSINE).ef_search(ef)


# device memory for the device-pointer entries: under the emulator hipMalloc memory is host memory, so a numpy array IS a valid
# "device" buffer; on the GPU the HIP runtime libidist.so already loaded is driven through ctypes
class DeviceMem:
    def __init__(self, kind):
        self.kind, self.keep, self.hip = kind, [], None
        if kind == "gpu":
            path = None
            for line in open("/proc/self/maps"):
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
            assert path, "libidist.so is loaded, so a HIP runtime must be mapped"
            self.hip = C.CDLL(path)
            self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            self.hip.hipFree.argtypes = [C.c_void_p]
            assert self.hip.hipSetDevice(0) == 0

    def up(self, arr):
        arr = np.ascontiguousarray(arr)
        if self.hip is None:
            self.keep.append(arr)
            return arr.ctypes.data
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(arr.nbytes, 16)) == 0
        self.keep.append(p)
        assert self.hip.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) == 0       # hipMemcpyHostToDevice
        return p.value

    def down(self, ptr, like):
        if self.hip is None:
            return next(a for a in self.keep if isinstance(a, np.ndarray) and a.ctypes.data == ptr)
        assert self.hip.hipDeviceSynchronize() == 0
        out = np.empty_like(like)
        assert self.hip.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), out.nbytes, 2) == 0   # hipMemcpyDeviceToHost
        return out

    def free(self):
        if self.hip is not None:
            for p in self.keep:
                self.hip.hipFree(p)
        self.keep = []


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------
DIMS = [1, 3, 4, 7, 8, 9, 12, 64, 96, 128, 300, 301, 768, 1030]


@pytest.mark.parametrize("dim", DIMS)
def test_normalize_kernel(eng, oracle, dim):
    ida, kind = eng
    rng = np.random.default_rng(100 + dim)
    n = S(kind, 21, 1003)                       # not a multiple of the eight rows a wave takes at a time
    x = scaled_rows(rng, n, dim)
    keep = x.copy()
    got, s = ida.normalize(x, return_norm2=True)
    want, want_s = np_normalize(oracle, x)
    assert np.array_equal(x, keep)
    assert np.array_equal(pc.bits(s), pc.bits(want_s))
    assert np.array_equal(pc.bits(got), pc.bits(want))
    assert np.array_equal(pc.bits(ida.normalize(x)), pc.bits(want))            # without the norms: same rows
    if dim > 1:
        assert np.any(pc.bits(got) != pc.bits(x))
    # scaling a row by a power of two does not change x^
    k = rng.integers(-20, 21, size=(n, 1))
    assert np.array_equal(pc.bits(ida.normalize(np.ldexp(x, k).astype(np.float32))), pc.bits(want))


@pytest.mark.parametrize("dim", [5, 300])
def test_normalize_kernel_past_the_grid(eng, oracle, dim):
    """more rows than the grid's waves take in one trip (eight each): a wave normalises rows r .. r + 7, then the eight rows a grid
    further.  1009 distinct rows, row i of the batch = row i % 1009 (the trip length is no multiple of 1009), the model over the 1009;
    the bit rule of test_normalize_kernel"""
    # cap: min(ceil(n / 8), n_cu * 32) waves of eight rows, launch_normalize (idist_capi.hip)
    from engines import cu_count
    ida, kind = eng
    m = 1009
    n = 8 * cu_count(kind) * 32 + 37
    assert n > m or kind == "emu"
    rng = np.random.default_rng(150 + dim)
    base = scaled_rows(rng, m, dim)
    rows = np.arange(n) % m
    x = np.ascontiguousarray(base[rows])
    want, want_s = np_normalize(oracle, base)
    got, s = ida.normalize(x, return_norm2=True)
    assert np.array_equal(pc.bits(s), pc.bits(want_s[rows]))
    assert np.array_equal(pc.bits(got), pc.bits(want[rows]))


@pytest.mark.parametrize("dim", [1, 5, 12, 300])
def test_normalize_special_rows(eng, oracle, dim):
    """zero, NaN, inf, an s that overflows and denormals whose s underflows: all come back unchanged"""
    ida, kind = eng
    rng = np.random.default_rng(7 + dim)
    x = rng.standard_normal((11, dim)).astype(np.float32)
    x[1] = 0.0
    x[3, dim // 2] = np.nan
    x[4, dim - 1] = np.inf
    x[6] = np.float32(3.0e19) * np.sign(x[6])                               # s = dim * 9e38 > f32 max
    x[8] = np.float32(1.0e-39) * x[8]                                       # denormals: every square underflows to 0
    x[9, 0] = -np.inf
    got, s = ida.normalize(x, return_norm2=True)
    want, want_s = np_normalize(oracle, x)
    special = [1, 3, 4, 6, 8, 9]
    assert np.array_equal(pc.bits(want[special]), pc.bits(x[special]))      # the restatement agrees that these stay
    assert np.array_equal(pc.bits(got), pc.bits(want))
    assert np.array_equal(pc.bits(got[special]), pc.bits(x[special]))
    nan = np.isnan(want_s)
    assert np.array_equal(np.isnan(s), nan) and list(np.flatnonzero(nan)) == [3]
    assert np.array_equal(pc.bits(s[~nan]), pc.bits(want_s[~nan]))
    assert s[1] == 0 and s[8] == 0 and np.isposinf(s[[4, 6, 9]]).all()


# ---- 2. search parity ---------------------------------------------------------------------------------------------------
_GRAPHS = {}


def cosine_graph(oracle, n, dim, seed=11):
    """raw rows, their normalised form and the oracle's L2SQ graph over the latter (cached: ef_search does not enter a build)"""
    key = (n, dim, seed)
    if key not in _GRAPHS:
        rng = np.random.default_rng(seed)
        x = scaled_rows(rng, n, dim, "uniform")
        xn, _ = np_normalize(oracle, x)
        o = oracle.Index.build(xn, oracle.default_config(metric=0), threads=8 if n > 1000 else 1)
        _GRAPHS.clear()
        _GRAPHS[key] = (x, xn, o.zero, o.layers)
    return _GRAPHS[key]


def check_cosine_search(ida, oracle, kind, n, dim, ef):
    x, xn, zero, layers = cosine_graph(oracle, n, dim)
    oix = oracle.Index.from_arrays(xn, zero, layers, oracle.default_config(metric=0, ef_search=ef))
    h = ida.Hnsw.from_parts(x, zero, layers, cosine_builder(ida, ef))       # raw rows: the import normalises
    assert h.info().metric == ida.METRIC_COSINE
    rng = np.random.default_rng(1000 * dim + ef)
    search = ida.Search()
    for nq in (7, S(kind, 70, 2048), 1):
        q = scaled_rows(rng, nq, dim, "uniform")
        if nq > 2:
            q[1] = x[min(5, n - 1)] * np.float32(4.0)                         # a stored direction: distance 0 first
        keep = q.copy()
        qn, _ = np_normalize(oracle, q)
        want = oix.search(qn, threads=8)
        got = h.search_batch(q, search, counters=True)
        assert np.array_equal(q, keep)
        assert np.array_equal(got.count, want.count)
        assert np.array_equal(got.pid, want.pid)
        assert np.array_equal(got.counters, want.counters)
        assert np.array_equal(pc.bits(got.distance), halved(want.dist))
    return h


@pytest.mark.parametrize("ef", [100, 37])
def test_search_parity(eng, oracle, ef):
    ida, kind = eng
    check_cosine_search(ida, oracle, kind, S(kind, 330, 30000), S(kind, 6, 96), ef)


@pytest.mark.gpu
@pytest.mark.parametrize("ef", [100, 37])
@pytest.mark.parametrize("n,dim", [(20000, 128), (12000, 300), (6000, 768)])
def test_search_parity_compiled_geometries_gpu(engine_loader, oracle, n, dim, ef):
    ida = engine_loader("gpu")
    check_cosine_search(ida, oracle, "gpu", n, dim, ef)


def test_search_device_pointers(eng, oracle):
    """idist_search_batch_device: the caller's device queries are read, never written; results as the host-pointer call's"""
    ida, kind = eng
    n, dim, ef, nq = S(kind, 330, 30000), S(kind, 6, 96), 37, S(kind, 9, 600)
    x, xn, zero, layers = cosine_graph(oracle, n, dim)
    h = ida.Hnsw.from_parts(x, zero, layers, cosine_builder(ida, ef))
    q = scaled_rows(np.random.default_rng(5), nq, dim, "uniform")
    want = h.search_batch(q, ida.Search(), counters=True)
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
    assert np.array_equal(pc.bits(got[1]), pc.bits(want.distance))


# ---- 3. build parity ----------------------------------------------------------------------------------------------------
def test_build_parity(eng, oracle):
    ida, kind = eng
    n, dim, seed = S(kind, 200, 6000), S(kind, 6, 32), 4321
    rng = np.random.default_rng(8)
    x = scaled_rows(rng, n, dim)
    keep = x.copy()
    b = ida.Builder().metric(ida.METRIC_COSINE).max_batch(1).seed(seed)
    h, ids = b.build_hnsw(x)
    assert np.array_equal(pc.bits(x), pc.bits(keep))
    out_pid, order = oracle.permutation(seed, n)
    assert ids == [int(p) for p in out_pid]
    raw = np.ascontiguousarray(x[order])
    xn, _ = np_normalize(oracle, raw)                                       # per row: commutes with the shuffle
    oix = oracle.Index.build(xn, oracle.default_config(metric=0), threads=1)
    zero, layers = h.into_parts()
    assert np.array_equal(zero, oix.zero) and len(layers) == len(oix.layers)
    assert all(np.array_equal(a, o) for a, o in zip(layers, oix.layers))
    # the host copies are the caller's rows
    assert all(np.array_equal(pc.bits(h[ids[i]]), pc.bits(x[i])) for i in range(0, n, max(1, n // 40)))
    q = scaled_rows(rng, 1, dim)[0]
    items = list(h.search(q, ida.Search()))
    want = oix.search(np_normalize(oracle, q[None, :])[0])
    assert [it.pid for it in items] == list(want.pid[0, : want.count[0]])
    assert all(np.array_equal(pc.bits(it.point), pc.bits(raw[it.pid])) for it in items)
    assert np.array_equal(pc.bits(np.array([it.distance for it in items], np.float32)), halved(want.dist[0, : want.count[0]]))
    # HnswMap: values follow the points, points stay raw
    m = b.build(x, list(range(n)))
    mi = list(m.search(q, ida.Search()))
    assert [it.pid for it in mi] == [it.pid for it in items]
    assert all(np.array_equal(pc.bits(it.point), pc.bits(x[it.value])) for it in mi)
    # rows already in HBM: the caller's device buffer is read, not written
    mem = DeviceMem(kind)
    try:
        d_x = mem.up(raw.copy())
        hd = ida.Hnsw.from_device_points(d_x, n, dim, ida.Builder().metric(ida.METRIC_COSINE).max_batch(1))
        zd, ld = hd.into_parts()
        assert np.array_equal(pc.bits(mem.down(d_x, raw)), pc.bits(raw))
    finally:
        mem.free()
    assert np.array_equal(zd, oix.zero) and all(np.array_equal(a, o) for a, o in zip(ld, oix.layers))


# ---- 4. the other outputs -----------------------------------------------------------------------------------------------
def scan_only(ida, rows, builder):
    """an index that can only be scanned (no graph)"""
    return ida.Hnsw.from_parts(rows, np.full((len(rows), 64), INVALID, np.uint32), [], builder)


@pytest.mark.parametrize("dim", [5, 64, 300])
def test_distances_and_filter_bounds(eng, oracle, dim):
    ida, kind = eng
    rng = np.random.default_rng(dim)
    n, nq, n_ids = S(kind, 90, 3000), 5, 70
    x, q = scaled_rows(rng, n, dim), scaled_rows(rng, nq, dim)
    h = scan_only(ida, x, cosine_builder(ida))
    ids = rng.integers(0, n, size=(nq, n_ids)).astype(np.uint32)
    ids[0, 3] = INVALID
    ids[-1, -1] = INVALID
    xn, qn = np_normalize(oracle, x)[0], np_normalize(oracle, q)[0]
    want = np.array([[oracle.distance(qn[i], xn[j], 0) if j != INVALID else np.inf for j in ids[i]] for i in range(nq)], np.float32)
    got = h.distances(q, ids)
    assert np.array_equal(pc.bits(got), halved(want))
    lb = h.filter_bounds(q, ids)
    assert np.all(lb <= got)
    assert np.all(lb >= 0)


def check_bruteforce(ida, oracle, n, dim, nq, k, seed):
    rng = np.random.default_rng(seed)
    x, q = scaled_rows(rng, n, dim), scaled_rows(rng, nq, dim)
    h = scan_only(ida, x, cosine_builder(ida))
    xn, qn = np_normalize(oracle, x)[0], np_normalize(oracle, q)[0]
    opid, odist = oracle.bruteforce(xn, qn, k, metric=0, threads=8)
    pid, dist = h.bruteforce(q, k)
    assert np.array_equal(pid, opid)
    assert np.array_equal(pc.bits(dist), halved(odist))


def test_bruteforce(eng, oracle):
    ida, kind = eng
    check_bruteforce(ida, oracle, S(kind, 220, 5000), S(kind, 10, 48), S(kind, 6, 100), 10, 1)


@pytest.mark.gpu
def test_bruteforce_mfma_gpu(engine_loader, oracle):
    """nq >= 256 and n >= 16384: the MFMA filter + canonical re-rank"""
    ida = engine_loader("gpu")
    check_bruteforce(ida, oracle, 20000, 64, 300, 10, 2)


def mfma_bruteforce_knobs(monkeypatch):
    """every brute force takes the MFMA filter + canonical re-rank, whatever its size; a sample of 64 rows sets the thresholds"""
    pc.use_test_build(monkeypatch)                     # (both knobs exist in the test build only)
    monkeypatch.setenv("IDIST_BRUTEFORCE", "mfma")
    monkeypatch.setenv("IDIST_BF_SAMPLE", "64")


def test_bruteforce_mfma_path(eng, oracle, monkeypatch):
    """The MFMA path at a size the emulator runs too: n = 300 and nq = 130 are no multiples of its tiles, and with n below the
    smallest candidate capacity (1024) no list can overflow, so the call cannot fall back to the scan."""
    ida, kind = eng
    mfma_bruteforce_knobs(monkeypatch)
    check_bruteforce(ida, oracle, 300, 20, 130, 10, 3)


def test_partitioned_bruteforce_mfma_path(eng, oracle, monkeypatch):
    """the parts' MFMA brute force leaves the distances raw: they are halved once, after the merge"""
    ida, kind = eng
    mfma_bruteforce_knobs(monkeypatch)
    rng = np.random.default_rng(6)
    x, q = scaled_rows(rng, 420, 20), scaled_rows(rng, 70, 20)
    ph = ida.PartitionedHnsw.from_hnsws([scan_only(ida, np.ascontiguousarray(r), cosine_builder(ida)) for r in (x[:150], x[150:])])
    xn, qn = np_normalize(oracle, x)[0], np_normalize(oracle, q)[0]
    opid, odist = oracle.bruteforce(xn, qn, 10, metric=0, threads=8)
    pid, dist = ph.bruteforce(q, 10)
    assert np.array_equal(pid, opid)
    assert np.array_equal(pc.bits(dist), halved(odist))


# ---- 5. replicas and parts ----------------------------------------------------------------------------------------------
def test_replicas_answer_as_the_root(eng, oracle):
    ida, kind = eng
    n, dim, ef = S(kind, 330, 30000), S(kind, 6, 96), 37
    x, xn, zero, layers = cosine_graph(oracle, n, dim)
    # the mistake this test exists for: a replica that normalised its (already normalised) rows again would hold other bits
    twice = np_normalize(oracle, xn)[0]
    changed = np.any(pc.bits(twice) != pc.bits(xn), axis=1).mean()
    assert 0.2 < changed < 0.5, changed
    oix = oracle.Index.from_arrays(xn, zero, layers, oracle.default_config(metric=0, ef_search=ef))
    h = ida.Hnsw.from_parts(x, zero, layers, cosine_builder(ida, ef))
    q = scaled_rows(np.random.default_rng(3), S(kind, 24, 1200), dim, "uniform")
    want = oix.search(np_normalize(oracle, q)[0], threads=8)

    def check(got):
        assert np.array_equal(got.pid, want.pid) and np.array_equal(got.count, want.count)
        assert np.array_equal(got.counters, want.counters)
        assert np.array_equal(pc.bits(got.distance), halved(want.dist))

    check(h.search_batch(q, ida.Search(), counters=True))
    (rep,) = h.replicate([0])
    assert rep.info().metric == ida.METRIC_COSINE
    check(rep.search_batch(q, ida.Search(), counters=True))
    check(ida.Hnsw.search_batch_sharded([h, rep], [ida.Search(), ida.Search()], q, counters=True))
    # the exact distances of a replica's rows: a second normalisation would show here too
    ids = np.random.default_rng(4).integers(0, n, size=(len(q), 16)).astype(np.uint32)
    assert np.array_equal(pc.bits(rep.distances(q, ids)), pc.bits(h.distances(q, ids)))


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
    n, dim, ef = S(kind, 330, 12000), S(kind, 6, 64), 37
    rng = np.random.default_rng(40 + P)
    x = scaled_rows(rng, n, dim)
    cuts = [0] + [int(n * (p + 1) * (p + 2) / (P * (P + 1))) for p in range(P)]
    rows = [np.ascontiguousarray(x[cuts[p]: cuts[p + 1]]) for p in range(P)]
    oixs = [oracle.Index.build(np_normalize(oracle, r)[0], oracle.default_config(metric=0, ef_search=ef), threads=8) for r in rows]
    hs = [ida.Hnsw.from_parts(r, o.zero, o.layers, cosine_builder(ida, ef)) for r, o in zip(rows, oixs)]
    ph = ida.PartitionedHnsw.from_hnsws(hs)
    assert ph.info().metric == ida.METRIC_COSINE
    for nq in (7, S(kind, 40, 1500)):
        q = scaled_rows(rng, nq, dim)
        qn = np_normalize(oracle, q)[0]
        w_pid, w_bits, w_cnt, w_ctr = merge_lists([o.search(qn, threads=8) for o in oixs], [len(r) for r in rows], ef)
        got = ph.search_batch(q, counters=True)
        assert np.array_equal(got.count, w_cnt) and np.array_equal(got.pid, w_pid) and np.array_equal(got.counters, w_ctr)
        assert np.array_equal(pc.bits(got.distance), halved(w_bits.view(np.float32)))      # scaled AFTER the merge
    # exact search over all parts
    xn = np_normalize(oracle, x)[0]
    opid, odist = oracle.bruteforce(xn, qn, 10, metric=0, threads=8)
    pid, dist = ph.bruteforce(q, 10)
    assert np.array_equal(pid, opid) and np.array_equal(pc.bits(dist), halved(odist))
    # a cosine part next to a squared-L2 part
    other = ida.Hnsw.from_parts(rows[0], oixs[0].zero, oixs[0].layers, ida.Builder().ef_search(ef))
    with pytest.raises(ida.IdistError) as e:
        ida.PartitionedHnsw.from_hnsws([hs[0], other])
    assert e.value.status == 1


# ---- 6. meaning, independent of the definition --------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [7, 32, 300])
def test_is_the_cosine_distance(eng, dim):
    """Exact cosine in float64: wherever the first eleven cosines of a query are pairwise more than 1e-5 apart, the top ten are
    exactly the float64 top ten, and every reported distance is within 1e-6 of 1 - cos.  At most 5 % of the queries may be left
    out by the condition (the oracle alone leaves out 0.5 %, 1.5 % and 2.75 % at dims 7, 32, 300, and agrees on all the rest);
    the oracle's own worst |distance - (1 - cos)| on these inputs is 2.2e-7 (300-d)."""
    ida, kind = eng
    rng = np.random.default_rng(dim)
    n, nq = 2000, 400
    x = (rng.standard_normal((n, dim)) * np.exp2(rng.uniform(-3, 3, size=(n, 1)))).astype(np.float32)
    q = (rng.standard_normal((nq, dim)) * np.exp2(rng.uniform(-3, 3, size=(nq, 1)))).astype(np.float32)
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    cos = (q64 / np.linalg.norm(q64, axis=1, keepdims=True)) @ (x64 / np.linalg.norm(x64, axis=1, keepdims=True)).T
    order = np.argsort(-cos, axis=1, kind="stable")[:, :11]
    top = np.take_along_axis(cos, order, axis=1)
    clear = np.all(top[:, :-1] - top[:, 1:] > 1e-5, axis=1)
    assert clear.mean() >= 0.95, clear.mean()
    h = scan_only(ida, x, cosine_builder(ida))
    pid, dist = h.bruteforce(q, 10)
    assert np.array_equal(pid[clear], order[clear, :10].astype(np.uint32))
    err = np.abs(dist.astype(np.float64) - (1.0 - np.take_along_axis(cos, pid.astype(np.int64), axis=1)))
    print(f"dim {dim}: {100 * (1 - clear.mean()):.2f} % of the queries left out, max |d - (1 - cos)| = {err.max():.3e}")
    assert err.max() < 1e-6, err.max()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    ida, kind = eng
    from instant_distance_amd import _capi

    L = _capi.lib()
    x = np.ones((4, 3), np.float32)
    with pytest.raises(ida.IdistError) as e:
        ida.Hnsw.from_ordered_points(x, ida.Builder().metric(3))
    assert e.value.status == 1
    with pytest.raises(ida.IdistError) as e:
        scan_only(ida, x, ida.Builder().metric(-1))
    assert e.value.status == 1
    out, s = np.zeros_like(x), np.zeros(4, np.float32)
    f = _capi.f32p
    assert L.idist_normalize_batch(f(x), 4, 0, f(out), f(s), 0) == 1
    assert L.idist_normalize_batch(None, 4, 3, f(out), f(s), 0) == 1
    assert L.idist_normalize_batch(f(x), 4, 3, None, f(s), 0) == 1
    assert L.idist_normalize_batch(f(x), 0, 3, f(out), f(s), 0) == 0
    assert L.idist_normalize_batch(f(x), 4, 3, f(out), None, 0) == 0
    assert np.array_equal(pc.bits(out), pc.bits(np.full((4, 3), np.float32(1.0) / np.sqrt(np.float32(3.0)), np.float32)))
    assert ida.normalize(np.zeros((0, 5), np.float32)).shape == (0, 5)
