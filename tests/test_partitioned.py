"""Partitioned index (include/idist.h): P ordinary indexes searched as one, merged on the device.

The answer of a partitioned search is DEFINED as the merge, by the reference's `Candidate` order (core/types.rs:229-234:
distance, then id), of what `Hnsw::search` returns on every part with ids made global — so everything here is compared
exactly: ids, counts and counters with array_equal, distances as bit patterns.  Expected values come from the oracle and
numpy, never from the code under test.  Every case runs on the CPU emulator and (-m gpu) on the MI355X."""
import ctypes as C

import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params

INVALID = 0xFFFFFFFF
INF_BITS = 0x7F800000
NAN_BITS = 0x7FC00000      # kNanBits: the one NaN pattern canonical distances carry (idist_device.hpp)


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


def S(kind, emu, gpu):
    return gpu if kind == "gpu" else emu


# ---------------------------------------------------------------------------------------------------------------------
# device memory for the device-pointer entry: under the emulator hipMalloc memory is host memory, so a numpy array IS a
# valid "device" buffer; on the GPU the HIP runtime libidist.so already loaded is driven through ctypes (a second runtime
# in the process — torch's bundled copy — could not see the first one's allocations)
# ---------------------------------------------------------------------------------------------------------------------
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

    def up_tiled(self, block, nq):
        """block [P][m][...] -> the device array [P][nq][...] whose row q is block row q % m, without making it on the host"""
        block = np.ascontiguousarray(block)
        if self.hip is None:
            return self.up(block[:, np.arange(nq) % block.shape[1]])
        P, m = block.shape[:2]
        row = block[0, 0].nbytes
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), P * nq * row) == 0
        self.keep.append(p)
        for l in range(P):
            for q0 in range(0, nq, m):
                rows = min(m, nq - q0)
                assert self.hip.hipMemcpy(C.c_void_p(p.value + (l * nq + q0) * row), block[l].ctypes.data, rows * row, 1) == 0
        return p.value

    def free(self):
        if self.hip is not None:
            for p in self.keep:
                self.hip.hipFree(p)
        self.keep = []


def run_merge(kind, pid, dist_bits, count, counters, base, out_width, nq=None):
    """idist_merge_topk_device on [P][nq][w] lists; returns (pid, dist bits, count, counters) of the merged result.
    nq: the lists are [P][m][w] and row q of the batch is their row q % m (tiled on the device: the wide batches of the grid tests)"""
    from instant_distance_amd import _capi

    P, m, w = pid.shape
    mem = DeviceMem(kind)
    if nq is not None:
        up = mem.up
        mem.up = lambda x: mem.up_tiled(x, nq) if (x.ndim >= 2 and x.shape[:2] == (P, m)) else up(x)
    else:
        nq = m
    try:
        # outputs start as a pattern no result can hold: every element must be written (results and padding alike)
        o_pid = np.full((nq, out_width), 0xABABABAB, np.uint32)
        o_dist = np.full((nq, out_width), 0xABABABAB, np.uint32)
        o_cnt = np.full(nq, 0xABABABAB, np.uint32)
        o_ctr = np.full((nq, 3), 0xABABABAB, np.uint32)
        d = [mem.up(x) for x in (pid, dist_bits, count)]
        d_ctr = mem.up(counters) if counters is not None else None
        d_out = [mem.up(x) for x in (o_pid, o_dist, o_cnt, o_ctr)]
        L = _capi.lib()
        b = np.ascontiguousarray(base, dtype=np.uint32)
        L.check(L.idist_merge_topk_device(d[0], d[1], d[2], d_ctr, P, nq, w, _capi.u32p(b), out_width, d_out[0], d_out[1],
                                          d_out[2], d_out[3] if counters is not None else None, 0, None))
        res = [mem.down(p, like).copy() for p, like in zip(d_out, (o_pid, o_dist, o_cnt, o_ctr))]
    finally:
        mem.free()
    return res[0], res[1], res[2], (res[3] if counters is not None else None)


def merge_reference(pid, dist_bits, count, counters, base, out_width):
    """numpy: per query the (distance bits, global id) pairs of the lists' first `count` entries, lexsorted, cut, padded."""
    P, nq, w = pid.shape
    o_pid = np.full((nq, out_width), INVALID, np.uint32)
    o_dist = np.full((nq, out_width), INF_BITS, np.uint32)
    o_cnt = np.zeros(nq, np.uint32)
    for q in range(nq):
        gids, bits = [], []
        for p in range(P):
            c = min(int(count[p, q]), w)
            gids.append(pid[p, q, :c].astype(np.uint64) + np.uint64(base[p]))
            bits.append(dist_bits[p, q, :c])
        gids, bits = np.concatenate(gids), np.concatenate(bits)
        order = np.lexsort((gids, bits))[:out_width]
        o_pid[q, : len(order)] = gids[order].astype(np.uint32)
        o_dist[q, : len(order)] = bits[order]
        o_cnt[q] = len(order)
    o_ctr = counters.astype(np.uint32).sum(axis=0, dtype=np.uint32) if counters is not None else None
    return o_pid, o_dist, o_cnt, o_ctr


def random_lists(rng, P, nq, w, full=False):
    """P sorted lists per query with everything the merge must cope with: counts 0, ragged and full; the same distance in
    several lists (a small pool of values, so the global id decides); +inf and NaN distances as real results; and behind
    every list's count GARBAGE that would win if it were read (distance 0 and small ids) — the counts rule, not the padding."""
    sizes = rng.integers(w, w + 40, size=P)
    base = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint32)
    pool = np.sort(rng.random(max(4, (P * w) // 3), dtype=np.float32)).view(np.uint32)
    pool = np.concatenate([pool, np.full(3, INF_BITS, np.uint32), np.full(3, NAN_BITS, np.uint32)])
    pid = rng.integers(0, 8, size=(P, nq, w)).astype(np.uint32)               # garbage: small ids ...
    bits = np.zeros((P, nq, w), np.uint32)                                      # ... at distance 0
    bits[:, :, 1::2] = rng.integers(0, 2**32, size=bits[:, :, 1::2].shape, dtype=np.uint64).astype(np.uint32)
    count = np.zeros((P, nq), np.uint32)
    for p in range(P):
        for q in range(nq):
            mode = 2 if full else rng.integers(0, 4)
            c = (0, int(rng.integers(0, w + 1)), w, w)[mode]
            ids = rng.choice(sizes[p], size=c, replace=False).astype(np.uint32)
            d = rng.choice(pool, size=c)
            order = np.lexsort((ids, d))
            pid[p, q, :c], bits[p, q, :c], count[p, q] = ids[order], d[order], c
    counters = rng.integers(0, 2**32, size=(P, nq, 3), dtype=np.uint64).astype(np.uint32)
    return pid, bits, count, counters, base


def check_merge(kind, lists, out_width, with_counters=True):
    pid, bits, count, counters, base = lists
    ctr = counters if with_counters else None
    got = run_merge(kind, pid, bits, count, ctr, base, out_width)
    want = merge_reference(pid, bits, count, ctr, base, out_width)
    assert np.array_equal(got[2], want[2]), "count"
    assert np.array_equal(got[0], want[0]), "global ids"
    assert np.array_equal(got[1], want[1]), "distance bits"
    if with_counters:
        assert np.array_equal(got[3], want[3]), "counters"


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 7, 64, 100, 257])
@pytest.mark.parametrize("P", [1, 2, 3, 8, 64])
def test_merge_kernel(eng, P, w):
    ida, kind = eng
    rng = np.random.default_rng(1000 * P + w)
    nq = S(kind, 5, 300)
    lists = random_lists(rng, P, nq, w)
    total = P * w
    # out_width below, equal to and above what the lists hold (and the lists' own width)
    widths = sorted({max(1, w // 2), w, min(4096, max(1, total - 1)), min(4096, total), min(4096, total + 9)})
    for i, ow in enumerate(widths):
        check_merge(kind, lists, ow, with_counters=(i % 2 == 0))
    # every list full: out_width == the number of results exactly
    check_merge(kind, random_lists(rng, P, S(kind, 2, 50), w, full=True), min(4096, total))


def test_merge_kernel_all_lists_empty(eng):
    ida, kind = eng
    rng = np.random.default_rng(5)
    pid, bits, count, counters, base = random_lists(rng, 3, 4, 16)
    count[:] = 0
    check_merge(kind, (pid, bits, count, counters, base), 16)


def test_merge_kernel_beyond_lds(eng):
    """64 x 1024 keys per query (512 KB) cannot be staged in LDS: the same ranking over the lists where they are."""
    ida, kind = eng
    rng = np.random.default_rng(77)
    lists = random_lists(rng, 64, S(kind, 2, 24), 1024)
    check_merge(kind, lists, 100)
    check_merge(kind, lists, 4096, with_counters=False)


@pytest.mark.gpu
@pytest.mark.parametrize("form, w, m", [("lds", 7, 521), ("beyond lds", 2710, 17)])
def test_merge_kernel_past_the_grid_gpu(engine_loader, form, w, m):
    """more queries than workgroups: a workgroup merges query q, then q + 16,384 with the same LDS head (len_s, base_s) and, in the LDS
    form, the same key region.  m distinct rows of random_lists, row q of the batch = row q % m (16,384 % m != 0: the two queries of a
    workgroup differ), the expected rows from merge_reference over the m.  P = 3; w = 2710: 3 x 2710 keys do not fit the LDS budget."""
    # cap: min(nq, 16384) workgroups of one query each, launch_merge (idist_capi.hip)
    engine_loader("gpu")
    P, nq = 3, 16384 + 37
    assert (P * w * 8 + 512 > 64 * 1024) == (form == "beyond lds") and 16384 % m
    rng = np.random.default_rng(600 + w)
    pid, bits, count, counters, base = random_lists(rng, P, m, w)
    rows = np.arange(nq) % m
    ow = 7 if form == "lds" else 100
    got = run_merge("gpu", pid, bits, count, counters, base, ow, nq=nq)          # (1.07 GB of lists on the device in the beyond-LDS form:
    #  nq > 16,384 rows of more than 8,128 keys is what that form past the grid takes; they are tiled there, never made on the host)
    want = merge_reference(pid, bits, count, counters, base, ow)
    assert not np.array_equal(want[0][0], want[0][16384 % m])                        # the two queries of workgroup 0 differ
    for g, x, name in zip(got, want, ("global ids", "distance bits", "count", "counters")):
        assert np.array_equal(g, x[rows]), (form, name)


def test_merge_kernel_rejects_bad_shapes(eng):
    ida, kind = eng
    from instant_distance_amd import _capi

    L = _capi.lib()
    a = np.zeros(64, np.uint32)
    p = a.ctypes.data
    for P, w, ow in ((0, 4, 4), (65, 4, 4), (2, 0, 4), (2, 4097, 4), (2, 4, 0), (2, 4, 4097)):
        st = L.idist_merge_topk_device(p, p, p, None, P, 1, w, _capi.u32p(a), ow, p, p, p, None, 0, None)
        assert st == 1, (P, w, ow)


# ---- helpers for the index-level cases ------------------------------------------------------------------------------------
def uneven_bounds(n, P):
    """cut [0, n) into P contiguous parts of different sizes (part p ~ p + 1 shares)"""
    shares = np.arange(1, P + 1, dtype=np.float64)
    cuts = np.floor(n * np.cumsum(shares) / shares.sum()).astype(int)
    return [0] + [int(c) for c in cuts[:-1]] + [n]


def merged_oracle_search(oixs, q, ef, threads=1):
    """oracle search per part, merged in numpy by (distance bits, global id)."""
    res = [o.search(q, threads=threads) for o in oixs]
    base = np.concatenate([[0], np.cumsum([o.n for o in oixs])[:-1]]).astype(np.uint32)
    pid = np.stack([r.pid for r in res])
    bits = np.stack([pc.bits(r.dist) for r in res])
    count = np.stack([r.count for r in res])
    counters = np.stack([r.counters for r in res])
    return merge_reference(pid, bits, count, counters, base, ef)


def check_partitioned_result(got, want):
    w_pid, w_bits, w_cnt, w_ctr = want
    assert np.array_equal(got.count, w_cnt)
    assert np.array_equal(got.pid, w_pid)
    assert np.array_equal(pc.bits(got.distance), w_bits)
    if got.counters is not None:
        assert np.array_equal(got.counters, w_ctr)


_GRAPHS = {}


def oracle_parts(oracle, kind, P, metric, n, dim):
    """the points, cut unevenly, and the oracle's graph of every part (cached per process: ef_search does not enter a build)"""
    key = (kind, P, metric, n, dim)
    if key not in _GRAPHS:
        rng = np.random.default_rng(4242 + P)
        pts = pc.gen_points(rng, n, dim)
        b = uneven_bounds(n, P)
        rows = [np.ascontiguousarray(pts[b[p]: b[p + 1]]) for p in range(P)]
        graphs = []
        for r in rows:
            o = oracle.Index.build(r, oracle.default_config(metric=metric), threads=1)
            graphs.append((o.zero, o.layers))
        _GRAPHS[key] = (rows, graphs)
    return _GRAPHS[key]


# ---- 2. search parity: depends on nothing but search ------------------------------------------------------------------
@pytest.mark.parametrize("ef", [100, 37])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_search_parity(eng, oracle, P, metric, ef):
    ida, kind = eng
    n, dim = S(kind, 330, 30000), S(kind, 6, 96)
    rows, graphs = oracle_parts(oracle, kind, P, metric, n, dim)
    cfg = oracle.default_config(metric=metric, ef_search=ef)
    oixs = [oracle.Index.from_arrays(r, z, l, cfg) for r, (z, l) in zip(rows, graphs)]
    hs = [ida.Hnsw.from_parts(r, z, l, ida.Builder().metric(metric).ef_search(ef)) for r, (z, l) in zip(rows, graphs)]
    ph = ida.PartitionedHnsw.from_hnsws(hs)
    info = ph.info()
    assert (info.n_parts, info.dim, info.ef_search, info.metric, info.n) == (P, dim, ef, metric, n)
    assert list(info.base[: P + 1]) == list(np.concatenate([[0], np.cumsum([len(r) for r in rows])]))
    rng = np.random.default_rng(99)
    for nq in (7, S(kind, 70, 2048)):       # narrow; wide (GPU: beyond the latency walks, the filtered thin walk runs underneath)
        q = pc.gen_points(rng, nq, dim)
        want = merged_oracle_search(oixs, q, ef, threads=8)
        check_partitioned_result(ph.search_batch(q, counters=True), want)
        check_partitioned_result(ph.search_batch(q), want)            # without counters: same lists
        assert ph.last_merge_ms() >= 0.0
        ks = ph.last_search_kernel_ms()                              # one search kernel per (non-empty) part, timed
        assert ks.shape == (P,) and np.all(ks >= 0.0)
    items = ph.search(q[0])
    assert [it.pid for it in items] == list(want[0][0, : want[2][0]])
    assert all(np.array_equal(it.point, ph[it.pid]) for it in items[:3])


# ---- 3. end to end through PartitionedHnsw.build ------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 3])
def test_build_end_to_end(eng, oracle, P):
    ida, kind = eng
    n, dim, ef, seed = S(kind, 200, 6000), S(kind, 6, 32), 50, 12345
    rng = np.random.default_rng(8)
    pts = pc.gen_points(rng, n, dim)
    ph, ids = ida.PartitionedHnsw.build(pts, ida.Builder().max_batch(1).seed(seed).ef_search(ef), parts=P)
    from instant_distance_amd.dist import shard_range

    # the id map: a bijection onto 0..n-1, consistent with part_of and __getitem__
    assert len(ph) == n and sorted(ids) == list(range(n))
    oixs = []
    for p in range(P):
        lo, hi = shard_range(n, p, P)
        out_pid, order = oracle.permutation(seed, hi - lo)
        for j in (0, (hi - lo) // 2, hi - lo - 1):
            assert ph.part_of(ids[lo + j]) == (p, int(out_pid[j]))
        permuted = np.ascontiguousarray(pts[lo:hi][order])
        oix = oracle.Index.build(permuted, oracle.default_config(ef_search=ef), threads=1)
        zero, layers = ph.parts[p].into_parts()                       # the part's graph is the oracle's for the same rows
        assert np.array_equal(zero, oix.zero) and len(layers) == len(oix.layers)
        assert all(np.array_equal(a, b) for a, b in zip(layers, oix.layers))
        oixs.append(oix)
    assert all(np.array_equal(ph[ids[i]], pts[i]) for i in range(0, n, max(1, n // 50)))
    with pytest.raises(IndexError):
        ph.part_of(n)
    for nq in (5, S(kind, 40, 1500)):
        q = pc.gen_points(rng, nq, dim)
        check_partitioned_result(ph.search_batch(q, counters=True), merged_oracle_search(oixs, q, ef, threads=8))


# ---- 4. exact search ------------------------------------------------------------------------------------------------------
def bruteforce_only(ida, rows, metric):
    """an index that can only be scanned (no graph): what the exact search needs"""
    return ida.Hnsw.from_parts(rows, np.full((len(rows), 64), INVALID, np.uint32), [], ida.Builder().metric(metric))


@pytest.mark.parametrize("data", ["random", "duplicates"])
@pytest.mark.parametrize("P", [1, 2, 3])
def test_bruteforce(eng, oracle, P, data):
    ida, kind = eng
    rng = np.random.default_rng(31 + P)
    if data == "random":
        n, dim, metric = S(kind, 220, 60000), S(kind, 10, 64), 0
        pts = pc.gen_points(rng, n, dim)
        q = pc.gen_points(rng, S(kind, 6, 300), dim)
    else:       # a handful of distinct rows: every query has masses of exact ties, within and across parts -> the id decides
        n, dim, metric = S(kind, 220, 20000), 4, 1
        pts = rng.integers(0, 2, size=(n, dim)).astype(np.float32)
        q = rng.integers(0, 2, size=(S(kind, 6, 40), dim)).astype(np.float32) + np.float32(0.5)
    b = uneven_bounds(n, P)
    hs = [bruteforce_only(ida, np.ascontiguousarray(pts[b[p]: b[p + 1]]), metric) for p in range(P)]
    ph = ida.PartitionedHnsw.from_hnsws(hs)
    pid, dist = ph.bruteforce(q, 10)
    opid, odist = oracle.bruteforce(pts, q, 10, metric=metric, threads=8)      # the concatenation IS the global-id order
    assert np.array_equal(pid, opid)
    assert np.array_equal(pc.bits(dist), pc.bits(odist))


def test_bruteforce_small_parts(eng, oracle):
    """parts with fewer than k points contribute what they have"""
    ida, kind = eng
    rng = np.random.default_rng(3)
    pts = pc.gen_points(rng, 23, 5)
    b = [0, 3, 3, 9, 23]                                                # 3, 0, 6 and 14 points
    hs = [bruteforce_only(ida, np.ascontiguousarray(pts[b[p]: b[p + 1]]).reshape(-1, 5), 0) for p in range(4)]
    ph = ida.PartitionedHnsw.from_hnsws(hs)
    q = pc.gen_points(rng, 4, 5)
    pid, dist = ph.bruteforce(q, 10)
    opid, odist = oracle.bruteforce(pts, q, 10, threads=1)
    assert np.array_equal(pid, opid) and np.array_equal(pc.bits(dist), pc.bits(odist))


# ---- 5. edges -------------------------------------------------------------------------------------------------------------
def test_one_part_is_the_identity(eng, oracle):
    ida, kind = eng
    rng = np.random.default_rng(2)
    n, dim = S(kind, 180, 5000), S(kind, 7, 48)
    pts = pc.gen_points(rng, n, dim)
    h = ida.Hnsw.from_ordered_points(pts, ida.Builder())
    ph = ida.PartitionedHnsw.from_hnsws([h])
    for nq in (1, 9, S(kind, 50, 1500)):
        q = pc.gen_points(rng, nq, dim)
        a, b = ph.search_batch(q, counters=True), h.search_batch(q, ida.Search(), counters=True)
        assert np.array_equal(a.pid, b.pid) and np.array_equal(a.count, b.count) and np.array_equal(a.counters, b.counters)
        assert np.array_equal(pc.bits(a.distance), pc.bits(b.distance))


def test_fewer_points_than_parts(eng, oracle):
    ida, kind = eng
    rng = np.random.default_rng(4)
    pts = pc.gen_points(rng, 3, 5)
    ph, ids = ida.PartitionedHnsw.build(pts, ida.Builder().seed(1), parts=5)      # two of the five parts are empty
    assert sorted(ids) == [0, 1, 2] and len(ph) == 3 and [len(p) for p in ph.parts].count(0) == 2
    q = pc.gen_points(rng, 4, 5)
    r = ph.search_batch(q, counters=True)
    assert np.array_equal(r.count, np.full(4, 3))
    opid, odist = oracle.bruteforce(np.stack([ph[g] for g in range(3)]), q, 3)
    assert np.array_equal(r.pid[:, :3], opid) and np.array_equal(pc.bits(r.distance[:, :3]), pc.bits(odist))
    assert np.all(r.pid[:, 3:] == INVALID) and np.all(np.isposinf(r.distance[:, 3:]))
    # no points at all
    ph0, ids0 = ida.PartitionedHnsw.build(np.zeros((0, 5), np.float32), ida.Builder(), parts=2)
    r0 = ph0.search_batch(q)
    assert ids0 == [] and np.all(r0.count == 0) and np.all(r0.pid == INVALID)


def test_no_queries(eng):
    ida, kind = eng
    pts = np.random.default_rng(0).random((40, 4), dtype=np.float32)
    ph, _ = ida.PartitionedHnsw.build(pts, ida.Builder(), parts=2)
    r = ph.search_batch(np.zeros((0, 4), np.float32), counters=True)
    assert r.pid.shape == (0, 100) and r.count.shape == (0,) and r.counters.shape == (0, 3)
    assert ph.bruteforce(np.zeros((0, 4), np.float32), 5)[0].shape == (0, 5)


def test_mismatching_parts_are_refused(eng):
    ida, kind = eng
    rng = np.random.default_rng(6)
    mk = lambda n, dim, b: ida.Hnsw.from_ordered_points(rng.random((n, dim), dtype=np.float32), b)   # noqa: E731
    a, b3, c = mk(40, 4, ida.Builder()), mk(40, 3, ida.Builder()), mk(40, 4, ida.Builder().ef_search(50))
    m = mk(40, 4, ida.Builder().metric(1))
    for bad in ([a, b3], [a, c], [a, m], [], [a] * 65):
        with pytest.raises(ida.IdistError) as e:
            ida.PartitionedHnsw.from_hnsws(bad)
        assert e.value.status == 1
    # 64 parts are legal (the same index may appear more than once: the parts are only read)
    assert ida.PartitionedHnsw.from_hnsws([a] * 64).info().n == 64 * 40
    # ... and the check is made again at every search: ef_search of one part changed afterwards
    a2 = mk(40, 4, ida.Builder())
    ph = ida.PartitionedHnsw.from_hnsws([a, a2])
    q = rng.random((3, 4), dtype=np.float32)
    each = a.search_batch(q, ida.Search()).count + a2.search_batch(q, ida.Search()).count
    assert np.array_equal(ph.search_batch(q).count, np.minimum(each, 100))
    a2.set_ef_search(50)
    with pytest.raises(ida.IdistError) as e:
        ph.search_batch(q)
    assert e.value.status == 1 and "part 1" in e.value.message
    a.set_ef_search(50)                                                    # equal again: the narrower search
    r = ph.search_batch(q)
    assert r.pid.shape == (3, 50) and np.all(r.count <= 50) and np.all(r.count >= 1)


def test_tie_overflow_never_escapes(eng, oracle):
    """Dense integer grid (`gen_points(rng, n, 3, "grid")`, the recipe of test_parity's tie tests): masses of un-expanded
    candidates tie at the furthest distance, so a device-pointer launch of a part answers "enqueue again" — the partitioned
    call does that itself (strict policy, wide batch) and returns the oracle's merge, no error.  With the default 64-entry
    region (GPU size) and with a ONE-entry region, which this data overflows in at least one part: a fresh context under
    the DROP policy flags it."""
    ida, kind = eng
    rng = np.random.default_rng(3000002)
    n, ef = S(kind, 420, 41640), S(kind, 8, 100)
    pts = pc.gen_points(rng, n, 3, "grid")
    q = np.ascontiguousarray(pts[: S(kind, 12, 1500)] + np.float32(0.25))
    cfg = oracle.default_config(metric=1, ef_search=ef, ef_construction=S(kind, 8, 64))
    b = uneven_bounds(n, 2)
    rows = [np.ascontiguousarray(pts[b[p]: b[p + 1]]) for p in range(2)]
    oixs = [oracle.Index.build(r, cfg, threads=4) for r in rows]
    want = merged_oracle_search(oixs, q, ef, threads=8)
    for cap in S(kind, (1,), (0, 1)):
        mk = lambda: ida.Builder().metric(1).ef_search(ef).tie_capacity(cap)   # noqa: E731
        hs = [ida.Hnsw.from_parts(r, o.zero, o.layers, mk()) for r, o in zip(rows, oixs)]
        ph = ida.PartitionedHnsw.from_hnsws(hs)
        check_partitioned_result(ph.search_batch(q, counters=True), want)
        check_partitioned_result(ph.search_batch(q[:5], counters=True), tuple(x[:5] for x in want))   # the contexts keep their room
        if cap == 1:
            flagged = []
            for r, o in zip(rows, oixs):
                hd = ida.Hnsw.from_parts(r, o.zero, o.layers, mk().tie_policy(ida.TIES_DROP))
                sd = ida.Search()
                hd.search_batch(q, sd)
                flagged.append(sd.tie_overflowed())
            assert any(flagged)          # at least one part's launch had to be repeated


# ---- 6. two devices -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 5])
def test_two_devices_gpu(engine_loader, oracle, P):
    ida = engine_loader("gpu")
    from instant_distance_amd import _capi

    if _capi.lib().device_count() < 2:
        pytest.skip("needs two GPUs")
    metric, ef, n, dim = 0, 100, 30000, 96
    rows, graphs = oracle_parts(oracle, "gpu", P, metric, n, dim)
    cfg = oracle.default_config(metric=metric, ef_search=ef)
    oixs = [oracle.Index.from_arrays(r, z, l, cfg) for r, (z, l) in zip(rows, graphs)]
    hs = [ida.Hnsw.from_parts(r, z, l, ida.Builder().ef_search(ef).device(p % 2)) for p, (r, (z, l)) in enumerate(zip(rows, graphs))]
    ph = ida.PartitionedHnsw.from_hnsws(hs)
    rng = np.random.default_rng(99)
    for nq in (7, 2048):
        q = pc.gen_points(rng, nq, dim)
        check_partitioned_result(ph.search_batch(q, counters=True), merged_oracle_search(oixs, q, ef, threads=8))
