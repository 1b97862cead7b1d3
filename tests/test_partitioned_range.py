"""Range search over a partitioned index (idist_partitioned_search_batch_range / idist_partitioned_range_fetch, include/idist.h;
DESIGN.md sections 4.9 and 8.1) and the merge kernels behind it (idist_range_merge_device).

The call is DEFINED by composing two exact things: row q is the merge, by the u64 key (raw distance bits, global id), of what the
single-index range search returns for query q on every non-empty part, the metric's report applied once, after the merge.  So
everything is compared exactly (lims, ids, rungs and counters with array_equal, distances as bit patterns), and the expected arrays
come from `RCase.model` of tests/test_range.py — the oracle's searches and brute force — applied per part and a numpy merge in this
file that lexsorts (raw bits, global id) per query, never from the new call.  Every case runs on the CPU emulator and (-m gpu) on the
MI355X."""
import atexit
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params
from test_allowed import Case, ladder
from test_cosine import np_normalize
from test_dot import np_augment, np_norms, np_queries
from test_partitioned import DeviceMem, uneven_bounds
from test_partitioned_allowed import SerialCase, main_parts
from test_range import EXACT, KINDS, NAN_BITS, NONE, RCase, radii_of

FILL = 0xABABABAB


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


def S(kind, emu, gpu):
    return gpu if kind == "gpu" else emu


# ---- the definition, restated ------------------------------------------------------------------------------------------------------
class PCase(RCase):
    """RCase for one PART: DOT rows are augmented with the bound of the WHOLE set (`bound`), and a graph the oracle has built already
    (`case`, over the rows as the kernels see them) is taken as it is.  `model` is RCase's, the very code."""

    def __init__(self, oracle, raw, q, ef, metric="l2sq", bound=0.0, case=None):
        self.raw, self.q, self.ef, self.mname = np.ascontiguousarray(raw), np.ascontiguousarray(q), ef, metric
        km = 0
        if metric == "cosine":
            rows, qt = np_normalize(oracle, raw)[0], np_normalize(oracle, q)[0]
        elif metric == "dot":
            rows, self.Sb, _ = np_augment(oracle, raw, bound)
            qt, self.sq = np_queries(q), np_norms(oracle, q)
        else:
            rows, qt, km = self.raw, self.q, (1 if metric == "l2" else 0)
        self.c = case if case is not None else Case(oracle, rows, qt, ef, metric=km)
        n = len(rows)
        bp, bd = oracle.bruteforce(rows, qt, n, metric=km, threads=8)
        b = np.where(np.isnan(bd), np.uint32(NAN_BITS), pc.bits(bd))
        order = np.stack([np.lexsort((bp[i], b[i])) for i in range(len(qt))]) if len(qt) else np.zeros((0, n), np.int64)
        self.all_pid = np.take_along_axis(bp, order, axis=1)
        self.all_d = np.take_along_axis(np.ascontiguousarray(bd, dtype=np.float32), order, axis=1)
        self.all_rep = np.stack([self.report(self.all_d[i], i) for i in range(len(qt))]) if len(qt) else self.all_d

    def model_raw(self, radii, max_rungs=-1, queries=None):
        """RCase.model, and the RAW distance bits of what it returns: a rung's answer is a prefix of that rung's list, the exact
        answer a prefix of all rows by (raw bits, id) — the report is monotone"""
        lims, pid, _, rung, ctr = self.model(radii, max_rungs, queries)
        qs = range(len(self.q)) if queries is None else queries
        E = ladder(self.ef)
        raw = []
        for i, qi in enumerate(qs):
            lo, c = int(lims[i]), int(lims[i + 1] - lims[i])
            if rung[i] == EXACT:
                assert np.array_equal(self.all_pid[qi][:c], pid[lo: lo + c])
                raw.append(self.all_d[qi][:c])
            else:
                res = self.c.rung(E[int(rung[i])])
                assert np.array_equal(res.pid[qi, :c], pid[lo: lo + c])
                raw.append(res.dist[qi, :c])
        raw = np.concatenate(raw).astype(np.float32) if raw else np.zeros(0, np.float32)
        return lims, pid, pc.bits(raw), rung, ctr


def expected(rcs, b, radii, max_rungs=-1, queries=None):
    """rcs[p]: the PCase of part p (None: an empty part), b: the parts' bounds.  Per part the model, ids local, raw distances; then per
    query the numpy merge: lexsort by (raw bits, global id), the report of the query applied to the merged raw distances.
    -> (lims, global ids, reported distance bits, rung [nq][P], counters summed)"""
    P = len(rcs)
    first = next(rc for rc in rcs if rc is not None)
    qs = list(range(len(first.q))) if queries is None else list(queries)
    nq = len(qs)
    parts = [rc.model_raw(radii, max_rungs, qs) if rc is not None else None for rc in rcs]
    rung = np.full((nq, P), NONE, np.uint32)
    ctr = np.zeros((nq, 3), np.uint32)
    for p, w in enumerate(parts):
        if w is not None:
            rung[:, p] = w[3]
            ctr += w[4]
    pids, reps, cnt = [], [], np.zeros((nq, P), np.int64)
    for i, qi in enumerate(qs):
        g, d = [], []
        for p, w in enumerate(parts):
            if w is None:
                continue
            lo, hi = int(w[0][i]), int(w[0][i + 1])
            cnt[i, p] = hi - lo
            g.append(w[1][lo:hi].astype(np.uint64) + np.uint64(b[p]))
            d.append(w[2][lo:hi])
        g, d = np.concatenate(g), np.concatenate(d)
        order = np.lexsort((g, d))
        pids.append(g[order].astype(np.uint32))
        reps.append(pc.bits(first.report(d[order].view(np.float32), qi)))
    lims = np.concatenate([[0], np.cumsum([len(x) for x in pids])]).astype(np.uint64)
    pid = np.concatenate(pids) if pids else np.zeros(0, np.uint32)
    rep = np.concatenate(reps) if reps else np.zeros(0, np.uint32)
    return (lims, pid, rep, rung, ctr), cnt


def check(got, want, what=""):
    w_lims, w_pid, w_bits, w_rung, w_ctr = want
    assert got.rung.shape == w_rung.shape, f"{what}: rung shape {got.rung.shape}"
    assert np.array_equal(got.rung, w_rung), f"{what}: rungs {np.unique(got.rung, return_counts=True)} != {np.unique(w_rung, return_counts=True)}"
    assert got.lims.dtype == np.uint64 and np.array_equal(got.lims, w_lims), f"{what}: lims"
    assert np.array_equal(got.pid, w_pid), f"{what}: ids"
    assert np.array_equal(pc.bits(got.distance), w_bits), f"{what}: distance bits"
    if got.counters is not None:
        assert np.array_equal(got.counters, w_ctr), f"{what}: counters"


def whole(rcs, b, pts):
    """what radii_of needs of the WHOLE set: every row's reported distance per query, by (raw bits, global id)"""
    first = next(rc for rc in rcs if rc is not None)
    nq = len(first.q)
    live = [(p, rc) for p, rc in enumerate(rcs) if rc is not None]
    g = np.concatenate([rc.all_pid.astype(np.uint64) + np.uint64(b[p]) for p, rc in live], axis=1)
    d = np.concatenate([rc.all_d for p, rc in live], axis=1)
    db = np.where(np.isnan(d), np.uint32(NAN_BITS), pc.bits(d))
    order = np.stack([np.lexsort((g[i], db[i])) for i in range(nq)])
    all_d = np.take_along_axis(d, order, axis=1)
    all_pid = np.take_along_axis(g, order, axis=1).astype(np.uint32)
    all_rep = np.stack([first.report(all_d[i], i) for i in range(nq)])
    return SimpleNamespace(raw=pts, q=first.q, ef=first.ef, mname=first.mname, all_rep=all_rep, all_pid=all_pid, all_d=all_d)


_RPARTS = {}
atexit.register(_RPARTS.clear)      # (the oracle's handles go before the interpreter takes its library apart)


def range_parts(oracle, kind, P):
    """the parts of tests/test_partitioned_allowed.py (660 x 8-d, ef_search 8, 24 queries / 12,000 x 32-d, ef_search 16, 600 queries, cut
    by uneven_bounds; their graphs and rungs are shared with that file) -> (pts, q, bounds, PCases, the whole set)"""
    if (kind, P) not in _RPARTS:
        pts, q, b, cs, _ = main_parts(oracle, kind, P)
        rcs = [PCase(oracle, c.pts, q, c.ef, case=c) for c in cs]
        _RPARTS[kind, P] = (pts, q, b, rcs, whole(rcs, b, pts))
    return _RPARTS[kind, P]


def requeried(oracle, rc, q2):
    """the part of `rc` — the same graph — under other queries"""
    c = Case.__new__(Case)
    c.__dict__.update(rc.c.__dict__, q=np.ascontiguousarray(q2), _rungs={})
    return PCase(oracle, rc.raw, q2, rc.ef, case=c)


def partitioned(ida, rcs, builder=None):
    hs = [rc.hnsw(ida, builder() if builder else None) for rc in rcs]
    return ida.PartitionedHnsw.from_hnsws(hs), hs


# ---- 1. the merge kernels alone ------------------------------------------------------------------------------------------------------
def synthetic_lists(rng, P, nq, lens):
    """lens [P][nq].  Per list ONE key buffer: the queries' ascending segments in a random (completion) order with garbage between
    them that would win if it were read (key 0); distance bits from a small pool, so that the same bits meet across lists and the
    global id decides.  -> (key buffers, offsets [P][nq] u64, base [P], per query the expected (gid, bits) arrays)"""
    sizes = np.maximum(lens.max(axis=1), 1) + rng.integers(1, 9, size=P)
    base = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint32)
    pool = np.sort(rng.random(48, dtype=np.float32)).view(np.uint32)
    pool = np.concatenate([pool, np.full(2, 0x7F800000, np.uint32)])                # +inf is a real result
    bufs, offs = [], np.zeros((P, nq), np.uint64)
    gid = [[] for _ in range(nq)]
    bits = [[] for _ in range(nq)]
    for l in range(P):
        chunks, at = [], 0
        for q in rng.permutation(nq):
            gap = int(rng.integers(0, 4))
            chunks.append(np.zeros(gap, np.uint64))
            at += gap
            c = int(lens[l, q])
            ids = rng.choice(int(sizes[l]), size=c, replace=False).astype(np.uint64)
            d = rng.choice(pool, size=c).astype(np.uint64)
            key = np.sort((d << np.uint64(32)) | ids)
            offs[l, q] = at
            chunks.append(key)
            at += c
            gid[q].append((key & np.uint64(0xFFFFFFFF)) + np.uint64(base[l]))
            bits[q].append((key >> np.uint64(32)).astype(np.uint32))
        chunks.append(np.zeros(2, np.uint64))
        bufs.append(np.concatenate(chunks))
    want = []
    for q in range(nq):
        g, d = np.concatenate(gid[q]), np.concatenate(bits[q])
        order = np.lexsort((g, d))
        want.append((g[order].astype(np.uint32), d[order]))
    return bufs, offs, base, want


def run_range_merge(kind, bufs, offs, lens, base, capacity, metric=0, sq=None, dot_bound=0.0):
    """-> (status, lims, pid, distance bits, total): the outputs start as a pattern no result holds"""
    from instant_distance_amd import _capi

    P, nq = lens.shape
    mem = DeviceMem(kind)
    try:
        d_keys = (C.c_void_p * P)(*[mem.up(x) for x in bufs])
        d_off = (C.c_void_p * P)(*[mem.up(np.ascontiguousarray(offs[l])) for l in range(P)])
        d_cnt = (C.c_void_p * P)(*[mem.up(np.ascontiguousarray(lens[l].astype(np.uint32))) for l in range(P)])
        o_lims = np.full(nq + 1, 0xABABABABABABABAB, np.uint64)
        o_pid, o_dist = np.full(capacity + 9, FILL, np.uint32), np.full(capacity + 9, FILL, np.uint32)
        d_lims, d_pid, d_dist = mem.up(o_lims), mem.up(o_pid), mem.up(o_dist)
        d_sq = mem.up(np.ascontiguousarray(sq, dtype=np.float32)) if sq is not None else None
        total = C.c_uint64(0)
        L = _capi.lib()
        st = L.idist_range_merge_device(d_keys, d_off, d_cnt, P, nq, _capi.u32p(np.ascontiguousarray(base, dtype=np.uint32)), metric, d_sq,
                                        dot_bound, capacity, d_lims, d_pid, d_dist, C.byref(total), 0, None)
        res = [mem.down(p, like).copy() for p, like in ((d_lims, o_lims), (d_pid, o_pid), (d_dist, o_dist))]
    finally:
        mem.free()
    return st, res[0], res[1], res[2], int(total.value)


def batch_lengths(rng, P, nq, kind):
    """0, 1, 63, 64, 65 and a few thousand in one batch; query 3 owns a list of several thousand, its neighbours 2 and 4 nothing at all"""
    lens = rng.choice([0, 0, 1, 63, 64, 65], size=(P, nq))
    lens[:, 2] = lens[:, 4] = 0
    lens[:, 3] = 0
    lens[0, 3] = S(kind, 2500, 9000)
    if P > 1:
        lens[1, 3] = S(kind, 1300, 4097)
        lens[P - 1, 3] = 70
    return lens


def check_range_merge(kind, rng, lens):
    bufs, offs, base, want = synthetic_lists(rng, *lens.shape, lens)
    total = int(lens.sum())
    st, lims, pid, dist, got_total = run_range_merge(kind, bufs, offs, lens, base, total)
    assert st == 0 and got_total == total
    assert np.array_equal(lims, np.concatenate([[0], np.cumsum(lens.sum(axis=0))]).astype(np.uint64))
    w_pid = np.concatenate([w[0] for w in want]) if total else np.zeros(0, np.uint32)
    w_bits = np.concatenate([w[1] for w in want]) if total else np.zeros(0, np.uint32)
    assert np.array_equal(pid[:total], w_pid), "global ids"         # every slot below the total is written ...
    assert np.array_equal(dist[:total], w_bits), "distance bits"
    assert np.all(pid[total:] == FILL) and np.all(dist[total:] == FILL)     # ... and nothing beyond it
    return bufs, offs, base, want


@pytest.mark.parametrize("P", [1, 2, 5, 64])
def test_merge_kernels(eng, P):
    ida, kind = eng
    rng = np.random.default_rng(500 + P)
    nq = 11
    lens = batch_lengths(rng, P, nq, kind)
    assert {0, 1, 63, 64, 65} <= set(lens.ravel().tolist()) or P < 5
    bufs, offs, base, want = check_range_merge(kind, rng, lens)
    total = int(lens.sum())
    # a capacity one short of the total is refused, and nothing is written
    from instant_distance_amd import _capi
    st, lims, pid, dist, got_total = run_range_merge(kind, bufs, offs, lens, base, total - 1)
    assert st == 1 and got_total == total and str(total).encode() in _capi.lib().idist_last_error()
    assert np.all(pid == FILL) and np.all(dist == FILL)


def test_merge_kernels_every_length_in_one_list_each(eng):
    """P = 5 lists that hold 0, 1, 63, 64, 65 keys of the same query; a second query with the lengths rotated"""
    ida, kind = eng
    rng = np.random.default_rng(9)
    lens = np.array([[0, 65], [1, 0], [63, 1], [64, 63], [65, 64]])
    check_range_merge(kind, rng, lens)


def test_merge_kernels_all_lists_empty(eng):
    ida, kind = eng
    rng = np.random.default_rng(5)
    lens = np.zeros((3, 4), np.int64)
    bufs, offs, base, _ = synthetic_lists(rng, 3, 4, lens)
    st, lims, pid, dist, total = run_range_merge(kind, bufs, offs, lens, base, 0)
    assert st == 0 and total == 0 and np.all(lims == 0) and np.all(pid == FILL) and np.all(dist == FILL)


def synthetic_lists_flat(rng, P, nq, lens):
    """synthetic_lists without a Python loop over the queries, for batches of thousands to millions: the same key buffers (ascending
    segments in a random completion order, zero keys between them, distance bits from a small pool so that the global id decides)
    -> (key buffers, offsets [P][nq] u64, base [P], the expected flat global ids, the expected flat distance bits)"""
    sizes = np.maximum(lens.max(axis=1), 1) + rng.integers(1, 9, size=P)
    base = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint32)
    pool = np.sort(rng.random(48, dtype=np.float32)).view(np.uint32)
    pool = np.concatenate([pool, np.full(2, 0x7F800000, np.uint32)])
    bufs, offs = [], np.zeros((P, nq), np.uint64)
    all_q, all_g, all_d = [], [], []
    for l in range(P):
        c = lens[l].astype(np.int64)
        qidx = np.repeat(np.arange(nq), c)
        first = np.concatenate([[0], np.cumsum(c)[:-1]])
        j = np.arange(len(qidx)) - first[qidx]
        ids = ((rng.integers(0, int(sizes[l]), size=nq)[qidx] + j) % int(sizes[l])).astype(np.uint64)   # distinct within a segment: c <= sizes[l]
        key = (rng.choice(pool, size=len(qidx)).astype(np.uint64) << np.uint64(32)) | ids
        key = key[np.lexsort((key, qidx))]                                          # every segment ascending
        perm = rng.permutation(nq)
        gap = rng.integers(0, 4, size=nq)
        start = np.zeros(nq, np.int64)
        start[perm] = np.cumsum(gap + c[perm]) - c[perm]
        buf = np.zeros(int(c.sum() + gap.sum()) + 2, np.uint64)
        buf[start[qidx] + j] = key
        offs[l] = start.astype(np.uint64)
        bufs.append(buf)
        all_q.append(qidx)
        all_g.append((key & np.uint64(0xFFFFFFFF)) + np.uint64(base[l]))
        all_d.append((key >> np.uint64(32)).astype(np.uint32))
    qs, g, d = np.concatenate(all_q), np.concatenate(all_g), np.concatenate(all_d)
    order = np.lexsort((g, d, qs))
    return bufs, offs, base, g[order].astype(np.uint32), d[order]


def check_range_merge_flat(kind, rng, lens):
    """check_range_merge's assertions on a wide batch"""
    bufs, offs, base, w_pid, w_bits = synthetic_lists_flat(rng, *lens.shape, lens)
    total = int(lens.sum())
    st, lims, pid, dist, got_total = run_range_merge(kind, bufs, offs, lens, base, total)
    assert st == 0 and got_total == total
    assert np.array_equal(lims, np.concatenate([[0], np.cumsum(lens.sum(axis=0))]).astype(np.uint64)), "lims"
    assert np.array_equal(pid[:total], w_pid), "global ids"
    assert np.array_equal(dist[:total], w_bits), "distance bits"
    assert np.all(pid[total:] == FILL) and np.all(dist[total:] == FILL)


def test_synthetic_lists_flat_rows_are_the_merge_of_its_buffers():
    """the vectorised model's expected rows, derived again query by query from the buffers, offsets and bases it returned"""
    rng = np.random.default_rng(77)
    lens = rng.choice([0, 1, 2, 65], size=(3, 40))
    bufs, offs, base, w_pid, w_bits = synthetic_lists_flat(rng, 3, 40, lens)
    g, d = [], []
    for q in range(40):
        keys = [bufs[l][int(offs[l, q]): int(offs[l, q]) + int(lens[l, q])] for l in range(3)]
        assert all(np.all(k[:-1] < k[1:]) for k in keys)                            # ascending, no id twice
        gq = np.concatenate([(k & np.uint64(0xFFFFFFFF)) + np.uint64(base[l]) for l, k in enumerate(keys)])
        dq = np.concatenate([(k >> np.uint64(32)).astype(np.uint32) for k in keys])
        order = np.lexsort((gq, dq))
        g.append(gq[order].astype(np.uint32))
        d.append(dq[order])
    assert np.array_equal(np.concatenate(g), w_pid) and np.array_equal(np.concatenate(d), w_bits)


@pytest.mark.parametrize("nq", [4095, 4096, 4097, 8193])
@pytest.mark.parametrize("P", [1, 3])
def test_merge_kernels_second_level_of_the_prefix_sum(eng, P, nq):
    """range_offsets_kernel sums the chunk sums in front of its chunk with `for (c = lane; c < b; c += 64)`: chunk b has b chunks in
    front of it, so the loop's second trip needs a chunk b > 64, that is nq > 65 x 64 = 4,160 — of these shapes 8193 alone (129
    chunks); 4095, 4096 and 4097 stand on both sides of the last full first trip.  Lengths from {0, 1, 2, 65}."""
    # cap: 64 lanes, one chunk of 64 items each, per trip of the chunk loop in range_offsets_kernel (idist_range.hpp), launched by range_prefix_on
    ida, kind = eng
    rng = np.random.default_rng(8000 + 10 * nq + P)
    lens = rng.choice([0, 1, 2, 65], size=(P, nq), p=[0.4, 0.3, 0.2, 0.1])
    assert {0, 1, 2, 65} <= set(lens.ravel().tolist())
    check_range_merge_flat(kind, rng, lens)


@pytest.mark.gpu
def test_merge_kernels_past_the_prefix_sum_grid_gpu(engine_loader):
    """the first batch at which range_prefix_on's grid strides: more than 65,536 chunks of 64 queries; lengths 0 / 1"""
    # cap: min(chunks, 65536) workgroups of 64 items, range_prefix_on (idist_capi.hip); range_merge_counts_kernel (n_cu * 8 x 256 rows,
    # launch_range_merge_counts) and range_merge_kernel (n_cu * 32 tiles, launch_range_merge) stride at this size too
    engine_loader("gpu")
    nq = 64 * 65536 + 37
    rng = np.random.default_rng(8100)
    lens = rng.integers(0, 2, size=(2, nq))
    check_range_merge_flat("gpu", rng, lens)


def test_merge_kernels_report(eng):
    """the report runs in the merge kernel: cosine halves, DOT subtracts the query's own term s(q) + S"""
    ida, kind = eng
    rng = np.random.default_rng(6)
    lens = rng.choice([0, 3, 70], size=(3, 5))
    bufs, offs, base, want = synthetic_lists(rng, 3, 5, lens)
    total = int(lens.sum())
    sq, Sb = rng.random(5, dtype=np.float32), np.float32(7.25)
    w_raw = np.concatenate([w[1] for w in want]).view(np.float32)
    per_q = np.repeat(np.arange(5), lens.sum(axis=0))
    st, _, _, dist, _ = run_range_merge(kind, bufs, offs, lens, base, total, metric=2)
    assert st == 0 and np.array_equal(dist[:total], pc.bits(np.float32(0.5) * w_raw))
    st, _, _, dist, _ = run_range_merge(kind, bufs, offs, lens, base, total, metric=4, sq=sq, dot_bound=float(Sb))
    t = (sq + Sb).astype(np.float32)[per_q]
    with np.errstate(all="ignore"):
        w = np.where(np.isposinf(w_raw), w_raw, np.float32(0.5) * (w_raw - t))
    assert st == 0 and w.dtype == np.float32 and np.array_equal(dist[:total], pc.bits(w))


def test_merge_does_not_depend_on_the_tile(eng, monkeypatch):
    """a wave's tile of 64 elements: every long list is cut over many waves, most tiles span several queries and lists"""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    rng = np.random.default_rng(12)
    lens = batch_lengths(rng, 5, 11, "emu")
    for tile in ("64", "128", "1024"):
        monkeypatch.setenv("IDIST_RANGE_MERGE_TILE", tile)
        check_range_merge(kind, np.random.default_rng(13), lens)


def test_merge_kernels_reject_bad_arguments(eng):
    ida, kind = eng
    from instant_distance_amd import _capi

    L = _capi.lib()
    a = np.zeros(8, np.uint64)
    one = (C.c_void_p * 1)(a.ctypes.data)
    base, total = np.zeros(1, np.uint32), C.c_uint64(0)
    p = a.ctypes.data

    def status(n_lists=1, metric=0, keys=one, lims=p, d_sq=None):
        return L.idist_range_merge_device(keys, one, one, n_lists, 1, _capi.u32p(base), metric, d_sq, 0.0, 0, lims, p, p, C.byref(total), 0, None)

    assert status(n_lists=0) == 1 and status(n_lists=65) == 1 and status(metric=7) == 1
    assert status(keys=None) == 1 and status(lims=None) == 1 and status(metric=4) == 1


# ---- 2. parity with the definition ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_parity_with_the_definition(eng, oracle, P):
    ida, kind = eng
    pts, q, b, rcs, w = range_parts(oracle, kind, P)
    ph, hs = partitioned(ida, rcs)
    rad = radii_of(w)
    seen, split = set(), False
    for max_rungs in (-1, 2):
        want, cnt = expected(rcs, b, rad, max_rungs)
        print("max_rungs", max_rungs, "rungs", dict(zip(*[x.tolist() for x in np.unique(want[3], return_counts=True)])))
        got = ph.search_range(q, rad, max_rungs=max_rungs, counters=True)
        assert got.rung.shape == (len(q), P)
        check(got, want, f"max_rungs {max_rungs}")
        check(ph.search_range(q, rad, max_rungs=max_rungs), want, f"max_rungs {max_rungs}, no counters")
        seen |= set(want[3].ravel().tolist())
        split = split or bool(np.any((cnt.min(axis=1) == 0) & (cnt.max(axis=1) > 0)))
    # the inputs reach the paths: rung 0, a later rung, the exact scan; a query with nothing in one part and something in another
    assert 0 in seen and len({r for r in seen if 0 < r < NONE}) >= 1 and EXACT in seen
    assert split or P == 1
    assert ph.last_range_merge_ms() >= 0.0 and ph.last_search_kernel_ms().shape == (P,)
    # one query
    want1, _ = expected(rcs, b, rad[5:6], -1, queries=[5])
    items = ph.search_one_range(q[5], rad[5])
    assert [it.pid for it in items] == want1[1].tolist() and len(items) == int(want1[0][1]) > 0
    assert np.array_equal(pc.bits(np.array([it.distance for it in items], np.float32)), want1[2])
    assert all(np.array_equal(it.point, pts[it.pid]) for it in items)


# ---- 3. max_rungs --------------------------------------------------------------------------------------------------------------------
def test_max_rungs(eng, oracle):
    ida, kind = eng
    pts, q, b, rcs, w = range_parts(oracle, kind, 3)
    ph, hs = partitioned(ida, rcs)
    rad = radii_of(w)
    for m in (0, 1, 2, -1):
        want, _ = expected(rcs, b, rad, m)
        got = ph.search_range(q, rad, max_rungs=m, counters=True)
        check(got, want, f"max_rungs {m}")
        assert set(want[3].ravel().tolist()) <= set(range(m if m >= 0 else 8)) | {EXACT}
        if m == 0:                                                     # ONE brute force over all rows, for every query
            assert np.all(got.rung == EXACT) and np.all(got.counters == 0)
            bp, bd = oracle.bruteforce(pts, q, len(pts), threads=8)
            for qi in range(len(q)):
                keep = bd[qi] <= rad[qi]
                ids, d = bp[qi][keep], pc.bits(bd[qi][keep])
                order = np.lexsort((ids, d))
                lo, hi = int(got.lims[qi]), int(got.lims[qi + 1])
                assert np.array_equal(got.pid[lo:hi], ids[order]) and np.array_equal(pc.bits(got.distance[lo:hi]), d[order]), qi


# ---- 4. the four metrics ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2sq", "l2", "cosine", "dot"])
def test_metrics(eng, oracle, metric):
    """radii exactly on reported values of the whole set; DOT with one large-norm row, so the bound S is large and the report rounds —
    and every part is built with the bound of the WHOLE set"""
    ida, kind = eng
    n, dim, ef, nq, P = S(kind, (300, 7, 8, 18, 3), (3000, 24, 16, 90, 3))
    rng = np.random.default_rng(11)
    raw = rng.random((n, dim), dtype=np.float32) - np.float32(0.3)
    q = rng.random((nq, dim), dtype=np.float32) - np.float32(0.3)
    bound, builder = 0.0, None
    if metric == "dot":
        raw[n // 3] *= np.float32(37.0)
        bound = float(np_augment(oracle, raw)[1])
        builder = lambda: ida.Builder().dot_bound(bound)                                # noqa: E731
    b = uneven_bounds(n, P)
    rcs = [PCase(oracle, raw[b[p]: b[p + 1]], q, ef, metric, bound=bound) for p in range(P)]
    w = whole(rcs, b, raw)
    kinds = ["below", 0, "ef-1", "ef", "ef+1", "4ef", "n/2", "inf", "neg"]
    rad = radii_of(w, kinds)
    if metric == "dot":
        assert {np.float32(rc.Sb).tobytes() for rc in rcs} == {np.float32(bound).tobytes()}      # one bound, bit for bit
        assert (rad[np.isfinite(rad)] < 0).any()                       # negative radii are meaningful here
        exact = 0.5 * (w.all_d.astype(np.float64) - (rcs[0].sq.astype(np.float64)[:, None] + float(rcs[0].Sb)))
        assert (w.all_rep.astype(np.float64) != exact).any()           # the report does round: the f32 steps matter
    ph, hs = partitioned(ida, rcs, builder)
    seen = set()
    for m in (-1, 2, 0):
        want, _ = expected(rcs, b, rad, m)
        check(ph.search_range(q, rad, max_rungs=m, counters=True), want, f"{metric}, max_rungs {m}")
        seen |= set(want[3].ravel().tolist())
    assert EXACT in seen and len(seen) >= 3
    c = np.diff(expected(rcs, b, rad, 0)[0][0].astype(np.int64))
    assert np.all(c[1::len(kinds)] >= 1) and np.all(c[0::len(kinds)] == 0)


# ---- 5. edges ----------------------------------------------------------------------------------------------------------------------------
def test_one_part_is_the_single_index(eng, oracle):
    ida, kind = eng
    pts, q, b, rcs, w = range_parts(oracle, kind, 1)
    ph, hs = partitioned(ida, rcs)
    rad = radii_of(w)
    for m in (-1, 2, 0):
        a = ph.search_range(q, rad, max_rungs=m, counters=True)
        o = hs[0].search_range(q, rad, ida.Search(), max_rungs=m, counters=True)
        assert a.rung.shape == (len(q), 1) and np.array_equal(a.rung[:, 0], o.rung)
        assert np.array_equal(a.lims, o.lims) and np.array_equal(a.pid, o.pid) and np.array_equal(a.counters, o.counters)
        assert np.array_equal(pc.bits(a.distance), pc.bits(o.distance)) and int(o.lims[-1]) > 0


def test_fewer_points_than_parts(eng, oracle):
    ida, kind = eng
    rng = np.random.default_rng(4)
    pts = pc.gen_points(rng, 3, 5)
    ph, ids = ida.PartitionedHnsw.build(pts, ida.Builder().seed(1), parts=5)      # two of the five parts are empty
    sizes_ = [len(p) for p in ph.parts]
    assert len(ph) == 3 and sizes_.count(0) == 2
    q = pc.gen_points(rng, 4, 5)
    stored = np.stack([ph[g] for g in range(3)])
    bp, bd = oracle.bruteforce(stored, q, 3)
    rad = bd[:, 1].copy()                                                          # two of the three points are within
    for m in (-1, 0):
        r = ph.search_range(q, rad, max_rungs=m, counters=True)
        assert np.array_equal(r.lims, np.arange(5, dtype=np.uint64) * 2)
        assert np.array_equal(r.pid.reshape(4, 2), bp[:, :2]) and np.array_equal(pc.bits(r.distance).reshape(4, 2), pc.bits(bd[:, :2]))
        assert r.rung.shape == (4, 5)
        for p in range(5):
            assert np.all(r.rung[:, p] == NONE) if sizes_[p] == 0 else np.all(r.rung[:, p] != NONE)
    # every part empty; ef_search == 0
    ph0, ids0 = ida.PartitionedHnsw.build(np.zeros((0, 5), np.float32), ida.Builder(), parts=2)
    r0 = ph0.search_range(q, np.inf, counters=True)
    assert np.all(r0.lims == 0) and r0.lims.shape == (5,) and r0.rung.shape == (4, 2) and np.all(r0.rung == NONE) and np.all(r0.counters == 0)
    assert r0.pid.shape == (0,)
    hz = [ida.Hnsw.from_ordered_points(np.ascontiguousarray(pts[i: i + 2]), ida.Builder().ef_search(0)) for i in (0, 1)]
    rz = ida.PartitionedHnsw.from_hnsws(hz).search_range(q, np.inf, counters=True)
    assert np.all(rz.lims == 0) and np.all(rz.rung == NONE) and np.all(rz.counters == 0)


def test_edges_of_the_call(eng, oracle):
    ida, kind = eng
    from instant_distance_amd import _capi

    pts, q, b, rcs, w = range_parts(oracle, kind, 3)
    ph, hs = partitioned(ida, rcs)
    L = _capi.lib()
    nq = 12
    q12, rad = q[:nq], radii_of(w)[:nq].copy()
    sub = list(range(nq))
    want, _ = expected(rcs, b, rad, -1, queries=sub)
    total = int(want[0][-1])
    assert total > 0
    lims, rung = np.zeros(nq + 1, np.uint64), np.zeros((nq, 3), np.uint32)
    pid, dist = np.zeros(total, np.uint32), np.zeros(total, np.float32)

    def call(radius, n_radius, max_total=1 << 40):
        return L.idist_partitioned_search_batch_range(ph._h, _capi.f32p(q12), nq, _capi.f32p(radius), n_radius, -1, max_total,
                                                      _capi.u64p(lims), _capi.u32p(rung), None)

    def fetch():
        return L.idist_partitioned_range_fetch(ph._h, _capi.u32p(pid), _capi.f32p(dist))

    assert fetch() == 1                                                            # nothing held yet
    with pytest.raises(ida.IdistError):
        ph.last_range_merge_ms()
    # nq == 0
    r0 = ph.search_range(np.zeros((0, q.shape[1]), np.float32), 1.0, counters=True)
    assert np.array_equal(r0.lims, np.zeros(1, np.uint64)) and r0.pid.shape == (0,) and r0.rung.shape == (0, 3) and r0.counters.shape == (0, 3)
    # a shared radius, as a float and as an array of one
    r = np.float32(np.median(w.all_rep[:nq]))
    want_s, _ = expected(rcs, b, r, 1, queries=sub)
    check(ph.search_range(q12, float(r), max_rungs=1, counters=True), want_s, "shared radius")
    check(ph.search_range(q12, np.array([r]), max_rungs=1), want_s, "shared radius, array of one")
    with pytest.raises(ValueError):
        ph.search_range(q12, rad[:5])
    # a NaN radius is refused and names the query; nothing is held afterwards
    bad = rad.copy()
    bad[7] = np.nan
    assert call(bad, nq) == 1 and b"query 7" in L.idist_last_error() and fetch() == 1
    with pytest.raises(ida.IdistError) as e:
        ph.search_range(q12, bad)
    assert e.value.status == 1 and "query 7" in str(e.value)
    assert call(rad, 5) == 1
    # max_total one below the true total is refused (the message says what was known), and a fetch afterwards too
    assert call(rad, nq, max_total=total - 1) == 1
    msg = L.idist_last_error().decode()
    assert "max_total" in msg and str(total - 1) in msg
    assert fetch() == 1
    with pytest.raises(ida.IdistError):
        ph.search_range(q12, rad, max_total=total - 1)
    check(ph.search_range(q12, rad, max_total=total, counters=True), want, "max_total == the total")
    # the results are handed out once
    assert call(rad, nq) == 0 and int(lims[nq]) == total and lims[0] == 0 and np.array_equal(rung, want[3])
    assert fetch() == 0
    assert np.array_equal(pid, want[1]) and np.array_equal(pc.bits(dist), want[2])
    assert fetch() == 1
    # a larger call, then fewer queries through the same handle: staging keeps its room
    rad_all = radii_of(w)
    check(ph.search_range(q, rad_all, max_rungs=0), expected(rcs, b, rad_all, 0)[0], "the whole batch, exact")
    check(ph.search_range(q[3:11], rad_all[3:11], max_rungs=1, counters=True), expected(rcs, b, rad_all[3:11], 1, queries=range(3, 11))[0],
          "then eight queries")
    # the parts are compared again at every call
    hs[1].set_ef_search(50)
    with pytest.raises(ida.IdistError) as e:
        ph.search_range(q12, rad)
    assert e.value.status == 1 and "part 1" in e.value.message
    hs[1].set_ef_search(rcs[1].ef)


def test_tie_overflow_never_escapes(eng, oracle):
    """the dense integer grid and the ONE-entry tie region of tests/test_partitioned_allowed.py, cut into two parts: rungs' launches
    overflow the region, the part searches the rung again itself and the call returns the model's arrays"""
    ida, kind = eng
    rng = np.random.default_rng(3000002)
    n, ef = S(kind, 420, 12000), 8
    pts = pc.gen_points(rng, n, 3, "grid")
    q = np.ascontiguousarray(pts[: S(kind, 12, 600)] + np.float32(0.25))
    b = uneven_bounds(n, 2)
    mk = SerialCase if kind == "emu" else Case
    rcs = []
    for p in range(2):
        rows = np.ascontiguousarray(pts[b[p]: b[p + 1]])
        rcs.append(PCase(oracle, rows, q, ef, "l2", case=mk(oracle, rows, q, ef, metric=1, ef_construction=S(kind, 8, 64))))
    w = whole(rcs, b, pts)
    rad = radii_of(w, ["ef", "4ef", 0, "ef+1", 40, 150])
    want, _ = expected(rcs, b, rad)
    assert len({r for r in want[3].ravel().tolist() if r < NONE}) >= 2             # the ladders climb
    ph, hs = partitioned(ida, rcs, lambda: ida.Builder().tie_capacity(1))
    check(ph.search_range(q, rad, counters=True), want)


# ---- 6. two devices ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 5])
def test_two_devices_gpu(engine_loader, oracle, P):
    """parts alternating over devices 0 and 1: the parts away from the merge device send keys, offsets and counts by peer copies; the
    check of the parity test at 7 queries (the whole ladder) and at 2048 (two rungs, then the exact scan)"""
    ida = engine_loader("gpu")
    from instant_distance_amd import _capi

    if _capi.lib().device_count() < 2:
        pytest.skip("needs two GPUs")
    pts, q, b, rcs, w = range_parts(oracle, "gpu", P)
    hs = [ida.Hnsw.from_parts(rc.raw, rc.c.zero, rc.c.layers, ida.Builder().ef_search(rc.ef).device(p % 2)) for p, rc in enumerate(rcs)]
    ph = ida.PartitionedHnsw.from_hnsws(hs)
    rad = radii_of(w)
    check(ph.search_range(q[:7], rad[:7], counters=True), expected(rcs, b, rad[:7], -1, queries=range(7))[0], "7 queries")
    rng = np.random.default_rng(31)
    q2 = rng.random((2048, pts.shape[1]), dtype=np.float32)
    rcs2 = [requeried(oracle, rc, q2) for rc in rcs]
    rad2 = radii_of(whole(rcs2, b, pts))
    check(ph.search_range(q2, rad2, max_rungs=2, counters=True), expected(rcs2, b, rad2, 2)[0], "2048 queries")
