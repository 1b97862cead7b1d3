"""Grouped search over a partitioned index (idist_partitioned_search_batch_grouped) and its union kernel
(idist_grouped_merge_device).  Row q is DEFINED as the collapse of the merge, by (raw distance bits, global id), of what the
single-index grouped search returns on every part: everything is compared exactly, and the expected arrays come from `Model.run` of
tests/test_grouped.py per part and the numpy `merge_collapse` below.  Every case runs on the CPU emulator and (-m gpu) on the MI355X."""
import atexit

import numpy as np
import pytest

import parity_cases as pc
from engines import cu_count, engine_params
from test_grouped import Model, collapse
from test_partitioned import INF_BITS, INVALID, NAN_BITS, DeviceMem
from test_partitioned_allowed import EXACT, NONE, main_parts

FILL = 0xABABABAB
VALUES = np.concatenate([np.array([0, 0xFFFFFFFF, 1, 0x80000000], np.uint64), np.arange(1, 17000, dtype=np.uint64) * 8192]).astype(np.uint32)


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


def merge_collapse(pid, bits, grp, cnt, ctr, base, k):
    """[P][nq][w] lists -> per query: concatenate the first count entries, sort by the u64 key, keep the first of each group, cut to k"""
    P, nq, w = pid.shape
    o_pid, o_bits = np.full((nq, k), INVALID, np.uint32), np.full((nq, k), INF_BITS, np.uint32)
    o_grp, o_cnt = np.zeros((nq, k), np.uint32), np.zeros(nq, np.uint32)
    for q in range(nq):
        c = [min(int(cnt[p, q]), w) for p in range(P)]
        gid = np.concatenate([pid[p, q, : c[p]].astype(np.uint64) + np.uint64(base[p]) for p in range(P)])
        d, g = np.concatenate([bits[p, q, : c[p]] for p in range(P)]), np.concatenate([grp[p, q, : c[p]] for p in range(P)])
        order = np.lexsort((gid, d))
        keep = order[np.sort(np.unique(g[order], return_index=True)[1])][:k]
        m = len(keep)
        o_pid[q, :m], o_bits[q, :m], o_grp[q, :m], o_cnt[q] = gid[keep].astype(np.uint32), d[keep], g[keep], m
    return o_pid, o_bits, o_grp, o_cnt, ctr.sum(axis=0, dtype=np.uint32)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------
def lists(rng, P, w, layout):
    """four queries of P lists (counts: full; random; list 0 empty, the others random; all empty), each ascending in (distance bits,
    pid) with distinct groups — indices into VALUES, so 0 and 0xFFFFFFFF are groups everywhere; behind a count: distance 0, groups of
    their own.  distinct: no group twice; same: every list holds the groups 0 .. w - 1; later: the same, every list nearer than the
    one before it; ties: the same, one distance for all; naninf: the same, NaN and +inf among the distances"""
    m = 4
    pid = np.stack([[rng.permutation(w) for _ in range(m)] for _ in range(P)]).astype(np.uint32)
    bits = rng.integers(1, 0x7F000000, (P, m, w)).astype(np.uint32)
    if layout == "later":
        bits = (bits >> 8) + (np.uint32(P) - np.arange(P, dtype=np.uint32))[:, None, None] * np.uint32(1 << 24)
    elif layout == "ties":
        bits[:] = 0x3F800000
    elif layout == "naninf":
        bits[rng.random((P, m, w)) < 0.3] = INF_BITS
        bits[rng.random((P, m, w)) < 0.2] = NAN_BITS
    gi = np.stack([[rng.permutation(w) for _ in range(m)] for _ in range(P)])
    if layout == "distinct":
        gi += np.arange(P)[:, None, None] * w
    cnt = np.stack([np.full(P, w), rng.integers(0, w + 1, P), rng.integers(0, w + 1, P), np.zeros(P, np.int64)], axis=1).astype(np.uint32)
    cnt[0, 2] = 0
    for p in range(P):
        for q in range(m):
            o = np.lexsort((pid[p, q], bits[p, q]))
            pid[p, q], bits[p, q], gi[p, q] = pid[p, q, o], bits[p, q, o], gi[p, q, o]
            bits[p, q, cnt[p, q]:], gi[p, q, cnt[p, q]:] = 0, P * w + p * w + np.arange(w - cnt[p, q])
    return pid, bits, VALUES[gi], cnt, rng.integers(0, 1000, (P, m, 3)).astype(np.uint32)


LAYOUTS = ["distinct", "same", "later", "ties", "naninf"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(1, 8, 8), (2, 5, 5), (5, 16, 7), (64, 3, 3), (3, 40, 40), (2, 4096, 4096), (8, 1024, 1024)])
def test_merge_kernel(eng, shape, layout):
    """(n_lists, width, k).  (64, 3, 3): one lane per list, one entry per step; (3, 40, 40): the k-th kept entry lies behind the first
    tile; (2, 4096, 4096): the largest set, 64 KiB of LDS before the tiles; (8, 1024, 1024): 64 KiB of keys that are never staged.  The
    small shapes run more queries than the grid has workgroups (32 per CU), row q holding lists q % 4; the two large ones run four."""
    ida, kind = eng
    from instant_distance_amd import _capi

    P, w, k = shape
    rng = np.random.default_rng([P, w, k, LAYOUTS.index(layout)])
    pid, bits, grp, cnt, ctr = lists(rng, P, w, layout)
    base = (np.arange(P) * w).astype(np.uint32)
    nq = 4 if w >= 1024 else 32 * cu_count(kind) + 5
    want = [x[np.arange(nq) % 4] for x in merge_collapse(pid, bits, grp, cnt, ctr, base, k)]
    mem, L = DeviceMem(kind), _capi.lib()
    try:
        d_in = [mem.up(x[:, np.arange(nq) % 4]) for x in (pid, bits, grp, cnt, ctr)]
        outs = [np.full(nq * k + 5, FILL, np.uint32) for _ in range(3)] + [np.full(nq + 5, FILL, np.uint32), np.full(nq * 3 + 5, FILL, np.uint32)]
        d_out = [mem.up(o) for o in outs]
        L.check(L.idist_grouped_merge_device(*d_in, P, nq, w, _capi.u32p(base), k, *d_out, 0, None))
        got = [mem.down(d, o) for d, o in zip(d_out, outs)]
        for i, name in enumerate(("ids", "distance bits", "groups", "counts", "counters")):
            body = want[i].size
            assert np.array_equal(got[i][:body].reshape(want[i].shape), want[i]), (shape, layout, name)
            assert np.all(got[i][body:] == FILL), (shape, layout, name)         # nothing behind the last row
        assert L.idist_grouped_merge_device(*d_in, 65, nq, w, _capi.u32p(base), k, *d_out, 0, None) == 1
        assert L.idist_grouped_merge_device(*d_in, P, nq, w, _capi.u32p(base), 0, *d_out, 0, None) == 1
    finally:
        mem.free()


# ---- 2. - 5. the call ------------------------------------------------------------------------------------------------------------------
def setting(ida, oracle, kind, P):
    """P = 1: one part; P = 3: test_partitioned_allowed's two-part cut around an EMPTY part"""
    pts, q, b, cs, k = main_parts(oracle, kind, 1 if P == 1 else 2)
    if P == 3:
        cs, b = [cs[0], None, cs[1]], [b[0], b[1], b[1], b[2]]
    empty = lambda: ida.Hnsw.from_ordered_points(np.zeros((0, pts.shape[1]), np.float32), ida.Builder().ef_search(cs[0].ef))   # noqa: E731
    hs = [c.hnsw(ida) if c else empty() for c in cs]
    return ida.PartitionedHnsw.from_hnsws(hs), hs, cs, b, pts, q, k


def columns(pts, b, lay):
    """documents of 4 chunks dealt at random over all parts, or every point its own; sel: 1 for a third of the LAST part only"""
    n = len(pts)
    rng = np.random.default_rng(31)
    g = (rng.permutation(n) // 4 if lay == "docs4" else np.arange(n)).astype(np.uint32)
    sel = np.zeros(n, np.uint32)
    sel[b[-2]:] = rng.random(n - b[-2]) < 0.33
    return g, sel


_MODELS = {}
atexit.register(_MODELS.clear)      # (the oracle's handles go before the interpreter takes its library apart)


def expected(cs, b, g, mask, k, max_rungs):
    """test_grouped's Model per part on the part's slices, then merge_collapse -> (pid, bits, count, rung [nq][P], counters, group)"""
    P, nq = len(cs), len(cs[0].q)
    pid, bits = np.full((P, nq, k), INVALID, np.uint32), np.full((P, nq, k), INF_BITS, np.uint32)
    grp, cnt = np.zeros((P, nq, k), np.uint32), np.zeros((P, nq), np.uint32)
    rung, ctr = np.full((P, nq), NONE, np.uint32), np.zeros((P, nq, 3), np.uint32)
    for p, c in enumerate(cs):
        if c:
            sl, model = slice(b[p], b[p + 1]), _MODELS.setdefault(id(c), Model(c))
            pid[p], bits[p], cnt[p], rung[p], ctr[p], grp[p] = model.run([mask[sl]], np.zeros(nq, np.int64), g[sl], k, max_rungs)[:6]
    o_pid, o_bits, o_grp, o_cnt, o_ctr = merge_collapse(pid, bits, grp, cnt, ctr, np.asarray(b[:-1], np.uint32), k)
    return o_pid, o_bits, o_cnt, np.ascontiguousarray(rung.T), o_ctr, o_grp


@pytest.mark.parametrize("lay", ["docs4", "own"])
@pytest.mark.parametrize("P", [1, 3])
def test_every_path_and_truth(eng, oracle, P, lay):
    """against the composition; at max_rungs = 0 also against the collapse of the oracle's brute force over ALL allowed rows; the
    identities against Hnsw.search_grouped (one part) and search_match (every point its own group)"""
    ida, kind = eng
    ph, hs, cs, b, pts, q, k = setting(ida, oracle, kind, P)
    g, sel = columns(pts, b, lay)
    table = ph.attribute_table({"g": g, "sel": sel})
    seen = set()
    for conds, mask in ((None, np.ones(len(pts), bool)), ({"sel": 1}, sel == 1)):
        for max_rungs in (-1, 0):
            pid, bits, cnt, rung, ctr, grp = expected(cs, b, g, mask, k, max_rungs)
            what = f"{conds}, max_rungs {max_rungs}"
            got = ph.search_grouped(q, table, "g", k, conds, max_rungs=max_rungs, counters=True)
            assert np.array_equal(got.rung, rung) and np.array_equal(got.count, cnt) and np.array_equal(got.counters, ctr), what
            assert np.array_equal(got.pid, pid) and np.array_equal(got.group, grp) and np.array_equal(pc.bits(got.distance), bits), what
            seen |= set(rung.ravel().tolist())
            o = None                                   # the identities: one part; every point its own group — rungs and counters included
            if P == 1:
                o = hs[0].search_grouped(q, hs[0].attribute_table({"g": g, "sel": sel}), "g", k, conds, ida.Search(), max_rungs=max_rungs, counters=True)
                o.rung = o.rung[:, None]
            elif lay == "own":
                o = ph.search_match(q, table, conds or {}, k, max_rungs=max_rungs, counters=True)
            if o is not None:
                assert np.array_equal(got.rung, o.rung) and np.array_equal(got.count, o.count) and np.array_equal(got.pid, o.pid), what
                assert np.array_equal(pc.bits(got.distance), pc.bits(o.distance)) and np.array_equal(got.counters, o.counters), what
            if max_rungs == 0:
                ids = np.flatnonzero(mask).astype(np.uint32)
                bp, bd = oracle.bruteforce(pts[ids], q, len(ids), threads=8)
                for qi in range(len(q)):
                    keep = collapse(ids[bp[qi]], np.ones(len(pts), bool), g, k)
                    assert len(keep) == k and np.array_equal(pid[qi], ids[bp[qi, keep]]) and np.array_equal(bits[qi], pc.bits(bd[qi, keep])), what
                    assert np.array_equal(grp[qi], g[pid[qi]]), what
    if lay == "docs4" and P == 3:                                               # groups span parts
        assert len(np.unique(np.stack([g, np.arange(len(g)) >= b[1]]), axis=1).T) > len(np.unique(g))
    assert any(r < NONE for r in seen) and EXACT in seen and (NONE in seen or P == 1) and ph.last_merge_ms() >= 0.0


def test_argument_errors(eng):
    ida, kind = eng
    from instant_distance_amd import _capi

    pts = np.random.default_rng(1).random((50, 4), dtype=np.float32)
    hs = [ida.Hnsw.from_ordered_points(np.ascontiguousarray(r), ida.Builder().ef_search(10)) for r in (pts[:21], pts[21:])]
    ph = ida.PartitionedHnsw.from_hnsws(hs)
    two = np.stack([np.arange(50) // 2, np.arange(50) % 5], axis=1)
    t, t_index = ph.attribute_table(two), hs[0].attribute_table(two[:21])
    L, u, f = _capi.lib(), _capi.u32p, _capi.f32p
    pid, dist, grp, cnt = np.zeros(30, np.uint32), np.zeros(30, np.float32), np.zeros(30, np.uint32), np.zeros(3, np.uint32)

    def call(attr=t, col=0, k=5, nq=3):
        return L.idist_partitioned_search_batch_grouped(ph._h, attr._h, col, f(pts[:3]), nq, None, k, -1, u(pid), f(dist), u(grp), u(cnt), None, None)

    assert call() == 0 and cnt.tolist() == [5, 5, 5] and np.array_equal(grp[:15], pid[:15] // 2)
    assert call(col=2) == 1 and b"2 columns" in L.idist_last_error()
    assert call(attr=t_index) == 1 and call(k=0) == 1 and call(k=11) == 1
    assert call(nq=0) == 0 and call(k=10) == 0 and cnt.tolist() == [10, 10, 10]
    r = ph.search_grouped(np.zeros((0, 4), np.float32), t, "0", 5, counters=True)
    assert r.pid.shape == (0, 5) and r.group.shape == (0, 5) and r.rung.shape == (0, 2)
