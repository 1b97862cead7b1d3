"""Restricted range search over a partitioned index (idist_partitioned_search_batch_range_allowed_sets, include/idist.h; DESIGN.md
sections 4.10 and 8.1): every point of a query's own allowed set within its radius, over all parts.

The call is DEFINED by composing exact things: row q is the merge, by the u64 key (raw distance bits, global id), of what the
single-index restricted range search returns for query q on every non-empty part, given the slice of q's set that falls into the
part; the metric's report runs once, after the merge.  So everything is compared exactly (lims, ids, rungs and counters with
array_equal, distances as bit patterns).  The expected arrays come from `model` of tests/test_range_allowed.py — the oracle's searches
and brute force, the mask and the end rule — applied per part to the slices, and the numpy merge `expected` of
tests/test_partitioned_range.py; never from the new call.  Every case runs on the CPU emulator and (-m gpu) on the MI355X."""
import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params
from test_allowed import ladder
from test_dot import np_augment
from test_partitioned import uneven_bounds
from test_partitioned_allowed import global_masks
from test_partitioned_range import PCase, check, expected, partitioned, range_parts, whole
from test_range import radii_of
from test_range_allowed import bitmaps, model

NONE, EXACT = 254, 255


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


def S(kind, emu, gpu):
    return gpu if kind == "gpu" else emu


# ---- the definition, restated ------------------------------------------------------------------------------------------------------
class RPart:
    """One part of a restricted call: tests/test_range_allowed.py's `model` — the very code — on the part's slices of the sets, and
    the RAW distance bits of what it returns (`expected` merges raw distances and reports afterwards).  masks: the part's slices,
    bool [n_sets][n_p]; set_of[i]: the set of the i-th query of the call."""

    def __init__(self, rc, masks, set_of):
        self.rc, self.masks, self.set_of = rc, masks, np.asarray(set_of)
        self.q, self.report = rc.q, rc.report

    def model_raw(self, radii, max_rungs=-1, queries=None):
        rc = self.rc
        lims, pid, _, rung, ctr, _ = model(rc, radii, self.masks, self.set_of, max_rungs, queries)
        qs = range(len(rc.q)) if queries is None else queries
        E = ladder(rc.ef)
        raw = []
        for i, qi in enumerate(qs):
            ids = pid[int(lims[i]): int(lims[i + 1])]
            if not len(ids):
                continue
            if rung[i] == EXACT:
                l_pid, l_d = rc.all_pid[qi], rc.all_d[qi]
            else:
                res = rc.c.rung(E[int(rung[i])])
                cnt = int(res.count[qi])
                l_pid, l_d = res.pid[qi, :cnt], res.dist[qi, :cnt]
            order = np.argsort(l_pid, kind="stable")
            pos = order[np.searchsorted(l_pid, ids, sorter=order)]
            assert np.array_equal(l_pid[pos], ids) and np.all(np.diff(pos) > 0)        # a sub-sequence of the list, in its order
            raw.append(l_d[pos])
        raw = np.concatenate(raw).astype(np.float32) if raw else np.zeros(0, np.float32)
        return lims, pid, pc.bits(raw), rung, ctr


def restricted(rcs, b, masks, set_of):
    """the parts of a call: rcs[p] with the slice [b[p], b[p + 1]) of every GLOBAL set (None stays None: an empty part)"""
    return [None if rc is None else RPart(rc, [np.asarray(m)[b[p]: b[p + 1]] for m in masks], set_of) for p, rc in enumerate(rcs)]


def want_of(rcs, b, masks, set_of, radii, max_rungs=-1, queries=None):
    so = np.asarray(set_of) if queries is None else np.asarray(set_of)[list(queries)]
    return expected(restricted(rcs, b, masks, so), b, radii, max_rungs, queries)


def cycle(nq, n_sets, shift):
    """radius kind q % 12 meets set (q + q // 12 + shift) % n_sets"""
    q = np.arange(nq)
    return ((q + q // 12 + shift) % n_sets).astype(np.uint32)


def k_of(kind):
    return S(kind, 5, 10)                                          # (the k the sets of test_partitioned_allowed.py are sized around)


# ---- 1. parity with the definition -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_parity_with_the_definition(eng, oracle, P):
    ida, kind = eng
    pts, q, b, rcs, w = range_parts(oracle, kind, P)
    ph, hs = partitioned(ida, rcs)
    masks = global_masks(pts, b, k_of(kind))
    rad, nq = radii_of(w), len(q)
    if P == 3 or (kind == "emu" and P > 1):
        assert any(x % 32 for x in b[:-1])                                  # a base that is no multiple of 32
    seen = set()
    for max_rungs, shift in ((-1, 0), (1, 3), (0, 5)):
        set_of = cycle(nq, len(masks), shift)
        want, cnt = want_of(rcs, b, masks, set_of, rad, max_rungs)
        print("max_rungs", max_rungs, "rungs", dict(zip(*[x.tolist() for x in np.unique(want[3], return_counts=True)])))
        check(ph.search_range_allowed_sets(q, rad, masks, set_of, max_rungs=max_rungs, counters=True), want, f"max_rungs {max_rungs}")
        check(ph.search_range_allowed_sets(q, rad, masks, set_of, max_rungs=max_rungs), want, f"max_rungs {max_rungs}, no counters")
        assert set(want[3].ravel().tolist()) <= set(range(max_rungs if max_rungs >= 0 else 8)) | {EXACT, NONE}
        if P > 1:                                                           # the confined set: NONE in every part but the last
            assert np.all(want[3][set_of == 4, : P - 1] == NONE)
        if max_rungs == 0:                                                  # every allowed point within, by (raw bits, global id)
            assert np.all(want[4] == 0)
            for qi in range(nq):
                with np.errstate(invalid="ignore"):
                    ids = w.all_pid[qi][(w.all_rep[qi] <= rad[qi]) & masks[set_of[qi]][w.all_pid[qi]]]
                assert np.array_equal(want[1][int(want[0][qi]): int(want[0][qi + 1])], ids), qi
        seen |= set(want[3].ravel().tolist())
    assert 0 in seen and EXACT in seen and NONE in seen
    assert ph.last_range_merge_ms() >= 0.0 and ph.last_allowed_slice_ms() >= 0.0
    # one shared set
    want, _ = want_of(rcs, b, [masks[3]], np.zeros(nq, np.int64), rad)
    check(ph.search_range_allowed(q, rad, masks[3], counters=True), want, "search_range_allowed")
    check(ph.search_range_allowed(q, rad, np.flatnonzero(masks[3])), want, "search_range_allowed, global ids")


# ---- 2. identities -----------------------------------------------------------------------------------------------------------------------
def test_one_part_is_the_single_index(eng, oracle):
    ida, kind = eng
    pts, q, b, rcs, w = range_parts(oracle, kind, 1)
    ph, hs = partitioned(ida, rcs)
    masks = global_masks(pts, b, k_of(kind))
    rad = radii_of(w)
    set_of = cycle(len(q), len(masks), 1)
    for m in (-1, 1, 0):
        a = ph.search_range_allowed_sets(q, rad, masks, set_of, max_rungs=m, counters=True)
        o = hs[0].search_range_allowed_sets(q, rad, masks, set_of, ida.Search(), max_rungs=m, counters=True)
        assert a.rung.shape == (len(q), 1) and np.array_equal(a.rung[:, 0], o.rung)
        assert np.array_equal(a.lims, o.lims) and np.array_equal(a.pid, o.pid) and np.array_equal(a.counters, o.counters)
        assert np.array_equal(pc.bits(a.distance), pc.bits(o.distance)) and int(o.lims[-1]) > 0


def test_all_ones_is_search_range(eng, oracle):
    ida, kind = eng
    pts, q, b, rcs, w = range_parts(oracle, kind, 3)
    ph, hs = partitioned(ida, rcs)
    rad = radii_of(w)
    # no part's end rule ever ends a rung iff 2 n_p > IDIST_MAX_EF everywhere; otherwise both sides answer exhaustively
    m = -1 if all(2 * (b[p + 1] - b[p]) > 4096 for p in range(3)) else 0
    a = ph.search_range_allowed_sets(q, rad, np.ones((2, len(pts)), bool), np.arange(len(q)) % 2, max_rungs=m, counters=True)
    o = ph.search_range(q, rad, max_rungs=m, counters=True)
    assert np.array_equal(a.lims, o.lims) and np.array_equal(a.pid, o.pid) and np.array_equal(a.rung, o.rung)
    assert np.array_equal(pc.bits(a.distance), pc.bits(o.distance)) and np.array_equal(a.counters, o.counters) and int(o.lims[-1]) > 0


# ---- 3. the metrics: the report runs after the merge -------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_metrics(eng, oracle, metric):
    ida, kind = eng
    n, dim, ef, nq, P = S(kind, (300, 7, 8, 18, 3), (3000, 24, 16, 90, 3))
    rng = np.random.default_rng(11)
    raw = rng.random((n, dim), dtype=np.float32) - np.float32(0.3)
    q = rng.random((nq, dim), dtype=np.float32) - np.float32(0.3)
    bound, builder = 0.0, None
    if metric == "dot":
        raw[n // 3] *= np.float32(37.0)                                     # S is large: the report rounds
        bound = float(np_augment(oracle, raw)[1])
        builder = lambda: ida.Builder().dot_bound(bound)                    # noqa: E731
    b = uneven_bounds(n, P)
    rcs = [PCase(oracle, raw[b[p]: b[p + 1]], q, ef, metric, bound=bound) for p in range(P)]
    w = whole(rcs, b, raw)
    kinds = ["below", 0, "ef-1", "ef", "ef+1", "4ef", "n/2", "inf", "neg"]
    rad = radii_of(w, kinds)
    masks = [rng.random(n) < 0.6, rng.random(n) < 0.08]
    masks[0][n // 3] = True
    set_of = ((np.arange(nq) // len(kinds)) % 2).astype(np.uint32)
    ph, hs = partitioned(ida, rcs, builder)
    seen = set()
    for m in (-1, 2, 0):
        want, _ = want_of(rcs, b, masks, set_of, rad, m)
        check(ph.search_range_allowed_sets(q, rad, masks, set_of, max_rungs=m, counters=True), want, f"{metric}, max_rungs {m}")
        seen |= set(want[3].ravel().tolist())
    assert EXACT in seen and len(seen) >= 2 and int(want[0][-1]) > 0


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------------------
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
    mask = np.array([True, False, True])
    for m in (-1, 0):
        r = ph.search_range_allowed(q, np.inf, mask, max_rungs=m, counters=True)
        assert np.array_equal(r.lims, np.arange(5, dtype=np.uint64) * 2) and r.rung.shape == (4, 5) and np.all(r.counters == 0)
        for qi in range(4):
            keep = mask[bp[qi]]
            assert np.array_equal(r.pid[2 * qi: 2 * qi + 2], bp[qi][keep]) and np.array_equal(pc.bits(r.distance[2 * qi: 2 * qi + 2]), pc.bits(bd[qi][keep]))
        for p in range(5):                                                  # an empty part or an empty slice: NONE; else 2 |A_p| <= E[0]: EXACT
            lo = int(ph._base[p])
            assert np.all(r.rung[:, p] == (EXACT if mask[lo: lo + sizes_[p]].any() else NONE))
    # every part empty
    ph0, ids0 = ida.PartitionedHnsw.build(np.zeros((0, 5), np.float32), ida.Builder(), parts=2)
    r0 = ph0.search_range_allowed_sets(q, np.inf, np.zeros((2, 0), bool), [0, 1, 1, 0], counters=True)
    assert np.all(r0.lims == 0) and r0.rung.shape == (4, 2) and np.all(r0.rung == NONE) and np.all(r0.counters == 0) and r0.pid.shape == (0,)
    # no queries
    e = ph.search_range_allowed_sets(np.zeros((0, 5), np.float32), 1.0, np.ones((2, 3), bool), np.zeros(0, np.int64), counters=True)
    assert np.array_equal(e.lims, np.zeros(1, np.uint64)) and e.rung.shape == (0, 5) and e.counters.shape == (0, 3)


def test_dirty_padding_bits(eng, oracle):
    """N no multiple of 32, straight through the ABI with EVERY padding bit of every set set; a set of padding bits only"""
    ida, kind = eng
    from instant_distance_amd import _capi

    n, dim, ef, nq, P = S(kind, 205, 1037), 5, 8, 13, 3
    rng = np.random.default_rng(12)
    pts, q = rng.random((n, dim), dtype=np.float32), rng.random((nq, dim), dtype=np.float32)
    b = uneven_bounds(n, P)
    assert n % 32 and any(x % 32 for x in b[1:-1])
    rcs = [PCase(oracle, pts[b[p]: b[p + 1]], q, ef) for p in range(P)]
    ph, hs = partitioned(ida, rcs)
    w = whole(rcs, b, pts)
    rad = radii_of(w, ["ef", "n/2", "inf", 0])
    last = np.zeros(n, bool)
    last[(n - 1) // 32 * 32:] = True                                        # members in the last, partial word only
    masks = [rng.random(n) < 0.4, np.ones(n, bool), last, np.zeros(n, bool), np.zeros(n, bool)]   # the fifth: padding bits only
    dirty = bitmaps(masks, n)
    dirty[:, -1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
    keep = dirty.copy()
    set_of = (np.arange(nq) % 5).astype(np.uint32)
    L = _capi.lib()
    for m in (-1, 0):
        want, _ = want_of(rcs, b, masks, set_of, rad, m)
        lims, rung, ctr = np.zeros(nq + 1, np.uint64), np.zeros((nq, P), np.uint32), np.zeros((nq, 3), np.uint32)
        L.check(L.idist_partitioned_search_batch_range_allowed_sets(ph._h, _capi.f32p(q), nq, _capi.f32p(rad), nq, _capi.u32p(dirty), 5,
                                                                    _capi.u32p(set_of), m, 1 << 40, _capi.u64p(lims), _capi.u32p(rung),
                                                                    _capi.u32p(ctr)))
        pid, dist = np.zeros(int(lims[nq]), np.uint32), np.zeros(int(lims[nq]), np.float32)
        L.check(L.idist_partitioned_range_fetch(ph._h, _capi.u32p(pid), _capi.f32p(dist)))
        check(ida.RangeResult(lims, pid, dist, rung, ctr), want, f"max_rungs {m}")
        pad = np.flatnonzero(set_of >= 3)                                   # the empty set and the set of padding bits only
        assert np.all(rung[pad] == NONE) and np.all(np.diff(lims.astype(np.int64))[pad] == 0)
    assert np.array_equal(dirty, keep)                                      # the caller's buffer is not written


def test_edges_of_the_call(eng, oracle):
    ida, kind = eng
    from instant_distance_amd import _capi

    pts, q, b, rcs, w = range_parts(oracle, kind, 3)
    ph, hs = partitioned(ida, rcs)
    L = _capi.lib()
    nq, n = 12, len(pts)
    q12, rad = q[:nq], radii_of(w)[:nq].copy()
    masks = [np.ones(n, bool), np.arange(n) % 2 == 0]
    bits = bitmaps(masks, n)
    set_of = (np.arange(nq) % 2).astype(np.uint32)
    want, cnt = want_of(rcs, b, masks, set_of, rad, -1, queries=range(nq))
    total, per_part = int(want[0][-1]), cnt.sum(axis=0)
    assert total > 0 and np.count_nonzero(per_part) >= 2
    lims, rung = np.zeros(nq + 1, np.uint64), np.zeros((nq, 3), np.uint32)
    pid, dist = np.zeros(total, np.uint32), np.zeros(total, np.float32)

    def call(radius=rad, n_radius=nq, max_total=1 << 40, n_sets=2, so=set_of, queries=q12, bitmap=bits, out=lims):
        return L.idist_partitioned_search_batch_range_allowed_sets(
            ph._h, None if queries is None else _capi.f32p(queries), nq, _capi.f32p(radius), n_radius, None if bitmap is None else _capi.u32p(bitmap),
            n_sets, None if so is None else _capi.u32p(np.asarray(so, np.uint32)), -1, max_total, None if out is None else _capi.u64p(out),
            _capi.u32p(rung), None)

    def fetch():
        return L.idist_partitioned_range_fetch(ph._h, _capi.u32p(pid), _capi.f32p(dist))

    assert fetch() == 1                                                     # nothing held yet
    # a NaN radius is refused and names the query; nothing is held afterwards
    bad = rad.copy()
    bad[7] = np.nan
    assert call(bad) == 1 and b"query 7" in L.idist_last_error() and fetch() == 1
    assert call(n_radius=5) == 1
    # the sets' arguments
    assert call(n_sets=0) == 1 and call(so=None) == 1                       # no set; one set per query needs n_sets == nq
    assert call(so=[0, 1, 2] + [0] * 9) == 1 and b"query 2" in L.idist_last_error()
    assert call(queries=None) == 1 and call(bitmap=None) == 1 and call(out=None) == 1
    # max_total exceeded in a part (the message names it) and at the merge
    assert call(max_total=int(per_part.max()) - 1) == 1
    msg = L.idist_last_error().decode()
    assert "max_total" in msg and msg.startswith("part ") and fetch() == 1
    assert int(per_part.max()) <= total - 1
    assert call(max_total=total - 1) == 1
    msg = L.idist_last_error().decode()
    assert "max_total" in msg and "the merge" in msg and str(total) in msg and fetch() == 1
    with pytest.raises(ida.IdistError):
        ph.search_range_allowed_sets(q12, rad, masks, set_of, max_total=total - 1)
    check(ph.search_range_allowed_sets(q12, rad, masks, set_of, max_total=total, counters=True), want, "max_total == the total")
    # the results are handed out once
    assert call() == 0 and int(lims[nq]) == total and lims[0] == 0 and np.array_equal(rung, want[3])
    assert fetch() == 0
    assert np.array_equal(pid, want[1]) and np.array_equal(pc.bits(dist), want[2])
    assert fetch() == 1
    # the Python layer
    with pytest.raises(ValueError):
        ph.search_range_allowed_sets(q12, rad[:5], masks, set_of)
    with pytest.raises(ValueError):
        ph.search_range_allowed_sets(q12, rad, masks, None)                 # 2 sets for 12 queries
    with pytest.raises(IndexError):
        ph.search_range_allowed_sets(q12, rad, masks, [0, 1, 2] + [0] * 9)
    with pytest.raises(ValueError):
        ph.search_range_allowed(q12, rad, np.ones(n - 1, bool))
    # the parts are compared again at every call
    hs[1].set_ef_search(50)
    with pytest.raises(ida.IdistError) as e:
        ph.search_range_allowed_sets(q12, rad, masks, set_of)
    assert e.value.status == 1 and "part 1" in e.value.message
    hs[1].set_ef_search(rcs[1].ef)
