"""Restricted range search (idist_search_batch_range_allowed_sets, include/idist.h): every point of a query's
own allowed set within its radius.

The answer is DEFINED through what is already exact — the rungs of the range search, each answer filtered by the query's set, while
E[r] < 2 |A| (the end rule), and an exhaustive scan of the set's rows where a query's rungs end — so everything here is compared
exactly: lims, ids, order, rungs and counters with array_equal, distances as bit patterns.  The expected arrays come from the model in
this file (tests/test_range.py's RCase — the oracle's searches and brute force — plus the mask and the end rule), never from the code
under test.  Every case runs on the CPU emulator and (-m gpu) on the MI355X."""
import atexit

import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params
from test_allowed import LDS_EF, LDS_R_END, ladder, lds_points, lds_rung0_refused
from test_range import KINDS, RCase, check, counts, radii_of

NONE, EXACT = 254, 255


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


def S(kind, emu, gpu):
    return gpu if kind == "gpu" else emu


# ---- the definition, restated --------------------------------------------------------------------------------------------
def n_permitted(E, a):
    """the end rule: the rungs with E[r] < 2 |A| (a prefix, E grows)"""
    R = 0
    while R < len(E) and E[R] < 2 * a:
        R += 1
    return R


def model(rc, radii, masks, set_of, max_rungs=-1, queries=None):
    """(lims, pid, reported distance bits, rung, counters, cause) by the definition; masks: bool [n_sets][n]; set_of[i]: the set of
    the i-th query of the call; cause[i]: why an exact answer is exact — "rule" (the end rule stopped the query) or "ladder" (its
    rungs were the whole permitted ladder)."""
    qs = range(len(rc.q)) if queries is None else queries
    rad = np.broadcast_to(np.asarray(radii, dtype=np.float32), (len(qs),))
    E = ladder(rc.ef) if rc.ef else []
    if max_rungs >= 0:
        E = E[:max_rungs]
    sizes = [int(np.count_nonzero(m)) for m in masks]
    pids, reps, rung, ctr = [], [], np.full(len(qs), NONE, np.uint32), np.zeros((len(qs), 3), np.uint32)
    cause = [""] * len(qs)
    for i, qi in enumerate(qs):
        mask, a, r = masks[set_of[i]], sizes[set_of[i]], rad[i]
        if a == 0 or len(rc.raw) == 0 or rc.ef == 0:
            pids.append(np.zeros(0, np.uint32))
            reps.append(np.zeros(0, np.float32))
            continue
        R = n_permitted(E, a)
        for ri, e in enumerate(E[:R]):
            res = rc.c.rung(e)
            cnt = int(res.count[qi])
            ctr[i] += res.counters[qi]
            rep = rc.report(res.dist[qi, :cnt], qi)
            with np.errstate(invalid="ignore"):
                w = rep <= r
            if cnt == e and w.all():
                continue                                                     # saturated, on the unrestricted list: the next rung
            pre = cnt if w.all() else int(np.argmin(w))
            keep = mask[res.pid[qi, :pre]]
            pids.append(res.pid[qi, :pre][keep])
            reps.append(rep[:pre][keep])
            rung[i] = ri
            break
        else:
            with np.errstate(invalid="ignore"):
                w = (rc.all_rep[qi] <= r) & mask[rc.all_pid[qi]]
            pids.append(rc.all_pid[qi][w])
            reps.append(rc.all_rep[qi][w])
            rung[i] = EXACT
            cause[i] = "rule" if R < len(E) else "ladder"
    lims = np.concatenate([[0], np.cumsum([len(p) for p in pids])]).astype(np.uint64)
    pid = np.concatenate(pids).astype(np.uint32) if pids else np.zeros(0, np.uint32)
    rep = np.concatenate(reps).astype(np.float32) if reps else np.zeros(0, np.float32)
    return lims, pid, pc.bits(rep), rung, ctr, cause


def bitmaps(masks, n):
    from instant_distance_amd.api import allowed_bitmap

    return np.stack([allowed_bitmap(m, n) for m in masks])


def row(r, i):
    """(ids, distance bits) of query i of a RangeResult or of a model's tuple"""
    if isinstance(r, tuple):
        lo, hi = int(r[0][i]), int(r[0][i + 1])
        return r[1][lo:hi], r[2][lo:hi]
    lo, hi = int(r.lims[i]), int(r.lims[i + 1])
    return r.pid[lo:hi], pc.bits(r.distance[lo:hi])


_CASES = {}
atexit.register(_CASES.clear)      # (the oracle's handles go before the interpreter takes its library apart)


def main_case(oracle, kind):
    """emu: 600 x 12-d, ef_search 8, 40 queries (ladder 8, 32, 128, 512, 2048, 4096); gpu: 8007 x 32-d — a multiple of neither 32 nor
    64: the bitmap's last word and the last window are partial — ef_search 16, 600 queries (ladder 16, 64, 256, 1024, 4096).  The
    queries whose radius will be 0 / -0.0 are stored rows."""
    if kind not in _CASES:
        n, dim, ef, nq, seed = S(kind, (600, 12, 8, 40, 1), (8007, 32, 16, 600, 2))
        rng = np.random.default_rng(seed)
        pts, q = rng.random((n, dim), dtype=np.float32), rng.random((nq, dim), dtype=np.float32)
        for j in (KINDS.index("zero"), KINDS.index("negzero")):
            q[j::len(KINDS)] = pts[rng.choice(n, len(q[j::len(KINDS)]), replace=False)]
        _CASES[kind] = RCase(oracle, pts, q, ef)
    return _CASES[kind]


SET_NAMES = ["empty", "one", "E0/2", "E0/2+1", "E1/2", "E1/2+1", "3%", "half", "all", "last window", "two windows", "dirty"]


def main_sets(rc):
    """(masks [12][n], bitmaps [12][words]): the sizes around the end rule's thresholds, the window walk's edges, and one bitmap with
    every padding bit of its last word set"""
    n, E = len(rc.raw), ladder(rc.ef)
    rng = np.random.default_rng(77)

    def some(k):
        m = np.zeros(n, bool)
        m[rng.choice(n, k, replace=False)] = True
        return m

    last = np.zeros(n, bool)
    last[64 * (n // 64) + (0 if n % 64 else -64):] = True               # only ids of the last (partial) window
    two = np.zeros(n, bool)
    w = (n // 64) // 2
    two[64 * w + 20: 64 * w + 85] = True                                # 44 ids of one window, 21 of the next: one is carried over
    masks = [np.zeros(n, bool), some(1), some(E[0] // 2), some(E[0] // 2 + 1), some(E[1] // 2), some(E[1] // 2 + 1), rng.random(n) < 0.03,
             rng.random(n) < 0.5, np.ones(n, bool), last, two, rng.random(n) < 0.04]
    assert len(masks) == len(SET_NAMES) and int(two.sum()) == 65 and n % 32 != 0
    bits = bitmaps(masks, n)
    bits[SET_NAMES.index("dirty"), -1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
    return masks, bits


def cycle(nq, shift):
    """radius kind q % 12 meets set (q + q // 12 + shift) % 12: the shifts 0, 4, 8 pair every kind with every set within 40 queries"""
    q = np.arange(nq)
    return ((q + q // len(KINDS) + shift) % len(SET_NAMES)).astype(np.uint32)


# ---- 1. sets x radii: every path ---------------------------------------------------------------------------------------------------
def test_sets_and_radii_every_path(eng, oracle):
    ida, kind = eng
    rc = main_case(oracle, kind)
    h, s = rc.hnsw(ida), ida.Search()
    masks, bits = main_sets(rc)
    rad, nq = radii_of(rc), len(rc.q)
    seen, causes = set(), set()
    for shift in S(kind, (0, 4, 8), (0,)):
        set_of = cycle(nq, shift)
        for m in S(kind, (-1, 2), (-1,)):                             # emu: 600 points never saturate a rung of 2048
            want = model(rc, rad, masks, set_of, max_rungs=m)
            print("shift", shift, "max_rungs", m, "rungs", dict(zip(*[x.tolist() for x in np.unique(want[3], return_counts=True)])),
                  "causes", sorted(set(want[5])))
            check(h.search_range_allowed_sets(rc.q, rad, bits, set_of, s, max_rungs=m, counters=True), want[:5], f"shift {shift}, max_rungs {m}")
            seen |= set(want[3].tolist())
            causes |= set(want[5])
    assert 0 in seen and len({r for r in seen if 0 < r < NONE}) >= 2 and EXACT in seen and NONE in seen
    assert {"rule", "ladder"} <= causes


# ---- 2. identities -----------------------------------------------------------------------------------------------------------------
def test_filter_identity(eng, oracle):
    """a query answered on rung r holds search_range's answer of that rung, filtered by its set"""
    ida, kind = eng
    rc = main_case(oracle, kind)
    masks, bits = main_sets(rc)
    rad, nq = radii_of(rc), len(rc.q)
    set_of = cycle(nq, 4)
    want = model(rc, rad, masks, set_of)
    got = rc.hnsw(ida).search_range_allowed_sets(rc.q, rad, bits, set_of, ida.Search())
    check(got, want[:5], "the call")
    rungs = sorted({int(r) for r in want[3] if r < NONE})
    assert len(rungs) >= 2
    for r in rungs:
        plain = rc.model(rad, max_rungs=r + 1)
        for qi in np.flatnonzero(want[3] == r):
            assert plain[3][qi] == r
            ids = row(plain, qi)[0]
            assert np.array_equal(row(got, qi)[0], ids[masks[set_of[qi]][ids]]), f"query {qi}, rung {r}"


def test_all_ones_is_search_range(eng, oracle):
    ida, kind = eng
    rc = main_case(oracle, kind)
    n, rad = len(rc.raw), radii_of(rc)
    h = rc.hnsw(ida)
    got = h.search_range_allowed(rc.q, rad, np.ones(n, bool), ida.Search(), counters=True)
    check(got, model(rc, rad, [np.ones(n, bool)], np.zeros(len(rc.q), np.int64))[:5], "all ones")
    if 2 * n > 4096:                                                   # no rung is ever ended by the rule
        plain = h.search_range(rc.q, rad, ida.Search(), counters=True)
        assert np.array_equal(got.lims, plain.lims) and np.array_equal(got.pid, plain.pid) and np.array_equal(got.rung, plain.rung)
        assert np.array_equal(pc.bits(got.distance), pc.bits(plain.distance)) and np.array_equal(got.counters, plain.counters)
    else:
        assert kind == "emu"


# ---- 3. max_rungs ----------------------------------------------------------------------------------------------------------------
def test_max_rungs(eng, oracle):
    ida, kind = eng
    rc = main_case(oracle, kind)
    h, s = rc.hnsw(ida), ida.Search()
    masks, bits = main_sets(rc)
    rad, nq = radii_of(rc), len(rc.q)
    set_of = cycle(nq, 8)
    empty = np.array([not masks[j].any() for j in set_of])
    for m in (0, 1, 2, -1):
        want = model(rc, rad, masks, set_of, max_rungs=m)
        got = h.search_range_allowed_sets(rc.q, rad, bits, set_of, s, max_rungs=m, counters=True)
        check(got, want[:5], f"max_rungs {m}")
        assert set(want[3].tolist()) <= set(range(m if m >= 0 else 8)) | {EXACT, NONE}
        if m == 0:                                                     # the exhaustive answer, for every query
            assert np.all(got.rung[~empty] == EXACT) and np.all(got.rung[empty] == NONE) and np.all(got.counters == 0)
            for qi in range(nq):
                with np.errstate(invalid="ignore"):
                    ids = rc.all_pid[qi][(rc.all_rep[qi] <= rad[qi]) & masks[set_of[qi]][rc.all_pid[qi]]]
                assert np.array_equal(row(got, qi)[0], ids)


# ---- 4. the metrics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2sq", "l2", "cosine", "dot"])
def test_metrics(eng, oracle, metric):
    """radii exactly on reported values; DOT with negative radii and one large-norm row, so the bound S is large and the report rounds"""
    ida, kind = eng
    n, dim, ef, nq = S(kind, (300, 7, 8, 24), (3000, 24, 16, 120))
    rng = np.random.default_rng(11)
    raw = rng.random((n, dim), dtype=np.float32) - np.float32(0.3)
    q = rng.random((nq, dim), dtype=np.float32) - np.float32(0.3)
    if metric == "dot":
        raw[n // 3] *= np.float32(37.0)
    rc = RCase(oracle, raw, q, ef, metric)
    kinds = ["below", 0, "ef-1", "ef", "ef+1", "4ef", "n/2", "inf", "neg"]
    rad = radii_of(rc, kinds)
    if metric == "dot":
        assert (rad[np.isfinite(rad)] < 0).any()                       # negative radii are meaningful here
    masks = [rng.random(n) < 0.6, rng.random(n) < 0.08]
    masks[0][n // 3] = True
    set_of = ((np.arange(nq) // len(kinds)) % 2).astype(np.uint32)
    h, s = rc.hnsw(ida), ida.Search()
    seen = set()
    for m in (-1, 2, 0):
        want = model(rc, rad, masks, set_of, max_rungs=m)
        check(h.search_range_allowed_sets(q, rad, masks, set_of, s, max_rungs=m, counters=True), want[:5], f"{metric}, max_rungs {m}")
        seen |= set(want[3].tolist())
    assert EXACT in seen and len(seen) >= 3


# ---- 5. the exact step does not depend on the segments ---------------------------------------------------------------------------
def test_exact_does_not_depend_on_the_segments(eng, oracle, monkeypatch):
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    rc = main_case(oracle, kind)
    h = rc.hnsw(ida)
    masks, bits = main_sets(rc)
    rad, nq = radii_of(rc), len(rc.q)
    set_of = cycle(nq, 0)
    want = model(rc, rad, masks, set_of, max_rungs=0)
    for seg in ("1", "3", "64"):
        monkeypatch.setenv("IDIST_RANGE_SEGMENTS", seg)               # (sampled when the context is made)
        check(h.search_range_allowed_sets(rc.q, rad, bits, set_of, ida.Search(), max_rungs=0, counters=True), want[:5], f"{seg} segments")
    monkeypatch.setenv("IDIST_RANGE_SEGMENTS", "3")
    three = np.array([SET_NAMES.index("half"), SET_NAMES.index("two windows"), SET_NAMES.index("last window")], np.uint32)
    check(h.search_range_allowed_sets(rc.q[:3], np.inf, bits, three, ida.Search(), max_rungs=0),
          model(rc, np.inf, masks, three, 0, queries=range(3))[:5], "3 segments, 3 queries")


# ---- 6. set_of forms and the shared set ------------------------------------------------------------------------------------------
def test_set_of_forms_and_the_shared_set(eng, oracle):
    ida, kind = eng
    rc = main_case(oracle, kind)
    h, s = rc.hnsw(ida), ida.Search()
    masks, bits = main_sets(rc)
    n, rad, nq = len(rc.raw), radii_of(rc), len(rc.q)
    set_of = cycle(nq, 4)
    want = model(rc, rad, masks, set_of)
    # set_of=None: one set per query
    check(h.search_range_allowed_sets(rc.q, rad, bits[set_of], None, s, counters=True), want[:5], "set_of=None")
    with pytest.raises(ValueError):
        h.search_range_allowed_sets(rc.q, rad, bits, None, s)
    # one set for the batch: a bool mask, an id array (duplicates, any order), a ready bitmap
    j = SET_NAMES.index("3%")
    shared = model(rc, rad, masks, np.full(nq, j))
    check(h.search_range_allowed(rc.q, rad, masks[j], s, counters=True), shared[:5], "bool mask")
    ids = np.flatnonzero(masks[j])
    ids = np.random.default_rng(3).permutation(np.concatenate([ids, ids[:5]]))
    check(h.search_range_allowed(rc.q, rad, ids, s, counters=True), shared[:5], "id array")
    check(h.search_range_allowed(rc.q, rad, bits[j:j + 1], s, counters=True), shared[:5], "ready bitmap")
    # row q is the call for query q alone with its own set
    whole = h.search_range_allowed_sets(rc.q, rad, bits, set_of, s, counters=True)
    for qi in range(0, nq, S(kind, 3, 47)):
        one = h.search_range_allowed(rc.q[qi], rad[qi], bits[set_of[qi]][None, :], s, counters=True)
        assert np.array_equal(one.rung, whole.rung[qi:qi + 1]) and np.array_equal(one.counters, whole.counters[qi:qi + 1])
        assert np.array_equal(one.pid, row(whole, qi)[0]) and np.array_equal(pc.bits(one.distance), row(whole, qi)[1])
        check(one, model(rc, rad[qi], masks, [set_of[qi]], queries=[qi])[:5], f"query {qi} alone")


# ---- 7. refusals and bounds ------------------------------------------------------------------------------------------------------
def test_refusals_and_bounds(eng, oracle):
    ida, kind = eng
    from instant_distance_amd import _capi

    rc = main_case(oracle, kind)
    h, s = rc.hnsw(ida), ida.Search()
    masks, bits = main_sets(rc)
    q, nq = rc.q[:12], 12
    rad = radii_of(rc)[:nq].copy()
    n_sets = len(masks)
    set_of = np.array([SET_NAMES.index(x) for x in ("half", "3%", "all", "half", "E1/2+1", "half", "3%", "all", "empty", "half", "one", "3%")],
                      np.uint32)
    L = _capi.lib()
    lims, rung = np.zeros(nq + 1, np.uint64), np.zeros(nq, np.uint32)

    def call(radius=rad, n_radius=nq, max_rungs=-1, max_total=1 << 40, queries=q, out_lims=lims, n=nq, b=bits, ns=n_sets, so=set_of):
        return L.idist_search_batch_range_allowed_sets(h._h, s._bind(h), _capi.f32p(queries) if queries is not None else None, n,
                                                       _capi.f32p(radius) if radius is not None else None, n_radius,
                                                       _capi.u32p(b) if b is not None else None, ns, _capi.u32p(so) if so is not None else None,
                                                       max_rungs, max_total, _capi.u64p(out_lims) if out_lims is not None else None,
                                                       _capi.u32p(rung), None)

    def nothing_to_fetch():
        pid, dist = np.zeros(8, np.uint32), np.zeros(8, np.float32)
        return L.idist_search_ctx_range_fetch(s._bind(h), _capi.u32p(pid), _capi.f32p(dist)) == 1

    assert nothing_to_fetch()                                                                          # fetch before any call
    bad = rad.copy()
    bad[7] = np.nan
    assert call(bad) == 1 and b"query 7" in L.idist_last_error()
    with pytest.raises(ida.IdistError) as e:
        h.search_range_allowed_sets(q, bad, bits, set_of, s)
    assert e.value.status == 1 and "query 7" in str(e.value)
    assert call(np.array([np.nan], np.float32), 1) == 1 and b"NaN" in L.idist_last_error()
    assert call(rad, 5) == 1 and call(rad, 0) == 1                                                    # n_radius not in {1, nq}
    with pytest.raises(ValueError):
        h.search_range_allowed_sets(q, rad[:5], bits, set_of, s)
    assert call(max_rungs=-2) == 1
    assert call(ns=0) == 1 and b"n_sets" in L.idist_last_error()
    assert call(b=bits[:5], ns=5, so=None) == 1 and b"set_of is null" in L.idist_last_error()         # n_sets != nq
    far = set_of.copy()
    far[5] = n_sets
    assert call(so=far) == 1 and b"query 5" in L.idist_last_error()
    with pytest.raises(IndexError):
        h.search_range_allowed_sets(q, rad, bits, far, s)
    assert call(radius=None) == 1 and call(queries=None) == 1 and call(out_lims=None) == 1 and call(b=None) == 1
    assert nothing_to_fetch()                                                                          # a refused call leaves nothing
    # max_total bounds the RESTRICTED total: one below it is an error that says what was known, the exact total succeeds although
    # the unrestricted answer is larger
    want = model(rc, rad, masks, set_of, queries=range(nq))
    total = int(want[0][-1])
    assert 0 < total < int(rc.model(rad, queries=range(nq))[0][-1])
    assert call(max_total=total - 1) == 1
    msg = L.idist_last_error().decode()
    assert "max_total" in msg and str(total - 1) in msg and str(total) in msg
    assert nothing_to_fetch()
    with pytest.raises(ida.IdistError):
        h.search_range_allowed_sets(q, rad, bits, set_of, s, max_total=total - 1)
    with pytest.raises(ida.IdistError):
        h.search_range_allowed_sets(q, rad, bits, set_of, s, max_rungs=0,
                                    max_total=int(model(rc, rad, masks, set_of, 0, queries=range(nq))[0][-1]) - 1)
    check(h.search_range_allowed_sets(q, rad, bits, set_of, s, max_total=total, counters=True), want[:5], "max_total == the total")
    # the results are handed out once
    assert call() == 0 and int(lims[nq]) == total and lims[0] == 0 and np.array_equal(rung, want[3])
    pid, dist = np.zeros(total, np.uint32), np.zeros(total, np.float32)
    assert L.idist_search_ctx_range_fetch(s._bind(h), _capi.u32p(pid), _capi.f32p(dist)) == 0
    assert np.array_equal(pid, want[1]) and np.array_equal(pc.bits(dist), want[2])
    assert nothing_to_fetch()
    # nq = 0
    r0 = h.search_range_allowed(np.zeros((0, q.shape[1]), np.float32), 1.0, masks[7], s, counters=True)
    assert np.array_equal(r0.lims, np.zeros(1, np.uint64)) and r0.pid.shape == (0,) and r0.rung.shape == (0,) and r0.counters.shape == (0, 3)
    # ef_search = 0, and no points: nothing to find
    h0 = ida.Hnsw.from_parts(rc.raw, rc.c.zero, rc.c.layers, ida.Builder().ef_search(0))
    r = h0.search_range_allowed_sets(q, np.inf, bits, set_of, ida.Search(), counters=True)
    assert np.all(r.lims == 0) and np.all(r.rung == NONE) and np.all(r.counters == 0) and r.pid.shape == (0,)
    he = ida.Hnsw.from_ordered_points(np.zeros((0, 4), np.float32), ida.Builder())
    r = he.search_range_allowed(np.zeros((3, 4), np.float32), np.inf, np.zeros(0, bool), ida.Search())
    assert np.all(r.lims == 0) and np.all(r.rung == NONE)


# ---- 8. the staging is shared safely ---------------------------------------------------------------------------------------------
def test_interleaving_on_one_context(eng, oracle):
    ida, kind = eng
    from test_allowed import check as check_allowed

    rc = main_case(oracle, kind)
    h, s = rc.hnsw(ida), ida.Search()
    masks, bits = main_sets(rc)
    rad, nq = radii_of(rc), len(rc.q)
    set_of = cycle(nq, 0)
    check(h.search_range_allowed_sets(rc.q, rad, bits, set_of, s, counters=True), model(rc, rad, masks, set_of)[:5], "restricted")
    check(h.search_range(rc.q, rad, s, counters=True), rc.model(rad), "then search_range")
    k, two = 5, [masks[SET_NAMES.index("half")], masks[SET_NAMES.index("3%")]]
    got = h.search_allowed_sets(rc.q, two, np.arange(nq) % 2, k, s, counters=True)
    models = [rc.c.model(m, k) for m in two]
    check_allowed(got, tuple(np.array([models[qi % 2][i][qi] for qi in range(nq)]) for i in range(5)) + (None,), "then search_allowed_sets")
    sub = list(range(3, 11))
    check(h.search_range_allowed_sets(rc.q[3:11], rad[3:11], bits, set_of[3:11], s, max_rungs=1, counters=True),
          model(rc, rad[3:11], masks, set_of[3:11], 1, queries=sub)[:5], "then eight queries")
    a, b, c = s.range_kernel_ms()
    assert a >= 0 and b >= 0 and c >= 0


# ---- 9. a rung that does not fit a wave's LDS ends the ladder (the shape and its arithmetic: tests/test_allowed.py) ---------------
def test_lds_short_rung_ends_the_ladder(eng, oracle):
    """with every point allowed the end rule permits rung 2 (256 < 2 * 256), which is refused: the queries still pending behind rung 1
    are answered exactly, as max_rungs = 2 defines"""
    ida, kind = eng
    if "lds" not in _CASES:
        _CASES["lds"] = RCase(oracle, *lds_points(), LDS_EF)
    rc = _CASES["lds"]
    n = len(rc.raw)
    rad = radii_of(rc, ["below", "ef", "4ef", "n/2", "inf", 0, "ef+1", "big"])
    masks = [np.ones(n, bool), np.random.default_rng(5).random(n) < 0.5]
    assert n_permitted(ladder(LDS_EF), n) > LDS_R_END
    for j in range(2):
        set_of = np.full(len(rc.q), j)
        want = model(rc, rad, masks, set_of, max_rungs=LDS_R_END)
        print("set", j, "rungs", want[3].tolist(), "counts", counts(want).tolist())
        assert {0, 1, EXACT} <= set(want[3].tolist())
        check(rc.hnsw(ida).search_range_allowed_sets(rc.q, rad, masks, set_of, ida.Search(), counters=True), want[:5], f"set {j}, the whole ladder")
    lds_rung0_refused(ida, rc.c, lambda hb: hb.search_range_allowed(rc.q, rad, masks[0], ida.Search()))


# ---- 10. HnswMap ---------------------------------------------------------------------------------------------------------------
def test_hnsw_map(eng):
    ida, kind = eng
    rng = np.random.default_rng(2)
    pts = rng.random((120, 5), dtype=np.float32)
    values = [f"v{i}" for i in range(120)]
    m = ida.Builder().seed(7).ef_search(12).build(pts, values)
    q = rng.random((4, 5), dtype=np.float32)
    rad = np.array([0.05, 0.2, 0.4, 10.0], np.float32)
    mask = rng.random(120) < 0.4
    items = m.search_range_allowed(q, rad, mask, ida.Search())
    r = m.hnsw.search_range_allowed(q, rad, mask, ida.Search())
    assert len(items) == 4 and len(items[3]) == int(mask.sum()) and len(items[2]) >= 1
    for i, its in enumerate(items):
        lo, hi = int(r.lims[i]), int(r.lims[i + 1])
        assert [it.pid for it in its] == r.pid[lo:hi].tolist()
        assert [np.float32(it.distance) for it in its] == r.distance[lo:hi].tolist() and all(it.distance <= rad[i] and mask[it.pid] for it in its)
        assert all(it.value == m.values[it.pid] and np.array_equal(it.point, m.hnsw[it.pid]) for it in its)
    sets = m.search_range_allowed_sets(q, rad, [mask, ~mask], [0, 1, 0, 1], ida.Search())
    assert [it.pid for it in sets[2]] == [it.pid for it in items[2]] and all(not mask[it.pid] for it in sets[3]) and len(sets[3]) == int((~mask).sum())


# ---- 11. NaN and +-inf in a query ------------------------------------------------------------------------------------------------
def test_non_finite_queries(eng, oracle):
    ida, kind = eng
    n, dim, ef = S(kind, 400, 1500), 6, 8
    rng = np.random.default_rng(21)
    pts, q = rng.random((n, dim), dtype=np.float32), rng.random((8, dim), dtype=np.float32)
    q[0, 2], q[1, 0], q[2, 5], q[3, 1], q[4, 4], q[5, 3] = np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf
    rc = RCase(oracle, pts, q, ef)
    rad = np.array([np.inf, np.inf, np.inf, 1.0, 1.0, 1.0, np.inf, 0.5], np.float32)
    mask = rng.random(n) < 0.5
    h = rc.hnsw(ida)
    for m in (-1, 0):
        want = model(rc, rad, [mask], np.zeros(8, np.int64), max_rungs=m)
        c = counts(want)
        assert c[0] == 0 and c[3] == 0 and c[4] == 0 and c[5] == 0        # a NaN distance is never within; inf is not <= 1
        assert c[1] > 0 and c[2] > 0 and c[6] > 0                         # inf <= inf
        got = h.search_range_allowed(q, rad, mask, ida.Search(), max_rungs=m, counters=True)
        check(got, want[:5], f"max_rungs {m}")
        assert np.all(np.isposinf(got.distance[int(got.lims[1]):int(got.lims[3])]))
    assert counts(model(rc, rad, [mask], np.zeros(8, np.int64), 0))[1] == int(mask.sum())
