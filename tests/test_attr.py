"""Attribute filters (include/idist.h): a u32 per point on the device, an interval per query, the bitmaps of
the restricted searches made by attr_bitmaps_kernel instead of being uploaded.

Every attribute call is DEFINED through the bitmap call it is listed with: with D the distinct (lo, hi) pairs of the call, bits[s]
the bitmap of pair s and set_of[q] the index of query q's pair, every output equals that call's given (bits, |D|, set_of).  So
everything is compared exactly (ids, order, counts, lims, rungs and counters with array_equal, distances as bit patterns) — against
the oracle-based models of the bitmap calls (tests/test_allowed.py, test_range_allowed.py, test_partitioned_allowed.py,
test_partitioned_range_allowed.py) with masks made by numpy from the same conditions, and against the bitmap call itself on the
same handle.  The kernel on its own is compared with a numpy packbits model.  Every case runs on the CPU emulator and (-m gpu) on
the MI355X."""
import ctypes as C
import mmap

import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params
from test_allowed import check as check_allowed
from test_allowed import main_case as allowed_case
from test_allowed_sets import rows_of, same
from test_partitioned_allowed import DeviceMem, guarded_words, main_parts
from test_partitioned_allowed import check as check_parts
from test_partitioned_allowed import expected as expected_parts
from test_partitioned_allowed import partitioned as partitioned_allowed
from test_partitioned_range import check as check_range_parts
from test_partitioned_range import partitioned as partitioned_range
from test_partitioned_range import range_parts
from test_partitioned_range_allowed import want_of
from test_range import check as check_range
from test_range import radii_of
from test_range_allowed import main_case as range_case
from test_range_allowed import model as range_model

NONE, EXACT = 254, 255
FILL = 0xABABABAB
TOP, FULL = 1 << 31, 0xFFFFFFFF


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


def S(kind, emu, gpu):
    return gpu if kind == "gpu" else emu


# ---- 1. the kernel on its own ----------------------------------------------------------------------------------------------------------
_GUARDED = []


def guarded_u32(n_words):
    """emulator only: n_words uint32 that END at a page no access is allowed to (tests/test_partitioned_allowed.py's guarded_words
    where one page is enough, several pages in front of the protected one otherwise)"""
    page = mmap.PAGESIZE
    if n_words * 4 <= page:
        return guarded_words(n_words)
    pages = (n_words * 4 + page - 1) // page
    mm = mmap.mmap(-1, (pages + 1) * page)
    addr = C.addressof(C.c_char.from_buffer(mm))
    libc = C.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    assert libc.mprotect(addr + pages * page, page, 0) == 0, C.get_errno()    # PROT_NONE
    _GUARDED.append(mm)
    return np.frombuffer(mm, dtype=np.uint32, count=n_words, offset=pages * page - 4 * n_words)


def bitmap_model(v, lo, hi):
    """[n_sets][(n + 31) // 32] by the kernel's contract: unsigned comparisons (uint64), bits at positions >= n zero"""
    n, words = len(v), (len(v) + 31) // 32
    v64 = v.astype(np.uint64)
    out = np.zeros((len(lo), words), np.uint32)
    for s in range(len(lo)):
        padded = np.zeros(words * 32, np.uint8)
        padded[:n] = (np.uint64(lo[s]) <= v64) & (v64 <= np.uint64(hi[s]))
        out[s] = np.packbits(padded, bitorder="little").view("<u4")
    return out


def conditions(rng, n_sets):
    """equality, everything, the empty set (lo > hi), the top half of the u32 range — a signed comparison gets it wrong —, then random
    intervals of the small range"""
    fixed = [(3, 3), (0, FULL), (5, 2), (TOP, FULL), (0, 0), (FULL, FULL), (1, TOP), (TOP, TOP)]
    lo = np.array([c[0] for c in fixed] + rng.integers(0, 8, max(n_sets - len(fixed), 0)).tolist(), np.uint32)[:n_sets]
    hi = np.array([c[1] for c in fixed] + rng.integers(0, 8, max(n_sets - len(fixed), 0)).tolist(), np.uint32)[:n_sets]
    return lo, hi


@pytest.mark.parametrize("n_sets", [1, 2, 65, 130])
def test_bitmap_kernel(eng, n_sets):
    """every word of every row against the model; an odd number of words per row (n = 33, 65, 95, 4097, 8007): the second word of the
    last window does not exist and every other row starts on an address that is no multiple of 8; the output pre-filled with a pattern
    and followed by guard words; on the emulator the values end at a protected page"""
    ida, kind = eng
    from instant_distance_amd import _capi

    L = _capi.lib()
    rng = np.random.default_rng(200 + n_sets)
    mem = DeviceMem(kind)
    try:
        lo, hi = conditions(rng, n_sets)
        d_lo, d_hi = mem.up(lo), mem.up(hi)
        for n in (1, 31, 32, 33, 63, 64, 65, 95, 4095, 4096, 4097, 8007):
            words = (n + 31) // 32
            v = guarded_u32(n) if kind == "emu" else np.empty(n, np.uint32)
            v[:] = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, 0, TOP, FULL], np.uint32), n)
            v[-1] = (FULL, TOP, 3)[n % 3]                                   # the last point decides the last bit
            out = np.full(n_sets * words + 5, FILL, np.uint32)
            d_v, d_out = mem.up(v), mem.up(out)
            L.check(L.idist_attr_bitmaps_device(d_v, n, d_lo, d_hi, n_sets, d_out, 0, None))
            got = mem.down(d_out, out)
            want = bitmap_model(v, lo, hi)
            assert np.array_equal(got[: n_sets * words].reshape(n_sets, words), want), (n_sets, n)
            assert np.all(got[n_sets * words:] == FILL), (n_sets, n)        # nothing behind the last row
            if n >= 64:
                assert want[1 % n_sets].any() or n_sets == 1
        # nothing to do: accepted, nothing written
        out = np.full(8, FILL, np.uint32)
        d_v, d_out = mem.up(np.zeros(8, np.uint32)), mem.up(out)
        L.check(L.idist_attr_bitmaps_device(d_v, 0, d_lo, d_hi, n_sets, d_out, 0, None))
        L.check(L.idist_attr_bitmaps_device(d_v, 8, d_lo, d_hi, 0, d_out, 0, None))
        assert np.all(mem.down(d_out, out) == FILL)
        assert L.idist_attr_bitmaps_device(None, 8, d_lo, d_hi, n_sets, d_out, 0, None) == 1
        assert L.idist_attr_bitmaps_device(d_v, 8, d_lo, d_hi, n_sets, None, 0, None) == 1
    finally:
        mem.free()


def test_bitmap_kernel_past_the_grid(eng):
    """more work items than workgroups.  attr_grid never cuts the sets into more chunks than the CUs want waves, so its cap binds only
    once the TILES alone exceed it: n > 4096 x 32 x the CU count (33.5M points on 256 CUs, 131,072 under the emulator's one) — a
    workgroup then takes tile t and tile t + grid.  n ends 37 points into a tile: no multiple of 64."""
    # cap: min(items, n_cu * 32) workgroups of one (tile, chunk of sets) each, attr_grid (idist_capi.hip)
    from engines import cu_count
    ida, kind = eng
    from instant_distance_amd import _capi

    L = _capi.lib()
    n = (cu_count(kind) * 32 + 1) * 4096 + 37
    words = (n + 31) // 32
    rng = np.random.default_rng(250)
    lo, hi = np.array([3, TOP], np.uint32), np.array([5, FULL], np.uint32)
    v = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, 0, TOP, FULL], np.uint32), n)
    v[-1] = 3
    mem = DeviceMem(kind)
    try:
        out = np.full(2 * words + 5, FILL, np.uint32)
        d_out = mem.up(out)
        L.check(L.idist_attr_bitmaps_device(mem.up(v), n, mem.up(lo), mem.up(hi), 2, d_out, 0, None))
        got = mem.down(d_out, out)
        assert np.array_equal(got[: 2 * words].reshape(2, words), bitmap_model(v, lo, hi))
        assert np.all(got[2 * words:] == FILL)
    finally:
        mem.free()


# ---- the attribute and the conditions of the parity tests ------------------------------------------------------------------------------
def attribute(n, seed, groups=100):
    """a uniform category in [0, groups) per point; one point alone in its category far above 2^31; a few points at 0xFFFFFFFF"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, groups, n).astype(np.uint32)
    special = rng.choice(n, 4, replace=False)
    v[special[0]] = TOP + 5
    v[special[1:]] = FULL
    return v


# (lo, hi): equality; intervals of 5 %, a half and everything; the empty set; one point; the top of the range; equality again
CONDS = [(7, 7), (10, 14), (0, 49), (0, FULL), (9, 3), (TOP + 5, TOP + 5), (TOP, FULL), (21, 21), (50, 99), (7, 7)]


def batch_conditions(nq, shift=0):
    """(lo [nq], hi [nq], the distinct pairs in first-appearance order, set_of [nq] into them): query q uses CONDS[(q + shift) % 10] —
    repeated conditions, and (7, 7) listed twice"""
    pairs = [CONDS[(q + shift) % len(CONDS)] for q in range(nq)]
    lo, hi = np.array([p[0] for p in pairs], np.uint64), np.array([p[1] for p in pairs], np.uint64)
    distinct = list(dict.fromkeys(pairs))
    set_of = np.array([distinct.index(p) for p in pairs], np.uint32)
    return lo, hi, distinct, set_of


def masks_of(v, distinct):
    v64 = v.astype(np.uint64)
    return [(np.uint64(lo) <= v64) & (v64 <= np.uint64(hi)) for lo, hi in distinct]


# ---- 2. parity of each attribute call -----------------------------------------------------------------------------------------------------
def test_search_where_parity(eng, oracle):
    ida, kind = eng
    c, k = allowed_case(oracle, kind)
    h, s = c.hnsw(ida), ida.Search()
    n, nq = len(c.pts), len(c.q)
    v = attribute(n, 5)
    attr = h.attributes(v)
    seen = set()
    for max_rungs, shift in ((-1, 0), (2, 3), (0, 6)):
        lo, hi, distinct, set_of = batch_conditions(nq, shift)
        masks = masks_of(v, distinct)
        assert [int(m.sum()) for m in masks][4:6] == [0, 1] or shift                     # the empty set and the set of one point
        want = rows_of([c.model(m, k, max_rungs) for m in masks], set_of)
        print("max_rungs", max_rungs, "rungs", dict(zip(*[x.tolist() for x in np.unique(want[3], return_counts=True)])))
        got = h.search_where(c.q, attr, lo, hi, k, s, max_rungs=max_rungs, counters=True)
        check_allowed(got, want, f"max_rungs {max_rungs}")
        check_allowed(h.search_where(c.q, attr, lo, hi, k, s, max_rungs=max_rungs), want, f"max_rungs {max_rungs}, no counters")
        same(got, h.search_allowed_sets(c.q, masks, set_of, k, s, max_rungs=max_rungs, counters=True), "the bitmap call, same handle")
        seen |= set(want[3].tolist())
    assert len({r for r in seen if r < NONE}) >= 2 and EXACT in seen and NONE in seen   # the ladder climbs; exact; nothing to find
    assert s.attr_bitmap_ms() >= 0.0
    # one condition for the whole batch: scalars, hi=None is equality
    for lo1, hi1 in ((0, 49), (7, None), (9, 3)):
        mask = masks_of(v, [(lo1, lo1 if hi1 is None else hi1)])[0]
        check_allowed(h.search_where(c.q, attr, lo1, hi1, k, s, counters=True), c.model(mask, k), f"one condition {lo1, hi1}")


def test_search_range_where_parity(eng, oracle):
    ida, kind = eng
    rc = range_case(oracle, kind)
    h, s = rc.hnsw(ida), ida.Search()
    n, nq = len(rc.raw), len(rc.q)
    assert n % 32 != 0
    v = attribute(n, 6)
    attr = h.attributes(v)
    rad = radii_of(rc)
    seen = set()
    for max_rungs, shift in ((-1, 0), (1, 1), (0, 5)):
        lo, hi, distinct, set_of = batch_conditions(nq, shift)
        masks = masks_of(v, distinct)
        want = range_model(rc, rad, masks, set_of, max_rungs=max_rungs)[:5]
        print("max_rungs", max_rungs, "rungs", dict(zip(*[x.tolist() for x in np.unique(want[3], return_counts=True)])))
        got = h.search_range_where(rc.q, rad, attr, lo, hi, s, max_rungs=max_rungs, counters=True)
        check_range(got, want, f"max_rungs {max_rungs}")
        check_range(h.search_range_where(rc.q, rad, attr, lo, hi, s, max_rungs=max_rungs), want, f"max_rungs {max_rungs}, no counters")
        o = h.search_range_allowed_sets(rc.q, rad, masks, set_of, s, max_rungs=max_rungs, counters=True)
        assert np.array_equal(got.lims, o.lims) and np.array_equal(got.pid, o.pid) and np.array_equal(got.rung, o.rung)
        assert np.array_equal(pc.bits(got.distance), pc.bits(o.distance)) and np.array_equal(got.counters, o.counters)
        seen |= set(want[3].tolist())
    assert 0 in seen and EXACT in seen and NONE in seen and int(want[0][-1]) > 0
    want = range_model(rc, rad[3], masks_of(v, [(10, 14)]), np.zeros(nq, np.int64))[:5]
    check_range(h.search_range_where(rc.q, float(rad[3]), attr, 10, 14, s, counters=True), want, "one radius, one condition")


@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_partitioned_search_where_parity(eng, oracle, P):
    ida, kind = eng
    pts, q, b, cs, k = main_parts(oracle, kind, P)
    n, nq = len(pts), len(q)
    if P == 3 or (kind == "emu" and P > 1):
        assert any(x % 32 for x in b[:-1])                                  # a base that is no multiple of 32
    ph, hs = partitioned_allowed(ida, cs)
    v = attribute(n, 7)
    v[b[P - 1]:][v[b[P - 1]:] == 21] = 22
    v[: b[P - 1]][v[: b[P - 1]] == 22] = 21                                # category 22 lives in the last part only, 21 in the others
    attr = ph.attributes(v)
    seen = set()
    for max_rungs, shift in ((-1, 0), (2, 3), (0, 6)):
        lo, hi, distinct, set_of = batch_conditions(nq, shift)
        masks = masks_of(v, distinct)
        want = expected_parts(cs, b, masks, set_of, k, max_rungs)
        got = ph.search_where(q, attr, lo, hi, k, max_rungs=max_rungs, counters=True)
        check_parts(got, want, f"max_rungs {max_rungs}")
        check_parts(ph.search_where(q, attr, lo, hi, k, max_rungs=max_rungs), want, f"max_rungs {max_rungs}, no counters")
        o = ph.search_allowed_sets(q, masks, set_of, k, max_rungs=max_rungs, counters=True)
        assert np.array_equal(got.rung, o.rung)
        same(got, o, "the bitmap call, same handle")
        seen |= set(want[3].ravel().tolist())
    assert EXACT in seen and NONE in seen and any(r < NONE for r in seen)
    assert ph.last_allowed_slice_ms() >= 0.0
    want = expected_parts(cs, b, masks_of(v, [(22, 22)]), np.zeros(nq, np.int64), k)
    check_parts(ph.search_where(q, attr, 22, None, k, counters=True), want, "one condition")
    if P > 1:
        assert np.all(want[3][:, : P - 1] == NONE)                          # a part that holds none of the category


@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_partitioned_search_range_where_parity(eng, oracle, P):
    ida, kind = eng
    pts, q, b, rcs, w = range_parts(oracle, kind, P)
    n, nq = len(pts), len(q)
    ph, hs = partitioned_range(ida, rcs)
    v = attribute(n, 8)
    attr = ph.attributes(v)
    rad = radii_of(w)
    seen = set()
    for max_rungs, shift in ((-1, 0), (1, 1), (0, 5)):
        lo, hi, distinct, set_of = batch_conditions(nq, shift)
        masks = masks_of(v, distinct)
        want, _ = want_of(rcs, b, masks, set_of, rad, max_rungs)
        got = ph.search_range_where(q, rad, attr, lo, hi, max_rungs=max_rungs, counters=True)
        check_range_parts(got, want, f"max_rungs {max_rungs}")
        check_range_parts(ph.search_range_where(q, rad, attr, lo, hi, max_rungs=max_rungs), want, f"max_rungs {max_rungs}, no counters")
        o = ph.search_range_allowed_sets(q, rad, masks, set_of, max_rungs=max_rungs, counters=True)
        assert np.array_equal(got.lims, o.lims) and np.array_equal(got.pid, o.pid) and np.array_equal(got.rung, o.rung)
        assert np.array_equal(pc.bits(got.distance), pc.bits(o.distance)) and np.array_equal(got.counters, o.counters)
        seen |= set(want[3].ravel().tolist())
    assert 0 in seen and EXACT in seen and NONE in seen and int(want[0][-1]) > 0
    want, _ = want_of(rcs, b, masks_of(v, [(0, 49)]), np.zeros(nq, np.int64), rad[3])
    check_range_parts(ph.search_range_where(q, float(rad[3]), attr, 0, 49, counters=True), want, "one radius, one condition")


# ---- 3. trivial cases -----------------------------------------------------------------------------------------------------------------------
def test_nothing_to_find(eng):
    ida, kind = eng
    rng = np.random.default_rng(3)
    q = rng.random((4, 5), dtype=np.float32)
    h0 = ida.Hnsw.from_ordered_points(np.zeros((0, 5), np.float32), ida.Builder())
    a0 = h0.attributes(np.zeros(0, np.uint32))                              # n == 0 is legal
    r = h0.search_where(q, a0, 1, 2, 3, ida.Search(), counters=True)
    assert len(a0) == 0 and np.all(r.count == 0) and np.all(r.rung == NONE) and np.all(r.pid == 0xFFFFFFFF) and np.all(r.counters == 0)
    rr = h0.search_range_where(q, 1.0, a0, 1, 2, ida.Search(), counters=True)
    assert np.all(rr.lims == 0) and np.all(rr.rung == NONE) and rr.pid.shape == (0,)
    ph0, _ = ida.PartitionedHnsw.build(np.zeros((0, 5), np.float32), ida.Builder(), parts=2)
    pa0 = ph0.attributes([])
    r = ph0.search_where(q, pa0, np.arange(4), None, 3, counters=True)
    assert r.rung.shape == (4, 2) and np.all(r.rung == NONE) and np.all(r.count == 0)
    rr = ph0.search_range_where(q, 1.0, pa0, 0, 9, counters=True)
    assert np.all(rr.lims == 0) and rr.rung.shape == (4, 2) and np.all(rr.rung == NONE)
    # no queries
    pts = rng.random((40, 5), dtype=np.float32)
    h = ida.Hnsw.from_ordered_points(pts, ida.Builder().ef_search(10))
    a = h.attributes(np.arange(40))
    e = h.search_where(np.zeros((0, 5), np.float32), a, 1, 2, 3, ida.Search(), counters=True)
    assert e.pid.shape == (0, 3) and e.rung.shape == (0,) and e.counters.shape == (0, 3)
    e = h.search_range_where(np.zeros((0, 5), np.float32), 1.0, a, np.zeros(0, np.int64), None, ida.Search())
    assert np.array_equal(e.lims, np.zeros(1, np.uint64))
    # fewer points than parts: two of the five parts are empty
    ph, ids = ida.PartitionedHnsw.build(pts[:3], ida.Builder().seed(1), parts=5)
    pa = ph.attributes([4, 9, 4])
    r = ph.search_where(q, pa, 4, None, 2, counters=True)
    assert np.all(r.count == 2) and np.all(np.sort(r.pid, axis=1) == np.array([0, 2], np.uint32)) and r.rung.shape == (4, 5)
    rr = ph.search_range_where(q, np.inf, pa, 9, 9)
    assert np.array_equal(rr.lims, np.arange(5, dtype=np.uint64)) and np.all(rr.pid == 1)


# ---- 4. argument errors -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors(eng):
    ida, kind = eng
    from instant_distance_amd import _capi

    rng = np.random.default_rng(1)
    pts = rng.random((50, 4), dtype=np.float32)
    mk = lambda rows, ef=10: ida.Hnsw.from_ordered_points(np.ascontiguousarray(rows), ida.Builder().ef_search(ef))   # noqa: E731
    h0, h1, other = mk(pts[:21]), mk(pts[21:]), mk(pts[:21])
    ph, ph2 = ida.PartitionedHnsw.from_hnsws([h0, h1]), ida.PartitionedHnsw.from_hnsws([h0, h1])
    a0, a_other = h0.attributes(np.arange(21)), other.attributes(np.arange(21))
    pa, pa2 = ph.attributes(np.arange(50)), ph2.attributes(np.arange(50))
    s = ida.Search()
    q = pts[:3]
    L = _capi.lib()
    nq, k = 3, 5
    lo, hi = np.array([0, 5, 30], np.uint32), np.array([40, 9, 49], np.uint32)
    rad = np.full(3, np.inf, np.float32)
    pid, dist, cnt = np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.float32), np.zeros(nq, np.uint32)
    lims = np.zeros(nq + 1, np.uint64)
    ctx = s._bind(h0)
    u, f = _capi.u32p, _capi.f32p

    def topk(attr=a0, n_cond=3, lo_=lo, hi_=hi, queries=q, out=pid, kk=k, max_rungs=-1):
        return L.idist_search_batch_attr(h0._h, ctx, None if attr is None else attr._h, None if queries is None else f(queries), nq,
                                         None if lo_ is None else u(lo_), None if hi_ is None else u(hi_), n_cond, kk, max_rungs,
                                         None if out is None else u(out), f(dist), u(cnt), None, None)

    def rng_(attr=a0, n_cond=3, radius=rad, lo_=lo, out=lims):
        return L.idist_search_batch_range_attr(h0._h, ctx, None if attr is None else attr._h, f(q), nq, f(radius), 3, None if lo_ is None else u(lo_),
                                               u(hi), n_cond, -1, 1 << 40, None if out is None else _capi.u64p(out), None, None)

    def ptopk(attr=pa, n_cond=3, lo_=lo, queries=q):
        return L.idist_partitioned_search_batch_attr(ph._h, None if attr is None else attr._h, None if queries is None else f(queries), nq,
                                                     None if lo_ is None else u(lo_), u(hi), n_cond, k, -1, u(pid), f(dist), u(cnt), None, None)

    def prng(attr=pa, n_cond=3, radius=rad, hi_=hi):
        return L.idist_partitioned_search_batch_range_attr(ph._h, None if attr is None else attr._h, f(q), nq, f(radius), 3, u(lo),
                                                           None if hi_ is None else u(hi_), n_cond, -1, 1 << 40, _capi.u64p(lims), None, None)

    assert topk() == 0 and cnt.tolist() == [5, 5, 0] and rng_() == 0 and ptopk() == 0 and prng() == 0    # out_rung / out_counters may be NULL
    # a foreign attribute; an index's attribute in a partitioned call and the reverse; none at all
    assert topk(attr=a_other) == 1 and rng_(attr=a_other) == 1 and ptopk(attr=pa2) == 1 and prng(attr=pa2) == 1
    assert topk(attr=pa) == 1 and rng_(attr=pa) == 1 and ptopk(attr=a0) == 1 and prng(attr=a0) == 1
    assert topk(attr=None) == 1 and rng_(attr=None) == 1 and ptopk(attr=None) == 1 and prng(attr=None) == 1
    # n_cond is 1 or nq
    for n_cond in (0, 2, 4):
        assert topk(n_cond=n_cond) == 1 and rng_(n_cond=n_cond) == 1 and ptopk(n_cond=n_cond) == 1 and prng(n_cond=n_cond) == 1
    assert b"n_cond" in L.idist_last_error()
    assert topk(n_cond=1) == 0 and cnt.tolist() == [5, 5, 5]
    # a NaN radius names the query
    bad = rad.copy()
    bad[2] = np.nan
    assert rng_(radius=bad) == 1 and b"query 2" in L.idist_last_error()
    assert prng(radius=bad) == 1 and b"query 2" in L.idist_last_error()
    # null pointers; the arguments of the calls they equal
    assert topk(lo_=None) == 1 and topk(hi_=None) == 1 and topk(queries=None) == 1 and topk(out=None) == 1
    assert rng_(lo_=None) == 1 and rng_(out=None) == 1 and ptopk(lo_=None) == 1 and ptopk(queries=None) == 1 and prng(hi_=None) == 1
    assert topk(kk=0) == 1 and topk(kk=11) == 1 and topk(max_rungs=-2) == 1
    out = C.c_void_p()
    assert L.idist_attr_new(None, u(lo), C.byref(out)) == 1 and L.idist_attr_new(h0._h, None, C.byref(out)) == 1
    assert L.idist_attr_new(h0._h, u(lo), None) == 1 and L.idist_partitioned_attr_new(ph._h, None, C.byref(out)) == 1
    L.idist_attr_free(None)
    ms = C.c_float(-1.0)
    assert L.idist_search_ctx_attr_bitmap_ms(None, C.byref(ms)) == 1 and L.idist_search_ctx_attr_bitmap_ms(ctx, C.byref(ms)) == 0 and ms.value >= 0.0
    # the Python layer raises for the same things
    with pytest.raises(ida.IdistError) as e:
        h0.search_where(q, a_other, 1, 2, k, s)
    assert e.value.status == 1
    with pytest.raises(ida.IdistError):
        ph.search_where(q, a0, 1, 2, k)
    with pytest.raises(ida.IdistError):
        h0.search_range_where(q, 1.0, pa, 1, 2, s)


# ---- 5. Python ------------------------------------------------------------------------------------------------------------------------------
def test_python_layer(eng):
    ida, kind = eng
    rng = np.random.default_rng(2)
    pts = rng.random((120, 5), dtype=np.float32)
    h, s = ida.Hnsw.from_ordered_points(pts, ida.Builder().ef_search(12)), ida.Search()
    v = rng.integers(0, 6, 120)
    attr = h.attributes(v)
    assert len(attr) == 120 and attr.values.dtype == np.uint32 and np.array_equal(attr.values, v)
    q = rng.random((4, 5), dtype=np.float32)
    k = 6
    mask = lambda lo, hi: (v >= lo) & (v <= hi)                             # noqa: E731
    # hi=None is equality; scalars against arrays; a scalar next to an array is repeated
    same(h.search_where(q, attr, 3, None, k, s), h.search_allowed(q, mask(3, 3), k, s), "equality, scalar")
    same(h.search_where(q, attr, np.array([3, 3, 3, 3]), None, k, s), h.search_allowed(q, mask(3, 3), k, s), "equality, array")
    lo, hi = np.array([0, 2, 5, 4]), np.array([1, 2, 5, 3])
    sets = [mask(a, b) for a, b in zip(lo, hi)]
    same(h.search_where(q, attr, lo, hi, k, s), h.search_allowed_sets(q, sets, None, k, s), "arrays")
    same(h.search_where(q, attr, 1, np.array([1, 2, 5, 0]), k, s), h.search_allowed_sets(q, [mask(1, b) for b in (1, 2, 5, 0)], None, k, s),
         "a scalar lo next to an array hi")
    same(h.search_where(q, attr, lo, None, k, s), h.search_allowed_sets(q, [mask(a, a) for a in lo], None, k, s), "equality per query")
    a = h.search_range_where(q, 0.5, attr, lo, hi, s, counters=True)
    o = h.search_range_allowed_sets(q, 0.5, sets, None, s, counters=True)
    assert np.array_equal(a.lims, o.lims) and np.array_equal(a.pid, o.pid) and np.array_equal(a.rung, o.rung) and int(a.lims[-1]) > 0
    assert np.array_equal(pc.bits(a.distance), pc.bits(o.distance)) and np.array_equal(a.counters, o.counters)
    assert isinstance(h.search_where(q, attr, 3), ida.AllowedResult)        # k and search have defaults
    # values and bounds outside u32 raise; so do wrong shapes and types
    for bad in (-1, 1 << 32, np.array([0, 1, 2, 1 << 32]), np.array([0, -1, 2, 3])):
        with pytest.raises(ValueError):
            h.search_where(q, attr, bad, None, k, s)
        with pytest.raises(ValueError):
            h.search_range_where(q, 0.5, attr, 0, bad, s)
    with pytest.raises(ValueError):
        h.attributes(np.full(120, -1))
    with pytest.raises(ValueError):
        h.attributes(np.full(120, 1 << 32))
    with pytest.raises(ValueError):
        h.attributes(np.zeros(119, np.uint32))
    with pytest.raises(TypeError):
        h.attributes(np.zeros(120, np.float32))
    with pytest.raises(TypeError):
        h.search_where(q, attr, 1.5, None, k, s)
    with pytest.raises(ValueError):
        h.search_where(q, attr, np.array([1, 2, 3]), None, k, s)            # one per query
    with pytest.raises(TypeError):
        h.search_where(q[:, :3], attr, 1, None, k, s)
    # HnswMap: the items carry their values
    values = [f"v{i}" for i in range(120)]
    m = ida.Builder().seed(7).ef_search(12).build(pts, values)
    tenant = np.array([int(x[1:]) % 7 for x in m.values])                   # PointId order, as m.values
    ma = m.attributes(tenant)
    items = m.search_where(q, ma, 2, 3, k, ida.Search())
    r = m.hnsw.search_where(q, ma, 2, 3, k, ida.Search())
    assert len(items) == 4
    for i, row in enumerate(items):
        assert [it.pid for it in row] == r.pid[i, : r.count[i]].tolist() and len(row) == k
        assert all(int(it.value[1:]) % 7 in (2, 3) and it.value == m.values[it.pid] and np.array_equal(it.point, m.hnsw[it.pid]) for it in row)
    ritems = m.search_range_where(q, 0.4, ma, 2, 3, ida.Search())
    rr = m.hnsw.search_range_where(q, 0.4, ma, 2, 3, ida.Search())
    assert [[it.pid for it in row] for row in ritems] == [rr.pid[int(rr.lims[i]): int(rr.lims[i + 1])].tolist() for i in range(4)]
    assert sum(len(row) for row in ritems) > 0 and all(int(it.value[1:]) % 7 in (2, 3) for row in ritems for it in row)
