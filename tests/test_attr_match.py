"""Attribute tables (include/idist.h): several u32 columns per point on the device, an OR of ANDs of interval
clauses per query, the bitmaps of the restricted searches made by attr_match_kernel.

Every match call is DEFINED through the bitmap call it is listed with: with bits[c] the bitmap of condition c, every output equals
that call's given (bits, n_cond, set_of = NULL).  So everything is compared exactly (ids, order, counts, lims, rungs and counters with
array_equal, distances as bit patterns) — against the oracle-based models of the bitmap calls with masks made by numpy from the same
conditions, and against the bitmap call itself on the same handle.  The kernel on its own is compared with a numpy model of the flat
program.  Every case runs on the CPU emulator and (-m gpu) on the MI355X; the encoder of the Python conditions needs neither."""
import ctypes as C
import mmap

import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params
from test_allowed import check as check_allowed
from test_allowed import main_case as allowed_case
from test_allowed_sets import rows_of, same
from test_attr import FILL, FULL, TOP, attribute, guarded_u32
from test_partitioned_allowed import DeviceMem, main_parts
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


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


# ---- 1. the kernel on its own ----------------------------------------------------------------------------------------------------------
_GUARDED = []


def guarded_columns(n, n_cols):
    """emulator only: n_cols columns of n uint32 in ONE mapping, EVERY column ending at a page no access is allowed to ->
    (the address of column 0, col_pitch in elements, the columns as arrays)"""
    page = mmap.PAGESIZE
    pages = (n * 4 + page - 1) // page
    mm = mmap.mmap(-1, n_cols * (pages + 1) * page)
    addr = C.addressof(C.c_char.from_buffer(mm))
    libc = C.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    for c in range(n_cols):
        assert libc.mprotect(addr + (c * (pages + 1) + pages) * page, page, 0) == 0, C.get_errno()    # PROT_NONE
    _GUARDED.append(mm)
    first = pages * page - 4 * n
    cols = [np.frombuffer(mm, dtype=np.uint32, count=n, offset=c * (pages + 1) * page + first) for c in range(n_cols)]
    return addr + first, (pages + 1) * page // 4, cols


def program(rng, n_sets, n_cols):
    """n_sets conditions, each a list of conjunctions, each a list of (col, lo, hi); the columns a three-column program names are
    folded into the table's.  FALSE, TRUE, one clause, lo > hi, the top half of the u32 range (a signed comparison gets it wrong), a
    column twice in a conjunction, two overlapping conjunctions, a conjunction over all three columns, a membership list of 70
    one-clause conjunctions, TRUE or FALSE next to a clause; then random small ones"""
    fixed = [
        [[(0, 0, 5), (1, 1, 7), (2, 2, FULL)]],
        [[(1, TOP, FULL)]],
        [],
        [[]],
        [[(0, 3, 3)]],
        [[(0, 5, 2)]],
        [[(0, 1, 6), (0, 3, 9)]],
        [[(0, 0, 4)], [(0, 3, 7)]],
        [[(i % 3, (i * 7) % 11, (i * 7) % 11)] for i in range(70)],
        [[(2, 1, 1)], []],
        [[(0, 5, 2)], [(1, 0, 0), (0, FULL, FULL)]],
        [[(0, 0, FULL), (1, 0, FULL), (2, 0, FULL), (1, 2, TOP)]],
    ]
    conds = fixed[:n_sets]
    edge = [0, 1, 2, 3, 4, 5, 6, 7, 8, TOP, FULL]
    while len(conds) < n_sets:
        conds.append([[(int(rng.integers(0, 3)), int(rng.choice(edge)), int(rng.choice(edge))) for _ in range(rng.integers(0, 4))]
                      for _ in range(rng.integers(0, 4))])
    return [[[(col % n_cols, lo, hi) for col, lo, hi in conj] for conj in cond] for cond in conds]


def flat(conds):
    """(clauses uint32 [m, 3], and_lims, or_lims) of a list of conditions"""
    clauses, and_lims, or_lims = [], [0], [0]
    for cond in conds:
        for conj in cond:
            clauses += conj
            and_lims.append(len(clauses))
        or_lims.append(len(and_lims) - 1)
    return np.array(clauses, np.uint32).reshape(-1, 3), np.array(and_lims, np.uint32), np.array(or_lims, np.uint32)


def program_model(cols, clauses, and_lims, or_lims):
    """[n_sets][(n + 31) // 32] by the kernel's contract, from the flat program: unsigned comparisons (uint64), bits at positions >= n
    zero"""
    n, words = len(cols[0]), (len(cols[0]) + 31) // 32
    c64 = [c.astype(np.uint64) for c in cols]
    out = np.zeros((len(or_lims) - 1, words), np.uint32)
    for s in range(len(or_lims) - 1):
        cond = np.zeros(n, bool)
        for j in range(or_lims[s], or_lims[s + 1]):
            conj = np.ones(n, bool)
            for col, lo, hi in clauses[and_lims[j]: and_lims[j + 1]]:
                conj &= (np.uint64(lo) <= c64[col]) & (c64[col] <= np.uint64(hi))
            cond |= conj
        padded = np.zeros(words * 32, np.uint8)
        padded[:n] = cond
        out[s] = np.packbits(padded, bitorder="little").view("<u4")
    return out


@pytest.mark.parametrize("n_cols", [1, 3])
@pytest.mark.parametrize("n_sets", [1, 2, 65, 130])
def test_match_kernel(eng, n_sets, n_cols):
    """every word of every row against the model, for col_pitch == n and n + 5 (and, on the emulator, a third layout in which EVERY
    column ends at a protected page; in the first two the table does); an odd number of words per row (n = 33, 65, 95, 4097, 8007):
    the second word of the last window does not exist and every other row starts on an address that is no multiple of 8; the output
    pre-filled with a pattern and followed by guard words"""
    ida, kind = eng
    from instant_distance_amd import _capi

    L = _capi.lib()
    rng = np.random.default_rng(300 + n_sets + n_cols)
    mem = DeviceMem(kind)
    try:
        conds = program(rng, n_sets, n_cols)
        clauses, and_lims, or_lims = flat(conds)
        d_cl, d_al, d_ol = mem.up(clauses if len(clauses) else np.zeros((1, 3), np.uint32)), mem.up(and_lims), mem.up(or_lims)
        for n in (1, 31, 32, 33, 63, 64, 65, 95, 4095, 4096, 4097, 8007):
            words = (n + 31) // 32
            vals = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, 0, TOP, FULL], np.uint32), (n_cols, n))
            vals[:, -1] = [(FULL, TOP, 3)[(n + c) % 3] for c in range(n_cols)]            # the last point decides the last bit
            want = program_model(list(vals), clauses, and_lims, or_lims)
            for layout in ("n", "n + 5") + (("pages",) if kind == "emu" else ()):
                if layout == "pages":
                    d_v, pitch, cols = guarded_columns(n, n_cols)
                    for c in range(n_cols):
                        cols[c][:] = vals[c]
                else:
                    pitch = n if layout == "n" else n + 5
                    size = (n_cols - 1) * pitch + n
                    table = guarded_u32(size) if kind == "emu" else np.empty(size, np.uint32)
                    table[:] = 0xDEADBEEF                                                 # (the gaps between the columns match no clause)
                    for c in range(n_cols):
                        table[c * pitch: c * pitch + n] = vals[c]
                    d_v = mem.up(table)
                out = np.full(n_sets * words + 5, FILL, np.uint32)
                d_out = mem.up(out)
                L.check(L.idist_attr_match_bitmaps_device(d_v, n, n_cols, pitch, d_cl, d_al, d_ol, n_sets, d_out, 0, None))
                got = mem.down(d_out, out)
                assert np.array_equal(got[: n_sets * words].reshape(n_sets, words), want), (n_sets, n_cols, n, layout)
                assert np.all(got[n_sets * words:] == FILL), (n_sets, n_cols, n, layout)  # nothing behind the last row
            if n >= 64:
                assert want[0].any() and (n_sets < 4 or (not want[2].any() and want[3, : n // 32].min() == FULL))   # FALSE and TRUE
        # nothing to do: accepted, nothing written
        out = np.full(8, FILL, np.uint32)
        d_v, d_out = mem.up(np.zeros(8 * n_cols, np.uint32)), mem.up(out)
        L.check(L.idist_attr_match_bitmaps_device(d_v, 0, n_cols, 8, d_cl, d_al, d_ol, n_sets, d_out, 0, None))
        L.check(L.idist_attr_match_bitmaps_device(d_v, 8, n_cols, 8, d_cl, d_al, d_ol, 0, d_out, 0, None))
        assert np.all(mem.down(d_out, out) == FILL)
        # null pointers, a pitch below n, no columns
        assert L.idist_attr_match_bitmaps_device(None, 8, n_cols, 8, d_cl, d_al, d_ol, n_sets, d_out, 0, None) == 1
        assert L.idist_attr_match_bitmaps_device(d_v, 8, n_cols, 8, d_cl, None, d_ol, n_sets, d_out, 0, None) == 1
        assert L.idist_attr_match_bitmaps_device(d_v, 8, n_cols, 8, d_cl, d_al, None, n_sets, d_out, 0, None) == 1
        assert L.idist_attr_match_bitmaps_device(d_v, 8, n_cols, 8, d_cl, d_al, d_ol, n_sets, None, 0, None) == 1
        assert L.idist_attr_match_bitmaps_device(d_v, 8, n_cols, 7, d_cl, d_al, d_ol, n_sets, d_out, 0, None) == 1
        assert L.idist_attr_match_bitmaps_device(d_v, 8, 0, 8, d_cl, d_al, d_ol, n_sets, d_out, 0, None) == 1
        assert np.all(mem.down(d_out, out) == FILL)
    finally:
        mem.free()


def test_match_kernel_past_the_grid(eng):
    """tests/test_attr.py's test_bitmap_kernel_past_the_grid for attr_match_kernel: two columns, col_pitch = n + 5, more tiles than
    workgroups (the grid is attr_grid's), n no multiple of 64; a workgroup keeps a loaded tile while consecutive clauses name its
    column — condition 0 ends and condition 1 starts on column 1, so the kept tile must not outlive the work item"""
    # cap: min(items, n_cu * 32) workgroups of one (tile, chunk of sets) each, attr_grid (idist_capi.hip)
    from engines import cu_count
    ida, kind = eng
    from instant_distance_amd import _capi

    L = _capi.lib()
    n = (cu_count(kind) * 32 + 1) * 4096 + 37
    words, pitch = (n + 31) // 32, n + 5
    rng = np.random.default_rng(350)
    conds = [[[(0, 1, 6), (1, 2, TOP)]], [[(1, 3, 3)], [(0, TOP, FULL)]]]
    clauses, and_lims, or_lims = flat(conds)
    vals = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, 0, TOP, FULL], np.uint32), (2, n))
    vals[:, -1] = (3, 3)
    table = np.full(pitch + n, 0xDEADBEEF, np.uint32)
    table[:n], table[pitch:] = vals[0], vals[1]
    mem = DeviceMem(kind)
    try:
        out = np.full(2 * words + 5, FILL, np.uint32)
        d_out = mem.up(out)
        L.check(L.idist_attr_match_bitmaps_device(mem.up(table), n, 2, pitch, mem.up(clauses), mem.up(and_lims), mem.up(or_lims), 2, d_out, 0, None))
        got = mem.down(d_out, out)
        assert np.array_equal(got[: 2 * words].reshape(2, words), program_model(list(vals), clauses, and_lims, or_lims))
        assert np.all(got[2 * words:] == FILL)
    finally:
        mem.free()


# ---- the table and the conditions of the parity tests -------------------------------------------------------------------------------------
def table_of(n, seed):
    """two columns: "a", tests/test_attr.py's attribute (a uniform category in [0, 100), one point alone at TOP + 5, a few at
    0xFFFFFFFF), and "b", uniform in [0, 4)"""
    return {"a": attribute(n, seed), "b": np.random.default_rng(seed + 1000).integers(0, 4, n).astype(np.uint32)}


def conds_list(ida):
    """a half; a quarter (two columns ANDed); a few percent (AnyOf of two equalities); TRUE; FALSE; the single point at TOP + 5; five
    percent; the first one written again, its columns in the other order in the quarter; a membership list ANDed with an interval"""
    A = ida.AnyOf
    return [{"a": (0, 49)}, {"a": (0, 49), "b": [0, 1]}, A({"a": 7}, {"a": 21}), {}, A(), {"a": TOP + 5}, {"a": (10, 14)}, {"a": (0, 49)},
            {"b": (0, 1), "a": (0, 49)}, A({"a": [50, 51, 52, 60, 99], "b": (1, 3)}, {"a": (TOP, FULL)})]


def mask_of(cond, cols):
    """the bool mask of a condition in the Python syntax, by numpy alone (unsigned: uint64)"""
    n = len(next(iter(cols.values())))
    out = np.zeros(n, bool)
    for d in ((cond,) if isinstance(cond, dict) else cond.conjunctions):
        conj = np.ones(n, bool)
        for name, spec in d.items():
            v = cols[name].astype(np.uint64)
            if isinstance(spec, tuple):
                conj &= (np.uint64(spec[0]) <= v) & (v <= np.uint64(spec[1]))
            elif isinstance(spec, (list, set, np.ndarray)):
                conj &= np.isin(v, np.array(sorted(spec), np.uint64))
            else:
                conj &= v == np.uint64(spec)
        out |= conj
    return out


def batch(ida, cols, nq, shift=0):
    """(the conditions of the nq queries, the masks of the list's conditions, set_of [nq] into them): query q uses condition
    (q + shift) % 10 of conds_list — repeated conditions, and one of them written twice"""
    cl = conds_list(ida)
    set_of = np.array([(q + shift) % len(cl) for q in range(nq)], np.uint32)
    return [cl[s] for s in set_of], [mask_of(c, cols) for c in cl], set_of


# ---- 2. parity of each match call -----------------------------------------------------------------------------------------------------------
def test_search_match_parity(eng, oracle):
    ida, kind = eng
    c, k = allowed_case(oracle, kind)
    h, s = c.hnsw(ida), ida.Search()
    n, nq = len(c.pts), len(c.q)
    cols = table_of(n, 5)
    table = h.attribute_table(cols)
    assert table.names == ["a", "b"] and table.n_cols == 2 and len(table) == n and np.array_equal(table.columns["b"], cols["b"])
    seen = set()
    for max_rungs, shift in ((-1, 0), (2, 3), (0, 6)):
        conds, masks, set_of = batch(ida, cols, nq, shift)
        assert [int(m.sum()) for m in masks][3:6] == [n, 0, 1] and np.array_equal(masks[1], masks[8])   # TRUE, FALSE, the set of one point
        want = rows_of([c.model(m, k, max_rungs) for m in masks], set_of)
        print("max_rungs", max_rungs, "rungs", dict(zip(*[x.tolist() for x in np.unique(want[3], return_counts=True)])))
        got = h.search_match(c.q, table, conds, k, s, max_rungs=max_rungs, counters=True)
        check_allowed(got, want, f"max_rungs {max_rungs}")
        check_allowed(h.search_match(c.q, table, conds, k, s, max_rungs=max_rungs), want, f"max_rungs {max_rungs}, no counters")
        same(got, h.search_allowed_sets(c.q, masks, set_of, k, s, max_rungs=max_rungs, counters=True), "the bitmap call, same handle")
        seen |= set(want[3].tolist())
    assert len({r for r in seen if r < NONE}) >= 2 and EXACT in seen and NONE in seen   # the ladder climbs; exact; nothing to find
    assert s.attr_bitmap_ms() >= 0.0
    # one condition for the whole batch
    for cond in ({"a": (0, 49), "b": 2}, ida.AnyOf({"a": 7}, {"b": 3, "a": [1, 2, 3, 9]}), ida.AnyOf()):
        check_allowed(h.search_match(c.q, table, cond, k, s, counters=True), c.model(mask_of(cond, cols), k), f"one condition {cond}")


def test_search_range_match_parity(eng, oracle):
    ida, kind = eng
    rc = range_case(oracle, kind)
    h, s = rc.hnsw(ida), ida.Search()
    n, nq = len(rc.raw), len(rc.q)
    assert n % 32 != 0
    cols = table_of(n, 6)
    table = h.attribute_table(cols)
    rad = radii_of(rc)
    seen = set()
    for max_rungs, shift in ((-1, 0), (1, 1), (0, 5)):
        conds, masks, set_of = batch(ida, cols, nq, shift)
        want = range_model(rc, rad, masks, set_of, max_rungs=max_rungs)[:5]
        print("max_rungs", max_rungs, "rungs", dict(zip(*[x.tolist() for x in np.unique(want[3], return_counts=True)])))
        got = h.search_range_match(rc.q, rad, table, conds, s, max_rungs=max_rungs, counters=True)
        check_range(got, want, f"max_rungs {max_rungs}")
        check_range(h.search_range_match(rc.q, rad, table, conds, s, max_rungs=max_rungs), want, f"max_rungs {max_rungs}, no counters")
        o = h.search_range_allowed_sets(rc.q, rad, masks, set_of, s, max_rungs=max_rungs, counters=True)
        assert np.array_equal(got.lims, o.lims) and np.array_equal(got.pid, o.pid) and np.array_equal(got.rung, o.rung)
        assert np.array_equal(pc.bits(got.distance), pc.bits(o.distance)) and np.array_equal(got.counters, o.counters)
        seen |= set(want[3].tolist())
        assert int(want[0][-1]) > 0
    assert len({r for r in seen if r < NONE}) >= 2 and EXACT in seen and NONE in seen
    cond = {"a": (10, 29), "b": [1, 3]}
    want = range_model(rc, rad[3], [mask_of(cond, cols)], np.zeros(nq, np.int64))[:5]
    check_range(h.search_range_match(rc.q, float(rad[3]), table, cond, s, counters=True), want, "one radius, one condition")


def part_table(n, b, seed):
    """table_of, with category 22 of "a" living in the last part only and 21 in the others"""
    cols = table_of(n, seed)
    a, last = cols["a"], b[len(b) - 2]
    a[last:][a[last:] == 21] = 22
    a[:last][a[:last] == 22] = 21
    return cols


@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_partitioned_search_match_parity(eng, oracle, P):
    ida, kind = eng
    pts, q, b, cs, k = main_parts(oracle, kind, P)
    n, nq = len(pts), len(q)
    ph, hs = partitioned_allowed(ida, cs)
    cols = part_table(n, b, 7)
    table = ph.attribute_table(cols)
    assert len(table) == n and table.n_cols == 2
    seen = set()
    for max_rungs, shift in ((-1, 0), (2, 3), (0, 6)):
        conds, masks, set_of = batch(ida, cols, nq, shift)
        want = expected_parts(cs, b, masks, set_of, k, max_rungs)
        got = ph.search_match(q, table, conds, k, max_rungs=max_rungs, counters=True)
        check_parts(got, want, f"max_rungs {max_rungs}")
        check_parts(ph.search_match(q, table, conds, k, max_rungs=max_rungs), want, f"max_rungs {max_rungs}, no counters")
        o = ph.search_allowed_sets(q, masks, set_of, k, max_rungs=max_rungs, counters=True)
        assert np.array_equal(got.rung, o.rung)
        same(got, o, "the bitmap call, same handle")
        seen |= set(want[3].ravel().tolist())
    assert len({r for r in seen if r < NONE}) >= 2 and EXACT in seen and NONE in seen
    assert ph.last_allowed_slice_ms() >= 0.0
    cond = {"a": 22, "b": (0, 3)}
    want = expected_parts(cs, b, [mask_of(cond, cols)], np.zeros(nq, np.int64), k)
    check_parts(ph.search_match(q, table, cond, k, counters=True), want, "one condition")
    if P > 1:
        assert np.all(want[3][:, : P - 1] == NONE) and np.all(want[3][:, P - 1] != NONE)   # a part that holds none of the category


@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_partitioned_search_range_match_parity(eng, oracle, P):
    ida, kind = eng
    pts, q, b, rcs, w = range_parts(oracle, kind, P)
    n, nq = len(pts), len(q)
    ph, hs = partitioned_range(ida, rcs)
    cols = part_table(n, b, 8)
    table = ph.attribute_table(cols)
    rad = radii_of(w)
    seen = set()
    for max_rungs, shift in ((-1, 0), (1, 1), (0, 5)):
        conds, masks, set_of = batch(ida, cols, nq, shift)
        want, _ = want_of(rcs, b, masks, set_of, rad, max_rungs)
        got = ph.search_range_match(q, rad, table, conds, max_rungs=max_rungs, counters=True)
        check_range_parts(got, want, f"max_rungs {max_rungs}")
        check_range_parts(ph.search_range_match(q, rad, table, conds, max_rungs=max_rungs), want, f"max_rungs {max_rungs}, no counters")
        o = ph.search_range_allowed_sets(q, rad, masks, set_of, max_rungs=max_rungs, counters=True)
        assert np.array_equal(got.lims, o.lims) and np.array_equal(got.pid, o.pid) and np.array_equal(got.rung, o.rung)
        assert np.array_equal(pc.bits(got.distance), pc.bits(o.distance)) and np.array_equal(got.counters, o.counters)
        seen |= set(want[3].ravel().tolist())
        assert int(want[0][-1]) > 0
    assert 0 in seen and EXACT in seen and NONE in seen
    cond = {"a": 22}
    want, _ = want_of(rcs, b, [mask_of(cond, cols)], np.zeros(nq, np.int64), np.float32(np.inf))
    check_range_parts(ph.search_range_match(q, np.inf, table, cond, counters=True), want, "one radius, one condition")
    if P > 1:
        assert np.all(want[3][:, : P - 1] == NONE) and int(want[0][-1]) > 0               # a part that holds none of the category


# ---- 3. the special case: one conjunction of one clause on column 0 is the interval call --------------------------------------------------
def test_interval_special_case(eng):
    ida, kind = eng
    rng = np.random.default_rng(4)
    n, nq, k = 150, 8, 6
    pts, q = rng.random((n, 6), dtype=np.float32), rng.random((nq, 6), dtype=np.float32)
    a, b2 = attribute(n, 9, groups=10), rng.integers(0, 4, n)
    lo, hi = rng.integers(0, 10, nq), rng.integers(0, 12, nq)
    lo[0], hi[0], lo[1], hi[1], lo[2], hi[2] = TOP, FULL, 5, 2, 0, FULL
    conds = [{"a": (int(x), int(y))} for x, y in zip(lo, hi)]
    rad = np.full(nq, 0.35, np.float32)

    def eq_range(x, y):
        assert np.array_equal(x.lims, y.lims) and np.array_equal(x.pid, y.pid) and np.array_equal(x.rung, y.rung)
        assert np.array_equal(pc.bits(x.distance), pc.bits(y.distance)) and np.array_equal(x.counters, y.counters)

    h, s = ida.Hnsw.from_ordered_points(pts, ida.Builder().ef_search(10)), ida.Search()
    ph, ids = ida.PartitionedHnsw.build(pts, ida.Builder().ef_search(10).seed(3), parts=3)
    for ix, kw in ((h, {"search": s}), (ph, {})):
        order = np.arange(n) if ix is h else np.argsort(ids)               # (PartitionedHnsw.build hands out its own global ids)
        attr, table = ix.attributes(a[order]), ix.attribute_table({"a": a[order], "b": b2[order]})
        want = ix.search_where(q, attr, lo, hi, k, counters=True, **kw)
        same(ix.search_match(q, table, conds, k, counters=True, **kw), want, "match against where")
        assert np.array_equal(ix.search_match(q, table, conds, k, **kw).rung, want.rung) and int(want.count.sum()) > 0
        same(ix.search_where(q, table, lo, hi, k, counters=True, **kw), want, "the interval call reads column 0 of a table")
        want = ix.search_range_where(q, rad, attr, lo, hi, counters=True, **kw)
        eq_range(ix.search_range_match(q, rad, table, conds, counters=True, **kw), want)
        eq_range(ix.search_range_where(q, rad, table, lo, hi, counters=True, **kw), want)
        assert int(want.lims[-1]) > 0
        # one condition for the batch
        same(ix.search_match(q, table, {"a": (2, 6)}, k, counters=True, **kw), ix.search_where(q, attr, 2, 6, k, counters=True, **kw), "one")
        eq_range(ix.search_range_match(q, 0.35, table, {"a": 3}, counters=True, **kw), ix.search_range_where(q, 0.35, attr, 3, None, counters=True, **kw))


# ---- 4. trivial cases and errors ------------------------------------------------------------------------------------------------------------
def test_nothing_to_find(eng):
    ida, kind = eng
    rng = np.random.default_rng(3)
    q = rng.random((4, 5), dtype=np.float32)
    h0 = ida.Hnsw.from_ordered_points(np.zeros((0, 5), np.float32), ida.Builder())
    t0 = h0.attribute_table({"a": np.zeros(0, np.uint32), "b": []})              # n == 0 is legal
    r = h0.search_match(q, t0, {"a": 1, "b": 2}, 3, ida.Search(), counters=True)
    assert len(t0) == 0 and t0.n_cols == 2 and np.all(r.count == 0) and np.all(r.rung == NONE) and np.all(r.pid == 0xFFFFFFFF)
    assert np.all(r.counters == 0)
    rr = h0.search_range_match(q, 1.0, t0, {}, ida.Search(), counters=True)
    assert np.all(rr.lims == 0) and np.all(rr.rung == NONE) and rr.pid.shape == (0,)
    ph0, _ = ida.PartitionedHnsw.build(np.zeros((0, 5), np.float32), ida.Builder(), parts=2)
    pt0 = ph0.attribute_table(np.zeros((0, 3), np.uint32))
    assert pt0.names == ["0", "1", "2"]
    r = ph0.search_match(q, pt0, [{"2": i} for i in range(4)], 3, counters=True)
    assert r.rung.shape == (4, 2) and np.all(r.rung == NONE) and np.all(r.count == 0)
    rr = ph0.search_range_match(q, 1.0, pt0, {"0": (0, 9)}, counters=True)
    assert np.all(rr.lims == 0) and rr.rung.shape == (4, 2) and np.all(rr.rung == NONE)
    # no queries
    pts = rng.random((40, 5), dtype=np.float32)
    h = ida.Hnsw.from_ordered_points(pts, ida.Builder().ef_search(10))
    t = h.attribute_table(np.stack([np.arange(40), np.arange(40) % 3], axis=1))
    e = h.search_match(np.zeros((0, 5), np.float32), t, {"0": 1}, 3, ida.Search(), counters=True)
    assert e.pid.shape == (0, 3) and e.rung.shape == (0,) and e.counters.shape == (0, 3)
    e = h.search_range_match(np.zeros((0, 5), np.float32), 1.0, t, [], ida.Search())
    assert np.array_equal(e.lims, np.zeros(1, np.uint64))
    # fewer points than parts: two of the five parts are empty
    ph, ids = ida.PartitionedHnsw.build(pts[:3], ida.Builder().seed(1), parts=5)
    pt = ph.attribute_table({"x": [4, 9, 4], "y": [1, 1, 2]})
    r = ph.search_match(q, pt, {"x": 4}, 2, counters=True)
    assert np.all(r.count == 2) and np.all(np.sort(r.pid, axis=1) == np.array([0, 2], np.uint32)) and r.rung.shape == (4, 5)
    r = ph.search_match(q, pt, {"x": 4, "y": 2}, 2)
    assert np.all(r.count == 1) and np.all(r.pid[:, 0] == 2)
    rr = ph.search_range_match(q, np.inf, pt, ida.AnyOf({"x": 9}, {"y": (5, 9)}))
    assert np.array_equal(rr.lims, np.arange(5, dtype=np.uint64)) and np.all(rr.pid == 1)


def test_argument_errors(eng):
    ida, kind = eng
    from instant_distance_amd import _capi

    rng = np.random.default_rng(1)
    pts = rng.random((50, 4), dtype=np.float32)
    mk = lambda rows, ef=10: ida.Hnsw.from_ordered_points(np.ascontiguousarray(rows), ida.Builder().ef_search(ef))   # noqa: E731
    h0, h1, other = mk(pts[:21]), mk(pts[21:]), mk(pts[:21])
    ph, ph2 = ida.PartitionedHnsw.from_hnsws([h0, h1]), ida.PartitionedHnsw.from_hnsws([h0, h1])
    two = lambda n: np.stack([np.arange(n), np.arange(n) % 5], axis=1)        # noqa: E731
    t0, t_other = h0.attribute_table(two(21)), other.attribute_table(two(21))
    pt, pt2 = ph.attribute_table(two(50)), ph2.attribute_table(two(50))
    s = ida.Search()
    q = pts[:3]
    L = _capi.lib()
    nq, k = 3, 5
    # query 0: col0 in [0, 40]; query 1: col0 in [5, 9] AND col1 == 2, OR col1 == 4; query 2: col0 in [30, 49]
    clauses = np.array([[0, 0, 40], [0, 5, 9], [1, 2, 2], [1, 4, 4], [0, 30, 49]], np.uint32)
    and_lims, or_lims = np.array([0, 1, 3, 4, 5], np.uint32), np.array([0, 1, 3, 4], np.uint32)
    rad = np.full(3, np.inf, np.float32)
    pid, dist, cnt = np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.float32), np.zeros(nq, np.uint32)
    lims = np.zeros(nq + 1, np.uint64)
    ctx = s._bind(h0)
    u, f = _capi.u32p, _capi.f32p
    keep = []

    def cs(n_cond=3, cl=clauses, al=and_lims, ol=or_lims, null=False):
        if null:
            return None
        keep.append((cl, al, ol))
        return C.byref(_capi.AttrConds(None if cl is None else u(cl), None if al is None else u(al), None if ol is None else u(ol), n_cond))

    def topk(attr=t0, queries=q, out=pid, kk=k, max_rungs=-1, **kw):
        return L.idist_search_batch_match(h0._h, ctx, None if attr is None else attr._h, None if queries is None else f(queries), nq, cs(**kw), kk,
                                          max_rungs, None if out is None else u(out), f(dist), u(cnt), None, None)

    def rng_(attr=t0, radius=rad, out=lims, max_rungs=-1, **kw):
        return L.idist_search_batch_range_match(h0._h, ctx, None if attr is None else attr._h, f(q), nq, f(radius), 3, cs(**kw), max_rungs, 1 << 40,
                                                None if out is None else _capi.u64p(out), None, None)

    def ptopk(attr=pt, queries=q, kk=k, max_rungs=-1, **kw):
        return L.idist_partitioned_search_batch_match(ph._h, None if attr is None else attr._h, None if queries is None else f(queries), nq, cs(**kw),
                                                      kk, max_rungs, u(pid), f(dist), u(cnt), None, None)

    def prng(attr=pt, radius=rad, max_rungs=-1, **kw):
        return L.idist_partitioned_search_batch_range_match(ph._h, None if attr is None else attr._h, f(q), nq, f(radius), 3, cs(**kw), max_rungs,
                                                            1 << 40, _capi.u64p(lims), None, None)

    calls = (topk, rng_, ptopk, prng)
    assert topk() == 0 and cnt.tolist() == [5, 5, 0] and rng_() == 0 and lims.tolist() == [0, 21, 26, 26]    # out_rung / out_counters may be NULL
    assert ptopk() == 0 and cnt.tolist() == [5, 5, 5] and prng() == 0 and lims.tolist() == [0, 41, 52, 72]
    # a foreign table; an index's table in a partitioned call and the reverse; none at all
    assert topk(attr=t_other) == 1 and rng_(attr=t_other) == 1 and ptopk(attr=pt2) == 1 and prng(attr=pt2) == 1
    assert topk(attr=pt) == 1 and rng_(attr=pt) == 1 and ptopk(attr=t0) == 1 and prng(attr=t0) == 1
    assert all(call(attr=None) == 1 for call in calls)
    # n_cond is 1 or nq
    for n_cond in (0, 2, 4):
        assert all(call(n_cond=n_cond) == 1 for call in calls)
        assert b"n_cond" in L.idist_last_error()
    assert topk(n_cond=1) == 0 and cnt.tolist() == [5, 5, 5]
    # null conds / lims; the first limit; a limit that decreases names the entry
    assert all(call(null=True) == 1 for call in calls) and all(call(al=None) == 1 for call in calls) and all(call(ol=None) == 1 for call in calls)
    assert all(call(cl=None) == 1 for call in calls)
    for call in calls:
        assert call(al=np.array([1, 1, 3, 4, 5], np.uint32)) == 1 and b"and_lims[0]" in L.idist_last_error()
        assert call(ol=np.array([1, 1, 3, 4], np.uint32)) == 1 and b"or_lims[0]" in L.idist_last_error()
        assert call(al=np.array([0, 3, 2, 4, 5], np.uint32)) == 1 and b"and_lims[2]" in L.idist_last_error()
        assert call(ol=np.array([0, 3, 2, 4], np.uint32)) == 1 and b"or_lims[2]" in L.idist_last_error()
        # a clause that names no column of the table: the condition and the clause
        bad = clauses.copy()
        bad[3, 0] = 2
        assert call(cl=bad) == 1 and b"condition 1, clause 3" in L.idist_last_error()
    # a program without clauses needs no clause array: TRUE, FALSE, TRUE
    assert topk(cl=None, al=np.array([0, 0, 0], np.uint32), ol=np.array([0, 1, 1, 2], np.uint32)) == 0 and cnt.tolist() == [5, 0, 5]
    # a NaN radius names the query
    bad = rad.copy()
    bad[2] = np.nan
    assert rng_(radius=bad) == 1 and b"query 2" in L.idist_last_error()
    assert prng(radius=bad) == 1 and b"query 2" in L.idist_last_error()
    # the arguments of the calls they equal
    assert topk(queries=None) == 1 and topk(out=None) == 1 and rng_(out=None) == 1 and ptopk(queries=None) == 1
    assert topk(kk=0) == 1 and topk(kk=11) == 1 and topk(max_rungs=-2) == 1 and ptopk(kk=0) == 1 and ptopk(kk=11) == 1 and ptopk(max_rungs=-2) == 1
    assert rng_(max_rungs=-2) == 1 and prng(max_rungs=-2) == 1
    # the table: 1 to 64 columns
    out = C.c_void_p()
    vals = np.zeros(65 * 50, np.uint32)
    for n_cols in (0, 65):
        assert L.idist_attr_new_columns(h0._h, u(vals), n_cols, C.byref(out)) == 1 and b"n_cols" in L.idist_last_error()
        assert L.idist_partitioned_attr_new_columns(ph._h, u(vals), n_cols, C.byref(out)) == 1 and b"n_cols" in L.idist_last_error()
    assert L.idist_attr_new_columns(h0._h, u(vals), 64, C.byref(out)) == 0
    L.idist_attr_free(out)
    assert L.idist_attr_new_columns(None, u(vals), 2, C.byref(out)) == 1 and L.idist_attr_new_columns(h0._h, None, 2, C.byref(out)) == 1
    assert L.idist_attr_new_columns(h0._h, u(vals), 2, None) == 1 and L.idist_partitioned_attr_new_columns(ph._h, None, 2, C.byref(out)) == 1
    # the Python layer raises for the same things
    with pytest.raises(ida.IdistError) as e:
        h0.search_match(q, t_other, {"0": 1}, k, s)
    assert e.value.status == 1
    with pytest.raises(ida.IdistError):
        ph.search_match(q, t0, {"0": 1}, k)
    with pytest.raises(ida.IdistError):
        h0.search_range_match(q, 1.0, pt, {"0": 1}, s)
    with pytest.raises(ida.IdistError):
        h0.attribute_table(np.zeros((21, 65), np.uint32))
    with pytest.raises(ida.IdistError):
        h0.attribute_table({})


# ---- 5. Python ------------------------------------------------------------------------------------------------------------------------------
def test_encoder():
    """the conditions of the Python layer as the ABI's flat program: a pure function, no engine"""
    import instant_distance_amd as ida
    from instant_distance_amd.api import MAX_CONJUNCTIONS, encode_conds

    names = ["t", "d", "c"]
    enc = lambda conds, nq=1: tuple(x.tolist() if isinstance(x, np.ndarray) else x for x in encode_conds(conds, names, nq))   # noqa: E731
    # equality, an interval (lo > hi stays: the empty clause), the columns by name
    assert enc({"d": 7, "t": (100, 200)}) == ([[1, 7, 7], [0, 100, 200]], [0, 2], [0, 1], 1)
    assert enc({"c": (9, 3)}) == ([[2, 9, 3]], [0, 1], [0, 1], 1)
    # membership: sorted, duplicates dropped, runs of consecutive values merged
    assert enc({"c": {3, 4, 5, 9}}) == ([[2, 3, 5], [2, 9, 9]], [0, 1, 2], [0, 2], 1)
    assert enc({"c": [9, 5, 3, 4, 4, 9]}) == enc({"c": {3, 4, 5, 9}}) == enc({"c": np.array([5, 9, 3, 4], np.int64)})
    assert enc({"c": [0xFFFFFFFF, 0, 0xFFFFFFFE]}) == ([[2, 0, 0], [2, 0xFFFFFFFE, 0xFFFFFFFF]], [0, 1, 2], [0, 2], 1)
    # TRUE, FALSE, an empty membership list
    assert enc({}) == ([], [0, 0], [0, 1], 1) and enc(ida.AnyOf()) == ([], [0], [0, 0], 1) and enc({"t": [], "d": 1}) == ([], [0], [0, 0], 1)
    assert enc(ida.AnyOf({}, {"t": 1})) == ([[0, 1, 1]], [0, 0, 1], [0, 2], 1)
    # several memberships: the Cartesian product, the dict's order of the columns
    assert enc({"t": [1, 5], "d": 2, "c": [7, 8, 20]}) == (
        [[0, 1, 1], [1, 2, 2], [2, 7, 8], [0, 1, 1], [1, 2, 2], [2, 20, 20], [0, 5, 5], [1, 2, 2], [2, 7, 8], [0, 5, 5], [1, 2, 2], [2, 20, 20]],
        [0, 3, 6, 9, 12], [0, 4], 1)
    # one per query; AnyOf
    assert enc([{"t": 1}, ida.AnyOf({"t": 2}, {"d": (3, 4), "c": 5}), {}], 3) == (
        [[0, 1, 1], [0, 2, 2], [1, 3, 4], [2, 5, 5]], [0, 1, 2, 4, 4], [0, 1, 3, 4], 3)
    assert enc([], 0) == ([], [0], [0], 0)
    # the cap: 64 * 64 conjunctions pass, one more does not
    even = list(range(0, 128, 2))
    assert len(encode_conds({"t": even, "d": even}, names, 1)[1]) == MAX_CONJUNCTIONS + 1 == 4097
    with pytest.raises(ValueError):
        encode_conds(ida.AnyOf({"t": even, "d": even}, {"c": 1}), names, 1)
    with pytest.raises(ValueError):
        encode_conds({"t": even, "d": even, "c": [1, 3]}, names, 1)
    # errors
    with pytest.raises(KeyError):
        encode_conds({"x": 1}, names, 1)
    for bad in (1.5, "7", None, (1.0, 2), True, [1.5], np.array([0.5])):
        with pytest.raises(TypeError):
            encode_conds({"t": bad}, names, 1)
    for bad in (-1, 1 << 32, (0, 1 << 32), (-1, 2), [1, -1], [1 << 32], (1, 2, 3), np.zeros((2, 2), np.int64)):
        with pytest.raises(ValueError):
            encode_conds({"t": bad}, names, 1)
    with pytest.raises(ValueError):
        encode_conds([{"t": 1}, {"t": 2}], names, 3)                            # one per query
    with pytest.raises(TypeError):
        encode_conds(7, names, 1)
    with pytest.raises(TypeError):
        encode_conds([{"t": 1}, 7], names, 2)
    with pytest.raises(TypeError):
        ida.AnyOf({"t": 1}, [("t", 1)])


def test_python_layer(eng):
    ida, kind = eng
    rng = np.random.default_rng(2)
    pts = rng.random((120, 5), dtype=np.float32)
    h, s = ida.Hnsw.from_ordered_points(pts, ida.Builder().ef_search(12)), ida.Search()
    tenant, day = rng.integers(0, 4, 120), rng.integers(100, 130, 120)
    table = h.attribute_table({"tenant": tenant, "day": day})
    assert isinstance(table, ida.AttrTable) and isinstance(table, ida.Attr) and len(table) == 120 and table.names == ["tenant", "day"]
    assert table.columns["day"].dtype == np.uint32 and np.array_equal(table.columns["day"], day) and np.array_equal(table.values, tenant)
    arr = h.attribute_table(np.stack([tenant, day], axis=1))
    assert arr.names == ["0", "1"] and arr.n_cols == 2 and np.array_equal(arr.columns["1"], day)
    q = rng.random((4, 5), dtype=np.float32)
    k = 6
    # one condition against nq conditions
    cond = {"tenant": 2, "day": (105, 120)}
    m = (tenant == 2) & (day >= 105) & (day <= 120)
    same(h.search_match(q, table, cond, k, s), h.search_allowed(q, m, k, s), "one condition")
    same(h.search_match(q, table, [cond] * 4, k, s), h.search_allowed(q, m, k, s), "the same condition per query")
    same(h.search_match(q, arr, {"0": 2, "1": (105, 120)}, k, s), h.search_allowed(q, m, k, s), "columns named by position")
    conds = [{"tenant": i, "day": [101, 102, 103, 110, 129]} for i in range(3)] + [ida.AnyOf({"tenant": 3}, {"day": (100, 104)})]
    sets = [(tenant == i) & np.isin(day, [101, 102, 103, 110, 129]) for i in range(3)] + [(tenant == 3) | (day <= 104)]
    same(h.search_match(q, table, conds, k, s, counters=True), h.search_allowed_sets(q, sets, None, k, s, counters=True), "per query")
    same(h.search_match(q, table, tuple(conds), k, s), h.search_allowed_sets(q, sets, None, k, s), "a tuple of conditions")
    a = h.search_range_match(q, 0.5, table, conds, s, counters=True)
    o = h.search_range_allowed_sets(q, 0.5, sets, None, s, counters=True)
    assert np.array_equal(a.lims, o.lims) and np.array_equal(a.pid, o.pid) and np.array_equal(a.rung, o.rung) and int(a.lims[-1]) > 0
    assert np.array_equal(pc.bits(a.distance), pc.bits(o.distance)) and np.array_equal(a.counters, o.counters)
    assert isinstance(h.search_match(q, table, {}), ida.AllowedResult)       # k and search have defaults
    # errors
    with pytest.raises(KeyError):
        h.search_match(q, table, {"month": 1}, k, s)
    with pytest.raises(KeyError):
        h.search_range_match(q, 0.5, arr, {"tenant": 1}, s)
    with pytest.raises(TypeError):
        h.search_match(q, table, {"tenant": 1.5}, k, s)
    with pytest.raises(TypeError):
        h.search_match(q, h.attributes(tenant), {"tenant": 1}, k, s)            # an Attr is no table
    with pytest.raises(TypeError):
        h.search_match(q[:, :3], table, {}, k, s)
    with pytest.raises(ValueError):
        h.search_match(q, table, {"tenant": -1}, k, s)
    with pytest.raises(ValueError):
        h.search_range_match(q, 0.5, table, {"day": (0, 1 << 32)}, s)
    with pytest.raises(ValueError):
        h.search_match(q, table, conds[:3], k, s)                               # one per query
    with pytest.raises(ValueError):
        h.attribute_table({"tenant": tenant, "day": np.full(120, -1)})
    with pytest.raises(ValueError):
        h.attribute_table({"tenant": tenant, "day": day[:119]})
    with pytest.raises(ValueError):
        h.attribute_table(np.zeros((119, 2), np.uint32))
    with pytest.raises(ValueError):
        h.attribute_table(np.zeros(120, np.uint32))
    with pytest.raises(TypeError):
        h.attribute_table({"tenant": tenant, "day": day.astype(np.float32)})
    with pytest.raises(TypeError):
        h.attribute_table({0: tenant})
    # HnswMap: the items carry their values and satisfy the condition
    values = [f"v{i}" for i in range(120)]
    mp = ida.Builder().seed(7).ef_search(12).build(pts, values)
    ten = np.array([int(x[1:]) % 7 for x in mp.values])                         # PointId order, as mp.values
    par = np.array([int(x[1:]) % 2 for x in mp.values])
    mt = mp.attribute_table({"ten": ten, "par": par})
    cond = ida.AnyOf({"ten": [2, 3], "par": 0}, {"ten": 6, "par": 1})
    ok = lambda it: (int(it.value[1:]) % 7 in (2, 3) and int(it.value[1:]) % 2 == 0) or (int(it.value[1:]) % 7 == 6 and int(it.value[1:]) % 2 == 1)   # noqa: E731
    items = mp.search_match(q, mt, cond, k, ida.Search())
    r = mp.hnsw.search_match(q, mt, cond, k, ida.Search())
    assert len(items) == 4
    for i, row in enumerate(items):
        assert [it.pid for it in row] == r.pid[i, : r.count[i]].tolist() and len(row) == k
        assert all(ok(it) and it.value == mp.values[it.pid] and np.array_equal(it.point, mp.hnsw[it.pid]) for it in row)
    ritems = mp.search_range_match(q, 0.4, mt, cond, ida.Search())
    rr = mp.hnsw.search_range_match(q, 0.4, mt, cond, ida.Search())
    assert [[it.pid for it in row] for row in ritems] == [rr.pid[int(rr.lims[i]): int(rr.lims[i + 1])].tolist() for i in range(4)]
    assert sum(len(row) for row in ritems) > 0 and all(ok(it) for row in ritems for it in row)
    # PartitionedHnsw: global ids, the columns in the order of its rows
    ph, ids = ida.PartitionedHnsw.build(pts, ida.Builder().ef_search(12).seed(5), parts=3)
    rows = np.stack([ph[i] for i in range(120)])
    t2 = (rows[:, 0] * 4).astype(np.int64)
    d2 = (rows[:, 1] * 30).astype(np.int64) + 100
    ptab = ph.attribute_table({"tenant": t2, "day": d2})
    pconds = [{"tenant": i % 4, "day": (100 + i, 125)} for i in range(4)]
    psets = [(t2 == i % 4) & (d2 >= 100 + i) & (d2 <= 125) for i in range(4)]
    same(ph.search_match(q, ptab, pconds, k, counters=True), ph.search_allowed_sets(q, psets, None, k, counters=True), "partitioned, per query")
    same(ph.search_match(q, ptab, pconds[1], k), ph.search_allowed(q, psets[1], k), "partitioned, one condition")
    a, o = ph.search_range_match(q, 0.6, ptab, pconds), ph.search_range_allowed_sets(q, 0.6, psets, None)
    assert np.array_equal(a.lims, o.lims) and np.array_equal(a.pid, o.pid) and np.array_equal(a.rung, o.rung) and int(a.lims[-1]) > 0
    with pytest.raises(KeyError):
        ph.search_match(q, ptab, {"x": 1}, k)
    with pytest.raises(ValueError):
        ph.search_range_match(q, 0.6, ptab, pconds[:2])
