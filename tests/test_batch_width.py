"""Batch-position independence past the grid caps of the kernels around the walks ("Grid caps").

Row q of a call depends on query q and its own arguments only — whatever the width of the batch and whichever walk the launch policy
picks for that width: every walk is bit-identical to the oracle by contract.  So each test takes the SMALL case its feature's module
holds against the oracle or the definition (m queries; the emulator-sized case on both engines), computes the expected rows once,
the way that module does, runs the same call with the queries and every per-query argument tiled to nq rows, and requires row t ==
expected row of the query it repeats, bit for bit: ids, distance bits, counts, rungs, the three work counters, and for the range forms
lims == the u64 cumulative sum of the tiled counts and the flat arrays.

nq on the GPU comes from the device's CU count at run time, strictly above the cap of the step under test and 37 beyond it (no
multiple of 64 or 256); under the emulator (one CU: the CU-derived caps are 8 to 64) nq = m + 37, or cap + 37 where m is below the
cap.  Every test asserts from the returned rungs that more rows than the cap took the step it is named for.

Shapes on a 256-CU device (the indexes: 600 x 12-d, ef_search 8, k 5; the metric cases 300 x 7-d; the parts: 660 x 8-d):
  rung tests     nq = 65,573 (above n_cu * 16 AND above the selects' fixed 65,536; the restricted range form 524,325, above
                 n_cu * 8 x 256), max_rungs <= 3: rung rows np x ef x 8 B <= 134 MB
  exact tests    nq = 16,421 (n_cu * 64 + 37); range results up to 600 per row: 16,421 x 600 x 8 B = 79 MB of keys at the peak
  match          8,229 distinct conditions (n_cu * 32 + 37): 8,229 bitmaps of 19 words
  metrics        nq = 262,181, k = 8 (nq x k above n_cu * 8 x 256 x 4 reported distances), rung 0 or exact: 17 MB of rung rows
  partitioned    top-k nq = 16,421 (merge_topk_kernel: 16,384) and 131,109 with a bitmap per row (11 MB); range nq = 524,325
                 (range_merge_counts_kernel: n_cu * 8 x 256), rung 0 only: 34 MB per part, about 2.3M merged results
The peak of the module is below 0.2 GB of device memory."""
import atexit

import numpy as np
import pytest

import parity_cases as pc
from engines import cu_count, engine_params
from test_allowed import EXACT, NONE, allowed_sets
from test_allowed import check as check_allowed
from test_allowed import main_case as allowed_case
from test_allowed_sets import rows_of, start_rung
from test_attr_match import mask_of, table_of
from test_grouped import check as check_grouped
from test_grouped import expected as grouped_expected
from test_grouped import layout, restriction, selections
from test_partitioned_allowed import check as check_parts
from test_partitioned_allowed import expected as parts_expected
from test_partitioned_allowed import global_masks, main_parts
from test_partitioned_allowed import partitioned as partitioned_allowed
from test_partitioned_range import check as check_range_parts
from test_partitioned_range import expected as range_parts_expected
from test_partitioned_range import partitioned as partitioned_range
from test_partitioned_range import range_parts
from test_range import RCase, radii_of
from test_range import check as check_range
from test_range import main_case as range_case
from test_range_allowed import cycle, main_sets
from test_range_allowed import main_case as range_allowed_case
from test_range_allowed import model as range_allowed_model

SMALL = "emu"        # the emulator-sized case of every module, on both engines


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


def width(kind, m, cap):
    """nq: 37 above `cap` rows on the GPU; m + 37 under the emulator, or 37 above the cap where m does not reach it"""
    nq = (cap if kind == "gpu" else max(m, cap)) + 37
    assert nq % 64 and nq % 256
    return nq


def tiled(rows, nq, grid):
    """the query each of the nq rows repeats: `rows` over and over — never with a period that divides the grid, so that the rows a
    workgroup takes one after the other are different queries"""
    rows = np.asarray(rows)
    if len(rows) > 1 and grid % len(rows) == 0:
        rows = rows[:-1]
    return rows[np.arange(nq) % len(rows)]


def tile_range(want, idx):
    """(lims, pid, distance bits, rung, counters) of the call whose row t is row idx[t] of `want`"""
    lims, pid, bits, rung, ctr = want[:5]
    lo, c = lims[:-1].astype(np.int64)[idx], np.diff(lims.astype(np.int64))[idx]
    t_lims = np.concatenate([[0], np.cumsum(c)]).astype(np.uint64)
    src = np.repeat(lo - t_lims[:-1].astype(np.int64), c) + np.arange(int(c.sum()))
    return t_lims, pid[src], bits[src], rung[idx], ctr[idx]


def hist(x):
    return dict(zip(*[v.tolist() for v in np.unique(x, return_counts=True)]))


def on_rung(rung):
    return rung < NONE


def caps(kind):
    """(rung, exact): the rows a rung test / an exact-step test must exceed"""
    cus = cu_count(kind)
    # rung: n_cu * 16 (the segments rule of the exact step, exact_segments) and the fixed min(np, 65536) of allowed_select_kernel,
    # range_select_kernel, range_copy_kernel and grouped_select_kernel's launches; exact: n_cu * 64, the grids of allowed_scan_bits_kernel,
    # range_scan_kernel, range_gather_kernel and grouped_exclude_kernel (idist_capi.hip)
    return max(cus * 16, 65536 if kind == "gpu" else 0), cus * 64


# ---- Hnsw.search_allowed_sets ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", ["rung", "exact"])
def test_allowed_sets(eng, oracle, step):
    """rung: four sets large enough to START on rung 0 (a launch's select sees only the pending rows whose set's first rung has come
    up), so the first select launch holds all nq rows; some rows close there, the others on rung 1 or 2"""
    ida, kind = eng
    c, k = allowed_case(oracle, SMALL)
    n, m = len(c.pts), len(c.q)
    if step == "rung":
        rng, x0 = np.random.default_rng(70), c.pts[:, 0]
        masks = [np.ones(n, bool), rng.random(n) < 0.7, x0 > np.quantile(x0, 0.3), rng.random(n) < 0.66]
        assert all(start_rung(c, mk, k, 3) == 0 for mk in masks)
    else:
        masks = list(allowed_sets(c, k).values())
    max_rungs = 3 if step == "rung" else 0
    set_of = np.arange(m) % len(masks)
    want = rows_of([c.model(mk, k, max_rungs) for mk in masks], set_of)
    rows = np.flatnonzero(on_rung(want[3]) if step == "rung" else want[3] == EXACT)
    cap = caps(kind)[step == "exact"]
    nq = width(kind, m, cap)
    idx = tiled(rows, nq, cap)
    assert len(set(want[3][rows].tolist())) >= (2 if step == "rung" else 1) and len(set(set_of[rows].tolist())) >= 2
    got = c.hnsw(ida).search_allowed_sets(c.q[idx], np.stack(masks), set_of[idx], k, ida.Search(), max_rungs=max_rungs, counters=True)
    print(step, "nq", nq, "rungs", hist(got.rung))
    assert int(np.sum(on_rung(got.rung) if step == "rung" else got.rung == EXACT)) == nq > cap
    check_allowed(got, tuple(x[idx] for x in want), step)


# ---- Hnsw.search_match: more distinct conditions than allowed_count_kernel's grid --------------------------------------------------------
def test_match_distinct_conditions(eng, oracle):
    """condition j = (base condition j % 10 on column "a") AND ("b" <= 2^31 + j): every j a condition of its own — one bitmap, one
    count, one start rung each — whose set is that of base j % 10.  A workgroup counts set j, then set j + grid: another base (the
    grids, n_cu * 32, are no multiples of 10)."""
    # cap: min(n_sets, n_cu * 32) workgroups of one set each, allowed_count_kernel's launch in allowed_sets_device (idist_capi.hip)
    ida, kind = eng
    c, k = allowed_case(oracle, SMALL)
    n, m = len(c.pts), len(c.q)
    cols = table_of(n, 5)
    base = [(0, 49), (10, 14), 7, (0, 99), (1 << 31) + 5, (50, 99), (20, 60), (100, 200), (0, 4), (30, 31)]
    masks = [mask_of({"a": b}, cols) for b in base]
    assert [int(mk.sum()) for mk in masks][7] == 0 and int(masks[4].sum()) == 1
    cap = cu_count(kind) * 32
    assert cap % 10
    nq = width(kind, m, cap)
    t = np.arange(nq)
    want = rows_of([c.model(mk, k) for mk in masks], np.arange(m) % 10)           # row i: query i under base i % 10 (m % 10 == 0)
    assert m % 10 == 0
    conds = [{"a": base[j % 10], "b": (0, (1 << 31) + j)} for j in range(nq)]
    h = c.hnsw(ida)
    got = h.search_match(c.q[t % m], h.attribute_table(cols), conds, k, ida.Search(), counters=True)
    print("nq", nq, "rungs", hist(got.rung))
    assert len({r for r in got.rung.tolist() if r < NONE}) >= 2 and EXACT in got.rung and NONE in got.rung
    check_allowed(got, tuple(x[t % m] for x in want), "distinct conditions")


def test_range_match_distinct_conditions(eng, oracle):
    """the same conditions through search_range_match: range_allowed_count_kernel counts set j, then set j + grid"""
    # cap: min(n_sets, n_cu * 32) workgroups of one set each, range_allowed_count_kernel's launch in range_search_device (idist_capi.hip)
    ida, kind = eng
    rc = range_allowed_case(oracle, SMALL)
    n, m = len(rc.raw), len(rc.q)
    cols = table_of(n, 6)
    base = [(0, 49), (10, 14), 7, (0, 99), (1 << 31) + 5, (50, 99), (20, 60), (100, 200), (0, 4), (30, 31)]
    masks = [mask_of({"a": b}, cols) for b in base]
    cap = cu_count(kind) * 32
    assert cap % 10 and m % 10 == 0
    nq = width(kind, m, cap)
    t = np.arange(nq)
    rad = radii_of(rc)
    want = range_allowed_model(rc, rad, masks, np.arange(m) % 10, max_rungs=2)[:5]
    conds = [{"a": base[j % 10], "b": (0, (1 << 31) + j)} for j in range(nq)]
    h = rc.hnsw(ida)
    got = h.search_range_match(rc.q[t % m], rad[t % m], h.attribute_table(cols), conds, ida.Search(), max_rungs=2, counters=True)
    print("nq", nq, "rungs", hist(got.rung), "total", int(got.lims[-1]))
    assert np.any(on_rung(got.rung)) and EXACT in got.rung and NONE in got.rung and int(got.lims[-1]) > 0
    check_range(got, tile_range(want, t % m), "distinct conditions")


# ---- Hnsw.search_range -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2sq", "cosine", "dot"])
@pytest.mark.parametrize("step", ["rung", "exact"])
def test_range(eng, oracle, step, metric):
    """exact: every row a list of its own length (radius kinds from "below", nothing, to "inf", every point) for the sort and the
    gather, and rows x segments above the 4,096 items of one trip of the prefix sum's second level.  Cosine and DOT: their prepare
    and report passes are lane-per-item kernels with caps of their own (launch_normalize, launch_dot_norms: n_cu * 32 waves of
    eight rows; scale_half_kernel, dot_report_kernel: n_cu * 8 workgroups)"""
    ida, kind = eng
    rc = range_case(oracle, SMALL) if metric == "l2sq" else metric_case(oracle, metric)
    m = len(rc.q)
    rad = radii_of(rc)
    max_rungs = 2 if step == "rung" else 0
    want = rc.model(rad, max_rungs=max_rungs)
    rows = np.flatnonzero(on_rung(want[3]) if step == "rung" else want[3] == EXACT)
    cap = caps(kind)[step == "exact"]
    nq = width(kind, m, cap)
    assert nq > 4096 or kind == "emu"
    idx = tiled(rows, nq, cap)
    assert len(set(np.diff(want[0].astype(np.int64))[rows].tolist())) >= 4                 # lists of different lengths
    got = rc.hnsw(ida).search_range(rc.q[idx], rad[idx], ida.Search(), max_rungs=max_rungs, counters=True, max_total=1 << 32)
    print(step, metric, "nq", nq, "rungs", hist(got.rung), "total", int(got.lims[-1]))
    assert int(np.sum(on_rung(got.rung) if step == "rung" else got.rung == EXACT)) == nq > cap
    check_range(got, tile_range(want, idx), f"{step}, {metric}")


_METRIC_CASES = {}
atexit.register(_METRIC_CASES.clear)      # (the oracle's handles go before the interpreter takes its library apart)


def metric_case(oracle, metric):
    """tests/test_range.py's test_metrics case at the emulator's shape: 300 x 7-d, ef_search 8, 18 queries"""
    if metric not in _METRIC_CASES:
        rng = np.random.default_rng(11)
        raw = rng.random((300, 7), dtype=np.float32) - np.float32(0.3)
        q = rng.random((18, 7), dtype=np.float32) - np.float32(0.3)
        if metric == "dot":
            raw[100] *= np.float32(37.0)
        _METRIC_CASES[metric] = RCase(oracle, raw, q, 8, metric)
    return _METRIC_CASES[metric]


# ---- Hnsw.search_allowed_sets on a cosine and a DOT index ---------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_allowed_sets_metrics(eng, oracle, metric):
    """the rows of the single-set call of each query's set at the module's own width (tests/test_allowed.py pins that call to the
    definition, the metric's report included), tiled past the caps of the passes around the search: the report over the nq x k
    distances (four per lane: k = 8), the prepare pass over the nq queries, allowed_init_kernel over nq x k items, and the exact step.
    Rung 0 or the exact step only (max_rungs = 1), so that the rows stay cheap."""
    # caps: n_cu * 8 workgroups of 256 lanes, four floats a lane, scale_half_kernel / dot_report_kernel (launch_scale_half,
    # launch_dot_report); n_cu * 32 waves of eight rows, normalize_rows_kernel / dot_norms_kernel (launch_normalize, launch_dot_norms);
    # n_cu * 8 workgroups of 256 items, allowed_init_kernel (allowed_sets_device) (idist_capi.hip)
    ida, kind = eng
    rc = metric_case(oracle, metric)
    n, m, k = len(rc.raw), len(rc.q), 8
    rng = np.random.default_rng(9)
    masks = [rng.random(n) < share for share in (1.0, 0.2, 0.05)]
    set_of = np.arange(m) % 3
    h = rc.hnsw(ida)
    ones = [h.search_allowed(rc.q, mk, k, ida.Search(), max_rungs=1, counters=True) for mk in masks]   # rung 0, or the exact step
    want = tuple(np.stack([getattr(ones[s], f)[i] for i, s in enumerate(set_of)]) for f in ("pid", "distance", "count", "rung", "counters"))
    assert EXACT in want[3] and np.any(on_rung(want[3])) and k % 4 == 0
    cus = cu_count(kind)
    report_cap, prepare_cap, exact_cap = cus * 8 * 256 * 4, cus * 32 * 8, cus * 64
    nq = max(report_cap // k, prepare_cap, 2 * exact_cap) + 37
    assert nq % 64 and nq % 256
    idx = tiled(np.arange(m), nq, cus * 8 * 256)
    got = h.search_allowed_sets(rc.q[idx], masks, set_of[idx], k, ida.Search(), max_rungs=1, counters=True)
    print(metric, "nq", nq, "rungs", hist(got.rung))
    assert nq * k > report_cap and nq > prepare_cap and int(np.sum(got.rung == EXACT)) > exact_cap and int(np.sum(got.rung == 0)) > nq // 4
    check_allowed(got, (want[0][idx], pc.bits(want[1])[idx], want[2][idx], want[3][idx], want[4][idx], None), metric)


# ---- Hnsw.search_range_allowed_sets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", ["rung", "exact"])
def test_range_allowed_sets(eng, oracle, step):
    ida, kind = eng
    rc = range_allowed_case(oracle, SMALL)
    m = len(rc.q)
    masks, bits = main_sets(rc)
    rad, set_of = radii_of(rc), cycle(m, 4)
    max_rungs = 2 if step == "rung" else 0
    want = range_allowed_model(rc, rad, masks, set_of, max_rungs=max_rungs)[:5]
    rows = np.flatnonzero(on_rung(want[3]) if step == "rung" else want[3] == EXACT)
    cap = caps(kind)[step == "exact"]
    if step == "rung" and kind == "gpu":
        # ... and n_cu * 8 workgroups of 256 rows, range_allowed_init_kernel (range_search_device, idist_capi.hip).  Every row of a
        # range call is gathered for rung 0 (no start rule), so that rung's select and copy launches hold all nq rows.
        cap = max(cap, cu_count(kind) * 8 * 256)
    nq = width(kind, m, cap)
    idx = tiled(rows, nq, cap)
    assert len(set(set_of[rows].tolist())) >= 4 and len(set(np.diff(want[0].astype(np.int64))[rows].tolist())) >= 3
    got = rc.hnsw(ida).search_range_allowed_sets(rc.q[idx], rad[idx], bits, set_of[idx], ida.Search(), max_rungs=max_rungs, counters=True,
                                                  max_total=1 << 32)
    print(step, "nq", nq, "rungs", hist(got.rung), "total", int(got.lims[-1]))
    assert int(np.sum(on_rung(got.rung) if step == "rung" else got.rung == EXACT)) == nq > cap
    check_range(got, tile_range(want, idx), step)


# ---- Hnsw.search_grouped ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", ["rung", "exact rounds"])
def test_grouped(eng, oracle, step):
    """exact rounds: bands of coordinate 0 as groups under per-query conditions, no rung permitted — the k nearest allowed points
    of a query share few bands, so its exact step takes several rounds, each behind grouped_exclude_kernel"""
    ida, kind = eng
    c, k = allowed_case(oracle, SMALL)
    m = len(c.q)
    lay, mask, max_rungs = ("docs4", "per query", -1) if step == "rung" else ("x0 bands 12", "per query", 0)
    want = grouped_expected(oracle, SMALL, lay, mask, max_rungs, want_rounds=True)
    conds = restriction(c, mask)[0]
    if step == "rung":
        rows = np.flatnonzero(on_rung(want[3]))
    else:
        rows = np.flatnonzero(want[3] == EXACT)
        assert want[6][rows].max() >= 2 and len(set(want[6][rows].tolist())) >= 2               # rounds, and not the same number for all
    cap = caps(kind)[step != "rung"]
    nq = width(kind, m, cap)
    idx = tiled(rows, nq, cap)
    h = c.hnsw(ida)
    table = h.attribute_table({"g": layout(c, lay), "sel": selections(c)})
    got = h.search_grouped(c.q[idx], table, "g", k, [conds[i] for i in idx], ida.Search(), max_rungs=max_rungs, counters=True)
    print(step, "nq", nq, "rungs", hist(got.rung), "counts", hist(got.count))
    assert int(np.sum(on_rung(got.rung) if step == "rung" else got.rung == EXACT)) == nq > cap
    check_grouped(got, tuple(x[idx] for x in want[:6]), step)


# ---- PartitionedHnsw, P = 3 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sets", ["shared", "one per query"])
def test_partitioned_allowed_sets(eng, oracle, sets):
    """one per query: the call is given nq bitmaps (set_of = None), and every part slices all of them — on the GPU more output words
    than the lanes of that launch's grid (under the emulator the form alone, at m + 37 rows)"""
    # caps: min(nq, 16384) workgroups of one query each, merge_topk_kernel's launch_merge; n_cu * 8 workgroups of 256 output words,
    # allowed_slice_kernel's launch in partitioned_stage_sets (idist_capi.hip)
    ida, kind = eng
    from instant_distance_amd.api import allowed_bitmap

    pts, q, b, cs, k = main_parts(oracle, SMALL, 3)
    m = len(q)
    masks = global_masks(pts, b, k)
    set_of = np.arange(m) % len(masks)
    want = parts_expected(cs, b, masks, set_of, k, 2)
    cap = 16384 if kind == "gpu" else 0
    words_min = min((b[p + 1] - b[p] + 31) // 32 for p in range(3))
    if sets == "one per query" and kind == "gpu":
        cap = max(cap, cu_count(kind) * 8 * 256 // words_min)              # n_sets x the words of the smallest part: above the lanes
    nq = width(kind, m, cap)
    idx = tiled(np.arange(m), nq, max(cap, 1))
    ph, hs = partitioned_allowed(ida, cs)
    bits = np.stack([allowed_bitmap(mk, len(pts)) for mk in masks])
    if sets == "shared":
        got = ph.search_allowed_sets(q[idx], bits, set_of[idx], k, max_rungs=2, counters=True)
    else:
        got = ph.search_allowed_sets(q[idx], np.ascontiguousarray(bits[set_of[idx]]), None, k, max_rungs=2, counters=True)
        assert kind == "emu" or nq * words_min > cu_count(kind) * 8 * 256
    print(sets, "nq", nq, "rungs", hist(got.rung))
    assert nq > cap and EXACT in got.rung and np.any(on_rung(got.rung))
    check_parts(got, tuple(x[idx] for x in want), f"P = 3, {sets}")


def test_partitioned_range(eng, oracle):
    """rung 0 alone (max_rungs = 1: what it does not answer is scanned exactly), so that half a million rows stay cheap"""
    # caps: min(ceil(nq / 256), n_cu * 8) workgroups of 256 rows, range_merge_counts_kernel (launch_range_merge_counts); min(tiles,
    # n_cu * 32) waves of 256 merged results, range_merge_kernel (launch_range_merge) (idist_capi.hip)
    ida, kind = eng
    pts, q, b, rcs, w = range_parts(oracle, SMALL, 3)
    m = len(q)
    rad = radii_of(w, ["below", 0, "ef-1", "ef", "ef-1", 2, "neg", 5])
    want, _ = range_parts_expected(rcs, b, rad, 1)
    rows = np.flatnonzero(np.all(on_rung(want[3]), axis=1))                          # answered by rung 0 in every part
    cus = cu_count(kind)
    cap = cus * 8 * 256 if kind == "gpu" else 0
    nq = width(kind, m, cap)
    idx = tiled(rows, nq, max(cap, 1))
    ph, hs = partitioned_range(ida, rcs)
    got = ph.search_range(q[idx], rad[idx], max_rungs=1, counters=True, max_total=1 << 32)
    total = int(got.lims[-1])
    print("nq", nq, "rungs", hist(got.rung), "total", total)
    assert nq > cap and np.all(on_rung(got.rung)) and (kind == "emu" or total > cus * 32 * 256)
    check_range_parts(got, tile_range(want, idx), "P = 3")
