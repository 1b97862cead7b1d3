"""Grouped search (idist_search_batch_grouped, include/idist.h): the nearest allowed point of each of the k
nearest groups, the group of a point being one column of an attribute table.

The answer is DEFINED through what is already exact — `Hnsw::search` at ef_search, 4 ef_search, ... 4096, each list collapsed to the
first allowed entry of every group, and the collapse of ALL allowed points in (distance bits, id) order where the ladder does not
apply or ends — so everything here is compared exactly: ids, groups, counts, rungs and counters with array_equal, distances as bit
patterns.  The expected arrays come from a model in this file (`Case.rung(E)` of test_allowed for the rungs, the oracle's brute force
over the allowed rows at k = |A| for the exact step, a numpy collapse), never from the code under test.  Every case runs on the CPU
emulator and (-m gpu) on the MI355X."""
import atexit
import ctypes as C

import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params
from test_allowed import EXACT, INF_BITS, INVALID, NONE, ladder
from test_allowed import check as check_allowed
from test_allowed import main_case
from test_allowed_sets import same
from test_attr import FILL, FULL, TOP, guarded_u32
from test_attr_match import mask_of
from test_partitioned import DeviceMem
from test_range import check as check_range
from test_range import radii_of
from test_range_allowed import main_case as range_case
from test_range_allowed import model as range_model


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


# ---- the definition, restated --------------------------------------------------------------------------------------------------------
def collapse(lst, allowed, groups, k):
    """positions of the kept entries of the id list `lst`: allowed, and the first allowed entry of its group; at most k"""
    pos = np.flatnonzero(allowed[lst])
    _, first = np.unique(groups[lst[pos]], return_index=True)
    return pos[np.sort(first)][:k]


class Model:
    """The definition over one Case: the rungs from `Case.rung`, the exact step from the oracle's brute force over the allowed rows
    at k = |A| — computed once per allowed set for ALL queries and shared"""

    def __init__(self, c):
        self.c, self._full = c, {}

    def full(self, mask):
        """(ids [nq, |A|], distance bits [nq, |A|]): all of A per query, ordered by (raw canonical distance bits, id)"""
        key = mask.tobytes()
        if key not in self._full:
            ids = np.flatnonzero(mask).astype(np.uint32)
            bp, bd = self.c.oracle.bruteforce(self.c.pts[ids], self.c.q, len(ids), metric=self.c.metric, threads=8)
            self._full[key] = (ids[bp], pc.bits(bd))
        return self._full[key]

    def run(self, masks, set_of, groups, k, max_rungs=-1, want_rounds=False):
        """(pid, distance bits, count, rung, counters, group, rounds): rounds[q] = the rounds of k nearest remaining points the exact
        step of query q needs (0: answered by a rung)"""
        c = self.c
        n, nq = len(c.pts), len(c.q)
        pid, bits = np.full((nq, k), INVALID, np.uint32), np.full((nq, k), INF_BITS, np.uint32)
        group = np.zeros((nq, k), np.uint32)
        count, rung, ctr = np.zeros(nq, np.uint32), np.full(nq, NONE, np.uint32), np.zeros((nq, 3), np.uint32)
        rounds = np.zeros(nq, np.int64)
        E = ladder(c.ef)
        if max_rungs >= 0:
            E = E[:max_rungs]
        for qi in range(nq):
            mask = masks[set_of[qi]]
            a = int(mask.sum())
            if n == 0 or c.ef == 0 or a == 0:
                continue
            r0 = next((r for r, e in enumerate(E) if e * a >= k * n), None) if a > k else None
            done = False
            for r in range(r0 if r0 is not None else len(E), len(E)):
                res = c.rung(E[r])
                lst = res.pid[qi, : res.count[qi]]
                ctr[qi] += res.counters[qi]
                sel = collapse(lst, mask, groups, k)
                if len(sel) == k:
                    pid[qi], bits[qi], group[qi], count[qi], rung[qi] = lst[sel], pc.bits(res.dist[qi, sel]), groups[lst[sel]], k, r
                    done = True
                    break
            if done:
                continue
            ids, db = self.full(mask)
            sel = collapse(ids[qi], mask, groups, k)
            m = len(sel)
            pid[qi, :m], bits[qi, :m], group[qi, :m], count[qi], rung[qi] = ids[qi, sel], db[qi, sel], groups[ids[qi, sel]], m, EXACT
            if want_rounds:
                found, rem = [], ids[qi]
                while True:
                    rounds[qi] += 1
                    lst = rem[:k]
                    for g in groups[lst]:
                        if g not in found and len(found) < k:
                            found.append(g)
                    if len(found) == k or len(lst) < k:
                        break
                    rem = rem[~np.isin(groups[rem], found)]
                assert found == group[qi, :m].tolist()                       # the rounds give the collapse of all of A
        return pid, bits, count, rung, ctr, group, rounds


def check(got, want, what=""):
    check_allowed(got, want[:5] + (None,), what)
    assert np.array_equal(got.group, want[5]), f"{what}: groups"


def hist(x):
    return dict(zip(*[v.tolist() for v in np.unique(x, return_counts=True)]))


_MODELS = {}
atexit.register(_MODELS.clear)      # (with test_allowed's cases: the oracle's handles go before the interpreter takes its library apart)


def case_of(oracle, kind):
    """test_allowed's main_case (emu: 600 x 12-d, ef 8, k 5, 40 queries; gpu: 8000 x 32-d, ef 16, k 10, 600 queries) with its model"""
    c, k = main_case(oracle, kind)
    if kind not in _MODELS:
        _MODELS[kind] = (Model(c), {})
    return c, k, _MODELS[kind][0]


LAYOUTS = ["own", "docs4", "x0 bands 12", "x0 bands 40", "three", "one", "giant+12"]
MASKS = ["all", "x0>q80", "x0>q50", "5%", "per query"]
# (restriction, max_rungs): the whole ladder; two rungs only — for the 5 % no permitted rung expects k hits, the start rule sends the
# queries to the exact step with k groups to find (at the emulator's shape every ladder ends saturated: n < 4096)
CASES = [(m, -1) for m in MASKS] + [("5%", 2), ("per query", 2)]


def layout(c, name):
    n, x0 = len(c.pts), c.pts[:, 0]
    rng = np.random.default_rng(31)
    if name == "own":
        g = np.arange(n)
    elif name == "docs4":
        g = rng.permutation(n) // 4
    elif name.startswith("x0 bands"):
        b = int(name.split()[-1])
        g = np.minimum((x0.astype(np.float64) * b).astype(np.int64), b - 1)
    elif name == "three":
        g = np.arange(n) % 3
    elif name == "one":
        g = np.full(n, 7)
    else:                        # 0 and the all-ones value are both groups; the small ones collide in any power-of-two table
        g = np.full(n, FULL)
        g[rng.choice(n, 12, replace=False)] = np.arange(12) * 8192
    return g.astype(np.uint32)


def selections(c):
    """the second column of the table: bit 0 = x0 > q80, bit 1 = x0 > q50, bit 2 = a random 5 %"""
    x0 = c.pts[:, 0]
    r5 = np.random.default_rng(32).random(len(x0)) < 0.05
    return ((x0 > np.quantile(x0, 0.8)) * 1 + (x0 > np.quantile(x0, 0.5)) * 2 + r5 * 4).astype(np.uint32)


def cond_of(name):
    bit = {"x0>q80": 1, "x0>q50": 2, "5%": 4}[name]
    return {"sel": [v for v in range(8) if v & bit]}


def restriction(c, name):
    """(conds of the call, the masks of its distinct conditions, set_of [nq])"""
    n, nq, sel = len(c.pts), len(c.q), selections(c)
    if name == "all":
        return None, [np.ones(n, bool)], np.zeros(nq, np.int64)
    if name == "per query":
        each = [{}, cond_of("x0>q80"), cond_of("x0>q50"), cond_of("5%")]
        masks = [np.ones(n, bool)] + [(sel & b) != 0 for b in (1, 2, 4)]
        set_of = np.arange(nq) % 4
        return [each[s] for s in set_of], masks, set_of
    bit = {"x0>q80": 1, "x0>q50": 2, "5%": 4}[name]
    return cond_of(name), [(sel & bit) != 0], np.zeros(nq, np.int64)


def expected(oracle, kind, lay, mask, max_rungs=-1, want_rounds=False):
    c, k, model = case_of(oracle, kind)
    cache = _MODELS[kind][1]
    key = (lay, mask, max_rungs, want_rounds)
    if key not in cache:
        _, masks, set_of = restriction(c, mask)
        cache[key] = model.run(masks, set_of, layout(c, lay), k, max_rungs, want_rounds)
    return cache[key]


# ---- 1. every path ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", LAYOUTS)
def test_every_path(eng, oracle, lay):
    ida, kind = eng
    c, k, _ = case_of(oracle, kind)
    h, s = c.hnsw(ida), ida.Search()
    groups = layout(c, lay)
    table = h.attribute_table({"g": groups, "sel": selections(c)})
    for mask, max_rungs in CASES:
        conds = restriction(c, mask)[0]
        want = expected(oracle, kind, lay, mask, max_rungs)
        print(lay, "/", mask, "max_rungs", max_rungs, "rungs", hist(want[3]), "counts", hist(want[2]))
        got = h.search_grouped(c.q, table, "g", k, conds, s, max_rungs=max_rungs, counters=True)
        check(got, want, f"{lay} / {mask}, max_rungs {max_rungs}")
        for row, cnt in zip(got.group, got.count):
            assert len(set(row[:cnt].tolist())) == cnt                       # pairwise distinct groups
    check(h.search_grouped(c.q, table, "g", k, restriction(c, "x0>q80")[0], s), expected(oracle, kind, lay, "x0>q80"), f"{lay}, no counters")
    assert sum(s.allowed_kernel_ms()) >= 0.0


def test_the_cases_reach_every_path(eng, oracle):
    """asserted from the model, over the cases of test_every_path: rung 0; at least two later rungs; EXACT with count < k; EXACT with
    count == k; one call holding both rung answers and exact answers — and that call, the first such case, is made here: queries
    answered by rungs and queries answered by the exact rounds in one batch, each row still what the call returns for it alone"""
    ida, kind = eng
    c, k, _ = case_of(oracle, kind)
    rungs, exact_short, exact_full, mixed = set(), False, False, []
    for lay in LAYOUTS:
        for mask, max_rungs in CASES:
            want = expected(oracle, kind, lay, mask, max_rungs)
            count, rung = want[2], want[3]
            rungs |= set(rung.tolist())
            exact_short |= bool(np.any((rung == EXACT) & (count < k)))
            exact_full |= bool(np.any((rung == EXACT) & (count == k)))
            if np.any(rung == EXACT) and np.any(rung < NONE):
                mixed.append((lay, mask, max_rungs))
    print("rungs", sorted(rungs), "mixed calls", mixed)
    assert 0 in rungs and len({r for r in rungs if 0 < r < NONE}) >= 2
    assert exact_short and exact_full and mixed
    lay, mask, max_rungs = mixed[0]
    h, s = c.hnsw(ida), ida.Search()
    table = h.attribute_table({"g": layout(c, lay), "sel": selections(c)})
    conds, want = restriction(c, mask)[0], expected(oracle, kind, lay, mask, max_rungs)
    check(h.search_grouped(c.q, table, "g", k, conds, s, max_rungs=max_rungs, counters=True), want, f"{lay} / {mask}, the whole batch")
    for qi in (int(np.flatnonzero(want[3] == EXACT)[0]), int(np.flatnonzero(want[3] < NONE)[0])):      # one of each kind, alone
        one = conds[qi: qi + 1] if isinstance(conds, list) else conds
        got = h.search_grouped(c.q[qi: qi + 1], table, "g", k, one, s, max_rungs=max_rungs, counters=True)
        check(got, tuple(x[qi: qi + 1] for x in want[:6]), f"{lay} / {mask}, query {qi} alone")


# ---- 2. ground truth: the exact step alone, the ladder cut short -------------------------------------------------------------------------
@pytest.mark.parametrize("lay", ["x0 bands 12", "docs4", "giant+12"])
def test_ground_truth(eng, oracle, lay, monkeypatch):
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    c, k, _ = case_of(oracle, kind)
    h = c.hnsw(ida)
    table = h.attribute_table({"g": layout(c, lay), "sel": selections(c)})
    words = (len(c.pts) + 31) // 32
    # (segments of the scans, staging bound of a round's bitmaps in bytes: the default; three queries per chunk; one; five)
    knobs = [("0", "0"), ("3", str(3 * 4 * words))] + ([("64", "1"), ("1", str(5 * 4 * words))] if kind == "emu" else [])
    most = 0
    for mask in ("all", "x0>q50"):
        conds = restriction(c, mask)[0]
        want = expected(oracle, kind, lay, mask, 0, True)
        print(lay, "/", mask, "counts", hist(want[2]), "rounds", hist(want[6]))
        assert np.all(want[3] == EXACT)
        most = max(most, int(want[6].max()))
        for seg, stage in knobs:
            monkeypatch.setenv("IDIST_ALLOWED_SEGMENTS", seg)                 # (sampled when the context is made)
            monkeypatch.setenv("IDIST_GROUPED_STAGE", stage)
            got = h.search_grouped(c.q, table, "g", k, conds, ida.Search(), max_rungs=0, counters=True)
            check(got, want, f"{lay} / {mask}, segments {seg}, stage {stage}")
            assert np.all(got.counters == 0)
            for row, cnt in zip(got.group, got.count):
                assert len(set(row[:cnt].tolist())) == cnt
            check(h.search_grouped(c.q[:3], table, "g", k, conds, ida.Search(), max_rungs=0), tuple(x[:3] for x in want), "3 queries")
    assert most > 2 or not lay.startswith("x0 bands")                         # the multi-round exact path: more than two rounds
    monkeypatch.delenv("IDIST_ALLOWED_SEGMENTS")
    monkeypatch.delenv("IDIST_GROUPED_STAGE")
    for max_rungs in (1, 2):                                                  # the ladder cut short, then exact
        want = expected(oracle, kind, lay, "all", max_rungs)
        check(h.search_grouped(c.q, table, "g", k, None, ida.Search(), max_rungs=max_rungs, counters=True), want, f"{lay}, {max_rungs} rungs")
        assert set(want[3].tolist()) <= set(range(max_rungs)) | {EXACT}


# ---- 3. identity: every point its own group -------------------------------------------------------------------------------------------
def test_identity_with_search_match(eng, oracle):
    ida, kind = eng
    c, k, _ = case_of(oracle, kind)
    h, s = c.hnsw(ida), ida.Search()
    n = len(c.pts)
    table = h.attribute_table({"g": np.arange(n), "sel": selections(c)})
    seen = set()
    for mask in MASKS[1:]:
        conds = restriction(c, mask)[0]
        for max_rungs in (-1, 2, 0):
            a = h.search_grouped(c.q, table, "g", k, conds, s, max_rungs=max_rungs, counters=True)
            b = h.search_match(c.q, table, conds, k, s, max_rungs=max_rungs, counters=True)
            same(a, b, f"{mask}, max_rungs {max_rungs}")
            assert np.array_equal(a.counters, b.counters) and np.array_equal(a.group, np.where(b.pid == INVALID, 0, b.pid))
            seen |= set(a.rung.tolist())
    assert EXACT in seen and len({r for r in seen if r < NONE}) >= 2
    for max_rungs in (-1, 0):
        a = h.search_grouped(c.q, table, "g", k, None, s, max_rungs=max_rungs, counters=True)
        b = h.search_allowed(c.q, np.ones(n, bool), k, s, max_rungs=max_rungs, counters=True)
        same(a, b, f"no conds, max_rungs {max_rungs}")
        assert np.array_equal(a.counters, b.counters) and np.array_equal(a.group, b.pid)


@pytest.mark.parametrize("metric", ["l2sq", "l2", "cosine", "dot"])
def test_identity_metrics(eng, oracle, metric):
    """the emulator's shape on both engines; the report runs once: the distances are search_match's, bit for bit"""
    ida, kind = eng
    rng = np.random.default_rng(11)
    n, dim, ef, nq, k = 300, 7, 8, 12, 4
    raw = rng.random((n, dim), dtype=np.float32) - np.float32(0.3)
    q = rng.random((nq, dim), dtype=np.float32) - np.float32(0.3)
    code = {"l2sq": ida.METRIC_L2SQ, "l2": ida.METRIC_L2, "cosine": ida.METRIC_COSINE, "dot": ida.METRIC_DOT}[metric]
    h, s = ida.Hnsw.from_ordered_points(raw, ida.Builder().metric(code).ef_search(ef).seed(3)), ida.Search()
    sel = rng.integers(0, 8, n)
    table = h.attribute_table({"g": np.arange(n), "sel": sel, "g3": np.arange(n) % 3})
    seen = set()
    for conds, mask in ((None, np.ones(n, bool)), ({"sel": [1, 3, 5, 7]}, (sel & 1) != 0), ({"sel": 4}, sel == 4)):
        for max_rungs in (-1, 0):
            a = h.search_grouped(q, table, "g", k, conds, s, max_rungs=max_rungs, counters=True)
            b = h.search_allowed(q, mask, k, s, max_rungs=max_rungs, counters=True)
            same(a, b, f"{metric}, {conds}, max_rungs {max_rungs}")
            assert np.array_equal(a.counters, b.counters)
            seen |= set(a.rung.tolist())
            if max_rungs == 0:
                # three groups: the true answer is the nearest allowed member of each, reported as the exact restricted search reports it
                t = h.search_grouped(q, table, "g3", 3, conds, s, max_rungs=0)
                assert np.all(t.count == 3) and np.all(t.rung == EXACT) and np.all(np.sort(t.group, axis=1) == np.arange(3))
                for r in range(3):
                    one = h.search_allowed(q, mask & (np.arange(n) % 3 == r), 1, s, max_rungs=0)
                    at = np.argmax(t.group == r, axis=1)
                    assert np.array_equal(t.pid[np.arange(nq), at], one.pid[:, 0])
                    assert np.array_equal(pc.bits(t.distance[np.arange(nq), at]), pc.bits(one.distance[:, 0]))
    assert EXACT in seen and 0 in seen


# ---- 4. the kernel on its own ---------------------------------------------------------------------------------------------------------
SPECIAL = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32)


def kernel_lists(rng, width, k):
    """(pid [nq][width], count [nq], groups [n], n): every list draws its ids from a pool of its own, so that the groups of its
    entries can be set position by position.  The lists: (0) random groups from the special values and j * 8192; (1) a group repeated
    in adjacent lanes, in lanes 0 and 63 and across the step boundary 63 | 64; (2) the k-th new group is the last entry; (3) fewer
    than k groups; (4) count 0; (5) a count below the width, new groups behind it; (6) all distinct; (7) ids >= n among the entries"""
    nq = 8
    n = nq * width + 3
    pid = np.stack([q * width + rng.permutation(width) for q in range(nq)]).astype(np.uint32)
    count = np.full(nq, width, np.uint32)
    values = np.concatenate([SPECIAL, (np.arange(1, 5000, dtype=np.uint64) * 8192).astype(np.uint32)])
    groups = np.zeros(n, np.uint32)
    groups[pid[0]] = rng.choice(values[: max(4, min(len(values), width // 2))], width)
    g1 = rng.choice(values[:40], width)
    for a, b in ((3, 4), (0, 63), (63, 64), (10, 127), (128, 64)):
        if max(a, b) < width:
            g1[b] = g1[a]
    groups[pid[1]] = g1
    kk = min(k, width)
    g2 = values[np.arange(width) % max(kk - 1, 1)] if kk > 1 else np.full(width, values[0])
    if kk > 1:
        g2[-1] = values[kk - 1]
    groups[pid[2]] = g2
    groups[pid[3]] = values[np.arange(width) % max(1, min(kk - 1, 3))]
    groups[pid[4]] = values[: width] if width <= len(values) else 0
    count[4] = 0
    groups[pid[5]] = values[np.arange(width) % len(values)]
    count[5] = width // 2
    groups[pid[6]] = values[np.arange(width) % len(values)]
    groups[pid[7]] = rng.choice(values[:9], width)
    bad = rng.random(width) < 0.3
    pid[7][bad] = rng.choice(np.array([n, n + 5, 0x7FFFFFFF, INVALID], np.uint32), int(bad.sum()))
    return pid, count, groups, n


def kernel_model(pid, dist, count, groups, n, allowed, k):
    nq = len(pid)
    o_pid, o_dist = np.full((nq, k), INVALID, np.uint32), np.full((nq, k), INF_BITS, np.uint32)
    o_group, o_count = np.zeros((nq, k), np.uint32), np.zeros(nq, np.uint32)
    for q in range(nq):
        lst = pid[q, : count[q]]
        ok = lst < n
        a = np.zeros(len(lst), bool)
        a[ok] = allowed[q][lst[ok]]
        pos = np.flatnonzero(a)
        _, first = np.unique(groups[lst[pos]], return_index=True)
        sel = pos[np.sort(first)][:k]
        m = len(sel)
        o_pid[q, :m], o_dist[q, :m], o_group[q, :m], o_count[q] = lst[sel], dist[q, sel], groups[lst[sel]], m
    return o_pid, o_dist, o_group, o_count


@pytest.mark.parametrize("width", [1, 63, 64, 65, 129, 4096])
def test_collapse_kernel(eng, width):
    ida, kind = eng
    from instant_distance_amd import _capi
    from instant_distance_amd.api import allowed_bitmaps

    L = _capi.lib()
    mem = DeviceMem(kind)
    try:
        for k in sorted({1, 5, 64, width}):
            rng = np.random.default_rng(1000 * width + k)
            pid, count, groups, n = kernel_lists(rng, width, k)
            nq = len(pid)
            dist = rng.integers(0, 0x7F000000, (nq, width)).astype(np.uint32)
            col = guarded_u32(n) if kind == "emu" else np.empty(n, np.uint32)    # the column ends at a protected page
            col[:] = groups
            d_pid, d_dist, d_count, d_groups = mem.up(pid), mem.up(dist), mem.up(count), mem.up(col)
            # a bitmap that forbids every other first occurrence, and none
            every = [np.ones(n, bool) for _ in range(nq)]
            forbid = [a.copy() for a in every]
            for q in range(nq):
                lst = pid[q, : count[q]]
                lst = lst[lst < n]
                _, first = np.unique(groups[lst], return_index=True)
                forbid[q][lst[np.sort(first)[::2]]] = False
            for what, allowed in (("bitmap", forbid), ("no bitmap", every)):
                want = kernel_model(pid, dist, count, groups, n, allowed, k)
                outs = [np.full(nq * k + 5, FILL, np.uint32) for _ in range(3)] + [np.full(nq + 5, FILL, np.uint32)]
                d_outs = [mem.up(o) for o in outs]
                d_bits = mem.up(allowed_bitmaps(allowed, n)) if what == "bitmap" else None
                L.check(L.idist_grouped_collapse_device(d_pid, d_dist, d_count, nq, width, d_groups, n, d_bits, k, *d_outs, 0, None))
                got = [mem.down(d, o) for d, o in zip(d_outs, outs)]
                for i, name in enumerate(("ids", "distance bits", "groups")):
                    assert np.array_equal(got[i][: nq * k].reshape(nq, k), want[i]), (width, k, what, name)
                    assert np.all(got[i][nq * k:] == FILL), (width, k, what, name)    # nothing behind the last row
                assert np.array_equal(got[3][:nq], want[3]) and np.all(got[3][nq:] == FILL), (width, k, what)
                if width >= 65 and k >= 5 and what == "no bitmap":
                    assert want[3][4] == 0 and want[3].max() == min(k, width) and want[3][3] < k
        # nothing to do; the arguments
        out = np.full(8, FILL, np.uint32)
        d = mem.up(out)
        L.check(L.idist_grouped_collapse_device(d, d, d, 0, 4, d, 8, None, 2, d, d, d, d, 0, None))
        assert np.all(mem.down(d, out) == FILL)
        assert L.idist_grouped_collapse_device(d, d, d, 1, 4, d, 8, None, 0, d, d, d, d, 0, None) == 1
        assert L.idist_grouped_collapse_device(d, d, d, 1, 4, d, 8, None, 4097, d, d, d, d, 0, None) == 1
        assert L.idist_grouped_collapse_device(None, d, d, 1, 4, d, 8, None, 2, d, d, d, d, 0, None) == 1
        assert L.idist_grouped_collapse_device(d, d, d, 1, 4, None, 8, None, 2, d, d, d, d, 0, None) == 1
        assert L.idist_grouped_collapse_device(d, d, d, 1, 4, d, 8, None, 2, d, d, None, d, 0, None) == 1
        assert np.all(mem.down(d, out) == FILL)
    finally:
        mem.free()


def collapse_model_flat(pid, dist, count, groups, n, allowed, k):
    """kernel_model without a Python loop over the lists: an entry is kept when it lies below the count, names a point, is allowed and
    no kept-or-not valid entry in front of it has its group; the first k kept entries, in order.  allowed: bool [nq][n]"""
    nq, width = pid.shape
    ok = (np.arange(width)[None, :] < count[:, None]) & (pid < n)
    safe = np.where(ok, pid, 0)
    ok &= allowed[np.arange(nq)[:, None], safe]
    g = groups[safe]
    keep = ok.copy()
    for j in range(1, width):
        keep[:, j] &= ~np.any(ok[:, :j] & (g[:, :j] == g[:, j: j + 1]), axis=1)
    rank = np.cumsum(keep, axis=1) - 1
    keep &= rank < k
    o_pid, o_dist = np.full((nq, k), INVALID, np.uint32), np.full((nq, k), INF_BITS, np.uint32)
    o_group = np.zeros((nq, k), np.uint32)
    rows, cols = np.nonzero(keep)
    o_pid[rows, rank[rows, cols]], o_dist[rows, rank[rows, cols]], o_group[rows, rank[rows, cols]] = pid[rows, cols], dist[rows, cols], g[rows, cols]
    return o_pid, o_dist, o_group, keep.sum(axis=1).astype(np.uint32)


def test_collapse_kernel_past_the_grid(eng):
    """65,536 + 37 lists of width 3, k = 2: the first run in which grouped_select_kernel's workgroups take a second list.  List j and
    list j + 65,536 — the two lists of one workgroup — hold other points of other groups under complementary bitmaps, so a group set
    left in LDS by the first list, or the first list's bitmap row, changes the second list's answer."""
    # cap: min(np, 65536) workgroups of one list each, launch_grouped_select (idist_capi.hip)
    ida, kind = eng
    from instant_distance_amd import _capi

    L = _capi.lib()
    grid, width, k, n = 65536, 3, 2, 61
    nq = grid + 37
    rng = np.random.default_rng(4242)
    groups = (np.arange(n) % 5).astype(np.uint32) * np.uint32(0x33333333)            # (0 and 0xCCCCCCCC among them; neighbours differ)
    pid = rng.integers(0, n, (nq, width)).astype(np.uint32)
    pid[rng.random((nq, width)) < 0.05] = INVALID
    pid[grid:] = np.where(pid[:37] < n, (pid[:37] + 1) % n, pid[:37])                # the second list of a workgroup: other groups
    count = rng.integers(0, width + 1, nq).astype(np.uint32)
    count[:37] = count[grid:] = width
    allowed = rng.random((nq, n)) < 0.6
    allowed[grid:] = ~allowed[:37]
    dist = rng.integers(0, 0x7F000000, (nq, width)).astype(np.uint32)
    words = (n + 31) // 32
    padded = np.zeros((nq, words * 32), np.uint8)
    padded[:, :n] = allowed
    bits = np.packbits(padded, axis=1, bitorder="little").view("<u4")
    every = np.ones((nq, n), bool)
    # the vectorised model is the module's kernel_model, held on the rows that share a workgroup and a sample of the others
    rows = np.concatenate([np.arange(37), np.arange(grid, nq), rng.choice(nq, 200)])
    for a in (allowed, every):
        flat, slow = collapse_model_flat(pid[rows], dist[rows], count[rows], groups, n, a[rows], k), kernel_model(pid[rows], dist[rows], count[rows], groups, n, a[rows], k)
        assert all(np.array_equal(x, y) for x, y in zip(flat, slow))
    mem = DeviceMem(kind)
    try:
        d_pid, d_dist, d_count, d_groups, d_bits = mem.up(pid), mem.up(dist), mem.up(count), mem.up(groups), mem.up(bits)
        for what, a, d_b in (("bitmap", allowed, d_bits), ("no bitmap", every, None)):
            want = collapse_model_flat(pid, dist, count, groups, n, a, k)
            if what == "bitmap":           # the complementary bitmaps do change the answers of the rows that share a workgroup
                assert np.any(want[0][:37] != collapse_model_flat(pid[:37], dist[:37], count[:37], groups, n, a[grid:], k)[0])
            outs = [np.full(nq * k + 5, FILL, np.uint32) for _ in range(3)] + [np.full(nq + 5, FILL, np.uint32)]
            d_outs = [mem.up(o) for o in outs]
            L.check(L.idist_grouped_collapse_device(d_pid, d_dist, d_count, nq, width, d_groups, n, d_b, k, *d_outs, 0, None))
            got = [mem.down(d, o) for d, o in zip(d_outs, outs)]
            for i, name in enumerate(("ids", "distance bits", "groups")):
                assert np.array_equal(got[i][: nq * k].reshape(nq, k), want[i]), (what, name)
                assert np.all(got[i][nq * k:] == FILL), (what, name)
            assert np.array_equal(got[3][:nq], want[3]) and np.all(got[3][nq:] == FILL), what
            assert want[3].max() == k and want[3].min() == 0
    finally:
        mem.free()


# ---- 5. arguments and trivial cases -----------------------------------------------------------------------------------------------------
def test_argument_errors(eng):
    ida, kind = eng
    from instant_distance_amd import _capi

    rng = np.random.default_rng(1)
    pts = rng.random((50, 4), dtype=np.float32)
    mk = lambda: ida.Hnsw.from_ordered_points(pts, ida.Builder().ef_search(10))   # noqa: E731
    h, other = mk(), mk()
    two = np.stack([np.arange(50) // 2, np.arange(50) % 5], axis=1)
    t, t_other = h.attribute_table(two), other.attribute_table(two)
    s = ida.Search()
    ctx = s._bind(h)
    L = _capi.lib()
    u, f = _capi.u32p, _capi.f32p
    nq, k = 3, 5
    q = pts[:3]
    pid, dist, grp, cnt = np.zeros((nq, 10), np.uint32), np.zeros((nq, 10), np.float32), np.zeros((nq, 10), np.uint32), np.zeros(nq, np.uint32)
    clauses, and_lims = np.array([[1, 0, 2]], np.uint32), np.array([0, 1], np.uint32)
    keep = []

    def conds(n_cond):
        ol = np.array([0] + [1] * n_cond, np.uint32)
        keep.append(ol)
        return C.byref(_capi.AttrConds(u(clauses), u(and_lims), u(ol), n_cond))

    def call(attr=t, col=0, queries=q, cs=None, kk=k, max_rungs=-1, out=pid, group=grp, n=nq):
        return L.idist_search_batch_grouped(h._h, ctx, None if attr is None else attr._h, col, None if queries is None else f(queries), n, cs, kk,
                                            max_rungs, None if out is None else u(out), f(dist), None if group is None else u(group), u(cnt),
                                            None, None)

    assert call() == 0 and cnt.tolist() == [5, 5, 5]                          # out_rung / out_counters may be NULL
    assert call(group=None) == 0                                              # ... and out_group
    assert call(cs=conds(1)) == 0 and cnt.tolist() == [5, 5, 5] and call(cs=conds(3)) == 0
    for col in (2, 3, 0xFFFFFFFF):
        assert call(col=col) == 1 and b"2 columns" in L.idist_last_error() and b"group_col" in L.idist_last_error()
    assert call(attr=t_other) == 1 and call(attr=None) == 1
    assert call(kk=0) == 1 and call(kk=11) == 1 and call(max_rungs=-2) == 1
    for n_cond in (0, 2, 4):
        assert call(cs=conds(n_cond)) == 1 and b"n_cond" in L.idist_last_error()
    assert call(queries=None) == 1 and call(out=None) == 1
    assert call(n=0) == 0 and call(n=0, queries=None, out=None) == 0          # nq == 0 is no error
    assert call(kk=10) == 0 and cnt.tolist() == [10, 10, 10]                  # k == ef_search


def test_trivial_cases(eng, oracle):
    ida, kind = eng
    c, k, model = case_of(oracle, kind)
    h, s = c.hnsw(ida), ida.Search()
    groups = layout(c, "docs4")
    table = h.attribute_table({"g": groups, "sel": selections(c)})
    n, nq = len(c.pts), len(c.q)
    every = [np.ones(n, bool)]
    # k = ef_search and k = 1
    for kk in (c.ef, 1):
        want = model.run(every, np.zeros(nq, np.int64), groups, kk)
        check(h.search_grouped(c.q, table, "g", kk, None, s, counters=True), want, f"k {kk}")
    # a context reused for 5, 300 (the batch repeated) and 5 queries again
    want = expected(oracle, kind, "docs4", "x0>q50")
    conds = restriction(c, "x0>q50")[0]
    reps = -(-300 // nq)
    many = np.tile(c.q, (reps, 1))[:300]
    for sel in (slice(0, 5), None, slice(0, 5)):
        if sel is None:
            check(h.search_grouped(many, table, "g", k, conds, s, counters=True), tuple(np.tile(x, (reps,) + (1,) * (x.ndim - 1))[:300] for x in want), "300")
        else:
            check(h.search_grouped(c.q[sel], table, "g", k, conds, s, counters=True), tuple(x[sel] for x in want), "5")
    # ... then the other searches of the context: the staging is shared
    mask = mask_of(conds, {"sel": selections(c)})
    check_allowed(h.search_match(c.q, table, conds, k, s, counters=True), c.model(mask, k), "search_match after search_grouped")
    rc = range_case(oracle, kind)
    hr = rc.hnsw(ida)
    sel_r = np.random.default_rng(5).integers(0, 8, len(rc.raw)).astype(np.uint32)
    tr = hr.attribute_table({"g": np.arange(len(rc.raw)) // 3, "sel": sel_r})
    sr = ida.Search()
    rad = radii_of(rc)
    hr.search_grouped(rc.q, tr, "g", 3, {"sel": [1, 3, 5, 7]}, sr, max_rungs=0)
    wantr = range_model(rc, rad, [(sel_r & 1) != 0], np.zeros(len(rc.q), np.int64))[:5]
    check_range(hr.search_range_match(rc.q, rad, tr, {"sel": [1, 3, 5, 7]}, sr, counters=True), wantr, "search_range_match after search_grouped")
    # no queries; no points
    e = h.search_grouped(np.zeros((0, c.pts.shape[1]), np.float32), table, "g", k, None, s, counters=True)
    assert e.pid.shape == (0, k) and e.group.shape == (0, k) and e.rung.shape == (0,) and e.counters.shape == (0, 3)
    h0 = ida.Hnsw.from_ordered_points(np.zeros((0, 5), np.float32), ida.Builder())
    t0 = h0.attribute_table({"g": np.zeros(0, np.uint32)})
    r = h0.search_grouped(np.zeros((4, 5), np.float32), t0, "g", 3, None, ida.Search(), counters=True)
    assert np.all(r.count == 0) and np.all(r.rung == NONE) and np.all(r.pid == INVALID) and np.all(r.group == 0) and np.all(r.counters == 0)
    assert np.all(np.isposinf(r.distance))
    # nothing allowed
    r = h.search_grouped(c.q, table, "g", k, ida.AnyOf(), s, counters=True)
    assert np.all(r.count == 0) and np.all(r.rung == NONE) and np.all(r.pid == INVALID) and np.all(r.group == 0)


# ---- 6. Python ----------------------------------------------------------------------------------------------------------------------------
def test_python_layer(eng):
    ida, kind = eng
    rng = np.random.default_rng(2)
    pts = rng.random((120, 5), dtype=np.float32)
    h, s = ida.Hnsw.from_ordered_points(pts, ida.Builder().ef_search(12)), ida.Search()
    doc, tenant = np.arange(120) // 4 + TOP, rng.integers(0, 3, 120)
    table = h.attribute_table({"tenant": tenant, "doc": doc})
    q = rng.random((4, 5), dtype=np.float32)
    k = 6
    r = h.search_grouped(q, table, "doc", k, search=s, max_rungs=0)
    assert isinstance(r, ida.GroupedResult) and isinstance(r, ida.AllowedResult) and r.group.dtype == np.uint32 and r.group.shape == (4, k)
    assert np.array_equal(r.group, doc[r.pid].astype(np.uint32)) and np.all(r.count == k)
    d = ((pts[None, :, :] - q[:, None, :]) ** 2).sum(axis=2)
    for i in range(4):                                                        # the nearest member of each of the k nearest documents
        best = {g: np.flatnonzero(doc == g)[np.argmin(d[i, doc == g])] for g in np.unique(doc)}
        order = sorted(best.values(), key=lambda p: (d[i, p], p))[:k]
        assert r.pid[i].tolist() == order
    assert isinstance(h.search_grouped(q, table, "doc"), ida.GroupedResult)    # k, conds and search have defaults
    rt = h.search_grouped(q, table, "doc", k, {"tenant": 1}, s, counters=True)
    assert np.all(tenant[rt.pid[rt.pid != ida.INVALID]] == 1) and rt.counters.shape == (4, 3)
    # by=None on a one-column Attr, and on a one-column table
    a1 = h.attributes(doc)
    same(h.search_grouped(q, a1, None, k, search=s, max_rungs=0), r, "by=None, Attr")
    assert np.array_equal(h.search_grouped(q, a1, None, k, search=s, max_rungs=0).group, r.group)
    same(h.search_grouped(q, h.attribute_table({"doc": doc}), None, k, search=s, max_rungs=0), r, "by=None, one-column table")
    # errors
    with pytest.raises(KeyError) as e:
        h.search_grouped(q, table, "document", k, search=s)
    assert "tenant" in str(e.value) and "doc" in str(e.value)
    with pytest.raises(ValueError) as e:
        h.search_grouped(q, table, None, k, search=s)
    assert "tenant" in str(e.value) and "doc" in str(e.value)
    with pytest.raises(KeyError):
        h.search_grouped(q, a1, "doc", k, search=s)
    with pytest.raises(KeyError):
        h.search_grouped(q, table, "doc", k, {"month": 1}, s)
    with pytest.raises(TypeError):
        h.search_grouped(q, doc, None, k, search=s)
    with pytest.raises(TypeError):
        h.search_grouped(q, a1, None, k, {"doc": 1}, s)                        # conditions need a table
    with pytest.raises(ida.IdistError):
        h.search_grouped(q, table, "doc", 13, search=s)                        # k > ef_search
    # HnswMap: the values in result order
    values = [f"v{i}" for i in range(120)]
    mp = ida.Builder().seed(7).ef_search(12).build(pts, values)
    docs = np.array([int(x[1:]) // 4 for x in mp.values])                      # PointId order, as mp.values
    mt = mp.attribute_table({"doc": docs, "par": docs % 2})
    items = mp.search_grouped(q, mt, "doc", k, {"par": 0}, ida.Search())
    rr = mp.hnsw.search_grouped(q, mt, "doc", k, {"par": 0}, ida.Search())
    assert len(items) == 4
    for i, row in enumerate(items):
        assert [it.pid for it in row] == rr.pid[i, : rr.count[i]].tolist() and len(row) == k
        assert [int(it.value[1:]) // 4 for it in row] == rr.group[i, : rr.count[i]].tolist()
        assert all(it.value == mp.values[it.pid] and np.array_equal(it.point, mp.hnsw[it.pid]) and int(it.value[1:]) // 4 % 2 == 0 for it in row)
        assert len({int(it.value[1:]) // 4 for it in row}) == k
