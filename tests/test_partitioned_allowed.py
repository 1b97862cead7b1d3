"""Restricted search over a partitioned index, one allowed set per query (idist_partitioned_search_batch_allowed_sets, include/idist.h;
DESIGN.md sections 4.8 and 8.1) and the bitmap slice kernel behind it (idist_allowed_slice_device).

The call is DEFINED by composing two exact things: row q is the merge, by (distance bits, global id), of what the single-index
restricted search returns on every part for the slice of query q's set that falls into the part.  So everything is compared exactly
(ids, counts, rungs and counters with array_equal, distances as bit patterns), and the expected arrays come from the oracle model
`Case.model` of tests/test_allowed.py applied per part and merged with `merge_reference` of tests/test_partitioned.py — never from
the new call.  Every case runs on the CPU emulator and (-m gpu) on the MI355X."""
import atexit
import ctypes as C
import mmap
from types import SimpleNamespace

import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params
from test_allowed import Case, ladder
from test_partitioned import DeviceMem, merge_reference, uneven_bounds

INVALID = 0xFFFFFFFF
INF_BITS = 0x7F800000
NONE, EXACT = 254, 255
HALF = np.float32(0.5)


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


def S(kind, emu, gpu):
    return gpu if kind == "gpu" else emu


# ---- the definition, restated ------------------------------------------------------------------------------------------------------
class Rows:
    """Case.model — the very code — on the queries `sel` of a case (what a rung returns for a query does not depend on who else is in
    the batch): the model of one set runs over the queries that use it, not over the whole batch."""
    model = Case.model

    def __init__(self, c, sel):
        self.c, self.sel = c, sel
        self.oracle, self.pts, self.q, self.ef, self.metric = c.oracle, c.pts, c.q[sel], c.ef, c.metric

    def rung(self, ef):
        r, sel = self.c.rung(ef), self.sel
        return SimpleNamespace(pid=r.pid[sel], count=r.count[sel], dist=r.dist[sel], counters=r.counters[sel])


class SerialCase(Case):
    """a Case over the oracle's SEQUENTIAL build: the concurrent build Case uses gives a valid graph that depends on the schedule, and
    with it whether a given launch overflows a tie region; this one is the same graph in every run"""

    def __init__(self, oracle, pts, q, ef, metric=0, ef_construction=100):
        self.oracle, self.pts, self.q, self.ef, self.metric = oracle, pts, q, ef, metric
        self.oix = oracle.Index.build(pts, oracle.default_config(metric=metric, ef_search=ef, ef_construction=ef_construction), threads=1)
        self.zero, self.layers = self.oix.zero, self.oix.layers
        self._rungs = {}


def expected(cs, b, masks, set_of, k, max_rungs=-1):
    """cs[p]: the Case of part p (None: an empty part), b: the parts' bounds, masks: the GLOBAL sets.  Per part the model of every
    set's slice over the queries that use the set, ids local; then the merge of the P lists with ids + base[p].
    -> (pid, distance bits, count, rung [nq][P], counters)"""
    P, nq = len(cs), len(set_of)
    set_of = np.asarray(set_of)
    pid = np.full((P, nq, k), INVALID, np.uint32)
    bits = np.full((P, nq, k), INF_BITS, np.uint32)
    cnt, rung, ctr = np.zeros((P, nq), np.uint32), np.full((P, nq), NONE, np.uint32), np.zeros((P, nq, 3), np.uint32)
    for p, c in enumerate(cs):
        if c is None:
            continue
        for si, m in enumerate(masks):
            sel = np.flatnonzero(set_of == si)
            if len(sel):
                w = Rows(c, sel).model(m[b[p]: b[p + 1]], k, max_rungs)
                pid[p, sel], bits[p, sel], cnt[p, sel], rung[p, sel], ctr[p, sel] = w[:5]
    o_pid, o_bits, o_cnt, o_ctr = merge_reference(pid, bits, cnt, ctr, np.asarray(b[:-1], np.uint32), k)
    return o_pid, o_bits, o_cnt, np.ascontiguousarray(rung.T), o_ctr


def check(got, want, what=""):
    w_pid, w_bits, w_cnt, w_rung, w_ctr = want
    assert got.rung.shape == w_rung.shape, f"{what}: rung shape {got.rung.shape}"
    assert np.array_equal(got.rung, w_rung), f"{what}: rungs {np.unique(got.rung, return_counts=True)} != {np.unique(w_rung, return_counts=True)}"
    assert np.array_equal(got.count, w_cnt), f"{what}: counts"
    assert np.array_equal(got.pid, w_pid), f"{what}: ids"
    assert np.array_equal(pc.bits(got.distance), w_bits), f"{what}: distance bits"
    if got.counters is not None:
        assert np.array_equal(got.counters, w_ctr), f"{what}: counters"


_PARTS = {}
atexit.register(_PARTS.clear)      # (the oracle's handles go before the interpreter takes its library apart)


def sizes(kind):
    """(n, dim, ef_search, k, nq)"""
    return S(kind, (660, 8, 8, 5, 24), (12000, 32, 16, 10, 600))


def main_parts(oracle, kind, P):
    """the points cut by uneven_bounds and one Case per part (cached per process) -> (pts, q, bounds, cases, k)"""
    if (kind, P) not in _PARTS:
        n, dim, ef, k, nq = sizes(kind)
        rng = np.random.default_rng(S(kind, 1, 2))
        pts, q = rng.random((n, dim), dtype=np.float32), rng.random((nq, dim), dtype=np.float32)
        b = uneven_bounds(n, P)
        _PARTS[kind, P] = (pts, q, b, [Case(oracle, np.ascontiguousarray(pts[b[p]: b[p + 1]]), q, ef) for p in range(P)], k)
    return _PARTS[kind, P]


def partitioned(ida, cs, builder=None):
    hs = [c.hnsw(ida, builder() if builder else None) for c in cs]
    return ida.PartitionedHnsw.from_hnsws(hs), hs


def global_masks(pts, b, k):
    """eight GLOBAL sets: all; random 0.5; random 0.05; coordinate 0 above its 0.8 quantile; a set confined to one part (the last);
    fewer than k members spread over two parts (the first and the last); exactly k members in one part (the last); empty"""
    n, P, x0 = len(pts), len(b) - 1, pts[:, 0]
    rng = np.random.default_rng(77)
    confined = np.zeros(n, bool)
    confined[b[P - 1]: n] = rng.random(n - b[P - 1]) < 0.5
    few = np.zeros(n, bool)
    few[rng.choice(b[1], (k - 1) // 2, replace=False)] = True
    few[b[P - 1] + rng.choice(n - b[P - 1], k - 1 - (k - 1) // 2, replace=False)] = True
    exactly_k = np.zeros(n, bool)
    exactly_k[b[P - 1] + rng.choice(n - b[P - 1], k, replace=False)] = True
    masks = [np.ones(n, bool), rng.random(n) < 0.5, rng.random(n) < 0.05, x0 > np.quantile(x0, 0.8), confined, few, exactly_k,
             np.zeros(n, bool)]
    assert few.sum() == k - 1 and exactly_k.sum() == k and (P == 1 or (few[: b[1]].any() and few[b[P - 1]:].any()))
    return masks


# ---- 1. the slice kernel alone ---------------------------------------------------------------------------------------------------
_GUARDED = []


def guarded_words(n_words):
    """emulator only ("device" memory is host memory): n_words uint32 that END at a page no access is allowed to — a read of one word
    past the source ends the process instead of going unnoticed"""
    page = mmap.PAGESIZE
    assert n_words * 4 <= page
    mm = mmap.mmap(-1, 2 * page)
    addr = C.addressof(C.c_char.from_buffer(mm))
    libc = C.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    assert libc.mprotect(addr + page, page, 0) == 0, C.get_errno()            # PROT_NONE
    _GUARDED.append(mm)                                                        # (stays mapped for the rest of the process)
    return np.frombuffer(mm, dtype=np.uint32, count=n_words, offset=page - 4 * n_words)


def slice_model(src_rows, bit_offset, n_out):
    words_out = (n_out + 31) // 32
    out = np.zeros((len(src_rows), words_out), np.uint32)
    for s, row in enumerate(src_rows):
        bits = np.unpackbits(np.ascontiguousarray(row).view(np.uint8), bitorder="little")[bit_offset: bit_offset + n_out]
        padded = np.zeros(words_out * 32, np.uint8)
        padded[:n_out] = bits
        out[s] = np.packbits(padded, bitorder="little").view("<u4")
    return out


@pytest.mark.parametrize("n_sets", [1, 3])
def test_slice_kernel(eng, n_sets):
    """random ("dirty") bits all around the range; a pitch larger than the row; a source that ENDS at the last word that may be read;
    the output pre-filled with a pattern, every word of it compared with a numpy unpackbits / packbits model"""
    ida, kind = eng
    from instant_distance_amd import _capi

    L = _capi.lib()
    rng = np.random.default_rng(100 + n_sets)
    mem = DeviceMem(kind)
    try:
        for bit_offset in (0, 1, 31, 32, 33, 63, 81):
            for n_out in (1, 31, 32, 33, 64, 65, 205):
                w_end = (bit_offset + n_out + 31) // 32                       # words of a row that may be read
                words_out = (n_out + 31) // 32
                for pitch in (w_end, w_end + 3):
                    n_src = (n_sets - 1) * pitch + w_end                      # the last row ends where reading must end
                    src = guarded_words(n_src) if kind == "emu" else np.empty(n_src, np.uint32)
                    src[:] = rng.integers(0, 2**32, n_src, dtype=np.uint64).astype(np.uint32)
                    rows = [src[s * pitch: s * pitch + w_end] for s in range(n_sets)]
                    out = np.full((n_sets, words_out), 0xABABABAB, np.uint32)
                    d_src, d_out = mem.up(src), mem.up(out)
                    L.check(L.idist_allowed_slice_device(d_src, n_sets, pitch, bit_offset, n_out, d_out, 0, None))
                    got = mem.down(d_out, out)
                    assert np.array_equal(got, slice_model(rows, bit_offset, n_out)), (n_sets, bit_offset, n_out, pitch)
        # nothing to do: accepted, nothing written
        out = np.full((n_sets, 2), 0xABABABAB, np.uint32)
        d_src, d_out = mem.up(np.zeros(8, np.uint32)), mem.up(out)
        L.check(L.idist_allowed_slice_device(d_src, n_sets, 2, 5, 0, d_out, 0, None))
        L.check(L.idist_allowed_slice_device(d_src, 0, 2, 5, 40, d_out, 0, None))
        assert np.all(mem.down(d_out, out) == 0xABABABAB)
        # a pitch below the words a row's range needs is refused
        assert L.idist_allowed_slice_device(d_src, n_sets, 1, 5, 40, d_out, 0, None) == 1
    finally:
        mem.free()


@pytest.mark.gpu
@pytest.mark.parametrize("bit_offset", [1, 31, 33])
def test_slice_kernel_past_the_grid_gpu(engine_loader, bit_offset):
    """more output words than lanes in the grid: 3 rows of 350,001 words, a lane writes word i and word i + 256 x 4096; the last word
    of a row holds 5 bits; random bits all around the range, the source ends at the last word that may be read"""
    # cap: min(ceil(total / 256), 4096) workgroups of 256 lanes, one output word per lane, idist_allowed_slice_device (idist_capi.hip)
    engine_loader("gpu")
    from instant_distance_amd import _capi

    L = _capi.lib()
    n_sets, n_out = 3, 32 * 350000 + 5
    words_out = (n_out + 31) // 32
    assert n_sets * words_out > 256 * 4096
    w_end = (bit_offset + n_out + 31) // 32
    pitch = w_end + 3
    rng = np.random.default_rng(170 + bit_offset)
    src = rng.integers(0, 2**32, (n_sets - 1) * pitch + w_end, dtype=np.uint64).astype(np.uint32)
    rows = [src[s * pitch: s * pitch + w_end] for s in range(n_sets)]
    mem = DeviceMem("gpu")
    try:
        out = np.full((n_sets, words_out), 0xABABABAB, np.uint32)
        d_out = mem.up(out)
        L.check(L.idist_allowed_slice_device(mem.up(src), n_sets, pitch, bit_offset, n_out, d_out, 0, None))
        assert np.array_equal(mem.down(d_out, out), slice_model(rows, bit_offset, n_out))
    finally:
        mem.free()


# ---- 2. composition parity: every path of every part in one call --------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_composition_parity(eng, oracle, P):
    ida, kind = eng
    pts, q, b, cs, k = main_parts(oracle, kind, P)
    n, nq = len(pts), len(q)
    # base[p] is no multiple of 32 in general: the three-part cut of both sizes has such a base (12000 points cut in two or five have
    # none), the emulator's 660 points at every P > 1
    assert any(x % 32 for x in uneven_bounds(n, 3))
    if P == 3 or (kind == "emu" and P > 1):
        assert any(x % 32 for x in b[:-1])
    ph, hs = partitioned(ida, cs)
    masks = global_masks(pts, b, k)
    assert len(masks) == 8
    sets = np.stack(masks)
    seen = set()
    for max_rungs in (-1, 2, 0):
        for shift in (0, 3):
            set_of = (np.arange(nq) + shift) % 8
            want = expected(cs, b, masks, set_of, k, max_rungs)
            print("max_rungs", max_rungs, "shift", shift, "rungs", dict(zip(*[x.tolist() for x in np.unique(want[3], return_counts=True)])))
            assert np.array_equal(want[2], np.minimum(k, sets.sum(axis=1))[set_of])           # count == min(k, |A|)
            if P > 1:                                                                         # the confined set: NONE in the other parts
                assert np.all(want[3][set_of == 4, : P - 1] == NONE) and np.all(want[3][set_of == 4, P - 1] != NONE)
            seen |= set(want[3].ravel().tolist())
            check(ph.search_allowed_sets(q, sets, set_of, k, max_rungs=max_rungs, counters=True), want, f"max_rungs {max_rungs}, shift {shift}")
            check(ph.search_allowed_sets(q, sets, set_of, k, max_rungs=max_rungs), want, f"max_rungs {max_rungs}, shift {shift}, no counters")
    # the inputs reach the paths: two different rungs of the ladder, the exact step, nothing to find
    assert len({r for r in seen if r < NONE}) >= 2 and EXACT in seen and NONE in seen
    assert ph.last_merge_ms() >= 0.0 and ph.last_allowed_slice_ms() >= 0.0
    ks = ph.last_search_kernel_ms()
    assert ks.shape == (P,)
    # one shared set, and one query
    want = expected(cs, b, [masks[3]], np.zeros(nq, np.int64), k)
    check(ph.search_allowed(q, masks[3], k, counters=True), want, "search_allowed")
    check(ph.search_allowed(q, np.flatnonzero(masks[3]), k), want, "search_allowed, global ids")
    items = ph.search_one_allowed(q[0], masks[3], k)
    assert [it.pid for it in items] == want[0][0, : want[2][0]].tolist()
    assert all(masks[3][it.pid] and np.array_equal(it.point, pts[it.pid]) for it in items)


# ---- 3. / 4. identities ------------------------------------------------------------------------------------------------------------------
def test_one_part_is_the_identity(eng, oracle):
    ida, kind = eng
    pts, q, b, cs, k = main_parts(oracle, kind, 1)
    ph, hs = partitioned(ida, cs)
    masks = global_masks(pts, b, k)
    set_of = np.arange(len(q)) % 8
    for max_rungs in (-1, 2):
        a = ph.search_allowed_sets(q, masks, set_of, k, max_rungs=max_rungs, counters=True)
        o = hs[0].search_allowed_sets(q, masks, set_of, k, ida.Search(), max_rungs=max_rungs, counters=True)
        assert a.rung.shape == (len(q), 1) and np.array_equal(a.rung[:, 0], o.rung)
        assert np.array_equal(a.pid, o.pid) and np.array_equal(a.count, o.count) and np.array_equal(a.counters, o.counters)
        assert np.array_equal(pc.bits(a.distance), pc.bits(o.distance))
        assert len(set(o.rung.tolist())) >= 4


def test_all_ones_is_search_batch(eng, oracle):
    ida, kind = eng
    pts, q, b, cs, _ = main_parts(oracle, kind, 3)
    ph, hs = partitioned(ida, cs)
    ef = cs[0].ef
    a = ph.search_allowed_sets(q, np.ones((2, len(pts)), bool), np.arange(len(q)) % 2, ef, counters=True)
    o = ph.search_batch(q, counters=True)
    assert np.all(a.rung == 0)
    assert np.array_equal(a.pid, o.pid) and np.array_equal(a.count, o.count) and np.array_equal(a.counters, o.counters)
    assert np.array_equal(pc.bits(a.distance), pc.bits(o.distance))


# ---- 5. max_rungs = 0 is the exact answer ------------------------------------------------------------------------------------------------
def test_no_rung_is_bruteforce_over_the_allowed_rows(eng, oracle):
    ida, kind = eng
    pts, q, b, cs, k = main_parts(oracle, kind, 3)
    ph, hs = partitioned(ida, cs)
    masks = global_masks(pts, b, k)
    set_of = np.arange(len(q)) % 8
    got = ph.search_allowed_sets(q, masks, set_of, k, max_rungs=0, counters=True)
    assert np.all((got.rung == EXACT) | (got.rung == NONE)) and np.all(got.counters == 0)
    for si, mask in enumerate(masks):
        ids = np.flatnonzero(mask).astype(np.uint32)
        sel = np.flatnonzero(set_of == si)
        kk = min(k, len(ids))
        assert np.all(got.count[sel] == kk)
        assert np.all(got.pid[sel, kk:] == INVALID) and np.all(np.isposinf(got.distance[sel, kk:]))
        if not kk:
            assert np.all(got.rung[sel] == NONE)
            continue
        bp, bd = oracle.bruteforce(pts[ids], q[sel], kk, threads=8)        # the concatenation IS the global-id order
        assert np.array_equal(got.pid[sel, :kk], ids[bp]) and np.array_equal(pc.bits(got.distance[sel, :kk]), pc.bits(bd)), f"set {si}"
        holds = np.array([mask[b[p]: b[p + 1]].any() for p in range(3)])    # EXACT where the part holds some of the set, else NONE
        assert np.all(got.rung[sel] == np.where(holds, EXACT, NONE)[None, :])


# ---- 6. the global bitmap's padding bits -----------------------------------------------------------------------------------------------
def test_global_padding_bits(eng, oracle):
    """N no multiple of 32, straight through the ABI with EVERY padding bit of every set set; a set of padding bits only"""
    ida, kind = eng
    from instant_distance_amd import _capi
    from instant_distance_amd.api import allowed_bitmap

    n, dim, ef, k, nq, P = S(kind, 205, 1037), 5, 8, 3, 13, 3
    rng = np.random.default_rng(12)
    pts, q = rng.random((n, dim), dtype=np.float32), rng.random((nq, dim), dtype=np.float32)
    b = uneven_bounds(n, P)
    assert n % 32 and any(x % 32 for x in b[1:-1])
    cs = [Case(oracle, np.ascontiguousarray(pts[b[p]: b[p + 1]]), q, ef) for p in range(P)]
    ph, hs = partitioned(ida, cs)
    last = np.zeros(n, bool)
    last[(n - 1) // 32 * 32:] = True                                        # members in the last, partial word only
    masks = [rng.random(n) < 0.4, np.ones(n, bool), last, np.zeros(n, bool), np.zeros(n, bool)]   # the fifth: padding bits only
    beyond = np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
    dirty = np.stack([allowed_bitmap(m, n) for m in masks])
    dirty[:, -1] |= beyond
    keep = dirty.copy()
    set_of = (np.arange(nq) % 5).astype(np.uint32)
    L = _capi.lib()
    for max_rungs in (-1, 0):
        pid, dist = np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.float32)
        cnt, rung, ctr = np.zeros(nq, np.uint32), np.zeros((nq, P), np.uint32), np.zeros((nq, 3), np.uint32)
        L.check(L.idist_partitioned_search_batch_allowed_sets(ph._h, _capi.f32p(q), nq, _capi.u32p(dirty), 5, _capi.u32p(set_of), k, max_rungs,
                                                              _capi.u32p(pid), _capi.f32p(dist), _capi.u32p(cnt), _capi.u32p(rung), _capi.u32p(ctr)))
        got = ida.AllowedResult(pid, dist, cnt, rung, ctr)
        check(got, expected(cs, b, masks, set_of, k, max_rungs), f"max_rungs {max_rungs}")
        pad = np.flatnonzero(set_of >= 3)                                   # the empty set and the set of padding bits only
        assert np.all(got.rung[pad] == NONE) and np.all(got.count[pad] == 0) and np.all(got.pid[pad] == INVALID)
        assert np.all(np.isposinf(got.distance[pad]))
    assert np.array_equal(dirty, keep)                                      # the caller's buffer is not written
    # out_rung and out_counters are optional
    pid, dist, cnt = np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.float32), np.zeros(nq, np.uint32)
    L.check(L.idist_partitioned_search_batch_allowed_sets(ph._h, _capi.f32p(q), nq, _capi.u32p(dirty), 5, _capi.u32p(set_of), k, -1,
                                                          _capi.u32p(pid), _capi.f32p(dist), _capi.u32p(cnt), None, None))
    want = expected(cs, b, masks, set_of, k)
    assert np.array_equal(pid, want[0]) and np.array_equal(pc.bits(dist), want[1]) and np.array_equal(cnt, want[2])


# ---- 7. the metrics --------------------------------------------------------------------------------------------------------------------
def metric_sizes(kind):
    """(n, dim, ef_search, nq, k, P)"""
    return S(kind, (300, 7, 8, 12, 4, 3), (5000, 24, 16, 300, 8, 3))


def test_metric_l2(eng, oracle):
    ida, kind = eng
    n, dim, ef, nq, k, P = metric_sizes(kind)
    rng = np.random.default_rng(11)
    pts, q = rng.random((n, dim), dtype=np.float32), rng.random((nq, dim), dtype=np.float32)
    b = uneven_bounds(n, P)
    cs = [Case(oracle, np.ascontiguousarray(pts[b[p]: b[p + 1]]), q, ef, 1) for p in range(P)]
    ph, hs = partitioned(ida, cs)
    rng = np.random.default_rng(8)
    masks = [rng.random(n) < share for share in (1.0, 0.2, 0.03)]
    set_of = rng.integers(0, 3, nq)
    for max_rungs in (-1, 0):
        check(ph.search_allowed_sets(q, masks, set_of, k, max_rungs=max_rungs, counters=True), expected(cs, b, masks, set_of, k, max_rungs),
              f"max_rungs {max_rungs}")


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_metric_by_definition(eng, oracle, metric):
    """the call on the metric parts == the model over L2SQ parts of the transformed rows with the query transformed the same way;
    distances 0.5f * d / 0.5f * (d - t) in numpy f32, bit for bit — the report runs once, after the merge of the raw distances"""
    ida, kind = eng
    n, dim, ef, nq, k, P = metric_sizes(kind)
    rng = np.random.default_rng(11)
    raw = rng.random((n, dim), dtype=np.float32) - np.float32(0.3)
    q = rng.random((nq, dim), dtype=np.float32) - np.float32(0.3)
    if metric == "cosine":
        rows, qt = ida.normalize(raw), ida.normalize(q)
        builder = lambda: ida.Builder().metric(ida.METRIC_COSINE)          # noqa: E731
    else:
        rows, Sb = ida.augment_dot(raw)                                     # the bound of the WHOLE set, shared by the parts
        qt = np.ascontiguousarray(np.concatenate([q, np.zeros((len(q), 1), np.float32)], axis=1))
        sq = ida.augment_dot(q, return_norm2=True)[2]
        t = (sq + np.float32(Sb)).astype(np.float32)
        builder = lambda: ida.Builder().metric(ida.METRIC_DOT).dot_bound(Sb)   # noqa: E731
    b = uneven_bounds(n, P)
    cs = [Case(oracle, np.ascontiguousarray(rows[b[p]: b[p + 1]]), qt, ef) for p in range(P)]   # the L2SQ graphs ARE the metric's
    hs = [ida.Hnsw.from_parts(np.ascontiguousarray(raw[b[p]: b[p + 1]]), c.zero, c.layers, builder().ef_search(ef)) for p, c in enumerate(cs)]
    if metric == "dot":
        bounds = {np.float32(h.info().dot_bound).tobytes() for h in hs}
        assert len(bounds) == 1 and np.float32(Sb).tobytes() in bounds      # the parts share one dot_bound, bit for bit
    ph = ida.PartitionedHnsw.from_hnsws(hs)
    rng = np.random.default_rng(9)
    masks = [rng.random(n) < share for share in (1.0, 0.2, 0.03)]
    set_of = np.arange(nq) % 3
    seen = set()
    for max_rungs in (-1, 0):
        w_pid, w_bits, w_cnt, w_rung, w_ctr = expected(cs, b, masks, set_of, k, max_rungs)
        a = ph.search_allowed_sets(q, masks, set_of, k, max_rungs=max_rungs, counters=True)
        assert np.array_equal(a.pid, w_pid) and np.array_equal(a.count, w_cnt) and np.array_equal(a.rung, w_rung)
        assert np.array_equal(a.counters, w_ctr)
        d_raw = w_bits.view(np.float32)
        with np.errstate(all="ignore"):
            d = HALF * d_raw if metric == "cosine" else np.where(np.isposinf(d_raw), d_raw, HALF * (d_raw - t[:, None]))
        assert d.dtype == np.float32 and np.array_equal(pc.bits(a.distance), pc.bits(d))
        seen |= set(w_rung.ravel().tolist())
    assert EXACT in seen and len(seen) >= 3


# ---- 8. strict ties ------------------------------------------------------------------------------------------------------------------------
def test_tie_overflow_never_escapes(eng, oracle):
    """the dense integer grid and the ONE-entry tie region of tests/test_allowed_sets.py, cut into two parts: rungs' launches
    overflow the region, the part searches the rung again itself and the call returns the model's arrays"""
    ida, kind = eng
    rng = np.random.default_rng(3000002)
    n, ef, k = S(kind, 420, 12000), 8, 4
    pts = pc.gen_points(rng, n, 3, "grid")
    q = np.ascontiguousarray(pts[: S(kind, 12, 600)] + np.float32(0.25))
    b = uneven_bounds(n, 2)
    # (emulator: the oracle's sequential build, so that the last assertion below speaks about the same graphs in every run; at the GPU
    #  size that build takes a quarter of a minute on this grid, so the concurrent one serves there and the assertion stays here)
    mk = SerialCase if kind == "emu" else Case
    cs = [mk(oracle, np.ascontiguousarray(pts[b[p]: b[p + 1]]), q, ef, metric=1, ef_construction=S(kind, 8, 64)) for p in range(2)]
    rng = np.random.default_rng(4)
    masks = [rng.random(n) < 0.15, rng.random(n) < 0.6]
    set_of = np.arange(len(q)) % 2
    want = expected(cs, b, masks, set_of, k)
    assert len({r for r in want[3].ravel().tolist() if r < NONE}) >= 2             # the ladders climb
    ph, hs = partitioned(ida, cs, lambda: ida.Builder().tie_capacity(1))
    check(ph.search_allowed_sets(q, masks, set_of, k, counters=True), want)
    if kind != "emu":
        return
    # the inputs do overflow that region: under the DROP policy, which flags an overflow instead of escalating, a launch of some
    # rung that answered queries of some part is flagged
    flagged = False
    for p, c in enumerate(cs):
        for r in sorted({r for r in want[3][:, p].tolist() if r < NONE}):
            hd = ida.Hnsw.from_parts(c.pts, c.zero, c.layers, ida.Builder().metric(1).ef_search(ladder(ef)[r]).tie_capacity(1).tie_policy(ida.TIES_DROP))
            sd = ida.Search()
            hd.search_batch(q, sd)
            flagged = flagged or sd.tie_overflowed()
            if flagged:
                break
    assert flagged


# ---- 9. degenerate shapes ----------------------------------------------------------------------------------------------------------------
def test_degenerate_shapes(eng, oracle):
    ida, kind = eng
    rng = np.random.default_rng(4)
    pts = pc.gen_points(rng, 3, 5)
    ph, ids = ida.PartitionedHnsw.build(pts, ida.Builder().seed(1), parts=5)      # two of the five parts are empty
    sizes_ = [len(p) for p in ph.parts]
    assert len(ph) == 3 and sizes_.count(0) == 2
    q = pc.gen_points(rng, 4, 5)
    mask = np.array([True, False, True])
    for max_rungs in (-1, 0):
        r = ph.search_allowed(q, mask, 2, max_rungs=max_rungs, counters=True)
        gids = np.flatnonzero(mask).astype(np.uint32)
        opid, odist = oracle.bruteforce(np.stack([ph[int(g)] for g in gids]), q, 2)
        assert np.all(r.count == 2) and np.array_equal(r.pid, gids[opid]) and np.array_equal(pc.bits(r.distance), pc.bits(odist))
        assert r.rung.shape == (4, 5) and np.all(r.counters == 0)
        for p in range(5):                                                         # an empty part or an empty slice: NONE; else |A_p| <= k: EXACT
            lo = int(ph._base[p])
            assert np.all(r.rung[:, p] == (EXACT if mask[lo: lo + sizes_[p]].any() else NONE))
    r = ph.search_allowed(q, np.ones(3, bool), 5, counters=True)                    # fewer points than k: what there is, padded
    assert np.all(r.count == 3) and np.all(r.pid[:, 3:] == INVALID) and np.all(np.isposinf(r.distance[:, 3:]))
    assert np.array_equal(np.sort(r.pid[:, :3], axis=1), np.tile(np.arange(3, dtype=np.uint32), (4, 1)))
    # every part empty
    ph0, ids0 = ida.PartitionedHnsw.build(np.zeros((0, 5), np.float32), ida.Builder(), parts=2)
    r0 = ph0.search_allowed_sets(q, np.zeros((2, 0), bool), [0, 1, 1, 0], 5, counters=True)
    assert ids0 == [] and r0.rung.shape == (4, 2)
    assert np.all(r0.rung == NONE) and np.all(r0.count == 0) and np.all(r0.pid == INVALID) and np.all(np.isposinf(r0.distance)) and np.all(r0.counters == 0)
    # no queries
    e = ph.search_allowed_sets(np.zeros((0, 5), np.float32), np.ones((2, 3), bool), np.zeros(0, np.int64), 2, counters=True)
    assert e.pid.shape == (0, 2) and e.distance.shape == (0, 2) and e.count.shape == (0,) and e.rung.shape == (0, 5) and e.counters.shape == (0, 3)
    assert ph.search_allowed(np.zeros((0, 5), np.float32), mask, 2).rung.shape == (0, 5)


# ---- 10. arguments -------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(eng):
    ida, kind = eng
    from instant_distance_amd import _capi

    rng = np.random.default_rng(1)
    pts = rng.random((50, 4), dtype=np.float32)
    mk = lambda rows, ef=10: ida.Hnsw.from_ordered_points(np.ascontiguousarray(rows), ida.Builder().ef_search(ef))   # noqa: E731
    h0, h1 = mk(pts[:21]), mk(pts[21:])
    ph = ida.PartitionedHnsw.from_hnsws([h0, h1])
    q, sets = pts[:3], np.ones((2, 50), bool)
    so = np.array([0, 1, 0])
    L = _capi.lib()
    bits = np.full((2, 2), 0xFFFFFFFF, np.uint32)
    pid, dist, cnt = np.zeros((3, 5), np.uint32), np.zeros((3, 5), np.float32), np.zeros(3, np.uint32)

    def status(n_sets, set_of, k=5, max_rungs=-1, queries=q, out=pid):
        return L.idist_partitioned_search_batch_allowed_sets(ph._h, None if queries is None else _capi.f32p(queries), 3, _capi.u32p(bits), n_sets,
                                                             None if set_of is None else _capi.u32p(np.asarray(set_of, np.uint32)), k, max_rungs,
                                                             None if out is None else _capi.u32p(out), _capi.f32p(dist), _capi.u32p(cnt), None, None)

    assert status(2, [0, 1, 0]) == 0 and np.all(cnt == 5)               # out_rung and out_counters may be NULL
    assert status(0, [0, 0, 0]) == 1                                    # no set
    assert status(2, None) == 1                                         # one set per query needs n_sets == nq
    assert status(2, [0, 1, 2]) == 1 and b"query 2" in L.idist_last_error()
    assert status(2, [0, 1, 0], k=0) == 1 and status(2, [0, 1, 0], k=11) == 1 and status(2, [0, 1, 0], max_rungs=-2) == 1
    assert status(2, [0, 1, 0], queries=None) == 1 and status(2, [0, 1, 0], out=None) == 1
    # the Python layer
    for k, max_rungs in ((0, -1), (11, -1), (5, -2)):
        with pytest.raises(ida.IdistError) as e:
            ph.search_allowed_sets(q, sets, so, k, max_rungs=max_rungs)
        assert e.value.status == 1
    with pytest.raises(IndexError):
        ph.search_allowed_sets(q, sets, [0, 1, 2], 5)                   # a set index out of range
    with pytest.raises(IndexError):
        ph.search_allowed_sets(q, [np.array([3, 50])], [0, 0, 0], 5)    # a global id out of range
    with pytest.raises(IndexError):
        ph.search_allowed(q, np.array([3, 50]), 5)
    with pytest.raises(ValueError):
        ph.search_allowed_sets(q, sets, None, 5)                        # 2 sets for 3 queries
    with pytest.raises(ValueError):
        ph.search_allowed_sets(q, sets, [0, 1], 5)                      # set_of: one entry per query
    with pytest.raises(ValueError):
        ph.search_allowed_sets(q, np.ones((2, 49), bool), so, 5)
    with pytest.raises(ValueError):
        ph.search_allowed_sets(q, np.zeros((2, 3), np.uint32), so, 5)   # a ready bitmap of the wrong width
    with pytest.raises(ValueError):
        ph.search_allowed(q, np.ones(49, bool), 5)
    with pytest.raises(TypeError):
        ph.search_allowed_sets(q, sets, np.array([0.0, 1.0, 0.0]), 5)
    with pytest.raises(TypeError):
        ph.search_allowed_sets(q[:, :3], sets, so, 5)
    assert np.all(ph.search_allowed_sets(q, sets, so, 10).count == 10)              # k == ef_search is legal
    assert np.all(ph.search_allowed_sets(q, bits, so, 5).count == 5)                # a ready uint32 bitmap (padding bits set)
    # the parts are compared again at every call
    h1.set_ef_search(50)
    with pytest.raises(ida.IdistError) as e:
        ph.search_allowed_sets(q, sets, so, 5)
    assert e.value.status == 1 and "part 1" in e.value.message


# ---- 11. two devices -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_devices_gpu(engine_loader, oracle):
    """parts alternating over devices 0 and 1: the parts away from the merge device answer into their own memory, peer copies
    follow; the expected arrays are those of the composition test"""
    ida = engine_loader("gpu")
    from instant_distance_amd import _capi

    if _capi.lib().device_count() < 2:
        pytest.skip("needs two GPUs")
    pts, q, b, cs, k = main_parts(oracle, "gpu", 3)
    hs = [ida.Hnsw.from_parts(c.pts, c.zero, c.layers, ida.Builder().ef_search(c.ef).device(p % 2)) for p, c in enumerate(cs)]
    ph = ida.PartitionedHnsw.from_hnsws(hs)
    masks = global_masks(pts, b, k)
    for max_rungs in (-1, 2, 0):
        set_of = (np.arange(len(q)) + max_rungs + 1) % 8
        check(ph.search_allowed_sets(q, masks, set_of, k, max_rungs=max_rungs, counters=True), expected(cs, b, masks, set_of, k, max_rungs),
              f"max_rungs {max_rungs}")
