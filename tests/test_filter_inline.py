"""The reject filter's third table (csrc/idist_capi.hip filter_inline_ensure): the 64-byte principal rows of a node's
neighbours stored once more with its adjacency, one 4-KB block per point, so that a thin principal walk has the compact rows of an
expansion with the candidate's id.  The blocks are byte copies of the principal rows: with them (IDIST_FILTER_INLINE=1) and without
(=0, the test build's A/B knob) ids, order, counts, distance bits and {n_dist, n_exp0, n_expU} are the oracle's, and the filter's own
counts — what it examined, what it rejected, on which rows — are equal between the two."""
import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params
from test_filter import ON_CHIP, S
from test_filter_principal import check, data, points_and_queries

BLOCK = 4096


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    return engine_loader(request.param), request.param


def search(ida, monkeypatch, h, q, inline, env=ON_CHIP, basis="principal", call=None):
    """One batch through a fresh Search (the knobs are sampled per context): the answer and the filter's three pairs of counts."""
    with pc.search_variant(env), monkeypatch.context() as m:
        m.setenv("IDIST_FILTER_INLINE", inline)
        if basis:
            m.setenv("IDIST_FILTER_BASIS", basis)
        else:
            m.delenv("IDIST_FILTER_BASIS", raising=False)
        srch = ida.Search()
        got = call(srch) if call else h.search_batch(q, srch, counters=True)
        return got, srch.filter_counts(), srch.filter_principal_counts(), srch.filter_inline_counts()


def both(ida, monkeypatch, h, q, want, nonfinite=False, **kw):
    """The batch with the blocks and without: each the oracle's, the filter's counts equal; returns (counts, principal share, blocks)."""
    got1, c1, p1, b1 = search(ida, monkeypatch, h, q, "1", **kw)
    got0, c0, p0, b0 = search(ida, monkeypatch, h, q, "0", **kw)
    check(got1, want, nonfinite)
    check(got0, want, nonfinite)
    assert c1 == c0 and p1 == p0, (c1, c0, p1, p0)
    assert b0 == (0, 0) and b1[1] <= b1[0], (b0, b1)
    return c1, p1, b1


def oracle_index(oracle, kind, pts, q, metric, ef):
    cfg = oracle.default_config(metric=metric, ef_search=ef, ef_construction=S(kind, 16, 100))
    oix = oracle.Index.build(pts, cfg, threads=S(kind, 1, 8))
    return oix, oix.search(q, threads=S(kind, 1, 8))


# (dim, metric, ef on the emulator / the GPU): 300-d, 128-d and a runtime geometry, squared L2 and L2, ef 12 and 100
CASES = [(d, m, (12, 100)) for d in (300, 128, 200) for m in (0, 1)] + [(300, 0, (100, 12))]


@pytest.mark.parametrize("dim,metric,efs", CASES)
def test_same_answers_and_counts_with_and_without_the_blocks(eng, oracle, monkeypatch, dim, metric, efs):
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    rng = np.random.default_rng(7000 + dim + metric + efs[0])
    n, ef = S(kind, 260, 20000), S(kind, *efs)
    pts, q = points_and_queries(rng, "lowrank", n, S(kind, 12, 600), dim)
    q[0] = pts[n // 2]                                                  # a stored point
    oix, want = oracle_index(oracle, kind, pts, q, metric, ef)
    h = ida.Hnsw.from_parts(pts, oix.zero, oix.layers, ida.Builder().metric(metric).ef_search(ef))
    (seen, rejected), (p_seen, _), (req, used) = both(ida, monkeypatch, h, q, want)
    assert h.info().filter_inline_bytes == n * BLOCK and h.info().filter_principal_bytes == n * 64
    assert p_seen > 0 and rejected > 0 and used > 0
    # every zero-layer expansion of a principal walk has its block requested at most twice (on demand, and as a wrong guess' neighbour)
    assert used <= int(want.counters[:, 1].sum()) and req <= 2 * int(want.counters[:, 1].sum()) + len(q)


def test_forty_points(eng, oracle, monkeypatch):
    """Every zero row has an INVALID tail — the blocks' zero slots — and there are fewer rows than basis directions."""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    rng = np.random.default_rng(7100)
    n, ef = 40, 12
    pts, q = points_and_queries(rng, "lowrank", n, S(kind, 12, 600), 300)
    oix, want = oracle_index(oracle, kind, pts, q, 1, ef)
    assert np.all(oix.zero[:, -1] == pc.INVALID)
    h = ida.Hnsw.from_parts(pts, oix.zero, oix.layers, ida.Builder().metric(1).ef_search(ef))
    _, _, (req, _) = both(ida, monkeypatch, h, q, want)
    assert req > 0 and h.info().filter_inline_bytes == n * BLOCK


def test_short_rows(eng, oracle, monkeypatch):
    """An imported graph whose zero rows hold 1-5 links: 59-63 zero slots per block."""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    rng = np.random.default_rng(7200)
    n, ef = S(kind, 260, 20000), S(kind, 12, 100)
    pts, q = points_and_queries(rng, "lowrank", n, S(kind, 12, 600), 300)
    cfg = oracle.default_config(ef_search=ef, ef_construction=S(kind, 16, 100))
    zero = oracle.Index.build(pts, cfg, threads=S(kind, 1, 8)).zero
    keep = 1 + np.arange(n) % 5
    zero[np.arange(64)[None, :] >= keep[:, None]] = pc.INVALID
    oix = oracle.Index.from_arrays(pts, zero, [], cfg)
    want = oix.search(q, threads=S(kind, 1, 8))
    h = ida.Hnsw.from_parts(pts, zero, [], ida.Builder().ef_search(ef))
    _, _, (req, _) = both(ida, monkeypatch, h, q, want)
    assert req > 0


def test_nearest_never_fills(eng, oracle, monkeypatch):
    """ef_search above n: the zero layer's `nearest` never fills, its blocks are requested and never tested."""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    rng = np.random.default_rng(7300)
    n = S(kind, 60, 200)
    ef = n + 40
    pts, q = points_and_queries(rng, "lowrank", n, S(kind, 12, 600), 128)
    oix, want = oracle_index(oracle, kind, pts, q, 0, ef)
    h = ida.Hnsw.from_parts(pts, oix.zero, oix.layers, ida.Builder().ef_search(ef))
    _, _, (req, used) = both(ida, monkeypatch, h, q, want)
    assert used == 0 and req > 0                                         # (the upper layers, ef = 1, are filtered as ever: rows, not blocks)


def test_queries_inside_and_outside_the_basis_in_one_launch(eng, oracle, monkeypatch):
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    rng = np.random.default_rng(7400)
    n, ef = S(kind, 260, 20000), S(kind, 12, 100)
    pts, q = points_and_queries(rng, "lowrank", n, S(kind, 12, 600), 300)
    q[1::2] = pc.gen_points(rng, len(q[1::2]), 300, "lowrank")           # (a second draw: another subspace than the rows')
    oix, want = oracle_index(oracle, kind, pts, q, 0, ef)
    h = ida.Hnsw.from_parts(pts, oix.zero, oix.layers, ida.Builder().ef_search(ef))
    (seen, _), (p_seen, _), (_, used) = both(ida, monkeypatch, h, q, want)
    assert 0 < p_seen < seen and used > 0                                # both tables served, the identity rows as before


def test_overflowing_quotient_set(eng, oracle, monkeypatch):
    """IDIST_TAB_LOG2=7: a set of 256 quotients.  A walk that computed more distances than that sent ids to the bitmap, whose answers
    arrive late: those ids take their verdicts from the same block in a second pass."""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    rng = np.random.default_rng(7500)
    n, ef = S(kind, 700, 20000), S(kind, 40, 100)
    pts, q = points_and_queries(rng, "lowrank", n, S(kind, 12, 600), 300)
    oix, want = oracle_index(oracle, kind, pts, q, 0, ef)
    assert int(want.counters[:, 0].max()) > 256                          # (n_dist = ids that were new to the visited set)
    h = ida.Hnsw.from_parts(pts, oix.zero, oix.layers, ida.Builder().ef_search(ef))
    _, _, (_, used) = both(ida, monkeypatch, h, q, want, env={**ON_CHIP, "IDIST_TAB_LOG2": "7"})
    assert used > 0


@pytest.mark.parametrize("kind_,dim", [("nonfinite", 300), ("constant", 128)])
def test_degenerate_rows(eng, oracle, monkeypatch, kind_, dim):
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    rng = np.random.default_rng(7600 + dim)
    n, ef = S(kind, 260, 20000), S(kind, 12, 100)
    a = data(rng, kind_, n + S(kind, 12, 600), dim)
    pts, q = np.ascontiguousarray(a[:n]), np.ascontiguousarray(a[n:])
    oix, want = oracle_index(oracle, kind, pts, q, 0, ef)
    h = ida.Hnsw.from_parts(pts, oix.zero, oix.layers, ida.Builder().ef_search(ef))
    if kind_ == "nonfinite":
        # (NaN distances all tie: a walk whose tie region overflows is run again, and the filter's counts include the abandoned
        #  pass — the same one either way)
        both(ida, monkeypatch, h, q, want, nonfinite=True)
    else:
        (_, rejected), _, _ = both(ida, monkeypatch, h, q, want)
        assert rejected == 0                                             # every distance is 0


def test_info(eng, oracle, monkeypatch):
    """filter_inline_bytes: n * 4096 where the principal format is in force by the index's own policy, 0 everywhere else."""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    rng = np.random.default_rng(7700)
    n = S(kind, 300, 20000)
    empty = lambda rows: np.full((rows, 64), pc.INVALID, dtype=np.uint32)   # noqa: E731  (format and policy need no graph)

    def after_a_search(pts, metric=0, inline="1"):
        h = ida.Hnsw.from_parts(pts, empty(len(pts)), [], ida.Builder().metric(metric).ef_search(20))
        assert h.info().filter_inline_bytes == 0                         # made on first use
        q = pts[:: max(1, len(pts) // 8)][:8].copy()
        _, _, _, blocks = search(ida, monkeypatch, h, q, inline, basis=None)
        return h.info(), blocks

    low = pc.gen_points(rng, n, 300, "lowrank")
    info, blocks = after_a_search(low)
    assert info.filter_format == 2 and info.filter_inline_bytes == n * BLOCK and blocks[0] > 0
    info, blocks = after_a_search(low, inline="0")                       # (the knob: no table is made for a walk that will not read it)
    assert info.filter_format == 2 and info.filter_inline_bytes == 0 and blocks == (0, 0)
    for pts, metric in ((pc.gen_points(rng, n, 300, "uniform"), 0),      # the policy takes the identity rows
                        (low, ida.METRIC_DOT),                           # no principal format
                        (pc.gen_points(rng, S(kind, 120, 3000), 768, "lowrank"), 0)):   # the fat walk
        info, blocks = after_a_search(pts, metric)
        assert info.filter_inline_bytes == 0 and blocks == (0, 0), (pts.shape, metric)
    # above the cap the index runs as it did before: not an error
    monkeypatch.setenv("IDIST_FILTER_INLINE_CAP", str(n * BLOCK - 1))
    info, blocks = after_a_search(low)
    assert info.filter_format == 2 and info.filter_principal_bytes == n * 64 and info.filter_inline_bytes == 0 and blocks == (0, 0)
    monkeypatch.setenv("IDIST_FILTER_INLINE_CAP", str(n * BLOCK))
    assert after_a_search(low)[0].filter_inline_bytes == n * BLOCK


def test_other_entry_points(eng, oracle, monkeypatch):
    """The restricted, the range and the partitioned search, and a replica: the same answers with the blocks as without."""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    rng = np.random.default_rng(7800)
    n, ef = S(kind, 260, 20000), S(kind, 12, 100)
    pts, q = points_and_queries(rng, "lowrank", n, S(kind, 12, 600), 300)
    oix, want = oracle_index(oracle, kind, pts, q, 1, ef)
    h = ida.Hnsw.from_parts(pts, oix.zero, oix.layers, ida.Builder().metric(1).ef_search(ef))
    both(ida, monkeypatch, h, q, want)                                   # (makes the table)
    allowed = rng.random(n) < 0.5
    radius = float(np.median(want.dist[:, min(ef, 8) - 1]))

    def fields(r):
        return [np.asarray(v) for v in vars(r).values() if v is not None]

    for call in (lambda s: h.search_allowed(q, allowed, 5, s, counters=True),
                 lambda s: h.search_range(q, radius, s, counters=True)):
        with_, without = (search(ida, monkeypatch, h, q, v, call=call)[0] for v in ("1", "0"))
        for a, b in zip(fields(with_), fields(without)):
            assert np.array_equal(a, b, equal_nan=True)
    # a replica makes its own table
    rep = h.replicate([0])[0]
    got, _, _, (req, used) = search(ida, monkeypatch, rep, q, "1")
    check(got, want)
    assert rep.info().filter_inline_bytes == n * BLOCK and used > 0
    # two parts behind one call (their contexts are the partitioned index's own: one index per setting)
    half = n // 2
    parts = []
    for lo, hi in ((0, half), (half, n)):
        o, _ = oracle_index(oracle, kind, pts[lo:hi], q, 1, ef)
        parts.append((pts[lo:hi], o.zero, o.layers))
    out = []
    for v in ("1", "0"):
        with pc.search_variant(ON_CHIP), monkeypatch.context() as m:
            m.setenv("IDIST_FILTER_INLINE", v)
            m.setenv("IDIST_FILTER_BASIS", "principal")
            hs = [ida.Hnsw.from_parts(p, z, l, ida.Builder().metric(1).ef_search(ef)) for p, z, l in parts]
            ph = ida.PartitionedHnsw.from_hnsws(hs)
            out.append(ph.search_batch(q, counters=True))
            assert all(x.info().filter_inline_bytes == (len(x.points) * BLOCK if v == "1" else 0) for x in hs)
    for a, b in zip(fields(out[0]), fields(out[1])):
        assert np.array_equal(a, b, equal_nan=True)
