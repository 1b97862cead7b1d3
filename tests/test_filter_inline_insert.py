"""The inlined thin walk inserts its new ids into the quotient set without testing for membership again (csrc/idist_device.hpp
q16_insert_new): its own lookup found them absent a moment ago and a row holds no id twice.  The principal walk
without the blocks (IDIST_FILTER_INLINE=0) still inserts through q16_insert: both are the oracle's — ids, order, counts, distance
bits, {n_dist, n_exp0, n_expU} — and the filter's counts are equal between them (`both` of test_filter_inline.py).  The cases press
on the insert with sets so small that buckets fill up in the middle of an expansion (the id goes to the bitmap from `mid`), that
lanes of one expansion contend for the same word (the compare-and-swap is tried again), and that later lookups answer "full"."""
import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params
from test_filter import ON_CHIP, S
from test_filter_inline import both, oracle_index
from test_filter_principal import points_and_queries


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    return engine_loader(request.param), request.param


# (dim, metric, IDIST_TAB_LOG2 on the emulator / the GPU): 300-d, 128-d and a runtime geometry; sets of 64 to 1024 quotients (2 << log2)
# against walks that compute several hundred (emulator) to a few thousand (GPU) distances
CASES = [(300, 0, (5, 5)), (300, 1, (7, 7)), (128, 0, (5, 5)), (128, 1, (7, 9)), (200, 0, (6, 7)), (300, 0, (6, 9))]


@pytest.mark.parametrize("dim,metric,log2s", CASES)
def test_small_sets_fill_up_during_an_expansion(eng, oracle, monkeypatch, dim, metric, log2s):
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    log2 = S(kind, *log2s)
    rng = np.random.default_rng(9800 + dim + metric + log2s[1])
    n, ef = S(kind, 700, 20000), S(kind, 40, 100)
    pts, q = points_and_queries(rng, "lowrank", n, S(kind, 12, 600), dim)
    q[0] = pts[n // 3]                                                   # a stored point
    oix, want = oracle_index(oracle, kind, pts, q, metric, ef)
    assert int(want.counters[:, 0].max()) > (2 << log2)                  # (n_dist = ids that were new to the visited set)
    h = ida.Hnsw.from_parts(pts, oix.zero, oix.layers, ida.Builder().metric(metric).ef_search(ef))
    (seen, rejected), _, (req, used) = both(ida, monkeypatch, h, q, want, env={**ON_CHIP, "IDIST_TAB_LOG2": str(log2)})
    assert seen > 0 and rejected > 0 and used > 0 and req >= used


def test_entry_expansion_inserts_a_full_row_at_once(eng, oracle, monkeypatch):
    """Forty points, complete zero rows: the entry point's expansion inserts 39 ids in one `mid`, into a set of 64 quotients: lanes
    contend for the same buckets and words in one pass."""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    rng = np.random.default_rng(9900)
    n, ef = 40, 12
    pts, q = points_and_queries(rng, "lowrank", n, S(kind, 12, 600), 300)
    oix, want = oracle_index(oracle, kind, pts, q, 0, ef)
    h = ida.Hnsw.from_parts(pts, oix.zero, oix.layers, ida.Builder().ef_search(ef))
    _, _, (req, _) = both(ida, monkeypatch, h, q, want, env={**ON_CHIP, "IDIST_TAB_LOG2": "5"})
    assert req > 0
