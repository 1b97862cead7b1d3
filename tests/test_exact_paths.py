"""Every exact path is the oracle's brute force.

The exhaustive scan, the MFMA filter with its canonical re-rank, the exact steps of the restricted searches (one set, several sets)
and of the range search are each other's ground truth elsewhere in the suite and share their device routines (stage_query,
scan_rank_batch / topk_rank, topk_emit_row / topk_emit_list, scan_segment).  Here all of them answer the same small problem and are
compared with `oracle.bruteforce`, never with each other: ids with array_equal, distances as bit patterns.  Every case runs on the CPU
emulator and (-m gpu) on the MI355X."""
import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params

N, NQ = 197, 5                    # three full batches of 64 ids and a last one of 5
TWINS = (5, 100, 196)             # equal rows: three exact ties at distance 0 for query 0, in the first, second and last batch
EXACT = 255


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


@pytest.mark.parametrize("dim", [128, 300, 40])      # the <4,0,0> geometry, <9,1,1> with its tail, a runtime geometry
def test_every_exact_path_is_the_oracles_bruteforce(eng, oracle, monkeypatch, dim):
    ida, kind = eng
    rng = np.random.default_rng(dim)
    pts = rng.standard_normal((N, dim)).astype(np.float32)
    q = rng.standard_normal((NQ, dim)).astype(np.float32)
    pts[TWINS[1]] = pts[TWINS[2]] = q[0] = pts[TWINS[0]]
    pc.use_test_build(monkeypatch)                   # (IDIST_BRUTEFORCE / IDIST_BF_SAMPLE exist in the test build only)
    h = ida.Hnsw.from_parts(pts, np.full((N, 64), pc.INVALID, np.uint32), [], ida.Builder())
    ones = np.ones(N, bool)
    rng_res = h.search_range(q, np.inf, ida.Search(), max_rungs=0)
    assert np.array_equal(rng_res.lims, np.arange(NQ + 1, dtype=np.uint64) * N) and np.all(rng_res.rung == EXACT)
    for k in (1, 10, 70):
        op, od = oracle.bruteforce(pts, q, k)
        ob = pc.bits(od)
        assert op[0, :min(k, 3)].tolist() == list(TWINS[:k]) and not ob[0, :min(k, 3)].any()      # the ties, in id order

        def same(pid, dist, what):
            assert np.array_equal(pid, op), f"k {k}, {what}: ids"
            assert np.array_equal(pc.bits(dist), ob), f"k {k}, {what}: distance bits"

        monkeypatch.setenv("IDIST_BRUTEFORCE", "scan")
        same(*h.bruteforce(q, k), "scan")
        monkeypatch.setenv("IDIST_BRUTEFORCE", "mfma")
        monkeypatch.setenv("IDIST_BF_SAMPLE", "64")   # rerank_kernel and kth_threshold_kernel
        same(*h.bruteforce(q, k), "mfma")
        r = h.search_allowed(q, ones, k, ida.Search(), max_rungs=0)
        assert np.all(r.rung == EXACT) and np.all(r.count == k)
        same(r.pid, r.distance, "one allowed set")
        r = h.search_allowed_sets(q, np.ones((2, N), bool), np.arange(NQ) % 2, k, ida.Search(), max_rungs=0)
        assert np.all(r.rung == EXACT) and np.all(r.count == k)
        same(r.pid, r.distance, "two allowed sets")
        first = rng_res.lims[:-1, None].astype(np.int64) + np.arange(k)
        same(rng_res.pid[first], rng_res.distance[first], "range, radius inf")
