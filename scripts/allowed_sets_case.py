"""Restricted search with several allowed sets per call measured on bench.py's C2 shape ->
profiles/allowed_sets.json.  100k x 128-d rows of bench.py's generator, 10k queries, ef_search 100, k 10; one index, host-pointer
calls, best of the rounds.  Three questions:
  one_set      one set, everyone on it (random 0.5 and 0.1): `search_allowed_sets` beside `search_allowed` on the same batch in the
               same run — wall time and the HIP-event times of the select / pending / exact kernels and of the rungs' search kernels:
               what the count pass and the pending pass in front of the first launch cost.
  mixed        16 sets of mixed selectivity (1.0, 0.5, 0.1 and 0.01, four each), the 10k queries spread evenly, one call, against the
               only way to do this without it: 16 `search_allowed` calls on the 16 query groups.  Queries/s, rungs reached, recall@10
               against max_rungs = 0.  The ratio is reported, not asserted.
  exact_only   max_rungs = 0: the scan straight from the bitmap against the id-list scan of the single-set call on one shared set at
               selectivity 0.5 and 0.001 — where reading n / 8 bytes of bitmap per query could show.
Every row of the new call is asserted equal to the single-set call's (ids and rungs).
usage: python scripts/allowed_sets_case.py [--out profiles/allowed_sets.json] [--rounds 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
import instant_distance_amd as ida  # noqa: E402
from allowed_case import EF, K, N_Q, ladder, recall  # noqa: E402
from instant_distance_amd.api import allowed_bitmaps  # noqa: E402
from metric_case import SHAPES  # noqa: E402


def rungs_launched(masks, set_of, rung, max_rungs):
    """the rungs a call launched, from the definition: a query runs the rungs from its start rung to the one that answered it (to the
    end of the permitted ladder when the exact step answered it after the ladder)"""
    E = ladder(EF)
    E = E[:max_rungs] if max_rungs >= 0 else E
    ran = set()
    for si, mask in enumerate(masks):
        n_a, n = int(mask.sum()), len(mask)
        r0 = next((i for i, e in enumerate(E) if e * n_a >= K * n), None) if n_a > K else None
        if r0 is None:
            continue
        for a in np.unique(rung[set_of == si]).tolist():
            ran |= set(range(r0, (len(E) if a == ida.RUNG_EXACT else a + 1)))
    return [E[r] for r in sorted(ran)]


def measure(call, s, rounds, masks, set_of, max_rungs):
    """best wall of `rounds` calls (after a warm-up: staging grows), the last call's result and kernel times"""
    call()
    wall = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        r = call()
        wall.append((time.perf_counter() - t0) * 1e3)
    sel_ms, pend_ms, exact_ms = s.allowed_kernel_ms()
    ran = rungs_launched(masks, set_of, r.rung, max_rungs)
    search_ms = [float(x) for x in s.kernel_times_ms(len(ran))] if ran else []
    hist = {int(a): int(b) for a, b in zip(*np.unique(r.rung, return_counts=True))}
    return r, dict(ms_per_batch=round(min(wall), 3), ms_per_batch_all=[round(x, 3) for x in wall],
                   queries_per_s=round(len(r.rung) / (min(wall) * 1e-3), 1), rung_histogram=hist, rungs_launched_ef=ran,
                   search_kernels_ms=[round(x, 4) for x in search_ms], select_kernels_ms=round(sel_ms, 4),
                   pending_kernels_ms=round(pend_ms, 4), scan_and_merge_ms=round(exact_ms, 4))


def both(h, q, mask, max_rungs, rounds):
    """one shared set: the several-sets call and the single-set call, the same batch, the same run"""
    s_new, s_old = ida.Search(), ida.Search()
    zero = np.zeros(len(q), np.uint32)
    bits = allowed_bitmaps([mask], len(mask))
    a, new = measure(lambda: h.search_allowed_sets(q, bits, zero, K, s_new, max_rungs=max_rungs, counters=True), s_new, rounds, [mask], zero, max_rungs)
    b, old = measure(lambda: h.search_allowed(q, mask, K, s_old, max_rungs=max_rungs, counters=True), s_old, rounds, [mask], zero, max_rungs)
    assert np.array_equal(a.pid, b.pid) and np.array_equal(a.rung, b.rung) and np.array_equal(a.counters, b.counters)
    spread = max(max(new["ms_per_batch_all"]) - min(new["ms_per_batch_all"]), max(old["ms_per_batch_all"]) - min(old["ms_per_batch_all"]))
    return dict(allowed_points=int(mask.sum()), selectivity=round(float(mask.mean()), 5), search_allowed_sets=new, search_allowed=old,
                new_minus_old_ms=round(new["ms_per_batch"] - old["ms_per_batch"], 3), spread_of_the_repeats_ms=round(spread, 3),
                new_over_old=round(new["ms_per_batch"] / old["ms_per_batch"], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "allowed_sets.json"))
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch

    torch.cuda.init()
    dev = torch.device("cuda", 0)
    n, dim = SHAPES["C2"]
    pts = np.ascontiguousarray(bench.synth(torch, n, dim, 123456789, dev).cpu().numpy())
    q = np.ascontiguousarray(bench.synth(torch, N_Q, dim, 123456790, dev).cpu().numpy())
    h, _ = ida.Builder().seed(1).ef_search(EF).build_hnsw(pts)
    rng = np.random.default_rng(5)
    doc = dict(probe="allowed_sets", commit=bench.source_stamp(), where="one MI355X", command="python scripts/allowed_sets_case.py --rounds %d" % args.rounds,
               n=n, dim=dim, queries=N_Q, ef_search=EF, k=K, ladder=ladder(EF), rounds=args.rounds)
    # 1. one set, everyone on it
    doc["one_set"] = []
    for p in (0.5, 0.1):
        row = dict(allowed_set=f"random {p}", **both(h, q, rng.random(n) < p, -1, args.rounds))
        print(json.dumps(row), flush=True)
        doc["one_set"].append(row)
    # 2. 16 sets of mixed selectivity in one call / in 16 calls
    shares = [1.0, 0.5, 0.1, 0.01] * 4
    masks = [rng.random(n) < p if p < 1 else np.ones(n, bool) for p in shares]
    bits = allowed_bitmaps(masks, n)
    set_of = (np.arange(N_Q) % 16).astype(np.uint32)
    groups = [np.flatnonzero(set_of == si) for si in range(16)]
    qs = [np.ascontiguousarray(q[g]) for g in groups]
    s_new, s_old = ida.Search(), ida.Search()
    got, one_call = measure(lambda: h.search_allowed_sets(q, bits, set_of, K, s_new, counters=True), s_new, args.rounds, masks, set_of, -1)
    truth = h.search_allowed_sets(q, bits, set_of, K, s_new, max_rungs=0)

    def sixteen():
        return [h.search_allowed(qs[si], masks[si], K, s_old, counters=True) for si in range(16)]

    sixteen()
    wall = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        parts = sixteen()
        wall.append((time.perf_counter() - t0) * 1e3)
    for si, g in enumerate(groups):
        assert np.array_equal(got.pid[g], parts[si].pid) and np.array_equal(got.rung[g], parts[si].rung)
        assert np.array_equal(got.counters[g], parts[si].counters)
    assert np.all(truth.rung == ida.RUNG_EXACT) and np.array_equal(truth.count, got.count)
    doc["mixed"] = dict(sets=16, selectivities=shares, queries_per_set=[len(g) for g in groups], one_call=one_call, recall_at_k=recall(got, truth),
                        sixteen_calls=dict(ms_per_batch=round(min(wall), 3), ms_per_batch_all=[round(x, 3) for x in wall],
                                           queries_per_s=round(N_Q / (min(wall) * 1e-3), 1)),
                        one_call_over_sixteen_calls_queries_per_s=round(min(wall) / one_call["ms_per_batch"], 3))
    print(json.dumps(doc["mixed"]), flush=True)
    # 3. the exact step alone: the bitmap scan against the id-list scan
    doc["exact_only"] = []
    for p in (0.5, 0.001):
        row = dict(allowed_set=f"random {p}", **both(h, q, rng.random(n) < p, 0, args.rounds))
        print(json.dumps(row), flush=True)
        doc["exact_only"].append(row)
    with open(args.out, "w") as fo:
        json.dump(doc, fo, indent=1)
        fo.write("\n")


if __name__ == "__main__":
    main()
