"""Restricted search measured on bench.py's C2 shape -> profiles/allowed_search.json.
100k x 128-d rows of bench.py's generator, 10k queries, ef_search 100, k 10; one index, one Search, host-pointer calls.
For random allowed sets of selectivity 1, 0.5, 0.1, 0.01 and 0.001 and for one correlated set (coordinate 0 above its 0.9
quantile) it records: queries/s of `search_allowed` (wall, best of the rounds), the rung histogram, recall@10 against the same call
with max_rungs = 0 (the exact scan of the allowed rows — the ground truth), the HIP-event time of the select, pending and scan + merge
kernels beside the rungs' search-kernel times (idist_search_ctx_kernel_times), and the same for the max_rungs = 0 call itself: where
the exact scan overtakes the ladder is read off the two columns.  Selectivity 1 is also set against plain `search_batch` on the
same batch (asserted: the same ids as its first k).
usage: python scripts/allowed_case.py [--out profiles/allowed_search.json] [--rounds 3]"""
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
from metric_case import SHAPES  # noqa: E402

N_Q, EF, K = 10_000, 100, 10


def ladder(ef):
    out = [ef]
    while out[-1] < ida.MAX_EF:
        out.append(min(4 * out[-1], ida.MAX_EF))
    return out


def timed(h, s, q, mask, max_rungs, rounds):
    """best wall of `rounds` calls, and the last call's result and kernel times"""
    h.search_allowed(q, mask, K, s, max_rungs=max_rungs)                         # warm-up: staging grows
    wall = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        r = h.search_allowed(q, mask, K, s, max_rungs=max_rungs, counters=True)
        wall.append((time.perf_counter() - t0) * 1e3)
    sel_ms, pend_ms, exact_ms = s.allowed_kernel_ms()
    hist = {int(a): int(b) for a, b in zip(*np.unique(r.rung, return_counts=True))}
    # the rungs this call launched: from the start rung to the last one any query was answered on (the whole permitted ladder
    # when queries fell through to the exact scan)
    E, n_a, n = ladder(EF), int(mask.sum()), len(mask)
    if max_rungs >= 0:
        E = E[:max_rungs]
    r0 = next((i for i, e in enumerate(E) if e * n_a >= K * n), None) if n_a > K else None
    ran = []
    if r0 is not None:
        on = [x for x in hist if x < ida.RUNG_NONE]
        last = len(E) - 1 if ida.RUNG_EXACT in hist else max(on)
        ran = E[r0: last + 1]
    search_ms = [float(x) for x in s.kernel_times_ms(len(ran))] if ran else []
    return r, dict(ms_per_batch=round(min(wall), 3), ms_per_batch_all=[round(x, 3) for x in wall], queries_per_s=round(len(q) / (min(wall) * 1e-3), 1),
                   rung_histogram=hist, rungs_launched_ef=ran, search_kernels_ms=[round(x, 4) for x in search_ms],
                   select_kernels_ms=round(sel_ms, 4), pending_kernels_ms=round(pend_ms, 4), scan_and_merge_ms=round(exact_ms, 4))


def recall(got, truth):
    hit = tot = 0
    for a, ca, b, cb in zip(got.pid, got.count, truth.pid, truth.count):
        hit += len(set(a[:ca].tolist()) & set(b[:cb].tolist()))
        tot += int(cb)
    return round(hit / tot, 5) if tot else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "allowed_search.json"))
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch

    torch.cuda.init()
    dev = torch.device("cuda", 0)
    n, dim = SHAPES["C2"]
    pts = np.ascontiguousarray(bench.synth(torch, n, dim, 123456789, dev).cpu().numpy())
    q = np.ascontiguousarray(bench.synth(torch, N_Q, dim, 123456790, dev).cpu().numpy())
    h, _ = ida.Builder().seed(1).ef_search(EF).build_hnsw(pts)
    pts = h.points                                                               # PointId order: masks are by PointId
    s, plain = ida.Search(), ida.Search()
    rng = np.random.default_rng(5)
    sets = [(f"random {p}", rng.random(n) < p if p < 1 else np.ones(n, bool)) for p in (1.0, 0.5, 0.1, 0.01, 0.001)]
    sets.append(("coordinate 0 above its 0.9 quantile", pts[:, 0] > np.quantile(pts[:, 0], 0.9)))
    doc = dict(probe="allowed_search", commit=bench.source_stamp(), where="one MI355X", command="python scripts/allowed_case.py --rounds %d" % args.rounds,   # (where the file is written is no part of the measurement)
               n=n, dim=dim, queries=N_Q, ef_search=EF, k=K, ladder=ladder(EF), rounds=args.rounds, rows=[])
    # plain search_batch on the same batch
    h.search_batch(q, plain)
    wall = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        base = h.search_batch(q, plain)
        wall.append((time.perf_counter() - t0) * 1e3)
    doc["search_batch"] = dict(ms_per_batch=round(min(wall), 3), ms_per_batch_all=[round(x, 3) for x in wall],
                               queries_per_s=round(N_Q / (min(wall) * 1e-3), 1), search_kernel_ms=round(float(plain.kernel_times_ms(1)[-1]), 4))
    for name, mask in sets:
        got, row = timed(h, s, q, mask, -1, args.rounds)
        truth, exact = timed(h, s, q, mask, 0, args.rounds)
        assert np.all(got.count == min(K, int(mask.sum()))) and np.all(truth.count == got.count)
        assert all(mask[got.pid[i, : got.count[i]]].all() for i in range(0, N_Q, 97))
        row.update(allowed_set=name, allowed_points=int(mask.sum()), selectivity=round(float(mask.mean()), 5), recall_at_k=recall(got, truth),
                   exact_only=exact, exact_over_ladder=round(exact["ms_per_batch"] / row["ms_per_batch"], 3))
        if mask.all():
            assert np.array_equal(got.pid, base.pid[:, :K]) and np.all(got.rung == 0)
            row["over_search_batch_ms"] = round(row["ms_per_batch"] - doc["search_batch"]["ms_per_batch"], 3)
            row["over_search_batch_share"] = round(row["ms_per_batch"] / doc["search_batch"]["ms_per_batch"] - 1.0, 4)
        print(json.dumps(row), flush=True)
        doc["rows"].append(row)
    with open(args.out, "w") as fo:
        json.dump(doc, fo, indent=1)
        fo.write("\n")


if __name__ == "__main__":
    main()
