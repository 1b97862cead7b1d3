"""Range search measured on bench.py's C2 shape -> profiles/range_search.json.
100k x 128-d rows of bench.py's generator, 10k queries, ef_search 100; one index, one Search, host-pointer calls.
For radii at the distance of the 1st, 10th, 100th, 1000th and 10,000th neighbour (the median over the batch of each query's k-th
smallest squared distance, computed with torch) it records: queries/s of `search_range` (wall, best of the rounds, the fetch
included), the queries answered per rung, the number of results, recall against the same call with max_rungs = 0 (the exact scan: the
ground truth), the HIP-event time of the select, scan and sort kernels beside the rungs' search-kernel times, and the same for the
max_rungs = 0 call itself.  At the smallest radius, where every query is answered on rung 0, the wall time and the added kernel time
are set beside plain `search_batch` on the same batch; the yardstick is section 4.8's 0.034 ms of select and pending passes beside a
3.47-ms search kernel.  Ratios are reported, not asserted.
usage: python scripts/range_case.py [--out profiles/range_search.json] [--rounds 3]"""
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

N_Q, EF = 10_000, 100
NEIGHBOURS = (1, 10, 100, 1000, 10_000)
MAX_TOTAL = 1 << 28


def ladder(ef):
    out = [ef]
    while out[-1] < ida.MAX_EF:
        out.append(min(4 * out[-1], ida.MAX_EF))
    return out


def timed(h, s, q, radius, max_rungs, rounds):
    """best wall of `rounds` calls, and the last call's result and kernel times"""
    h.search_range(q, radius, s, max_rungs=max_rungs, max_total=MAX_TOTAL)       # warm-up: staging grows
    wall = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        r = h.search_range(q, radius, s, max_rungs=max_rungs, max_total=MAX_TOTAL, counters=True)
        wall.append((time.perf_counter() - t0) * 1e3)
    sel_ms, scan_ms, sort_ms = s.range_kernel_ms()
    hist = {int(a): int(b) for a, b in zip(*np.unique(r.rung, return_counts=True))}
    E = ladder(EF)
    if max_rungs >= 0:
        E = E[:max_rungs]
    on = [x for x in hist if x < ida.RUNG_NONE]
    last = len(E) - 1 if ida.RUNG_EXACT in hist else (max(on) if on else -1)
    ran = E[: last + 1]
    search_ms = [float(x) for x in s.kernel_times_ms(len(ran))] if ran else []
    return r, dict(ms_per_batch=round(min(wall), 3), ms_per_batch_all=[round(x, 3) for x in wall], queries_per_s=round(len(q) / (min(wall) * 1e-3), 1),
                   results=int(r.lims[-1]), rung_histogram=hist, rungs_launched_ef=ran, search_kernels_ms=[round(x, 4) for x in search_ms],
                   select_kernels_ms=round(sel_ms, 4), scan_kernels_ms=round(scan_ms, 4), sort_kernels_ms=round(sort_ms, 4))


def recall(got, truth):
    hit = tot = 0
    for i in range(len(got.lims) - 1):
        a = got.pid[int(got.lims[i]):int(got.lims[i + 1])]
        b = truth.pid[int(truth.lims[i]):int(truth.lims[i + 1])]
        hit += len(np.intersect1d(a, b, assume_unique=True))
        tot += len(b)
    return round(hit / tot, 5) if tot else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_search.json"))
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch

    torch.cuda.init()
    dev = torch.device("cuda", 0)
    n, dim = SHAPES["C2"]
    pts_t = bench.synth(torch, n, dim, 123456789, dev)
    q_t = bench.synth(torch, N_Q, dim, 123456790, dev)
    d2 = torch.cdist(q_t, pts_t).pow(2)
    radii = {k: float(d2.kthvalue(k, dim=1).values.median().item()) for k in NEIGHBOURS}
    del d2
    pts, q = np.ascontiguousarray(pts_t.cpu().numpy()), np.ascontiguousarray(q_t.cpu().numpy())
    h, _ = ida.Builder().seed(1).ef_search(EF).build_hnsw(pts)
    s, plain = ida.Search(), ida.Search()
    doc = dict(probe="range_search", commit=bench.source_stamp(), where="one MI355X", command="python scripts/range_case.py --rounds %d" % args.rounds,
               n=n, dim=dim, queries=N_Q, ef_search=EF, ladder=ladder(EF), rounds=args.rounds, rows=[])
    h.search_batch(q, plain)
    wall = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        h.search_batch(q, plain)
        wall.append((time.perf_counter() - t0) * 1e3)
    doc["search_batch"] = dict(ms_per_batch=round(min(wall), 3), ms_per_batch_all=[round(x, 3) for x in wall],
                               queries_per_s=round(N_Q / (min(wall) * 1e-3), 1), search_kernel_ms=round(float(plain.kernel_times_ms(1)[-1]), 4))
    for k in NEIGHBOURS:
        got, row = timed(h, s, q, radii[k], -1, args.rounds)
        truth, exact = timed(h, s, q, radii[k], 0, args.rounds)
        row.update(radius_at_neighbour=k, radius=radii[k], exact_results=int(truth.lims[-1]), recall=recall(got, truth), exact_only=exact)
        if set(row["rung_histogram"]) == {0}:
            base = doc["search_batch"]
            added = row["select_kernels_ms"]
            row["beside_search_batch"] = dict(wall_ms=row["ms_per_batch"], search_batch_wall_ms=base["ms_per_batch"],
                                              wall_ratio=round(row["ms_per_batch"] / base["ms_per_batch"], 4), added_kernels_ms=added,
                                              added_over_search_kernel=round(added / base["search_kernel_ms"], 4),
                                              yardstick="section 4.8: 0.034 ms beside a 3.47-ms search kernel")
        print(json.dumps(row), flush=True)
        doc["rows"].append(row)
    with open(args.out, "w") as fo:
        json.dump(doc, fo, indent=1)
        fo.write("\n")


if __name__ == "__main__":
    main()
