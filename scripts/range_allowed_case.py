"""Restricted range search measured on bench.py's C2 shape -> profiles/range_allowed_search.json.
100k x 128-d rows of bench.py's generator, 10k queries, ef_search 100, as scripts/range_case.py; one index, one Search, host-pointer
calls.  For allowed sets of 0.1 %, 1 %, 10 % and 100 % of the points (random ids, one set shared by the batch) and radii at the distance
of the 10th, 1000th and 10,000th neighbour (the median over the batch of each query's k-th smallest squared distance, computed with
torch) it records: queries/s of `search_range_allowed` (wall, best of the rounds, the fetch included), the queries answered per rung,
the number of results, recall against the same call with max_rungs = 0 (the exact scan of the set: the ground truth), and the HIP-event
times of the select, scan and sort kernels.  Beside them the way without the call: `search_range` on the same batch followed by a
numpy filter of its ids by the mask — wall time, and the max_total that call needs (its unrestricted total).  Ratios are reported, not
asserted.
usage: python scripts/range_allowed_case.py [--out profiles/range_allowed_search.json] [--rounds 2]"""
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
from instant_distance_amd.api import allowed_bitmap  # noqa: E402
from metric_case import SHAPES  # noqa: E402
from range_case import EF, MAX_TOTAL, N_Q, ladder, recall  # noqa: E402

SHARES = (0.001, 0.01, 0.1, 1.0)
NEIGHBOURS = (10, 1000, 10_000)


def timed(h, s, q, radius, bits, max_rungs, rounds):
    """best wall of `rounds` calls, and the last call's result and kernel times"""
    h.search_range_allowed(q, radius, bits, s, max_rungs=max_rungs, max_total=MAX_TOTAL)       # warm-up: staging grows
    wall = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        r = h.search_range_allowed(q, radius, bits, s, max_rungs=max_rungs, max_total=MAX_TOTAL, counters=True)
        wall.append((time.perf_counter() - t0) * 1e3)
    sel_ms, scan_ms, sort_ms = s.range_kernel_ms()
    hist = {int(a): int(b) for a, b in zip(*np.unique(r.rung, return_counts=True))}
    return r, dict(ms_per_batch=round(min(wall), 3), ms_per_batch_all=[round(x, 3) for x in wall], queries_per_s=round(len(q) / (min(wall) * 1e-3), 1),
                   results=int(r.lims[-1]), rung_histogram=hist, select_kernels_ms=round(sel_ms, 4), scan_kernels_ms=round(scan_ms, 4),
                   sort_kernels_ms=round(sort_ms, 4))


def range_then_filter(h, s, q, radius, mask, rounds):
    """the way without the call: search_range, then a host-side filter of its ids by the mask"""
    wall = []
    for _ in range(rounds + 1):                                        # (the first round warms the staging up)
        t0 = time.perf_counter()
        r = h.search_range(q, radius, s, max_total=MAX_TOTAL)
        keep = mask[r.pid]
        pid, dist = r.pid[keep], r.distance[keep]
        lims = np.concatenate([[0], np.cumsum(keep)])[r.lims.astype(np.int64)]
        wall.append((time.perf_counter() - t0) * 1e3)
    wall = wall[1:]
    return ida.RangeResult(lims.astype(np.uint64), pid, dist, r.rung, None), dict(
        ms_per_batch=round(min(wall), 3), ms_per_batch_all=[round(x, 3) for x in wall], max_total_needed=int(r.lims[-1]), results=int(lims[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_allowed_search.json"))
    ap.add_argument("--rounds", type=int, default=2)
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
    doc = dict(probe="range_allowed_search", commit=bench.source_stamp(), where="one MI355X",
               command="python scripts/range_allowed_case.py --rounds %d" % args.rounds, n=n, dim=dim, queries=N_Q, ef_search=EF,
               ladder=ladder(EF), rounds=args.rounds, rows=[])
    rng = np.random.default_rng(5)
    for k in NEIGHBOURS:
        for share in SHARES:
            mask = np.ones(n, bool) if share == 1.0 else rng.random(n) < share
            bits = allowed_bitmap(mask, n)[None, :]
            got, row = timed(h, s, q, radii[k], bits, -1, args.rounds)
            truth, exact = timed(h, s, q, radii[k], bits, 0, args.rounds)
            other, parent = range_then_filter(h, plain, q, radii[k], mask, args.rounds)
            row.update(share=share, allowed=int(mask.sum()), rungs_permitted=sum(e < 2 * int(mask.sum()) for e in ladder(EF)),
                       radius_at_neighbour=k, radius=radii[k], exact_results=int(truth.lims[-1]), recall=recall(got, truth),
                       exact_only=exact, search_range_then_filter=dict(parent, recall=recall(other, truth)),
                       wall_ratio_filter_over_call=round(parent["ms_per_batch"] / row["ms_per_batch"], 3))
            print(json.dumps(row), flush=True)
            doc["rows"].append(row)
            with open(args.out, "w") as fo:                            # (kept after every row: a long combination may be cut short)
                json.dump(doc, fo, indent=1)
                fo.write("\n")


if __name__ == "__main__":
    main()
