"""Range search over a partitioned index measured on bench.py's C2 shape -> profiles/partitioned_range.json.
100k x 128-d rows of bench.py's generator, 10k queries, ef_search 100; the same points as P = 1, 2, 4, 8 parts, ALL on device 0,
host-pointer calls, best of the rounds, the fetch included.  Radii at the distance of the 1st, 100th and 10,000th neighbour (the
median over the batch of each query's k-th smallest squared distance, computed with torch).  Per P and radius one row:
  reported    queries/s, the number of results, the per-part rung histogram, recall against the same call with max_rungs = 0 (every
              part's exact scan: the ground truth), every part's last search-kernel time beside the time of the counts, prefix-sum and
              merge kernels.
  P = 1       beside `Hnsw.search_range` on the SAME index in the same run: the cost of the merge path itself.
Nothing is asserted on these numbers.  The file is rewritten after every row, so an interrupted run leaves the rows it finished.
usage: python scripts/partition_range_case.py [--out profiles/partitioned_range.json] [--rounds 3] [--parts 1,2,4,8]"""
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
from range_case import EF, MAX_TOTAL, N_Q, ladder, recall  # noqa: E402

NEIGHBOURS = (1, 100, 10_000)


def best_of(call, rounds):
    """best wall (ms) of `rounds` calls after a warm-up (staging grows), all walls, and the last result"""
    call()
    wall = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        r = call()
        wall.append((time.perf_counter() - t0) * 1e3)
    return min(wall), [round(x, 3) for x in wall], r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partitioned_range.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parts", default="1,2,4,8")
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
    doc = dict(probe="partitioned_range", commit=bench.source_stamp(), where="one MI355X, all parts on device 0",
               command="python scripts/partition_range_case.py --rounds %d --parts %s" % (args.rounds, args.parts),
               n=n, dim=dim, queries=N_Q, ef_search=EF, ladder=ladder(EF), rounds=args.rounds, rows=[])

    def save():
        with open(args.out, "w") as fo:
            json.dump(doc, fo, indent=1)
            fo.write("\n")

    for P in [int(x) for x in args.parts.split(",")]:
        ph, _ = ida.PartitionedHnsw.build(pts, ida.Builder().seed(1).ef_search(EF), parts=P)
        for k in NEIGHBOURS:
            r = radii[k]
            ms, walls, got = best_of(lambda: ph.search_range(q, r, max_total=MAX_TOTAL, counters=True), args.rounds)
            merge_ms, search_ms = ph.last_range_merge_ms(), [round(float(x), 4) for x in ph.last_search_kernel_ms()]
            ms_x, walls_x, truth = best_of(lambda: ph.search_range(q, r, max_rungs=0, max_total=MAX_TOTAL), args.rounds)
            hist = [{int(a): int(b) for a, b in zip(*np.unique(got.rung[:, p], return_counts=True))} for p in range(P)]
            row = dict(parts=P, radius_at_neighbour=k, radius=r, ms_per_batch=round(ms, 3), ms_per_batch_all=walls,
                       queries_per_s=round(N_Q / (ms * 1e-3), 1), results=int(got.lims[-1]), exact_results=int(truth.lims[-1]),
                       rung_histogram_per_part=hist, recall=recall(got, truth), search_kernels_ms_last=search_ms,
                       range_merge_kernels_ms=round(merge_ms, 4),
                       exact_only=dict(ms_per_batch=round(ms_x, 3), ms_per_batch_all=walls_x, range_merge_kernels_ms=round(ph.last_range_merge_ms(), 4)))
            if P == 1:                                                 # the same index through the single-index call
                s = ida.Search()
                ms_1, walls_1, got_1 = best_of(lambda: ph.parts[0].search_range(q, r, s, max_total=MAX_TOTAL, counters=True), args.rounds)
                same = bool(np.array_equal(got_1.lims, got.lims) and np.array_equal(got_1.pid, got.pid) and
                            np.array_equal(got_1.distance.view(np.uint32), got.distance.view(np.uint32)))
                row["single_index_call"] = dict(ms_per_batch=round(ms_1, 3), ms_per_batch_all=walls_1, queries_per_s=round(N_Q / (ms_1 * 1e-3), 1),
                                                same_answer=same)
                row["partitioned_over_single_ms"] = round(ms / ms_1, 3)
            print(json.dumps(row), flush=True)
            doc["rows"].append(row)
            save()
        del ph
    save()


if __name__ == "__main__":
    main()
