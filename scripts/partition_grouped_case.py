"""Grouped search over a partitioned index measured on bench.py's C2 shape -> profiles/partitioned_grouped.json.
100k x 128-d rows of bench.py's generator, 10k queries, ef_search 100, k 10; the same points as P = 1, 2, 4, 8 parts, ALL on device 0,
host-pointer calls, best of the rounds.  Per P and layout one row:
  layouts     own: every point its own group (g = global id); docs16: documents of 16 chunks dealt at random, so groups span parts.
  reported    the call's wall time, the parts' search kernels (their last launches), the grouped merge kernel, the per-part rung
              histogram and the group recall against the same call with max_rungs = 0.
  comparison  on `own` the answer is `search_match`'s (checked equal first), whose union step is merge_topk_kernel — code this change
              does not touch: `last_merge_ms` after `search_grouped` against the same reading after `search_match`, same process, same
              graph, same condition, alternating rounds; the median of each, their ratio and the spread of the per-round ratio.
Nothing is asserted on these numbers.
usage: python scripts/partition_grouped_case.py [--out profiles/partitioned_grouped.json] [--rounds 3] [--ab-rounds 9] [--parts 1,2,4,8]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
import instant_distance_amd as ida  # noqa: E402
from allowed_case import EF, K, N_Q, ladder  # noqa: E402
from metric_case import SHAPES  # noqa: E402
from partition_allowed_case import best_of  # noqa: E402


def group_recall(got, truth):
    """share of the true groups (max_rungs = 0) that the call returned, over all queries"""
    hit = sum(len(np.intersect1d(a[:c], b[:d])) for a, c, b, d in zip(got.group, got.count, truth.group, truth.count))
    return round(hit / max(int(truth.count.sum()), 1), 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partitioned_grouped.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ab-rounds", type=int, default=9)
    ap.add_argument("--parts", default="1,2,4,8")
    args = ap.parse_args()
    import torch

    torch.cuda.init()
    dev = torch.device("cuda", 0)
    n, dim = SHAPES["C2"]
    pts = np.ascontiguousarray(bench.synth(torch, n, dim, 123456789, dev).cpu().numpy())
    q = np.ascontiguousarray(bench.synth(torch, N_Q, dim, 123456790, dev).cpu().numpy())
    docs = (np.random.default_rng(5).permutation(n) // 16).astype(np.uint32)
    doc = dict(probe="partitioned_grouped", commit=bench.source_stamp(), where="one MI355X, all parts on device 0",
               command="python scripts/partition_grouped_case.py --rounds %d --ab-rounds %d --parts %s" % (args.rounds, args.ab_rounds, args.parts),
               n=n, dim=dim, queries=N_Q, ef_search=EF, k=K, ladder=ladder(EF), rounds=args.rounds, rows=[])
    for P in [int(x) for x in args.parts.split(",")]:
        ph, _ = ida.PartitionedHnsw.build(pts, ida.Builder().seed(1).ef_search(EF), parts=P)
        table = ph.attribute_table({"own": np.arange(n), "docs16": docs})
        for lay in ("own", "docs16"):
            ms, walls, got = best_of(lambda: ph.search_grouped(q, table, lay, K, counters=True), args.rounds)
            merge_ms, kernels = ph.last_merge_ms(), ph.last_search_kernel_ms()
            truth = ph.search_grouped(q, table, lay, K, max_rungs=0)
            hist = [{int(a): int(b) for a, b in zip(*np.unique(got.rung[:, p], return_counts=True))} for p in range(P)]
            row = dict(parts=P, layout=lay, ms_per_batch=round(ms, 3), ms_per_batch_all=walls, queries_per_s=round(N_Q / (ms * 1e-3), 1),
                       search_kernels_ms_last=[round(float(x), 4) for x in kernels], merge_kernel_ms=round(merge_ms, 4),
                       merge_share_of_call=round(merge_ms / ms, 5), rung_histogram_per_part=hist, group_recall=group_recall(got, truth))
            if lay == "own":                                       # the union steps side by side: grouped merge against merge_topk_kernel
                g, m = ph.search_grouped(q, table, lay, K, {}, counters=True), ph.search_match(q, table, {}, K, counters=True)
                assert all(np.array_equal(a, b) for a, b in ((g.pid, m.pid), (g.distance.view(np.uint32), m.distance.view(np.uint32)),
                                                              (g.count, m.count), (g.rung, m.rung), (g.counters, m.counters)))
                ab = []
                for _ in range(args.ab_rounds):
                    ph.search_grouped(q, table, lay, K, {}, counters=True)
                    a = ph.last_merge_ms()
                    ph.search_match(q, table, {}, K, counters=True)
                    ab.append((a, ph.last_merge_ms()))
                ratio = [a / b for a, b in ab]
                row["merge_ab"] = dict(rounds=args.ab_rounds, grouped_merge_ms=[round(a, 4) for a, _ in ab], merge_topk_ms=[round(b, 4) for _, b in ab],
                                       grouped_median_ms=round(float(np.median([a for a, _ in ab])), 4),
                                       merge_topk_median_ms=round(float(np.median([b for _, b in ab])), 4),
                                       ratio_of_medians=round(float(np.median([a for a, _ in ab]) / np.median([b for _, b in ab])), 3),
                                       per_round_ratio_min_max=[round(min(ratio), 3), round(max(ratio), 3)])
            print(json.dumps(row), flush=True)
            doc["rows"].append(row)
        del table, ph
    with open(args.out, "w") as fo:
        json.dump(doc, fo, indent=1)
        fo.write("\n")


if __name__ == "__main__":
    main()
