"""Restricted search over a partitioned index measured on bench.py's C2 shape -> profiles/partitioned_allowed.json.
100k x 128-d rows of bench.py's generator, 10k queries, ef_search 100, k 10; the same points as P = 1, 2, 4, 8 parts, ALL on device 0,
host-pointer calls, best of the rounds.  Per P and allowed set one row:
  sets        one shared set at selectivity 0.5, 0.1 and 0.01; one "tenant" set confined to a single part (half of that part's points);
              16 mixed sets (1.0, 0.5, 0.1 and 0.01, four each), the queries spread evenly.
  reported    queries/s, the per-part rung histogram, recall@10 against the same call with max_rungs = 0, the slice + upload time
              (host time on the bitmaps), the merge kernel's time, and the ratio to `Hnsw.search_allowed_sets` on the unpartitioned
              index in the same run.
  overlap     P = 4: the wall time of the call next to the sum of the four parts' individual `Hnsw.search_allowed_sets` calls on their
              slices — whether the parts' ladders run side by side.
Nothing is asserted on these numbers.
usage: python scripts/partition_allowed_case.py [--out profiles/partitioned_allowed.json] [--rounds 3] [--parts 1,2,4,8]"""
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
from instant_distance_amd.dist import shard_range  # noqa: E402
from metric_case import SHAPES  # noqa: E402


def best_of(call, rounds):
    """best wall (ms) of `rounds` calls after a warm-up (staging grows), all walls, and the last result"""
    call()
    wall = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        r = call()
        wall.append((time.perf_counter() - t0) * 1e3)
    return min(wall), [round(x, 3) for x in wall], r


def to_ids(row_masks, ids, n):
    """sets given per caller's row -> per id of an index (ids[row] = the id the build gave the row)"""
    out = np.zeros((len(row_masks), n), bool)
    out[:, np.asarray(ids, dtype=np.int64)] = np.stack(row_masks)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partitioned_allowed.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parts", default="1,2,4,8")
    args = ap.parse_args()
    import torch

    torch.cuda.init()
    dev = torch.device("cuda", 0)
    n, dim = SHAPES["C2"]
    pts = np.ascontiguousarray(bench.synth(torch, n, dim, 123456789, dev).cpu().numpy())
    q = np.ascontiguousarray(bench.synth(torch, N_Q, dim, 123456790, dev).cpu().numpy())
    h, h_ids = ida.Builder().seed(1).ef_search(EF).build_hnsw(pts)
    s1 = ida.Search()
    rng = np.random.default_rng(5)
    zero = np.zeros(N_Q, np.uint32)
    shares = [1.0, 0.5, 0.1, 0.01] * 4
    shared = {f"random {p}": ([rng.random(n) < p], zero) for p in (0.5, 0.1, 0.01)}
    mixed = ([rng.random(n) < p if p < 1 else np.ones(n, bool) for p in shares], (np.arange(N_Q) % 16).astype(np.uint32))
    tenant_draw = rng.random(n) < 0.5
    doc = dict(probe="partitioned_allowed", commit=bench.source_stamp(), where="one MI355X, all parts on device 0",
               command="python scripts/partition_allowed_case.py --rounds %d --parts %s" % (args.rounds, args.parts),
               n=n, dim=dim, queries=N_Q, ef_search=EF, k=K, ladder=ladder(EF), rounds=args.rounds, rows=[])
    for P in [int(x) for x in args.parts.split(",")]:
        ph, g_ids = ida.PartitionedHnsw.build(pts, ida.Builder().seed(1).ef_search(EF), parts=P)
        base = [int(x) for x in ph._base]
        lo, hi = shard_range(n, P - 1, P)
        tenant = np.zeros(n, bool)
        tenant[lo:hi] = tenant_draw[lo:hi]                         # rows of the last part only
        cases = dict(shared)
        cases[f"tenant: half of part {P - 1}"] = ([tenant], zero)
        cases["16 mixed sets"] = mixed
        for name, (row_masks, set_of) in cases.items():
            bits_p = allowed_bitmaps(to_ids(row_masks, g_ids, n), n)
            bits_1 = allowed_bitmaps(to_ids(row_masks, h_ids, n), n)
            ms, walls, got = best_of(lambda: ph.search_allowed_sets(q, bits_p, set_of, K, counters=True), args.rounds)
            slice_ms, merge_ms = ph.last_allowed_slice_ms(), ph.last_merge_ms()
            truth = ph.search_allowed_sets(q, bits_p, set_of, K, max_rungs=0)
            ms_1, walls_1, got_1 = best_of(lambda: h.search_allowed_sets(q, bits_1, set_of, K, s1, counters=True), args.rounds)
            hist = [{int(a): int(b) for a, b in zip(*np.unique(got.rung[:, p], return_counts=True))} for p in range(P)]
            row = dict(parts=P, allowed_set=name, n_sets=len(row_masks), selectivity=[round(float(m.mean()), 5) for m in row_masks],
                       ms_per_batch=round(ms, 3), ms_per_batch_all=walls, queries_per_s=round(N_Q / (ms * 1e-3), 1),
                       rung_histogram_per_part=hist, recall_at_k=recall(got, truth), slice_and_upload_ms=round(slice_ms, 4),
                       merge_kernel_ms=round(merge_ms, 4), search_kernels_ms_last=[round(float(x), 4) for x in ph.last_search_kernel_ms()],
                       unpartitioned=dict(ms_per_batch=round(ms_1, 3), ms_per_batch_all=walls_1, queries_per_s=round(N_Q / (ms_1 * 1e-3), 1),
                                          rung_histogram={int(a): int(b) for a, b in zip(*np.unique(got_1.rung, return_counts=True))}),
                       partitioned_over_unpartitioned_ms=round(ms / ms_1, 3))
            if P == 4:                                             # do the parts' ladders overlap?
                each = []
                for p, part in enumerate(ph.parts):
                    sp = ida.Search()
                    local = allowed_bitmaps(to_ids(row_masks, g_ids, n)[:, base[p]: base[p + 1]], base[p + 1] - base[p])
                    each.append(best_of(lambda: part.search_allowed_sets(q, local, set_of, K, sp, counters=True), args.rounds)[0])
                row["parts_individual_calls_ms"] = [round(x, 3) for x in each]
                row["parts_individual_calls_ms_sum"] = round(sum(each), 3)
                row["call_over_sum_of_parts"] = round(ms / sum(each), 3)
            print(json.dumps(row), flush=True)
            doc["rows"].append(row)
        del ph
    with open(args.out, "w") as fo:
        json.dump(doc, fo, indent=1)
        fo.write("\n")


if __name__ == "__main__":
    main()
