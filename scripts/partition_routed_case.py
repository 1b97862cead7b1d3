"""Routed search over a partitioned index -> profiles/partitioned_routed.json.
bench.py's C2 (100k x 128-d) and C3 (1M x 300-d) shapes, P = 8 parts ALL on device 0, 10k queries, ef_search 100, on bench.py's
generator and on uniform rows (a gain must not be an artefact of clustered synthetic rows).  Per shape and data set: range parts
against k-means parts, each through search_batch (every part) and nprobe = 1, 2, 4, 8.  Per row: recall@10 against
PartitionedHnsw.bruteforce, the call's best wall time, the parts' search kernels summed, the route kernels; per k-means build the
time of one iteration (assign + update, rows resident: idist_kmeans with i and with 0 iterations, divided) beside the floor of one
pass over the rows at 8 TB/s.  Nothing is asserted on these numbers.
usage: python scripts/partition_routed_case.py [--out profiles/partitioned_routed.json] [--rounds 3] [--shapes C2,C3]"""
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
from allowed_case import EF, K, N_Q  # noqa: E402
from metric_case import SHAPES  # noqa: E402
from partition_allowed_case import best_of  # noqa: E402

P, ITERS = 8, 10


def recall(got, truth):
    return round(float(np.mean([len(np.intersect1d(a[:K], b)) / K for a, b in zip(got.pid, truth)])), 5)


def kmeans_ms_per_iteration(pts):
    def wall(iters):
        t0 = time.perf_counter()
        run = ida.kmeans(pts, P, iters, return_iters=True)[3]
        return (time.perf_counter() - t0) * 1e3, run
    wall(0)
    (t0, _), (t1, run) = wall(0), wall(ITERS)
    return dict(iterations_run=run, ms_per_iteration=round((t1 - t0) / max(run, 1), 3), floor_ms_one_pass_at_8TBs=round(pts.nbytes / 8e12 * 1e3, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partitioned_routed.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="C2,C3")
    args = ap.parse_args()
    import torch

    torch.cuda.init()
    dev = torch.device("cuda", 0)
    doc = dict(probe="partitioned_routed", commit=bench.source_stamp(), where="one MI355X, all parts on device 0",
               command="python scripts/partition_routed_case.py --rounds %d --shapes %s" % (args.rounds, args.shapes),
               parts=P, queries=N_Q, ef_search=EF, recall_at=K, kmeans_iters=ITERS, rounds=args.rounds, rows=[], kmeans=[])
    for shape in args.shapes.split(","):
        n, dim = SHAPES[shape]
        for data in ("bench", "uniform"):
            if data == "bench":
                pts = np.ascontiguousarray(bench.synth(torch, n, dim, 123456789, dev).cpu().numpy())
                q = np.ascontiguousarray(bench.synth(torch, N_Q, dim, 123456790, dev).cpu().numpy())
            else:
                rng = np.random.default_rng(11)
                pts, q = rng.random((n, dim), dtype=np.float32), rng.random((N_Q, dim), dtype=np.float32)
            km = dict(shape=shape, data=data, **kmeans_ms_per_iteration(pts))
            print(json.dumps(km), flush=True)
            doc["kmeans"].append(km)
            for partition in ("ranges", "kmeans"):
                ph, ids = ida.PartitionedHnsw.build(pts, ida.Builder().seed(1).ef_search(EF), parts=P, partition=partition, kmeans_iters=ITERS)
                if partition == "ranges":                          # range parts have centroids too: the means of their rows
                    sizes = np.diff(ph._base)
                    ph.set_centroids(np.stack([pts[int(a):int(a) + int(m)].mean(axis=0) for a, m in zip(ph._base[:-1], sizes)]))
                truth = ph.bruteforce(q, K)[0]
                for nprobe in (None, 1, 2, 4, 8):
                    ms, walls, got = best_of(lambda: ph.search_batch(q, nprobe=nprobe), args.rounds)
                    kernels = ph.last_search_kernel_ms()
                    row = dict(shape=shape, data=data, partition=partition, nprobe=nprobe, part_sizes=[int(x) for x in np.diff(ph._base)],
                               recall=recall(got, truth), ms_per_batch=round(ms, 3), ms_per_batch_all=walls,
                               search_kernels_ms_sum=round(float(kernels[kernels > 0].sum()), 3),
                               route_ms=round(ph.last_route_ms(), 4) if nprobe else None)
                    print(json.dumps(row), flush=True)
                    doc["rows"].append(row)
                del ph
    with open(args.out, "w") as fo:
        json.dump(doc, fo, indent=1)
        fo.write("\n")


if __name__ == "__main__":
    main()
