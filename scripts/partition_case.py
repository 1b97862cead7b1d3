"""Partitioned index on ONE GPU: the same points as P = 1, 2, 4, 8 parts, all on device 0.
Per P one JSON line: build seconds (sum over the parts, HIP events), search ms per 10k-query batch (wall, best of 3),
the merge kernel's time beside the floor it is measured against — the bytes it must move over the 8 TB/s spec — and
its share of the same call's search kernels, recall@10 against the partitioned exact search.
usage: python scripts/partition_case.py out.jsonl [C2|C3] [parts,parts,...]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import instant_distance_amd as ida  # noqa: E402

SHAPES = {"C2": (100_000, 128), "C3": (1_000_000, 300)}
HBM_BYTES_PER_S = 8e12


def synth(n, dim, seed, latent=32):
    """bench.synth's 'fastText-shape' rows on the host: z A + 0.05 noise, L2-normalised"""
    a = np.random.default_rng(4242).standard_normal((latent, dim)).astype(np.float32)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, latent)).astype(np.float32) @ a + np.float32(0.05) * rng.standard_normal((n, dim)).astype(np.float32)
    return np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True), dtype=np.float32)


def main():
    out, shape = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "C2")
    parts = [int(x) for x in (sys.argv[3] if len(sys.argv) > 3 else "1,2,4,8").split(",")]
    n, dim = SHAPES[shape]
    nq, ef, k = 10_000, 100, 10
    pts, q = synth(n, dim, 123456789), synth(nq, dim, 123456790)
    with open(out, "a") as fo:
        for P in parts:
            t0 = time.perf_counter()
            ph, _ = ida.PartitionedHnsw.build(pts, ida.Builder().seed(1).ef_search(ef), parts=P)
            build_wall = time.perf_counter() - t0
            build_s = sum(h.build_stats().seconds for h in ph.parts)
            ph.search_batch(q, counters=True)                          # warm-up: contexts grow, staging is allocated
            wall, merge, kern = [], [], []
            for _ in range(3):
                t0 = time.perf_counter()
                r = ph.search_batch(q, counters=True)
                wall.append((time.perf_counter() - t0) * 1e3)
                merge.append(ph.last_merge_ms())
                kern.append(float(ph.last_search_kernel_ms().sum()))
            exact, _ = ph.bruteforce(q[:1000], k)
            hit = sum(len(set(r.pid[i, :k].tolist()) & set(exact[i].tolist())) for i in range(len(exact)))
            merge_bytes = (P + 1) * nq * (ef * 8 + 4 + 12)           # lists in, result out: ids + distances, counts, counters
            floor_us = merge_bytes / HBM_BYTES_PER_S * 1e6
            i = int(np.argmin(wall))
            row = dict(probe="partitioned_index", commit=bench.source_stamp(), shape=shape, n=n, dim=dim, queries=nq, ef=ef, parts=P,
                       devices=1, build_seconds_sum=round(build_s, 3), build_wall_seconds=round(build_wall, 3),
                       search_ms_per_batch=round(min(wall), 3), search_kernels_ms_sum=round(kern[i], 3),
                       merge_ms=round(min(merge), 4), merge_bytes=merge_bytes, merge_floor_us=round(floor_us, 2),
                       merge_over_floor=round(min(merge) * 1e3 / floor_us, 1),
                       merge_share_of_search_kernels=round(min(merge) / kern[i], 5) if kern[i] > 0 else None,
                       recall_at_10=round(hit / (len(exact) * k), 4), recall_queries=len(exact),
                       checksum=int(r.pid.astype(np.int64).sum()))
            print(json.dumps(row), flush=True)
            fo.write(json.dumps(row) + "\n")
            fo.flush()
            del ph


if __name__ == "__main__":
    main()
