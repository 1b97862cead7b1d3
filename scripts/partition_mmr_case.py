"""Diverse search over a partitioned index measured on bench.py's C2 rows (100k x 128-d) ->
profiles/partitioned_mmr.json.  P = 1, 2, 4, 8 range parts on one GPU, 10k queries, ef_search 100, k 10, lam 0.5, fetch 32 / 64 / 100,
both selection kernels (IDIST_MMR=tile|global, a knob of the test build: everything runs through libidist_variants.so), alternately
call by call.  Per configuration three times, the best of the rounds and every round's reading: the pool kernels (lists + row
gathers), the selection kernel (both HIP events, `PartitionedHnsw.last_mmr_ms`) and the whole call (wall).  Beside them
  1. the only way without the call: `PartitionedHnsw.search_batch`, a numpy gather of fetch rows per query from the caller's rows in
     global-id order and mmr_case.py's greedy loop (timed on a slice of the queries and scaled; the file says so);
  2. at P = 1, `Hnsw.search_mmr` on the same part with the same kernel: the pool indirection against direct rows.
Nothing here is a bar: the comparison at P = 1 and the gather's share of the call are what the file is for.
usage: python scripts/partition_mmr_case.py [--out profiles/partitioned_mmr.json] [--rounds 3] [--parts 1,2,4,8] [--host-queries 500]"""
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
from attr_case import best  # noqa: E402
from instant_distance_amd import _capi  # noqa: E402
from metric_case import SHAPES  # noqa: E402
from mmr_case import FETCH, KNOBS, LAM, host_mmr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partitioned_mmr.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parts", default="1,2,4,8")
    ap.add_argument("--host-queries", type=int, default=500)
    args = ap.parse_args()
    import torch

    torch.cuda.init()
    dev = torch.device("cuda", 0)
    test_lib = _capi.Lib(os.path.join(os.path.dirname(_capi.LIB_PATH), "libidist_variants.so"))
    n, dim = SHAPES["C2"]
    pts = np.ascontiguousarray(bench.synth(torch, n, dim, 123456789, dev).cpu().numpy())
    q = np.ascontiguousarray(bench.synth(torch, N_Q, dim, 123456790, dev).cpu().numpy())
    doc = dict(probe="partitioned_mmr", where="one MI355X", shape="C2", n=n, dim=dim, queries=N_Q, ef_search=EF, k=K, lam=LAM,
               commit=bench.source_stamp(), rounds=args.rounds, host_baseline_queries=args.host_queries,
               command="python scripts/partition_mmr_case.py --rounds %d --parts %s" % (args.rounds, args.parts), parts=[])
    for P in [int(x) for x in args.parts.split(",")]:
        with _capi._using(test_lib):                       # everything of this P belongs to the test build, its release included
            ph, ids = ida.PartitionedHnsw.build(pts, ida.Builder().seed(1).ef_search(EF), parts=P)
            rows = np.empty_like(pts)
            rows[np.asarray(ids)] = pts                    # the caller's rows in global-id order
            ms_plain, b = best(lambda: ph.search_batch(q), args.rounds)
            row = dict(parts=P, search_batch_wall_ms=ms_plain, fetch=[])
            for fetch in FETCH:
                cell = dict(fetch=fetch, pool_bytes_per_call=int(b.count.clip(max=fetch).sum()) * int(ph.parts[0].info().row_stride) * 4)
                obj, ctx, results, reads, direct = {}, {}, {}, {}, {}
                for knob in KNOBS:
                    os.environ["IDIST_MMR"] = knob         # (sampled when the parts' contexts are made)
                    obj[knob] = ida.PartitionedHnsw.from_hnsws(ph.parts)
                    ctx[knob] = ida.Search()
                    obj[knob].search_mmr(q, K, LAM, fetch)                     # warm-up: staging grows
                    if P == 1:
                        ph.parts[0].search_mmr(q, K, LAM, fetch, ctx[knob])
                    reads[knob], direct[knob] = [], []
                os.environ.pop("IDIST_MMR")
                for _ in range(args.rounds):               # the two kernels alternately, call by call
                    for knob in KNOBS:
                        t0 = time.perf_counter()
                        results[knob] = obj[knob].search_mmr(q, K, LAM, fetch)
                        reads[knob].append(((time.perf_counter() - t0) * 1e3,) + obj[knob].last_mmr_ms())
                        if P == 1:
                            t0 = time.perf_counter()
                            one = ph.parts[0].search_mmr(q, K, LAM, fetch, ctx[knob])
                            direct[knob].append(((time.perf_counter() - t0) * 1e3, ctx[knob].mmr_kernel_ms()))
                            assert np.array_equal(one.pids, results[knob].pids) and np.array_equal(one.ranks, results[knob].ranks)
                for knob in KNOBS:
                    wall, gather, select = zip(*reads[knob])
                    cell[knob] = dict(wall_ms=round(min(wall), 3), gather_ms=round(min(gather), 4), select_ms=round(min(select), 4),
                                      gather_ms_all=[round(x, 4) for x in gather], select_ms_all=[round(x, 4) for x in select],
                                      gather_share_of_wall=round(min(gather) / min(wall), 4))
                    if P == 1:
                        wall1, select1 = zip(*direct[knob])
                        cell[knob]["hnsw_search_mmr"] = dict(wall_ms=round(min(wall1), 3), select_ms=round(min(select1), 4),
                                                             select_ms_all=[round(x, 4) for x in select1],
                                                             pool_over_direct_select=round(min(select) / min(select1), 3))
                del obj, ctx
                assert all(np.array_equal(getattr(results["tile"], f), getattr(results["global"], f)) for f in ("pids", "ranks", "counts"))
                hq = min(args.host_queries, N_Q)
                t0 = time.perf_counter()
                ranks = host_mmr(rows, b.pid[:hq], b.distance[:hq], b.count[:hq], K, fetch, LAM)
                ms_host = (time.perf_counter() - t0) * 1e3
                cell["host"] = dict(search_batch_wall_ms=ms_plain, gather_and_greedy_ms_measured=round(ms_host, 3), on_queries=hq,
                                    gather_and_greedy_ms_scaled_to_all=round(ms_host * N_Q / hq, 1),
                                    total_ms_scaled=round(ms_plain + ms_host * N_Q / hq, 1),
                                    same_selection_as_the_device_share=round(float(np.mean(np.all(ranks == results["tile"].ranks[:hq], axis=1))), 4))
                print(json.dumps(dict(parts=P, **cell)), flush=True)
                row["fetch"].append(cell)
            del ph
        doc["parts"].append(row)
        with open(args.out, "w") as fo:                    # (after every P: a partial file beats none)
            json.dump(doc, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
