"""Diverse search measured on bench.py's shapes -> profiles/mmr_search.json.  Per shape (C2 100k x 128-d,
C3 1M x 300-d, W768 100k x 768-d rows of bench.py's generator): one index, 10k queries, ef_search 100, k 10, lam 0.5, host-pointer
calls, best of the rounds.  A run measures the shapes it is given and keeps the file's rows of the others; every row names its own
commit and command.  It records the wall time and the search-kernel time of `search_batch` alone and, for fetch 32 / 64 / 100,
  - `search_mmr` with the tile kernel and with the global kernel (IDIST_MMR=tile|global, a knob of the test build: both run through
    libidist_variants.so on the same index, alternately call by call): the best wall, search kernel and selection kernel (HIP
    events) of the rounds, and every round's selection-kernel reading, so that the spread stands next to the difference;
  - the only way without the call: `search_batch`, a numpy gather of fetch rows per query from the caller's points and the greedy
    loop in numpy (squared L2 by the product form — a host baseline, not the definition; it is timed on a slice of the queries and
    scaled, and the file says so).
The comparison that decides plan_mmr is tile against global per shape and fetch; nothing here is a bar.
usage: python scripts/mmr_case.py [--out profiles/mmr_search.json] [--rounds 3] [--shapes C2,C3,W768] [--host-queries 500]"""
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
from metric_case import SHAPES as BENCH_SHAPES  # noqa: E402

SHAPES = dict(BENCH_SHAPES, W768=(100_000, 768))          # + the third tile geometry: no bench.py shape has it
LAM = 0.5
FETCH = (32, 64, 100)
KNOBS = ("tile", "global")


def host_mmr(pts, pid, dist, count, k, fetch, lam):
    """gather + greedy loop on the host for the rows of a `search_batch` result -> the selected list positions [nq][k]"""
    lam, mu = np.float32(lam), np.float32(1) - np.float32(lam)
    out = np.zeros((len(pid), k), np.uint32)
    for i in range(len(pid)):
        m = min(int(count[i]), fetch)
        rows = pts[pid[i, :m]]
        n2 = (rows * rows).sum(axis=1)
        mi, free, s = np.full(m, np.inf, np.float32), np.ones(m, bool), 0
        for t in range(min(k, m)):
            out[i, t], free[s] = s, False
            mi = np.minimum(mi, n2 + n2[s] - np.float32(2) * (rows @ rows[s]))
            score = np.where(free, lam * dist[i, :m] - mu * mi, np.inf)
            s = int(np.argmin(score))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmr_search.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="C2,C3,W768")
    ap.add_argument("--host-queries", type=int, default=500)
    args = ap.parse_args()
    import torch

    torch.cuda.init()
    dev = torch.device("cuda", 0)
    test_lib = _capi.Lib(os.path.join(os.path.dirname(_capi.LIB_PATH), "libidist_variants.so"))
    doc = dict(probe="mmr_search", where="one MI355X", queries=N_Q, ef_search=EF, k=K, lam=LAM, shapes=[])
    if os.path.exists(args.out):                           # a shape per run is enough: the rows of the other shapes stay, each names its own run
        with open(args.out) as fi:
            old = json.load(fi)
        if all(old.get(f) == doc[f] for f in ("probe", "queries", "ef_search", "k", "lam")):
            doc["shapes"] = [r for r in old["shapes"] if r["shape"] not in args.shapes.split(",") and "commit" in r]
    for shape in args.shapes.split(","):
        n, dim = SHAPES[shape]
        pts = np.ascontiguousarray(bench.synth(torch, n, dim, 123456789, dev).cpu().numpy())
        q = np.ascontiguousarray(bench.synth(torch, N_Q, dim, 123456790, dev).cpu().numpy())
        with _capi._using(test_lib):                       # everything of this shape belongs to the test build, its release included
            h, _ = ida.Builder().seed(1).ef_search(EF).build_hnsw(pts)
            pts = h.points
            plain = ida.Search()
            ms_plain, b = best(lambda: h.search_batch(q, plain), args.rounds)
            row = dict(shape=shape, n=n, dim=dim, commit=bench.source_stamp(), rounds=args.rounds, host_baseline_queries=args.host_queries,
                       command="python scripts/mmr_case.py --rounds %d --shapes %s" % (args.rounds, args.shapes), search_batch=dict(wall_ms=ms_plain, search_kernel_ms=round(float(plain.kernel_times_ms(1)[0]), 4)),
                       fetch=[])
            for fetch in FETCH:
                cell = dict(fetch=fetch, pool_bytes_per_call=int(N_Q * fetch * h.info().row_stride * 4))
                ctx, results, reads = {}, {}, {}
                for knob in KNOBS:
                    os.environ["IDIST_MMR"] = knob
                    ctx[knob] = ida.Search()               # (the knob is sampled when the context is made)
                    h.search_mmr(q, K, LAM, fetch, ctx[knob])                  # warm-up: staging grows
                    reads[knob] = []
                os.environ.pop("IDIST_MMR")
                for _ in range(args.rounds):               # the two kernels alternately, call by call
                    for knob in KNOBS:
                        t0 = time.perf_counter()
                        results[knob] = h.search_mmr(q, K, LAM, fetch, ctx[knob])
                        wall = (time.perf_counter() - t0) * 1e3
                        reads[knob].append((wall, float(ctx[knob].kernel_times_ms(1)[0]), ctx[knob].mmr_kernel_ms()))
                for knob in KNOBS:
                    wall, search, mmr = zip(*reads[knob])
                    cell[knob] = dict(wall_ms=round(min(wall), 3), search_kernel_ms=round(min(search), 4), mmr_kernel_ms=round(min(mmr), 4),
                                      mmr_kernel_ms_all=[round(x, 4) for x in mmr])
                del ctx
                assert all(np.array_equal(getattr(results["tile"], f), getattr(results["global"], f)) for f in ("pids", "ranks", "counts"))
                cell["tile_over_global_kernel"] = round(cell["tile"]["mmr_kernel_ms"] / cell["global"]["mmr_kernel_ms"], 3)
                # the tile is ahead only where its slowest reading beats the global kernel's fastest
                cell["tile_ahead_in_every_reading"] = max(cell["tile"]["mmr_kernel_ms_all"]) < min(cell["global"]["mmr_kernel_ms_all"])
                hq = min(args.host_queries, N_Q)
                t0 = time.perf_counter()
                ranks = host_mmr(pts, b.pid[:hq], b.distance[:hq], b.count[:hq], K, fetch, LAM)
                ms_host = (time.perf_counter() - t0) * 1e3
                cell["host"] = dict(search_batch_wall_ms=ms_plain, gather_and_greedy_ms_measured=round(ms_host, 3), on_queries=hq,
                                    gather_and_greedy_ms_scaled_to_all=round(ms_host * N_Q / hq, 1),
                                    total_ms_scaled=round(ms_plain + ms_host * N_Q / hq, 1),
                                    same_selection_as_the_device_share=round(float(np.mean(np.all(ranks == results["tile"].ranks[:hq], axis=1))), 4),
                                    result_bytes_downloaded=int(b.pid.nbytes + b.distance.nbytes))
                print(json.dumps(dict(shape=shape, **cell)), flush=True)
                row["fetch"].append(cell)
            del plain, h
        doc["shapes"].append(row)
        with open(args.out, "w") as fo:                    # (after every shape: a partial file beats none)
            json.dump(doc, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
