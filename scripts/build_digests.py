"""Graph A/B of the build driver: builds a fixed list of indexes and prints, per index, sha256 of the zero layer and of every upper
layer, the number of steps (n_batches) and the device seconds — one JSON line each.  Two libraries built the same graphs exactly when
their outputs agree in everything but `seconds`.
usage: python scripts/build_digests.py [--lib PATH/libidist.so]   (GPU box; default: the package's own library)"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import instant_distance_amd as ida  # noqa: E402
from instant_distance_amd import _capi  # noqa: E402

# (n, dim, builder settings)
CASES = [(30_000, 32, {}),
         (20_000, 128, {}),
         (20_000, 300, {}),
         (10_000, 768, {}),
         (6_000, 1024, {}),
         (2_000, 64, {"extend_candidates": True}),
         (20_000, 64, {"heuristic": False}),
         (20_000, 128, {"max_batch": 1})]


def builder(opts):
    b = ida.Builder().seed(7)
    if opts.get("extend_candidates"):
        b.select_heuristic(ida.Heuristic(extend_candidates=True))
    if opts.get("heuristic") is False:
        b.select_heuristic(None)
    if "max_batch" in opts:
        b.max_batch(opts["max_batch"])
    return b


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--cases", default="", help="comma-separated indexes into CASES (default: all)")
    ap.add_argument("--progress", action="store_true", help="report every twentieth of a build on stderr (the extend_candidates case "
                    "builds one insertion per single-wave launch)")
    args = ap.parse_args()
    if args.lib:
        _capi._singleton = _capi.Lib(os.path.abspath(args.lib))
    for n, dim, opts in ([CASES[int(i)] for i in args.cases.split(",")] if args.cases else CASES):
        pts = np.random.default_rng(1000 + dim).random((n, dim), dtype=np.float32)
        b = builder(opts)
        if args.progress:
            seen, t0 = [-1], time.time()

            def bar(done, total, layer, seen=seen, t0=t0):
                step = done * 20 // max(total, 1)
                if step > seen[0]:
                    seen[0] = step
                    print(f"{done}/{total} layer {layer} after {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
            b.progress(bar)
        h = ida.Hnsw.from_ordered_points(pts, b)
        st = h.build_stats()
        zero, layers = h.into_parts()
        print(json.dumps({"n": n, "dim": dim, "opts": opts, "n_batches": int(st.n_batches), "zero": sha(zero), "layers": [sha(x) for x in layers],
                          "seconds": round(float(st.seconds), 4)}), flush=True)


if __name__ == "__main__":
    main()
