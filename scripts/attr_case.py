"""Attribute filters measured on bench.py's C2 shape -> profiles/attr_search.json.  100k x 128-d rows of
bench.py's generator, 10k queries, ef_search 100, k 10; host-pointer calls, best of the rounds; one index and P = 4 parts on one GPU.
  equality   |D| = 1, 16, 256 distinct equality conditions over a uniform attribute in [0, 256) (query q asks for value q % |D|);
  interval   one interval for the batch over a uniform attribute in [0, 100000), covering 0.1 %, 1 %, 10 % and 100 % of the points.
Per case, in the same run: the wall time of `search_where`; the wall time of the only way without it — numpy bitmaps on the host, then
`search_allowed_sets` — with the host's bitmap time listed separately; the HIP-event time of the bitmap kernel (P = 4: the parts'
kernels, summed); the rung histogram.  Both ways are asserted to return the same ids and rungs.  Nothing is asserted on the numbers.
usage: python scripts/attr_case.py [--out profiles/attr_search.json] [--rounds 3]"""
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
from instant_distance_amd.api import allowed_bitmaps  # noqa: E402
from metric_case import SHAPES  # noqa: E402


def best(call, rounds):
    """(best wall in ms of `rounds` calls after a warm-up: staging grows, the last result)"""
    call()
    wall = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        r = call()
        wall.append((time.perf_counter() - t0) * 1e3)
    return round(min(wall), 3), r


def case(where, bitmaps_way, kernel_ms, v, lo, hi, rounds):
    """where(lo, hi) -> result; bitmaps_way(bits, set_of) -> result; v: the attribute in the order of the index's ids"""
    pairs = sorted(set(zip(lo.tolist(), hi.tolist())))
    index = {p: i for i, p in enumerate(pairs)}
    set_of = np.array([index[p] for p in zip(lo.tolist(), hi.tolist())], np.uint32)
    ms_where, a = best(lambda: where(lo, hi), rounds)
    bitmap_ms = kernel_ms()

    def host_bitmaps():
        return allowed_bitmaps(np.stack([(v >= p[0]) & (v <= p[1]) for p in pairs]), len(v))

    ms_host, bits = best(host_bitmaps, rounds)
    ms_sets, b = best(lambda: bitmaps_way(bits, set_of), rounds)
    assert np.array_equal(a.pid, b.pid) and np.array_equal(a.rung, b.rung) and np.array_equal(a.count, b.count)
    hist = {int(x): int(y) for x, y in zip(*np.unique(a.rung, return_counts=True))}
    return dict(distinct_conditions=len(pairs), allowed_points_per_set=[int(bits_row_count(bits[i])) for i in range(min(len(pairs), 4))],
                search_where_ms=ms_where, bitmap_kernel_ms=round(bitmap_ms, 4), host_bitmaps_ms=ms_host, search_allowed_sets_ms=ms_sets,
                host_bitmaps_plus_search_allowed_sets_ms=round(ms_host + ms_sets, 3), bitmap_upload_bytes=int(bits.nbytes), rung_histogram=hist)


def bits_row_count(row):
    return np.unpackbits(row.view(np.uint8)).sum()


def cases(where, bitmaps_way, kernel_ms, tenant, day, rounds):
    out = dict(equality=[], interval=[])
    for d in (1, 16, 256):
        lo = (np.arange(N_Q) % d).astype(np.uint32)
        row = case(where(0), bitmaps_way, kernel_ms, tenant, lo, lo, rounds)
        print(json.dumps(row), flush=True)
        out["equality"].append(row)
    for share in (0.001, 0.01, 0.1, 1.0):
        lo, hi = np.zeros(N_Q, np.uint32), np.full(N_Q, int(share * 100000) - 1, np.uint32)
        row = dict(share=share, **case(where(1), bitmaps_way, kernel_ms, day, lo, hi, rounds))
        print(json.dumps(row), flush=True)
        out["interval"].append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attr_search.json"))
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch

    torch.cuda.init()
    dev = torch.device("cuda", 0)
    n, dim = SHAPES["C2"]
    pts = np.ascontiguousarray(bench.synth(torch, n, dim, 123456789, dev).cpu().numpy())
    q = np.ascontiguousarray(bench.synth(torch, N_Q, dim, 123456790, dev).cpu().numpy())
    rng = np.random.default_rng(5)
    tenant, day = rng.integers(0, 256, n).astype(np.uint32), rng.integers(0, 100000, n).astype(np.uint32)
    doc = dict(probe="attr_search", commit=bench.source_stamp(), where="one MI355X", command="python scripts/attr_case.py --rounds %d" % args.rounds,
               n=n, dim=dim, queries=N_Q, ef_search=EF, k=K, rounds=args.rounds)

    def in_id_order(values, ids):
        out = np.zeros(n, np.uint32)
        out[np.asarray(ids)] = values
        return out

    # one index
    h, ids = ida.Builder().seed(1).ef_search(EF).build_hnsw(pts)
    s, s2 = ida.Search(), ida.Search()
    vs = [in_id_order(tenant, ids), in_id_order(day, ids)]
    attrs = [h.attributes(x) for x in vs]
    doc["one_index"] = cases(lambda i: (lambda lo, hi: h.search_where(q, attrs[i], lo, hi, K, s)),
                             lambda bits, set_of: h.search_allowed_sets(q, bits, set_of, K, s2), s.attr_bitmap_ms, vs[0], vs[1], args.rounds)
    # P = 4 parts on one GPU
    ph, gids = ida.PartitionedHnsw.build(pts, ida.Builder().seed(1).ef_search(EF), parts=4)
    vs = [in_id_order(tenant, gids), in_id_order(day, gids)]
    pattrs = [ph.attributes(x) for x in vs]
    doc["four_parts"] = cases(lambda i: (lambda lo, hi: ph.search_where(q, pattrs[i], lo, hi, K)),
                              lambda bits, set_of: ph.search_allowed_sets(q, bits, set_of, K), ph.last_allowed_slice_ms, vs[0], vs[1], args.rounds)
    with open(args.out, "w") as fo:
        json.dump(doc, fo, indent=1)
        fo.write("\n")


if __name__ == "__main__":
    main()
