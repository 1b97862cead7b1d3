"""Attribute tables measured on bench.py's C2 shape -> profiles/attr_match.json.  100k x 128-d rows of
bench.py's generator, 10k queries, ef_search 100, k 10; host-pointer calls, best of the rounds; one index and P = 4 parts on one GPU.
The table has two columns: tenant, uniform in [0, 256), and day, uniform in [0, 100000).
  tenant_day   query q asks for tenant == q % |D| AND day in [20000, 59999], |D| = 1, 16, 256;
  membership   one condition for the batch, tenant in a list of 8 and of 64 values (no two consecutive: as many conjunctions);
  one_clause   tenant in [0, 63] through the interval kernel (`search_where` on the table's column 0) and through the new one.
Per cell, in the same run: the wall time of `search_match`; the wall time of the only way without it — numpy bitmaps on the host, then
`search_allowed_sets` — with the host's bitmap time listed separately; the HIP-event time of the bitmap kernel (P = 4: the parts'
kernels, summed); the rung histogram.  Both ways are asserted to return the same ids and rungs.  Nothing is asserted on the numbers.
usage: python scripts/attr_match_case.py [--out profiles/attr_match.json] [--rounds 3]"""
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
from allowed_case import EF, K, N_Q  # noqa: E402
from attr_case import best, bits_row_count  # noqa: E402
from instant_distance_amd.api import allowed_bitmaps  # noqa: E402
from metric_case import SHAPES  # noqa: E402

DAY = (20000, 59999)


def mask_of(cond, cols):
    """the bool mask of a condition (a dict or an AnyOf of dicts; an int, a (lo, hi) tuple or a list per column), by numpy"""
    n = len(cols["tenant"])
    out = np.zeros(n, bool)
    for d in ((cond,) if isinstance(cond, dict) else cond.conjunctions):
        conj = np.ones(n, bool)
        for name, spec in d.items():
            v = cols[name]
            conj &= ((v >= spec[0]) & (v <= spec[1])) if isinstance(spec, tuple) else np.isin(v, spec) if isinstance(spec, list) else v == spec
        out |= conj
    return out


def case(match, bitmaps_way, kernel_ms, cols, distinct, set_of, rounds):
    """match(conds) -> result; bitmaps_way(bits, set_of) -> result; distinct: the call's distinct conditions, set_of [nq] into them"""
    conds = distinct[0] if len(distinct) == 1 else [distinct[s] for s in set_of]
    ms_match, a = best(lambda: match(conds), rounds)
    bitmap_ms = kernel_ms()

    def host_bitmaps():
        return allowed_bitmaps(np.stack([mask_of(c, cols) for c in distinct]), len(cols["tenant"]))

    ms_host, bits = best(host_bitmaps, rounds)
    ms_sets, b = best(lambda: bitmaps_way(bits, set_of), rounds)
    assert np.array_equal(a.pid, b.pid) and np.array_equal(a.rung, b.rung) and np.array_equal(a.count, b.count)
    hist = {int(x): int(y) for x, y in zip(*np.unique(a.rung, return_counts=True))}
    return dict(distinct_conditions=len(distinct), allowed_points_per_set=[int(bits_row_count(bits[i])) for i in range(min(len(distinct), 4))],
                search_match_ms=ms_match, bitmap_kernel_ms=round(bitmap_ms, 4), host_bitmaps_ms=ms_host, search_allowed_sets_ms=ms_sets,
                host_bitmaps_plus_search_allowed_sets_ms=round(ms_host + ms_sets, 3), bitmap_upload_bytes=int(bits.nbytes), rung_histogram=hist), a


def cells(match, where, bitmaps_way, kernel_ms, cols, rounds):
    out = dict(tenant_day=[], membership=[])
    for d in (1, 16, 256):
        distinct = [{"tenant": t, "day": DAY} for t in range(d)]
        row, _ = case(match, bitmaps_way, kernel_ms, cols, distinct, (np.arange(N_Q) % d).astype(np.uint32), rounds)
        print(json.dumps(row), flush=True)
        out["tenant_day"].append(row)
    rng = np.random.default_rng(11)
    for m in (8, 64):
        values = sorted((2 * rng.choice(128, m, replace=False)).tolist())
        row, _ = case(match, bitmaps_way, kernel_ms, cols, [{"tenant": values}], np.zeros(N_Q, np.uint32), rounds)
        row = dict(values=m, **row)
        print(json.dumps(row), flush=True)
        out["membership"].append(row)
    # one clause on column 0: the interval kernel and the new one
    row, a = case(match, bitmaps_way, kernel_ms, cols, [{"tenant": (0, 63)}], np.zeros(N_Q, np.uint32), rounds)
    ms_where, w = best(lambda: where(0, 63), rounds)
    assert np.array_equal(a.pid, w.pid) and np.array_equal(a.rung, w.rung) and np.array_equal(a.count, w.count)
    out["one_clause"] = dict(search_where_ms=ms_where, interval_kernel_ms=round(kernel_ms(), 4), **row)
    print(json.dumps(out["one_clause"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attr_match.json"))
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
    doc = dict(probe="attr_match", commit=bench.source_stamp(), where="one MI355X", command="python scripts/attr_match_case.py --rounds %d" % args.rounds,
               n=n, dim=dim, queries=N_Q, ef_search=EF, k=K, rounds=args.rounds)

    def in_id_order(values, ids):
        out = np.zeros(n, np.uint32)
        out[np.asarray(ids)] = values
        return out

    # one index
    h, ids = ida.Builder().seed(1).ef_search(EF).build_hnsw(pts)
    s, s2 = ida.Search(), ida.Search()
    cols = {"tenant": in_id_order(tenant, ids), "day": in_id_order(day, ids)}
    table = h.attribute_table(cols)
    doc["one_index"] = cells(lambda conds: h.search_match(q, table, conds, K, s), lambda lo, hi: h.search_where(q, table, lo, hi, K, s),
                             lambda bits, set_of: h.search_allowed_sets(q, bits, set_of, K, s2), s.attr_bitmap_ms, cols, args.rounds)
    # P = 4 parts on one GPU
    ph, gids = ida.PartitionedHnsw.build(pts, ida.Builder().seed(1).ef_search(EF), parts=4)
    cols = {"tenant": in_id_order(tenant, gids), "day": in_id_order(day, gids)}
    ptable = ph.attribute_table(cols)
    doc["four_parts"] = cells(lambda conds: ph.search_match(q, ptable, conds, K), lambda lo, hi: ph.search_where(q, ptable, lo, hi, K),
                              lambda bits, set_of: ph.search_allowed_sets(q, bits, set_of, K), ph.last_allowed_slice_ms, cols, args.rounds)
    with open(args.out, "w") as fo:
        json.dump(doc, fo, indent=1)
        fo.write("\n")


if __name__ == "__main__":
    main()
