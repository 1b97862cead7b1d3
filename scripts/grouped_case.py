"""Grouped search measured on bench.py's C2 shape -> profiles/grouped_search.json.  100k x 128-d rows of
bench.py's generator, 10k queries, ef_search 100, k 10; one index, host-pointer calls, no condition.
Group layouts: every point its own group; documents of 4, 16 and 64 chunks assigned at random; the same sizes assigned to contiguous
points of a sort by the first coordinate (clustered in that coordinate); and documents that are neighbourhoods in all coordinates:
every point assigned to the nearest of n / 64 rows drawn as centres (the chunks of a document lie close together); and the worst case,
one document that holds all but 12 points.
Per layout it records: the wall time of `search_grouped` (best of the rounds), the rung histogram, group recall against the same call
with max_rungs = 0 (the ground truth), the HIP-event times of the collapse (select), pending and exact-round kernels beside the rungs'
search-kernel times; and beside them the only way without the call — `search_batch` at ef_search 100 / 400 / 1600 plus a numpy
collapse on the host — with its wall time, its group recall and the share of queries it leaves with fewer than k groups.

One comparison is a bar (nothing else is): on the `own` layout the rungs launch the search kernels of `search_allowed`, so the
collapse kernel is set against allowed_select_kernel — select_ms of `search_grouped` against select_ms of the PARENT commit's
`search_allowed` with every bit set, same data, same queries, measured alternately in this run.  --parent-lib names a libidist.so
built from the parent commit; without it this build's `search_allowed` stands in (the kernel's source is the parent's) and the file
says so.  The run-to-run spread (largest minus smallest per-round ratio) is added to the bar of 2.  A miss is reported, not tuned away.
usage: python scripts/grouped_case.py [--out profiles/grouped_search.json] [--rounds 3] [--ab-rounds 9] [--parent-lib PATH --parent-commit SHA]"""
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
from allowed_case import EF, K, N_Q, ladder  # noqa: E402
from attr_case import best  # noqa: E402
from instant_distance_amd import _capi  # noqa: E402
from metric_case import SHAPES  # noqa: E402

NEW_SYMBOLS = ("idist_search_batch_grouped", "idist_grouped_collapse_device")


def layouts(pts):
    """name -> the group of every point, in the order of `pts`"""
    n = len(pts)
    rng = np.random.default_rng(7)
    out = {"own": np.arange(n, dtype=np.uint32)}
    by_x0 = np.argsort(pts[:, 0], kind="stable")
    for size in (4, 16, 64):
        out[f"documents of {size}, random"] = (rng.permutation(n) // size).astype(np.uint32)
        g = np.zeros(n, np.uint32)
        g[by_x0] = np.arange(n) // size
        out[f"documents of {size}, clustered"] = g
    # one coordinate of 128 says little about who is near whom: a layout whose documents ARE neighbourhoods — every point goes to
    # the nearest of n / 64 rows drawn as centres
    centres = pts[rng.choice(n, n // 64, replace=False)].astype(np.float64)
    c2 = (centres ** 2).sum(axis=1)
    g = np.zeros(n, np.uint32)
    for lo in range(0, n, 8192):
        x = pts[lo: lo + 8192].astype(np.float64)
        g[lo: lo + 8192] = np.argmin(c2[None, :] - 2.0 * (x @ centres.T), axis=1)
    out["documents around n / 64 centres (nearest centre)"] = g
    # the worst case: one document holds everything but 12 points — the ladder runs to its end, then the exact rounds
    g = np.full(n, 0xFFFFFFFF, np.uint32)
    g[rng.choice(n, 12, replace=False)] = np.arange(12, dtype=np.uint32) * 8192
    out["one giant document and 12 single points"] = g
    return out


def host_collapse(pid, count, groups, k):
    """the first entry of each group of every row of a `search_batch` result, at most k: (ids [nq][k] INVALID padded, counts)"""
    out = np.full((len(pid), k), ida.INVALID, np.uint32)
    cnt = np.zeros(len(pid), np.uint32)
    for i in range(len(pid)):
        lst = pid[i, : count[i]]
        _, first = np.unique(groups[lst], return_index=True)
        sel = np.sort(first)[:k]
        out[i, : len(sel)] = lst[sel]
        cnt[i] = len(sel)
    return out, cnt


def group_recall(pid, count, groups, truth):
    """the share of the true groups (the rows of `truth`, a GroupedResult) that a result's rows hold"""
    hit = tot = 0
    for a, ca, b, cb in zip(pid, count, truth.group, truth.count):
        hit += len(set(groups[a[:ca]].tolist()) & set(b[:cb].tolist()))
        tot += int(cb)
    return round(hit / tot, 5) if tot else None


def rungs_launched(hist):
    """ef_search of the rungs an unrestricted call launched: from rung 0 to the last one that answered a query — the whole ladder
    when queries fell through to the exact rounds"""
    E = ladder(EF)
    on = [r for r in hist if r < ida.RUNG_NONE]
    return E if ida.RUNG_EXACT in hist else E[: max(on) + 1] if on else []


def grouped_row(h, s, q, table, groups, rounds):
    ms, r = best(lambda: h.search_grouped(q, table, "g", K, None, s), rounds)
    sel_ms, pend_ms, exact_ms = s.allowed_kernel_ms()
    hist = {int(a): int(b) for a, b in zip(*np.unique(r.rung, return_counts=True))}
    ran = rungs_launched(hist)
    search_ms = [round(float(x), 4) for x in s.kernel_times_ms(len(ran))] if ran else []
    ms0, truth = best(lambda: h.search_grouped(q, table, "g", K, None, s, max_rungs=0), rounds)
    sel0, pend0, exact0 = s.allowed_kernel_ms()
    assert np.all(truth.rung == ida.RUNG_EXACT) and np.array_equal(truth.group, np.where(truth.pid == ida.INVALID, 0, groups[np.minimum(truth.pid, len(groups) - 1)]))
    assert all(len(set(row[:c].tolist())) == c for row, c in zip(r.group[::97], r.count[::97]))
    return truth, dict(search_grouped_ms=ms, queries_per_s=round(len(q) / (ms * 1e-3), 1), rung_histogram=hist, rungs_launched_ef=ran,
                       search_kernels_ms=search_ms, select_kernels_ms=round(sel_ms, 4), pending_kernels_ms=round(pend_ms, 4),
                       exact_rounds_ms=round(exact_ms, 4), group_recall=group_recall(r.pid, r.count, groups, truth),
                       groups_found_histogram={int(a): int(b) for a, b in zip(*np.unique(r.count, return_counts=True))},
                       exact_only=dict(search_grouped_ms=ms0, select_kernels_ms=round(sel0, 4), pending_kernels_ms=round(pend0, 4),
                                       exact_rounds_ms=round(exact0, 4)))


def overfetch_rows(h, plain, q, groups, truth, rounds):
    """`search_batch` at ef_search 100 / 400 / 1600 plus the numpy collapse"""
    out = []
    for ef in (EF, 4 * EF, 16 * EF):
        h.set_ef_search(ef)
        ms_search, b = best(lambda: h.search_batch(q, plain), rounds)
        t0 = time.perf_counter()
        pid, cnt = host_collapse(b.pid, b.count, groups, K)
        ms_host = round((time.perf_counter() - t0) * 1e3, 3)
        out.append(dict(ef_search=ef, search_batch_ms=ms_search, host_collapse_ms=ms_host, total_ms=round(ms_search + ms_host, 3),
                        result_bytes_downloaded=int(b.pid.nbytes + b.distance.nbytes),
                        queries_short_of_k_share=round(float(np.mean(cnt < truth.count)), 5), group_recall=group_recall(pid, cnt, groups, truth)))
    h.set_ef_search(EF)
    return out


def select_bar(h, q, table, parent_lib, ab_rounds):
    """select_ms of search_grouped on `own` against select_ms of the parent's search_allowed with every bit set, alternately"""
    n = len(h.points)
    every = np.ones(n, bool)
    this_lib = _capi.lib()
    lib = parent_lib or this_lib
    zero, layers = h.into_parts()
    with _capi._using(lib):                                        # the parent's own index over the same graph, its own Search
        hp = ida.Hnsw.from_parts(h.points, zero, layers, ida.Builder().ef_search(EF))
        sp = ida.Search()
        ref = hp.search_allowed(q, every, K, sp)
    s = ida.Search()
    got = h.search_grouped(q, table, "g", K, None, s)
    assert np.array_equal(got.pid, ref.pid) and np.array_equal(got.rung, ref.rung) and np.array_equal(got.distance.view(np.uint32), ref.distance.view(np.uint32))
    a_ms, b_ms = [], []
    for _ in range(ab_rounds):
        with _capi._using(lib):
            hp.search_allowed(q, every, K, sp)
            a_ms.append(sp.allowed_kernel_ms()[0])
        h.search_grouped(q, table, "g", K, None, s)
        b_ms.append(s.allowed_kernel_ms()[0])
    with _capi._using(lib):                                        # freed by the library that made them
        del hp, sp
    ratios = [b / a for a, b in zip(a_ms, b_ms)]
    ratio, spread = float(np.median(b_ms) / np.median(a_ms)), float(max(ratios) - min(ratios))
    return dict(parent_library="a libidist.so built from the parent commit" if parent_lib else "this build (allowed_select_kernel is the parent's source)",
                rounds=ab_rounds, parent_search_allowed_select_ms=[round(x, 4) for x in a_ms], search_grouped_select_ms=[round(x, 4) for x in b_ms],
                parent_median_ms=round(float(np.median(a_ms)), 4), grouped_median_ms=round(float(np.median(b_ms)), 4), ratio=round(ratio, 3),
                spread_of_the_per_round_ratio=round(spread, 3), bar=round(2.0 + spread, 3), within_bar=bool(ratio <= 2.0 + spread),
                note="an unrestricted call: neither side reads a count pass, search_grouped reads no bitmap")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_search.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ab-rounds", type=int, default=9)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-commit", default=None, help="the commit --parent-lib was built from (recorded)")
    args = ap.parse_args()
    import torch

    torch.cuda.init()
    dev = torch.device("cuda", 0)
    n, dim = SHAPES["C2"]
    pts = np.ascontiguousarray(bench.synth(torch, n, dim, 123456789, dev).cpu().numpy())
    q = np.ascontiguousarray(bench.synth(torch, N_Q, dim, 123456790, dev).cpu().numpy())
    h, _ = ida.Builder().seed(1).ef_search(EF).build_hnsw(pts)
    pts = h.points                                                               # PointId order: the columns are by PointId
    s, plain = ida.Search(), ida.Search()
    doc = dict(probe="grouped_search", commit=bench.source_stamp(), parent_commit=args.parent_commit, where="one MI355X",
               command="python scripts/grouped_case.py --rounds %d --ab-rounds %d%s" % (args.rounds, args.ab_rounds, " --parent-lib <parent's libidist.so>" if args.parent_lib else ""),
               n=n, dim=dim, queries=N_Q, ef_search=EF, k=K, ladder=ladder(EF), rounds=args.rounds, rows=[])
    parent = _capi.Lib(args.parent_lib, without=NEW_SYMBOLS) if args.parent_lib else None   # every symbol but this feature's
    for name, groups in layouts(pts).items():
        table = h.attribute_table({"g": groups})
        truth, row = grouped_row(h, s, q, table, groups, args.rounds)
        row = dict(layout=name, groups=int(len(np.unique(groups))), **row)
        row["search_batch_plus_host_collapse"] = overfetch_rows(h, plain, q, groups, truth, args.rounds)
        if name == "own":
            row["select_against_parent_search_allowed"] = select_bar(h, q, table, parent, args.ab_rounds)
        print(json.dumps(row), flush=True)
        doc["rows"].append(row)
        with open(args.out, "w") as fo:                                          # (after every layout: a partial file beats none)
            json.dump(doc, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
