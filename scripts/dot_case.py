"""Inner-product metric against what a user does without it -> profiles/dot_metric.json.
(a) a METRIC_DOT index over the raw rows, searched with the raw queries;
(b) an L2SQ index over rows augmented beforehand with `augment_dot()` (dim + 1 coordinates), searched with queries that carry a
    trailing 0 — the same bits by definition;
(c) a plain L2SQ index over the same dim-wide rows: only for the reject filter's counts (and its rate, as context: a 301-d index
    has no compile-time geometry, a 300-d one has).
All three are built from the same seed and searched alternately in one process after a warm-up.  Asserted: (a) and (b) return
the same ids and counters, and (a)'s distances are 0.5f * (d_b - (s(q) + S)) bit for bit.  Recorded: queries/s of (a) and (b)
(host-pointer call, wall), the search kernel's own HIP-event time, what a device-pointer launch of (a) costs beyond its search
kernel (two HIP events on the null stream around the launch: the query augmentation and the report pass) beside the floor of
their bytes over the 6.29 TB/s copy rate of DESIGN.md section 7, and the filter's examined / rejected counts of (a), (b), (c).
Data: `C3` = bench.py's generator as it is (1M x 300-d, L2-normalised rows: every extra coordinate is tiny), `C3raw` = the same
rows scaled by 2^U(-3, 3) (scripts/metric_case.py's: the extra coordinate then dwarfs the other 300 for most rows).
--headline-this / --headline-parent: files of bench.py result lines (default run) measured alternately on this commit and on
its parent in the same session; both value lists and the parent's own spread go into the same JSON.
usage: python scripts/dot_case.py [C3|C3raw|C2|C2raw ...] [--out profiles/dot_metric.json] [--headline-this F --headline-parent F]"""
import argparse
import ctypes as C
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
from metric_case import COPY_BYTES_PER_S, SHAPES, Hip, synth_raw  # noqa: E402


def data(shape):
    n, dim = SHAPES[shape[:2]]
    nq = 10_000
    if shape.endswith("raw"):
        return synth_raw(n, dim, 123456789), synth_raw(nq, dim, 123456790)
    import torch

    dev = torch.device("cuda", 0)
    pts = bench.synth(torch, n, dim, 123456789, dev).cpu().numpy()
    q = bench.synth(torch, nq, dim, 123456790, dev).cpu().numpy()
    return np.ascontiguousarray(pts), np.ascontiguousarray(q)


def one_shape(shape, hip):
    pts, q = data(shape)
    n, dim = pts.shape
    nq, ef, rounds = len(q), 100, 5
    t0 = time.perf_counter()
    pts_a, S = ida.augment_dot(pts)
    rows_augment_wall = time.perf_counter() - t0
    _, _, sq = ida.augment_dot(q, return_norm2=True)
    q_a = np.ascontiguousarray(np.concatenate([q, np.zeros((nq, 1), np.float32)], axis=1))
    extra = pts_a[:, dim]
    variants = {"dot": (pts, q, ida.Builder().seed(1).ef_search(ef).metric(ida.METRIC_DOT)),
                "l2sq_preaugmented": (pts_a, q_a, ida.Builder().seed(1).ef_search(ef)),
                "l2sq_plain": (pts, q, ida.Builder().seed(1).ef_search(ef))}
    st = {}
    for name, (rows, queries, b) in variants.items():
        t0 = time.perf_counter()
        h, _ = b.build_hnsw(rows)
        s = dict(h=h, q=queries, search=ida.Search(), dsearch=ida.Search(), build_wall=time.perf_counter() - t0,
                 build_s=h.build_stats().seconds, wall=[], kern=[], launch=[], launch_kern=[], filt=[])
        s["res"] = h.search_batch(queries, s["search"], counters=True)          # warm-up: the context grows, staging is allocated
        s["d"] = [hip.alloc(queries.nbytes, queries), hip.alloc(nq * ef * 4), hip.alloc(nq * ef * 4), hip.alloc(nq * 4), hip.alloc(nq * 12)]
        s["dsearch"].reserve(h, 4096)
        s["go"] = (lambda s=s, h=h: h.search_batch_device(s["dsearch"], s["d"][0].value, nq, s["d"][1].value, s["d"][2].value,
                                                          s["d"][3].value, s["d"][4].value))
        hip.timed(s["go"])                                                       # warm-up of the device-pointer context
        st[name] = s
    for _ in range(rounds):                                                      # alternating
        for name, s in st.items():
            s["search"].filter_counts()                                          # reset
            t0 = time.perf_counter()
            s["h"].search_batch(s["q"], s["search"], counters=True)
            s["wall"].append((time.perf_counter() - t0) * 1e3)
            s["kern"].append(float(s["search"].kernel_times_ms(1)[-1]))
            s["filt"].append(s["search"].filter_counts())
            s["launch"].append(hip.timed(s["go"]))
            s["launch_kern"].append(float(s["dsearch"].kernel_times_ms(1)[-1]))
    a, b = st["dot"]["res"], st["l2sq_preaugmented"]["res"]
    same_ids = bool(np.array_equal(a.pid, b.pid) and np.array_equal(a.count, b.count))
    same_counters = bool(np.array_equal(a.counters, b.counters))
    t = (sq + np.float32(S)).astype(np.float32)
    want = np.where(np.isinf(b.distance) | np.isnan(b.distance), b.distance, np.float32(0.5) * (b.distance - t[:, None])).astype(np.float32)
    formula = bool(np.array_equal(a.distance.view(np.uint32), want.view(np.uint32)))
    assert same_ids and same_counters and formula, (same_ids, same_counters, formula)
    info = st["dot"]["h"].info()
    assert info.dim == dim and np.float32(info.dot_bound) == np.float32(S)
    row = dict(probe="dot_metric", commit=bench.source_stamp(), shape=shape, n=n, dim=dim, kdim=dim + 1, queries=nq, ef=ef, rounds=rounds,
               same_ids=same_ids, same_counters=same_counters, reported_formula_bitwise=formula,
               dot_bound=float(S), extra_coordinate=dict(min=float(extra.min()), median=float(np.median(extra)), max=float(extra.max()),
                                                         other_coordinates_abs_p99=float(np.quantile(np.abs(pts[:2048]), 0.99))),
               row_stride_floats=int(info.row_stride), row_stride_floats_plain=int(st["l2sq_plain"]["h"].info().row_stride),
               user_side_augment_rows_wall_s=round(rows_augment_wall, 3),
               floor_us=dict(augment_queries=round((nq * dim + nq * (dim + 1) + nq) * 4 / COPY_BYTES_PER_S * 1e6, 2),
                             report_distances=round((2 * nq * ef + nq) * 4 / COPY_BYTES_PER_S * 1e6, 2)))
    for name, s in st.items():
        i = int(np.argmin(s["launch"]))
        ex, rej = s["filt"][-1]
        row[name] = dict(build_seconds=round(s["build_s"], 3), build_wall_seconds=round(s["build_wall"], 3),
                         search_ms_per_batch=round(min(s["wall"]), 3), search_ms_per_batch_all=[round(x, 3) for x in s["wall"]],
                         queries_per_s=round(nq / (min(s["wall"]) * 1e-3), 1),
                         search_kernel_ms=round(min(s["kern"]), 4),
                         device_launch_ms=round(s["launch"][i], 4), device_launch_search_kernel_ms=round(s["launch_kern"][i], 4),
                         device_launch_beyond_search_kernel_us=round((s["launch"][i] - s["launch_kern"][i]) * 1e3, 2),
                         filter_examined=int(ex), filter_rejected=int(rej), filter_rejected_share=round(rej / ex, 4) if ex else None)
    d = row["dot"]
    d["added_passes_share_of_launch"] = round(d["device_launch_beyond_search_kernel_us"] * 1e-3 / d["device_launch_ms"], 5)
    return row


def headline(path):
    vals = []
    for line in open(path):
        line = line.strip()
        if line.startswith("{"):
            try:
                v = json.loads(line).get("value")
            except ValueError:
                continue
            if v is not None:
                vals.append(float(v))
    return vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["C3"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dot_metric.json"))
    ap.add_argument("--headline-this", default="")
    ap.add_argument("--headline-parent", default="")
    args = ap.parse_args()
    doc = dict(probe="dot_metric", commit=bench.source_stamp(), where="one MI355X",
               command="python scripts/dot_case.py " + " ".join(sys.argv[1:]), rows=[])
    if os.path.exists(args.out):                                                 # a later call adds to what an earlier one measured
        try:
            old = json.load(open(args.out))
            doc["rows"] = [r for r in old.get("rows", []) if r.get("shape") not in args.shapes]
            if "headline" in old:
                doc["headline"] = old["headline"]
        except ValueError:
            pass
    if args.shapes and args.shapes != ["none"]:
        if any(not sh.endswith("raw") for sh in args.shapes):
            import torch                                                         # (bench.synth runs on the device: torch's HIP runtime has to come up first — _capi.Lib)

            torch.cuda.init()
        ida.Hnsw.from_ordered_points(np.zeros((4, 3), np.float32))               # brings the HIP runtime up before Hip() looks for it
        hip = Hip()
        for shape in args.shapes:
            row = one_shape(shape, hip)
            print(json.dumps(row), flush=True)
            doc["rows"].append(row)
    if args.headline_this and args.headline_parent:
        this, parent = headline(args.headline_this), headline(args.headline_parent)
        doc["headline"] = dict(what="bench.py --gpus 1 (default run) queries/s, this commit and its parent alternating in one session",
                               this=this, parent=parent, parent_spread=round(max(parent) - min(parent), 1) if parent else None,
                               this_median=float(np.median(this)) if this else None,
                               parent_median=float(np.median(parent)) if parent else None)
    with open(args.out, "w") as fo:
        json.dump(doc, fo, indent=1)
        fo.write("\n")


if __name__ == "__main__":
    main()
