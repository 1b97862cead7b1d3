"""Cosine metric against what a user does without it, one JSON line per shape.
(a) a METRIC_COSINE index over raw rows (lengths spread over 2^-3 .. 2^3), searched with raw queries;
(b) an L2SQ index over rows and queries normalised beforehand with `normalize()` — the same bits by definition.
Both are built from the same seed and searched alternately in one process after a warm-up.  Reported: build seconds (HIP events
of the build, and wall time, which holds the upload and for (a) the row pass), search ms per 10k-query batch (host-pointer call,
wall), the search kernel's own time (the context's HIP events), and — from a device-pointer launch between two HIP events on the
null stream — what a launch costs beyond its search kernel: for (a) that is the query normalisation plus the scaling pass, set
beside the floor of their bytes (read + written) over the 6.29 TB/s copy rate of DESIGN.md section 7.  (a) and (b) must return
the same ids and counters, and (a)'s distances must be half of (b)'s, bit for bit: asserted.
Kernel names and per-kernel durations: run this under `rocprofv3 --kernel-trace --stats -- python scripts/metric_case.py ...`.
usage: python scripts/metric_case.py out.jsonl [C2|C3]"""
import ctypes as C
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
COPY_BYTES_PER_S = 6.29e12


def synth_raw(n, dim, seed, latent=32):
    """bench.synth's 'fastText-shape' rows on the host, NOT normalised: every row scaled by 2^U(-3, 3)"""
    a = np.random.default_rng(4242).standard_normal((latent, dim)).astype(np.float32)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, latent)).astype(np.float32) @ a + np.float32(0.05) * rng.standard_normal((n, dim)).astype(np.float32)
    return np.ascontiguousarray(x * np.exp2(rng.uniform(-3, 3, size=(n, 1))).astype(np.float32))


class Hip:
    """the HIP runtime libidist.so already loaded, for device buffers and events of our own"""

    def __init__(self):
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        self.h = C.CDLL(path)
        self.h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.h.hipFree.argtypes = [C.c_void_p]
        self.h.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.h.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.h.hipEventSynchronize.argtypes = [C.c_void_p]
        self.h.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            assert self.h.hipEventCreate(C.byref(e)) == 0

    def alloc(self, nbytes, src=None):
        p = C.c_void_p()
        assert self.h.hipMalloc(C.byref(p), max(nbytes, 16)) == 0
        if src is not None:
            assert self.h.hipMemcpy(p, src.ctypes.data, src.nbytes, 1) == 0
        return p

    def timed(self, fn):
        assert self.h.hipEventRecord(self.ev[0], None) == 0
        fn()
        assert self.h.hipEventRecord(self.ev[1], None) == 0
        assert self.h.hipEventSynchronize(self.ev[1]) == 0
        ms = C.c_float(0)
        assert self.h.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1]) == 0
        return float(ms.value)


def main():
    out, shape = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "C2")
    n, dim = SHAPES[shape]
    nq, ef, rounds = 10_000, 100, 5
    pts, q = synth_raw(n, dim, 123456789), synth_raw(nq, dim, 123456790)
    t0 = time.perf_counter()
    pts_n = ida.normalize(pts)
    rows_normalize_wall = time.perf_counter() - t0
    t0 = time.perf_counter()
    q_n = ida.normalize(q)
    queries_normalize_wall_ms = (time.perf_counter() - t0) * 1e3

    variants = {"cosine": (pts, q, ida.Builder().seed(1).ef_search(ef).metric(ida.METRIC_COSINE)),
                "l2sq_prenormalized": (pts_n, q_n, ida.Builder().seed(1).ef_search(ef))}
    hip, st = None, {}
    for name, (rows, queries, b) in variants.items():
        t0 = time.perf_counter()
        h, _ = b.build_hnsw(rows)
        s = dict(h=h, q=queries, search=ida.Search(), dsearch=ida.Search(), build_wall=time.perf_counter() - t0,
                 build_s=h.build_stats().seconds, wall=[], kern=[], launch=[], launch_kern=[])
        s["res"] = h.search_batch(queries, s["search"], counters=True)          # warm-up: the context grows, staging is allocated
        hip = hip or Hip()
        s["d"] = [hip.alloc(queries.nbytes, queries), hip.alloc(nq * ef * 4), hip.alloc(nq * ef * 4), hip.alloc(nq * 4), hip.alloc(nq * 12)]
        s["dsearch"].reserve(h, 4096)
        s["go"] = (lambda s=s, h=h: h.search_batch_device(s["dsearch"], s["d"][0].value, nq, s["d"][1].value, s["d"][2].value,
                                                          s["d"][3].value, s["d"][4].value))
        hip.timed(s["go"])                                                       # warm-up of the device-pointer context
        st[name] = s
    for _ in range(rounds):                                                      # alternating
        for name, s in st.items():
            t0 = time.perf_counter()
            s["h"].search_batch(s["q"], s["search"], counters=True)
            s["wall"].append((time.perf_counter() - t0) * 1e3)
            s["kern"].append(float(s["search"].kernel_times_ms(1)[-1]))
            s["launch"].append(hip.timed(s["go"]))
            s["launch_kern"].append(float(s["dsearch"].kernel_times_ms(1)[-1]))
    a, b = st["cosine"]["res"], st["l2sq_prenormalized"]["res"]
    same_ids = bool(np.array_equal(a.pid, b.pid) and np.array_equal(a.count, b.count))
    same_counters = bool(np.array_equal(a.counters, b.counters))
    halved = bool(np.array_equal(a.distance.view(np.uint32), (b.distance * np.float32(0.5)).view(np.uint32)))
    assert same_ids and same_counters and halved, (same_ids, same_counters, halved)
    stride = int(st["cosine"]["h"].info().row_stride)
    row = dict(probe="cosine_metric", commit=bench.source_stamp(), shape=shape, n=n, dim=dim, queries=nq, ef=ef, rounds=rounds,
               same_ids=same_ids, same_counters=same_counters, distances_halved_bitwise=halved,
               user_side_normalize_rows_wall_s=round(rows_normalize_wall, 3),
               user_side_normalize_queries_wall_ms=round(queries_normalize_wall_ms, 3),
               floor_us=dict(normalize_rows=round(2 * n * stride * 4 / COPY_BYTES_PER_S * 1e6, 2),
                             normalize_queries=round(2 * nq * dim * 4 / COPY_BYTES_PER_S * 1e6, 2),
                             scale_distances=round(2 * nq * ef * 4 / COPY_BYTES_PER_S * 1e6, 2)))
    for name, s in st.items():
        i = int(np.argmin(s["launch"]))
        row[name] = dict(build_seconds=round(s["build_s"], 3), build_wall_seconds=round(s["build_wall"], 3),
                         search_ms_per_batch=round(min(s["wall"]), 3), search_ms_per_batch_all=[round(x, 3) for x in s["wall"]],
                         search_kernel_ms=round(min(s["kern"]), 4),
                         device_launch_ms=round(s["launch"][i], 4), device_launch_search_kernel_ms=round(s["launch_kern"][i], 4),
                         device_launch_beyond_search_kernel_us=round((s["launch"][i] - s["launch_kern"][i]) * 1e3, 2))
    print(json.dumps(row), flush=True)
    with open(out, "a") as fo:
        fo.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
