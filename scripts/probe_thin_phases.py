"""Where a zero-layer expansion of the inlined thin principal walk spends its time (needs a GPU; measurement build `make probe`):
one C3-shaped wide launch (1M x 300-d, 10k queries, ef 100) through libidist_probe.so, then the walk's phase stamps — 10-ns
ticks per segment, summed over all walks of the launch and divided by the expansions (idist_probe_thin, QP_MARK in
idist_device.hpp).  "rows arrived" is what is left of the f32 round trip after `mid`: the wave waits there and nowhere else.
The stamped kernel waits for all rows of a pass before its arithmetic and keeps a few registers in scratch, so its launch is
slower than the product's; the split between the segments is what the numbers are for.
The whole query slot as well (QS_MARK in search_kernel / search_layers): ticks per query from one queue pull to the next —
queue pull, query into LDS, filter_stage_query, push_entry, upper layers, layer transitions, zero layer, emit + clear + counter
atomics — beside `slot_ticks_per_query` = kernel time x slots / queries; `unaccounted` is the difference: the slots' wait for
the last walks of the launch (`idle_at_the_ends` from the slots' own lifetimes) plus each slot's last, failed pull.
usage: python scripts/probe_thin_phases.py <tag> [out.jsonl] [n] [nq]"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
import instant_distance_amd as ida  # noqa: E402
from instant_distance_amd import _capi  # noqa: E402

# mark index -> segment (the time since the previous mark); indices as in search_layer
SEGMENTS = [(0, "pop"), (1, "peek_adjacency_block_taken"), (12, "lookup"), (13, "verdicts_next_block_requested"),
            (14, "compact_loads_issued"), (15, "mid"), (16, "rows_arrived"), (3, "fma_fold_done"), (5, "push_truncate")]
COUNTS = [(6, "expansions"), (17, "f32_trips"), (10, "new_ids")]
# the whole slot: word 24 + i = slot mark i (per query); 32 upper-layer expansions, 33 queries, 34 slots, 35 the slots' lifetimes
SLOT_SEGMENTS = [(0, "queue_pull"), (1, "query_into_lds"), (2, "filter_stage_query"), (3, "push_entry"), (4, "upper_layers"),
                 (5, "layer_transitions"), (6, "zero_layer"), (7, "emit_clear_counters")]

torch.cuda.init()
lib = _capi.Lib(os.path.join(ROOT, "instant-distance_amd", "csrc", os.environ.get("PB_LIB", "libidist_probe.so")))
_capi._singleton = lib
probe = lib.cdll.idist_probe_thin
probe.restype = C.c_int
probe.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]

tag = sys.argv[1] if len(sys.argv) > 1 else "thin_phases"
out_path = sys.argv[2] if len(sys.argv) > 2 else None            # the line is printed; appended to this file if one is named
n = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
nq = int(sys.argv[4]) if len(sys.argv) > 4 else 10_000
dim = 300
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
dev = torch.device("cuda", 0)
d_pts = bench.synth(torch, n, dim, 123456789, dev)
d_q = bench.synth(torch, nq, dim, 123456790, dev)
torch.cuda.synchronize()
h = ida.Hnsw.from_device_points(d_pts.data_ptr(), n, dim, ida.Builder())
o = (torch.empty(nq, 100, dtype=torch.int32, device=dev), torch.empty(nq, 100, dtype=torch.float32, device=dev),
     torch.empty(nq, dtype=torch.int32, device=dev), torch.zeros(nq, 3, dtype=torch.int32, device=dev))
st = torch.cuda.current_stream().cuda_stream
s = ida.Search()
buf = (C.c_ulonglong * 40)()


def launch():
    h.search_batch_device(s, d_q.data_ptr(), nq, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), st)
    torch.cuda.synchronize()
    s.check_status()


for _ in range(3):
    launch()
assert probe(buf, 1) == 0                                       # (the build's and the warm-up's ticks are dropped)
s.filter_inline_counts()
launch()
assert probe(buf, 1) == 0
t = [int(v) for v in buf]
nexp = max(t[6], 1)
row = {"tag": tag, "n": n, "nq": nq, "kernel_ms": round(float(s.kernel_times_ms(1)[-1]), 3)}
row.update({name: t[i] for i, name in COUNTS})
row["filter_inline_counts"] = list(s.filter_inline_counts())
row["ticks_per_expansion"] = {name: round(t[i] / nexp, 2) for i, name in SEGMENTS}
row["ticks_per_expansion"]["total"] = round(sum(t[i] for i, _ in SEGMENTS) / nexp, 2)
row["rows_arrived_ticks_per_f32_trip"] = round(t[16] / max(t[17], 1), 2)
ctr = o[3].cpu().numpy().astype(np.int64)
row["n_exp0"] = int(ctr[:, 1].sum())
w = t[24:]
queries, slots = max(w[9], 1), max(w[10], 1)
row["slots"] = w[10]
row["stamped_queries"] = w[9]
row["upper_expansions_per_query"] = round(w[8] / queries, 2)
row["ticks_per_query"] = {name: round(w[i] / queries, 1) for i, name in SLOT_SEGMENTS}
row["ticks_per_query"]["total"] = round(sum(w[i] for i, _ in SLOT_SEGMENTS) / queries, 1)
row["ticks_per_upper_expansion"] = round(w[4] / max(w[8], 1), 1)
row["slot_ticks_per_query"] = round(row["kernel_ms"] * 1e5 * slots / queries, 1)
row["unaccounted"] = round(row["slot_ticks_per_query"] - row["ticks_per_query"]["total"], 1)
row["idle_at_the_ends"] = round((row["kernel_ms"] * 1e5 * slots - w[11]) / queries, 1)
print(json.dumps(row), flush=True)
if out_path:
    open(out_path, "a").write(json.dumps(row) + "\n")
