"""The Python layer (api.py, partition.py) against its recorded call transcript, tests/golden/api_calls.txt: what every restricted,
range, attribute and condition search of `Hnsw`, `HnswMap` and `PartitionedHnsw` hands to the C ABI — symbols, scalars, dtypes, shapes,
contiguity, bytes — what it returns and what it refuses, in which order.  No engine, no device: a recorder stands in for the library
(tests/golden/make_api_calls.py, which also says where the golden comes from: the commit before a change, never the code under test).
An intended change of the layer is made by recording the table from the parent commit first and reviewing the diff of the file."""
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def test_calls_match_recorded_transcript(monkeypatch):
    spec = importlib.util.spec_from_file_location("make_api_calls", os.path.join(HERE, "golden", "make_api_calls.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    import instant_distance_amd as ida

    got = gen.transcript(ida, monkeypatch.setattr)
    with open(gen.GOLDEN) as f:
        want = f.read()
    if got != want:                                  # name the first line that differs, under its case
        g, w = got.splitlines(), want.splitlines()
        i = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        case = next((line for line in reversed(w[:i + 1]) if line.startswith("#")), "")
        raise AssertionError(f"line {i + 1} ({case}):\n  recorded: {w[i] if i < len(w) else '<end>'}\n  now:      {g[i] if i < len(g) else '<end>'}")
