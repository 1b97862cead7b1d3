"""`python bench.py --gpus N` must start itself: the driver's N = 1 command shape (`python bench.py --gpus 1 ...`) repeated at N = 8
has no launcher around it.  These run without a GPU: the command that would be started, the fail-fast line on a node with too few
devices, and the pass-through of rank 0's line (Hnsw::search takes &self, core/lib.rs:352-356); and what a plain run
(no --full) does and writes with --dump-outputs."""
import json
import os
import subprocess
import sys
import time
import types

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_self_launch_command_is_the_drivers_shape():
    cmd = bench.self_launch_command(["--gpus", "8", "--steps", "20", "--warmup", "3"], 8, 29517)
    assert cmd == [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=8", "--master-addr", "127.0.0.1",
                   "--master-port", "29517", os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "20", "--warmup", "3"]


def test_gpus_2_without_devices_fails_fast_with_one_json_line():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2"], env=env, capture_output=True,
                       text=True, timeout=300)
    took = time.time() - t0
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 2 and len(lines) == 1, (r.returncode, r.stdout, r.stderr[-400:])
    line = json.loads(lines[0])
    assert line["value"] is None and line["n_gpus"] == 2 and "device(s) visible" in line["error"]
    assert "Traceback" not in r.stderr
    assert took < 120, took          # (the first `import torch` of a fresh container pages the image in; afterwards this is ~3 s)


def test_self_launch_passes_rank0_line_through(monkeypatch, capsys):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 4)
    seen = {}

    def fake_run(cmd, **kw):
        seen["cmd"], seen["kw"] = cmd, kw
        return types.SimpleNamespace(returncode=0, stdout="noise\n" + json.dumps({"value": 1.0, "n_gpus": 4}) + "\n")

    monkeypatch.setattr(subprocess, "run", fake_run)
    args = bench.parse_args(["--gpus", "4"])
    assert bench.self_launch(args, ["--gpus", "4"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == {"value": 1.0, "n_gpus": 4}
    assert seen["cmd"][:5] == [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=4"]
    assert seen["cmd"][-2:] == ["--gpus", "4"] and seen["kw"]["timeout"] == args.launch_timeout
    assert seen["kw"]["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"

    # ranks that die without a line: still ONE JSON line, and a non-zero exit code
    monkeypatch.setattr(subprocess, "run", lambda cmd, **kw: types.SimpleNamespace(returncode=1, stdout="boom\n"))
    assert bench.self_launch(args, ["--gpus", "4"]) == 1
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["value"] is None and "no result line" in line["error"]


def test_plain_run_is_the_headline_and_dumps_the_last_step(engine_loader, tmp_path):
    """`bench.py --steps K --warmup W` without --full: exactly K timed steps, the headline fields, none of the --full objects;
    --dump-outputs writes the last timed step's answers, identical for identical arguments (emulated kernels, toy size)."""
    import torch

    engine_loader("emu")
    job = bench.Job(torch, dev=torch.device("cpu"))
    toy = ["--n", "300", "--dim", "12", "--nq", "9", "--steps", "3", "--warmup", "1", "--max-batch", "1", "--gt-queries", "0"]
    outs, dumps = [], []
    for i in range(2):
        d = tmp_path / f"run{i}"
        outs.append(bench.run_bench(job, bench.parse_args(toy + ["--dump-outputs", str(d)])))
        dumps.append({f.name: np.load(f) for f in d.iterdir()})
    out = outs[0]
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["unit"] == "queries/s" and out["dtype"] == "f32"
    assert abs(out["value"] - 9 / (out["ms_per_step"] * 1e-3)) <= 1e-3 * out["value"]
    assert out["higher_is_better"] is True and out["metric"].startswith("queries/sec @ recall@10>=0.95")
    assert not {"cpu_baseline", "parity", "single_query", "pcie_inclusive", "checks", "gpu_over_cpu"} & set(out)
    assert out["roofline"]["traffic"] is None and "cpu_baseline" not in out["build"]
    ef = out["config"]["ef_search"]
    a, b = dumps
    assert set(a) == {"pid.npy", "distance.npy", "count.npy", "counters.npy"}
    assert a["pid.npy"].shape == (9, ef) and a["distance.npy"].shape == (9, ef) and a["counters.npy"].shape == (9, 3)
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert np.all(a["count.npy"] == min(ef, 300)) and np.all(a["pid.npy"] < 300) and np.all(a["counters.npy"][:, 0] > 0)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    with pytest.raises(SystemExit):
        bench.parse_args(["--check"])                 # the oracle's checks belong to --full


def test_dump_outputs_pads_like_the_host_call_and_samples_within_budget(tmp_path):
    import torch

    nq, ef = 50, 4
    pid = torch.arange(nq * ef, dtype=torch.int32).reshape(nq, ef)
    dist = torch.rand(nq, ef)
    cnt = torch.full((nq,), ef, dtype=torch.int32)
    cnt[7] = 2
    ctr = torch.randint(0, 1000, (nq, 3), dtype=torch.int32)
    bench.dump_outputs(str(tmp_path / "all"), (pid, dist, cnt, ctr))
    got = {k: np.load(tmp_path / "all" / f"{k}.npy") for k in ("pid", "distance", "count", "counters")}
    assert got["pid"].dtype == np.float64 and got["distance"].dtype == np.float32
    assert np.all(got["pid"][7, 2:] == 0xFFFFFFFF) and np.all(np.isinf(got["distance"][7, 2:]))
    assert np.array_equal(got["pid"][8], pid[8].numpy()) and np.array_equal(got["counters"], ctr.numpy())
    # above the byte budget: a fixed, ordered sample of whole query rows
    row = ef * 8 + ef * 4 + 8 + 3 * 8
    bench.dump_outputs(str(tmp_path / "s1"), (pid, dist, cnt, ctr), budget=10 * row)
    bench.dump_outputs(str(tmp_path / "s2"), (pid, dist, cnt, ctr), budget=10 * row)
    s1, s2 = (np.load(tmp_path / s / "pid.npy") for s in ("s1", "s2"))
    assert s1.shape == (10, ef) and np.array_equal(s1, s2)
    rows = (s1[:, 0] // ef).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(s1, got["pid"][rows])
