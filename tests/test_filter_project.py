"""filter_project (csrc/idist_device.hpp): the one evaluation of y = B (x - mu) behind the principal rows and a query's staging.  The
device build requests its operands a block of 32 positions ahead of the arithmetic; the chain of FMAs — and with it every compact
row, every staged query and every verdict — is what the plain loop gives.  Alone on the emulator against a loop written out in the
test (tests/host/project.cpp), and through whole searches at row lengths with and without half a block at the end: ids, order,
counts, distance bits and {n_dist, n_exp0, n_expU} are the oracle's, the filter's counts equal with the inlined blocks and without."""
import os
import subprocess

import numpy as np
import pytest

import engines
import parity_cases as pc
from engines import engine_params
from test_filter import ON_CHIP, S
from test_filter_inline import both, oracle_index
from test_filter_principal import points_and_queries


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    return engine_loader(request.param), request.param


@pytest.mark.parametrize("variant", ["blocked", "plain"])
def test_projection_alone(tmp_path, variant):
    """y and |x - mu|^2 bit for bit, strides 16 ... 624 (remainders 0 and 16 modulo 32), random / one-coordinate / mixed-scale /
    non-finite inputs; `blocked` compiles the device build's blocks for the CPU, `plain` is the emulator's own loop."""
    exe = str(tmp_path / "project")
    simt = os.path.join(engines.ROOT, "tests", "simt")
    flags = ["-DIDIST_EMU"] + (["-DIDIST_PROJECT_BLOCKED"] if variant == "blocked" else [])
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-unused-variable",
                           "-Wno-unused-value", "-Wno-unused-result", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-fast-math", *flags,
                           "-I" + simt, os.path.join(engines.ROOT, "tests", "host", "project.cpp"), os.path.join(simt, "hip_emu.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "project ok" in out.stdout, out.stdout + out.stderr


# 136 -> stride 144 (four blocks and a half), 200 -> 208 (six and a half), 300 -> 304 (nine and a half), 620 -> 624 (nineteen and a half,
# the longest row of a thin walk); 300 and 136 / 200 / 620 are a compile-time and the runtime geometry's kernels
@pytest.mark.parametrize("dim", [136, 200, 300, 620])
def test_search_parity(eng, oracle, monkeypatch, dim):
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    rng = np.random.default_rng(9100 + dim)
    n, ef = S(kind, 700, 20000), S(kind, 12, 100)
    pts, q = points_and_queries(rng, "lowrank", n, S(kind, 12, 600), dim)
    q[0] = pts[n // 2]                                                  # a stored point
    oix, want = oracle_index(oracle, kind, pts, q, 0, ef)
    h = ida.Hnsw.from_parts(pts, oix.zero, oix.layers, ida.Builder().ef_search(ef))
    (seen, rejected), (p_seen, p_rejected), _ = both(ida, monkeypatch, h, q, want, env=ON_CHIP, basis="principal")
    assert h.info().filter_principal_bytes == n * 64
    assert p_seen > 0 and rejected > 0 and p_rejected > 0, (seen, rejected, p_seen, p_rejected)
