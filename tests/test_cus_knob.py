"""IDIST_CUS, the CU count the search side and the helper kernels size their grids by (launch_cus, idist_capi.hip; a test knob: it
exists in the test build, the measurement build and the emulator, not in libidist.so).

The results must not depend on it.  On the GPU, through the test build: the every-path case of each feature's module and one plain
search_batch parity case, with the knob unset, at IDIST_CUS=1 — the geometry the emulator runs: every CU-derived cap is 8 to 64, the
helper kernels take dozens of items per workgroup, a search slot many queries — and at IDIST_CUS=3, grids that do not divide the
work.  Under the emulator (one CU without the knob): IDIST_CUS=256, a full chip's segment counts — many short and empty segments per
query.

Why any count is a legal geometry: search_kernel's workgroups pull queries from the context's queue until it is empty (its grid is
min(nq, slots, resident) and its end-of-launch counter is an atomic add that nobody waits for), every helper kernel strides over
its work items with its grid, and none of them waits for another workgroup — the emulator runs exactly the one-CU geometry to
completion with the workgroups executed one after the other.  The build keeps the device's own count.

The count is sampled when an index is made (idist_index::n_cu), so every run makes its index under the setting it tests."""
import numpy as np
import pytest

import parity_cases as pc
from engines import engine_params
from test_allowed import EXACT, NONE, allowed_sets
from test_allowed import check as check_allowed
from test_allowed import main_case as allowed_case
from test_allowed_sets import rows_of
from test_grouped import CASES as GROUPED_CASES
from test_grouped import check as check_grouped
from test_grouped import expected as grouped_expected
from test_grouped import layout, restriction, selections
from test_partitioned_range import check as check_range_parts
from test_partitioned_range import expected as range_parts_expected
from test_partitioned_range import partitioned as partitioned_range
from test_partitioned_range import range_parts
from test_range import check as check_range
from test_range import main_case as range_case
from test_range import radii_of
from test_range_allowed import cycle, main_sets
from test_range_allowed import main_case as range_allowed_case
from test_range_allowed import model as range_allowed_model


@pytest.fixture(params=engine_params())
def eng(request, engine_loader):
    ida = engine_loader(request.param)
    return ida, request.param


def settings(kind):
    """GPU: unset, 1, 3.  Emulator: 256 (unset is what the neighbouring modules run there, with one CU)"""
    return (None, "1", "3") if kind == "gpu" else ("256",)


def under(monkeypatch, cus):
    if cus is None:
        monkeypatch.delenv("IDIST_CUS", raising=False)
    else:
        monkeypatch.setenv("IDIST_CUS", cus)


def test_allowed_sets_every_path(eng, oracle, monkeypatch):
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    c, k = allowed_case(oracle, kind)
    masks = list(allowed_sets(c, k).values())
    set_of = np.arange(len(c.q)) % 8
    wants = {m: rows_of([c.model(mk, k, m) for mk in masks], set_of) for m in (-1, 2, 0)}
    seen = set().union(*[set(w[3].tolist()) for w in wants.values()])
    assert 0 in seen and any(2 <= r < NONE for r in seen) and NONE in seen and EXACT in seen
    for cus in settings(kind):
        under(monkeypatch, cus)
        h = c.hnsw(ida)
        for m, want in wants.items():
            check_allowed(h.search_allowed_sets(c.q, np.stack(masks), set_of, k, ida.Search(), max_rungs=m, counters=True), want,
                          f"IDIST_CUS {cus}, max_rungs {m}")


def test_range_every_path(eng, oracle, monkeypatch):
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    rc = range_case(oracle, kind)
    rad = radii_of(rc)
    wants = {m: rc.model(rad, max_rungs=m) for m in (-1, 2)}
    seen = set().union(*[set(w[3].tolist()) for w in wants.values()])
    assert 0 in seen and len({r for r in seen if 0 < r < NONE}) >= 2 and EXACT in seen
    for cus in settings(kind):
        under(monkeypatch, cus)
        h = rc.hnsw(ida)
        for m, want in wants.items():
            check_range(h.search_range(rc.q, rad, ida.Search(), max_rungs=m, counters=True), want, f"IDIST_CUS {cus}, max_rungs {m}")


def test_range_allowed_every_path(eng, oracle, monkeypatch):
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    rc = range_allowed_case(oracle, kind)
    masks, bits = main_sets(rc)
    rad, set_of = radii_of(rc), cycle(len(rc.q), 0)
    wants = {m: range_allowed_model(rc, rad, masks, set_of, max_rungs=m) for m in (-1, 2)}
    seen = set().union(*[set(w[3].tolist()) for w in wants.values()])
    assert 0 in seen and EXACT in seen and NONE in seen and {"rule", "ladder"} <= set().union(*[set(w[5]) for w in wants.values()])
    for cus in settings(kind):
        under(monkeypatch, cus)
        h = rc.hnsw(ida)
        for m, want in wants.items():
            got = h.search_range_allowed_sets(rc.q, rad, bits, set_of, ida.Search(), max_rungs=m, counters=True)
            check_range(got, want[:5], f"IDIST_CUS {cus}, max_rungs {m}")


def test_grouped_every_path(eng, oracle, monkeypatch):
    """groups of four documents; on the GPU also twelve bands of coordinate 0, where the exact step takes several rounds (a third of
    a minute of emulated lanes)"""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    c, k = allowed_case(oracle, kind)
    for cus in settings(kind):
        under(monkeypatch, cus)
        h = c.hnsw(ida)
        for lay in ("docs4", "x0 bands 12") if kind == "gpu" else ("docs4",):
            table = h.attribute_table({"g": layout(c, lay), "sel": selections(c)})
            for mask, max_rungs in GROUPED_CASES:
                want = grouped_expected(oracle, kind, lay, mask, max_rungs)
                got = h.search_grouped(c.q, table, "g", k, restriction(c, mask)[0], ida.Search(), max_rungs=max_rungs, counters=True)
                check_grouped(got, want, f"IDIST_CUS {cus}, {lay} / {mask}, max_rungs {max_rungs}")


def test_partitioned_range_every_path(eng, oracle, monkeypatch):
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    pts, q, b, rcs, w = range_parts(oracle, kind, 3)
    rad = radii_of(w)
    wants = {m: range_parts_expected(rcs, b, rad, m)[0] for m in (-1, 2)}
    seen = set().union(*[set(x[3].ravel().tolist()) for x in wants.values()])
    assert 0 in seen and len({r for r in seen if 0 < r < NONE}) >= 1 and EXACT in seen
    for cus in settings(kind):
        under(monkeypatch, cus)
        ph, hs = partitioned_range(ida, rcs)
        for m, want in wants.items():
            check_range_parts(ph.search_range(q, rad, max_rungs=m, counters=True), want, f"IDIST_CUS {cus}, max_rungs {m}")


def test_search_batch_parity(eng, oracle, monkeypatch):
    """tests/test_parity.py's test_search_parity at 16-d: every walk variant, the batch a single slot's queue at IDIST_CUS=1 where it
    is narrow enough for the four-wave walk only up to two queries"""
    ida, kind = eng
    pc.use_test_build(monkeypatch)
    for cus in settings(kind):
        under(monkeypatch, cus)
        pc.check_search_parity(ida, oracle, n=20000 if kind == "gpu" else 260, dim=16, nq=400 if kind == "gpu" else 6, seed=16)
