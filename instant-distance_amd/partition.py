"""Partitioned index: several `Hnsw` parts searched as one (include/idist.h).

The reference has one `Hnsw` per set of points; across GPUs this package could so far only copy ONE index everywhere and
split the queries (`Hnsw.replicate`, dist.py).  A `PartitionedHnsw` cuts the POINTS instead: P ordinary indexes, on any
devices, each built and searched exactly as before; a query is answered by searching every part and keeping the best
`ef_search` of the union, merged on the GPU by the reference's `Candidate` order (distance, then id).

    global id of a point = base[p] + its PointId inside part p        (base[p] = points in parts 0..p-1)

"Partitioned", not "sharded": in this package sharded means queries split over replicas.
"""
from __future__ import annotations

import copy
import ctypes as C
import threading
from typing import Sequence

import numpy as np

from . import _capi
from ._capi import INVALID, METRIC_DOT
from .api import (AllowedResult, Attr, AttrTable, BatchResult, Builder, Hnsw, Item, RangeResult, _as_points, _attr_values, _Everything, _Match,
                  _range_rows, _RestrictedSearch, _rows, _Sets, _table_columns, _Where, allowed_bitmap)
from .dist import shard_range


def _lib():
    return _capi.lib()


class PartitionedHnsw(_RestrictedSearch):
    """An ordered list of `Hnsw` parts with the same dim, metric and ef_search (METRIC_DOT: and the same dot_bound) behind one
    search call."""

    def __init__(self, handle, hnsws: Sequence[Hnsw]):
        self._h = handle
        self.parts = list(hnsws)      # kept alive for as long as the C handle exists (it borrows them)
        info = self.info()
        self._base = np.array(info.base[: info.n_parts + 1], dtype=np.int64)

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None:
                _lib().idist_partitioned_free(self._h)   # before the parts: their own __del__ frees the indexes
                self._h = None
        except Exception:
            pass

    # -- construction --
    @classmethod
    def from_hnsws(cls, hnsws: Sequence[Hnsw]) -> "PartitionedHnsw":
        """Adopt existing indexes as parts 0..P-1 (1 <= P <= 64)."""
        hnsws = list(hnsws)
        k = len(hnsws)
        hs = (C.c_void_p * max(k, 1))(*[h._h for h in hnsws])
        out = C.c_void_p()
        L = _lib()
        L.check(L.idist_partitioned_new(hs, k, C.byref(out)))
        return cls(out, hnsws)

    @classmethod
    def build(cls, points, builder: Builder | None = None, parts: int = 2,
              devices: Sequence[int] | None = None) -> tuple["PartitionedHnsw", list[int]]:
        """Cut `points` into `parts` contiguous ranges (dist.shard_range), build an ordinary `Hnsw` of each with `builder`
        (its seed drives every part's own shuffle) on devices[p % len(devices)] (default: all on the builder's device).
        Parts on different devices build side by side, one host thread per distinct device; parts that share a device
        one after the other.  Returns (index, caller's row index -> global id), as `Builder.build_hnsw` does for PointIds."""
        builder = builder or Builder()
        pts = _as_points(points)
        n = pts.shape[0]
        P = int(parts)
        if builder._metric == METRIC_DOT and builder._dot_bound == 0.0 and n:
            # one query augmentation and one report serve all parts: every part is built with the bound of the WHOLE set
            S = C.c_float(0.0)
            L = _lib()
            L.check(L.idist_dot_augment_batch(_capi.f32p(pts), n, max(pts.shape[1], 1), 0.0, None, None, C.byref(S), builder._device))
            builder = copy.copy(builder).dot_bound(S.value)
        devs = [int(d) for d in devices] if devices else [builder._device]
        hnsws: list = [None] * P
        local: list = [None] * P
        errors: list = []

        def work(device: int, mine: list[int]):
            try:
                b = copy.copy(builder)
                b._device = device
                for p in mine:
                    lo, hi = shard_range(n, p, P)
                    hnsws[p], local[p] = Hnsw._new(pts[lo:hi], b)
            except BaseException as e:  # noqa: BLE001 - handed to the calling thread
                errors.append(e)

        by_dev: dict[int, list[int]] = {}
        for p in range(P):
            by_dev.setdefault(devs[p % len(devs)], []).append(p)
        groups = list(by_dev.items())
        threads = [threading.Thread(target=work, args=g) for g in groups[1:]]
        for t in threads:
            t.start()
        if groups:
            work(*groups[0])
        for t in threads:
            t.join()
        if errors:
            raise errors[0]
        self = cls.from_hnsws(hnsws)
        ids = np.zeros(n, dtype=np.int64)
        for p in range(P):
            lo, hi = shard_range(n, p, P)
            ids[lo:hi] = self._base[p] + np.asarray(local[p], dtype=np.int64)
        return self, [int(x) for x in ids]

    # -- introspection --
    def info(self) -> _capi.PartitionedInfo:
        info = _capi.PartitionedInfo()
        _lib().check(_lib().idist_partitioned_get_info(self._h, C.byref(info)))
        return info

    def last_merge_ms(self) -> float:
        """HIP-event duration of the last merge kernel, milliseconds."""
        ms = C.c_float(0.0)
        _lib().check(_lib().idist_partitioned_last_merge_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def last_search_kernel_ms(self) -> np.ndarray:
        """Per part, the HIP-event duration of its last search kernel (0: empty part, -1: nothing timed), milliseconds."""
        out = np.zeros(64, dtype=np.float32)
        n = C.c_uint32(0)
        _lib().check(_lib().idist_partitioned_last_search_kernel_ms(self._h, _capi.f32p(out), 64, C.byref(n)))
        return out[: n.value]

    def part_of(self, gid: int) -> tuple[int, int]:
        """(part, PointId inside it) of a global id."""
        gid = int(gid)
        if not 0 <= gid < int(self._base[-1]):
            raise IndexError(f"global id {gid} out of range [0, {int(self._base[-1])})")
        p = int(np.searchsorted(self._base, gid, side="right")) - 1
        return p, gid - int(self._base[p])

    def __len__(self):
        return int(self._base[-1])

    def __getitem__(self, gid: int) -> np.ndarray:
        p, pid = self.part_of(gid)
        return self.parts[p].points[pid]

    # -- search --
    def search_batch(self, queries, counters: bool = False) -> BatchResult:
        """Hnsw::search on every part, merged: <= ef_search (global id, distance) pairs per query, nearest first."""
        q = _as_points(queries)
        info = self.info()
        if q.shape[0] and len(self) and q.shape[1] != info.dim:
            raise TypeError(f"query dim {q.shape[1]} != index dim {info.dim}")
        nq, ef = q.shape[0], int(info.ef_search)
        pid = np.full((nq, ef), INVALID, dtype=np.uint32)
        dist = np.full((nq, ef), np.inf, dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint32)
        ctr = np.zeros((nq, 3), dtype=np.uint32) if counters else None
        if nq:
            L = _lib()
            L.check(L.idist_partitioned_search_batch(self._h, _capi.f32p(q), nq, _capi.u32p(pid), _capi.f32p(dist),
                                                     _capi.u32p(cnt), _capi.u32p(ctr) if counters else None))
        return BatchResult(pid, dist, cnt, ctr)

    def search(self, point) -> list[Item]:
        """One query: the merged items, nearest first; `Item.pid` is the global id."""
        return _rows(self.search_batch(np.asarray(point, dtype=np.float32).reshape(1, -1)), self._item)[0]

    def _item(self, distance: float, gid: int) -> Item:
        return Item(distance, gid, self[gid])

    # what `_RestrictedSearch` asks of the index class
    _SEARCH = {(False, _Sets): "idist_partitioned_search_batch_allowed_sets",
               (False, _Where): "idist_partitioned_search_batch_attr",
               (False, _Match): "idist_partitioned_search_batch_match",
               (True, _Everything): "idist_partitioned_search_batch_range",
               (True, _Sets): "idist_partitioned_search_batch_range_allowed_sets",
               (True, _Where): "idist_partitioned_search_batch_range_attr",
               (True, _Match): "idist_partitioned_search_batch_range_match"}
    _FETCH = "idist_partitioned_range_fetch"

    def _lead(self, search=None) -> tuple:
        return (self._h,)

    def _rung_shape(self, nq: int, info) -> tuple:
        return nq, int(info.n_parts)

    def search_allowed_sets(self, queries, sets, set_of, k: int, max_rungs: int = -1, counters: bool = False) -> AllowedResult:
        """The k nearest among an allowed subset, several sets in one call, one per query
        (idist_partitioned_search_batch_allowed_sets): `Hnsw.search_allowed_sets` on every part with the slice of each set that
        falls into it, merged — exactly min(k, allowed points) results per query, global ids.  `sets` names GLOBAL ids: a sequence of
        bool masks of length len(self) or of global-id arrays, a 2-D bool array [n_sets][len(self)] or a ready uint32 bitmap
        [n_sets][(len(self) + 31) // 32].  `set_of`: the set index of every query; None: query q uses set q.  `AllowedResult.rung` has
        shape (nq, n_parts): every part climbs its own ladder (a part that holds none of a query's allowed points answers RUNG_NONE
        at once; one where they are rare scans them exactly)."""
        return self._topk(queries, _Sets(sets, set_of), k, max_rungs, counters)

    def search_allowed(self, queries, allowed, k: int, max_rungs: int = -1, counters: bool = False) -> AllowedResult:
        """`search_allowed_sets` with ONE set shared by the batch: `allowed` is a bool mask of length len(self) or an integer array
        of global ids (`allowed_bitmap`'s rules)."""
        q = _as_points(queries)
        bits = allowed_bitmap(allowed, len(self)).reshape(1, -1)    # (whatever it is: no ready bitmaps here)
        return self.search_allowed_sets(q, bits, np.zeros(q.shape[0], dtype=np.uint32), k, max_rungs=max_rungs, counters=counters)

    def search_one_allowed(self, point, allowed, k: int) -> list[Item]:
        """One query: its min(k, allowed points) nearest allowed items, nearest first; `Item.pid` is the global id."""
        return _rows(self.search_allowed(np.asarray(point, dtype=np.float32).reshape(1, -1), allowed, k), self._item)[0]

    def last_allowed_slice_ms(self) -> float:
        """Host time the last restricted search spent on the bitmaps (the parts' strided uploads + slice kernels), milliseconds;
        after `search_where` / `search_range_where`: the HIP-event time of the parts' bitmap kernels, summed."""
        ms = C.c_float(0.0)
        _lib().check(_lib().idist_partitioned_last_allowed_slice_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def search_range(self, queries, radius, max_rungs: int = -1, max_total: int = 64 * 2**20, counters: bool = False) -> RangeResult:
        """Every point of the whole set within `radius` of each query (idist_partitioned_search_batch_range): `Hnsw.search_range` on
        every part — each climbs its own ladder and ends in its own exact scan — merged on the GPU by (raw distance bits, global id),
        the metric's report applied once, after the merge.  `radius`, `max_rungs` and `max_total` as in `Hnsw.search_range`;
        `max_total` bounds the merged total.  `RangeResult.pid` holds GLOBAL ids, `RangeResult.rung` has shape (nq, n_parts)
        (RUNG_NONE for an empty part), the counters are summed over the parts."""
        return self._range(queries, radius, _Everything(), max_rungs, max_total, counters)

    def search_range_allowed_sets(self, queries, radius, sets, set_of, max_rungs: int = -1, max_total: int = 64 * 2**20,
                                  counters: bool = False) -> RangeResult:
        """`search_range` restricted to one allowed set per query (idist_partitioned_search_batch_range_allowed_sets):
        `Hnsw.search_range_allowed_sets` on every part with the slice of each set that falls into it — every part applies its own
        end rule, climbs its own ladder and ends in its own exact scan — merged on the GPU by (raw distance bits, global id), the
        metric's report applied once, after the merge.  `sets` / `set_of` name GLOBAL ids as in `search_allowed_sets`; `radius`,
        `max_rungs`, `max_total` as in `search_range`, `max_total` bounding the merged restricted total.  `RangeResult.rung` has
        shape (nq, n_parts): RUNG_NONE for an empty part or an empty slice."""
        return self._range(queries, radius, _Sets(sets, set_of), max_rungs, max_total, counters)

    def search_range_allowed(self, queries, radius, allowed, max_rungs: int = -1, max_total: int = 64 * 2**20,
                             counters: bool = False) -> RangeResult:
        """`search_range_allowed_sets` with ONE set shared by the batch: `allowed` is a bool mask of length len(self) or an integer
        array of global ids (`allowed_bitmap`'s rules)."""
        q = _as_points(queries)
        bits = allowed_bitmap(allowed, len(self)).reshape(1, -1)    # (whatever it is: no ready bitmaps here)
        return self.search_range_allowed_sets(q, radius, bits, np.zeros(q.shape[0], dtype=np.uint32), max_rungs, max_total, counters)

    # -- attribute filters --
    def attributes(self, values) -> Attr:
        """One uint32 per point in GLOBAL-id order (the order of a bool `allowed` mask of this index): every non-empty part's slice
        goes to that part's own device, once (idist_partitioned_attr_new).  Values outside uint32 raise."""
        v = _attr_values(values, len(self))
        h = C.c_void_p()
        L = _lib()
        L.check(L.idist_partitioned_attr_new(self._h, _capi.u32p(v), C.byref(h)))
        return Attr(h, self, v)

    def search_where(self, queries, attr: Attr, lo, hi=None, k: int = 10, max_rungs: int = -1, counters: bool = False) -> AllowedResult:
        """The k nearest among the points whose attribute lies in the query's interval lo <= attr <= hi
        (idist_partitioned_search_batch_attr): row q is exactly what `search_allowed_sets` returns for the mask
        `(attr.values >= lo[q]) & (attr.values <= hi[q])` over the global ids; every part makes its bitmaps from its own slice of the
        values on its own device.  `lo` / `hi`: one integer for the batch or an array of one per query; hi=None means equality."""
        return self._topk(queries, _Where(attr, lo, hi), k, max_rungs, counters)

    def search_range_where(self, queries, radius, attr: Attr, lo, hi=None, max_rungs: int = -1, max_total: int = 64 * 2**20,
                           counters: bool = False) -> RangeResult:
        """Every point within `radius` whose attribute lies in the query's interval (idist_partitioned_search_batch_range_attr): row q
        is exactly what `search_range_allowed_sets` returns for the mask of `search_where`."""
        return self._range(queries, radius, _Where(attr, lo, hi), max_rungs, max_total, counters)

    # -- attribute tables --
    def attribute_table(self, columns) -> AttrTable:
        """Several uint32 columns per point in GLOBAL-id order (idist_partitioned_attr_new_columns): every non-empty part's slice of
        every column goes to that part's own device, once.  `columns` as in `Hnsw.attribute_table`."""
        names, cols = _table_columns(columns, len(self))
        h = C.c_void_p()
        L = _lib()
        L.check(L.idist_partitioned_attr_new_columns(self._h, _capi.u32p(cols), len(names), C.byref(h)))
        return AttrTable(h, self, names, cols)

    def search_match(self, queries, table: AttrTable, conds, k: int = 10, max_rungs: int = -1, counters: bool = False) -> AllowedResult:
        """The k nearest among the points that satisfy the query's condition over the table's columns
        (idist_partitioned_search_batch_match): row q is exactly what `search_allowed_sets` returns for the mask of its condition over
        the global ids; every part evaluates the conditions over its own slice of the columns on its own device.  `conds` as in
        `Hnsw.search_match`."""
        return self._topk(queries, _Match(table, conds), k, max_rungs, counters)

    def search_range_match(self, queries, radius, table: AttrTable, conds, max_rungs: int = -1, max_total: int = 64 * 2**20,
                           counters: bool = False) -> RangeResult:
        """Every point within `radius` that satisfies the query's condition (idist_partitioned_search_batch_range_match): row q is
        exactly what `search_range_allowed_sets` returns for the mask of its condition."""
        return self._range(queries, radius, _Match(table, conds), max_rungs, max_total, counters)

    def search_one_range(self, point, radius) -> list[Item]:
        """One query: every item within `radius`, nearest first; `Item.pid` is the global id."""
        return _range_rows(self.search_range(np.asarray(point, dtype=np.float32).reshape(1, -1), float(radius)), self._item)[0]

    def last_range_merge_ms(self) -> float:
        """HIP-event duration of the last range search's counts, prefix-sum and merge kernels, milliseconds."""
        ms = C.c_float(0.0)
        _lib().check(_lib().idist_partitioned_last_range_merge_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def bruteforce(self, queries, k: int) -> tuple[np.ndarray, np.ndarray]:
        """Exact k-NN over all parts (global ids, ties by id): every part's exhaustive scan, merged."""
        q = _as_points(queries)
        pid = np.full((q.shape[0], k), INVALID, dtype=np.uint32)
        dist = np.full((q.shape[0], k), np.inf, dtype=np.float32)
        L = _lib()
        L.check(L.idist_partitioned_bruteforce(self._h, _capi.f32p(q), q.shape[0], k, _capi.u32p(pid), _capi.f32p(dist)))
        return pid, dist
