"""Sparse-splat selection (src/query/sparse.rs): which splats have fewer than `neighbor_threshold` splats within `radius`
of them, themselves included — the floaters of a trained asset.

The counting runs on the device (`bgss_neighbor_counts`, csrc_sparse/sparse_kernels.hip, through libbgs_sparse.so) on
points and entries that live in device memory; this module holds the component `SparseSelect`, the ctypes wrapper
`SparseGrid`, and `neighbor_counts_reference`, a numpy twin of the arithmetic contract (csrc_sparse/sparse_math.h) that
the tests compare the device with bit for bit. The twin tests all n x n pairs; the device's grid must give the same.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _native_sparse

KEEP_SPARSE = _native_sparse.BGSS_KEEP_SPARSE
KEEP_DENSE = _native_sparse.BGSS_KEEP_DENSE
CULLED_KEY = 0xFFFFFFFF


@dataclass(frozen=True)
class SparseSelect:
    """The reference's component, with its defaults (sparse.rs:25-38)."""
    radius: float = 0.05
    neighbor_threshold: int = 3


def radius_squared(radius) -> np.float32:
    """radius * radius in float32, rounded once; what `bgss_neighbor_counts` refuses is refused here in its words."""
    r = np.float32(radius)
    with np.errstate(all="ignore"):
        r2 = r * r
    assert r2.dtype == np.float32
    if not np.isfinite(r) or not r > 0:
        raise ValueError(f"radius {float(r):g} must be finite and positive")
    if not r2 > 0 or not np.isfinite(r2):
        raise ValueError(f"radius {float(r):g} has the square {float(r2):g} in f32")
    return r2


def neighbor_counts_reference(points, radius, cap: int = 0, block: int = 1024) -> np.ndarray:
    """The neighbour counts as the device reports them (csrc_sparse/sparse_math.h): all pairs, op by op in float32, every
    operation rounded once. `points` is [n, 3] or [n, 4] (xyz read). Returns uint32 [n]."""
    p = np.asarray(points, np.float32)
    r2 = radius_squared(radius)
    n = p.shape[0]
    out = np.zeros(n, np.uint32)
    if n == 0:
        return out
    x, y, z = (np.ascontiguousarray(p[:, k]) for k in range(3))
    zero = np.float32(0.0)
    with np.errstate(all="ignore"):
        for lo in range(0, n, block):
            d = x[None, :] - x[lo:lo + block, None]       # dx = x_j - x_i, row i, column j
            np.multiply(d, d, out=d)
            d2 = zero + d
            for lane in (y, z):
                d = lane[None, :] - lane[lo:lo + block, None]
                np.multiply(d, d, out=d)
                np.add(d2, d, out=d2)
            assert d.dtype == d2.dtype == np.float32
            out[lo:lo + block] = (d2 < r2).sum(axis=1, dtype=np.uint32)
    if cap:
        np.minimum(out, np.uint32(cap), out=out)
    return out


def selected_indices(counts: np.ndarray, neighbor_threshold: int) -> np.ndarray:
    """Ascending indices of the points with counts < neighbor_threshold: the reference's `Select.indicies`."""
    return np.flatnonzero(np.asarray(counts) < np.uint32(neighbor_threshold)).astype(np.uint32)


def select_reference(points, radius, neighbor_threshold: int) -> np.ndarray:
    return selected_indices(neighbor_counts_reference(points, radius), neighbor_threshold)


def keep_reference(entries: np.ndarray, counts: np.ndarray, neighbor_threshold: int, dense: bool = False) -> np.ndarray:
    """`bgss_entries_keep` on host entries: a copy in which every entry with index < n and a live key whose point fails
    the predicate has key 0xFFFFFFFF. Index and order are untouched."""
    e = np.array(entries, copy=True)
    n = counts.shape[0]
    named = (e["index"] < n) & (e["key"] != CULLED_KEY)
    sparse = np.zeros(e.shape[0], bool)
    sparse[named] = counts[e["index"][named]] < np.uint32(neighbor_threshold)
    e["key"][named & (sparse == bool(dense))] = CULLED_KEY
    return e


class SparseGrid:
    """The device scratch of the counting stages (`bgss_grid`) for clouds of up to `max_points`, allocated once and held
    until `free()`. `neighbor_counts` and `entries_keep` only enqueue on the stream they are given; one grid serves one
    stream at a time."""

    def __init__(self, max_points: int, device: int = 0):
        if not 0 <= int(max_points) <= 0xFFFFFFFF:
            raise ValueError("max_points must fit in uint32")
        self._lib = _native_sparse.load()
        self.device = int(device)
        out = ctypes.c_void_p()
        _native_sparse.check(self._lib, self._lib.bgss_grid_create(self.device, int(max_points), ctypes.byref(out)))
        self._ptr: Optional[ctypes.c_void_p] = out

    def free(self) -> None:
        if getattr(self, "_ptr", None) is not None:
            self._lib.bgss_grid_free(self._ptr)
            self._ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def _grid(self):
        if self._ptr is None:
            raise ValueError("the grid has been freed")
        return self._ptr

    @property
    def capacity(self) -> int:
        return int(self._lib.bgss_grid_capacity(self._grid()))

    def set_table_bits(self, bits: int) -> None:
        """`bgss_debug_set_table_bits` (test hook): 0 = automatic."""
        _native_sparse.check(self._lib, self._lib.bgss_debug_set_table_bits(self._grid(), int(bits)))

    def neighbor_counts(self, stream: int, points_ptr: int, n: int, radius: float, counts_ptr: int, cap: int = 0) -> None:
        """Enqueue `bgss_neighbor_counts` on `stream`: n points (float4, xyz read) at `points_ptr`, n uint32 out at
        `counts_ptr`."""
        _native_sparse.check(self._lib, self._lib.bgss_neighbor_counts(
            self._grid(), ctypes.c_void_p(stream or 0), ctypes.c_void_p(points_ptr or 0), int(n), ctypes.c_float(radius), int(cap),
            ctypes.c_void_p(counts_ptr or 0)))

    def entries_keep(self, stream: int, entries_ptr: int, entry_count: int, counts_ptr: int, n: int, neighbor_threshold: int,
                     dense: bool = False) -> None:
        """Enqueue `bgss_entries_keep` on `stream`."""
        _native_sparse.check(self._lib, self._lib.bgss_entries_keep(
            self.device, ctypes.c_void_p(stream or 0), ctypes.c_void_p(entries_ptr or 0), int(entry_count),
            ctypes.c_void_p(counts_ptr or 0), int(n), int(neighbor_threshold), KEEP_DENSE if dense else KEEP_SPARSE))
