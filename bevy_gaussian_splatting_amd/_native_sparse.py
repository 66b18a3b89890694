"""ctypes binding of libbgs_sparse.so (the C ABI in include/bgs_sparse.h): sparse-splat selection on the device.

What is specific to this library: its status codes, prototype table and version handshake. The library is built in-tree
(`make -C bevy_gaussian_splatting_amd/csrc_sparse`; `__graft_entry__.build()` does it), and `load()` keeps it the one
built from this tree's sources through `_loader` + `_build_id`, as `_native.load()` does for libbgs.so. There is no CPU
fallback."""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_char_p, c_float, c_int
from typing import Optional

from . import _build_id, _loader

SPEC = _build_id.LIBBGS_SPARSE
LIB_PATH = SPEC.path

BGSS_OK = 0
BGSS_EINVAL = -1
BGSS_ENOMEM = -2
BGSS_EHIP = -3
BGSS_KEEP_SPARSE = 0
BGSS_KEEP_DENSE = 1
ABI_VERSION = (0 << 16) | 1

vp, u32 = ctypes.c_void_p, ctypes.c_uint32

# Every function include/bgs_sparse.h declares, in its order: (name, restype, argtypes). Held against the header by
# tests/test_native_binding.py (names, order, parameter counts, return types).
PROTOTYPES = (
    ("bgss_version", u32, ()),
    ("bgss_last_error", c_char_p, ()),
    ("bgss_grid_create", c_int, (c_int, u32, POINTER(vp))),
    ("bgss_grid_free", None, (vp,)),
    ("bgss_grid_capacity", u32, (vp,)),
    ("bgss_neighbor_counts", c_int, (vp, vp, vp, u32, c_float, u32, vp)),
    ("bgss_entries_keep", c_int, (c_int, vp, vp, u32, vp, u32, u32, u32)),
    ("bgss_debug_set_table_bits", c_int, (vp, u32)),
)
EXPORTED_SYMBOLS = tuple(name for name, _, _ in PROTOTYPES)


class BgsSparseError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libbgs_sparse error {status}: {message}")
        self.status = status


_lib: Optional[ctypes.CDLL] = None


def load() -> ctypes.CDLL:
    """Load libbgs_sparse.so once and declare prototypes. Raises if it is not built from this tree's sources and cannot
    be rebuilt."""
    global _lib
    if _lib is None:
        _lib = _loader.open_library(SPEC, LIB_PATH, PROTOTYPES, "bgss_version", ABI_VERSION)
    return _lib


def check(lib: ctypes.CDLL, status: int) -> None:
    _loader.check_status(status, lib.bgss_last_error, BgsSparseError)
