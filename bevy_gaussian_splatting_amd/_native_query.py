"""ctypes binding of libbgs_query.so (the C ABI in include/bgs_query.h): point-in-mesh selection on the device.

What is specific to this library: its status codes, prototype table and version handshake. The library is built in-tree
(`make -C bevy_gaussian_splatting_amd/csrc_query`; `__graft_entry__.build()` does it), and `load()` keeps it the one
built from this tree's sources through `_loader` + `_build_id`, as `_native.load()` does for libbgs.so. There is no CPU
fallback."""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_char_p, c_float, c_int
from typing import Optional

from . import _build_id, _loader

SPEC = _build_id.LIBBGS_QUERY
LIB_PATH = SPEC.path

BGSQ_OK = 0
BGSQ_EINVAL = -1
BGSQ_ENOMEM = -2
BGSQ_EHIP = -3
BGSQ_KEEP_INSIDE = 0
BGSQ_KEEP_OUTSIDE = 1
ABI_VERSION = (0 << 16) | 1

vp, u32 = ctypes.c_void_p, ctypes.c_uint32

# Every function include/bgs_query.h declares, in its order: (name, restype, argtypes). Held against the header by
# tests/test_native_binding.py (names, parameter counts, return types).
PROTOTYPES = (
    ("bgsq_version", u32, ()),
    ("bgsq_last_error", c_char_p, ()),
    ("bgsq_mesh_create", c_int, (c_int, vp, u32, vp, u32, POINTER(vp))),
    ("bgsq_mesh_free", None, (vp,)),
    ("bgsq_mesh_triangles", u32, (vp,)),
    ("bgsq_crossings", c_int, (vp, vp, vp, u32, POINTER(c_float), vp)),
    ("bgsq_entries_keep", c_int, (c_int, vp, vp, u32, vp, u32, u32)),
    ("bgsq_debug_set_slices", c_int, (vp, u32)),
)
EXPORTED_SYMBOLS = tuple(name for name, _, _ in PROTOTYPES)


class BgsQueryError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libbgs_query error {status}: {message}")
        self.status = status


_lib: Optional[ctypes.CDLL] = None


def load() -> ctypes.CDLL:
    """Load libbgs_query.so once and declare prototypes. Raises if it is not built from this tree's sources and cannot
    be rebuilt."""
    global _lib
    if _lib is None:
        _lib = _loader.open_library(SPEC, LIB_PATH, PROTOTYPES, "bgsq_version", ABI_VERSION)
    return _lib


def check(lib: ctypes.CDLL, status: int) -> None:
    _loader.check_status(status, lib.bgsq_last_error, BgsQueryError)
