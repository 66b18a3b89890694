"""ctypes binding of libbgs_slice.so (the C ABI in include/bgs_slice.h): the time slice of a 4D cloud on the device.

What is specific to this library: its status codes, prototype table and version handshake. The library is built in-tree
(`make -C bevy_gaussian_splatting_amd/csrc_slice`; `__graft_entry__.build()` does it), and `load()` keeps it the one
built from this tree's sources through `_loader` + `_build_id`, as `_native.load()` does for libbgs.so. There is no CPU
fallback."""
from __future__ import annotations

import ctypes
from ctypes import c_char_p, c_float, c_int
from typing import Optional

from . import _build_id, _loader

SPEC = _build_id.LIBBGS_SLICE
LIB_PATH = SPEC.path

BGST_OK = 0
BGST_EINVAL = -1
BGST_ENOMEM = -2
BGST_EHIP = -3
ABI_VERSION = (0 << 16) | 1

vp, u32 = ctypes.c_void_p, ctypes.c_uint32

# Every function include/bgs_slice.h declares, in its order: (name, restype, argtypes). Held against the header by
# tests/test_native_binding.py (names, order, parameter counts, return types).
PROTOTYPES = (
    ("bgst_version", u32, ()),
    ("bgst_last_error", c_char_p, ()),
    ("bgst_slice", c_int, (c_int, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, c_float, c_float, c_float, c_float)),
)
EXPORTED_SYMBOLS = tuple(name for name, _, _ in PROTOTYPES)


class BgsSliceError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libbgs_slice error {status}: {message}")
        self.status = status


_lib: Optional[ctypes.CDLL] = None


def load() -> ctypes.CDLL:
    """Load libbgs_slice.so once and declare prototypes. Raises if it is not built from this tree's sources and cannot
    be rebuilt."""
    global _lib
    if _lib is None:
        _lib = _loader.open_library(SPEC, LIB_PATH, PROTOTYPES, "bgst_version", ABI_VERSION)
    return _lib


def check(lib: ctypes.CDLL, status: int) -> None:
    _loader.check_status(status, lib.bgst_last_error, BgsSliceError)
