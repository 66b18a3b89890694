"""ctypes binding of libbgs_morph.so (the C ABI in include/bgs_morph.h): the morph between two clouds on the device.

What is specific to this library: its status codes, prototype table and version handshake. The library is built in-tree
(`make -C bevy_gaussian_splatting_amd/csrc_morph`; `__graft_entry__.build()` does it), and `load()` keeps it the one
built from this tree's sources through `_loader` + `_build_id`, as `_native.load()` does for libbgs.so. There is no CPU
fallback."""
from __future__ import annotations

import ctypes
from ctypes import c_char_p, c_float, c_int
from typing import Optional

from . import _build_id, _loader

SPEC = _build_id.LIBBGS_MORPH
LIB_PATH = SPEC.path

BGSM_OK = 0
BGSM_EINVAL = -1
BGSM_ENOMEM = -2
BGSM_EHIP = -3
ABI_VERSION = (0 << 16) | 1

vp, u32 = ctypes.c_void_p, ctypes.c_uint32

# Every function include/bgs_morph.h declares, in its order: (name, restype, argtypes). Held against the header by
# tests/test_native_binding.py (names, order, parameter counts, return types).
PROTOTYPES = (
    ("bgsm_version", u32, ()),
    ("bgsm_last_error", c_char_p, ()),
    ("bgsm_interpolate_f32", c_int, (c_int, vp, u32) + (vp,) * 12 + (c_float,) * 3),
    ("bgsm_interpolate_cov3d_f32", c_int, (c_int, vp, u32) + (vp,) * 9 + (c_float,) * 3),
)
EXPORTED_SYMBOLS = tuple(name for name, _, _ in PROTOTYPES)


class BgsMorphError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libbgs_morph error {status}: {message}")
        self.status = status


_lib: Optional[ctypes.CDLL] = None


def load() -> ctypes.CDLL:
    """Load libbgs_morph.so once and declare prototypes. Raises if it is not built from this tree's sources and cannot
    be rebuilt."""
    global _lib
    if _lib is None:
        _lib = _loader.open_library(SPEC, LIB_PATH, PROTOTYPES, "bgsm_version", ABI_VERSION)
    return _lib


def check(lib: ctypes.CDLL, status: int) -> None:
    _loader.check_status(status, lib.bgsm_last_error, BgsMorphError)
