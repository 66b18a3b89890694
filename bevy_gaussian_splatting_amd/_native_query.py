"""ctypes binding of libbgs_query.so (the C ABI in include/bgs_query.h): point-in-mesh selection on the device.

The library is built in-tree (`make -C bevy_gaussian_splatting_amd/csrc_query`; `__graft_entry__.build()` does it) and
carries the SHA-256 of the sources it was compiled from as the byte string `BGSQ_BUILD_ID=<hex>`. `load()` rebuilds a
library that is missing or stale (unless BGS_NO_AUTOBUILD=1) and refuses one that still does not match, in the way
`_native.load()` treats libbgs.so. There is no CPU fallback.

`python bevy_gaussian_splatting_amd/_native_query.py` prints the hash (used by csrc_query/Makefile)."""
from __future__ import annotations

import ctypes
import hashlib
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC_QUERY = os.path.join(_HERE, "csrc_query")
HEADER = os.path.join(_HERE, "..", "include", "bgs_query.h")
LIB_PATH = os.path.join(CSRC_QUERY, "libbgs_query.so")
MARKER = b"BGSQ_BUILD_ID="

BGSQ_OK = 0
BGSQ_EINVAL = -1
BGSQ_ENOMEM = -2
BGSQ_EHIP = -3
BGSQ_KEEP_INSIDE = 0
BGSQ_KEEP_OUTSIDE = 1
ABI_VERSION = (0 << 16) | 1

# every symbol include/bgs_query.h declares (tests check the library exports exactly these)
EXPORTED_SYMBOLS = (
    "bgsq_version",
    "bgsq_last_error",
    "bgsq_mesh_create",
    "bgsq_mesh_free",
    "bgsq_mesh_triangles",
    "bgsq_crossings",
    "bgsq_entries_keep",
    "bgsq_debug_set_slices",
)


class BgsQueryError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libbgs_query error {status}: {message}")
        self.status = status


def source_sha256() -> str:
    """SHA-256 over csrc_query's sources (*.hip, *.h, the version script, the Makefile with the compiler flags) and
    include/bgs_query.h."""
    h = hashlib.sha256()
    for name in sorted(os.listdir(CSRC_QUERY)):
        if name.endswith((".hip", ".h", ".map")) or name == "Makefile":   # (build_id.inc is generated FROM this hash)
            h.update(name.encode())
            with open(os.path.join(CSRC_QUERY, name), "rb") as f:
                h.update(f.read())
    h.update(b"bgs_query.h")
    with open(HEADER, "rb") as f:
        h.update(f.read())
    return h.hexdigest()


def library_build_id(path: str) -> Optional[str]:
    """The id compiled into a libbgs_query.so, read from the file's bytes (no dlopen); None if there is none."""
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError:
        return None
    at = data.find(MARKER)
    while at >= 0:
        hexid = data[at + len(MARKER): at + len(MARKER) + 64]
        if len(hexid) == 64 and all(c in b"0123456789abcdef" for c in hexid):
            return hexid.decode()
        at = data.find(MARKER, at + 1)
    return None


def rebuild() -> str:
    """`make -C csrc_query` (hipcc cross-compiles gfx950 without a GPU). Returns the build log; raises on failure."""
    import subprocess
    p = subprocess.run(["make", "-C", CSRC_QUERY, "ARCH=gfx950"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise ImportError(f"building libbgs_query.so failed:\n{p.stdout}")
    return p.stdout


def ensure_current() -> str:
    """The library on disk must have been compiled from this tree's sources: one that is missing or stale is rebuilt (one
    builder at a time, under a file lock), and anything that still does not match is refused. Returns the id."""
    want = source_sha256()
    have = library_build_id(LIB_PATH)
    if have != want and os.environ.get("BGS_NO_AUTOBUILD", "0") != "1":
        import fcntl
        with open(os.path.join(CSRC_QUERY, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            try:
                have = library_build_id(LIB_PATH)
                if have != want:
                    rebuild()
                    have = library_build_id(LIB_PATH)
            finally:
                fcntl.flock(lock, fcntl.LOCK_UN)
    if have is None:
        raise ImportError(f"{LIB_PATH} not found (or it carries no build id): build it first "
                          "(make -C bevy_gaussian_splatting_amd/csrc_query); there is no CPU fallback")
    if have != want:
        raise ImportError(f"{LIB_PATH} was built from sources {have[:12]}, this tree is {want[:12]}: rebuild it "
                          "(make -C bevy_gaussian_splatting_amd/csrc_query)")
    return want


_lib: Optional[ctypes.CDLL] = None


def load() -> ctypes.CDLL:
    """Load libbgs_query.so once and declare prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    ensure_current()
    lib = ctypes.CDLL(LIB_PATH)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.bgsq_version.argtypes = []
    lib.bgsq_version.restype = u32
    lib.bgsq_last_error.argtypes = []
    lib.bgsq_last_error.restype = ctypes.c_char_p
    lib.bgsq_mesh_create.argtypes = [ctypes.c_int, vp, u32, vp, u32, ctypes.POINTER(vp)]
    lib.bgsq_mesh_create.restype = ctypes.c_int
    lib.bgsq_mesh_free.argtypes = [vp]
    lib.bgsq_mesh_free.restype = None
    lib.bgsq_mesh_triangles.argtypes = [vp]
    lib.bgsq_mesh_triangles.restype = u32
    lib.bgsq_crossings.argtypes = [vp, vp, vp, u32, ctypes.POINTER(ctypes.c_float), vp]
    lib.bgsq_crossings.restype = ctypes.c_int
    lib.bgsq_entries_keep.argtypes = [ctypes.c_int, vp, vp, u32, vp, u32, u32]
    lib.bgsq_entries_keep.restype = ctypes.c_int
    lib.bgsq_debug_set_slices.argtypes = [vp, u32]
    lib.bgsq_debug_set_slices.restype = ctypes.c_int
    if lib.bgsq_version() != ABI_VERSION:
        raise ImportError(f"libbgs_query.so is version {lib.bgsq_version():#x}, this binding was written against {ABI_VERSION:#x}")
    _lib = lib
    return lib


def check(lib: ctypes.CDLL, status: int) -> None:
    if status != BGSQ_OK:
        msg = lib.bgsq_last_error()
        raise BgsQueryError(status, msg.decode("utf-8", "replace") if msg else "")


if __name__ == "__main__":
    print(source_sha256())
