"""What the bindings of the native libraries (`_native` and the `_native_*` of the small libraries) share: a library on
disk is the one built from this tree's sources (`_build_id`) or it is rebuilt, one builder at a time; failing that it is
refused. The prototypes of a loaded library come from one table. And a small library's binding opens its library with
`open_library` and turns a status into its exception with `check_status`: what is left in the binding is the table, the
constants and the error class. There is no CPU fallback."""
from __future__ import annotations

import ctypes
import fcntl
import os
import subprocess
from typing import Callable, Iterable, Optional, Sequence, Tuple

from . import _build_id
from ._build_id import NativeLibrary

# (name, restype, argtypes): one row per function, in the order of the header that declares it
Prototype = Tuple[str, Optional[type], Sequence[type]]


def rebuild(spec: NativeLibrary) -> str:
    """`make` in the library's source directory (hipcc cross-compiles gfx950 without a GPU). Returns the build log;
    raises on failure."""
    p = subprocess.run(["make", "-C", spec.source_dir, *spec.make_args, "ARCH=gfx950"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise ImportError(f"building {spec.name}.so failed:\n{p.stdout}")
    return p.stdout


def ensure_current(spec: NativeLibrary, path: str) -> str:
    """The library at `path` must have been compiled from THIS tree's sources: one that is missing or stale is rebuilt
    (unless BGS_NO_AUTOBUILD=1), and anything that still does not match is refused. Returns the id."""
    want = _build_id.source_sha256(spec)
    have = _build_id.library_build_id(path, spec)
    if have != want and os.environ.get("BGS_NO_AUTOBUILD", "0") != "1":
        # One builder at a time: bench.py's ranks and pytest-xdist workers import the package concurrently, and N
        # `make` processes in one directory corrupt each other's objects. The id is looked at again under the lock —
        # whoever waited finds the library its predecessor built.
        with open(os.path.join(spec.source_dir, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            try:
                have = _build_id.library_build_id(path, spec)
                if have != want:
                    rebuild(spec)
                    have = _build_id.library_build_id(path, spec)
            finally:
                fcntl.flock(lock, fcntl.LOCK_UN)
    make = f"make -C {spec.source_dir}"
    if have is None:
        raise ImportError(f"{path} not found (or it carries no build id): build it first ({make}, or "
                          "python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
    if have != want:
        raise ImportError(f"{path} was built from sources {have[:12]}, this tree is {want[:12]}: rebuild it ({make})")
    return want


def declare(lib: ctypes.CDLL, prototypes: Iterable[Prototype]) -> None:
    """Give every function of the table its prototype. A name the library does not export is an AttributeError."""
    for name, restype, argtypes in prototypes:
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = list(argtypes)


def open_library(spec: NativeLibrary, path: str, prototypes: Sequence[Prototype], version_function: str, abi_version: int) -> ctypes.CDLL:
    """A small library's `load()`: the library at `path` is made current, opened, given its prototypes, and asked for the
    version of its ABI, which must be the one the binding was written against."""
    ensure_current(spec, path)
    lib = ctypes.CDLL(path, mode=spec.dlopen_mode)
    declare(lib, prototypes)
    version = getattr(lib, version_function)()
    if version != abi_version:
        raise ImportError(f"{spec.name}.so is version {version:#x}, this binding was written against {abi_version:#x}")
    return lib


def check_status(status: int, last_error: Callable[[], Optional[bytes]], error_class: type) -> None:
    """A small library's `check()`: a status other than 0 is raised as `error_class(status, the library's last error)`."""
    if status != 0:
        msg = last_error()
        raise error_class(status, msg.decode("utf-8", "replace") if msg else "")
