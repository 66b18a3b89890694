"""Build identity of the package's native libraries: what each one is, the SHA-256 of the sources it is built from, and
the id a built library carries.

Each library's Makefile runs this file and compiles the hash into the library as the byte string `<MARKER><hex>`, where
it can be read without loading the library (libbgs.so also returns it from `bgs_build_id()`). `_loader.ensure_current`
rebuilds a library that carries another id and refuses one it cannot rebuild, so a stale prebuilt binary can never be
what the tests or `bench.py` ran. Counter files under `profiles/` are stamped with libbgs's hash. Not the commit id:
that also changes with every documentation commit.

What a hash covers is data of the library's description, and part of the id: change a recipe and every library built
before is stale.

`LIBRARIES` is the one table of them, in build order: libbgs, then the four small libraries, whose specs come from one
constructor and whose hashes also cover what they share (small_lib/). A further library is one more line there.

`python bevy_gaussian_splatting_amd/_build_id.py [NAME]` prints the hash of the library of `LIBRARIES` so named (libbgs's
by default). Standard library only and no relative import: the Makefiles run it as a plain script, and
scripts/build_*_variant.sh copy this one file next to a bare csrc/."""
from __future__ import annotations

import hashlib
import os
import sys
from dataclasses import dataclass
from typing import Optional, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))


@dataclass(frozen=True)
class NativeLibrary:
    name: str                                   # this file's argument; the library file is <name>.so
    source_dir: str                             # holds the Makefile, the sources, the built library and the build lock
    marker: bytes                               # the id stands behind it in the library's bytes
    hashed_suffixes: Tuple[str, ...]            # the hash covers source_dir's files that end so, and its Makefile ...
    hashed_elsewhere: Tuple[Tuple[str, str], ...] = ()   # ... then these (label, path from source_dir), as listed
    make_args: Tuple[str, ...] = ()             # between `make -C source_dir` and ARCH=gfx950
    dlopen_mode: int = os.RTLD_LOCAL

    @property
    def path(self) -> str:
        return os.path.join(self.source_dir, self.name + ".so")


# The compiler flags are in the Makefile and the Makefile is in the hash. build_id.inc is generated FROM the hash and
# is no source. libbgs's recipe leaves out libbgs.map and include/bgs*.h, and stays so: adding them would move its id.
LIBBGS = NativeLibrary("libbgs", os.path.join(_HERE, "csrc"), b"BGS_BUILD_ID=", (".hip", ".h"),
                       make_args=("-j4",), dlopen_mode=os.RTLD_GLOBAL)


def _small_library(name: str, directory: str, marker: bytes, header: str) -> NativeLibrary:
    """A small device library: its own directory with its map file, its public header under include/, then what all of
    them are built with (small_lib/: the API support headers and the Makefile recipe, where the compiler flags are)."""
    elsewhere = [(header, os.path.join("..", "..", "include", header))]
    elsewhere += [(shared, os.path.join("..", "small_lib", shared)) for shared in ("api_support.h", "api_support_hip.h", "library.mk")]
    return NativeLibrary(name, os.path.join(_HERE, directory), marker, (".hip", ".h", ".map"), hashed_elsewhere=tuple(elsewhere))


LIBBGS_QUERY = _small_library("libbgs_query", "csrc_query", b"BGSQ_BUILD_ID=", "bgs_query.h")     # point-in-mesh selection
LIBBGS_SPARSE = _small_library("libbgs_sparse", "csrc_sparse", b"BGSS_BUILD_ID=", "bgs_sparse.h")  # sparse-splat selection
LIBBGS_SLICE = _small_library("libbgs_slice", "csrc_slice", b"BGST_BUILD_ID=", "bgs_slice.h")      # the time slice of a 4D cloud
LIBBGS_MORPH = _small_library("libbgs_morph", "csrc_morph", b"BGSM_BUILD_ID=", "bgs_morph.h")      # the morph between two clouds
# Every native library, in build order; this file's argument names one of them.
LIBRARIES = {spec.name: spec for spec in (LIBBGS, LIBBGS_QUERY, LIBBGS_SPARSE, LIBBGS_SLICE, LIBBGS_MORPH)}
MARKER = LIBBGS.marker


def source_sha256(spec: NativeLibrary) -> str:
    """For every covered name in sorted order, the name then the file's bytes; then the same for the files elsewhere."""
    covered = [(name, name) for name in sorted(os.listdir(spec.source_dir))
               if name.endswith(spec.hashed_suffixes) or name == "Makefile"]
    h = hashlib.sha256()
    for label, path in covered + list(spec.hashed_elsewhere):
        h.update(label.encode())
        with open(os.path.join(spec.source_dir, path), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def kernel_source_sha256() -> str:
    return source_sha256(LIBBGS)


def library_build_id(path: str, spec: NativeLibrary = LIBBGS) -> Optional[str]:
    """The id compiled into a built library, read from the file's bytes (no dlopen); None if the file is missing or
    carries none."""
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError:
        return None
    at = data.find(spec.marker)
    while at >= 0:
        hexid = data[at + len(spec.marker): at + len(spec.marker) + 64]
        if len(hexid) == 64 and all(c in b"0123456789abcdef" for c in hexid):
            return hexid.decode()
        at = data.find(spec.marker, at + 1)
    return None


if __name__ == "__main__":
    print(source_sha256(LIBRARIES[sys.argv[1]] if len(sys.argv) > 1 else LIBBGS))
