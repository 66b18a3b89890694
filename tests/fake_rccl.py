"""The tests' stand-in for librccl (tests/host_shim/fake_rccl.cpp): built like the other host shims, reached by libbgs
through BGS_RCCL_LIBRARY (an absolute path, nothing is preloaded), and opened a second time by the test itself, which
gets the same loaded object and with it the stand-in's queries. Not a product path."""
from __future__ import annotations

import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_shim", "fake_rccl.cpp")
LIB = os.path.join(HERE, "host_shim", "libfake_rccl.so")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
GXX_FLAGS = ["-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include")]

NCCL_UINT8 = 1            # ncclDataType_t
NCCL_INVALID_ARGUMENT = 4  # ncclResult_t
NCCL_INVALID_USAGE = 5
ID_BYTES = 128


class CommInfo(ctypes.Structure):
    """fake_rccl_comm_info."""

    _fields_ = [("gather_calls", ctypes.c_uint64), ("gathers_completed", ctypes.c_uint64), ("last_count", ctypes.c_uint64),
                ("last_stream", ctypes.c_uint64), ("last_datatype", ctypes.c_int32), ("last_root", ctypes.c_int32),
                ("last_result", ctypes.c_int32), ("nranks", ctypes.c_int32)]


class UniqueId(ctypes.Structure):
    """ncclUniqueId: passed BY VALUE to ncclCommInitRank."""

    _fields_ = [("internal", ctypes.c_char * ID_BYTES)]


def build() -> str:
    """g++ the stand-in against the HIP runtime (host code only) if it is missing or older than its source. Returns the
    library's absolute path: what BGS_RCCL_LIBRARY is set to."""
    if not os.path.exists(LIB) or os.path.getmtime(SRC) > os.path.getmtime(LIB):
        libdir = os.path.join(ROCM, "lib")
        subprocess.run(["g++", *GXX_FLAGS, "-shared", "-fPIC", SRC, "-o", LIB, "-L" + libdir, "-Wl,-rpath," + libdir, "-lamdhip64"],
                       check=True, capture_output=True)
    return LIB


def load() -> ctypes.CDLL:
    """The stand-in with its prototypes: the queries, and the nccl* calls the host tests make themselves."""
    lib = ctypes.CDLL(build())
    vp = ctypes.c_void_p
    for name, res, args in (("fake_rccl_live_comms", ctypes.c_int, []),
                            ("fake_rccl_comm_query", ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(CommInfo)]),
                            ("fake_rccl_pending_posts", ctypes.c_uint64, []),
                            ("ncclGetUniqueId", ctypes.c_int, [ctypes.POINTER(UniqueId)]),
                            ("ncclCommInitRank", ctypes.c_int, [ctypes.POINTER(vp), ctypes.c_int, UniqueId, ctypes.c_int]),
                            ("ncclCommDestroy", ctypes.c_int, [vp]),
                            ("ncclGather", ctypes.c_int, [vp, vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, vp, vp]),
                            ("ncclGetErrorString", ctypes.c_char_p, [ctypes.c_int])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def comm_info(lib: ctypes.CDLL, unique_id: bytes, rank: int) -> CommInfo:
    """What the stand-in recorded for the live communicator (id, rank)."""
    out = CommInfo()
    assert len(unique_id) == ID_BYTES
    assert lib.fake_rccl_comm_query(unique_id, int(rank), ctypes.byref(out)) == 0, f"the stand-in has no communicator of rank {rank}"
    return out
