"""The frame gather's seam to RCCL (csrc/bgs_comm.hip), the part that needs no GPU: the build without the RCCL header, the
values that build restates, and the stand-in the GPU tests put behind BGS_RCCL_LIBRARY (tests/host_shim/fake_rccl.cpp): it
builds, and its rules for ids and ranks, which touch no device, hold."""
import ctypes
import os
import re
import subprocess

import pytest

import fake_rccl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bevy_gaussian_splatting_amd", "csrc")
RCCL_HEADER = os.path.join(fake_rccl.ROCM, "include", "rccl", "rccl.h")


def makefile_variable(name: str) -> str:
    """`NAME ?= value` of csrc/Makefile."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(rf"^{name}\s*\??=\s*(.*)$", text, re.M).group(1).strip()


def test_bgs_comm_compiles_without_the_rccl_header(tmp_path):
    """A ROCm install without the RCCL development headers builds libbgs: -DBGS_NO_RCCL_HEADER takes the branch such an
    install takes, with the Makefile's own compiler and flags. (Before the fallback block defined NCCL_UNIQUE_ID_BYTES the
    static_assert in bgs_comm_unique_id named an undeclared identifier.)"""
    flags = makefile_variable("HIPFLAGS").replace("$(ARCH)", makefile_variable("ARCH")).split()
    p = subprocess.run([makefile_variable("HIPCC"), *flags, "-DBGS_NO_RCCL_HEADER", "-H", "-c", os.path.join(CSRC, "bgs_comm.hip"),
                        "-o", str(tmp_path / "bgs_comm_no_header.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    assert (tmp_path / "bgs_comm_no_header.o").stat().st_size > 0
    # the switch was honoured: what was compiled is the fallback block, not the header this host happens to have
    # (-H lists the files each pass really included)
    included = [line.lstrip(". ").strip() for line in p.stdout.splitlines() if line.startswith(".")]
    assert any(f.endswith("bgs_context.h") for f in included) and not any(f.endswith("rccl.h") for f in included)


def test_fallback_declarations_restate_the_header(tmp_path):
    """What the fallback block of csrc/bgs_comm.hip (and the stand-in) restates of RCCL's ABI, held against the header where
    there is one."""
    if not os.path.exists(RCCL_HEADER):
        pytest.skip("no rccl/rccl.h on this host: nothing to hold the fallback against")
    src = tmp_path / "rccl_values.cpp"
    src.write_text("#include <rccl/rccl.h>\n"
                   "static_assert(sizeof(ncclUniqueId) == 128, \"ncclUniqueId\");\n"
                   "static_assert(NCCL_UNIQUE_ID_BYTES == 128, \"NCCL_UNIQUE_ID_BYTES\");\n"
                   "static_assert(ncclUint8 == 1, \"ncclUint8\");\n"
                   "static_assert(ncclInt8 == 0, \"ncclInt8\");\n"
                   "static_assert(ncclSuccess == 0, \"ncclSuccess\");\n"
                   f"static_assert(ncclInvalidArgument == {fake_rccl.NCCL_INVALID_ARGUMENT}, \"ncclInvalidArgument\");\n"
                   f"static_assert(ncclInvalidUsage == {fake_rccl.NCCL_INVALID_USAGE}, \"ncclInvalidUsage\");\n"
                   "int main() { return 0; }\n")
    p = subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(fake_rccl.ROCM, "include"), "-fsyntax-only",
                        str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    # ... and the fallback block says the same
    text = open(os.path.join(CSRC, "bgs_comm.hip")).read()
    block = text[text.index("#else"):text.index("#endif")]
    assert "#define NCCL_UNIQUE_ID_BYTES 128" in block and "char internal[128]" in block
    assert re.search(r"ncclSuccess = 0\b", block) and re.search(r"ncclInt8 = 0, ncclUint8 = 1\b", block)


def test_the_library_override_is_documented_and_the_stand_in_builds():
    assert "BGS_RCCL_LIBRARY" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert 'getenv("BGS_RCCL_LIBRARY")' in open(os.path.join(CSRC, "bgs_comm.hip")).read()
    lib = ctypes.CDLL(fake_rccl.build())
    for name in ("ncclGetUniqueId", "ncclCommInitRank", "ncclCommDestroy", "ncclGather", "ncclGetErrorString",
                 "fake_rccl_live_comms", "fake_rccl_comm_query", "fake_rccl_pending_posts"):
        getattr(lib, name)
    # the gather's queries are the stand-in's own: libbgs exports nothing for them
    assert "fake_rccl" not in open(os.path.join(CSRC, "libbgs.map")).read()


def test_stand_in_ids_and_ranks():
    """ncclGetUniqueId and ncclCommInitRank of the stand-in, which touch no device: ids are non-zero and differ; a group is
    found by its id; a rank taken twice, a world size that disagrees with the group's, a rank outside the world and an id
    the stand-in did not hand out are refused with no communicator made; destroying the members empties the table."""
    lib = fake_rccl.load()
    a, b = fake_rccl.UniqueId(), fake_rccl.UniqueId()
    assert lib.ncclGetUniqueId(ctypes.byref(a)) == 0 and lib.ncclGetUniqueId(ctypes.byref(b)) == 0
    ida, idb = bytes(a)[:], bytes(b)[:]
    assert len(ida) == 128 and any(ida) and ida != idb
    live0 = lib.fake_rccl_live_comms()
    comms = []
    for rank in (2, 0):
        c = ctypes.c_void_p()
        assert lib.ncclCommInitRank(ctypes.byref(c), 3, a, rank) == 0 and c.value
        comms.append(c)
    assert lib.fake_rccl_live_comms() == live0 + 2
    info = fake_rccl.comm_info(lib, ida, 2)
    assert (info.nranks, info.gather_calls, info.gathers_completed) == (3, 0, 0)
    assert lib.fake_rccl_comm_query(ida, 1, ctypes.byref(info)) == -1     # rank 1 never joined
    assert lib.fake_rccl_comm_query(idb, 0, ctypes.byref(info)) == -1     # no group of that id
    c = ctypes.c_void_p(0xDEAD)
    for nranks, uid, rank, want in ((3, a, 2, fake_rccl.NCCL_INVALID_USAGE),        # the rank is taken
                                    (4, a, 1, fake_rccl.NCCL_INVALID_ARGUMENT),     # the group has 3 ranks
                                    (3, a, 3, fake_rccl.NCCL_INVALID_ARGUMENT),     # rank >= nranks
                                    (3, a, -1, fake_rccl.NCCL_INVALID_ARGUMENT),
                                    (0, b, 0, fake_rccl.NCCL_INVALID_ARGUMENT),
                                    (1, fake_rccl.UniqueId(), 0, fake_rccl.NCCL_INVALID_ARGUMENT)):   # all zero: not an id
        c.value = 0xDEAD
        got = lib.ncclCommInitRank(ctypes.byref(c), nranks, uid, rank)
        assert got == want and not c.value, (nranks, rank, got)
        assert lib.ncclGetErrorString(got).startswith(b"fake rccl: ")
    assert lib.fake_rccl_live_comms() == live0 + 2
    assert lib.fake_rccl_comm_query(idb, 0, ctypes.byref(info)) == -1     # a refused call made no group either
    for c in comms:
        assert lib.ncclCommDestroy(c) == 0
    assert lib.fake_rccl_live_comms() == live0
    assert lib.fake_rccl_comm_query(ida, 0, ctypes.byref(info)) == -1
    assert lib.ncclCommDestroy(None) == fake_rccl.NCCL_INVALID_ARGUMENT
