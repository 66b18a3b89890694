"""Sparse-splat selection, the part that needs no GPU: the arithmetic — the g++ build of csrc_sparse/sparse_math.h (the
operations the HIP kernels run) against the numpy twin `neighbor_counts_reference`, bit for bit, all pairs and through the
grid's rules; the twin against float64 geometry; known answers; the third library's ABI, its headers and its host-side
validation; and that the other two libraries did not move."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sparse_select_cases as C
from bevy_gaussian_splatting_amd import (
    SparseGrid, SparseSelect, _build_id, _native, _native_query, _native_sparse, neighbor_counts_reference, select_reference)
from bevy_gaussian_splatting_amd import sparse_select as SS
from test_native_binding import declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "bevy_gaussian_splatting_amd")
CSRC_SPARSE = os.path.join(PKG, "csrc_sparse")
SHIM_SRC = os.path.join(HERE, "host_shim", "sparse_math_shim.cpp")
SHIM_LIB = os.path.join(HERE, "host_shim", "libsparse_math_shim.so")
R = np.float32(C.RADIUS)


@pytest.fixture(scope="module")
def shim():
    """g++ build of sparse_math.h, with the flags of helpers.shim()."""
    deps = [SHIM_SRC, os.path.join(CSRC_SPARSE, "sparse_math.h")]
    if not os.path.exists(SHIM_LIB) or any(os.path.getmtime(d) > os.path.getmtime(SHIM_LIB) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-shared", "-fPIC",
                        "-Wno-unknown-pragmas", SHIM_SRC, "-o", SHIM_LIB], check=True, capture_output=True)
    lib = ctypes.CDLL(SHIM_LIB)
    vp, u32, f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float
    lib.shim_counts.argtypes = [vp, u32, u32, f32, u32, vp]
    lib.shim_counts.restype = None
    lib.shim_cells.argtypes = [vp, u32, u32, f32, vp]
    lib.shim_cells.restype = None
    lib.shim_grid_counts.argtypes = [vp, u32, u32, f32, u32, u32, vp]
    lib.shim_grid_counts.restype = None
    return lib


def shim_counts(lib, points, radius=C.RADIUS, cap=0, table_bits=None):
    """All pairs, or with table_bits the walk through a grid of 2^table_bits slots."""
    p = np.ascontiguousarray(points, np.float32)
    out = np.full(p.shape[0], 0xDEADBEEF, np.uint32)
    args = (p.ctypes.data_as(ctypes.c_void_p), p.shape[0], p.shape[1], radius, cap)
    if table_bits is None:
        lib.shim_counts(*args, out.ctypes.data_as(ctypes.c_void_p))
    else:
        lib.shim_grid_counts(*args, table_bits, out.ctypes.data_as(ctypes.c_void_p))
    return out


# ---- 1. the compiled arithmetic against the twin ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(C.CASES))
def test_shim_equals_the_twin(shim, case):
    """Random clouds, the boundary lattice, non-finite lanes and a NaN visibility lane: all pairs, bit for bit; and the
    grid's rules (cells, tags, slots) give the same counts, with a table so small that every slot is shared."""
    p, want = C.points(case, 5000), C.reference(case, 5000)
    assert want.dtype == np.uint32 and np.array_equal(shim_counts(shim, p), want)
    for bits in (1, 4, 14):
        assert np.array_equal(shim_counts(shim, p, table_bits=bits), want), bits
    assert np.array_equal(shim_counts(shim, p, cap=3, table_bits=14), np.minimum(want, 3))
    if case == "nonfinite":
        bad = ~np.isfinite(p[:, :3]).all(axis=1)
        assert bad.sum() > 400 and (want[bad] == 0).all() and (want[~bad] >= 1).all()
        assert np.isnan(p[~bad, 3]).sum() > 500                    # a NaN visibility changes nothing:
        clean = p.copy()
        clean[:, 3] = 1.0
        assert np.array_equal(neighbor_counts_reference(clean, C.RADIUS), want)
        huge = np.abs(p[:, :3]).max(axis=1) > 1e30
        # the largest finite value is a coordinate like any other: such a point counts itself, and whoever shares that lane
        # and is close in the other two; both sit in the last (clamped) cell of the axis
        assert (huge & ~bad).sum() > 100 and (want[huge & ~bad] >= 1).all() and (want[huge & ~bad] > 1).any()
    if case == "lattice":
        assert len(np.unique(want)) > 8 and want.min() >= 1


def test_near_points_lie_in_neighbouring_cells(shim):
    """What the kernels rely on, looked at where it is tightest: every pair of the lattice that the
    twin's test accepts lies in cells that differ by at most 1 along every axis, clamped cells included."""
    p = np.ascontiguousarray(C.lattice())
    cells = np.zeros((p.shape[0], 3), np.uint32)
    shim.shim_cells(p.ctypes.data_as(ctypes.c_void_p), p.shape[0], 3, C.RADIUS, cells.ctypes.data_as(ctypes.c_void_p))
    assert cells.max() == 2 << 20 and cells.min() == 0            # both clamps are reached
    cells = cells.astype(np.int64)
    r2 = R * R
    pairs = 0
    for lo in range(0, p.shape[0], 512):
        d = p[None, :, :] - p[lo:lo + 512, None, :]
        d2 = ((np.float32(0) + d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        i, j = np.nonzero(d2 < r2)
        pairs += len(i)
        assert np.abs(cells[lo + i] - cells[j]).max() <= 1
    assert pairs > 10 * p.shape[0]


# ---- 2. the twin against float64 geometry ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["clustered", "uniform"])
def test_twin_agrees_with_float64_geometry_away_from_the_radius(case):
    """6000 points, radius 0.05. A point is excluded when some neighbour's float64 distance lies within 1e-5 * radius =
    5e-7 of the radius; every other point's count equals the float64 count; at most 2 % may be excluded.

    Why 5e-7 is enough. Were the coordinates real numbers known to half an ulp, |x| <= 2.5 would put 2^-23 = 1.2e-7 on a
    coordinate and sqrt(3) times that, 2.1e-7, on a distance. Here the float32 coordinates ARE the points, and what is
    left is the twin's own rounding: a difference below 0.0625 is off by at most 2^-29, and the squares, the two sums and
    radius * radius by 2^-24 relative each, which moves a distance near 0.05 by some 1e-8. Either way below the band."""
    p = C.CASES[case]()
    assert p.shape == (6000, 3) and np.abs(p).max() <= 2.5
    q = p.astype(np.float64)
    radius = float(R)
    band = 1e-5 * radius
    count64 = np.zeros(6000, np.int64)
    excluded = np.zeros(6000, bool)
    for lo in range(0, 6000, 1000):
        dist = np.sqrt(((q[None, :, :] - q[lo:lo + 1000, None, :]) ** 2).sum(axis=2))
        count64[lo:lo + 1000] = (dist < radius).sum(axis=1)
        excluded[lo:lo + 1000] = (np.abs(dist - radius) < band).any(axis=1)
    print(f"{case}: {excluded.sum()} of 6000 points ({100.0 * excluded.mean():.2f} %) have a neighbour within {band:.1e} of the radius")
    assert excluded.sum() <= 6000 * 2 // 100
    want = C.reference(case, 6000)
    assert np.array_equal(want[~excluded].astype(np.int64), count64[~excluded])
    if case == "clustered":
        assert want.max() > 100 and (want < 3).any()
    else:
        assert 2.5 < want.mean() < 4.5


# ---- 3. known answers -----------------------------------------------------------------------------------------------------------
def test_known_answers():
    r = np.float32(0.0625)                                         # a power of two: r * r and the differences below are exact
    at = lambda x: np.array([[1.0, 2.0, -3.0], [x, 2.0, -3.0]], np.float32)
    assert neighbor_counts_reference(at(1.0 + 0.0625), r).tolist() == [1, 1]               # exactly radius apart: strict, not near
    closer = np.nextafter(np.float32(1.0 + 0.0625), np.float32(0))
    assert neighbor_counts_reference(at(closer), r).tolist() == [2, 2]                     # one ulp closer: near
    for axis in (1, 2):
        two = np.zeros((2, 3), np.float32)
        two[1, axis] = r
        assert neighbor_counts_reference(two, r).tolist() == [1, 1]
        two[1, axis] = np.nextafter(r, np.float32(0))
        assert neighbor_counts_reference(two, r).tolist() == [2, 2]
    assert neighbor_counts_reference(np.array([[5.0, 6.0, 7.0]], np.float32), C.RADIUS).tolist() == [1]   # a lone point
    assert neighbor_counts_reference(np.zeros((0, 3), np.float32), C.RADIUS).shape == (0,)
    k = 7
    same = np.tile(np.array([[0.1, 0.2, 0.3]], np.float32), (k, 1))
    assert neighbor_counts_reference(same, C.RADIUS).tolist() == [k] * k
    assert neighbor_counts_reference(same, C.RADIUS, cap=3).tolist() == [3] * k
    assert neighbor_counts_reference(same, C.RADIUS, cap=k + 1).tolist() == [k] * k
    want = C.reference("uniform", 5000)
    assert np.array_equal(neighbor_counts_reference(C.points("uniform", 5000), C.RADIUS, cap=2), np.minimum(want, 2))
    assert neighbor_counts_reference(C.points("uniform", 64).astype(np.float64), C.RADIUS).dtype == np.uint32


def test_the_rule_is_symmetric():
    """near(i, j) == near(j, i) on a random cloud: the matrix of the twin's decisions is its own transpose."""
    p = C.points("clustered", 1500)
    d = p[None, :, :] - p[:, None, :]
    d2 = ((np.float32(0) + d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    near = d2 < R * R
    assert d2.dtype == np.float32 and np.array_equal(near, near.T) and near.diagonal().all()
    assert np.array_equal(near.sum(axis=1).astype(np.uint32), C.reference("clustered", 1500))


def test_select_reference_and_the_component():
    assert SparseSelect() == SparseSelect(radius=0.05, neighbor_threshold=3)
    p, counts = C.points("uniform", 5000), C.reference("uniform", 5000)
    got = select_reference(p, C.RADIUS, 3)
    assert got.dtype == np.uint32 and np.array_equal(got, np.flatnonzero(counts < 3)) and (np.diff(got.astype(np.int64)) > 0).all()
    assert 500 < len(got) < 4500
    assert len(select_reference(p, C.RADIUS, 1)) == 0 and len(select_reference(p, C.RADIUS, 100)) == 5000
    for bad, words in ((0.0, "finite and positive"), (-1.0, "finite and positive"), (np.nan, "finite and positive"),
                       (np.inf, "finite and positive"), (1e-30, "has the square 0"), (1e30, "has the square inf")):
        with pytest.raises(ValueError, match=words):
            neighbor_counts_reference(p[:4], bad)


def test_keep_reference_rule():
    e = np.zeros(8, np.dtype([("key", np.uint32), ("index", np.uint32)]))
    e["key"] = (5, 6, 0xFFFFFFFF, 7, 8, 9, 0xFFFFFFFF, 3)
    e["index"] = (0, 1, 1, 4, 0xFFFFFFFF, 2, 0, 3)
    counts = np.array([1, 3, 2, 40], np.uint32)   # sparse under threshold 3: points 0 and 2
    kept = SS.keep_reference(e, counts, 3)
    assert kept["key"].tolist() == [5, 0xFFFFFFFF, 0xFFFFFFFF, 7, 8, 9, 0xFFFFFFFF, 0xFFFFFFFF]
    out = SS.keep_reference(e, counts, 3, dense=True)
    assert out["key"].tolist() == [0xFFFFFFFF, 6, 0xFFFFFFFF, 7, 8, 0xFFFFFFFF, 0xFFFFFFFF, 3]
    assert np.array_equal(kept["index"], e["index"]) and np.array_equal(out["index"], e["index"])
    assert SS.keep_reference(e, counts, 0)["key"].tolist() == [0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 7, 8, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]


# ---- 4. ABI and build ----------------------------------------------------------------------------------------------------------
def test_the_library_exports_exactly_what_its_header_declares():
    lib = _native_sparse.load()
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _native_sparse.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    assert defined == set(_native_sparse.EXPORTED_SYMBOLS), sorted(defined ^ set(_native_sparse.EXPORTED_SYMBOLS))
    assert len(defined) == 8 and all(hasattr(lib, n) for n in defined)
    assert lib.bgss_version() == (0 << 16) | 1 == _native_sparse.ABI_VERSION
    # it links the HIP runtime, not the other two libraries
    readelf = shutil.which("readelf") or "/opt/rocm/lib/llvm/bin/llvm-readelf"
    needed = subprocess.run([readelf, "-d", _native_sparse.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "libamdhip64" in needed and "libbgs" not in needed


def test_prototype_table_agrees_with_the_header():
    """What is this header's own; the table against the header, function by function, is tests/test_native_binding.py's."""
    assert len(declarations(("bgs_sparse.h",), "bgss_")) == 8
    assert (_native_sparse.BGSS_OK, _native_sparse.BGSS_EINVAL, _native_sparse.BGSS_ENOMEM, _native_sparse.BGSS_EHIP) == (0, -1, -2, -3)
    for name, value in (("BGSS_KEEP_SPARSE", "0u"), ("BGSS_KEEP_DENSE", "1u"), ("BGSS_VERSION_MAJOR", "0"), ("BGSS_VERSION_MINOR", "1")):
        assert re.search(r"#define %s %s\b" % (name, value), open(os.path.join(ROOT, "include", "bgs_sparse.h")).read())


def test_the_build_id_is_the_source_hash_and_nobody_elses():
    """The built library carries its own id and nobody else's marker. The recipe of the hash and the table of libraries
    are tests/test_native_binding.py's, for all five."""
    spec = _build_id.LIBBGS_SPARSE
    _native_sparse.load()
    assert _build_id.library_build_id(_native_sparse.LIB_PATH, spec) == _build_id.source_sha256(spec)
    data = open(_native_sparse.LIB_PATH, "rb").read()
    assert b"BGS_BUILD_ID=" not in data and b"BGSQ_BUILD_ID=" not in data


def test_the_other_libraries_and_headers_do_not_know_of_this_one():
    for d in ("csrc", "csrc_query"):
        for name in sorted(os.listdir(os.path.join(PKG, d))):
            path = os.path.join(PKG, d, name)
            if os.path.isfile(path) and (name.endswith((".hip", ".h", ".map", ".inc")) or name == "Makefile"):
                assert b"bgss_" not in open(path, "rb").read() and b"BGSS_" not in open(path, "rb").read(), path
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name not in ("bgs_sparse.h", "bgs_sparse.hpp"):
            assert "bgss_" not in open(os.path.join(ROOT, "include", name)).read(), name
    assert not any(n.startswith("bgss") for n in _native.EXPORTED_SYMBOLS + _native_query.EXPORTED_SYMBOLS)
    for name in os.listdir(CSRC_SPARSE):
        if name.endswith((".hip", ".h")):
            text = open(os.path.join(CSRC_SPARSE, name)).read()
            assert "bgsq_" not in text and '"../csrc' not in text and "bgs.h" not in text, name


def test_header_is_plain_c_and_the_cpp_layer_is_standard_cpp17(tmp_path):
    c = tmp_path / "abi.c"
    c.write_text('#include "bgs_sparse.h"\nint main(void) { bgss_grid* g = 0; bgss_grid_free(g); '
                 "return (int)bgss_version() == (int)BGSS_KEEP_DENSE; }\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-c", str(c), "-o", str(tmp_path / "abi.o")], check=True)
    cpp = tmp_path / "host.cpp"
    cpp.write_text('#include "bgs_sparse.hpp"\nint main() { const bgs::sparse::SparseSelect s; '
                   "return s.neighbor_threshold == 3u && s.radius == 0.05f ? 0 : 1; }\n")
    subprocess.run(["g++", "-std=c++17", "-pedantic", "-Wall", "-Wextra", "-Wshadow", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-c", str(cpp), "-o", str(tmp_path / "host.o")], check=True)


def test_cpp_layer_carries_the_c_abis_errors(tmp_path):
    """bgs_sparse.hpp linked against the library: a refusal of the C ABI that needs no device arrives as
    bgs::sparse::Error with the status and the offender named."""
    _native_sparse.load()
    src = tmp_path / "tool.cpp"
    src.write_text(r'''
#include <cstdio>
#include "bgs_sparse.hpp"
int main() {
    namespace s = bgs::sparse;
    try { s::check(bgss_neighbor_counts(nullptr, nullptr, nullptr, 0, -1.0f, 0, nullptr)); std::printf("no error\n"); }
    catch (const s::Error& e) { std::printf("%d %s\n", e.status(), e.what()); }
    try { s::check(bgss_entries_keep(0, nullptr, nullptr, 0, nullptr, 0, 3, BGSS_KEEP_DENSE)); std::printf("ok\n"); }
    catch (const s::Error& e) { std::printf("%d %s\n", e.status(), e.what()); }
    return 0;
}
''')
    exe = tmp_path / "tool"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L" + CSRC_SPARSE, "-lbgs_sparse", "-Wl,-rpath," + CSRC_SPARSE], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert lines[0].startswith("-1 ") and "radius -1 must be finite and positive" in lines[0]
    assert lines[1] == "ok"


# ---- 5. validation without a device ----------------------------------------------------------------------------------------------
def test_validation_names_the_offender():
    lib = _native_sparse.load()
    EINVAL, OK = _native_sparse.BGSS_EINVAL, _native_sparse.BGSS_OK
    p16, p4, f = ctypes.c_void_p(16), ctypes.c_void_p(4), ctypes.c_float
    assert lib.bgss_neighbor_counts(None, None, p16, 4, f(0.05), 0, p4) == EINVAL and lib.bgss_last_error() == b"bgss_neighbor_counts: grid is NULL"
    assert lib.bgss_neighbor_counts(None, None, None, 0, f(0.05), 0, None) == EINVAL and b"grid is NULL" in lib.bgss_last_error()
    for radius, words in ((0.0, b"radius 0 must be finite and positive"), (-0.05, b"radius -0.05 must be finite and positive"),
                          (float("nan"), b"must be finite and positive"), (float("inf"), b"radius inf must be finite and positive"),
                          (1e-30, b"radius 1e-30 has the square 0 in f32"), (1e30, b"radius 1e+30 has the square inf in f32")):
        assert lib.bgss_neighbor_counts(None, None, p16, 4, f(radius), 0, p4) == EINVAL
        assert words in lib.bgss_last_error(), (radius, lib.bgss_last_error())
    for points, counts, words in ((None, p4, b"points_device_ptr must be a 16-byte aligned"), (ctypes.c_void_p(8), p4, b"points_device_ptr"),
                                  (p16, None, b"counts_device_ptr must be a 4-byte aligned"), (p16, ctypes.c_void_p(6), b"counts_device_ptr")):
        assert lib.bgss_neighbor_counts(None, None, points, 4, f(0.05), 0, counts) == EINVAL
        assert words in lib.bgss_last_error()
    assert lib.bgss_entries_keep(0, None, ctypes.c_void_p(8), 4, p4, 4, 3, 2) == EINVAL and b"flags 2" in lib.bgss_last_error()
    assert lib.bgss_entries_keep(0, None, p4, 4, p4, 4, 3, 0) == EINVAL and b"8-byte aligned" in lib.bgss_last_error()
    assert lib.bgss_entries_keep(0, None, ctypes.c_void_p(8), 4, ctypes.c_void_p(2), 4, 3, 1) == EINVAL and b"counts_device_ptr" in lib.bgss_last_error()
    assert lib.bgss_entries_keep(0, None, None, 0, None, 0, 3, 1) == OK and lib.bgss_last_error() == b""
    assert lib.bgss_entries_keep(0, None, ctypes.c_void_p(8), 4, None, 0, 3, 0) == OK and lib.bgss_last_error() == b""   # a plane of no points
    assert lib.bgss_debug_set_table_bits(None, 2) == EINVAL and b"grid is NULL" in lib.bgss_last_error()
    assert lib.bgss_grid_create(0, 16, None) == EINVAL and b"out is NULL" in lib.bgss_last_error()
    out = ctypes.c_void_p()
    assert lib.bgss_grid_create(-1, 16, ctypes.byref(out)) == EINVAL and b"hip_device -1" in lib.bgss_last_error() and not out.value
    assert lib.bgss_grid_capacity(None) == 0
    lib.bgss_grid_free(None)
    with pytest.raises(ValueError):
        SparseGrid(1 << 32)


def test_no_cpu_fallback_without_a_usable_device():
    import torch
    device = 99 if torch.cuda.is_available() else 0
    with pytest.raises(_native_sparse.BgsSparseError) as ei:
        SparseGrid(16, device)
    assert ei.value.status == _native_sparse.BGSS_EHIP and f"no usable HIP device {device}" in str(ei.value)
