"""Point-in-mesh selection, the part that needs no GPU: the arithmetic — the g++ build of csrc_query/mesh_query_math.h (the
operations the HIP kernels run) against the numpy twin `crossings_reference`, bit for bit; the twin against float64
geometry; the second library's ABI, its headers and its host-side validation; and that libbgs did not move."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mesh_query_cases as C
from bevy_gaussian_splatting_amd import (
    MeshQuery, TriangleMesh, _build_id, _native, _native_query, crossings_reference, cube_mesh, icosphere_mesh, mesh_from_points)
from bevy_gaussian_splatting_amd import mesh_query as MQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC_QUERY = os.path.join(ROOT, "bevy_gaussian_splatting_amd", "csrc_query")
SHIM_SRC = os.path.join(HERE, "host_shim", "mesh_query_math_shim.cpp")
SHIM_LIB = os.path.join(HERE, "host_shim", "libmesh_query_math_shim.so")


@pytest.fixture(scope="module")
def shim():
    """g++ build of mesh_query_math.h, with the flags of helpers.shim()."""
    deps = [SHIM_SRC, os.path.join(CSRC_QUERY, "mesh_query_math.h")]
    if not os.path.exists(SHIM_LIB) or any(os.path.getmtime(d) > os.path.getmtime(SHIM_LIB) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-shared", "-fPIC",
                        "-Wno-unknown-pragmas", SHIM_SRC, "-o", SHIM_LIB], check=True, capture_output=True)
    lib = ctypes.CDLL(SHIM_LIB)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.shim_crossings.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp]
    lib.shim_crossings.restype = None
    lib.shim_triangle_records.argtypes = [vp, vp, u32, vp]
    lib.shim_triangle_records.restype = None
    lib.shim_record_bytes.argtypes = []
    lib.shim_record_bytes.restype = u32
    return lib


def shim_crossings(lib, points, mesh, matrix=None):
    p = np.ascontiguousarray(points, np.float32)
    m = np.ascontiguousarray(np.asarray(np.eye(4) if matrix is None else matrix, np.float32).T).reshape(16)
    out = np.full(p.shape[0], 0xDEADBEEF, np.uint32)
    lib.shim_crossings(p.ctypes.data_as(ctypes.c_void_p), p.shape[0], p.shape[1], mesh.vertices.ctypes.data_as(ctypes.c_void_p),
                       mesh.indices.ctypes.data_as(ctypes.c_void_p), mesh.triangle_count, m.ctypes.data_as(ctypes.c_void_p),
                       out.ctypes.data_as(ctypes.c_void_p))
    return out


# ---- 1. the compiled arithmetic against the twin ----------------------------------------------------------------------------
def test_shim_equals_the_twin_on_random_points_and_the_icosphere(shim):
    s = C.sphere()
    want = crossings_reference(C.random_points(), s.vertices, s.indices)
    assert want.dtype == np.uint32 and np.array_equal(shim_crossings(shim, C.random_points(), s), want)
    hist = np.bincount(want)
    assert len(hist) == 3 and hist[1] > 2500 and hist[2] > 1000   # inside, and outside on the -x side of the sphere
    # ... and under a matrix with rotation, non-uniform scale and translation, on the float4 layout
    m = C.matrix_of("affine")
    for t in (1280, 1283):
        assert np.array_equal(shim_crossings(shim, C.cloud_points("affine"), C.mesh_with(t), m), C.cloud_reference(t, "affine"))
    assert np.array_equal(C.cloud_reference(1283, "affine"), C.cloud_reference(1280, "affine"))   # the rejected triangles never hit


def test_shim_equals_the_twin_on_the_boundary_lattice(shim):
    """k/8 against the cube at +-0.5: every product and sum is exact, so u == 0, u + v == 1 and a == 0 are hit exactly."""
    cube = cube_mesh()
    want = C.lattice_reference()
    assert np.array_equal(shim_crossings(shim, C.lattice_points(), cube), want)
    p = C.lattice_points()
    strictly_inside = (np.abs(p) < 0.5).all(axis=1)
    strictly_outside_yz = (np.abs(p[:, 1:]) > 0.5).any(axis=1)
    # The +x face is cut along y == z, and both of its triangles accept a ray through their common edge (u + v == 1 and
    # v == 0 are inclusive, as in the reference): such a point counts 2 crossings and is reported OUTSIDE. That is the
    # reference's rule, kept bit for bit.
    diagonal = p[:, 1] == p[:, 2]
    assert (want[strictly_inside & ~diagonal] == 1).all() and (want[strictly_inside & diagonal] == 2).all()
    assert (want[strictly_outside_yz] == 0).all()
    # the faces parallel to the ray are rejected on `a`: the 48-byte records say so
    rec = np.zeros((12, 12), np.float32)
    assert shim.shim_record_bytes() == 48
    shim.shim_triangle_records(cube.vertices.ctypes.data_as(ctypes.c_void_p), cube.indices.ctypes.data_as(ctypes.c_void_p), 12,
                               rec.ctypes.data_as(ctypes.c_void_p))
    assert np.isnan(rec[4:, 9]).all() and (np.abs(rec[:4, 9]) == 1.0).all()   # +-x faces: a = +-1; the other eight: never hit
    assert np.array_equal(rec[:, 0:3], cube.vertices[cube.indices[:, 0]])
    # points ON the boundary get whatever the rounded tests say — the same in both builds; some of them do count
    on_boundary = ~strictly_inside & ~strictly_outside_yz & (np.abs(p[:, 0]) <= 0.5)
    assert on_boundary.sum() > 100 and len(np.unique(want[on_boundary])) > 1


def test_shim_equals_the_twin_on_non_finite_points(shim):
    s = C.sphere()
    p = C.nonfinite_points()
    want = C.nonfinite_reference()
    assert np.array_equal(shim_crossings(shim, p, s), want)
    bad = ~np.isfinite(p).all(axis=1)
    assert bad.sum() == 10 and (want[bad] == 0).all()
    good = crossings_reference(C.random_points()[:64], s.vertices, s.indices)
    huge = np.abs(p).max(axis=1) > 1e30
    assert np.array_equal(want[~bad & ~huge], good[~bad & ~huge]) and (want[~bad & ~huge] > 0).any()
    # a finite point that a matrix throws to infinity: the LOCAL position decides
    m = np.diag([1e30, 1.0, 1.0, 1.0]).astype(np.float32)
    far = np.array([[1e30, 0.0, 0.0], [0.1, 0.0, 0.0]], np.float32)
    assert crossings_reference(far, s.vertices, s.indices, m).tolist()[0] == 0 == int(shim_crossings(shim, far, s, m)[0])


# ---- 2. the twin against float64 geometry ------------------------------------------------------------------------------------
def _float64_parity_and_margins(points, mesh, margin):
    """Moeller-Trumbore in float64 on the same (float32) polyhedron: inside by parity, and which points come within
    `margin` of a threshold of u, v, 1 - u - v or t for some triangle."""
    v = mesh.vertices.astype(np.float64)
    v0, e1, e2 = v[mesh.indices[:, 0]], v[mesh.indices[:, 1]] - v[mesh.indices[:, 0]], v[mesh.indices[:, 2]] - v[mesh.indices[:, 0]]
    d = np.array([1.0, 0.0, 0.0])
    h = np.cross(d, e2)
    a = (e1 * h).sum(axis=1)
    # The sphere has triangles that the plane x = 0 cuts in mirror halves: their normals have no x, the ray is parallel to
    # them and `a` is 0 (exactly, here). They never hit, in either precision; every other triangle is far from that test.
    parallel = np.abs(a) < 1e-6
    assert 0 < parallel.sum() < 64 and (np.abs(a[~parallel]) > 1e-4).all()
    v0, e1, e2, h, a = v0[~parallel], e1[~parallel], e2[~parallel], h[~parallel], a[~parallel]
    f = 1.0 / a
    inside = np.zeros(points.shape[0], bool)
    near = np.zeros(points.shape[0], bool)
    for lo in range(0, points.shape[0], 2000):
        s = points[lo:lo + 2000, None, :].astype(np.float64) - v0[None]
        u = f * (s * h[None]).sum(axis=2)
        q = np.cross(s, e1[None])
        vv = f * q[..., 0]
        t = f * (q * e2[None]).sum(axis=2)
        w = 1.0 - u - vv
        hit = (u >= 0) & (u <= 1) & (vv >= 0) & (w >= 0) & (t > 1e-6)
        inside[lo:lo + 2000] = hit.sum(axis=1) & 1
        close = (np.abs(u) < margin) | (np.abs(u - 1.0) < margin) | (np.abs(vv) < margin) | (np.abs(w) < margin) | (np.abs(t - 1e-6) < margin)
        near[lo:lo + 2000] = close.any(axis=1)
    return inside, near


def test_twin_agrees_with_float64_geometry_away_from_the_thresholds():
    """20 000 seeded points in [-1.5, 1.5]^3 against the icosphere of radius 1. A point is excluded when, in the float64 run,
    any of u, v, 1 - u - v, t lies within 1e-5 of its threshold for some triangle; at most 1 % may be. All the rest agree."""
    s, p = C.sphere(), C.random_points()
    inside64, near = _float64_parity_and_margins(p, s, 1e-5)
    print(f"seed {C.SEED_RANDOM}: {near.sum()} of {len(p)} points within 1e-5 of a threshold")
    assert near.sum() <= len(p) // 100
    inside32 = (crossings_reference(p, s.vertices, s.indices) & 1).astype(bool)
    assert np.array_equal(inside32[~near], inside64[~near])
    # and the polyhedron is the sphere to within its own sagitta: inside it below the inscribed radius, outside above 1
    r = np.linalg.norm(p.astype(np.float64), axis=1)
    assert inside64[r < 0.99].all() and not inside64[r > 1.0 + 1e-6].any() and 2500 < inside64.sum() < 3300


def test_generators_and_transforms():
    c, s0, s3 = cube_mesh(), icosphere_mesh(0), C.sphere()
    assert c.triangle_count == 12 and s0.triangle_count == 20 and s3.vertices.shape == (642, 3)
    assert c.vertices.dtype == np.float32 and c.indices.dtype == np.uint32 and np.abs(c.vertices).max() == 0.5
    assert np.allclose(np.linalg.norm(s3.vertices.astype(np.float64), axis=1), 1.0, atol=1e-7)
    for m in (c, s3):   # closed and consistently wound: every directed edge has its opposite exactly once
        e = np.concatenate([m.indices[:, [0, 1]], m.indices[:, [1, 2]], m.indices[:, [2, 0]]]).astype(np.int64)
        assert sorted(map(tuple, e)) == sorted(map(tuple, e[:, ::-1])) and len(set(map(tuple, e))) == len(e)
        v = m.vertices.astype(np.float64)
        vol = np.einsum("ij,ij->i", v[m.indices[:, 0]], np.cross(v[m.indices[:, 1]], v[m.indices[:, 2]])).sum() / 6.0
        assert vol > 0   # outward
    t, m = C.affine()
    assert m.dtype == np.float32 and m.shape == (4, 4)
    assert np.array_equal(m, np.linalg.inv(t).astype(np.float32))   # composed in float64, rounded once
    cloud = np.diag([2.0, 2.0, 2.0, 1.0])
    assert np.array_equal(mesh_from_points(t, cloud), (np.linalg.inv(t) @ cloud).astype(np.float32))
    # a mesh moved by T and queried through inverse(T) selects what the mesh at rest selects from the points at rest
    # (up to rounding at the surface: compared away from it)
    rest = crossings_reference(C.cloud_points("identity"), s3.vertices, s3.indices) & 1
    moved = C.cloud_reference(1280, "affine") & 1
    r = np.linalg.norm(C.cloud_points("identity")[:, :3].astype(np.float64), axis=1)
    clear = (r < 0.98) | (r > 1.001)
    assert np.array_equal(rest[clear], moved[clear]) and 0 < rest.sum() < 5000


def test_keep_reference_rule():
    e = np.zeros(8, np.dtype([("key", np.uint32), ("index", np.uint32)]))
    e["key"] = (5, 6, 0xFFFFFFFF, 7, 8, 9, 0xFFFFFFFF, 3)
    e["index"] = (0, 1, 1, 4, 0xFFFFFFFF, 2, 0, 3)
    crossings = np.array([1, 2, 3, 0], np.uint32)   # inside: 0 and 2
    kept = MQ.keep_reference(e, crossings)
    assert kept["key"].tolist() == [5, 0xFFFFFFFF, 0xFFFFFFFF, 7, 8, 9, 0xFFFFFFFF, 0xFFFFFFFF]
    out = MQ.keep_reference(e, crossings, outside=True)
    assert out["key"].tolist() == [0xFFFFFFFF, 6, 0xFFFFFFFF, 7, 8, 0xFFFFFFFF, 0xFFFFFFFF, 3]
    assert np.array_equal(kept["index"], e["index"]) and np.array_equal(out["index"], e["index"])


# ---- 3. ABI and build ----------------------------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(ROOT, "include", "bgs_query.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(bgsq_[a-z0-9_]+)\s*\(", text))


def test_the_library_exports_exactly_what_its_header_declares():
    lib = _native_query.load()
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _native_query.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    assert defined == _declared() == set(_native_query.EXPORTED_SYMBOLS), sorted(defined ^ _declared())
    assert len(defined) == 8 and all(hasattr(lib, n) for n in defined)
    assert lib.bgsq_version() == (0 << 16) | 1 == _native_query.ABI_VERSION
    assert _build_id.library_build_id(_native_query.LIB_PATH, _build_id.LIBBGS_QUERY) == _build_id.source_sha256(_build_id.LIBBGS_QUERY)
    # it links the HIP runtime, not libbgs
    readelf = shutil.which("readelf") or "/opt/rocm/lib/llvm/bin/llvm-readelf"
    needed = subprocess.run([readelf, "-d", _native_query.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "libamdhip64" in needed and "libbgs" not in needed


def test_libbgs_and_its_headers_did_not_move():
    """This feature lives in csrc_query/ and leaves libbgs's build id where the parent commit had it (aed671d032bf...,
    taken on both trees when this was written). A literal id here would fail the next change to csrc/, so the test holds
    what keeps the id still instead: the id is a hash of csrc/'s own files and of nothing below or beside it, none of
    which knows of the query, and the query's directory is not one it reads."""
    import hashlib
    csrc = os.path.join(ROOT, "bevy_gaussian_splatting_amd", "csrc")
    h = hashlib.sha256()
    for name in sorted(os.listdir(csrc)):
        path = os.path.join(csrc, name)
        if os.path.isfile(path) and (name.endswith((".hip", ".h")) or name == "Makefile"):
            h.update(name.encode())
            h.update(open(path, "rb").read())
            assert b"bgsq" not in open(path, "rb").read() and b"mesh_query" not in open(path, "rb").read(), name
    assert _build_id.kernel_source_sha256() == h.hexdigest() == _build_id.library_build_id(_native.LIB_PATH)
    assert os.path.realpath(CSRC_QUERY) != os.path.realpath(csrc) and not os.path.exists(os.path.join(csrc, "csrc_query"))
    for name in ("bgs.h", "bgs_diag.h", "bgs.hpp", "bgs_host.hpp"):
        assert "bgsq_" not in open(os.path.join(ROOT, "include", name)).read()
    assert not any(n.startswith("bgsq") for n in _native.EXPORTED_SYMBOLS)
    assert _build_id.source_sha256(_build_id.LIBBGS_QUERY) != _build_id.kernel_source_sha256()


def test_header_is_plain_c_and_the_cpp_layer_is_standard_cpp17(tmp_path):
    c = tmp_path / "abi.c"
    c.write_text('#include "bgs_query.h"\nint main(void) { bgsq_mesh* m = 0; bgsq_mesh_free(m); '
                 "return (int)bgsq_version() == (int)BGSQ_KEEP_OUTSIDE; }\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-c", str(c), "-o", str(tmp_path / "abi.o")], check=True)
    cpp = tmp_path / "host.cpp"
    cpp.write_text('#include "bgs_query.hpp"\nint main() { bgs::query::TriangleMesh m = bgs::query::cube_mesh(); '
                   "return (int)m.triangle_count() - 12; }\n")
    subprocess.run(["g++", "-std=c++17", "-pedantic", "-Wall", "-Wextra", "-Wshadow", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-c", str(cpp), "-o", str(tmp_path / "host.o")], check=True)


def test_cpp_layer_validates_and_generates_like_python(tmp_path):
    """bgs_query.hpp linked against the library: its generators give the Python ones' meshes, and the C ABI's validation
    errors (no device needed: they come before any HIP call) arrive as bgs::query::Error with the offender named."""
    _native_query.load()
    src = tmp_path / "tool.cpp"
    src.write_text(r'''
#include <cmath>
#include <cstdio>
#include "bgs_query.hpp"
int main() {
    namespace q = bgs::query;
    const q::TriangleMesh c = q::cube_mesh(), s = q::icosphere_mesh(3);
    std::printf("%zu %zu %zu %zu\n", c.vertices.size(), c.triangle_count(), s.vertices.size(), s.triangle_count());
    for (const auto& t : c.indices) std::printf("%u %u %u\n", t[0], t[1], t[2]);
    double sum = 0;
    for (const auto& v : s.vertices) sum += (double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2];
    std::printf("%.6f\n", sum / (double)s.vertices.size());
    q::TriangleMesh bad = c;
    bad.indices[3][1] = 8;
    try { q::MeshQuery m(bad, 0); std::printf("no error\n"); } catch (const q::Error& e) { std::printf("%d %s\n", e.status(), e.what()); }
    bad = c;
    bad.vertices[5][2] = HUGE_VALF;
    try { q::MeshQuery m(bad, 0); std::printf("no error\n"); } catch (const q::Error& e) { std::printf("%d %s\n", e.status(), e.what()); }
    const q::Mat4 t{2, 0, 0, 0, 0, 4, 0, 0, 0, 0, 8, 0, 1, 2, 3, 1};   // scale (2, 4, 8), then translation (1, 2, 3)
    for (float x : q::mesh_from_points(t)) std::printf("%g ", x);
    std::printf("\n");
    return 0;
}
''')
    exe = tmp_path / "tool"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L" + CSRC_QUERY, "-lbgs_query", "-Wl,-rpath," + CSRC_QUERY], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert lines[0].split() == ["8", "12", "642", "1280"]
    assert np.array_equal(np.array([l.split() for l in lines[1:13]], np.uint32), cube_mesh().indices)
    assert abs(float(lines[13]) - 1.0) < 1e-6
    assert lines[14].startswith("-1 ") and "triangle 3 names vertex 8, the mesh has 8" in lines[14]
    assert lines[15].startswith("-1 ") and "vertex 5 has a non-finite z" in lines[15]
    assert [float(x) for x in lines[16].split()] == [0.5, 0, 0, 0, 0, 0.25, 0, 0, 0, 0, 0.125, 0, -0.5, -0.5, -0.375, 1]


def test_mesh_validation_names_the_offender():
    c = cube_mesh()
    with pytest.raises(ValueError, match="triangle 3 names vertex 8, the mesh has 8"):
        idx = c.indices.copy()
        idx[3, 1] = 8
        TriangleMesh(c.vertices, idx)
    with pytest.raises(ValueError, match="vertex 5 has a non-finite z"):
        v = c.vertices.copy()
        v[5, 2] = np.inf
        TriangleMesh(v, c.indices)
    with pytest.raises(TypeError):
        TriangleMesh(c.vertices[:, :2], c.indices)
    with pytest.raises(TypeError):
        MeshQuery((c.vertices, c.indices))
    assert TriangleMesh(np.zeros((0, 3)), []).triangle_count == 0
    # the C ABI refuses the same before it touches a device
    lib = _native_query.load()
    out = ctypes.c_void_p()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    bad_idx = c.indices.copy()
    bad_idx[3, 1] = 8
    assert lib.bgsq_mesh_create(0, vp(c.vertices), 8, vp(bad_idx), 12, ctypes.byref(out)) == _native_query.BGSQ_EINVAL
    assert b"triangle 3 names vertex 8, the mesh has 8" in lib.bgsq_last_error() and not out.value
    bad_v = c.vertices.copy()
    bad_v[5, 2] = np.nan
    assert lib.bgsq_mesh_create(0, vp(bad_v), 8, vp(c.indices), 12, ctypes.byref(out)) == _native_query.BGSQ_EINVAL
    assert b"vertex 5 has a non-finite z" in lib.bgsq_last_error()
    assert lib.bgsq_mesh_create(0, None, 8, vp(c.indices), 12, ctypes.byref(out)) == _native_query.BGSQ_EINVAL
    assert b"vertices_xyz is NULL" in lib.bgsq_last_error()
    assert lib.bgsq_mesh_create(0, vp(c.vertices), 8, None, 12, ctypes.byref(out)) == _native_query.BGSQ_EINVAL
    assert b"indices is NULL" in lib.bgsq_last_error()
    assert lib.bgsq_mesh_create(0, vp(c.vertices), 8, vp(c.indices), 12, None) == _native_query.BGSQ_EINVAL
    # calls that need no mesh or device: argument checks
    assert lib.bgsq_crossings(None, None, None, 4, None, None) == _native_query.BGSQ_EINVAL and b"mesh is NULL" in lib.bgsq_last_error()
    assert lib.bgsq_entries_keep(0, None, ctypes.c_void_p(8), 4, ctypes.c_void_p(4), 4, 2) == _native_query.BGSQ_EINVAL
    assert b"flags 2" in lib.bgsq_last_error()
    assert lib.bgsq_entries_keep(0, None, ctypes.c_void_p(4), 4, ctypes.c_void_p(4), 4, 0) == _native_query.BGSQ_EINVAL
    assert b"8-byte aligned" in lib.bgsq_last_error()
    assert lib.bgsq_entries_keep(0, None, None, 0, None, 0, 1) == _native_query.BGSQ_OK and lib.bgsq_last_error() == b""
    assert lib.bgsq_debug_set_slices(None, 2) == _native_query.BGSQ_EINVAL
    assert lib.bgsq_mesh_triangles(None) == 0
    lib.bgsq_mesh_free(None)


def test_no_cpu_fallback_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the loud-failure path is covered on the CPU box")
    with pytest.raises(_native_query.BgsQueryError) as ei:
        MeshQuery(cube_mesh(), 0)
    assert ei.value.status == _native_query.BGSQ_EHIP and "no usable HIP device" in str(ei.value)
