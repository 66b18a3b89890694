"""Point-in-mesh selection (src/query/raycast.rs): which splats lie inside a triangle mesh, by the parity of the triangles
a +x ray from the splat's mesh-local position crosses.

The counting runs on the device (`bgsq_crossings`, csrc_query/mesh_query_kernels.hip, through libbgs_query.so) on points
and entries that live in device memory; this module holds the host-side mesh with its validation, two mesh generators,
the ctypes wrapper `MeshQuery`, and `crossings_reference`, a numpy twin of the arithmetic contract
(csrc_query/mesh_query_math.h) that the tests compare the device with bit for bit.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _native_query

RAY_EPSILON = np.float32(1e-6)   # `let epsilon = 0.000_001;` (raycast.rs:93)
KEEP_INSIDE = _native_query.BGSQ_KEEP_INSIDE
KEEP_OUTSIDE = _native_query.BGSQ_KEEP_OUTSIDE
CULLED_KEY = 0xFFFFFFFF


def validate(vertices: np.ndarray, indices: np.ndarray) -> None:
    """What `bgsq_mesh_create` refuses, checked on the host with the same words: a non-finite vertex, an index that
    names no vertex."""
    bad = np.argwhere(~np.isfinite(vertices))
    if bad.size:
        raise ValueError(f"vertex {int(bad[0][0])} has a non-finite {'xyz'[int(bad[0][1])]}")
    if indices.size and int(indices.max()) >= vertices.shape[0]:
        t = int(np.argwhere(indices >= vertices.shape[0])[0][0])
        raise ValueError(f"triangle {t} names vertex {int(indices[t].max())}, the mesh has {vertices.shape[0]}")


class TriangleMesh:
    """A triangle list as the reference reads one (`Mesh::ATTRIBUTE_POSITION` as float3, `Indices::U32`, TriangleList):
    `vertices` [V, 3] float32, `indices` [T, 3] uint32, validated (`validate`). T = 0 is legal: nobody is inside."""

    def __init__(self, vertices, indices):
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        i = np.asarray(indices)
        if v.ndim != 2 or v.shape[1] != 3:
            raise TypeError("vertices must be [V, 3]")
        if i.size == 0:
            i = np.zeros((0, 3), np.uint32)
        if i.ndim != 2 or i.shape[1] != 3 or not np.issubdtype(i.dtype, np.integer):
            raise TypeError("indices must be an integer array [T, 3]")
        if i.size and (int(i.min()) < 0 or int(i.max()) > 0xFFFFFFFF):
            raise ValueError("indices must fit in uint32")
        i = np.ascontiguousarray(i, dtype=np.uint32)
        validate(v, i)
        self.vertices = v
        self.indices = i

    @property
    def triangle_count(self) -> int:
        return int(self.indices.shape[0])

    def transformed(self, matrix) -> "TriangleMesh":
        """The mesh with `matrix` (4x4, column-vector) applied to every vertex, in float64, rounded once."""
        m = np.asarray(matrix, np.float64)
        v = self.vertices.astype(np.float64) @ m[:3, :3].T + m[:3, 3]
        return TriangleMesh(v.astype(np.float32), self.indices)


def cube_mesh(half_extent: float = 0.5) -> TriangleMesh:
    """The axis-aligned cube [-h, h]^3 as 12 triangles, outward winding (two per face)."""
    h = float(half_extent)
    v = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], np.float32)   # index = 4 ix + 2 iy + iz
    quads = [(0, 1, 3, 2), (4, 6, 7, 5),   # -x, +x
             (0, 4, 5, 1), (2, 3, 7, 6),   # -y, +y
             (0, 2, 6, 4), (1, 5, 7, 3)]   # -z, +z
    tris = []
    for a, b, c, d in quads:
        tris += [(a, b, c), (a, c, d)]
    return TriangleMesh(v, np.array(tris, np.uint32))


def icosphere_mesh(subdivisions: int = 0, radius: float = 1.0) -> TriangleMesh:
    """An icosahedron, each triangle split in four `subdivisions` times, every vertex pushed onto the sphere of `radius`:
    20 * 4^subdivisions triangles (3 -> 1280), closed, outward winding. Built in float64, rounded once."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
             (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    verts = [np.array(v, np.float64) / np.linalg.norm(v) for v in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(int(subdivisions)):
        middle = {}

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in middle:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                middle[key] = len(verts) - 1
            return middle[key]

        split = []
        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            split += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = split
    return TriangleMesh((np.array(verts) * float(radius)).astype(np.float32), np.array(faces, np.uint32))


def mesh_from_points(mesh_transform, cloud_transform=None) -> np.ndarray:
    """inverse(mesh GlobalTransform) @ cloud GlobalTransform as a 4x4 float32 (column-vector) matrix: what takes a
    position of the cloud's plane into the mesh's local space (raycast.rs:43-46, with the cloud's own transform in front).
    Composed in float64 and rounded once."""
    m = np.linalg.inv(np.asarray(mesh_transform, np.float64))
    if cloud_transform is not None:
        m = m @ np.asarray(cloud_transform, np.float64)
    if m.shape != (4, 4):
        raise ValueError("transforms must be 4x4")
    return m.astype(np.float32)


def _matrix_f32(matrix) -> np.ndarray:
    m = np.asarray(np.eye(4) if matrix is None else matrix, dtype=np.float32)
    if m.shape != (4, 4):
        raise ValueError("mesh_from_points must be 4x4")
    return m


def local_points_reference(points: np.ndarray, matrix) -> np.ndarray:
    """xyz of M * (x, y, z, 1) as the kernel forms it: r = col0*x; r = col1*y + r; r = col2*z + r; r = col3 + r."""
    m = _matrix_f32(matrix)
    p = np.asarray(points, np.float32)
    x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    r = m[:3, 0][None, :] * x
    r = m[:3, 1][None, :] * y + r
    r = m[:3, 2][None, :] * z + r
    r = m[:3, 3][None, :] + r
    assert r.dtype == np.float32
    return r


def crossings_reference(points, vertices, indices, mesh_from_points=None, block: int = 2048) -> np.ndarray:
    """The crossing counts as the device computes them (csrc_query/mesh_query_math.h), op by op in float32, every
    operation rounded once. `points` is [n, 3] or [n, 4] (xyz read). Returns uint32 [n]; inside = crossings & 1."""
    pts = np.asarray(points, np.float32)
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    idx = np.asarray(indices, np.uint32).reshape(-1, 3)
    n = pts.shape[0]
    out = np.zeros(n, np.uint32)
    if n == 0 or idx.shape[0] == 0:
        return out
    with np.errstate(all="ignore"):
        p = local_points_reference(pts, mesh_from_points)
        finite = np.isfinite(p).all(axis=1)
        # per triangle
        v0 = v[idx[:, 0]]
        e1 = v[idx[:, 1]] - v0
        e2 = v[idx[:, 2]] - v0
        hy, hz = -e2[:, 2], e2[:, 1]
        a = e1[:, 1] * hy + e1[:, 2] * hz
        rejected = (a > -RAY_EPSILON) & (a < RAY_EPSILON)
        f = np.where(rejected, np.float32(np.nan), np.float32(1.0) / a).astype(np.float32)
        one, zero = np.float32(1.0), np.float32(0.0)
        for lo in range(0, n, block):
            q = p[lo:lo + block]
            sx = q[:, 0:1] - v0[None, :, 0]
            sy = q[:, 1:2] - v0[None, :, 1]
            sz = q[:, 2:3] - v0[None, :, 2]
            u = f[None, :] * (sy * hy[None, :] + sz * hz[None, :])
            qx = sy * e1[None, :, 2] - e1[None, :, 1] * sz
            qy = sz * e1[None, :, 0] - e1[None, :, 2] * sx
            qz = sx * e1[None, :, 1] - e1[None, :, 0] * sy
            vv = f[None, :] * qx
            t = f[None, :] * ((e2[None, :, 0] * qx + e2[None, :, 1] * qy) + e2[None, :, 2] * qz)
            assert u.dtype == vv.dtype == t.dtype == np.float32
            hit = (u >= zero) & (u <= one) & ~(vv < zero) & ~((u + vv) > one) & (t > RAY_EPSILON)
            out[lo:lo + block] = hit.sum(axis=1, dtype=np.uint32)
    out[~finite] = 0   # the stated deviation: a non-finite local position has no crossings
    return out


def keep_reference(entries: np.ndarray, crossings: np.ndarray, outside: bool = False) -> np.ndarray:
    """`bgsq_entries_keep` on host entries: a copy in which every entry with index < n and a live key whose point fails
    the predicate has key 0xFFFFFFFF. Index and order are untouched."""
    e = np.array(entries, copy=True)
    n = crossings.shape[0]
    named = (e["index"] < n) & (e["key"] != CULLED_KEY)
    inside = np.zeros(e.shape[0], bool)
    inside[named] = (crossings[e["index"][named]] & 1).astype(bool)
    e["key"][named & (inside == bool(outside))] = CULLED_KEY
    return e


class MeshQuery:
    """A `TriangleMesh` prepared on one HIP device (`bgsq_mesh`): its triangle records live in device memory until
    `free()`. `crossings` and `entries_keep` only enqueue on the stream they are given."""

    def __init__(self, mesh: TriangleMesh, device: int = 0):
        if not isinstance(mesh, TriangleMesh):
            raise TypeError("mesh must be a TriangleMesh")
        self._lib = _native_query.load()
        self.device = int(device)
        self.triangle_count = mesh.triangle_count
        out = ctypes.c_void_p()
        _native_query.check(self._lib, self._lib.bgsq_mesh_create(
            self.device, mesh.vertices.ctypes.data_as(ctypes.c_void_p), mesh.vertices.shape[0],
            mesh.indices.ctypes.data_as(ctypes.c_void_p), mesh.triangle_count, ctypes.byref(out)))
        self._ptr: Optional[ctypes.c_void_p] = out

    def free(self) -> None:
        if getattr(self, "_ptr", None) is not None:
            self._lib.bgsq_mesh_free(self._ptr)
            self._ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def _mesh(self):
        if self._ptr is None:
            raise ValueError("the mesh has been freed")
        return self._ptr

    def set_slices(self, slices: int) -> None:
        """`bgsq_debug_set_slices` (test hook): 0 = automatic."""
        _native_query.check(self._lib, self._lib.bgsq_debug_set_slices(self._mesh(), int(slices)))

    def crossings(self, stream: int, points_ptr: int, n: int, matrix, crossings_ptr: int) -> None:
        """Enqueue `bgsq_crossings` on `stream`: n points (float4, xyz read) at `points_ptr`, n uint32 out at
        `crossings_ptr`. `matrix` is the 4x4 (column-vector) mesh_from_points, None = identity."""
        m = np.ascontiguousarray(_matrix_f32(matrix).T).reshape(16)   # column-major
        _native_query.check(self._lib, self._lib.bgsq_crossings(
            self._mesh(), ctypes.c_void_p(stream or 0), ctypes.c_void_p(points_ptr or 0), int(n),
            m.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.c_void_p(crossings_ptr or 0)))

    def entries_keep(self, stream: int, entries_ptr: int, entry_count: int, crossings_ptr: int, n: int, outside: bool = False) -> None:
        """Enqueue `bgsq_entries_keep` on `stream`."""
        _native_query.check(self._lib, self._lib.bgsq_entries_keep(
            self.device, ctypes.c_void_p(stream or 0), ctypes.c_void_p(entries_ptr or 0), int(entry_count),
            ctypes.c_void_p(crossings_ptr or 0), int(n), KEEP_OUTSIDE if outside else KEEP_INSIDE))
