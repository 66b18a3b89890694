"""Point-in-mesh selection on the device (libbgs_query.so): every comparison is BITWISE against the numpy twin
`crossings_reference` (tests/test_mesh_query_host.py ties the twin to the compiled arithmetic and to geometry). The
selection reaches the draw only through a kept chunk, whose frames are compared bitwise too."""
import ctypes

import numpy as np
import pytest

import mesh_query_cases as C
from bevy_gaussian_splatting_amd import (
    CloudSettings, DrawMode, MeshQuery, PlanarGaussian3d, SortMode, View, _native_query, crossings_reference, cube_mesh,
    mesh_from_points, random_gaussians_3d_seeded, rotation_y, transform_from)
from bevy_gaussian_splatting_amd.mesh_query import CULLED_KEY, keep_reference
from bevy_gaussian_splatting_amd.plugin import SORT_ENTRY_DTYPE

pytestmark = pytest.mark.gpu

N = 5000
W = HT = 128
SIZES = (1, 63, 64, 65, 5000)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def float4(points):
    p = np.asarray(points, np.float32)
    if p.shape[1] == 4:
        return np.ascontiguousarray(p)
    out = np.ones((p.shape[0], 4), np.float32)
    out[:, :3] = p
    return out


class DevicePoints:
    """n float4 points and an n-word counts plane in device memory of the plugin's context; the plane starts as garbage."""

    def __init__(self, plugin, points):
        self.plugin = plugin
        p = float4(points)
        self.n = p.shape[0]
        self.points = plugin.device_alloc(max(p.nbytes, 16))
        self.counts = plugin.device_alloc(max(4 * self.n, 16))
        plugin.upload_bytes(self.points, p)

    def crossings(self, mesh_query, matrix=None, n=None):
        n = self.n if n is None else n
        self.plugin.upload_bytes(self.counts, np.full(self.n, 0xDEADBEEF, np.uint32))
        mesh_query.crossings(self.plugin.stream_handle(), self.points, n, matrix, self.counts)
        self.plugin.synchronize()
        return self.plugin.download(self.counts, np.empty(self.n, np.uint32))

    def free(self):
        self.plugin.device_free(self.points)
        self.plugin.device_free(self.counts)


@pytest.fixture()
def quiet(plugin):
    plugin.set_async(False)
    plugin.set_pipeline_depth(1)
    plugin.set_binning("scan")
    plugin.reset_adaptive_state()
    yield plugin
    plugin.set_async(False)
    plugin.set_pipeline_depth(1)


# ---- 1. crossing counts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix", ["identity", "affine"])
@pytest.mark.parametrize("triangles", C.TRIANGLE_COUNTS)
def test_crossing_counts_equal_the_twin(quiet, triangles, matrix):
    want = C.cloud_reference(triangles, matrix)
    dp = DevicePoints(quiet, C.cloud_points(matrix))
    try:
        with MeshQuery(C.mesh_with(triangles), quiet.device) as mq:
            assert mq.triangle_count == triangles == mq._lib.bgsq_mesh_triangles(mq._ptr)
            for n in SIZES:
                got = dp.crossings(mq, C.matrix_of(matrix), n)
                assert same_bits(got[:n], want[:n]), (triangles, matrix, n)
                assert (got[n:] == 0xDEADBEEF).all()   # nothing is written past n
    finally:
        dp.free()
    if triangles >= 12:
        assert 0 < int((want & 1).sum()) < N   # some inside, some outside
    if triangles == 1283:
        assert same_bits(want, C.cloud_reference(1280, matrix))
    if triangles == 0:
        assert not want.any()


# ---- 2. slices ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 5000])
def test_the_counts_do_not_depend_on_the_slices(quiet, n):
    want = C.cloud_reference(1280, "affine")
    dp = DevicePoints(quiet, C.cloud_points("affine"))
    try:
        with MeshQuery(C.sphere(), quiet.device) as mq:
            for slices in (1, 2, 7, 0):   # 7 does not divide 1280; 0 = automatic
                mq.set_slices(slices)
                assert same_bits(dp.crossings(mq, C.matrix_of("affine"), n)[:n], want[:n]), slices
            mq.set_slices(5000)   # more than there are triangles, or than the grid allows: clamped
            assert same_bits(dp.crossings(mq, C.matrix_of("affine"), n)[:n], want[:n])
    finally:
        dp.free()


# ---- 3. boundary and non-finite -------------------------------------------------------------------------------------------------
def test_boundary_lattice_and_non_finite_points_on_the_device(quiet):
    for points, mesh, want in ((C.lattice_points(), cube_mesh(), C.lattice_reference()),
                               (C.nonfinite_points(), C.sphere(), C.nonfinite_reference())):
        dp = DevicePoints(quiet, points)
        try:
            with MeshQuery(mesh, quiet.device) as mq:
                for slices in (0, 1, 3):
                    mq.set_slices(slices)
                    assert same_bits(dp.crossings(mq), want), slices
        finally:
            dp.free()
    # 0 outside the cube's shadow, 1 inside, 2 in front of both x faces or on the +x face's diagonal, 4 in front of both
    # faces ON their diagonals (y == z), which both triangles of a face accept
    assert np.unique(C.lattice_reference()).tolist() == [0, 1, 2, 4] and (C.nonfinite_reference() > 0).any()


# ---- 4. the kept chunk, and the draw it drives -----------------------------------------------------------------------------------
def _hull():
    """An ellipsoid round the middle of what the headless camera sees of the cloud: (mesh GlobalTransform, matrix)."""
    t = transform_from((0.0, 1.5, -10.0), rotation_y(0.4)).astype(np.float64)
    t[:3, :3] = t[:3, :3] @ np.diag([6.0, 5.0, 8.0])
    return t, mesh_from_points(t)


def test_keep_inside_chunk_and_the_frames_it_draws(quiet):
    plugin = quiet
    cloud = random_gaussians_3d_seeded(N, 21)
    v, s = View.headless(W, HT, msaa_samples=4), CloudSettings(sort_mode=SortMode.Radix)
    _, matrix = _hull()
    sphere = C.sphere()
    crossings = crossings_reference(cloud.position_visibility, sphere.vertices, sphere.indices, matrix)
    inside = (crossings & 1).astype(bool)
    h = plugin.upload(cloud)
    dse = plugin.device_sorted_entries(2, h)
    points = plugin.device_alloc(cloud.position_visibility.nbytes)
    plugin.upload_bytes(points, cloud.position_visibility)
    selected = None
    try:
        with MeshQuery(sphere, plugin.device) as mq:
            entries = plugin.sort(h, v, s, into=dse.chunk(0))
            plugin.sort(h, v, s, download=False, into=dse.chunk(1))
            assert same_bits(dse.download(0), entries)
            live = entries["key"] != CULLED_KEY
            assert 20 < int((live & inside[entries["index"]]).sum()) < int(live.sum()) - 20   # the hull splits what the camera sees
            all_frame = plugin.render(h, v, s, entries=dse.chunk(0))
            # keep inside
            plugin.keep_inside_mesh(dse.chunk(0), points, mq, matrix)
            got = dse.download(0)
            want = keep_reference(entries, crossings)
            assert same_bits(got, want)
            assert same_bits(got["index"], entries["index"])                       # index and order untouched
            changed = got["key"] != entries["key"]
            assert (got["key"][changed] == CULLED_KEY).all() and not inside[entries["index"][changed]].any()
            assert same_bits(got[~live], entries[~live])                          # what the sort culled stays as it was
            # keep outside: the complement on the live entries
            plugin.keep_inside_mesh(dse.chunk(1), points, mq, matrix, outside=True)
            got_out = dse.download(1)
            assert same_bits(got_out, keep_reference(entries, crossings, outside=True))
            assert ((got["key"] == CULLED_KEY) ^ (got_out["key"] == CULLED_KEY))[live].all()
            assert same_bits(got_out[~live], entries[~live])
            # entries that name no point of the plane (index >= n) are left alone: a plane of the first 3000 points only
            plugin.sort(h, v, s, download=False, into=dse.chunk(1))
            plugin.keep_inside_mesh(dse.chunk(1), points, mq, matrix, n=3000)
            got_short = dse.download(1)
            assert same_bits(got_short, keep_reference(entries, crossings[:3000]))
            beyond = entries["index"] >= 3000
            assert same_bits(got_short[beyond], entries[beyond]) and (live & beyond & ~inside[entries["index"]]).any()
            # the selection drives the draw: the device-made chunk, a host-made chunk, and DrawMode::Selected
            frame = plugin.render(h, v, s, entries=dse.chunk(0))
            dse.upload(1, want)
            host_frame = plugin.render(h, v, s, entries=dse.chunk(1))
            assert np.array_equal(frame, host_frame)
            assert not np.array_equal(frame, all_frame) and np.abs(frame[..., :3]).max() > 0.05
            pv = cloud.position_visibility.copy()
            pv[:, 3] = inside.astype(np.float32)
            selected = plugin.upload(PlanarGaussian3d(pv, cloud.spherical_harmonic, cloud.rotation, cloud.scale_opacity))
            selected_frame = plugin.render(selected, v, CloudSettings(sort_mode=SortMode.Radix, draw_mode=DrawMode.Selected))
            assert np.array_equal(frame, selected_frame)
    finally:
        if selected is not None:
            selected.free()
        plugin.device_free(points)
        dse.free()
        h.free()


# ---- 5. stream ordering -------------------------------------------------------------------------------------------------------
def test_mesh_create_and_free_around_frames_in_flight(quiet):
    """Twelve async frames, four in flight; a mesh is created, queried and freed between them. Every frame is the blocking
    frame bit for bit, and the counts are the twin's: the query ran on bgs_stream(ctx), nowhere else."""
    plugin = quiet
    cloud = random_gaussians_3d_seeded(N, 21)
    s = CloudSettings()
    views = (View.headless(W, HT, yaw=0.0), View.headless(W, HT, yaw=0.3))
    _, matrix = _hull()
    sphere = C.sphere()
    want_counts = crossings_reference(cloud.position_visibility, sphere.vertices, sphere.indices, matrix)
    h = plugin.upload(cloud)
    dp = DevicePoints(plugin, cloud.position_visibility)
    planes = [plugin.device_alloc(4 * N) for _ in range(4)]   # one per query: two of them may run at the same time
    try:
        want = [plugin.render(h, view, s) for view in views]
        for plane in planes:
            plugin.upload_bytes(plane, np.full(N, 0xDEADBEEF, np.uint32))
        plugin.set_pipeline_depth(4)
        plugin.set_async(True)
        got, expected, held, queries = [], [], [], 0

        def pop():
            ptr, _ = plugin.pipeline_pop()
            got.append(plugin.download(ptr, np.empty((HT, W, 4), np.float32)))

        for f in range(12):
            if plugin.frames_in_flight() == 4:
                pop()
            plugin.render(h, views[f % 2], s, download=False)
            expected.append(f % 2)
            if f % 3 == 1:
                assert plugin.frames_in_flight() >= 2
                mq = MeshQuery(sphere, plugin.device)                      # created with frames in flight
                mq.crossings(plugin.stream_handle(), dp.points, N, matrix, planes[queries])
                queries += 1
                held.append(mq)
            elif held:
                held.pop().free()                                          # freed with frames (and its launch) in flight
        while plugin.frames_in_flight():
            pop()
        plugin.synchronize()
        assert queries == 4 and not held
        for plane in planes:
            assert same_bits(plugin.download(plane, np.empty(N, np.uint32)), want_counts)
        assert len(got) == 12 and all(same_bits(g, want[k]) for g, k in zip(got, expected))
        assert not same_bits(want[0], want[1])
    finally:
        plugin.set_async(False)
        plugin.set_pipeline_depth(1)
        for plane in planes:
            plugin.device_free(plane)
        dp.free()
        h.free()


# ---- 6. errors on a live device ------------------------------------------------------------------------------------------------
def test_errors_name_the_argument(quiet):
    with MeshQuery(cube_mesh(), quiet.device) as mq:
        stream = quiet.stream_handle()
        with pytest.raises(_native_query.BgsQueryError, match="points_device_ptr") as ei:
            mq.crossings(stream, 8, 4, None, 16)
        assert ei.value.status == _native_query.BGSQ_EINVAL
        with pytest.raises(_native_query.BgsQueryError, match="crossings_device_ptr"):
            mq.crossings(stream, 16, 4, None, 0)
        mq.crossings(stream, 0, 0, None, 0)          # n == 0: nothing is enqueued, nothing is looked at
        mq.entries_keep(stream, 0, 0, 0, 0)
    with pytest.raises(_native_query.BgsQueryError, match="no usable HIP device 99"):
        MeshQuery(cube_mesh(), 99)
    assert ctypes.sizeof(ctypes.c_void_p) == 8 and SORT_ENTRY_DTYPE.itemsize == 8
