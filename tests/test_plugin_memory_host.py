"""Who owns a `bgs_device_alloc` block on the Python side, and which C entry point a cloud upload reaches: the
constructors' unwinding, `free()` and use after it, the call order of `at()` and of the scratch users, the initial
entries, the upload routes and the import paths. Everything runs over a recording fake plugin or a recording fake
library. No GPU, no library. Sections 1 to 4 and 6 use only names that existed before `device_memory.py`, `entries.py` and
`resident.py` did, and pin what those modules must not have changed (`profiles/plugin_memory.md`)."""
import ctypes
import importlib

import numpy as np
import pytest

import bevy_gaussian_splatting_amd as bgs
from bevy_gaussian_splatting_amd import (
    CloudSettings, DeviceEntriesChunk, DeviceSortedEntries, GaussianSplattingPlugin, MorphPair, PlanarGaussian3dF16,
    ResidentCloud4d, SortedEntries, SparseSelect, random_gaussians_3d_seeded, random_gaussians_4d_seeded)
from bevy_gaussian_splatting_amd.interpolate import COV3D_WIDTHS, F32_WIDTHS
from bevy_gaussian_splatting_amd.particles import PARTICLE_BEHAVIOR_DTYPE, ParticleBehaviorsHandle
from bevy_gaussian_splatting_amd.plugin import DEVICE_PLANE_FORMATS, SORT_ENTRY_DTYPE

N = 3
STREAM = 0x5EED
LHS, RHS = random_gaussians_3d_seeded(N, 1), random_gaussians_3d_seeded(N, 2)
CLOUD_4D = random_gaussians_4d_seeded(N, 3)
SETTINGS = CloudSettings(time=0.25)


class Boom(Exception):
    pass


class RecordingPlugin:
    """What the owners of device memory need of a plugin, over a log. Addresses are distinct and 16-byte aligned.
    `fail_alloc` / `fail_upload`: the index of the `device_alloc` / `upload_bytes` call that raises."""

    def __init__(self, fail_alloc=None, fail_upload=None):
        self._ctx, self.device = object(), 0
        self.log, self.handed_out, self.freed, self.uploads = [], [], [], []
        self.fail_alloc, self.fail_upload, self.raised = fail_alloc, fail_upload, None
        self.allocs = 0

    def _maybe_fail(self, k, at):
        if k == at:
            self.raised = Boom(f"call {k}")
            raise self.raised

    def device_alloc(self, nbytes):
        self._maybe_fail(self.allocs, self.fail_alloc)
        self.allocs += 1
        addr = 0x7F0000000000 + 0x10000 * self.allocs
        self.handed_out.append(addr)
        self.log.append(("alloc", int(nbytes), addr))
        return addr

    def device_free(self, ptr):
        self.freed.append(ptr)
        self.log.append(("free", ptr))

    def upload_bytes(self, ptr, host):
        self._maybe_fail(len(self.uploads), self.fail_upload)
        self.uploads.append((ptr, np.array(host, copy=True)))
        self.log.append(("upload_bytes", ptr, host.nbytes))

    def download(self, ptr, host_out):
        self.log.append(("download", ptr, host_out.shape, host_out.dtype))
        return host_out

    def synchronize(self):
        self.log.append(("synchronize",))

    def stream_handle(self):
        return STREAM

    def upload_device_planes(self, fmt, n, pointers):
        self.log.append(("upload_device_planes", fmt, n, list(pointers)))
        return ("handle", len(self.log))


class FakeInterpolator:
    def __init__(self, plugin):
        self.log = plugin.log

    def interpolate(self, stream, n, lhs_ptrs, rhs_ptrs, out_ptrs, settings):
        self.log.append(("produce", stream, n, list(lhs_ptrs) + list(rhs_ptrs), list(out_ptrs), settings))


class FakeSlicer:
    def __init__(self, plugin):
        self.log = plugin.log

    def slice(self, stream, n, in_ptrs, out_ptrs, settings):
        self.log.append(("produce", stream, n, list(in_ptrs), list(out_ptrs), settings))


def morph_f32(p, lhs=LHS, rhs=RHS):
    return MorphPair(p, lhs, rhs, interpolator=FakeInterpolator(p))


def morph_cov3d(p, lhs=LHS, rhs=RHS):
    return MorphPair(p, lhs, rhs, precompute_covariance_3d=True, interpolator=FakeInterpolator(p))


def resident_4d(p, cloud=CLOUD_4D):
    return ResidentCloud4d(p, cloud, slicer=FakeSlicer(p))


def sorted_entries(p):
    return DeviceSortedEntries(p, 2, N)


# what each makes: (constructor, device_alloc calls, upload_bytes calls, output widths, cloud format)
RESIDENT = {
    "morph_f32": (morph_f32, 12, 8, F32_WIDTHS, "f32"),
    "morph_cov3d": (morph_cov3d, 9, 6, COV3D_WIDTHS, "cov3d"),
    "resident_4d": (resident_4d, 8, 5, (4, 48, 8), "cov3d"),
}
OWNERS = dict(RESIDENT, sorted_entries=(sorted_entries, 1, 1, None, None))


# -- 1. failure at every step of construction ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(OWNERS))
def test_a_constructor_that_fails_frees_what_it_was_handed_exactly_once(kind):
    make, allocs, uploads = OWNERS[kind][:3]
    whole = RecordingPlugin()
    make(whole)
    assert (whole.allocs, len(whole.uploads), whole.freed) == (allocs, uploads, [])
    for where, count in (("fail_alloc", allocs), ("fail_upload", uploads)):
        for k in range(count):
            p = RecordingPlugin(**{where: k})
            with pytest.raises(Boom) as ei:
                make(p)
            assert ei.value is p.raised, (where, k)
            assert sorted(p.freed) == sorted(p.handed_out), (where, k)          # every block, and each once
            assert len(set(p.freed)) == len(p.freed), (where, k)
            assert len(p.handed_out) == k or where == "fail_upload", (where, k)  # nothing is allocated behind a failure


# -- 2. free() and use after free ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(RESIDENT))
def test_a_resident_producer_frees_once_and_refuses_use_after_free(kind):
    make = RESIDENT[kind][0]
    p = RecordingPlugin()
    r = make(p)
    assert len(r) == N
    r.free()
    r.free()
    assert sorted(p.freed) == sorted(p.handed_out) and len(set(p.freed)) == len(p.freed)
    with pytest.raises(RuntimeError, match="was freed"):
        r.at(SETTINGS)
    # a closed plugin has released its memory itself: no call
    p = RecordingPlugin()
    r = make(p)
    p._ctx = None
    before = list(p.log)
    r.free()
    assert p.log == before
    with pytest.raises(RuntimeError, match="was freed"):
        r.at(SETTINGS)
    # `with` frees on exit ...
    p = RecordingPlugin()
    with make(p) as r:
        assert p.freed == []
    assert sorted(p.freed) == sorted(p.handed_out)
    # ... and on an exception, which it lets through
    p = RecordingPlugin()
    with pytest.raises(Boom):
        with make(p):
            raise Boom()
    assert sorted(p.freed) == sorted(p.handed_out) and len(set(p.freed)) == len(p.freed)


def test_device_sorted_entries_free_once_and_ptr_none():
    p = RecordingPlugin()
    e = sorted_entries(p)
    assert e.ptr == p.handed_out[0]
    e.free()
    e.free()
    assert p.freed == p.handed_out and e.ptr is None
    with pytest.raises(ValueError, match="the entries have been freed"):
        e.chunk(0)
    p = RecordingPlugin()
    e = sorted_entries(p)
    p._ctx = None
    before = list(p.log)
    e.free()
    assert p.log == before and e.ptr is None


# -- the recording library: stands where the loaded one would -------------------------------------------------------------
ROW_BYTES = {"position_visibility": 16, "spherical_harmonic": 192, "spherical_harmonic_h2": 96, "rotation": 16,
             "scale_opacity": 16, "rotation_scale_opacity": 16, "covariance_3d_opacity": 32}
CLOUD_UPLOADS = {entry: names for entry, names, _ in DEVICE_PLANE_FORMATS.values()}
CLOUD_HANDLE = 0xC10D0


def address(arg):
    return ctypes.cast(arg, ctypes.c_void_p).value or 0


class RecordingLibrary:
    """Logs the calls the tests expect and answers BGS_OK; any other call fails the test. A cloud upload logs, for every
    plane, its address and the bytes that lie there during the call."""

    def __init__(self, log):
        self.log, self.allocs = log, 0

    def __getattr__(self, name):
        if name not in CLOUD_UPLOADS and not hasattr(type(self), "_" + name):
            raise AssertionError(f"the library was called ({name})")
        return lambda *args: self._call(name, *args)

    def _call(self, name, ctx, *args):
        if name in CLOUD_UPLOADS:
            n, planes, out = args[0], args[1:-1], args[-1]
            assert len(planes) == len(CLOUD_UPLOADS[name])
            self.log.append((name, n, [(address(a), ctypes.string_at(address(a), n * ROW_BYTES[plane]))
                                       for a, plane in zip(planes, CLOUD_UPLOADS[name])]))
            out._obj.value = CLOUD_HANDLE
        else:
            getattr(self, "_" + name)(*args)
        return 0

    def _bgs_device_alloc(self, nbytes, out):
        self.allocs += 1
        out._obj.value = 0x7E0000000000 + 0x10000 * self.allocs
        self.log.append(("bgs_device_alloc", int(nbytes), out._obj.value))

    def _bgs_device_free(self, ptr):
        self.log.append(("bgs_device_free", ptr.value))

    def _bgs_upload(self, dst, src, nbytes):
        self.log.append(("bgs_upload", dst.value, ctypes.string_at(src, nbytes)))

    def _bgs_download(self, src, dst, nbytes):
        ctypes.memset(dst, 0, nbytes)
        self.log.append(("bgs_download", src.value, nbytes))

    def _bgs_synchronize(self):
        self.log.append(("bgs_synchronize",))

    def _bgs_stream(self, out):
        out._obj.value = STREAM


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def bare_plugin(library):
    """A plugin object over `library` instead of the loaded one (tests/test_device_hand_off_host.py)."""
    p = object.__new__(GaussianSplattingPlugin)
    p._lib, p._ctx, p.device = library, ctypes.c_void_p(0xC7C7), 0
    return p


def test_particle_behaviors_handle_free_once_and_ptr_zero():
    for count in (2, 0):
        log = []
        p = bare_plugin(RecordingLibrary(log))
        records = np.zeros(count, PARTICLE_BEHAVIOR_DTYPE)
        h = p.upload_particle_behaviors(records)
        assert isinstance(h, ParticleBehaviorsHandle) and len(h) == count
        ptr = log[0][2]
        expect = [("bgs_device_alloc", max(64 * count, 64), ptr)]      # never fewer than 64 bytes
        if count:
            expect.append(("bgs_upload", ptr, records.tobytes()))
        assert log == expect and h.ptr == ptr
        h.free()
        h.free()
        assert log[len(expect):] == [("bgs_device_free", ptr)] and h.ptr == 0
        h = p.upload_particle_behaviors(records)
        p._ctx = None
        before = list(log)
        h.free()
        assert log == before and h.ptr == 0


# -- 3. the call log of at() -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("return_planes", (False, True))
@pytest.mark.parametrize("kind", sorted(RESIDENT))
def test_at_enqueues_the_producer_then_uploads_then_downloads(kind, return_planes):
    make, allocs, _, widths, fmt = RESIDENT[kind]
    p = RecordingPlugin()
    r = make(p)
    k = len(widths)
    in_ptrs, out_ptrs = p.handed_out[:allocs - k], p.handed_out[allocs - k:]
    assert [e[1] for e in p.log if e[0] == "alloc"][allocs - k:] == [N * w * 4 for w in widths]
    del p.log[:]
    result = r.at(SETTINGS, return_planes=return_planes)
    produce, upload, downloads = p.log[0], p.log[1], p.log[2:]
    assert produce[0] == "produce" and produce[1:5] == (STREAM, N, in_ptrs, out_ptrs) and produce[5] is SETTINGS
    assert upload == ("upload_device_planes", fmt, N, out_ptrs)             # (no synchronize in between: the log has none)
    if return_planes:
        handle, planes = result
        assert downloads == [("download", ptr, (N, w), np.dtype(np.float32)) for ptr, w in zip(out_ptrs, widths)]
        assert isinstance(planes, tuple) and [a.shape for a in planes] == [(N, w) for w in widths]
    else:
        handle = result
        assert downloads == []
    assert handle == ("handle", 2)
    r.free()


@pytest.mark.parametrize("return_planes", (False, True))
@pytest.mark.parametrize("kind", sorted(RESIDENT))
def test_at_of_an_empty_cloud_allocates_nothing_and_uploads_null_planes(kind, return_planes):
    make, _, _, widths, fmt = RESIDENT[kind]
    p = RecordingPlugin()
    r = make(p, CLOUD_4D.slice(0, 0)) if kind == "resident_4d" else make(p, LHS.slice(0, 0), RHS.slice(0, 0))
    assert len(r) == 0 and p.log == []
    result = r.at(SETTINGS, return_planes=return_planes)
    assert p.log == [("upload_device_planes", fmt, 0, [0] * len(widths))]
    if return_planes:
        assert result[0] == ("handle", 1) and [a.shape for a in result[1]] == [(0, w) for w in widths]
    else:
        assert result == ("handle", 1)
    r.free()
    assert len(p.log) == 1
    r.at(SETTINGS)      # an empty producer owns nothing that a free could take away


# -- 4. the scratch users ---------------------------------------------------------------------------------------------------
class FakeMesh:
    def __init__(self, log, fail=None):
        self.log, self.fail = log, fail

    def _step(self, name, *args):
        self.log.append((name,) + args)
        if self.fail == name:
            raise Boom(name)

    def crossings(self, stream, points_ptr, n, matrix, scratch):
        self._step("crossings", stream, points_ptr, n, matrix, int(scratch))

    def entries_keep(self, stream, entries_ptr, count, scratch, n, outside=False):
        self._step("entries_keep", stream, entries_ptr, count, int(scratch), n, outside)


class FakeGrid(FakeMesh):
    def neighbor_counts(self, stream, points_ptr, n, radius, scratch, cap=None):
        self._step("neighbor_counts", stream, points_ptr, n, radius, int(scratch), cap)

    def entries_keep(self, stream, entries_ptr, count, scratch, n, threshold, dense=False):
        self._step("entries_keep", stream, entries_ptr, count, int(scratch), n, threshold, dense)


POINTS, CHUNK, SELECT = 0x9000, DeviceEntriesChunk(0xA000, 5), SparseSelect(radius=0.5, neighbor_threshold=4)


def scratch_user(name, p, log, n, chunk=CHUNK, fail=None):
    if name == "keep_inside_mesh":
        return p.keep_inside_mesh(chunk, POINTS, FakeMesh(log, fail), matrix=None, outside=True, n=n)
    if name == "keep_sparse":
        return p.keep_sparse(chunk, POINTS, FakeGrid(log, fail), SELECT, dense=True, n=n)
    return p.sparse_select(POINTS, n, FakeGrid(log, fail), SELECT)


def expected_launches(name, n, scratch):
    if name == "keep_inside_mesh":
        return [("crossings", STREAM, POINTS, n, None, scratch), ("entries_keep", STREAM, CHUNK.ptr, CHUNK.count, scratch, n, True)]
    counts = ("neighbor_counts", STREAM, POINTS, n, 0.5, scratch, 4)
    if name == "keep_sparse":
        return [counts, ("entries_keep", STREAM, CHUNK.ptr, CHUNK.count, scratch, n, 4, True)]
    return [counts]


@pytest.mark.parametrize("name", ("keep_inside_mesh", "keep_sparse", "sparse_select"))
def test_a_scratch_user_synchronises_launches_synchronises_and_frees(name):
    n = 7
    log = []
    result = scratch_user(name, bare_plugin(RecordingLibrary(log)), log, n)
    scratch = log[1][2]
    tail = [("bgs_download", scratch, 4 * n)] if name == "sparse_select" else []
    assert log == [("bgs_synchronize",), ("bgs_device_alloc", 4 * n, scratch)] + expected_launches(name, n, scratch) + \
        [("bgs_synchronize",)] + tail + [("bgs_device_free", scratch)]
    if name == "sparse_select":
        assert result.dtype == np.uint32 and list(result) == list(range(n))     # downloaded counts of 0: every splat is sparse
    else:
        assert result is None
    # either launch raising: the block is freed, once, and the exception comes through
    for k, launch in enumerate(expected_launches(name, n, scratch)):
        log = []
        with pytest.raises(Boom, match=launch[0]):
            scratch_user(name, bare_plugin(RecordingLibrary(log)), log, n, fail=launch[0])
        assert [e[0] for e in log] == ["bgs_synchronize", "bgs_device_alloc"] + [e[0] for e in expected_launches(name, n, 0)[:k + 1]] + \
            ["bgs_device_free"]
        assert log[-1][1] == log[1][2]
    # nothing to do: the frames in flight are completed all the same, and nothing else happens
    empties = [dict(n=0)] + ([dict(n=n, chunk=DeviceEntriesChunk(0xA000, 0))] if name != "sparse_select" else [])
    for kw in empties:
        log = []
        result = scratch_user(name, bare_plugin(RecordingLibrary(log)), log, **kw)
        assert log == [("bgs_synchronize",)]
        if name == "sparse_select":
            assert result.dtype == np.uint32 and result.shape == (0,)


# -- 5. the initial entries -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cameras,count", ((1, 0), (1, 5), (3, 4)))
def test_initial_entries_are_what_both_classes_start_from(cameras, count):
    from bevy_gaussian_splatting_amd.entries import initial_entries
    init = initial_entries(cameras, count)
    assert init.dtype == SORT_ENTRY_DTYPE and init.shape == (cameras * count,)
    assert (init["key"] == 1).all() and np.array_equal(init["index"], np.tile(np.arange(count, dtype=np.uint32), cameras))
    assert np.array_equal(SortedEntries.new(cameras, count).sorted, init)
    p = RecordingPlugin()
    e = DeviceSortedEntries(p, cameras, count)
    assert [a[1] for a in p.log if a[0] == "alloc"] == [max(8 * cameras * count, 8)]
    if count:
        (ptr, uploaded), = p.uploads
        assert ptr == e.ptr and uploaded.dtype == SORT_ENTRY_DTYPE and np.array_equal(uploaded, init)
    else:
        assert p.uploads == []
    assert [DeviceSortedEntries.chunk_offset(c, count) for c in range(cameras + 1)] == [8 * c * count for c in range(cameras + 1)]
    assert [(e.chunk(c).ptr, e.chunk(c).count) for c in range(cameras)] == [(e.ptr + 8 * c * count, count) for c in range(cameras)]
    for bad in (-1, cameras):
        with pytest.raises(IndexError, match="camera chunk out of range"):
            e.chunk(bad)
    host = SortedEntries.new(cameras, count)
    if count:                                                   # (an empty chunk lies inside an empty array wherever it is)
        with pytest.raises(IndexError, match="camera chunk out of range"):
            host.chunk(cameras)
    assert host.chunk(cameras - 1).shape == (count,)


# -- 6. the upload routes -----------------------------------------------------------------------------------------------------
def host_planes(fmt, cloud):
    if fmt == "cov3d":
        return cloud.position_visibility, cloud.spherical_harmonic, np.ascontiguousarray(bgs.covariance_3d_opacity(cloud), np.float32)
    return tuple(getattr(cloud, name.replace("_h2", "")) for name in DEVICE_PLANE_FORMATS[fmt][1])


@pytest.mark.parametrize("route", ("f32", "f16", "cov3d", "covariance_planes"))
def test_an_upload_calls_the_entry_point_its_format_names(route):
    fmt = "cov3d" if route == "covariance_planes" else route
    entry, names, splat_bytes = DEVICE_PLANE_FORMATS[fmt]
    assert sum(ROW_BYTES[name] for name in names) == splat_bytes
    cloud = PlanarGaussian3dF16.from_f32(LHS) if fmt == "f16" else LHS
    planes = host_planes(fmt, cloud)
    log = []
    p = bare_plugin(RecordingLibrary(log))
    if route == "covariance_planes":
        handle = p.upload_covariance_planes(*planes)
    else:
        handle = p.upload(cloud, precompute_covariance_3d=(fmt == "cov3d"))
    (called, n, seen), = log                                        # exactly one call, of the table's entry point
    assert called == entry and n == N
    assert [content for _, content in seen] == [a.tobytes() for a in planes]       # the planes in the table's order, alive
    if route in ("f32", "f16"):
        assert [addr for addr, _ in seen] == [a.ctypes.data for a in planes]        # ... and where the cloud keeps them
    assert (handle.format, handle.n, len(handle), handle.nbytes) == (fmt, N, N, N * splat_bytes)
    assert handle._ptr.value == CLOUD_HANDLE and handle._plugin is p


def test_a_cloud_is_as_many_bytes_as_its_format_states():
    for n in (0, 1, N, 1000):
        cloud = random_gaussians_3d_seeded(n, 5) if n else LHS.slice(0, 0)
        assert len(cloud) == n and cloud.nbytes() == n * DEVICE_PLANE_FORMATS["f32"][2]
        assert PlanarGaussian3dF16.from_f32(cloud).nbytes() == n * DEVICE_PLANE_FORMATS["f16"][2]


def test_the_uploads_refuse_on_the_host_before_any_library_call():
    p = bare_plugin(NoLibrary())
    with pytest.raises(TypeError, match="cloud must be PlanarGaussian3d or PlanarGaussian3dF16"):
        p.upload(CLOUD_4D)
    for cloud in (PlanarGaussian3dF16.from_f32(LHS), CLOUD_4D):
        with pytest.raises(TypeError, match="precompute_covariance_3d needs an f32 PlanarGaussian3d"):
            p.upload(cloud, precompute_covariance_3d=True)
    pv, sh, cov = host_planes("cov3d", LHS)
    for planes in ((pv[:, :3], sh, cov), (pv, sh[:, :47], cov), (pv, sh, cov[:, :6]), (pv, sh[:2], cov), (pv, sh, cov[:1])):
        with pytest.raises(ValueError, match=r"expected planes of shape \[n, 4\], \[n, 48\] and \[n, 8\]"):
            p.upload_covariance_planes(*planes)
    with pytest.raises(TypeError, match="behaviors must be ParticleBehaviors or a 1-D array of PARTICLE_BEHAVIOR_DTYPE"):
        p.upload_particle_behaviors(np.zeros(4, np.float32))
    with pytest.raises(ValueError, match="depth must be"):
        p.upload_depth(np.zeros((4, 4, 3), np.float32))


# -- 7. the import paths ---------------------------------------------------------------------------------------------------------
HOMES = {"entries": ("SORT_ENTRY_DTYPE", "SortedEntries", "DeviceEntriesChunk", "DeviceSortedEntries"),
         "resident": ("MorphPair", "ResidentCloud4d"),
         "plugin": ("PreparedView", "PlanarGaussian3dHandle", "DEVICE_PLANE_FORMATS", "GaussianSplattingPlugin"),
         "particles": ("ParticleBehaviorsHandle",)}
FROM_THE_PACKAGE = ("SORT_ENTRY_DTYPE", "SortedEntries", "DeviceEntriesChunk", "DeviceSortedEntries", "MorphPair", "ResidentCloud4d",
                    "PlanarGaussian3dHandle", "GaussianSplattingPlugin", "ParticleBehaviorsHandle")


def test_every_public_name_is_importable_from_its_old_path_and_is_one_object():
    plugin = importlib.import_module("bevy_gaussian_splatting_amd.plugin")
    for module, names in HOMES.items():
        home = importlib.import_module("bevy_gaussian_splatting_amd." + module)
        for name in names:
            obj = getattr(home, name)
            if module != "particles":
                assert getattr(plugin, name) is obj, name         # the old path of all of them
            if name in FROM_THE_PACKAGE:
                assert getattr(bgs, name) is obj and name in bgs.__all__, name
            if isinstance(obj, type):
                assert obj.__module__ == home.__name__, name      # defined there, not passed through
    from bevy_gaussian_splatting_amd.device_memory import DeviceBlock
    assert DeviceBlock.__module__ == "bevy_gaussian_splatting_amd.device_memory"


def test_device_block_is_the_one_owner():
    from bevy_gaussian_splatting_amd.device_memory import DeviceBlock
    p = RecordingPlugin()
    init = np.arange(6, dtype=np.float32)
    with DeviceBlock.allocate(p, 24, init) as block:
        assert (block.ptr, block.nbytes) == (p.handed_out[0], 24) and np.array_equal(p.uploads[0][1], init)
        assert p.freed == []
    assert p.freed == p.handed_out and not block.ptr
    block.free()
    assert p.freed == p.handed_out
    # an empty `init` is not uploaded; a failing upload frees the block and comes through
    p = RecordingPlugin()
    DeviceBlock.allocate(p, 64, np.zeros(0, np.float32))
    assert p.uploads == [] and [e[0] for e in p.log] == ["alloc"]
    p = RecordingPlugin(fail_upload=0)
    with pytest.raises(Boom) as ei:
        DeviceBlock.allocate(p, 24, init)
    assert ei.value is p.raised and p.freed == p.handed_out and len(p.freed) == 1
    # the plugin's own method is the same thing over the library
    log = []
    q = bare_plugin(RecordingLibrary(log))
    with q.device_block(24, init) as block:
        assert isinstance(block, DeviceBlock) and log == [("bgs_device_alloc", 24, block.ptr), ("bgs_upload", block.ptr, init.tobytes())]
    assert log[-1][0] == "bgs_device_free" and len(log) == 3
    q = bare_plugin(RecordingLibrary([]))
    block = q.device_block(16)
    q._ctx = None
    block.free()
    assert q._lib.log == [("bgs_device_alloc", 16, q._lib.log[0][2])] and not block.ptr
