"""The device hand-off: `bgs_cloud_upload_*` given planes that lie in device memory (include/bgs.h "DEVICE PLANES"). A cloud
packed from device planes is the cloud uploaded from the same planes on the host: equal sort entries, and images equal
with `np.array_equal`. Then what stands on it: the upload ordered behind a producer on `bgs_stream`, and the resident
forms `ResidentCloud4d` / `MorphPair` against the host route. Frames are 64 x 64."""
import numpy as np
import pytest

from bevy_gaussian_splatting_amd import (
    CloudSettings, GaussianInterpolator, PlanarGaussian3d, TimeSlicer, View, _native, covariance_3d_opacity,
    random_gaussians_3d_seeded, random_gaussians_4d_seeded)
from bevy_gaussian_splatting_amd.interpolate import covariance_planes, planes_of

pytestmark = pytest.mark.gpu

W = H = 64
SIZES = (1, 255, 257, 4099)      # either side of a 256-thread block; 4099 divides by neither record stride (8 and 16 words)
FORMATS = ("f32", "f16", "cov3d")
DRAW = CloudSettings()


@pytest.fixture()
def quiet(plugin):
    plugin.set_async(False)
    plugin.set_pipeline_depth(1)
    plugin.reset_adaptive_state()
    yield plugin
    plugin.synchronize()
    plugin.set_async(False)
    plugin.set_pipeline_depth(1)


_clouds = {}


def cloud_of(n):
    """One random cloud a size, made once and left unchanged."""
    if n not in _clouds:
        _clouds[n] = random_gaussians_3d_seeded(n, 40 + n % 7)
    return _clouds[n]


def host_planes(fmt, cloud):
    """The planes of `cloud` in the order of the format's C entry point."""
    if fmt == "f32":
        return [np.ascontiguousarray(p) for p in (cloud.position_visibility, cloud.spherical_harmonic, cloud.rotation, cloud.scale_opacity)]
    if fmt == "f16":
        h = cloud.to_f16()
        return [np.ascontiguousarray(p) for p in (h.position_visibility, h.spherical_harmonic, h.rotation_scale_opacity)]
    return [np.ascontiguousarray(p, np.float32) for p in (cloud.position_visibility, cloud.spherical_harmonic, covariance_3d_opacity(cloud))]


def upload_host(plugin, fmt, cloud):
    """The cloud through the plugin's host uploads, as before device planes existed."""
    if fmt == "f32":
        return plugin.upload(cloud)
    if fmt == "f16":
        return plugin.upload(cloud.to_f16())
    return plugin.upload_covariance_planes(*host_planes("cov3d", cloud))


class DevicePlanes:
    """Host planes copied into device memory of the plugin's context (`device_alloc` + `upload_bytes`)."""

    def __init__(self, plugin, planes):
        self.plugin, self.host, self.ptrs = plugin, planes, []
        try:
            for p in planes:
                self.ptrs.append(plugin.device_alloc(max(p.nbytes, 16)))
                if p.nbytes:
                    plugin.upload_bytes(self.ptrs[-1], p)
        except BaseException:
            self.free()
            raise

    def unchanged(self):
        return all(np.array_equal(self.plugin.download(ptr, np.empty_like(p)).view(np.uint8), p.view(np.uint8))
                   for ptr, p in zip(self.ptrs, self.host) if p.nbytes)

    def free(self):
        ptrs, self.ptrs = self.ptrs, []
        for p in ptrs:
            self.plugin.device_free(p)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def views():
    return [View.headless(W, H, msaa_samples=s) for s in (1, 4)]


def assert_same_cloud(plugin, got, want, what):
    """Equal sort entries and, at sample counts 1 and 4, equal images. Returns the images of `got`."""
    assert len(got) == len(want) and got.format == want.format, what
    images = []
    for view in views():
        e_got, e_want = plugin.sort(got, view, DRAW), plugin.sort(want, view, DRAW)
        assert np.array_equal(e_got["key"], e_want["key"]) and np.array_equal(e_got["index"], e_want["index"]), what
        i_got, i_want = plugin.render(got, view, DRAW), plugin.render(want, view, DRAW)
        assert np.array_equal(i_got.view(np.uint32), i_want.view(np.uint32)), f"{what}: images differ at {view.msaa_samples} samples"
        images.append(i_got)
    return images


# ---- 1. a cloud from device planes is the cloud from host planes -------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_device_planes_give_the_host_planes_cloud(quiet, fmt, n):
    plugin, cloud = quiet, cloud_of(n)
    with DevicePlanes(plugin, host_planes(fmt, cloud)) as dev:
        got, want = plugin.upload_device_planes(fmt, n, dev.ptrs), upload_host(plugin, fmt, cloud)
        try:
            assert got.nbytes == want.nbytes
            images = assert_same_cloud(plugin, got, want, f"{fmt} n={n}")
            if n == SIZES[-1]:
                assert np.abs(images[0][..., :3]).max() > 0.0             # something was drawn
            assert dev.unchanged()
        finally:
            got.free()
            want.free()


# ---- 2. mixed planes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", range(4))
def test_one_device_plane_among_host_planes(quiet, on_device):
    """f32, 257 splats: plane `on_device` (0 = the position plane, which is copied, not packed in place) is on the device,
    the other three on the host, all through the C entry point itself."""
    plugin, n = quiet, 257
    cloud = cloud_of(n)
    planes = host_planes("f32", cloud)
    with DevicePlanes(plugin, [planes[on_device]]) as dev:
        pointers = [p.ctypes.data for p in planes]
        pointers[on_device] = dev.ptrs[0]
        got, want = plugin.upload_device_planes("f32", n, pointers), upload_host(plugin, "f32", cloud)
        try:
            assert_same_cloud(plugin, got, want, f"plane {on_device} on the device")
            assert dev.unchanged()
        finally:
            got.free()
            want.free()


# ---- 3. the edges ----------------------------------------------------------------------------------------------------------------------
def test_an_empty_cloud_from_device_pointers(quiet):
    plugin = quiet
    with DevicePlanes(plugin, host_planes("f32", cloud_of(1))) as dev:
        for fmt, count in (("f32", 4), ("f16", 3), ("cov3d", 3)):
            empty = plugin.upload_device_planes(fmt, 0, dev.ptrs[:count])
            try:
                assert len(empty) == 0 and empty.format == fmt
                view = views()[0]
                assert plugin.sort(empty, view, DRAW).shape == (0,)
                image = plugin.render(empty, view, DRAW)
                assert np.array_equal(image, np.broadcast_to(image[0, 0], image.shape))      # the clear colour everywhere
            finally:
                empty.free()
        assert dev.unchanged()


@pytest.mark.parametrize("fmt,plane", [("f32", 0), ("f32", 1), ("f32", 2), ("f32", 3), ("f16", 1), ("f16", 2), ("cov3d", 2)])
def test_a_misaligned_device_plane_is_refused_by_name(quiet, fmt, plane):
    from bevy_gaussian_splatting_amd.plugin import DEVICE_PLANE_FORMATS
    plugin, n = quiet, 255
    with DevicePlanes(plugin, host_planes(fmt, cloud_of(257))) as dev:        # (two rows more than are read: + 4 bytes stays inside)
        bad = list(dev.ptrs)
        bad[plane] += 4
        with pytest.raises(_native.BgsError, match=f"{DEVICE_PLANE_FORMATS[fmt][1][plane]} is a device plane and is not 16-byte aligned") as ei:
            plugin.upload_device_planes(fmt, n, bad)
        assert ei.value.status == _native.BGS_EINVAL
        good = plugin.upload_device_planes(fmt, n, dev.ptrs)                    # a correct upload right after it succeeds
        want = upload_host(plugin, fmt, cloud_of(257).slice(0, n))
        try:
            assert_same_cloud(plugin, good, want, f"{fmt} after a refusal")
        finally:
            good.free()
            want.free()
        # a HOST plane has no alignment rule, as before
        planes = host_planes(fmt, cloud_of(257))
        shifted = np.empty(planes[plane].nbytes + 4, np.uint8)
        shifted[4:] = planes[plane].view(np.uint8).reshape(-1)
        pointers = [p.ctypes.data for p in planes]
        pointers[plane] = shifted.ctypes.data + 4
        assert pointers[plane] % 16 != 0
        off = plugin.upload_device_planes(fmt, n, pointers)
        off.free()


def test_a_plane_on_a_second_device_is_refused(quiet):
    from bevy_gaussian_splatting_amd import GaussianSplattingPlugin
    try:
        second = GaussianSplattingPlugin(1)
    except _native.BgsError as e:
        assert e.status == _native.BGS_EINVAL and "hip_device out of range" in str(e)
        pytest.skip("needs two devices")
    plugin, n = quiet, 255
    planes = host_planes("f32", cloud_of(n))
    try:
        with DevicePlanes(second, [planes[2]]) as other:
            pointers = [p.ctypes.data for p in planes]
            pointers[2] = other.ptrs[0]
            with pytest.raises(_native.BgsError, match="rotation is memory of device 1, the context is on device 0") as ei:
                plugin.upload_device_planes("f32", n, pointers)
            assert ei.value.status == _native.BGS_EINVAL
        plugin.upload_device_planes("f32", n, [p.ctypes.data for p in planes]).free()
    finally:
        second.close()


# ---- 4. ordering behind a producer on bgs_stream ------------------------------------------------------------------------------------------
def test_the_upload_waits_for_a_slice_enqueued_on_bgs_stream(quiet):
    """Three asynchronous frames at pipeline depth 4 leave `bgs_stream` on a lane other than lane 0, whose stream packs.
    The slice of 100 000 splats is enqueued there into planes that hold zeros, nothing synchronises, and the upload
    follows: the cloud must be the slice's, not the zeros'."""
    plugin, n = quiet, 100_000
    cloud4d = random_gaussians_4d_seeded(n, 9)
    settings = CloudSettings(global_scale=0.75, time=0.4)
    want, planes = plugin.slice_4d(cloud4d, settings, return_planes=True)
    host = plugin.upload_covariance_planes(*planes)
    small = plugin.upload(cloud_of(4099))
    lane0_stream = plugin.stream_handle()
    ptrs = []
    try:
        for plane in cloud4d.planes():
            ptrs.append(plugin.device_alloc(plane.nbytes))
            plugin.upload_bytes(ptrs[-1], plane)
        for p in planes:
            ptrs.append(plugin.device_alloc(p.nbytes))
            plugin.upload_bytes(ptrs[-1], np.zeros_like(p))
        plugin.set_pipeline_streams(4)                      # (the default: each of the four lanes has a stream of its own)
        plugin.set_pipeline_depth(4)
        plugin.set_async(True)
        for view in (views() * 2)[:3]:
            plugin.render(small, view, DRAW, download=False)
        stream = plugin.stream_handle()
        assert stream != lane0_stream and plugin.frames_in_flight() > 0
        TimeSlicer(plugin.device).slice(stream, n, ptrs[:5], ptrs[5:], settings)
        got = plugin.upload_device_planes("cov3d", n, ptrs[5:])
        plugin.synchronize()
        plugin.set_async(False)
        plugin.set_pipeline_depth(1)
        try:
            assert np.abs(planes[2]).max() > 0.0
            assert_same_cloud(plugin, got, host, "slice enqueued on bgs_stream")
            assert_same_cloud(plugin, got, want, "slice_4d's own handle")
        finally:
            got.free()
    finally:
        plugin.synchronize()
        for h in (want, host, small):
            h.free()
        for p in ptrs:
            plugin.device_free(p)


# ---- 5. resident playback against the host route -------------------------------------------------------------------------------------------
def host_route(plugin, run, in_planes, out_shapes):
    """The parent's route: inputs into device buffers, `run(stream, in_ptrs, out_ptrs)`, synchronise, download."""
    ptrs = []
    try:
        for p in in_planes:
            ptrs.append(plugin.device_alloc(p.nbytes))
            plugin.upload_bytes(ptrs[-1], p)
        outs = [np.zeros(shape, np.float32) for shape in out_shapes]
        for o in outs:
            ptrs.append(plugin.device_alloc(o.nbytes))
        run(plugin.stream_handle(), ptrs[:len(in_planes)], ptrs[len(in_planes):])
        plugin.synchronize()
        for ptr, o in zip(ptrs[len(in_planes):], outs):
            plugin.download(ptr, o)
    finally:
        for p in ptrs:
            plugin.device_free(p)
    return outs


def test_a_resident_4d_cloud_plays(quiet):
    plugin, n = quiet, 4099
    cloud4d = random_gaussians_4d_seeded(n, 11)
    slicer = TimeSlicer(plugin.device)
    times = [("time_start", 0.25), ("interior", 0.6), ("time_stop", 1.5), ("all masked", 1000.0)]
    with plugin.resident_4d(cloud4d) as resident:
        assert len(resident) == n
        previous = None
        for name, time in times + times[:2]:                  # ... and round again: the planes are reused, the handle before is freed
            settings = CloudSettings(global_scale=0.8, time=time, time_start=0.25, time_stop=1.5)
            outs = host_route(plugin, lambda st, i, o: slicer.slice(st, n, i, o, settings), cloud4d.planes(), [(n, 4), (n, 48), (n, 8)])
            want = plugin.upload_covariance_planes(*outs)
            if previous is not None:
                previous.free()
            got, planes = resident.at(settings, return_planes=True)
            try:
                assert got.format == "cov3d" and len(got) == n
                assert all(np.array_equal(p.view(np.uint32), o.view(np.uint32)) for p, o in zip(planes, outs)), name
                assert (np.abs(outs[2]).max() == 0.0) == (name == "all masked")
                assert_same_cloud(plugin, got, want, f"4D cloud at {name}")
                again = resident.at(settings)                                 # without the planes: the same cloud
                assert_same_cloud(plugin, again, want, f"4D cloud at {name}, no planes returned")
                again.free()
            finally:
                want.free()
            previous = got
        previous.free()
    assert plugin.frames_in_flight() == 0
    resident.free()                                                            # twice is harmless
    with pytest.raises(RuntimeError, match="freed"):
        resident.at(CloudSettings())
    with plugin.resident_4d(cloud4d.slice(0, 0)) as empty:
        handle = empty.at(CloudSettings())
        assert len(empty) == 0 and len(handle) == 0 and handle.format == "cov3d"
        handle.free()


@pytest.mark.parametrize("layout", ("f32", "cov3d"))
def test_a_resident_morph_pair_plays(quiet, layout):
    plugin, n = quiet, 4099
    lhs, rhs = random_gaussians_3d_seeded(n, 12), random_gaussians_3d_seeded(n, 13)
    precompute = layout == "cov3d"
    sides = [planes_of(covariance_planes(c) if precompute else c) for c in (lhs, rhs)]
    k = len(sides[0])
    interpolator = GaussianInterpolator(plugin.device)
    times = [("time_start", 0.5), ("interior", 1.1), ("time_stop", 2.0)]
    with plugin.morph_pair(lhs, rhs, precompute_covariance_3d=precompute) as pair:
        previous = None
        for name, time in times + times[:2]:
            settings = CloudSettings(time=time, time_start=0.5, time_stop=2.0)
            outs = host_route(plugin, lambda st, i, o: interpolator.interpolate(st, n, i[:k], i[k:], o, settings),
                              sides[0] + sides[1], [p.shape for p in sides[0]])
            want = plugin.upload_covariance_planes(*outs) if precompute else plugin.upload(PlanarGaussian3d(*outs))
            if previous is not None:
                previous.free()
            got, planes = pair.at(settings, return_planes=True)
            try:
                assert got.format == layout and len(got) == n
                assert all(np.array_equal(p.view(np.uint32), o.view(np.uint32)) for p, o in zip(planes, outs)), name
                assert_same_cloud(plugin, got, want, f"{layout} morph at {name}")
            finally:
                want.free()
            previous = got
        previous.free()
    assert plugin.frames_in_flight() == 0
