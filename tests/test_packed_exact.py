"""The packed outputs (Rgba8UnormSrgb, Rgba16Float) against their exact conversion (tests/packed_exact.py): the
product's conversion kernel on every binary32 input in every channel (bgs_selftest_pack), and every path that writes
packed bytes against the exact conversion of the f32 frame of the same call. No tolerance anywhere."""
import numpy as np
import pytest

import helpers as H
import packed_exact as P
from bevy_gaussian_splatting_amd import (
    CloudSettings, GaussianMode, PlanarGaussian3d, RasterizeMode, View, _native, random_gaussians_3d_seeded)
from bevy_gaussian_splatting_amd.multiview import device_ptr_as_tensor, headless_view

pytestmark = pytest.mark.gpu

SEPARATE_ENCODE, MIDROUND_ALWAYS, NO_MIDROUND = 0x40000, 0x20000, 0x1000000
STRIPS_ANY_DEPTH, RERUN_EVERY_FRAME = 0x4000000, 0x8000000


def test_selftest_pack_rejects_bad_arguments(plugin):
    import torch
    src = torch.zeros(64 * 4 + 4, dtype=torch.float32, device="cuda:0")
    dst = torch.zeros(64 * 8 + 8, dtype=torch.uint8, device="cuda:0")
    for fmt in (0, 3, 0xFFFFFFFF):
        with pytest.raises(_native.BgsError, match="format") as e:
            plugin.selftest_pack(fmt, src.data_ptr(), 64, dst.data_ptr())
        assert e.value.status == _native.BGS_EINVAL
    for args in ((0, 64, dst.data_ptr()), (src.data_ptr(), 64, 0), (src.data_ptr(), 0, dst.data_ptr())):
        with pytest.raises(_native.BgsError, match="pixels >= 1 and both device buffers") as e:
            plugin.selftest_pack("srgb8", *args)
        assert e.value.status == _native.BGS_EINVAL
    with pytest.raises(_native.BgsError, match="aligned"):
        plugin.selftest_pack("srgb8", src.data_ptr() + 4, 64, dst.data_ptr())
    with pytest.raises(_native.BgsError, match="aligned"):
        plugin.selftest_pack("rgba16f", src.data_ptr(), 64, dst.data_ptr() + 4)
    # the context still works after the refusals
    plugin.selftest_pack("rgba16f", src.data_ptr(), 64, dst.data_ptr())
    assert int(dst[: 64 * 8].sum()) == 0


@pytest.mark.parametrize("fmt", ["srgb8", "rgba16f"])
def test_packed_conversion_every_f32_input_every_channel(plugin, fmt):
    """All 2^32 binary32 bit patterns in each of the four channels (2^34 conversions) through the product's
    encode_srgb8_kernel, compared on the device with the exact references: sRGB8 colour = the number of colour
    thresholds reached (0 for NaN, -0 and negatives, 255 from 1 on and for +inf), alpha the same with the alpha
    thresholds, Rgba16Float = binary32 -> binary16 round to nearest even (a NaN to some NaN)."""
    bad, report, checked = P.exhaustive_pack(plugin, fmt)
    assert checked == 1 << 34
    assert sum(bad) == 0, P.format_report(fmt, bad, report)


# ---------------------------------------------------------------------------------------------------------------------
# every path that writes packed bytes
# ---------------------------------------------------------------------------------------------------------------------
class _Checker:
    def __init__(self, oracle):
        self.oracle = oracle
        self.codes = [set() for _ in range(4)]
        self.frames = {"srgb8": 0, "rgba16f": 0}

    def check(self, f32, packed, fmt, what):
        """packed bytes (uint8 [h, w, 4] or uint16 [h, w, 4]) == the exact conversion of the f32 frame"""
        f32 = np.ascontiguousarray(f32, np.float32)
        if fmt == "srgb8":
            want = self.oracle.srgb8_codes(f32)
            bad = packed != want
            for c in range(4):
                self.codes[c].update(np.unique(packed[..., c]).tolist())
        else:
            import torch
            want = P.f16_bits(torch.from_numpy(f32.view(np.int32))).numpy()
            got = torch.from_numpy(packed.view(np.int16).astype(np.int32) & 0xFFFF)
            bad = P.f16_mismatch(got, torch.from_numpy(want)).numpy()
        self.frames[fmt] += 1
        if bad.any():
            where = np.argwhere(bad)[:20]
            lines = [f"{what} ({fmt}): {int(bad.sum())} packed values differ from the exact conversion"]
            for y, x, c in where:
                lines.append(f"  ({y}, {x}, {c}) f32 {f32[y, x, c]!r} (0x{f32.view(np.uint32)[y, x, c]:08x}): "
                             f"got {int(packed[y, x, c]) & 0xFFFF:#x}, want {int(want[y, x, c]) & 0xFFFF:#x}")
            raise AssertionError("\n".join(lines))


def _packed_ptr(plugin, fmt):
    return (plugin.framebuffer_srgb8_device_ptr() if fmt == "srgb8" else plugin.framebuffer_rgba16f_device_ptr())[0]


def _download(ptr, h, w, fmt):
    return device_ptr_as_tensor(ptr, (h, w, 4), "|u1" if fmt == "srgb8" else "<u2", "cuda:0").cpu().numpy()


def _set_format(plugin, fmt):
    if fmt == "srgb8":
        plugin.set_output_srgb8(True)
    else:
        plugin.set_output_rgba16f(True)


def _off(plugin):
    plugin.set_debug_flags(0)
    plugin.set_packed_only(False)
    plugin.set_async(False)
    plugin.set_graphs(False)
    plugin.set_profiling(2)
    plugin.set_pipeline_depth(1)
    plugin.set_output_srgb8(False)
    plugin.set_output_rgba16f(False)
    plugin.set_binning("scan")


def _blocking(plugin, chk, h, v, s, fmt, what):
    """One blocking frame with the packed output on: its f32 frame and packed bytes, checked."""
    _set_format(plugin, fmt)
    f32 = plugin.render(h, v, s)
    packed = _download(_packed_ptr(plugin, fmt), v.height, v.width, fmt)
    chk.check(f32, packed, fmt, what)
    return f32, packed


@pytest.mark.parametrize("fmt", ["srgb8", "rgba16f"])
def test_packed_bytes_are_the_exact_conversion_on_every_path(plugin, oracle, fmt):
    import torch
    chk = _Checker(oracle)
    c = random_gaussians_3d_seeded(2_000, 33)   # sparse: fractional coverage, the clear colour shows between splats
    c.spherical_harmonic *= 4.0   # channels past 1 (and, over the clear colour's blue, below 0)
    v = View.headless(320, 180)
    v.clear_color = (0.25, 0.0015, -0.3, 0.37)   # fractional alpha, a colour in the linear segment of the OETF, one below 0
    s = CloudSettings()
    h = plugin.upload(c)
    try:
        # binning scan / sort, the separate encode pass, mid-round exits forced on and off, forced re-runs
        for binning, flags, what in (("scan", 0, "scan"), ("sort", 0, "sort"), ("scan", SEPARATE_ENCODE, "separate encode"),
                                     ("sort", SEPARATE_ENCODE, "sort, separate encode"),
                                     ("scan", MIDROUND_ALWAYS, "mid-round always"), ("scan", NO_MIDROUND, "no mid-round"),
                                     ("scan", RERUN_EVERY_FRAME, "re-run every frame")):
            plugin.set_binning(binning)
            plugin.set_debug_flags(flags)
            f32, packed = _blocking(plugin, chk, h, v, s, fmt, what)
            if what == "scan":
                ref_f32, ref_packed = f32, packed
            _off(plugin)
        assert (ref_f32 > 1).any() and (ref_f32 < 0).any() and ((ref_f32 > 0) & (ref_f32 < 1)).any()
        # sample counts, a depth buffer, the bounding-box overlay, 2DGS surfels
        for samples in (1, 2, 4, 8):
            vs = View.headless(320, 180, msaa_samples=samples)
            vs.clear_color = v.clear_color
            _blocking(plugin, chk, h, vs, s, fmt, f"{samples} samples")
            _off(plugin)
        vd = View.headless(320, 180, msaa_samples=4)
        vd.clear_color = v.clear_color
        dptr = plugin.upload_depth(H.random_depth_buffer(c, vd, s, np.random.default_rng(5)))
        try:
            vd.depth_device_ptr = dptr
            _blocking(plugin, chk, h, vd, s, fmt, "depth buffer")
        finally:
            vd.depth_device_ptr = 0
            plugin.device_free(dptr)
        _off(plugin)
        _blocking(plugin, chk, h, v, CloudSettings(visualize_bounding_box=True), fmt, "bounding-box overlay")
        _off(plugin)
        _blocking(plugin, chk, h, v, CloudSettings(gaussian_mode=GaussianMode.Gaussian2d, global_scale=0.5), fmt, "2DGS")
        _off(plugin)
        # packed-only: the same bytes as the frame that kept its f32 target
        plugin.set_binning("scan")
        _set_format(plugin, fmt)
        plugin.set_packed_only(True)
        plugin.render(h, v, s, download=False)
        only = _download(_packed_ptr(plugin, fmt), 180, 320, fmt)
        assert np.array_equal(only, ref_packed), "packed-only frame"
        _off(plugin)
        # the caller's target (bgs_set_srgb8_target; Rgba16Float frames write theirs there as well)
        tgt = torch.full((180 * 320 * (4 if fmt == "srgb8" else 8),), 0xA5, dtype=torch.uint8, device="cuda:0")
        _set_format(plugin, fmt)
        plugin.set_srgb8_target(tgt.data_ptr())
        f32 = plugin.render(h, v, s)
        chk.check(f32, _download(tgt.data_ptr(), 180, 320, fmt), fmt, "caller's target")
        _off(plugin)
        # pipeline depth 3 with graphs: every popped frame's packed bytes against its own f32 frame
        _set_format(plugin, fmt)
        plugin.set_async(True)
        plugin.set_pipeline_depth(3)
        plugin.set_profiling(0)   # (frames that record HIP events are not captured)
        plugin.set_graphs(True)
        views = [headless_view(g % 8, 320, 180) for g in range(48)]   # enough frames for the graph replays to start
        for vk in views:
            vk.clear_color = v.clear_color
        popped = []

        def pop():
            p32, pk = plugin.pipeline_pop()
            popped.append((device_ptr_as_tensor(p32, (180, 320, 4), "<f4", "cuda:0").cpu().numpy(), _download(pk, 180, 320, fmt)))
        for vk in views:
            plugin.render(h, vk, s, download=False)
            if plugin.frames_in_flight() >= 3:
                pop()
        while plugin.frames_in_flight():
            pop()
        assert len(popped) == len(views) and plugin.graph_counters()[1] > 0
        for k, (f32, packed) in enumerate(popped):
            chk.check(f32, packed, fmt, f"pipelined frame {k}")
        _off(plugin)
    finally:
        _off(plugin)
        h.free()
    # the Depth-mode frame of test_rasterize_mode_edge_cases (one splat; its colour is finite, in the oracle as here:
    # NaN inputs are covered by the exhaustive test above)
    one = PlanarGaussian3d(np.array([[0.3, 1.2, 0, 1]], np.float32), np.zeros((1, 48), np.float32),
                           np.array([[1, 0, 0, 0]], np.float32), np.array([[0.5, 0.5, 0.5, 0.9]], np.float32))
    h1 = plugin.upload(one)
    try:
        sd = CloudSettings(rasterize_mode=RasterizeMode.Depth, position_min=(-1, -1, -1), position_max=(1, 2, 1))
        _blocking(plugin, chk, h1, View.headless(64, 64), sd, fmt, "Depth-mode frame")
    finally:
        _off(plugin)
        h1.free()
    if fmt == "srgb8":
        assert all(len(k) >= 128 for k in chk.codes), [len(k) for k in chk.codes]


@pytest.mark.parametrize("fmt", ["srgb8", "rgba16f"])
def test_packed_bytes_exact_on_heavy_tile_strip_waves(plugin, oracle, fmt):
    """A dense frame (1 M splats at 1080p) whose heavy tiles are drawn by strip waves (forced at any pipeline depth,
    debug flag 0x4000000): the packed bytes of the frame that used them equal the exact conversion of its f32 frame."""
    chk = _Checker(oracle)
    c = random_gaussians_3d_seeded(1_000_000, 2)
    v = View.headless(1920, 1080)
    v.clear_color = (0.1, 0.2, 0.3, 0.45)
    s = CloudSettings()
    h = plugin.upload(c)
    plugin.reset_adaptive_state()
    try:
        plugin.set_debug_flags(STRIPS_ANY_DEPTH)
        strips = []
        for k in range(8):
            f32, packed = _blocking(plugin, chk, h, v, s, fmt, f"dense frame {k}")
            strips.append(plugin.stats()["strip_tiles"])
        assert strips[-1] > 0, strips
    finally:
        _off(plugin)
        plugin.reset_adaptive_state()
        h.free()
