"""The cloud's own bounds on the device (BGS_BOUNDS_CLOUD, bgs_settings.reserved[0]). Every comparison is bitwise: the box
is a contract numpy reproduces exactly (`bounds_reference`, pinned to the compiled arithmetic in test_cloud_bounds_host.py),
and the box has no read-back in the C ABI, so it is pinned through what it does: a Position-mode frame drawn with the flag
set and deliberately WRONG caller bounds is the frame drawn with the flag clear and the twin's bounds. Frames are 64 x 64."""
import ctypes

import numpy as np
import pytest

from bevy_gaussian_splatting_amd import (
    CloudSettings, GaussianSplattingPlugin, PlanarGaussian3d, RasterizeMode, View, _native, bounds_reference,
    interpolate_reference, random_gaussians_3d_seeded, random_gaussians_4d_seeded, random_particle_behaviors,
    slice_reference, step_reference)
from bevy_gaussian_splatting_amd.bounds import bounds_grid, bounds_single_sweep_reach

pytestmark = pytest.mark.gpu

W = H = 64
WRONG_MIN, WRONG_MAX = (5.0, -7.0, 2.5), (5.5, 40.0, 2.75)      # what a flagged frame must not read
SMALL = (1, 63, 64, 65, 257, 5000)
FORMATS = ("f32", "f16", "cov3d")
_clouds = {}


def compute_units() -> int:
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def beyond_one_sweep() -> int:
    """A splat count the reduction's largest grid (two workgroups a compute unit) does not reach in one sweep of its lanes:
    257 more, so that the second sweep has a full workgroup, a lone lane, and workgroups with nothing left."""
    n = bounds_single_sweep_reach(compute_units()) + 257
    assert bounds_grid(n, compute_units()) * 256 < n
    return n


def cloud_of(n, seed=0):
    """One random cloud a size (and seed), made once and never modified."""
    if (n, seed) not in _clouds:
        c = random_gaussians_3d_seeded(n, 60 + seed + n % 11)
        c.position_visibility.setflags(write=False)
        _clouds[(n, seed)] = c
    return _clouds[(n, seed)]


def with_positions(cloud, pv):
    return PlanarGaussian3d(np.ascontiguousarray(pv, np.float32), cloud.spherical_harmonic, cloud.rotation, cloud.scale_opacity)


def upload(plugin, cloud, fmt):
    if fmt == "f16":
        return plugin.upload(cloud.to_f16())
    return plugin.upload(cloud, precompute_covariance_3d=(fmt == "cov3d"))


def flagged(mode=RasterizeMode.Position, **kw):
    return CloudSettings(rasterize_mode=mode, bounds_from_cloud=True, position_min=WRONG_MIN, position_max=WRONG_MAX, **kw)


def with_twin_bounds(pv, mode=RasterizeMode.Position, **kw):
    lo, hi = bounds_reference(pv)
    return CloudSettings(rasterize_mode=mode, position_min=tuple(lo.tolist()), position_max=tuple(hi.tolist()), **kw)


def same_frame(a, b):
    """NaN masks first (as test_rasterize_mode_edge_cases compares them), then every bit."""
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture()
def quiet(plugin):
    plugin.set_async(False)
    plugin.set_pipeline_depth(1)
    plugin.set_binning("scan")
    plugin.set_grid_cap(0)
    plugin.reset_adaptive_state()
    yield plugin
    plugin.synchronize()
    plugin.set_graphs(False)
    plugin.set_async(False)
    plugin.set_pipeline_depth(1)
    plugin.set_binning("scan")
    plugin.set_grid_cap(0)
    plugin.set_profiling(2)


def assert_flag_is_the_twin(plugin, handle, pv, what, samples=(1, 4)):
    """The flagged frame with wrong caller bounds == the unflagged frame with the twin's bounds; and the wrong bounds,
    unflagged, are a different frame wherever anything is drawn (so the comparison sees the bounds)."""
    frames = []
    for s in samples:
        view = View.headless(W, H, msaa_samples=s)
        got = plugin.render(handle, view, flagged())
        want = plugin.render(handle, view, with_twin_bounds(pv))
        assert same_frame(got, want), f"{what}, {s} samples: the flagged frame is not the frame with the twin's bounds"
        frames.append(got)
    return frames


# ---- 1. bitwise frames -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binning", ["scan", "sort"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_flagged_position_frame_is_the_frame_with_the_twins_bounds(quiet, fmt, binning):
    """Fails on a library that ignores the word: the frame is then drawn with WRONG_MIN / WRONG_MAX."""
    plugin = quiet
    plugin.set_binning(binning)
    drew_something = False
    for n in SMALL + (beyond_one_sweep(),):
        cloud = cloud_of(n)
        h = upload(plugin, cloud, fmt)
        try:
            frames = assert_flag_is_the_twin(plugin, h, cloud.position_visibility, f"{fmt} {binning} n={n}")
            if n == 5000:
                wrong = plugin.render(h, View.headless(W, H, msaa_samples=1),
                                      CloudSettings(rasterize_mode=RasterizeMode.Position, position_min=WRONG_MIN, position_max=WRONG_MAX))
                drew_something = np.abs(np.nan_to_num(frames[0][..., :3])).max() > 0.0 and not same_frame(wrong, frames[0])
        finally:
            h.free()
    assert drew_something, "the 5000-splat frame does not show the bounds: the comparison above proves nothing"


@pytest.mark.parametrize("cap,n", [(1, 257), (1, 5000), (2, 5000), (3, 4099)])
def test_lanes_that_come_back_for_more_under_a_grid_cap(quiet, cap, n):
    """bgs_set_grid_cap caps the reduction's grid like every persistent launch: with 1 .. 3 workgroups a 5000-splat cloud
    takes the lanes through the unrolled sweeps (eight splats a lane and round) and then the single ones."""
    plugin = quiet
    cloud = cloud_of(n, seed=1)
    assert bounds_grid(n, compute_units(), cap) == cap and cap * 256 < n
    plugin.set_grid_cap(cap)
    h = upload(plugin, cloud, "f32")
    try:
        assert_flag_is_the_twin(plugin, h, cloud.position_visibility, f"cap {cap} n={n}")
    finally:
        plugin.set_grid_cap(0)
        h.free()


# ---- 2. non-finite input ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nan_lanes", "nan_and_inf", "all_nan_axis"])
def test_non_finite_positions_give_the_twins_bounds(quiet, kind):
    plugin, n = quiet, 1500
    pv = cloud_of(n, seed=2).position_visibility.copy()
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    pv[3::7, 0] = nan
    pv[5::11, 1] = np.array(0xFFC00123, np.uint32).view(np.float32)
    pv[np.argmin(pv[:, 2]), 2] = nan          # the splat that held the z minimum no longer counts
    pv[1::13, 3] = nan                        # (the visibility lane is not read)
    if kind == "nan_and_inf":
        pv[10, 0], pv[20, 1], pv[30, 2], pv[40, 2] = inf, -inf, inf, -inf
    if kind == "all_nan_axis":
        pv[:, 1] = nan
    lo, hi = bounds_reference(pv)
    assert np.isfinite(lo).all() == (kind == "nan_lanes")
    cloud = with_positions(cloud_of(n, seed=2), pv)
    for fmt in ("f32", "f16"):
        h = upload(plugin, cloud, fmt)
        try:
            assert_flag_is_the_twin(plugin, h, pv, f"{kind} {fmt}")
        finally:
            h.free()


# ---- 3. particle step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_particle_step_invalidates_the_box(quiet, fmt):
    """After a step the flagged frame of the stepped cloud is a fresh upload of the twin-stepped positions drawn with THAT
    cloud's twin bounds; a second step is followed again. The box was valid before each step (a flagged frame had asked)."""
    plugin, n, dt = quiet, 5000, 0.25
    cloud = cloud_of(n, seed=3)
    rec0 = random_particle_behaviors(n, 9).records
    rec0["velocity"] *= np.float32(8.0)       # the cloud's extremes move well past a rounding error of the box
    pv1, rec1 = step_reference(cloud.position_visibility, rec0, dt)
    pv2, _ = step_reference(pv1, rec1, dt)
    boxes = [np.concatenate(bounds_reference(p)) for p in (cloud.position_visibility, pv1, pv2)]
    assert not np.array_equal(boxes[0], boxes[1]) and not np.array_equal(boxes[1], boxes[2])
    view = View.headless(W, H)
    a = upload(plugin, cloud, fmt)
    b = plugin.upload_particle_behaviors(rec0)
    fresh = []
    try:
        before = assert_flag_is_the_twin(plugin, a, cloud.position_visibility, "before the step", samples=(4,))[0]
        for step, pv in enumerate((pv1, pv2)):
            plugin.apply_particle_behaviors(a, b, dt)
            fresh.append(upload(plugin, with_positions(cloud, pv), fmt))
            got = plugin.render(a, view, flagged())
            want = plugin.render(fresh[-1], view, with_twin_bounds(pv))
            assert same_frame(got, want), f"step {step + 1}"
            assert same_frame(plugin.render(a, view, flagged()), want), f"step {step + 1}, the cached box"
            assert not same_frame(got, before)
    finally:
        b.free()
        a.free()
        for h in fresh:
            h.free()


# ---- 4. device-born clouds -------------------------------------------------------------------------------------------
def test_a_morphed_cloud_draws_position_mode_without_host_positions(quiet):
    plugin, n = quiet, 3001
    lhs, rhs = cloud_of(n, seed=4), cloud_of(n, seed=5)
    morph = CloudSettings(time=0.375)
    twin_pv = interpolate_reference(lhs, rhs, morph)[0]
    h = plugin.interpolate(lhs, rhs, morph)
    try:
        assert_flag_is_the_twin(plugin, h, twin_pv, "plugin.interpolate")
    finally:
        h.free()


def test_a_time_slice_draws_position_mode_without_host_positions(quiet):
    plugin, n = quiet, 3001
    cloud4d = random_gaussians_4d_seeded(n, 17)
    at = CloudSettings(time=0.4)
    twin_pv = slice_reference(cloud4d, at).position_visibility
    h, planes = plugin.slice_4d(cloud4d, at, return_planes=True)
    try:
        # (diagnosis only: the slice's positions are the twin's bits except for splats within a rounding error of its
        # mask; were one of those an extreme of the cloud, the two boxes below would differ and this line says so)
        assert all(np.array_equal(a, b) for a, b in zip(bounds_reference(planes[0]), bounds_reference(twin_pv)))
        assert_flag_is_the_twin(plugin, h, twin_pv, "plugin.slice_4d")
    finally:
        h.free()


# ---- 5. lanes and graphs ---------------------------------------------------------------------------------------------
def _alternating(plugin, handle, pv, flag_odd, frames=16):
    """`frames` asynchronous Position frames on one cloud, every second one with other caller bounds; with flag_odd the
    odd frames say BGS_BOUNDS_CLOUD with wrong caller bounds instead of carrying the twin's. Pops every frame."""
    view = View.headless(W, H)
    other = CloudSettings(rasterize_mode=RasterizeMode.Position, position_min=(-30.0, -30.0, -30.0), position_max=(30.0, 31.0, 32.0))
    odd = flagged() if flag_odd else with_twin_bounds(pv)
    out = []
    for k in range(frames):
        plugin.render(handle, view, odd if k % 2 else other, download=False)
        if plugin.frames_in_flight() == 4 or k == frames - 1:
            while plugin.frames_in_flight():
                f32, _ = plugin.pipeline_pop()
                out.append(plugin.download(f32, np.empty((H, W, 4), np.float32)))
    assert len(out) == frames
    return out, view, other


@pytest.mark.parametrize("graphs", [False, True], ids=["lanes", "graphs"])
def test_flagged_and_unflagged_frames_alternate_on_four_lanes(graphs):
    """Contexts of their own, so that both sequences start from the same (fresh) state: every popped frame is the bits of
    its blocking twin, and with bgs_set_graphs(1) the flagged sequence takes no capture the unflagged one does not."""
    n = 5000
    cloud = cloud_of(n, seed=6)
    pv = cloud.position_visibility
    counters = []
    for flag_odd in (False, True):
        with GaussianSplattingPlugin(0) as plugin:
            h = plugin.upload(cloud)
            try:
                view = View.headless(W, H)
                want_odd = plugin.render(h, view, with_twin_bounds(pv))
                plugin.set_profiling(0)      # (timed frames are launched directly)
                plugin.set_pipeline_depth(4)
                plugin.set_async(True)
                plugin.set_graphs(graphs)
                c0, r0 = plugin.graph_counters()
                got, view, other = _alternating(plugin, h, pv, flag_odd)
                c1, r1 = plugin.graph_counters()
                counters.append((c1 - c0, r1 - r0))
                plugin.set_graphs(False)
                plugin.set_async(False)
                plugin.set_pipeline_depth(1)
                want_even = plugin.render(h, view, other)
                assert not same_frame(want_even, want_odd)
                for k, frame in enumerate(got):
                    assert same_frame(frame, want_odd if k % 2 else want_even), f"frame {k}, flag_odd={flag_odd}"
            finally:
                h.free()
    (clear_captures, clear_replays), (flag_captures, flag_replays) = counters
    assert flag_captures <= clear_captures, counters
    if graphs:
        assert flag_replays > 0 and flag_replays >= clear_replays, counters
    else:
        assert flag_captures == 0 and flag_replays == 0


# ---- 6. other modes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [RasterizeMode.Color, RasterizeMode.Depth, RasterizeMode.Normal, RasterizeMode.Classification])
def test_other_modes_do_not_see_the_flag(quiet, mode):
    plugin = quiet
    cloud = cloud_of(5000)
    h = plugin.upload(cloud)
    try:
        for samples in (1, 4):
            view = View.headless(W, H, msaa_samples=samples)
            clear = plugin.render(h, view, CloudSettings(rasterize_mode=mode, num_classes=3))
            flag = plugin.render(h, view, flagged(mode, num_classes=3))
            assert same_frame(clear, flag), (mode, samples)
        e_clear = plugin.sort(h, view, CloudSettings())
        e_flag = plugin.sort(h, view, CloudSettings(bounds_from_cloud=True))
        assert e_clear.tobytes() == e_flag.tobytes()
    finally:
        h.free()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------
def test_a_value_above_one_is_refused_with_the_field_named(quiet):
    plugin = quiet
    lib, ctx = plugin._lib, plugin._ctx
    h = plugin.upload(cloud_of(257))
    try:
        v = View.headless(W, H).to_native()
        for bad in (2, 3, 0xFFFFFFFF):
            s = CloudSettings(rasterize_mode=RasterizeMode.Position).to_native()
            s.reserved[0] = bad
            assert lib.bgs_render(ctx, h._ptr, ctypes.byref(v), ctypes.byref(s), None) == _native.BGS_EINVAL
            assert b"bgs_settings.reserved[0]" in lib.bgs_last_error(ctx)
            assert lib.bgs_sort(ctx, h._ptr, ctypes.byref(v), ctypes.byref(s), None) == _native.BGS_EINVAL
            assert b"bgs_settings.reserved[0]" in lib.bgs_last_error(ctx)
        s.reserved[0] = 1
        assert lib.bgs_render(ctx, h._ptr, ctypes.byref(v), ctypes.byref(s), None) == _native.BGS_OK
        assert lib.bgs_sort(ctx, h._ptr, ctypes.byref(v), ctypes.byref(s), None) == _native.BGS_OK
    finally:
        h.free()


def test_an_empty_cloud_keeps_the_callers_values_and_launches_nothing(quiet):
    plugin = quiet
    h = plugin.upload(random_gaussians_3d_seeded(0, 1))
    try:
        view = View.headless(W, H)
        clear = plugin.render(h, view, CloudSettings(rasterize_mode=RasterizeMode.Position, position_min=WRONG_MIN, position_max=WRONG_MAX))
        assert same_frame(plugin.render(h, view, flagged()), clear)
        assert plugin.sort(h, view, CloudSettings(bounds_from_cloud=True)).shape == (0,)
    finally:
        h.free()
