"""The morph between two clouds on the device (libbgs_morph.so) against the numpy twin `interpolate_reference`
(tests/test_interpolate_host.py ties the twin to the compiled arithmetic and to float64): bit for bit on every lane that
is not NaN, NaN where the twin is NaN, with no tolerance — the square root and the divisions are correctly rounded, and
this is where that is proven. Then a morphed cloud drawn end to end against the oracle's render of the twin's cloud."""
import numpy as np
import pytest

import interpolate_cases as C
from bevy_gaussian_splatting_amd import (
    CloudSettings, GaussianInterpolator, PlanarGaussian3d, View, _native_morph, interpolate_reference)
from bevy_gaussian_splatting_amd.interpolate import covariance_planes
from test_gpu_parity import _assert_image

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)
SENTINEL_FLOATS = 16
WIDTHS = {"f32": (4, 48, 4, 4), "cov3d": (4, 48, 8)}
same_bits, same_values, same_numbers = C.same_bits, C.same_values, C.same_numbers


@pytest.fixture()
def quiet(plugin):
    plugin.set_async(False)
    plugin.set_pipeline_depth(1)
    plugin.reset_adaptive_state()
    yield plugin
    plugin.set_async(False)
    plugin.set_pipeline_depth(1)


class DevicePair:
    """Both sides of a pair and sentinel-backed output planes in device buffers of the plugin's context. `run` enqueues
    one blend, downloads the outputs (the sentinels must have come back) and returns them; `inputs` downloads the sides."""

    def __init__(self, plugin, lhs, rhs, same_side=False):
        self.plugin, self.n, self.widths = plugin, lhs[0].shape[0], tuple(p.shape[1] for p in lhs)
        self.host_in = [tuple(lhs), tuple(lhs if same_side else rhs)]
        self.ptrs = []
        try:
            self.lhs = [self._put(p) for p in lhs]
            self.rhs = self.lhs if same_side else [self._put(p) for p in rhs]
            self.out = [self._put(np.full(self.n * w + SENTINEL_FLOATS, SENTINEL, np.float32)) for w in self.widths]
        except BaseException:
            self.free()
            raise

    def _put(self, host):
        self.ptrs.append(self.plugin.device_alloc(max(host.nbytes, 16)))
        if host.nbytes:
            self.plugin.upload_bytes(self.ptrs[-1], host)
        return self.ptrs[-1]

    def run(self, settings, interpolator=None):
        (interpolator or GaussianInterpolator(self.plugin.device)).interpolate(
            self.plugin.stream_handle(), self.n, self.lhs, self.rhs, self.out, settings)
        self.plugin.synchronize()
        got = [self.plugin.download(p, np.empty(self.n * w + SENTINEL_FLOATS, np.float32)) for p, w in zip(self.out, self.widths)]
        for g, w in zip(got, self.widths):
            assert (g[self.n * w:] == SENTINEL).all(), "the sentinel behind an output plane was overwritten"
        return [g[:self.n * w].reshape(self.n, w) for g, w in zip(got, self.widths)]

    def inputs_untouched(self):
        for ptrs, hosts in zip((self.lhs, self.rhs), self.host_in):
            for p, h in zip(ptrs, hosts):
                if h.nbytes and not same_bits(self.plugin.download(p, np.empty_like(h)), np.ascontiguousarray(h)):
                    return False
        return True

    def free(self):
        ptrs, self.ptrs = self.ptrs, []
        for p in ptrs:
            self.plugin.device_free(p)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


# ---- 1. device against twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.SIZES)
@pytest.mark.parametrize("layout", C.LAYOUTS)
@pytest.mark.parametrize("case", C.CASES)
def test_interpolation_equals_the_twin(quiet, case, layout, n):
    lhs, rhs = (C.prefix(side, n) for side in C.sides(case, layout))
    with DevicePair(quiet, lhs, rhs) as pair:
        for name in C.GPU_SETTINGS[case]:
            got = pair.run(C.settings(name))
            want = C.reference(case, layout, name)
            for k, (g, w) in enumerate(zip(got, want)):
                assert same_values(g, np.ascontiguousarray(w[:n])), f"{case} {layout} n={n} {name}: plane {k} differs from the twin"
        assert pair.inputs_untouched()
    if case == "antipodal" and layout == "f32" and n:
        assert same_bits(np.ascontiguousarray(C.reference(case, layout, "half")[2][:n]), np.tile(np.float32([0, 0, 0, 1]), (n, 1)))


# ---- 2. a side given twice, and the end points --------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", C.LAYOUTS)
def test_a_side_given_twice_and_the_end_points(quiet, layout):
    n = 5000
    lhs = C.sides("random", layout)[0]
    with DevicePair(quiet, lhs, lhs, same_side=True) as pair:
        assert pair.lhs == pair.rhs                                      # by address
        for name in ("zero", "one"):
            got = pair.run(C.settings(name))
            mixed = [0, 1, 3] if layout == "f32" else [0, 1]
            for k in mixed:
                assert same_numbers(got[k], lhs[k]), (name, k)
            if layout == "cov3d":
                assert same_numbers(got[2][:, :7], lhs[2][:, :7]) and (got[2][:, 7].view(np.uint32) == 0).all()
        got = pair.run(C.settings("inside"))
        want = interpolate_reference(lhs, lhs, C.settings("inside"))
        assert all(same_values(g, w) for g, w in zip(got, want))
        assert pair.inputs_untouched()
    assert n == lhs[0].shape[0]


# ---- 3. end to end against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", C.LAYOUTS)
def test_a_morphed_cloud_draws_what_the_oracle_draws(quiet, oracle, layout):
    """A 2000-splat random pair at t = 0.5, 320 x 180: interpolate, sort, render, against the oracle's sort and render of
    the cloud built from the twin's planes. The returned planes equal the twin's to the bit first, so that the oracle and
    the device see the same cloud. The oracle has no precomputed-covariance cloud of its own: there the two sides are
    given equal rotations and scales, whose covariance planes are then the same bits and blend to themselves exactly
    (c * 0.5 + c * 0.5 = c), so the morphed cloud IS the f32 cloud with that rotation and scale and the blended rest."""
    plugin, n = quiet, 2000
    lhs, rhs = (c.slice(0, n) for c in C.clouds("random"))
    precompute = layout == "cov3d"
    if precompute:
        rhs = PlanarGaussian3d(rhs.position_visibility, rhs.spherical_harmonic, lhs.rotation,
                               np.concatenate([lhs.scale_opacity[:, :3], rhs.scale_opacity[:, 3:]], axis=1))
    view, draw = View.headless(320, 180), CloudSettings()
    settings = C.settings("half")
    if precompute:
        twin = interpolate_reference(covariance_planes(lhs), covariance_planes(rhs), settings)
        f32_twin = interpolate_reference(lhs, rhs, settings)
        assert same_bits(twin[2][:, :6], covariance_planes(lhs)[2][:, :6]) and same_bits(twin[2][:, 6], f32_twin[3][:, 3])
        equivalent = PlanarGaussian3d(twin[0], twin[1], lhs.rotation, np.concatenate([lhs.scale_opacity[:, :3], twin[2][:, 6:7]], axis=1))
        assert same_bits(covariance_planes(equivalent)[2], twin[2])
    else:
        twin = interpolate_reference(lhs, rhs, settings)
        equivalent = PlanarGaussian3d(*twin)
    handle, planes = plugin.interpolate(lhs, rhs, settings, precompute_covariance_3d=precompute, return_planes=True)
    try:
        assert handle.format == ("cov3d" if precompute else "f32") and len(handle) == n and len(planes) == len(twin)
        assert all(same_bits(p, np.ascontiguousarray(w)) for p, w in zip(planes, twin))
        entries = plugin.sort(handle, view, draw)
        image = plugin.render(handle, view, draw)
    finally:
        handle.free()
    ref_entries = oracle.sort(equivalent, view, draw)
    assert np.array_equal(entries["key"], ref_entries["key"]) and np.array_equal(entries["index"], ref_entries["index"])
    ref, amb = oracle.render(equivalent, ref_entries, view, draw, with_ambiguity=True)
    _assert_image(ref, image, amb, frac_slack=0.01, what=f"morphed cloud, {layout} layout, t = 0.5")
    assert np.abs(ref[..., :3]).max() > 0.05


# ---- 4. a resident pair -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", C.LAYOUTS)
def test_a_resident_pair_is_reused(quiet, layout):
    plugin, n = quiet, 2000
    lhs, rhs = (c.slice(0, n) for c in C.clouds("random"))
    precompute = layout == "cov3d"
    pair = plugin.morph_pair(lhs, rhs, precompute_covariance_3d=precompute)
    try:
        for name in ("inside", "reversed", "after"):
            handle, planes = pair.at(C.settings(name), return_planes=True)
            fresh_handle, fresh = plugin.interpolate(lhs, rhs, C.settings(name), precompute_covariance_3d=precompute, return_planes=True)
            try:
                assert len(handle) == len(fresh_handle) == n and handle.format == fresh_handle.format
                assert all(same_bits(p, f) for p, f in zip(planes, fresh))
                want = C.reference("random", layout, name)
                if not precompute:                        # (C.sides puts junk into the covariance layout's pad lane: other inputs)
                    assert all(same_bits(p, np.ascontiguousarray(w[:n])) for p, w in zip(planes, want))
            finally:
                handle.free()
                fresh_handle.free()
    finally:
        pair.free()
    assert plugin.frames_in_flight() == 0
    pair.free()                                                            # twice is harmless
    with plugin.morph_pair(lhs, rhs, precompute_covariance_3d=precompute) as again:
        assert len(again) == n
    with pytest.raises(ValueError, match="equal length"):
        plugin.interpolate(lhs, rhs.slice(0, n - 1), CloudSettings())


# ---- 5. errors on a live device ---------------------------------------------------------------------------------------------------
def test_errors_name_the_argument(quiet):
    n = 257
    lhs, rhs = (C.prefix(side, n) for side in C.sides("random", "f32"))
    interpolator = GaussianInterpolator(quiet.device)
    stream, ok = quiet.stream_handle(), C.settings("inside")
    with DevicePair(quiet, lhs, rhs) as pair:
        with pytest.raises(_native_morph.BgsMorphError, match="rhs_rotation_device_ptr must be a 16-byte aligned") as ei:
            interpolator.interpolate(stream, n, pair.lhs, pair.rhs[:2] + [pair.rhs[2] + 4] + pair.rhs[3:], pair.out, ok)
        assert ei.value.status == _native_morph.BGSM_EINVAL
        with pytest.raises(_native_morph.BgsMorphError, match="out_spherical_harmonic_device_ptr is lhs_spherical_harmonic_device_ptr as well"):
            interpolator.interpolate(stream, n, pair.lhs, pair.rhs, [pair.out[0], pair.lhs[1]] + pair.out[2:], ok)
        with pytest.raises(_native_morph.BgsMorphError, match="time_stop inf must be finite"):
            interpolator.interpolate(stream, n, pair.lhs, pair.rhs, pair.out, CloudSettings(time_stop=float("inf")))
        with pytest.raises(_native_morph.BgsMorphError, match="lhs_covariance_3d_opacity_device_ptr is NULL"):
            interpolator.interpolate(stream, n, pair.lhs[:2] + [0], pair.rhs[:3], pair.out[:3], ok)
        quiet.synchronize()
        # nothing was enqueued: the outputs still hold what was put there
        for p, w in zip(pair.out, pair.widths):
            assert (quiet.download(p, np.empty(n * w + SENTINEL_FLOATS, np.float32)) == SENTINEL).all()
        interpolator.interpolate(stream, 0, [0] * 4, [0] * 4, [0] * 4, ok)      # n == 0: nothing is enqueued, nothing is looked at
        with pytest.raises(_native_morph.BgsMorphError, match="no usable HIP device 99"):
            GaussianInterpolator(99).interpolate(stream, n, pair.lhs, pair.rhs, pair.out, ok)
        got = pair.run(ok, interpolator)                                        # a following valid call still equals the twin
        want = C.reference("random", "f32", "inside")
        assert all(same_values(g, np.ascontiguousarray(w[:n])) for g, w in zip(got, want))
