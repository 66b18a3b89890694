"""The time slice of a 4D cloud on the device (libbgs_slice.so) against the numpy twin `slice_reference`
(tests/test_time_slice_host.py ties the twin to the compiled arithmetic and to float64): bit for bit on every lane that
does not pass through the device's exp / cos, within the math library's documented error on those that do
(tests/time_slice_cases.py has the bounds and where they come from). Then a slice drawn end to end against the oracle's
render of the equivalent 3D cloud."""
import numpy as np
import pytest

import time_slice_cases as C
from bevy_gaussian_splatting_amd import (
    CloudSettings, PlanarGaussian3d, TimeSlicer, View, _native_slice, compute_covariance_3d, slice_float64, slice_reference)
from test_gpu_parity import _assert_image
from test_time_slice_host import _six, spatial_rotation_cloud

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)
SENTINEL_FLOATS = 16
same_bits, same_values = C.same_bits, C.same_values


@pytest.fixture()
def quiet(plugin):
    plugin.set_async(False)
    plugin.set_pipeline_depth(1)
    plugin.reset_adaptive_state()
    yield plugin
    plugin.set_async(False)
    plugin.set_pipeline_depth(1)


def device_slice(plugin, cloud, settings):
    """`bgst_slice` of a host cloud through device buffers of the plugin's context; each output plane is followed by a
    sentinel, which comes back with it."""
    n = len(cloud)
    widths = (4, 48, 8)
    outs = [np.full(n * w + SENTINEL_FLOATS, SENTINEL, np.float32) for w in widths]
    ptrs = []
    try:
        for plane in cloud.planes():
            ptrs.append(plugin.device_alloc(max(plane.nbytes, 16)))
            if plane.nbytes:
                plugin.upload_bytes(ptrs[-1], plane)
        for o in outs:
            ptrs.append(plugin.device_alloc(o.nbytes))
            plugin.upload_bytes(ptrs[-1], o)
        TimeSlicer(plugin.device).slice(plugin.stream_handle(), n, ptrs[:5], ptrs[5:], settings)
        plugin.synchronize()
        got = [plugin.download(p, np.empty_like(o)) for p, o in zip(ptrs[5:], outs)]
    finally:
        for p in ptrs:
            plugin.device_free(p)
    for g, w in zip(got, widths):
        assert (g[n * w:] == SENTINEL).all(), "the sentinel behind an output plane was overwritten"
    return [g[:n * w].reshape(n, w) for g, w in zip(got, widths)]


# ---- 6. device against twin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.SIZES)
@pytest.mark.parametrize("case", sorted(C.CASES))
def test_slice_equals_the_twin(quiet, case, n):
    cloud, ref = C.cloud(case, n), C.reference(case)
    pv, sh, cov = device_slice(quiet, cloud, C.SETTINGS)
    if n == 0:
        return
    r_pv, r_sh, r_cov = ref.position_visibility[:n], ref.spherical_harmonic[:n], ref.covariance_3d_opacity[:n]
    use = ~C.near_the_mask(case)[:n]
    assert (~use).sum() <= 0.005 * n
    # bit identical: positions (p + delta_mean, or copied), visibility, the covariance, the zeros of the masked, the pad
    # (a NaN lane, as a NaN scale leaves one in an unmasked splat, is NaN on both sides: same_values)
    assert same_values(pv[use], r_pv[use])
    assert same_values(cov[use][:, [0, 1, 2, 3, 4, 5, 7]], r_cov[use][:, [0, 1, 2, 3, 4, 5, 7]])
    masked = ~ref.mask[:n] & use
    assert same_bits(cov[masked], np.zeros((int(masked.sum()), 8), np.float32))
    assert same_bits(pv[masked], np.ascontiguousarray(cloud.position_visibility[masked]))
    # the opacity: opacity * exp(exponent) in float64 of the twin's float32 exponent
    live = ref.mask[:n] & use
    with np.errstate(all="ignore"):
        true_opacity = cloud.scale_opacity[:, 3].astype(np.float64) * np.exp(ref.exponent[:n].astype(np.float64))
    d_op = C.ulp_distance(cov[live, 6], true_opacity[live])
    # the folded coefficients: within FOLD_RELATIVE of |sh0| + |sh1| + |sh2|, NaN where the twin is NaN
    s = np.abs(cloud.spherindrical_harmonic.astype(np.float64)).reshape(n, 3, 48).sum(axis=1)
    with np.errstate(all="ignore"):
        err = np.abs(sh.astype(np.float64) - r_sh.astype(np.float64))
        fold_ok = (err <= C.FOLD_RELATIVE * s) | (np.isnan(sh) & np.isnan(r_sh)) | (sh == r_sh)
        worst = np.nanmax(np.where(s > 0, err / (s * 2.0 ** -24), 0.0)) if n else 0.0
    print(f"{case} n={n}: opacity within {d_op.max() if live.any() else 0:.2f} ulp (bound {C.OPACITY_ULP}), "
          f"folded coefficients within {worst:.2f} x 2^-24 of |sh0|+|sh1|+|sh2| (bound {C.FOLD_RELATIVE * 2 ** 24:.0f})")
    assert (d_op <= C.OPACITY_ULP).all() and fold_ok.all()
    if case == "probe":
        # the three library lanes themselves: marginal = the opacity lane (opacity 1), t1 and t2 = coefficients 0 and 1
        with np.errstate(all="ignore"):
            d_m = C.ulp_distance(cov[live, 6], np.exp(ref.exponent[:n].astype(np.float64))[live])
            d_1 = C.ulp_distance(sh[:, 0], np.cos(ref.cosine_arguments[:n, 0].astype(np.float64)))
            d_2 = C.ulp_distance(sh[:, 1], np.cos(ref.cosine_arguments[:n, 1].astype(np.float64)))
        print(f"probe n={n}: marginal within {d_m.max() if live.any() else 0:.2f} ulp of the float64 exp (bound {C.EXP_ULP}: OCML's 3 + 1), "
              f"t1 {d_1.max():.2f}, t2 {d_2.max():.2f} ulp of the float64 cos (bound {C.COS_ULP}: OCML's 4 + 1)")
        assert (d_m <= C.EXP_ULP).all()         # documented: exp <= 3 ulp, plus one rounding
        assert (d_1 <= C.COS_ULP).all() and (d_2 <= C.COS_ULP).all()    # documented: cos <= 4 ulp, plus one rounding
        assert same_bits(sh[:, 2:], np.ascontiguousarray(cloud.spherindrical_harmonic[:, 2:48]))    # sh + t * 0 + t * 0


# ---- 7. end to end against the oracle --------------------------------------------------------------------------------------------
def test_a_slice_draws_what_the_oracle_draws_of_the_equivalent_3d_cloud(quiet, oracle):
    """2000 splats whose rotation pair is a pure spatial rotation (test_time_slice_host.spatial_rotation_cloud), nonzero
    time coefficients, 320 x 180: slice, upload, sort, render, against the oracle's render of the equivalent
    PlanarGaussian3d — the twin's folded coefficients, opacity * marginal, scales g * s and, since the reference's
    Sigma = M^T M cancels the pair's rotation (slice_math.h), NO rotation: slice_float64's covariance is checked against
    compute_covariance_3d of exactly that cloud first. Then a second frame at a time where most splats are masked."""
    plugin = quiet
    n = 2000
    cloud, _ = spatial_rotation_cloud(n, 77, time_scale=(0.15, 0.5))
    view, draw = View.headless(320, 180), CloudSettings()
    g = 0.75
    frames = []
    for time, lo, hi in ((0.5, 0.5, 1.0), (1.6, 0.01, 0.3)):
        settings = CloudSettings(global_scale=g, time=time, time_start=0.0, time_stop=2.0)
        twin, f = slice_reference(cloud, settings), slice_float64(cloud, settings)
        assert lo <= twin.mask.mean() <= hi, twin.mask.mean()
        keep = twin.mask
        rot = np.tile(np.float32([1, 0, 0, 0]), (n, 1))
        so = np.zeros((n, 4), np.float32)
        so[:, :3] = np.float32(g) * cloud.scale_opacity[:, :3]
        so[:, 3] = twin.covariance_3d_opacity[:, 6]                      # opacity * marginal, 0 for the masked
        assert np.abs(_six(f.covariance) - compute_covariance_3d(rot, so[:, :3]).astype(np.float64))[keep].max() < 1e-6
        # ... and for these pairs the twin's planes ARE that cloud's, bit for bit (spatial_rotation_cloud says why it must be so)
        assert same_bits(twin.covariance_3d_opacity[keep][:, :6], compute_covariance_3d(rot, so[:, :3])[keep])
        assert same_bits(twin.position_visibility, cloud.position_visibility)
        assert np.abs(twin.spherical_harmonic - cloud.spherindrical_harmonic[:, :48]).max() > 0.5    # the time groups matter
        # the masked splats are not in the equivalent cloud at all: the slice must draw only the others
        equivalent = PlanarGaussian3d(twin.position_visibility[keep], twin.spherical_harmonic[keep], rot[keep], so[keep])
        handle, planes = plugin.slice_4d(cloud, settings, return_planes=True)
        try:
            assert handle.format == "cov3d" and len(handle) == n
            differ = (planes[2][:, 6] != 0) != (keep & (so[:, 3] != 0))       # a marginal at the threshold may fall either way
            assert same_bits(planes[0][~differ], twin.position_visibility[~differ])
            assert differ.sum() <= 0.005 * n and same_bits(planes[2][~keep & ~differ], np.zeros((int((~keep & ~differ).sum()), 8), np.float32))
            plugin.sort(handle, view, draw, download=False)
            image = plugin.render(handle, view, draw)
        finally:
            handle.free()
        ref, amb = oracle.render(equivalent, oracle.sort(equivalent, view, draw), view, draw, with_ambiguity=True)
        _assert_image(ref, image, amb, frac_slack=0.01, what=f"4D slice at time {time}")
        assert np.abs(ref[..., :3]).max() > 0.05
        frames.append(image)
    assert not np.array_equal(frames[0], frames[1])


# ---- errors on a live device ----------------------------------------------------------------------------------------------------
def test_errors_name_the_argument(quiet):
    slicer, stream = TimeSlicer(quiet.device), quiet.stream_handle()
    good_in, good_out = [0x1000 * (k + 1) for k in range(5)], [0x1000 * (k + 6) for k in range(3)]
    with pytest.raises(_native_slice.BgsSliceError, match="scale_opacity_device_ptr must be a 16-byte aligned") as ei:
        slicer.slice(stream, 4, good_in[:3] + [good_in[3] + 4] + good_in[4:], good_out, CloudSettings())
    assert ei.value.status == _native_slice.BGST_EINVAL
    with pytest.raises(_native_slice.BgsSliceError, match="out_spherical_harmonic_device_ptr is spherindrical_harmonic_device_ptr as well"):
        slicer.slice(stream, 4, good_in, [good_out[0], good_in[1], good_out[2]], CloudSettings())
    with pytest.raises(_native_slice.BgsSliceError, match="time_stop == time_start"):
        slicer.slice(stream, 4, good_in, good_out, CloudSettings(time_start=1.0, time_stop=1.0))
    slicer.slice(stream, 0, [0] * 5, [0] * 3, CloudSettings())              # n == 0: nothing is enqueued, nothing is looked at
    with pytest.raises(_native_slice.BgsSliceError, match="no usable HIP device 99"):
        TimeSlicer(99).slice(stream, 4, good_in, good_out, CloudSettings())
