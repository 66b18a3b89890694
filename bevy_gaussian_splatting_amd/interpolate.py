"""The morph between two Gaussian clouds (src/morph/interpolate.rs, src/morph/interpolate.wgsl): an entity with
`GaussianInterpolate { lhs, rhs }` gets an output cloud that is the per-splat linear blend of two clouds of equal length
at `CloudSettings.time` between `time_start` and `time_stop`.

The blend runs on the device (`bgsm_interpolate_f32` / `bgsm_interpolate_cov3d_f32`, csrc_morph/morph_kernels.hip,
through libbgs_morph.so) on planes that live in device memory; this module holds the ctypes wrapper
`GaussianInterpolator`, `interpolate_reference`, a numpy twin of the arithmetic contract (csrc_morph/morph_math.h) that
the tests compare the device with bit for bit, `interpolation_factor`, and `interpolate_float64`, the same blend in
float64 for the tests.

A side is a `PlanarGaussian3d` (the f32 layout: position_visibility, spherical_harmonic, rotation, scale_opacity) or a
tuple of planes: four for that layout, three for the precomputed-covariance layout (position_visibility,
spherical_harmonic, covariance_3d_opacity; `covariance_planes` makes them of a cloud)."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native_morph
from .gaussian import SH_COEFF_COUNT, PlanarGaussian3d, covariance_3d_opacity
from .settings import CloudSettings

STEP_BELOW = np.float32(1e-6)
F32_WIDTHS = (4, SH_COEFF_COUNT, 4, 4)       # position_visibility, spherical_harmonic, rotation, scale_opacity
COV3D_WIDTHS = (4, SH_COEFF_COUNT, 8)        # position_visibility, spherical_harmonic, covariance_3d_opacity


def covariance_planes(cloud: PlanarGaussian3d):
    """The three planes of a cloud in the precomputed-covariance layout, the covariance plane made by the function
    `plugin.upload(..., precompute_covariance_3d=True)` uses."""
    return cloud.position_visibility, cloud.spherical_harmonic, np.ascontiguousarray(covariance_3d_opacity(cloud), np.float32)


def planes_of(side):
    """A side's planes as contiguous float32 arrays, their shapes checked: four or three (see the module's text)."""
    planes = (side.position_visibility, side.spherical_harmonic, side.rotation, side.scale_opacity) \
        if isinstance(side, PlanarGaussian3d) else tuple(side)
    widths = {4: F32_WIDTHS, 3: COV3D_WIDTHS}.get(len(planes))
    if widths is None:
        raise ValueError("a side has four planes (f32 layout) or three (precomputed-covariance layout)")
    planes = tuple(np.ascontiguousarray(p, np.float32) for p in planes)
    n = planes[0].shape[0]
    for p, w in zip(planes, widths):
        if p.shape != (n, w):
            raise ValueError(f"expected a plane of shape {(n, w)}, got {p.shape}")
    return planes


def _times(settings: CloudSettings):
    t, t0, t1 = np.float32(settings.time), np.float32(settings.time_start), np.float32(settings.time_stop)
    for name, v in (("time", t), ("time_start", t0), ("time_stop", t1)):
        if not np.isfinite(v):
            raise ValueError(f"{name} {float(v):g} must be finite")
    return t, t0, t1


def interpolation_factor(settings: CloudSettings) -> np.float32:
    """`t` of interpolate.wgsl:51-57 in float32, operation by operation (morph_math.h FACTOR): the clamped quotient, or
    the step at `time_stop` where |time_stop - time_start| < 1e-6. The weight of the lhs is `float32(1) - t`."""
    time, start, stop = _times(settings)
    with np.errstate(all="ignore"):
        duration = stop - start
        if np.abs(duration) < STEP_BELOW:
            return np.float32(1.0) if time >= stop else np.float32(0.0)
        x = (time - start) / duration
    t = x if x > np.float32(0.0) else np.float32(0.0)
    return np.float32(1.0) if t > np.float32(1.0) else np.float32(t)


def _mix(a, b, t, u):
    return (a * u) + (b * t)


def normalize_quaternion_reference(q: np.ndarray) -> np.ndarray:
    """morph_math.h normalize_quaternion on [n, 4] float32 rows in stored order [w, x, y, z]: q / sqrt(len2), or the
    stored lanes (0, 0, 0, 1) where len2 <= 0; a NaN len2 gives four NaNs."""
    with np.errstate(all="ignore"):
        len2 = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
        out = q / np.sqrt(len2)[:, None]
    out[len2 <= np.float32(0.0)] = np.float32([0.0, 0.0, 0.0, 1.0])
    assert out.dtype == np.float32
    return out


def interpolate_reference(lhs, rhs, settings: CloudSettings):
    """The morph as the device computes it (csrc_morph/morph_math.h): float32, operation by operation, every one rounded
    once, in the contract's order. Returns the output's planes in the sides' layout: four, or three."""
    a, b = planes_of(lhs), planes_of(rhs)
    if len(a) != len(b):
        raise ValueError("lhs and rhs are in different layouts")
    if a[0].shape[0] != b[0].shape[0]:
        raise ValueError(f"lhs has {a[0].shape[0]} splats, rhs {b[0].shape[0]}: a morph needs two clouds of equal length")
    t = interpolation_factor(settings)
    u = np.float32(1.0) - t
    with np.errstate(all="ignore"):
        out = [_mix(p, q, t, u) for p, q in zip(a, b)]
    if len(a) == 4:
        out[2] = normalize_quaternion_reference(out[2])
    else:
        out[2][:, 7] = np.float32(0.0)
    for p in out:
        assert p.dtype == np.float32 and p.flags.c_contiguous
    return tuple(out)


def interpolate_float64(lhs, rhs, settings: CloudSettings):
    """The same blend in float64, for the tests: a (1 - t) + b t with the float32 factor taken as exact; the rotation
    normalised in float64 (rows of length 0 are left 0); the covariance layout's pad lane 0."""
    a, b = planes_of(lhs), planes_of(rhs)
    t = float(interpolation_factor(settings))
    with np.errstate(all="ignore"):
        out = [p.astype(np.float64) * (1.0 - t) + q.astype(np.float64) * t for p, q in zip(a, b)]
        if len(a) == 4:
            norm = np.sqrt((out[2] ** 2).sum(axis=1, keepdims=True))
            out[2] = np.where(norm > 0, out[2] / np.where(norm > 0, norm, 1.0), 0.0)
        else:
            out[2][:, 7] = 0.0
    return tuple(out)


class GaussianInterpolator:
    """`bgsm_interpolate_f32` / `bgsm_interpolate_cov3d_f32` over device buffers the caller owns. It keeps no device
    state: `interpolate` only enqueues on the stream it is given, and what it writes is complete once that stream reaches
    that point (include/bgs_morph.h "ORDERING")."""

    F32_ROW_BYTES = (16, 192, 16, 16)        # position_visibility, spherical_harmonic, rotation, scale_opacity, a splat
    COV3D_ROW_BYTES = (16, 192, 32)          # position_visibility, spherical_harmonic, covariance_3d_opacity

    def __init__(self, device: int = 0):
        self._lib = _native_morph.load()
        self.device = int(device)

    def interpolate(self, stream: int, n: int, lhs_ptrs, rhs_ptrs, out_ptrs, settings: CloudSettings) -> None:
        """Enqueue the blend of the `n` splats whose planes are at `lhs_ptrs` and `rhs_ptrs` into the planes at
        `out_ptrs`, at `settings.time` (time_start and time_stop are read as well). Four planes a side are the f32
        layout, three the precomputed-covariance layout."""
        sides = [[ctypes.c_void_p(p or 0) for p in ptrs] for ptrs in (lhs_ptrs, rhs_ptrs, out_ptrs)]
        planes = len(sides[0])
        if planes not in (3, 4) or any(len(s) != planes for s in sides):
            raise ValueError("a morph takes four planes a side (f32 layout) or three (precomputed-covariance layout), the same on "
                             "the lhs, the rhs and the output")
        fn = self._lib.bgsm_interpolate_f32 if planes == 4 else self._lib.bgsm_interpolate_cov3d_f32
        _native_morph.check(self._lib, fn(self.device, ctypes.c_void_p(stream or 0), int(n), *sides[0], *sides[1], *sides[2],
                                          ctypes.c_float(settings.time), ctypes.c_float(settings.time_start),
                                          ctypes.c_float(settings.time_stop)))
