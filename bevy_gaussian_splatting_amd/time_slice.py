"""The time slice of a 4D Gaussian cloud (src/render/gaussian_4d.wgsl, src/material/spherindrical_harmonics.wgsl): at
`CloudSettings.time` a `PlanarGaussian4d` is a 3D cloud in the precomputed-covariance layout — conditioned mean,
conditional covariance, opacity times the temporal marginal, and 48 coefficients into which the two time cosines are
folded.

The slice runs on the device (`bgst_slice`, csrc_slice/slice_kernels.hip, through libbgs_slice.so) on planes that live
in device memory; this module holds the ctypes wrapper `TimeSlicer`, `slice_reference`, a numpy twin of the arithmetic
contract (csrc_slice/slice_math.h) that the tests compare the device with bit for bit, and `slice_float64`, the same
geometry as linear algebra in float64 together with the reference's own colour formula."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _native_slice
from .gaussian import SH_COEFF_COUNT, PlanarGaussian4d
from .settings import CloudSettings

MASK_THRESHOLD = np.float32(0.05)
TWO_PI = np.float32(2.0) * np.float32(np.pi)
FOUR_PI = np.float32(4.0) * np.float32(np.pi)

# src/material/spherical_harmonics.wgsl:3-20
SHC = (0.28209479177387814, -0.4886025119029199, 0.4886025119029199, -0.4886025119029199, 1.0925484305920792,
       -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396, -0.5900435899266435,
       2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
       -0.5900435899266435)


@dataclass
class SliceReference:
    """What `slice_reference` returns: the three planes of the slice, the mask, and the lanes that pass through a math
    library, with the float32 arguments they are functions of."""
    position_visibility: np.ndarray      # [n, 4] float32
    spherical_harmonic: np.ndarray       # [n, 48] float32
    covariance_3d_opacity: np.ndarray    # [n, 8] float32
    mask: np.ndarray                     # [n] bool: marginal > 0.05
    exponent: np.ndarray                 # [n] float32: marginal = exp(exponent)
    marginal: np.ndarray                 # [n] float32
    cosine_arguments: np.ndarray         # [n, 2] float32: t1 = cos([:, 0]), t2 = cos([:, 1])
    cosines: np.ndarray                  # [n, 2] float32

    def planes(self):
        return self.position_visibility, self.spherical_harmonic, self.covariance_3d_opacity


def _settings(settings: CloudSettings):
    g, t = np.float32(settings.global_scale), np.float32(settings.time)
    t0, t1 = np.float32(settings.time_start), np.float32(settings.time_stop)
    for name, v in (("global_scale", g), ("time", t), ("time_start", t0), ("time_stop", t1)):
        if not np.isfinite(v):
            raise ValueError(f"{name} {float(v):g} must be finite")
    if t0 == t1:
        raise ValueError(f"time_stop == time_start ({float(t0):g}): the duration is 0")
    with np.errstate(all="ignore"):
        return g, t, t1 - t0


def _dot4(a0, b0, a1, b1, a2, b2, a3, b3):
    return ((a0 * b0 + a1 * b1) + a2 * b2) + a3 * b3


def _rotation_rows(cloud_rot):
    """M_l and M_r of gaussian_4d.wgsl as [row][column] lists of lanes: the WGSL constructors take columns."""
    w, x, y, z, wr, xr, yr, zr = (np.ascontiguousarray(cloud_rot[:, k]) for k in range(8))
    ml = [[w, x, y, z], [-x, w, z, -y], [-y, -z, w, x], [-z, y, -x, w]]
    mr = [[wr, xr, yr, zr], [-xr, wr, -zr, yr], [-yr, zr, wr, -xr], [-zr, -yr, xr, wr]]
    return ml, mr


def slice_reference(cloud: PlanarGaussian4d, settings: CloudSettings, exp=None, cos=None) -> SliceReference:
    """The slice as the device computes it (csrc_slice/slice_math.h): float32, operation by operation, every one
    rounded once, in the contract's order. `exp` and `cos` (float32 array -> float32 array) stand for the math library;
    by default the float64 function of the float32 argument, rounded to float32."""
    exp = exp or (lambda a: np.exp(a.astype(np.float64)).astype(np.float32))
    cos = cos or (lambda a: np.cos(a.astype(np.float64)).astype(np.float32))
    g, time, duration = _settings(settings)
    pv, sh, rot, so, tt = cloud.planes()
    n = len(cloud)
    with np.errstate(all="ignore"):
        ml, mr = _rotation_rows(rot)
        s = [g * so[:, 0], g * so[:, 1], g * so[:, 2], np.ascontiguousarray(tt[:, 1])]
        m = [[_dot4(mr[r][0], ml[0][c], mr[r][1], ml[1][c], mr[r][2], ml[2][c], mr[r][3], ml[3][c]) * s[c] for c in range(4)]
             for r in range(4)]
        sigma = lambda i, j: _dot4(m[0][i], m[0][j], m[1][i], m[1][j], m[2][i], m[2][j], m[3][i], m[3][j])
        dt = time - tt[:, 0]
        cov_t = sigma(3, 3)
        exponent = ((np.float32(-0.5) * dt) * dt) / cov_t
        c = [sigma(0, 3), sigma(1, 3), sigma(2, 3)]
        cov3d = [sigma(i, j) - (c[i] * c[j]) / cov_t for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
        delta = [(c[k] / cov_t) * dt for k in range(3)]
        marginal = exp(exponent)
        mask = marginal > MASK_THRESHOLD
        out_pv = np.array(pv, np.float32, copy=True)
        cov = np.zeros((n, 8), np.float32)
        for k in range(3):
            out_pv[:, k] = np.where(mask, pv[:, k] + delta[k], pv[:, k])
        for k in range(6):
            cov[:, k] = np.where(mask, cov3d[k], np.float32(0.0))
        cov[:, 6] = np.where(mask, so[:, 3] * marginal, np.float32(0.0))
        theta = dt / duration
        args = np.stack([TWO_PI * theta, FOUR_PI * theta], axis=1)
        cosines = np.stack([cos(args[:, 0]), cos(args[:, 1])], axis=1)
        K = SH_COEFF_COUNT
        out_sh = (sh[:, :K] + cosines[:, :1] * sh[:, K:2 * K]) + cosines[:, 1:] * sh[:, 2 * K:]
    for a in (out_pv, cov, out_sh, exponent, marginal, args, cosines):
        assert a.dtype == np.float32
    return SliceReference(out_pv, np.ascontiguousarray(out_sh), cov, mask, exponent, marginal, args, cosines)


@dataclass
class SliceFloat64:
    """What `slice_float64` returns, every array float64."""
    sigma: np.ndarray             # [n, 4, 4]: M^T M
    covariance: np.ndarray        # [n, 3, 3]: the Schur complement of sigma[3, 3] in sigma
    delta_mean: np.ndarray        # [n, 3]
    marginal: np.ndarray          # [n]
    dt: np.ndarray                # [n]
    cosines: np.ndarray           # [n, 2]


def slice_float64(cloud: PlanarGaussian4d, settings: CloudSettings) -> SliceFloat64:
    """The geometry of the slice as linear algebra in float64: Sigma = M^T M with M = (M_r M_l) S, its Schur complement,
    the conditioned mean's offset and the temporal marginal — what gaussian_4d.wgsl computes, without its order."""
    g, time, duration = (float(v) for v in _settings(settings))
    _, _, rot, so, tt = (p.astype(np.float64) for p in cloud.planes())
    ml, mr = _rotation_rows(rot)
    ML = np.stack([np.stack(row, axis=1) for row in ml], axis=1)      # [n, row, column]
    MR = np.stack([np.stack(row, axis=1) for row in mr], axis=1)
    S = np.concatenate([g * so[:, :3], tt[:, 1:2]], axis=1)
    M = (MR @ ML) * S[:, None, :]
    sigma = np.transpose(M, (0, 2, 1)) @ M
    with np.errstate(all="ignore"):
        cov_t = sigma[:, 3, 3]
        c12 = sigma[:, :3, 3]
        covariance = sigma[:, :3, :3] - c12[:, :, None] * c12[:, None, :] / cov_t[:, None, None]
        dt = time - tt[:, 0]
        theta = dt / duration
        return SliceFloat64(sigma, covariance, c12 / cov_t[:, None] * dt[:, None], np.exp(-0.5 * dt * dt / cov_t), dt,
                            np.stack([np.cos(2.0 * np.pi * theta), np.cos(4.0 * np.pi * theta)], axis=1))


def sh_basis_float64(direction) -> np.ndarray:
    """The 16 basis terms of spherical_harmonics.wgsl / spherindrical_harmonics.wgsl (shc[0], l1m1 .. l3p3) for unit
    directions [m, 3], float64 [m, 16]."""
    d = np.asarray(direction, np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, xz, yz = x * x, y * y, z * z, x * y, x * z, y * z
    b = [np.ones_like(x), y, z, x, xy, yz, 2.0 * zz - xx - yy, xz, xx - yy, y * (3.0 * xx - yy), z * xy, y * (4.0 * zz - xx - yy),
         z * (2.0 * zz - 3.0 * xx - 3.0 * yy), x * (4.0 * zz - xx - yy), z * (xx - yy), x * (xx - 3.0 * yy)]
    return np.stack([SHC[k] * b[k] for k in range(16)], axis=1)


def color_4d_float64(spherindrical_harmonic, direction, cosines) -> np.ndarray:
    """spherindrical_harmonics_lookup in float64, in the reference's grouping: 0.5 + the static sum + t1 * (the sum of the
    second group) + t2 * (the sum of the third). Rows pair up: coefficients [m, 144], directions [m, 3], cosines [m, 2]."""
    sh = np.asarray(spherindrical_harmonic, np.float64).reshape(-1, 3, 16, 3)     # [m, group, basis term, channel]
    sums = np.einsum("mb,mgbc->mgc", sh_basis_float64(direction), sh)
    t = np.asarray(cosines, np.float64)
    return 0.5 + sums[:, 0] + t[:, :1] * sums[:, 1] + t[:, 1:] * sums[:, 2]


def color_3d_float64(spherical_harmonic, direction) -> np.ndarray:
    """spherical_harmonics_lookup in float64: 0.5 + the sum over the 16 basis terms; coefficients [m, 48]."""
    sh = np.asarray(spherical_harmonic, np.float64).reshape(-1, 16, 3)
    return 0.5 + np.einsum("mb,mbc->mc", sh_basis_float64(direction), sh)


class TimeSlicer:
    """`bgst_slice` over device buffers the caller owns. It keeps no device state: `slice` only enqueues on the stream it
    is given, and what it writes is complete once that stream reaches that point (include/bgs_slice.h "ORDERING")."""

    IN_ROW_BYTES = (16, 576, 32, 16, 16)      # the five planes of a PlanarGaussian4d, a splat
    OUT_ROW_BYTES = (16, 192, 32)             # position_visibility, spherical_harmonic, covariance_3d_opacity

    def __init__(self, device: int = 0):
        self._lib = _native_slice.load()
        self.device = int(device)

    def slice(self, stream: int, n: int, in_ptrs, out_ptrs, settings: CloudSettings) -> None:
        """Enqueue the slice of the `n` splats whose five planes are at `in_ptrs` into the three planes at `out_ptrs`,
        at `settings.time` (global_scale, time_start and time_stop are read as well)."""
        ins, outs = [ctypes.c_void_p(p or 0) for p in in_ptrs], [ctypes.c_void_p(p or 0) for p in out_ptrs]
        if len(ins) != 5 or len(outs) != 3:
            raise ValueError("a slice takes five planes and writes three")
        _native_slice.check(self._lib, self._lib.bgst_slice(
            self.device, ctypes.c_void_p(stream or 0), int(n), *ins, *outs, ctypes.c_float(settings.global_scale),
            ctypes.c_float(settings.time), ctypes.c_float(settings.time_start), ctypes.c_float(settings.time_stop)))
