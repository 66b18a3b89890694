"""4D clouds the time-slice tests share (host and GPU), the twin's slice of each, computed once per run and left
unchanged, and the bounds of the lanes that pass through a math library, with where they come from."""
import functools

import numpy as np

from bevy_gaussian_splatting_amd import CloudSettings, PlanarGaussian4d, random_gaussians_4d_seeded
from bevy_gaussian_splatting_amd.time_slice import slice_float64, slice_reference

SIZES = (0, 1, 63, 64, 65, 257, 5000)
N = 5000
SEED_RANDOM = 41          # test_time_slice_host.py checks that these draws leave under 0.5 % of a case near the mask
SEED_EDGE = 42
SEED_PROBE = 43
SETTINGS = CloudSettings(global_scale=0.875, time=0.375, time_start=-0.25, time_stop=1.5)

# ---- the lanes that pass through exp / cos --------------------------------------------------------------------------------
# The device's expf and cosf are the ROCm device library's (OCML), which documents that it meets the accuracy the OpenCL
# specification requires: exp <= 3 ulp, cos <= 4 ulp. One more ulp for the rounding that the word "ulp" hides (the
# spacing of float32 changes at a power of two, and the distance is taken at the float64 value's binade).
EXP_ULP = 3 + 1
COS_ULP = 4 + 1
# opacity * marginal: B ulp on the marginal are at most B * 2^-23 relative, the product rounds once more (2^-24), and a
# relative error r is at most r * 2^24 ulp of the product: 2 B + 1.
OPACITY_ULP = 2 * EXP_ULP + 1
# A folded coefficient (sh0 + t1 sh1) + t2 sh2 with |t| <= 1: the twin's cosine is the float64 one rounded, the device's
# within COS_ULP of it, an ulp of a cosine is at most 2^-24, so the cosines differ by (COS_ULP + 1) * 2^-24 at most; the
# four operations round to 2^-24 of a result that is at most S = |sh0| + |sh1| + |sh2|, on both sides: 8 * 2^-24 * S.
FOLD_RELATIVE = (COS_ULP + 1 + 8) * 2.0 ** -24


def frozen(cloud: PlanarGaussian4d) -> PlanarGaussian4d:
    for p in cloud.planes():
        p.setflags(write=False)
    return cloud


@functools.lru_cache(maxsize=None)
def random() -> PlanarGaussian4d:
    """The reference's distribution as it is: rotations that are not normalised, time scales of both signs."""
    return frozen(random_gaussians_4d_seeded(N, SEED_RANDOM))


@functools.lru_cache(maxsize=None)
def edge() -> PlanarGaussian4d:
    """The random draw with, in turn on every 5th splat from splat 1 on: time_scale 0; time_scale 0 AND dt = 0; dt = 0;
    a zero first quaternion; both quaternions zero; a NaN, +inf or -inf in one lane of position, rotation, scale, opacity,
    timestamp or time_scale; a time_scale so small that cov_t is denormal; a timestamp far away (marginal 0). Shuffled
    into every prefix by the stride."""
    c = random_gaussians_4d_seeded(N, SEED_EDGE)
    pv, sh, rot, so, tt = (np.array(p) for p in c.planes())
    t = np.float32(SETTINGS.time)
    specials = (np.nan, np.inf, -np.inf)
    for k, row in enumerate(range(1, N, 5)):
        kind = k % 12
        if kind == 0:
            tt[row, 1] = 0.0
        elif kind == 1:
            tt[row, 1], tt[row, 0] = 0.0, t
        elif kind == 2:
            tt[row, 0] = t
        elif kind == 3:
            rot[row, :4] = 0.0
        elif kind == 4:
            rot[row] = 0.0
        elif kind == 5:
            pv[row, k % 3] = specials[k % 3]
        elif kind == 6:
            rot[row, k % 8] = specials[k % 3]
        elif kind == 7:
            so[row, k % 4] = specials[k % 3]
        elif kind == 8:
            tt[row, k % 2] = specials[k % 3]
        elif kind == 9:
            tt[row, 1] = 1e-20
        elif kind == 10:
            tt[row, 0] = 1e6
        else:
            tt[row, 1] = -tt[row, 1]
    return frozen(PlanarGaussian4d(pv, sh, rot, so, tt))


@functools.lru_cache(maxsize=None)
def probe() -> PlanarGaussian4d:
    """A cloud whose outputs SHOW the three library lanes: opacity 1, so the opacity lane is the marginal itself
    (1 * m = m); coefficient 0 has groups (0, 1, 0) and coefficient 1 (0, 0, 1), so those two outputs are t1 and t2
    themselves ((0 + t1 * 1) + t2 * 0 = t1); every other coefficient has zero time groups and must come out as it went
    in. Time scales in [0.05, 0.65] keep most splats unmasked, not all."""
    c = random_gaussians_4d_seeded(N, SEED_PROBE)
    pv, sh, rot, so, tt = (np.array(p) for p in c.planes())
    so[:, 3] = 1.0
    sh[:, 48:] = 0.0
    sh[:, 0], sh[:, 48] = 0.0, 1.0
    sh[:, 1], sh[:, 97] = 0.0, 1.0
    tt[:, 1] = 0.05 + 0.6 * np.abs(tt[:, 1])
    return frozen(PlanarGaussian4d(pv, sh, rot, so, tt))


CASES = {"random": random, "edge": edge, "probe": probe}


def cloud(case: str, n: int) -> PlanarGaussian4d:
    """The first n splats of a case."""
    return CASES[case]().slice(0, n)


@functools.lru_cache(maxsize=None)
def reference(case: str):
    """The twin's slice of a whole case at SETTINGS (a splat's slice does not depend on the others: a prefix of it is the
    slice of the prefix)."""
    r = slice_reference(CASES[case](), SETTINGS)
    for a in vars(r).values():
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def float64(case: str):
    return slice_float64(CASES[case](), SETTINGS)


def same_bits(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_values(a, b) -> bool:
    """Bit for bit, but for NaNs: a NaN's sign and payload are no part of the contract (slice_math.h), so NaN equals NaN."""
    if a.dtype != np.float32 or b.dtype != np.float32 or a.shape != b.shape:
        return False
    return bool(((np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def ulp_distance(got, true64) -> np.ndarray:
    """|got - true| in units of float32's spacing at the true value; 0 where both are the same non-finite value or
    both NaN, inf where only one is finite."""
    got64, true64 = np.asarray(got, np.float64), np.asarray(true64, np.float64)
    with np.errstate(all="ignore"):
        spacing = np.spacing(np.abs(true64).astype(np.float32)).astype(np.float64)
        d = np.abs(got64 - true64) / spacing
    same = (np.isnan(got64) & np.isnan(true64)) | (got64 == true64)
    d = np.where(same, 0.0, d)
    return np.where(np.isnan(d), np.inf, d)


@functools.lru_cache(maxsize=None)
def near_the_mask(case: str) -> np.ndarray:
    """Splats whose float64 marginal (of the twin's float32 exponent) lies within EXP_ULP of 0.05: a math library may put
    them on either side of the mask. They are left out of the device comparison."""
    r = reference(case)
    with np.errstate(all="ignore"):
        m = np.exp(r.exponent.astype(np.float64))
    out = np.abs(m - float(np.float32(0.05))) <= EXP_ULP * float(np.spacing(np.float32(0.05)))
    out.setflags(write=False)
    return out
