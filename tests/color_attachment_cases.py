"""The smallest case of the colour-attachment tests (include/bgs.h BGS_VIEW_ATTACH_COLOR), shared by
test_color_attachment_host.py and test_color_attachment_gpu.py.

A 40 x 24 viewport (the last tile column and the last tile row are partial) and 300 splats of
random_gaussians_3d_seeded at a global_scale that saturates some pixels and leaves others empty. The depth plane has three
parts, left to right: a third of the pixels at 0.0 (everything passes), a third fully occluding (1.0, the near plane: nothing
passes), and a third a diagonal cuts — 0.0 above it, occluding below it, and along it a band of pixels whose SAMPLES
alternate between 0.0 and occluding (at one sample per pixel: whose pixels alternate), the pixels a host cannot composite
after the fact. The colour plane is random in [0, 2) per sample and channel."""
import numpy as np

from bevy_gaussian_splatting_amd import CloudSettings, View, random_gaussians_3d_seeded

W, H = 40, 24
N = 300
SEED = 61
GLOBAL_SCALE = 0.8
GLOBAL_OPACITY = 2.0   # fragments reach the alpha cap of 0.999: a pixel two of them cover is saturated
OCCLUDING = 1.0   # reverse-Z: the near plane; a quad's depth is in (0, 1), so z >= 1.0 never holds
HALF_ULP = 2.0 ** -24   # of a value in [1, 2); a half-ulp of x is at most HALF_ULP * |x|

_CACHE = {}


def cloud(seed: int = SEED):
    key = ("cloud", seed)
    if key not in _CACHE:
        c = random_gaussians_3d_seeded(N, seed)
        for a in (c.position_visibility, c.spherical_harmonic, c.rotation, c.scale_opacity):
            a.setflags(write=False)
        _CACHE[key] = c
    return _CACHE[key]


def view(samples: int, clear=(0.0, 0.0, 0.0, 0.0)) -> View:
    v = View.headless(W, H, msaa_samples=samples)
    v.clear_color = tuple(float(c) for c in clear)
    return v


def settings(**kw) -> CloudSettings:
    kw.setdefault("global_scale", GLOBAL_SCALE)
    kw.setdefault("global_opacity", GLOBAL_OPACITY)
    return CloudSettings(**kw)


def depth_plane(samples: int) -> np.ndarray:
    """[H, W, samples] float32, read-only."""
    key = ("depth", samples)
    if key not in _CACHE:
        d = np.zeros((H, W, samples), np.float32)
        x1, x2 = W // 3, 2 * W // 3
        d[:, x1:x2] = OCCLUDING
        yy, xx, ss = np.mgrid[0:H, x2:W, 0:samples]
        t = (xx - x2) - yy * ((W - x2) / H)          # > 0 above the diagonal, < 0 below it
        band = np.where((xx + yy + ss) % 2 == 1, OCCLUDING, 0.0)
        d[:, x2:] = np.where(t > 2.0, 0.0, np.where(t < -2.0, OCCLUDING, band)).astype(np.float32)
        d.setflags(write=False)
        _CACHE[key] = d
    return _CACHE[key]


def mixed_pixels(samples: int) -> np.ndarray:
    """[H, W] bool: pixels whose samples (S = 1: whose horizontal neighbours) disagree about the occluder."""
    d = depth_plane(samples)
    if samples > 1:
        return d.min(axis=2) != d.max(axis=2)
    m = np.zeros((H, W), bool)
    m[:, 1:] = d[:, 1:, 0] != d[:, :-1, 0]
    return m


def color_plane(samples: int, seed: int = 7) -> np.ndarray:
    """[H, W, samples, 4] float32 in [0, 2), read-only."""
    key = ("color", samples, seed)
    if key not in _CACHE:
        c = (2.0 * np.random.default_rng(seed).random((H, W, samples, 4), dtype=np.float32)).astype(np.float32)
        c.setflags(write=False)
        _CACHE[key] = c
    return _CACHE[key]


def composite_float64(C, T, dst) -> np.ndarray:
    """C + mean_s(T_s d_s) in float64: what the twin (camera.composite_reference) rounds S + 1 times on the way to."""
    C, T, dst = (np.asarray(a, np.float64) for a in (C, T, dst))
    return C + (T[..., None] * dst).sum(axis=-2) / T.shape[-1]


def twin_bound(C, T, dst) -> np.ndarray:
    """The twin's rounding model against composite_float64, per value: the accumulator takes S roundings (one product, S - 1
    fused multiply-adds), each at most a half-ulp of a partial sum, i.e. of at most A = sum_s |T_s d_s|, and is then scaled by
    1/S exactly; the last fused multiply-add rounds once more, at most a half-ulp of |C| + A/S; and the float64 evaluation
    itself is within a half-ulp of f32 of the same magnitude many times over. (S + 2) half-ulps of M = |C| + A, the largest
    magnitude any term or partial sum can reach."""
    C, T, dst = (np.asarray(a, np.float64) for a in (C, T, dst))
    S = T.shape[-1]
    M = np.abs(C) + np.abs(T[..., None] * dst).sum(axis=-2)
    return (S + 2) * HALF_ULP * M
