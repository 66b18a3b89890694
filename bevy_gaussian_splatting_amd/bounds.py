"""The box of a cloud as `BGS_BOUNDS_CLOUD` takes it on the device (include/bgs.h, `bgs_settings.reserved[0]`;
`CloudSettings(bounds_from_cloud=True)`): the numpy twin of csrc/bounds_math.h, bit for bit.

`CommonCloud::compute_aabb` (src/gaussian/interface.rs:22-63): per axis, over the untransformed `position_visibility[:, :3]`,
`min = fold(+inf, f32::min)` of `p - 0.1f` and `max = fold(-inf, f32::max)` of `p + 0.1f`, every operation rounded once in
f32. `f32::min` / `max` ignore a NaN operand, which is what `numpy.fmin` / `fmax` do; an axis with no contributor keeps
`+inf` / `-inf`. The visibility lane is not read. (`settings.compute_aabb` is the other route the reference takes to the
same box, through Bevy's `Aabb {center, half_extents}`, which rounds twice more; the device follows `compute_aabb` itself.)"""
from __future__ import annotations

import numpy as np

BOUNDS_CALLER = 0     # BGS_BOUNDS_CALLER
BOUNDS_CLOUD = 1      # BGS_BOUNDS_CLOUD
MAX_SCALE = np.float32(0.1)
BOUNDS_THREADS = 256


def bounds_reference(position_visibility):
    """(min, max), two float32 arrays of three: the box `BGS_BOUNDS_CLOUD` gives a cloud with these positions ([n, 3] or
    [n, 4]; a fourth column is ignored). None for an empty cloud, like the reference."""
    p = np.asarray(position_visibility, dtype=np.float32)
    if p.ndim != 2 or p.shape[1] not in (3, 4):
        raise ValueError("positions must be [n, 3] or [n, 4]")
    if p.shape[0] == 0:
        return None
    xyz = p[:, :3]
    with np.errstate(invalid="ignore"):
        lo = np.fmin.reduce((xyz - MAX_SCALE).astype(np.float32), axis=0, initial=np.float32(np.inf))
        hi = np.fmax.reduce((xyz + MAX_SCALE).astype(np.float32), axis=0, initial=np.float32(-np.inf))
    return lo.astype(np.float32), hi.astype(np.float32)


def bounds_key(bits):
    """The order-preserving key of float32 bit patterns (uint32): `bits ^ (sign ? 0xFFFFFFFF : 0x80000000)`. Unsigned order
    of the keys is the order of the floats, -0 below +0."""
    b = np.asarray(bits, dtype=np.uint32)
    return b ^ np.where(b & np.uint32(0x80000000), np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def bounds_key_bits(key):
    """The inverse of `bounds_key`."""
    k = np.asarray(key, dtype=np.uint32)
    return k ^ np.where(k & np.uint32(0x80000000), np.uint32(0x80000000), np.uint32(0xFFFFFFFF)).astype(np.uint32)


def bounds_grid(n: int, compute_units: int, grid_cap: int = 0) -> int:
    """Workgroups of the device reduction for `n` splats (csrc/bounds_math.h `bounds_grid`): one per 256 splats, at most
    two per compute unit, at most `grid_cap` when that is set (`bgs_set_grid_cap`)."""
    most = 2 * max(int(compute_units), 1)
    if grid_cap and grid_cap < most:
        most = int(grid_cap)
    return min(-(-int(n) // BOUNDS_THREADS), most)


def bounds_single_sweep_reach(compute_units: int, grid_cap: int = 0) -> int:
    """Splats the largest grid visits in one sweep of its lanes: a cloud beyond it makes lanes come back for more."""
    return bounds_grid(1 << 30, compute_units, grid_cap) * BOUNDS_THREADS
