"""Point sets the sparse-selection tests share (host and GPU), and the twin's counts for them, each computed once per
run and left unchanged."""
import functools
import itertools

import numpy as np

from bevy_gaussian_splatting_amd.sparse_select import neighbor_counts_reference

RADIUS = 0.05                 # SparseSelect::default
SEED_CLUSTERED = 11           # test_sparse_select_host.py prints the share of points these draws leave near the radius
SEED_UNIFORM = 12
SIZES = (0, 1, 63, 64, 65, 257, 5000)
CELL_EDGE = float(np.float32(RADIUS)) * (1.0 + 1.0 / 1024.0)   # sparse_math.h cell_scale


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def clustered() -> np.ndarray:
    """6000 points in ten Gaussian clusters (sigma 0.03) with centres in [-2, 2]^3, the clusters mixed along the array:
    a point near a centre has some 300 neighbours, one in a tail has none."""
    rng = np.random.default_rng(SEED_CLUSTERED)
    centres = rng.uniform(-2.0, 2.0, (10, 3))
    p = centres[rng.integers(0, 10, 6000)] + rng.normal(0.0, 0.03, (6000, 3))
    return frozen(p.astype(np.float32))


@functools.lru_cache(maxsize=None)
def uniform() -> np.ndarray:
    """6000 points uniform in [-0.5, 0.5]^3: 3.1 neighbours a point on average, so the default threshold splits them."""
    return frozen(np.random.default_rng(SEED_UNIFORM).uniform(-0.5, 0.5, (6000, 3)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def lattice() -> np.ndarray:
    """The boundary lattice. A block of 6^3 points at multiples of radius / 2, and pairs (a, a + radius * (1 - 2^-20))
    along each axis with `a` on a multiple of the cell edge and one f32 to either side of it — then the whole set at
    offsets 0, 1000 and 10^6 in all eight sign octants (so -1000 and -10^6 too): negative coordinates, cells past the
    clamp (10^6 / 0.05 > 2^20) and coordinates whose ulp (0.0625 at 10^6) exceeds the radius all occur. Shuffled, so that a
    short prefix holds some of everything."""
    r = float(np.float32(RADIUS))
    k = np.arange(-2, 4, dtype=np.float64) * (r / 2.0)
    base = [np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)]
    step = r * (1.0 - 2.0 ** -20)
    for axis, multiple in itertools.product(range(3), (-1, 0, 1, 3)):
        on = np.float32(multiple * CELL_EDGE)
        for a in (np.nextafter(on, np.float32(-np.inf)), on, np.nextafter(on, np.float32(np.inf))):
            pair = np.full((2, 3), 0.3 * r)
            pair[0, axis] = float(a)
            pair[1, axis] = float(a) + step
            base.append(pair)
    base = np.concatenate(base)
    copies = [np.array(s) * (base + o) for o in (0.0, 1000.0, 1.0e6) for s in itertools.product((1.0, -1.0), repeat=3)]
    p = np.concatenate(copies).astype(np.float32)
    assert p.shape[0] == 24 * (216 + 72) > 5000
    return frozen(p[np.random.default_rng(3).permutation(p.shape[0])])


@functools.lru_cache(maxsize=None)
def coincident() -> np.ndarray:
    """5000 times the same point: one heavy cell, every count 5000."""
    return frozen(np.tile(np.array([[0.3, -1.2, 7.5]], np.float32), (5000, 1)))


@functools.lru_cache(maxsize=None)
def nonfinite() -> np.ndarray:
    """The uniform draw with every 7th point's lanes in turn NaN, +inf, -inf or the largest finite value (finite: it counts
    itself), as float4 whose visibility lane is NaN on every 5th point, which nothing may read."""
    p = np.ones((6000, 4), np.float32)
    p[:, :3] = uniform()
    specials = (np.nan, np.inf, -np.inf, np.finfo(np.float32).max, -np.finfo(np.float32).max)
    for t, row in enumerate(range(1, 6000, 7)):
        p[row, t % 3] = specials[t % 5]
    p[3] = (np.nan, np.inf, -np.inf, 1.0)
    p[::5, 3] = np.nan
    return frozen(p)


CASES = {"clustered": clustered, "uniform": uniform, "lattice": lattice, "nonfinite": nonfinite}


def points(case: str, n: int) -> np.ndarray:
    """The first n points of a case."""
    return CASES[case]()[:n]


@functools.lru_cache(maxsize=None)
def reference(case: str, n: int, radius: float = RADIUS) -> np.ndarray:
    """The twin's counts of the first n points of a case (counted among themselves)."""
    return frozen(neighbor_counts_reference(points(case, n), radius))


def float4(p) -> np.ndarray:
    p = np.asarray(p, np.float32)
    if p.shape[1] == 4:
        return np.ascontiguousarray(p)
    out = np.ones((p.shape[0], 4), np.float32)
    out[:, :3] = p
    return out
