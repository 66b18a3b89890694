"""The reference and the cases of tests/test_bin_stage_gpu.py (the binning stage against an exact host reference, list by
list) and of tests/test_bin_stage_host.py, which shows on the CPU that every case holds what it is named for. numpy only,
deterministic. All of it is integer work: every comparison made with these references is exact equality.

The stage: bin_kernel<4> / <16> (BINNING_SCAN: packed tile rectangles -> ordered supertile lists) and, for BINNING_SORT,
the instance expansion of project_emit_kernel, the two tile-id digit passes and tile_ranges_kernel
(bevy_gaussian_splatting_amd/csrc/render_kernels.hip)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import vertex_stage_cases as VC
from bevy_gaussian_splatting_amd import CloudSettings, SortMode, View, compute_aabb

RECT_EMPTY = 0x000000FF     # csrc/bgs_device.h
BIN_RANKS = 1024            # ranks per bin_kernel workgroup (render_kernels.hip)
BIN_LOOKBACK = 4            # status words per look-back hop (BGS_BIN_LOOKBACK)
MAX_SUPERTILES = 256
GUARD = 64                  # BGS_SELFTEST_BIN_GUARD (include/bgs_diag.h)
FILL = 0xFFFFFFFF           # what bgs_selftest_bin fills the lists with


def pack(x0, x1, y0, y1) -> np.ndarray:
    return (np.asarray(x0, np.uint32) | (np.asarray(x1, np.uint32) << 8) | (np.asarray(y0, np.uint32) << 16) |
            (np.asarray(y1, np.uint32) << 24)).astype(np.uint32)


def unpack(rects):
    r = np.asarray(rects, np.uint32).astype(np.int64)
    return r & 255, (r >> 8) & 255, (r >> 16) & 255, r >> 24


def grid_supertiles(tiles_x: int, tiles_y: int, edge: int):
    return -(-tiles_x // edge), -(-tiles_y // edge)


# ---- the references --------------------------------------------------------------------------------------------------
def reference_lists(rects, tiles_x: int, tiles_y: int, edge: int) -> list:
    """The list of supertile (sx, sy), at index sy * sup_x + sx: the ascending ranks j whose rectangle is not RECT_EMPTY
    and has x0 // edge <= sx <= x1 // edge and y0 // edge <= sy <= y1 // edge, each entry (j, rects[j]); uint32 [len, 2].
    Plain integer division."""
    rects = np.asarray(rects, np.uint32)
    x0, x1, y0, y1 = unpack(rects)
    live = rects != RECT_EMPTY
    sx0, sx1, sy0, sy1 = x0 // edge, x1 // edge, y0 // edge, y1 // edge
    sup_x, sup_y = grid_supertiles(tiles_x, tiles_y, edge)
    lists = []
    for sy in range(sup_y):
        row = live & (sy0 <= sy) & (sy <= sy1)
        for sx in range(sup_x):
            j = np.nonzero(row & (sx0 <= sx) & (sx <= sx1))[0]
            lists.append(np.stack([j.astype(np.uint32), rects[j]], axis=1))
    return lists


def brute_force_lists(rects, tiles_x: int, tiles_y: int, edge: int) -> list:
    """reference_lists as a triple loop over (rank, sx, sy) on Python integers (the host test holds the two together)."""
    sup_x, sup_y = grid_supertiles(tiles_x, tiles_y, edge)
    lists = [[] for _ in range(sup_x * sup_y)]
    for j, r in enumerate(int(v) for v in rects):
        if r == RECT_EMPTY:
            continue
        x0, x1, y0, y1 = r & 255, (r >> 8) & 255, (r >> 16) & 255, r >> 24
        for sx in range(sup_x):
            for sy in range(sup_y):
                if x0 // edge <= sx <= x1 // edge and y0 // edge <= sy <= y1 // edge:
                    lists[sy * sup_x + sx].append((j, r))
    return [np.array(l, np.uint32).reshape(-1, 2) for l in lists]


def reference_instances(rects):
    """(instances, ranges, present) of the sort pipeline: instances uint32 [count, 2] = every (ty << 8 | tx, j) for the
    tiles inside rank j's rectangle, sorted by (key, j); ranges int64 [65536, 2] = [first, end) of the keys present (and
    0, 0 of the absent ones: what is asked of those is start == end); present bool [65536]."""
    rects = np.asarray(rects, np.uint32)
    x0, x1, y0, y1 = unpack(rects)
    live = np.nonzero(rects != RECT_EMPTY)[0]
    w, h = (x1 - x0 + 1)[live], (y1 - y0 + 1)[live]
    area = w * h
    j = np.repeat(live, area)
    k = np.arange(int(area.sum())) - np.repeat(np.cumsum(area) - area, area)
    wj = np.repeat(w, area)
    row, col = k // wj, k % wj
    key = ((y0[j] + row) << 8) | (x0[j] + col)
    order = np.lexsort((j, key))
    key, j = key[order], j[order]
    inst = np.stack([key.astype(np.uint32), j.astype(np.uint32)], axis=1)
    ranges = np.zeros((65536, 2), np.int64)
    present = np.zeros(65536, bool)
    if len(key):
        first = np.nonzero(np.concatenate([[True], key[1:] != key[:-1]]))[0]
        end = np.concatenate([first[1:], [len(key)]])
        ranges[key[first], 0], ranges[key[first], 1] = first, end
        present[key[first]] = True
    return inst, ranges, present


def block_hits(lists, n: int) -> np.ndarray:
    """int64 [blocks, supertiles]: how many entries each BIN_RANKS block of ranks appends to each list."""
    blocks = -(-n // BIN_RANKS)
    out = np.zeros((blocks, len(lists)), np.int64)
    for s, l in enumerate(lists):
        if len(l):
            out[:, s] = np.bincount(l[:, 0].astype(np.int64) // BIN_RANKS, minlength=blocks)
    return out


def supertile_edge(tiles_x: int, tiles_y: int, level: int):
    """(edge, level run at) of a frame forced to `level`: frame_params.h's supertile_edges + canonical_supertile_level +
    plan_frame's supertile_bins_fit fall-back, restated."""
    def fit(edge):
        bx, by = grid_supertiles(tiles_x, tiles_y, edge)
        return bx * by <= MAX_SUPERTILES and bx <= 32 and by <= 32
    edge_c = 8
    while not fit(edge_c):
        edge_c *= 2
    edge_f = (3 * edge_c + 3) // 4
    while not fit(edge_f):
        edge_f += 1
    edges = [min(edge_f, edge_c)] + [min(edge_c << (k - 1), 32) for k in (1, 2, 3)]
    while level > 1 and edges[level - 1] == edges[level]:
        level -= 1
    return (edges[level] if fit(edges[level]) else edges[1]), level


# ---- rectangle families ----------------------------------------------------------------------------------------------
def _small_live(rng, n, tx, ty):
    w, h = np.minimum(rng.integers(1, 3, n), tx), np.minimum(rng.integers(1, 3, n), ty)
    x0, y0 = rng.integers(0, tx - w + 1), rng.integers(0, ty - h + 1)
    return pack(x0, x0 + w - 1, y0, y0 + h - 1)


def _small(rng, n, tx, ty, first_rank=0):
    r = _small_live(rng, n, tx, ty)
    r[(np.arange(n) + first_rank) % 8 == 5] = RECT_EMPTY      # an eighth of them
    return r


def _wide(rng, n, tx, ty):
    w, h = rng.integers(-(-tx // 2), tx + 1, n), rng.integers(-(-ty // 2), ty + 1, n)
    x0, y0 = rng.integers(0, tx - w + 1), rng.integers(0, ty - h + 1)
    return pack(x0, x0 + w - 1, y0, y0 + h - 1)


def _full(n, tx, ty):
    return np.full(n, pack(0, tx - 1, 0, ty - 1), np.uint32)


def _mixed(rng, n, tx, ty):
    out = np.empty(n, np.uint32)
    for b, lo in enumerate(range(0, n, BIN_RANKS)):
        m = min(BIN_RANKS, n - lo)
        out[lo:lo + m] = (_small(rng, m, tx, ty, lo), _wide(rng, m, tx, ty), np.full(m, RECT_EMPTY, np.uint32))[b % 3]
    return out


def _border_coords(tiles: int, edge: int) -> np.ndarray:
    c = {0, tiles - 1}
    for k in range(1, -(-tiles // edge)):
        c |= {k * edge - 1, k * edge}
    return np.array(sorted(v for v in c if 0 <= v < tiles))


def _boundary(rng, n, tx, ty, edge):
    """Edges at k * edge - 1, k * edge, the last tile and tile 0: a third of the rectangles one tile wide / high on such a
    coordinate, a third two wide from it (k * edge - 1 .. k * edge straddles the border), a third from one such coordinate
    to another."""
    def axis(tiles):
        c = _border_coords(tiles, edge)
        a, b = c[rng.integers(0, len(c), n)], c[rng.integers(0, len(c), n)]
        kind = np.arange(n) % 3
        lo = np.where(kind == 2, np.minimum(a, b), a)
        hi = np.where(kind == 0, a, np.where(kind == 1, np.minimum(a + 1, tiles - 1), np.maximum(a, b)))
        return lo, hi
    x0, x1 = axis(tx)
    p = rng.permutation(n)                                # the two axes' kinds are independent
    y0, y1 = axis(ty)
    return pack(x0, x1, y0[p], y1[p])


THRESHOLD_COUNTS = (31, 32, 33)   # non-empty rectangles per block: either side of 32 * num_st on a one-supertile grid


def _threshold(rng, tx, ty):
    n = 2 * BIN_RANKS + 700
    out = np.full(n, RECT_EMPTY, np.uint32)
    for b, count in enumerate(THRESHOLD_COUNTS):
        m = min(BIN_RANKS, n - b * BIN_RANKS)
        at = b * BIN_RANKS + rng.choice(m, count, replace=False)
        out[at] = _small_live(rng, count, tx, ty)
    return out


# ---- the self-test cases ---------------------------------------------------------------------------------------------
GRIDS = ((5, 3, 8), (120, 68, 8), (120, 68, 6), (128, 128, 8), (256, 7, 8), (7, 256, 8), (256, 256, 32))
RANK_COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 4097, 5121, 9217, 20481)


@dataclass(frozen=True)
class BinCase:
    family: str
    grid: tuple                 # (tiles_x, tiles_y, edge)
    n: int
    blocks: tuple = ()          # workgroup counts to launch with, besides ceil(n / BIN_RANKS)
    caps: tuple = ()            # list capacities besides n: an int, or "longest-1"

    @property
    def name(self) -> str:
        return f"{self.family}_{self.grid[0]}x{self.grid[1]}e{self.grid[2]}_n{self.n}"

    @property
    def num_blocks(self) -> int:
        return -(-self.n // BIN_RANKS)

    @property
    def num_st(self) -> int:
        sup_x, sup_y = grid_supertiles(*self.grid)
        return sup_x * sup_y


def _all_bin_cases() -> list:
    cases = []
    for grid in GRIDS:
        for family in ("small", "wide", "mixed", "boundary"):
            extra = {}
            if family == "mixed" and grid == (120, 68, 6):
                extra = dict(blocks=(1, 3))              # the ticket loop: several tiles per workgroup
            if family == "mixed" and grid in ((120, 68, 8), (128, 128, 8)):
                extra = dict(caps=(64, "longest-1"))     # lists that overflow
            cases.append(BinCase(family, grid, 9217, **extra))
    for n in RANK_COUNTS:
        if n != 9217:
            cases.append(BinCase("mixed", (120, 68, 8), n))
    cases.append(BinCase("mixed", (120, 68, 6), 20481, blocks=(1, 3)))
    cases.append(BinCase("full", (128, 128, 8), 5121))
    cases.append(BinCase("threshold", (5, 3, 8), 2 * BIN_RANKS + 700))
    return cases


BIN_CASES = _all_bin_cases()
BIN_CASE_NAMES = [c.name for c in BIN_CASES]
assert len(set(BIN_CASE_NAMES)) == len(BIN_CASE_NAMES)


def bin_case(name: str) -> BinCase:
    return BIN_CASES[BIN_CASE_NAMES.index(name)]


_built: dict = {}


def built(case: BinCase) -> dict:
    """The case's rectangles and their reference lists, once: {rects, lists, lengths, hits}. Left unchanged by its users."""
    if case.name not in _built:
        tx, ty, edge = case.grid
        rng = np.random.default_rng(1_000_003 * case.n + 7919 * tx + 104_729 * ty + 31 * edge + sum(map(ord, case.family)))
        rects = {"small": lambda: _small(rng, case.n, tx, ty), "wide": lambda: _wide(rng, case.n, tx, ty),
                 "full": lambda: _full(case.n, tx, ty), "mixed": lambda: _mixed(rng, case.n, tx, ty),
                 "boundary": lambda: _boundary(rng, case.n, tx, ty, edge), "threshold": lambda: _threshold(rng, tx, ty)}[case.family]()
        assert rects.dtype == np.uint32 and len(rects) == case.n
        lists = reference_lists(rects, tx, ty, edge)
        rects.setflags(write=False)
        _built[case.name] = dict(rects=rects, lists=lists, lengths=np.array([len(l) for l in lists], np.int64), hits=block_hits(lists, case.n))
    return _built[case.name]


def capacities(case: BinCase) -> list:
    longest = int(built(case)["lengths"].max())
    return [case.n] + [longest - 1 if c == "longest-1" else c for c in case.caps]


def expected_buffer(lists, cap: int) -> np.ndarray:
    """uint32 [supertiles, cap, 2]: what bgs_selftest_bin's list buffer must hold — the first min(len, cap) entries of
    every list, the fill everywhere else."""
    out = np.full((len(lists), cap, 2), FILL, np.uint32)
    for s, l in enumerate(lists):
        out[s, :min(len(l), cap)] = l[:cap]
    return out


# ---- the frame cases -------------------------------------------------------------------------------------------------
VERTEX_STAGE_FRAME_CASES = ("ranks_1", "ranks_255", "ranks_256", "ranks_257", "ranks_3000", "target_37x21", "target_4096x64",
                            "global_scale_0p05", "edge_borders_250x130")


def _screen_frame(n, seed, **settings):
    def build():
        v = View.headless(250, 130)
        c = VC.screen_cloud(v, n, seed)
        mn, mx = compute_aabb(c)
        base = dict(sort_mode=SortMode.Rayon, color_space=VC.LIN, position_min=mn, position_max=mx)
        base.update(settings)
        return c, v, CloudSettings(**base)
    return build


# SortMode::Rayon keeps every splat in the draw list: 12 bin_kernel blocks / 47 project_emit_kernel blocks; global_scale 4:
# tens of tiles per splat, thousands of instances per 256-rank block
NEW_FRAME_CASES = (VC.Case("bin_12000_250x130", _screen_frame(12_000, 301), populated=False, rank_count=12_000, tags=("bin",)),
                   VC.Case("bin_3000_global_scale_4", _screen_frame(3000, 302, global_scale=4.0), populated=False, rank_count=3000, tags=("bin",)))
FRAME_CASE_NAMES = VERTEX_STAGE_FRAME_CASES + tuple(c.name for c in NEW_FRAME_CASES)


def frame_case(name: str) -> VC.Case:
    for c in NEW_FRAME_CASES:
        if c.name == name:
            return c
    return VC.by_name(name)


def _left_third():
    """A cloud confined to the left third of the 250 x 130 target (NDC x in [-0.95, -0.4], far and small: no quad reaches
    the right half)."""
    v = View.headless(250, 130)
    c = VC.screen_cloud(v, 1500, 312, spread=1.0)
    rng = np.random.default_rng(313)
    inv = np.linalg.inv(np.asarray(v.clip_from_world, np.float64))
    near = float(np.asarray(v.clip_from_view, np.float64)[2, 3])
    n = len(c)
    dist = rng.uniform(20.0, 40.0, n)
    ndc = np.stack([rng.uniform(-0.95, -0.4, n), rng.uniform(-0.9, 0.9, n)], axis=1)
    clip = np.stack([ndc[:, 0] * dist, ndc[:, 1] * dist, np.full(n, near), dist], axis=1)
    w = clip @ inv.T
    c.position_visibility[:, :3] = (w[:, :3] / w[:, 3:4]).astype(np.float32)
    c.scale_opacity[:, :3] = np.minimum(c.scale_opacity[:, :3], np.float32(0.3))
    return c, v, CloudSettings(sort_mode=SortMode.Rayon, color_space=VC.LIN)


# the stale-range sequence (BINNING_SORT, one context): a cloud over the whole target, then one over its left third
STALE_FULL = VC.Case("bin_stale_full_screen", _screen_frame(1500, 311), populated=False, tags=("bin",))
STALE_LEFT = VC.Case("bin_stale_left_third", _left_third, populated=False, tags=("bin",))
