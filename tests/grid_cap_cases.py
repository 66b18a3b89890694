"""Shapes of tests/test_grid_cap_gpu.py: the smallest at which a persistent kernel's tile loop goes round again under a grid
cap of 1, 2 or 3 workgroups (bgs_set_grid_cap) — at least five tiles of the kernel under test, the last one ragged.

Tile sizes (csrc/bgs_device.h, kernels.h, render_kernels.hip, entries_math.h): keygen 2048 splats (4096 from 2^19), onesweep
2048 pairs (4096 past 4 M pairs, and for the tile-id passes), project 256 ranks, bin 1024 ranks, compaction 2048 entries."""
import numpy as np

import vertex_stage_cases as VC
from bevy_gaussian_splatting_amd import RasterizeMode, SortMode

CAPS = (1, 2, 3)
SMALL_TILE, LARGE_TILE, KEYGEN_TILE, ENTRIES_TILE = 2048, 4096, 2048, 2048
PAIR_SIZES = (5 * SMALL_TILE + 1, 9 * SMALL_TILE - 1)
LARGE_PAIRS = (4 << 20) + 4097            # past the 4096-pair switch: 1026 tiles, the last of 1 pair
SORT_SIZES = (5 * KEYGEN_TILE + 1, 20_000)
BIG_SORT = (1 << 19) + 4097               # 4096-splat keygen tiles: 130 of them, the last of 1 splat

NO_BUCKET_SORT, NO_DRAW_HINT, SMALL_LISTS, RERUN_EVERY_FRAME = 0x80000, 0x2000, 0x100000, 0x8000000   # include/bgs_diag.h


def key_families(n, passes, seed):
    """The families of test_onesweep_kernel_on_arbitrary_keys: random with many ties, seven values, all equal, sorted, reversed."""
    rng = np.random.default_rng(seed)
    mask = np.uint32((1 << (8 * passes)) - 1) if passes < 4 else np.uint32(0xFFFFFFFF)
    return {"random with ties": (rng.integers(0, 1 << 12, size=n, dtype=np.uint64).astype(np.uint32) * np.uint32(0x00100401)) & mask,
            "seven values": (rng.integers(0, 7, size=n, dtype=np.uint64).astype(np.uint32) * np.uint32(0x01010101)) & mask,
            "all equal": np.full(n, 0x00ABCDEF, np.uint32) & mask,
            "sorted": (np.arange(n, dtype=np.uint32) * np.uint32(3)) & mask,
            "reversed": np.arange(n, dtype=np.uint32)[::-1].copy() & mask}


# Vertex stage: vertex_stage_cases' builders grown to 3000 splats (about 1900 drawn ranks; 12 tiles of 256 ranks, the last of
# 184): one per cloud format, one surfel, one ANY_MODE, one kept order.
VERTEX_CASES = (
    VC.Case("cap_f32_obb", VC._basic(3000, 401), tags=("grid_cap",)),
    VC.Case("cap_f16_surfel", VC._basic(3000, 402, fmt="f16", **VC._shape("surfel")), fmt="f16", tags=("grid_cap",)),
    VC.Case("cap_cov3d_aabb_any", VC._basic(3000, 403, fmt="cov3d", rasterize_mode=RasterizeMode.Classification, **VC._shape("aabb")), fmt="cov3d",
            tags=("grid_cap",)),
    VC.Case("cap_kept_order", VC._basic(3000, 404, sort_mode=SortMode.Radix), kept=VC._kept_chunk, tags=("grid_cap",)),
)
VERTEX_CASE_NAMES = tuple(c.name for c in VERTEX_CASES)
MIN_DRAWN = 1500


def vertex_case(name):
    return VERTEX_CASES[VERTEX_CASE_NAMES.index(name)]


def looped(grids, kernel):
    """The condition every test asserts before it compares: some workgroup of `kernel` took at least two tiles."""
    blocks, tiles = grids[kernel]
    return 0 < blocks < tiles
