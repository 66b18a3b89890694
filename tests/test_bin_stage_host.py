"""The cases of tests/bin_stage_cases.py hold what they are named for, and its references agree with independent
restatements. CPU only; the device side is tests/test_bin_stage_gpu.py."""
import os
import re

import numpy as np
import pytest

import bin_stage_cases as B
import helpers as H
import vertex_stage_cases as VC

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "bevy_gaussian_splatting_amd", "csrc")


def _src(*path):
    return open(os.path.join(*path)).read()


def test_the_cases_are_sized_for_the_kernels_constants():
    """BIN_RANKS, BGS_BIN_LOOKBACK, MAX_SUPERTILES, RECT_EMPTY and the self-test's guard as the sources state them: the rank
    counts (blocks of 1024; block 5 the first with a second look-back hop, block 9 with a third), the 32 * num_st
    threshold family and the grids were sized for these values. If one changes, re-size the cases."""
    kernels, device, diag = _src(CSRC, "render_kernels.hip"), _src(CSRC, "bgs_device.h"), _src(ROOT, "include", "bgs_diag.h")
    groups = int(re.search(r"constexpr uint32_t BIN_GROUPS = (\d+)u, BIN_RANKS = 64u \* BIN_GROUPS;", kernels).group(1))
    assert 64 * groups == B.BIN_RANKS == 1024
    assert int(re.search(r"#define BGS_BIN_LOOKBACK (\d+)", kernels).group(1)) == B.BIN_LOOKBACK == 4
    assert "lookback_u32<BGS_BIN_LOOKBACK>(bin_status + tid, tile, MAX_SUPERTILES" in kernels
    assert "if (s_block_hits >= 32u * num_st) {" in kernels
    assert int(re.search(r"constexpr uint32_t MAX_SUPERTILES = (\d+);", device).group(1)) == B.MAX_SUPERTILES == 256
    assert int(re.search(r"constexpr uint32_t MAX_SUPERTILES_PER_AXIS = (\d+);", device).group(1)) == 32
    assert int(re.search(r"constexpr uint32_t RECT_EMPTY = (0x[0-9A-Fa-f]+)u;", device).group(1), 16) == B.RECT_EMPTY == H.RECT_EMPTY
    assert int(re.search(r"#define BGS_SELFTEST_BIN_GUARD (\d+)u", diag).group(1)) == B.GUARD
    from bevy_gaussian_splatting_amd import _native
    assert _native.SELFTEST_BIN_GUARD == B.GUARD
    # blocks of BIN_RANKS the rank counts give, and the look-back hops their last block needs (BIN_LOOKBACK words per hop)
    blocks = sorted({-(-n // B.BIN_RANKS) for n in B.RANK_COUNTS})
    assert blocks == [1, 2, 5, 6, 10, 21]
    hops = lambda block: -(-block // B.BIN_LOOKBACK)     # block b looks back over b predecessors
    assert [hops(b) for b in (4, 5, 8, 9)] == [1, 2, 2, 3]
    assert B.BIN_CASES and all(c.n >= 1 for c in B.BIN_CASES)


def test_the_asked_combinations_are_all_there():
    have = {(c.family, c.grid, c.n) for c in B.BIN_CASES}
    for grid in B.GRIDS:
        for family in ("small", "wide", "mixed", "boundary"):
            assert (family, grid, 9217) in have
    for n in B.RANK_COUNTS:
        assert ("mixed", (120, 68, 8), n) in have
    assert ("full", (128, 128, 8), 5121) in have and any(c.family == "threshold" and c.grid == (5, 3, 8) for c in B.BIN_CASES)
    for n in (9217, 20481):
        c = B.bin_case(f"mixed_120x68e6_n{n}")
        assert c.blocks == (1, 3) and c.num_blocks > 3
    assert [grid for grid in B.GRIDS if B.grid_supertiles(*grid) == (1, 1)] == [(5, 3, 8)]
    assert {B.grid_supertiles(*g) for g in B.GRIDS} == {(1, 1), (15, 9), (20, 12), (16, 16), (32, 1), (1, 32), (8, 8)}
    overflowing = [c for c in B.BIN_CASES if c.caps]
    assert len(overflowing) == 2 and all(c.family == "mixed" and c.caps == (64, "longest-1") for c in overflowing)
    for c in overflowing:
        caps = B.capacities(c)
        lengths = B.built(c)["lengths"]
        assert caps[0] == c.n and caps[1] == 64 and caps[2] == lengths.max() - 1
        assert (lengths > 64).any() and 1 <= (lengths > caps[2]).sum() < len(lengths)   # cap 64: lists overflow; longest - 1: few do


@pytest.mark.parametrize("name", B.BIN_CASE_NAMES)
def test_case_holds_what_it_is_named_for(name):
    case = B.bin_case(name)
    tx, ty, edge = case.grid
    d = B.built(case)
    rects, lists, hits = d["rects"], d["lists"], d["hits"]
    x0, x1, y0, y1 = B.unpack(rects)
    live = rects != B.RECT_EMPTY
    assert (x0 <= x1)[live].all() and (y0 <= y1)[live].all() and (x1 < tx)[live].all() and (y1 < ty)[live].all()
    assert case.num_st <= B.MAX_SUPERTILES and max(B.grid_supertiles(*case.grid)) <= 32 and edge <= 32 and max(tx, ty) <= 256
    # every list is ascending in rank and carries the rank's own rectangle
    for l in lists:
        assert (np.diff(l[:, 0].astype(np.int64)) > 0).all() and np.array_equal(l[:, 1], rects[l[:, 0]])
    assert d["lengths"].max() <= case.n
    assert hits.shape == (case.num_blocks, case.num_st) and hits.max() <= B.BIN_RANKS       # bin_kernel's uint16 offsets hold
    assert hits.sum() == d["lengths"].sum()
    if case.n <= 1025:
        brute = B.brute_force_lists(rects, tx, ty, edge)
        assert len(brute) == len(lists) and all(np.array_equal(a, b) for a, b in zip(brute, lists))
    # which append path each block takes: bin_kernel compares the block's entries with 32 * num_st
    total, threshold = hits.sum(axis=1), 32 * case.num_st
    complete = np.arange(case.num_blocks) < case.n // B.BIN_RANKS      # (the last block of 9217 / 5121 ranks holds one rank)
    if case.family == "small" and case.num_st > 1:
        assert (total < threshold).all() and (total[complete] > 0).all()
    if case.family in ("wide", "full"):
        # every block of 1024 ranks; the one-rank tail block cannot reach 32 entries per supertile and walks the bits
        assert (total[complete] >= threshold).all() and complete.sum() == case.num_blocks - 1 and 0 < total[~complete].sum() < threshold
    if case.family == "full":
        assert all(np.array_equal(l[:, 0], np.arange(case.n)) for l in lists)
    if case.family == "mixed" and case.num_blocks >= 3:
        assert (total >= threshold).any() and ((total > 0) & (total < threshold)).any() and (total == 0).any()
        zero = np.nonzero(total == 0)[0]
        assert zero.min() > 0 and (zero.max() < case.num_blocks - 1 or case.num_blocks % 3 == 0)   # a zero block INSIDE the chains
        if case.num_st > 1:     # neighbouring blocks on different paths: small (bit-walk), wide (wave-wide), empty, ...
            kinds = np.where(total == 0, 0, np.where(total < threshold, 1, 2))[complete]
            assert np.array_equal(kinds, np.array([1, 2, 0] * case.num_blocks)[:complete.sum()])
    if case.family == "boundary":
        xs, ys = set(B._border_coords(tx, edge)), set(B._border_coords(ty, edge))
        assert live.all() and set(x0) | set(x1) <= xs | {v + 1 for v in xs} and set(y0) <= ys
        if case.num_st > 1:     # rectangles that end on, start on and straddle a supertile border, on an axis that has one
            axes = [(x0, x1, tx)] * (tx > edge) + [(y0, y1, ty)] * (ty > edge)
            for lo, hi, tiles in axes:
                assert ((hi % edge == edge - 1) & (hi < tiles - 1)).any() and ((lo % edge == 0) & (lo > 0)).any()
                assert ((lo // edge) < (hi // edge)).any() and (lo == 0).any() and (hi == tiles - 1).any()
    if case.family == "threshold":
        assert case.num_st == 1 and tuple(total) == B.THRESHOLD_COUNTS == (31, 32, 33) and threshold == 32


def test_supertile_edge_restatement_on_the_frame_grids():
    # (tiles, level) -> edge, by hand from frame_params.h: 1080p's 120 x 68 tiles are 6 / 8 / 16 / 32
    assert [B.supertile_edge(120, 68, lv) for lv in range(4)] == [(6, 0), (8, 1), (16, 2), (32, 3)]
    assert [B.supertile_edge(16, 9, lv) for lv in (0, 1, 3)] == [(6, 0), (8, 1), (32, 3)]           # 250 x 130
    assert [B.supertile_edge(256, 4, lv) for lv in (0, 1, 3)] == [(8, 0), (8, 1), (32, 3)]          # 4096 x 64: 6 and 7 leave > 32 bins on x
    assert [B.supertile_edge(256, 256, lv) for lv in range(4)] == [(16, 0), (16, 1), (32, 2), (32, 2)]   # levels 2 and 3 are one level


FRAME_NAMES = B.FRAME_CASE_NAMES + (B.STALE_FULL.name, B.STALE_LEFT.name)


def _frame_case(name):
    return {B.STALE_FULL.name: B.STALE_FULL, B.STALE_LEFT.name: B.STALE_LEFT}.get(name) or B.frame_case(name)


@pytest.mark.parametrize("name", FRAME_NAMES)
def test_reference_instances_agree_with_the_twin(name):
    d = VC.twin_of(_frame_case(name))
    rects = d["rects"]
    inst, ranges, present = B.reference_instances(rects)
    assert len(inst) == H.twin_instances(d["twin"])
    key, rank = inst[:, 0].astype(np.int64), inst[:, 1].astype(np.int64)
    assert (np.diff(key * (1 << 32) + rank) > 0).all()                        # sorted by (key, rank), no instance twice
    x0, x1, y0, y1 = B.unpack(rects[rank])
    assert ((x0 <= (key & 255)) & ((key & 255) <= x1) & (y0 <= (key >> 8)) & ((key >> 8) <= y1)).all()
    assert present.sum() == len(np.unique(key)) and (ranges[present, 1] - ranges[present, 0]).sum() == len(inst)
    assert (ranges[~present] == 0).all()
    for k in np.unique(key)[:50]:
        assert (key[ranges[k, 0]:ranges[k, 1]] == k).all()
    if len(rects) <= 300:      # brute force
        want = sorted((ty << 8 | tx, j) for j, r in enumerate(int(v) for v in rects) if r != B.RECT_EMPTY
                      for ty in range((r >> 16) & 255, (r >> 24) + 1) for tx in range(r & 255, ((r >> 8) & 255) + 1))
        assert [tuple(int(v) for v in row) for row in inst] == want


def test_the_new_frame_cases_reach_what_they_are_for():
    big = VC.twin_of(B.frame_case("bin_12000_250x130"))
    assert big["twin"]["count"] == 12_000 > 4 * B.BIN_RANKS and 12_000 > 40 * 256         # > 4 bin blocks, > 40 emit blocks
    lists = B.reference_lists(big["rects"], 16, 9, 8)
    assert B.block_hits(lists, 12_000).sum(axis=1).min() > 0
    fat = VC.twin_of(B.frame_case("bin_3000_global_scale_4"))
    x0, x1, y0, y1 = B.unpack(fat["rects"])
    area = np.where(fat["rects"] != B.RECT_EMPTY, (x1 - x0 + 1) * (y1 - y0 + 1), 0)
    per_block = np.add.reduceat(area, np.arange(0, len(area), 256))
    print("instances per 256-rank block:", per_block.tolist())
    assert fat["twin"]["count"] == 3000 and np.median(per_block) > 8 * 256 and per_block.max() > 16 * 256
    # the stale-range sequence: the second frame leaves tiles the first one covered
    _, _, full = B.reference_instances(VC.twin_of(B.STALE_FULL)["rects"])
    _, _, left = B.reference_instances(VC.twin_of(B.STALE_LEFT)["rects"])
    assert (full & ~left).sum() >= 60 and left.sum() >= 20 and not left[np.arange(65536) & 255 >= 8].any()
