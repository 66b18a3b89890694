"""The tile-instance budget cases (tests/instance_budget_cases.py) hold what they are named for, on the host twin: exact
totals, whole-target cover rectangles, finite inputs, draw counts, and covers opaque enough that every pixel saturates
within a few records. No GPU."""
import numpy as np
import pytest

import instance_budget_cases as I


@pytest.mark.parametrize("name", I.CASE_NAMES)
def test_the_case_holds_what_it_is_named_for(name):
    d = I.built(name)
    case, cloud, twin = d["case"], d["cloud"], d["twin"]
    tx, ty = case.tiles
    for plane in (cloud.position_visibility, cloud.spherical_harmonic, cloud.rotation, cloud.scale_opacity):
        assert np.isfinite(plane).all()
    assert len(cloud) == case.covers + case.dots
    # every splat is kept by the frustum cull, visible and drawn
    assert len(d["draw"]) == len(cloud) and twin["visible"].all() and twin["draw"].all() and d["drawn"].all()
    is_cover = d["draw"]["index"] < case.covers
    assert int(is_cover.sum()) == case.covers
    whole = np.array([0, tx - 1, 0, ty - 1])
    bad = np.nonzero((twin["rect"][is_cover] != whole).any(axis=1))[0]
    assert not len(bad), f"{name}: cover {bad[0]} has the rectangle {twin['rect'][is_cover][bad[0]].tolist()}"
    dots = twin["rect"][~is_cover]
    areas = (dots[:, 1] - dots[:, 0] + 1) * (dots[:, 3] - dots[:, 2] + 1)
    assert (areas == 1).all(), f"{name}: dots of {areas.tolist()} tiles"
    assert d["total"] == case.total == case.covers * tx * ty + case.dots, f"{name}: the twin counts {d['total']} instances"
    floor = I.cover_alpha_floor(d)
    print(f"{name}: {d['total']} instances of {len(cloud)} splats on {tx} x {ty} tiles, lowest cover alpha at a pixel centre {floor.min():.4f}")
    assert len(floor) == case.covers and floor.min() >= I.ALPHA_FLOOR
    # the dots are in front of every cover: the last entries of the draw list (drawn on top), the first ranks
    if case.dots:
        assert not is_cover[-case.dots:].any()


def test_the_totals_sit_on_the_edges_they_are_named_for():
    total = {c.name: c.total for c in I.CASES}
    assert (by := I.by_name)("at_capacity").tiles == (16, 16) and by("refused_2pow30").tiles == (256, 256)
    assert total["at_capacity"] == I.MIN_CAPACITY                         # `total > capacity` is false by one
    assert total["one_over"] - I.MIN_CAPACITY == 1                        # the excess the twin allows: a one-tile dot
    assert I.capacity_for(total["one_over"]) == 1 << 23
    assert 1 << 23 < total["second_growth"] <= (1 << 23) * 5 // 4 and I.capacity_for(total["second_growth"]) == 1 << 24
    # fits 2^23 as it is, and not with a quarter of head-room
    assert total["head_room"] <= 1 << 23 < total["head_room"] + total["head_room"] // 4 and I.capacity_for(total["head_room"]) == 1 << 24
    assert total["refused_2pow30"] == I.MAX_CAPACITY + 65536 and I.capacity_for(total["refused_2pow30"]) is None
    assert total["carry_2pow32"] >> 32 == 1 and total["carry_2pow32"] & 0xFFFFFFFF == 65536
    assert I.capacity_for(total["carry_2pow32"]) is None
    # a count whose low word alone would pass for a frame that fits: the refusal needs the high word
    assert (total["carry_2pow32"] & 0xFFFFFFFF) <= I.MIN_CAPACITY


@pytest.mark.parametrize("name", ("at_capacity", "one_over"))
def test_the_reference_expansion_has_the_twin_s_total(name):
    d = I.built(name)
    inst, ranges, present = I.reference(name)
    tx, ty = d["case"].tiles
    assert len(inst) == d["total"]
    assert int(present.sum()) == tx * ty and int((ranges[:, 1] - ranges[:, 0]).sum()) == d["total"]
    per_tile = (ranges[:, 1] - ranges[:, 0])[present]
    assert per_tile.min() == d["case"].covers and per_tile.max() == d["case"].covers + (1 if d["case"].dots else 0)
    # within a tile the ranks ascend: front to back
    same = inst[1:, 0] == inst[:-1, 0]
    assert (inst[1:, 1][same] > inst[:-1, 1][same]).all()


def test_a_yawed_view_keeps_the_totals():
    """The two-lane frames turn the camera a little: the covers still span the target, the dot moves with the view."""
    for yaw in (0.0, 0.01):
        d = I.built("one_over", yaw)
        assert d["twin"]["draw"].all() and d["total"] >= I.MIN_CAPACITY + 1
        assert I.capacity_for(d["total"]) == 1 << 23
