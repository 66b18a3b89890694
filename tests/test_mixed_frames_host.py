"""The kinds and the schedule of tests/mixed_frame_cases.py, without a GPU: what tests/test_mixed_frames_in_flight_gpu.py
relies on is asserted here as a condition. A schedule that skips a pair of kinds, a same-lane pair or an event placement
fails here, so the GPU test cannot pass on one."""
import itertools

import numpy as np
import pytest

import mixed_frame_cases as M
from bevy_gaussian_splatting_amd import RasterizeMode
from bevy_gaussian_splatting_amd.settings import SortMode


def missing(steps, depth):
    """What a schedule lacks: (adjacent pairs, same-lane pairs, event placements)."""
    have, want = M.coverage(steps, depth), M.required(depth)
    return tuple(sorted(w - h) for h, w in zip(have, want))


CASES = [(d, s) for d in M.DEPTHS for s in M.SEEDS]


@pytest.mark.parametrize("depth,seed", CASES)
def test_the_schedule_holds_every_pair_and_every_event_placement(depth, seed):
    steps = M.schedule(depth, seed)
    adjacent, same_lane, placed = missing(steps, depth)
    assert not adjacent, f"depth {depth}: no two frames in a row for {adjacent[:5]} ({len(adjacent)} pairs)"
    assert not same_lane, f"depth {depth}: no two frames in a row on one lane for {same_lane[:5]} ({len(same_lane)} pairs)"
    assert not placed, f"depth {depth}: no such event directly before a frame of that binning: {placed}"
    frames = [s for s in steps if s[0] == "frame"]
    events = [s for s in steps if s[0] != "frame"]
    for name in M.EVENTS:
        assert sum(1 for e in events if e[0] == name) >= 2, name
    assert steps[0][0] == "frame" and steps[-1][0] == "frame", "an event runs between frames"
    assert set(s[0] for s in events) == set(M.EVENTS) and all(f[1] in M.KIND_NAMES for f in frames)
    assert 144 <= len(frames) <= 1000, len(frames)
    M._schedules.pop((depth, seed))
    assert M.schedule(depth, seed) == steps, "the schedule is a function of the depth and the seed"


@pytest.mark.parametrize("depth,seed", CASES)
def test_the_particle_steps_come_in_pairs_and_no_upload_undoes_one(depth, seed):
    steps = M.schedule(depth, seed)
    stepped = False
    for s in steps:
        if s[0] == "particle_step":
            assert s[1] == (-M.STEP_DT if stepped else M.STEP_DT)
            stepped = not stepped
        if s[0] == "reupload":
            assert s[1] in M.CLOUDS and not (stepped and s[1] == M.STEP_CLOUD)
        if s[0] == "sort":
            assert s[1] in M.KIND_NAMES
    assert not stepped, "the schedule ends on the stepped cloud"
    frames = M.walk(steps, depth)
    between = [f for f in frames if f.stepped]
    assert any(M.by_name(f.kind).cloud == M.STEP_CLOUD for f in between), "no frame of the stepped cloud between the step and its inverse"
    assert any(f.rerun and not M.is_sort(f.kind) for f in frames), "no BINNING_SCAN frame is re-run"


@pytest.mark.parametrize("depth", M.DEPTHS)
def test_a_schedule_that_lost_a_pair_or_an_event_is_found_out(depth):
    steps = list(M.schedule(depth, M.SEEDS[0]))
    frames = M.walk(steps, depth)
    # an adjacent pair: its second frame becomes another kind, wherever it occurs
    a, b = next((f.kind, g.kind) for f, g in zip(frames, frames[1:]) if f.kind != g.kind)
    other = next(k for k in M.KIND_NAMES if k not in (a, b))
    swapped = list(steps)
    for f, g in zip(frames, frames[1:]):
        if (f.kind, g.kind) == (a, b):
            swapped[g.step] = ("frame", other)
    assert (a, b) in missing(swapped, depth)[0]
    # a same-lane pair: its second frame becomes another kind, wherever it occurs
    f = next(f for f in frames if f.lane_prev is not None and not M.barrier(f.events))
    pair = (f.lane_prev.kind, f.kind)
    other = next(k for k in M.KIND_NAMES if k not in pair and M.is_sort(k) == M.is_sort(f.kind))
    swapped = list(steps)
    for g in frames:
        if g.lane_prev is not None and (g.lane_prev.kind, g.kind) == pair:
            swapped[g.step] = ("frame", other)
    assert M.walk(swapped, depth)[f.index].lane == f.lane, "a kind of the same binning takes the same lane"
    assert pair in missing(swapped, depth)[1]
    # an event placement: every event goes in turn
    for i, s in enumerate(steps):
        if s[0] != "frame":
            binning = M.by_name(steps[i + 1][1]).binning
            assert (s[0], binning) in missing(steps[:i] + steps[i + 1:], depth)[2], (i, s)


def test_the_lane_rule():
    """run(), csrc/bgs_frame.hip: scan frames go round the ring, BINNING_SORT frames to lane 0 without moving it."""
    scan = [k for k in M.KIND_NAMES if not M.is_sort(k)]
    srt = [k for k in M.KIND_NAMES if M.is_sort(k)]
    rule = M.LaneRule(3)
    assert [rule.place(k) for k in (scan[0], scan[1], srt[0], scan[2], srt[1], srt[0], scan[3], scan[4])] == [0, 1, 0, 2, 0, 0, 0, 1]
    frames = M.walk([("frame", scan[0]), ("frame", scan[1]), ("frame", srt[0]), ("rerun_next",), ("frame", scan[2])], 2)
    assert [f.lane for f in frames] == [0, 1, 0, 0] and frames[2].lane_prev is frames[0] and frames[3].lane_prev is frames[2]
    assert frames[3].rerun and not frames[2].rerun and frames[3].events == (("rerun_next",),)
    # lanes of a deep ring are not i % depth once a BINNING_SORT frame has been drawn
    for depth in M.DEPTHS:
        frames = M.walk(M.schedule(depth, M.SEEDS[0]), depth)
        assert any(f.lane != f.index % depth for f in frames)
        assert {f.lane for f in frames} == set(range(depth))
        assert all(f.lane == 0 for f in frames if M.is_sort(f.kind))


def test_the_kinds_cover_every_axis_value():
    K = M.KINDS
    assert 10 <= len(K) <= 14 and len(set(M.KIND_NAMES)) == len(K)
    assert {k.cloud for k in K} == {"f32", "f16", "cov"} and {k.format for k in K} == {"f32", "f16", "cov3d"}
    assert [M.CLOUDS[c][0] for c in ("f32", "f16", "cov")] == [3000, 9000, 30000]
    assert {k.size for k in K} == {(80, 48), (250, 130), (320, 192), (384, 160)}
    assert M.by_name("cov_dense").tiles == (24, 10) and M.by_name("f16_kept").tiles == (20, 12)   # 240 tiles both
    assert all(k.n <= 30000 and k.size[0] <= 384 and k.size[1] <= 192 for k in K)
    assert {k.binning for k in K} == {"scan", "sort"}
    assert {k.samples for k in K} == {1, 4}
    assert sum(k.depth_buffer for k in K) == 1
    assert {k.shape for k in K} == {"obb", "aabb3d", "surfel"}
    assert any(k.shape == "surfel" and k.samples == 4 for k in K)
    assert {k.sort_mode for k in K} == {SortMode.Radix, SortMode.Rayon} and {k.bits for k in K} == {32, 16}
    assert sum(k.kept for k in K) == 1 and not any(k.kept and k.binning == "sort" for k in K)
    assert {k.outputs for k in K} == {"f32", "srgb8", "f16_only"}
    assert not any(k.outputs == "f16_only" and k.binning == "sort" for k in K), "bgs_set_packed_only is of BINNING_SCAN frames"
    assert sum(k.mode == RasterizeMode.Depth for k in K) == 1 and {k.mode for k in K} == {RasterizeMode.Color, RasterizeMode.Depth}
    dense = {k.scale for k in K if k.cloud == "cov"}
    assert dense == {1.0, 0.05}
    # a precomputed-covariance cloud has no surfels
    assert not any(k.format == "cov3d" and k.shape == "surfel" for k in K)
    for axis in M.AXES:
        assert len({getattr(k, axis) for k in K}) >= 2, axis
    for a, b in itertools.combinations(K, 2):
        differ = [axis for axis in M.AXES if getattr(a, axis) != getattr(b, axis)]
        assert len(differ) >= 2, (a.name, b.name, differ)


def test_no_two_kinds_share_what_a_graph_is_keyed_by():
    keys = [M.graph_tuple(k) for k in M.KINDS]
    assert len(set(keys)) == len(keys)
    # and two scan kinds that could share a lane's graph slot (same graph kind, any parity) differ in more than the cloud
    for a, b in itertools.combinations([k for k in M.KINDS if k.binning == "scan"], 2):
        assert M.graph_tuple(a)[1:] != M.graph_tuple(b)[1:], (a.name, b.name)


def test_the_particle_step_has_an_exact_inverse():
    rec, stepped = M.particle_step()
    pv = M.cloud(M.STEP_CLOUD).position_visibility
    from bevy_gaussian_splatting_amd.particles import step_reference
    back, rec2 = step_reference(stepped, rec.records, -M.STEP_DT)
    assert back.tobytes() == pv.tobytes() and rec2.tobytes() == rec.records.tobytes()
    moved = np.flatnonzero((stepped != pv).any(axis=1))
    assert len(rec) >= 1000 and len(moved) >= 1000, (len(rec), len(moved))
    assert (stepped[:, 3] == pv[:, 3]).all(), "the visibility lane is not moved"
    assert float(np.abs(stepped - pv).max()) > 0.1, "a step too small to show in an 80 x 48 image"
