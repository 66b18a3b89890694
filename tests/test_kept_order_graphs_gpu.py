"""Kept-order frames (bgs_view.entries_device_ptr) replayed from captured frame graphs (bgs_set_graphs): a lane holds a
graph per KIND of frame (sorting, kept order) and Control parity; the kept kind's first node is the compaction of
csrc/entries_kernels.hip, and a replay sets that node's arguments: the frame's parameters AND the chunk's device address.

Every frame here is compared BITWISE with its direct twin: the same frame launched directly (bgs_set_graphs(0), or
BGS_DEBUG_NO_GRAPHS), rendered first. Conventions (fixture, same_bits, what is restored) as in test_kept_order_gpu.py.

The capture rule the counts below are derived from (enqueue_frame, csrc/bgs_frame.hip). An async BINNING_SCAN frame
without profiling events goes through a graph unless the lane's scratch is not known to be clean (the lane's first frame,
the frame after a bgs_sort on the lane, after a buffer grew: a memset and a direct launch). A graph frame REPLAYS when the
lane's graph of its (kind, parity) has the frame's key, else it CAPTURES; the lane's parity flips with every frame. The
key holds nothing that differs between frames of one cloud, viewport size and settings once the context's hints (draw
count, list capacity, supertile level) have been raised by a completed frame of the largest draw count, which the direct
twins are: the hints rise at once and fall only after 64 frames."""
import os

import numpy as np
import pytest

from bevy_gaussian_splatting_amd import (
    CloudSettings, PlanarGaussian3d, View, random_gaussians_3d_seeded, random_particle_behaviors, step_reference)
from bevy_gaussian_splatting_amd.plugin import SORT_ENTRY_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 5000
W = HT = 128
CULLED = 0xFFFFFFFF
NO_GRAPHS = 0x4000            # BGS_DEBUG_NO_GRAPHS (include/bgs_diag.h)
RERUN_EVERY_FRAME = 0x8000000  # BGS_DEBUG_RERUN_EVERY_FRAME
_CLOUD = None


def base_cloud() -> PlanarGaussian3d:
    global _CLOUD
    if _CLOUD is None:
        _CLOUD = random_gaussians_3d_seeded(N, 21)
        _CLOUD.position_visibility.setflags(write=False)
    return _CLOUD


def view(yaw=0.0, size=W):
    return View.headless(size, size, yaw=yaw, msaa_samples=4)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def restore(plugin):
    plugin.set_async(False)
    plugin.set_graphs(False)
    plugin.set_debug_flags(0)
    plugin.set_profiling(2)
    plugin.set_pipeline_depth(1)
    plugin.set_binning("scan")


@pytest.fixture()
def scene(plugin):
    """The 5000-splat cloud resident, two chunks of device entries; async frames on one lane, graphs off, no profiling
    events. Everything released and restored after."""
    restore(plugin)
    plugin.reset_adaptive_state()
    h = plugin.upload(base_cloud())
    dse = plugin.device_sorted_entries(2, h)
    plugin.set_profiling(0)
    plugin.set_async(True)
    yield h, dse
    restore(plugin)
    dse.free()
    h.free()


def frame(plugin, h, v, s, chunk=None, size=W):
    """One async frame, completed and downloaded: (image, captures it took, replays it took)."""
    c0, r0 = plugin.graph_counters()
    plugin.render(h, v, s, download=False, entries=chunk)
    c1, r1 = plugin.graph_counters()
    ptr, _ = plugin.pipeline_pop()
    return plugin.download(ptr, np.empty((size, size, 4), np.float32)), c1 - c0, r1 - r0


def direct(plugin, h, v, s, chunk=None, size=W):
    """The same frame launched directly: graphs off (the caller switches them on afterwards). Three times over, so that
    the hints are where frames of this kind leave them: the supertile level moves one step per completed frame, and
    there are four levels."""
    plugin.set_graphs(False)
    imgs = []
    for _ in range(3):
        img, c, r = frame(plugin, h, v, s, chunk, size)
        assert (c, r) == (0, 0)
        imgs.append(img)
    assert same_bits(imgs[0], imgs[1]) and same_bits(imgs[1], imgs[2])
    return imgs[2]


# ---- 1. replays happen (the test that fails without the kept kind of graph) ---------------------------------------------------
@pytest.mark.gpu
def test_kept_frames_are_captured_and_replayed(plugin, scene):
    """Six kept frames of one view on one lane: the direct twin left the scratch clean, so the first two capture (one per
    parity) and the other four replay. (The plugin is the session's: a cloud of this length uploaded to the same
    addresses by an earlier test may have left graphs that still fit, in which case fewer frames capture.)"""
    h, dse = scene
    v, s = view(0.2), CloudSettings()
    plugin.sort(h, v, s, download=False, into=dse.chunk(0))
    want = direct(plugin, h, v, s, dse.chunk(0))
    assert np.abs(want[..., :3]).max() > 0.05   # (not an empty frame)
    plugin.set_graphs(True)
    c0, r0 = plugin.graph_counters()
    for f in range(6):
        got, _, _ = frame(plugin, h, v, s, dse.chunk(0))
        assert same_bits(got, want), f
    c1, r1 = plugin.graph_counters()
    print(f"[kept graphs] captures +{c1 - c0}, replays +{r1 - r0}")
    assert c1 - c0 >= 1 and r1 - r0 >= 1
    assert c1 - c0 <= 2 and (c1 - c0) + (r1 - r0) == 6   # every frame through a graph, a capture per parity at most
    st = plugin.stats()
    assert st["sort_path"] == "kept" and st["depth_passes"] == 0 and st["frames_averaged"] == 0
    assert all(ms == 0.0 for ms in st["stage_ms"].values())   # (no stage events under a graph)


# ---- 2. the chunk address is an argument, not captured state ----------------------------------------------------------------------
@pytest.mark.gpu
def test_the_chunk_address_is_a_node_argument(plugin, scene):
    """chunk(0) is sorted for view A, chunk(1) for view B. (a) A / B in turn for 8 frames: the lane's two parities capture
    at most once each, in the first two frames, and never after. (b) pairs, A A B B A A B B: now EACH parity's graph is
    handed both chunks in turn, so a chunk address frozen at capture would draw the other camera's order; no capture at
    all. (c) view B from chunk(1) and from the STALE chunk(0) in pairs: the view is the same, the chunk alone differs."""
    h, dse = scene
    s = CloudSettings()
    a, b = view(0.0), view(0.65)
    plugin.sort(h, a, s, download=False, into=dse.chunk(0))
    plugin.sort(h, b, s, download=False, into=dse.chunk(1))
    want_a, want_b = direct(plugin, h, a, s, dse.chunk(0)), direct(plugin, h, b, s, dse.chunk(1))
    want_stale = direct(plugin, h, b, s, dse.chunk(0))
    assert not same_bits(want_a, want_b) and not same_bits(want_b, want_stale)
    cases = {"a": (a, dse.chunk(0), want_a), "b": (b, dse.chunk(1), want_b), "stale": (b, dse.chunk(0), want_stale)}
    plugin.set_graphs(True)

    def run(order):
        captures = []
        for f, name in enumerate(order):
            v, chunk, want = cases[name]
            got, c, r = frame(plugin, h, v, s, chunk)
            assert same_bits(got, want), (order, f, name)
            assert c + r == 1, (order, f, name)   # every one of them went through a graph
            captures.append(c)
        return captures

    caps = run(["a", "b"] * 4)
    assert sum(caps[2:]) == 0, caps
    assert sum(run(["a", "a", "b", "b"] * 2)) == 0
    assert sum(run(["b", "b", "stale", "stale"] * 2)) == 0


# ---- 3. kept and sorting frames in turn, four in flight -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_kept_and_sorting_frames_alternate_on_four_lanes(plugin, scene):
    """Depth 4, frame f on lane f % 4, kept when f is even: a lane sees ONE kind. 12 warm-up frames, three per lane: at
    worst (a lane never used, or whose scratch a buffer outgrew) one direct frame and one capture per parity. The 12
    frames counted after them are three per lane again, on a clean scratch, with both parities' graphs of the lane's kind
    captured and the hints settled by the direct twins: every one is a replay. Lower bound: replays >= 12 - captures,
    with captures == 0, so 12: six of the kept kind and six of the sorting kind."""
    h, dse = scene
    s, b = CloudSettings(), view(0.3)
    plugin.sort(h, view(0.0), s, download=False, into=dse.chunk(0))
    want = [direct(plugin, h, b, s, dse.chunk(0)), direct(plugin, h, b, s)]   # [kept, sorting]
    assert not same_bits(want[0], want[1])
    plugin.set_pipeline_depth(4)
    plugin.set_async(True)
    plugin.set_graphs(True)
    got = []

    def pop():
        ptr, _ = plugin.pipeline_pop()
        got.append(plugin.download(ptr, np.empty((HT, W, 4), np.float32)))

    def twelve():
        for f in range(12):
            if plugin.frames_in_flight() == 4:
                pop()
            plugin.render(h, b, s, download=False, entries=None if f % 2 else dse.chunk(0))
        while plugin.frames_in_flight():
            pop()

    twelve()
    c0, r0 = plugin.graph_counters()
    twelve()
    c1, r1 = plugin.graph_counters()
    assert len(got) == 24 and all(same_bits(g, want[f % 2]) for f, g in enumerate(got))
    print(f"[alternating] counted frames: captures +{c1 - c0}, replays +{r1 - r0}")
    assert r1 - r0 >= 12 - (c1 - c0)
    assert c1 - c0 == 0 and r1 - r0 == 12


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2])
def test_both_kinds_on_both_parities_of_one_lane(plugin, scene, depth):
    """What pins Lane::graph[kind][parity]. A lane's parity flips with every frame, so kinds in strict turn would tie each
    kind to one parity; in PAIRS, K K S S as a lane sees it, each kind meets both parities and each Control block is
    used by a kept frame right behind a sorting frame's and the other way round. Depth 1: the frames are K K S S ...;
    depth 2 (frame f on lane f % 2): K K K K S S S S ..., which is K K S S on either lane, two frames in flight.
    Warm-up, two periods (8 frames per lane): a lane never used launches its first frame directly (memset), the next
    four frames capture its four graphs at the latest, so the warm-up's last three frames per lane already replay.
    Counted, two more periods, 8 * depth frames: the hints are settled by the direct twins, no key changes, so
    captures == 0 and replays == 8 * depth. With one graph per parity instead, a frame of the other kind would find
    its parity's graph under the other kind's key and capture: four captures per period and lane."""
    h, dse = scene
    s, b = CloudSettings(), view(0.3)
    plugin.sort(h, view(0.0), s, download=False, into=dse.chunk(0))
    want = {"K": direct(plugin, h, b, s, dse.chunk(0)), "S": direct(plugin, h, b, s)}
    assert not same_bits(want["K"], want["S"])
    plugin.set_pipeline_depth(depth)
    plugin.set_async(True)
    plugin.set_graphs(True)
    period = "K" * (2 * depth) + "S" * (2 * depth)
    got = []

    def pop():
        ptr, _ = plugin.pipeline_pop()
        got.append(plugin.download(ptr, np.empty((HT, W, 4), np.float32)))

    def run(kinds):
        for k in kinds:
            if plugin.frames_in_flight() == depth:
                pop()
            plugin.render(h, b, s, download=False, entries=dse.chunk(0) if k == "K" else None)
        while plugin.frames_in_flight():
            pop()

    run(period * 2)
    c0, r0 = plugin.graph_counters()
    run(period * 2)
    c1, r1 = plugin.graph_counters()
    assert len(got) == 16 * depth and all(same_bits(g, want[k]) for g, k in zip(got, period * 4))
    print(f"[pairs, depth {depth}] counted frames: captures +{c1 - c0}, replays +{r1 - r0}")
    assert c1 - c0 == 0 and r1 - r0 == 8 * depth


# ---- 4. entries the compaction skips ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_skipped_entries_under_replay(plugin, scene):
    h, dse = scene
    v, s = view(0.1), CloudSettings()
    e = plugin.sort(h, v, s, into=dse.chunk(0)).copy()
    e["key"][::3] = CULLED
    e["index"][5::97] = N + np.arange(len(e["index"][5::97]), dtype=np.uint32)
    e["index"][7] = 0xFFFFFFFF
    drawable = int(((e["key"] != CULLED) & (e["index"] < N)).sum())
    assert 0 < drawable < N
    dse.upload(0, e)
    want = direct(plugin, h, v, s, dse.chunk(0))
    plugin.set_graphs(True)
    replays = 0
    for f in range(4):
        got, _, r = frame(plugin, h, v, s, dse.chunk(0))
        replays += r
        assert same_bits(got, want), f
    assert replays >= 2   # (a capture per parity at most)
    st = plugin.stats()   # (of the last frame: a replay)
    assert st["draw_count"] == drawable and st["splat_count"] == N and st["sort_path"] == "kept"
    assert 0 < st["visible_count"] <= drawable and st["algorithmic_bytes"] > 0


# ---- 5. shapes at the compaction's seams --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2049, 4097])
def test_replays_at_the_compaction_seams(plugin, n):
    """The compaction's tile is 2048 entries (256 x 8): one entry, a wave's seam, one ragged tile, two tiles plus one. Two
    captures at most, then two replays; bgs_synchronize checks the chain's watchdog word."""
    restore(plugin)
    plugin.reset_adaptive_state()
    small = base_cloud()
    reps = -(-n // N)
    tile = lambda a: np.ascontiguousarray(np.tile(a, (reps, 1))[:n])
    cloud = PlanarGaussian3d(tile(small.position_visibility), tile(small.spherical_harmonic), tile(small.rotation), tile(small.scale_opacity))
    h = plugin.upload(cloud)
    dse = plugin.device_sorted_entries(1, h)
    v, s = View.headless(64, 64, msaa_samples=1), CloudSettings()
    rng = np.random.default_rng(n)
    try:
        e = np.empty(n, SORT_ENTRY_DTYPE)
        e["key"], e["index"] = rng.integers(0, CULLED, n, dtype=np.uint32), rng.permutation(n).astype(np.uint32)
        e["key"][3::4] = CULLED
        e["index"][2::4] = n + (e["index"][2::4] % 5)
        dse.upload(0, e)
        plugin.set_profiling(0)
        plugin.set_async(True)
        want = direct(plugin, h, v, s, dse.chunk(0), 64)
        plugin.set_graphs(True)
        counts = []
        for f in range(4):
            got, c, r = frame(plugin, h, v, s, dse.chunk(0), 64)
            counts.append((c, r))
            assert same_bits(got, want), (n, f)
        plugin.synchronize()   # (raises unless BGS_OK)
        assert all(c + r == 1 for c, r in counts) and counts[2:] == [(0, 1), (0, 1)], (n, counts)
        assert plugin.stats()["draw_count"] == int(((e["key"] != CULLED) & (e["index"] < n)).sum())
    finally:
        restore(plugin)
        dse.free()
        h.free()


# ---- 6. a particle step between replays ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_replayed_kept_graph_draws_the_stepped_cloud(plugin, scene):
    h, dse = scene
    cloud, s, v = base_cloud(), CloudSettings(), view(0.0)
    rec = random_particle_behaviors(N, 3).records
    pv, _ = step_reference(cloud.position_visibility, rec, 0.25)
    stepped = plugin.upload(PlanarGaussian3d(pv, cloud.spherical_harmonic, cloud.rotation, cloud.scale_opacity))
    beh = plugin.upload_particle_behaviors(rec)
    try:
        plugin.sort(h, v, s, download=False, into=dse.chunk(0))
        old, new = direct(plugin, h, v, s, dse.chunk(0)), direct(plugin, stepped, v, s, dse.chunk(0))
        assert not same_bits(old, new)
        direct(plugin, h, v, s, dse.chunk(0))   # (the lane's buffers as the frames of `h` leave them)
        plugin.set_graphs(True)
        for f in range(4):
            got, _, _ = frame(plugin, h, v, s, dse.chunk(0))
            assert same_bits(got, old), f
        plugin.apply_particle_behaviors(h, beh, 0.25)
        for f in range(2):
            got, c, r = frame(plugin, h, v, s, dse.chunk(0))
            assert (c, r) == (0, 1), (f, c, r)   # a step changes no address: no capture
            assert same_bits(got, new), f
    finally:
        beh.free()
        stepped.free()


# ---- 7. a new cloud ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_new_cloud_recaptures(plugin, scene):
    """A shorter cloud, so that no buffer of the lane grows: its first kept graph frame is a capture (the key names the
    cloud's planes and its length), never a replay of the old cloud's graph."""
    h, dse = scene
    v, s = view(0.2), CloudSettings()
    plugin.sort(h, v, s, download=False, into=dse.chunk(0))
    want = direct(plugin, h, v, s, dse.chunk(0))
    plugin.set_graphs(True)
    for f in range(3):
        assert same_bits(frame(plugin, h, v, s, dse.chunk(0))[0], want)
    dse.free()
    h.free()
    n2 = 3000
    h2 = plugin.upload(random_gaussians_3d_seeded(n2, 22))
    dse2 = plugin.device_sorted_entries(1, h2)
    try:
        plugin.set_async(False)
        plugin.sort(h2, v, s, download=False, into=dse2.chunk(0))
        plugin.set_async(True)
        want2 = direct(plugin, h2, v, s, dse2.chunk(0))
        assert not same_bits(want2, want)
        plugin.set_graphs(True)
        got, c, r = frame(plugin, h2, v, s, dse2.chunk(0))
        assert (c, r) == (1, 0) and same_bits(got, want2)
        got, c, r = frame(plugin, h2, v, s, dse2.chunk(0))
        assert (c, r) == (1, 0) and same_bits(got, want2)   # (the other parity)
        got, c, r = frame(plugin, h2, v, s, dse2.chunk(0))
        assert (c, r) == (0, 1) and same_bits(got, want2)
    finally:
        restore(plugin)
        dse2.free()
        h2.free()
        # (the fixture frees these two once more: both calls tolerate it)


# ---- 8. what stays direct, and a frame that is run again ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_timed_and_no_graphs_kept_frames_stay_direct(plugin, scene):
    h, dse = scene
    v, s = view(0.2), CloudSettings()
    plugin.sort(h, v, s, download=False, into=dse.chunk(0))
    want = direct(plugin, h, v, s, dse.chunk(0))
    plugin.set_graphs(True)
    plugin.set_profiling(2)
    for f in range(3):
        got, c, r = frame(plugin, h, v, s, dse.chunk(0))
        assert (c, r) == (0, 0) and same_bits(got, want)
    st = plugin.stats()
    assert st["sort_path"] == "kept" and st["frames_averaged"] >= 1 and st["stage_ms"]["depth_sort"] == 0.0
    plugin.set_profiling(0)
    plugin.set_debug_flags(NO_GRAPHS)
    for f in range(3):
        got, c, r = frame(plugin, h, v, s, dse.chunk(0))
        assert (c, r) == (0, 0) and same_bits(got, want)


@pytest.mark.gpu
def test_a_kept_graph_frame_that_is_run_again(plugin, scene):
    """BGS_DEBUG_RERUN_EVERY_FRAME: finish_lane enqueues every frame a second time from the lane's copy of its inputs, as
    after a list overflow. The second attempt of a kept graph frame goes through the graph of the lane's other parity and
    reads the same, caller-owned chunk."""
    h, dse = scene
    v, s = view(0.2), CloudSettings()
    plugin.sort(h, v, s, download=False, into=dse.chunk(0))
    want = direct(plugin, h, v, s, dse.chunk(0))
    plugin.set_debug_flags(RERUN_EVERY_FRAME)
    plugin.set_graphs(True)
    c0, r0 = plugin.graph_counters()
    for f in range(3):
        plugin.render(h, v, s, download=False, entries=dse.chunk(0))
        ptr, _ = plugin.pipeline_pop()
        assert same_bits(plugin.download(ptr, np.empty((HT, W, 4), np.float32)), want), f
    c1, r1 = plugin.graph_counters()
    assert (c1 - c0) + (r1 - r0) == 6 and c1 - c0 <= 2   # six launches: one capture per parity at most, then replays
    assert plugin.stats()["regrow_count"] >= 1


# ---- the documents (no GPU) -----------------------------------------------------------------------------------------------------------------------
def test_the_header_no_longer_says_kept_frames_are_launched_directly():
    text = " ".join(open(os.path.join(ROOT, "include", "bgs.h")).read().replace("*", " ").split())
    assert "such a frame is launched directly, as timed frames are" not in text
    assert "chunk" in text and "may change between replays" in text
