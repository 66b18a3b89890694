"""BINNING_SORT's tile-instance budget on the device (tests/instance_budget_cases.py): the overflow verdict at
total == capacity and one past it, the host's growth and its one re-run, and the refusal past 2^30 with the context usable
afterwards. Every comparison is of integers or of bytes.

The image reference is the same frame under BINNING_SCAN — the path that is pinned to the float64 reference and the oracle
(test_binning_modes_give_bit_identical_images holds the two to each other) —, the list reference bin_stage_cases'
expansion of the twin's rectangles.

What the library does, as the tests below state it: a BINNING_SORT frame is always a blocking frame on lane 0, also under
bgs_set_async (csrc/bgs_frame.hip run(): async frames are BINNING_SCAN frames). So one lane's instance buffers grow, a
refusal surfaces in the render call itself, no BINNING_SORT frame is captured or replayed as a graph, and such a frame
leaves its scratch region to the next frame's memset (scratch_clean 0): the clean state is asserted on the scan frame
drawn behind it."""
import time

import numpy as np
import pytest

import instance_budget_cases as I
from bevy_gaussian_splatting_amd import GaussianSplattingPlugin, _native

pytestmark = pytest.mark.gpu


def _restore(p):
    p.set_async(False)
    p.set_graphs(False)
    p.set_debug_flags(0)
    p.set_profiling(2)
    p.set_pipeline_depth(1)
    p.set_binning("scan")


class Scene:
    """A case's cloud resident on a context."""

    def __init__(self, p, name):
        self.name, self.d = name, I.built(name)
        self.handle = p.upload(self.d["cloud"])

    def frame(self, p, binning, yaw=0.0, download=True):
        p.set_binning(binning)
        d = self.d if yaw == 0.0 else I.built(self.name, yaw)
        return p.render(self.handle, d["view"], d["settings"], download=download)


def _reruns(p):
    return p.adaptive_counters()["reruns_instances"]


def _check_lists(what, p, name):
    """The sorted instances and the tile ranges of the frame just drawn against the reference expansion."""
    inst, ranges, present = I.reference(name)
    dev = p.debug_frame_lists()
    assert dev["binning"] == "sort" and dev["draw_count"] == len(I.built(name)["rects"]), what
    assert dev["instance_count"] == len(inst), f"{what}: instance_count {dev['instance_count']}, reference {len(inst)}"
    bad = np.nonzero((dev["instances"] != inst).any(axis=1))[0]
    assert not len(bad), (f"{what}: {len(bad)} of {len(inst)} sorted instances differ, the first at {bad[0]}: device "
                          f"{dev['instances'][bad[0]].tolist()} reference {inst[bad[0]].tolist()}")
    got = dev["ranges"].astype(np.int64)
    bad = np.nonzero(present & (got != ranges).any(axis=1))[0]
    assert not len(bad), f"{what}: range of tile 0x{bad[0]:04x} is {got[bad[0]].tolist()}, reference {ranges[bad[0]].tolist()} ({len(bad)} differ)"
    bad = np.nonzero(~present & (got[:, 0] != got[:, 1]))[0]
    assert not len(bad), f"{what}: tile 0x{bad[0]:04x} holds no instance but its range is {got[bad[0]].tolist()}"


def test_a_frame_of_exactly_the_capacity_does_not_overflow():
    t0 = time.perf_counter()
    with GaussianSplattingPlugin(0) as p:
        try:
            p.reset_adaptive_state()
            s = Scene(p, "at_capacity")
            before = _reruns(p)
            img = s.frame(p, "sort")
            st = p.stats()
            assert _reruns(p) == before and st["regrow_count"] == 0, f"{_reruns(p) - before} re-runs, regrow_count {st['regrow_count']}"
            assert st["instance_count"] == 1 << 22 == st["instance_capacity"] == s.d["total"], (st["instance_count"], st["instance_capacity"])
            assert st["binning"] == "sort" and st["draw_count"] == len(s.d["cloud"])
            _check_lists("at_capacity", p, "at_capacity")
            ref = s.frame(p, "scan")
            assert np.isfinite(img).all() and img.tobytes() == ref.tobytes(), "at_capacity: the image is not the scan frame's"
            assert img[..., 3].min() > 0.999      # every pixel is covered until it saturates
        finally:
            _restore(p)
    print(f"at_capacity: {time.perf_counter() - t0:.2f} s")


def test_one_instance_over_grows_once_and_a_larger_frame_grows_again():
    t0 = time.perf_counter()
    with GaussianSplattingPlugin(0) as p:
        try:
            p.reset_adaptive_state()
            s = Scene(p, "one_over")
            before = _reruns(p)
            img = s.frame(p, "sort")
            st = p.stats()
            assert _reruns(p) - before == 1 and st["regrow_count"] == 1, f"{_reruns(p) - before} re-runs, regrow_count {st['regrow_count']}"
            assert st["instance_capacity"] == 1 << 23
            assert st["instance_count"] == s.d["total"] == (1 << 22) + 1
            # (a histogram carried over from the voided attempt would move every tile's first instance)
            _check_lists("one_over", p, "one_over")
            left = p.debug_frame_leftovers()
            assert left["binning"] == 1 and left["scratch_clean"] == 0     # the next frame's memset, not a clean-up
            # a second, identical frame: no re-run, the same bytes
            again = s.frame(p, "sort")
            assert _reruns(p) - before == 1 and p.stats()["regrow_count"] == 0 and p.stats()["instance_capacity"] == 1 << 23
            assert again.tobytes() == img.tobytes()
            # the scan frame behind it, on the lane whose scratch region the growth rebuilt: the same image, a clean scratch
            ref = s.frame(p, "scan")
            assert np.isfinite(img).all() and img.tobytes() == ref.tobytes(), "one_over: the image is not the scan frame's"
            left = p.debug_frame_leftovers()
            assert left["scratch_clean"] == 1 and left["dirty_words"] == 0, (left["scratch_clean"], left["dirty_words"])
            t1 = time.perf_counter()
            # in the same context: past 2^23, with room for a quarter more
            g = Scene(p, "second_growth")
            before = _reruns(p)
            img = g.frame(p, "sort")
            st = p.stats()
            assert _reruns(p) - before == 1 and st["regrow_count"] == 1
            assert st["instance_capacity"] == 1 << 24 and st["instance_count"] == g.d["total"]
            ref = g.frame(p, "scan")
            assert img.tobytes() == ref.tobytes(), "second_growth: the image is not the scan frame's"
            # the lane keeps what it grew to: the smaller frame fits at once
            img = s.frame(p, "sort")
            assert _reruns(p) - before == 1 and p.stats()["instance_capacity"] == 1 << 24 and img.tobytes() == again.tobytes()
        finally:
            _restore(p)
    print(f"one_over: {t1 - t0:.2f} s, second_growth: {time.perf_counter() - t1:.2f} s")


def test_a_need_that_fits_a_power_of_two_without_head_room_gets_the_next_one():
    t0 = time.perf_counter()
    with GaussianSplattingPlugin(0) as p:
        try:
            s = Scene(p, "head_room")
            before = _reruns(p)
            img = s.frame(p, "sort")
            st = p.stats()
            assert _reruns(p) - before == 1 and st["regrow_count"] == 1
            assert st["instance_count"] == s.d["total"] <= 1 << 23 and st["instance_capacity"] == 1 << 24
            assert img.tobytes() == s.frame(p, "scan").tobytes()
        finally:
            _restore(p)
    print(f"head_room: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("graphs", (False, True))
def test_frames_under_async_at_depth_two_grow_one_lane_once(graphs):
    """bgs_set_async and a pipeline depth of 2, four frames at two yaws: a BINNING_SORT frame is a blocking frame on lane 0
    whatever the mode, so nothing is in flight behind it, the one lane re-runs once (<= 2: at most once per lane) and every
    frame is its blocking reference. With graphs on and profiling off the same, and no BINNING_SORT frame is a replay."""
    t0 = time.perf_counter()
    yaws = (0.0, 0.01, 0.0, 0.01)
    with GaussianSplattingPlugin(0) as p:
        s = Scene(p, "one_over")
        want = {yaw: s.frame(p, "scan", yaw) for yaw in set(yaws)}
    with GaussianSplattingPlugin(0) as p:
        try:
            s = Scene(p, "one_over")
            p.reset_adaptive_state()
            p.set_pipeline_depth(2)
            p.set_async(True)
            if graphs:
                p.set_profiling(0)
                p.set_graphs(True)
            before, replays = _reruns(p), p.graph_counters()[1]
            for i, yaw in enumerate(yaws):
                s.frame(p, "sort", yaw, download=False)
                assert p.frames_in_flight() == 0, f"frame {i}: a BINNING_SORT frame was left in flight"
                ptr, nbytes = p.framebuffer_device_ptr()
                img = p.download(ptr, np.empty((256, 256, 4), np.float32))
                assert nbytes == img.nbytes and img.tobytes() == want[yaw].tobytes(), f"frame {i} (yaw {yaw}, graphs {graphs}) is not its blocking reference"
                assert p.stats()["instance_count"] == I.built("one_over", yaw)["total"]
            reruns, replayed = _reruns(p) - before, p.graph_counters()[1] - replays
            print(f"async depth 2, graphs {graphs}: {reruns} instance re-runs, {replayed} BINNING_SORT frames replayed from a graph, "
                  f"{time.perf_counter() - t0:.2f} s")
            assert 1 <= reruns <= 2 and p.stats()["instance_capacity"] == 1 << 23
            assert replayed == 0
        finally:
            _restore(p)


def _assert_refused(p, s):
    """The frame is refused with its exact count. (That the lane's capacity has not grown shows in _assert_still_draws: the
    buffers only ever grow, and at_capacity's frame finds 2^22.)"""
    with pytest.raises(_native.BgsError) as err:
        s.frame(p, "sort", download=False)
    assert err.value.status == _native.BGS_ECAPACITY, str(err.value)
    assert f"needs {s.d['total']} tile instances" in str(err.value), f"{str(err.value)!r} does not hold the twin's count {s.d['total']}"
    assert p.frames_in_flight() == 0


def _assert_still_draws(p):
    """The context after a refusal: at_capacity's frame (on the buffers the refused frame left: no growth) and an everyday
    frame under both binnings."""
    a = Scene(p, "at_capacity")
    before = _reruns(p)
    img = a.frame(p, "sort")
    st = p.stats()
    assert st["instance_capacity"] == 1 << 22 == st["instance_count"] and _reruns(p) == before, (st["instance_capacity"], st["instance_count"])
    assert img.tobytes() == a.frame(p, "scan").tobytes(), "at_capacity after a refusal: the image is not the scan frame's"
    cloud, view, settings = I.ordinary_frame()
    h = p.upload(cloud)
    p.set_binning("sort")
    one = p.render(h, view, settings)
    p.set_binning("scan")
    two = p.render(h, view, settings)
    assert np.isfinite(one).all() and one.tobytes() == two.tobytes(), "an everyday frame after a refusal"
    left = p.debug_frame_leftovers()
    assert left["scratch_clean"] == 1 and left["dirty_words"] == 0


@pytest.mark.parametrize("name", ("refused_2pow30", "carry_2pow32"))
def test_a_frame_past_the_limit_is_refused_with_its_count_and_the_context_draws_on(name):
    t0 = time.perf_counter()
    with GaussianSplattingPlugin(0) as p:
        try:
            p.reset_adaptive_state()
            s = Scene(p, name)
            before = _reruns(p)
            _assert_refused(p, s)
            t1 = time.perf_counter()
            assert _reruns(p) == before
            # refused again just the same: the lane is not left pending, its capacity has not grown
            _assert_refused(p, s)
            _assert_still_draws(p)
        finally:
            _restore(p)
    print(f"{name}: the refusal {t1 - t0:.2f} s, the whole test {time.perf_counter() - t0:.2f} s")


def test_a_refusal_under_async_at_depth_two_surfaces_in_the_call_and_the_pipeline_runs_on():
    """A BINNING_SORT frame under bgs_set_async is blocking: the refusal is the render call's, not a later pop's. The image
    the other lane drew before it is intact, and async BINNING_SCAN frames run on both lanes afterwards."""
    t0 = time.perf_counter()
    cloud, view, settings = I.ordinary_frame()
    with GaussianSplattingPlugin(0) as p:
        try:
            h = p.upload(cloud)
            want = p.render(h, view, settings)
            s = Scene(p, "refused_2pow30")
            p.set_pipeline_depth(2)
            p.set_async(True)
            for _ in range(2):     # lane 0, then lane 1
                p.render(h, view, settings, download=False)
            p.pipeline_pop()
            ptr, _ = p.pipeline_pop()
            assert p.frames_in_flight() == 0
            _assert_refused(p, s)
            # the other lane's frame: the refused frame ran on lane 0, lane 1's image is where it was
            assert p.download(ptr, np.empty_like(want)).tobytes() == want.tobytes()
            p.set_binning("scan")
            popped = []
            for i in range(4):
                p.render(h, view, settings, download=False)
                if p.frames_in_flight() == 2:
                    popped.append(p.download(p.pipeline_pop()[0], np.empty_like(want)))
            while p.frames_in_flight():
                popped.append(p.download(p.pipeline_pop()[0], np.empty_like(want)))
            p.synchronize()
            assert len(popped) == 4 and all(img.tobytes() == want.tobytes() for img in popped)
            p.set_async(False)
            _assert_still_draws(p)
        finally:
            _restore(p)
    print(f"refusal under async: {time.perf_counter() - t0:.2f} s")
