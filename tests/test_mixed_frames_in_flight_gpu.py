"""Frames of different kinds on shared lanes (tests/mixed_frame_cases.py: the kinds, the schedule, the lane rule): every frame
of a mixed schedule is, bit for bit, the same frame drawn alone in a fresh context. Every comparison is of bytes.

  alone   every kind once in a context of its own (synchronous, one lane, no graphs); the kinds of the f32 cloud also on the
          stepped cloud, and once more behind the inverse step, which must give the first image back.
  mixed   the session's context with the three clouds resident, async, `depth` lanes on `streams` streams, graphs off or on:
          the schedule is walked, a frame popped whenever `depth` are in flight, the ring drained at the end; with graphs
          on the schedule is walked three times, so that lanes replay graphs captured for other kinds. The enqueue counters
          must show the flagged re-runs, and the early-completion counter that frames waited in the ring.
  after   on what the mix left, one lane, blocking: every kind once more, with the counts of its alone twin; then the scan
          kinds at supertile level 2 with the mid-round exit (the plan under which a frame leaves and reads the heavy-tile
          lists), the two grids of 240 tiles in turn. At these sizes no strip workgroup drew a tile (the count is printed),
          so the rounds pin level 2 and the mid-round exit on the mix's leftovers, not the use of a stale list.
  named   the same walk against a table in which one kind has another's image: exactly that kind's frames are reported.

The targets are far below the tile count from which plan_frame orders a frame's workgroups (more tile waves than the chip
holds: over a thousand tiles), so no frame here consults cost_done_grid or order_grid.

A BINNING_SORT kind is never in flight beside another frame (run(), csrc/bgs_frame.hip: it completes the ring and draws on
lane 0, blocking), and the calls that complete the ring take a completed frame off it unseen. So the walk pops what is in
flight before such a call; before a cloud's free and before bgs_reset_adaptive_state it leaves the newest frame in flight and
reads it afterwards as the context's most recent frame. No kind needed another reference than its alone twin.

A frame that differs is reported with its position, kind and lane, the lane's previous frame, its neighbours in the
schedule, the events before it, its first differing pixel, and whether it was a re-run or a replay; the test fails once,
with the count."""
import time
from collections import deque

import numpy as np
import pytest

import mixed_frame_cases as M
from bevy_gaussian_splatting_amd import GaussianSplattingPlugin
from bevy_gaussian_splatting_amd.multiview import device_ptr_as_tensor

pytestmark = pytest.mark.gpu

DEFAULT_STREAMS = 4   # bgs_ctx::num_streams of a new context


def _read(ptr, k, what):
    h, w = k.size[1], k.size[0]
    typestr = {"f32": "<f4", "srgb8": "|u1", "f16_only": "<u2"}[what]
    return device_ptr_as_tensor(ptr, (h, w, 4), typestr, "cuda:0").cpu().numpy()


class Scene:
    """A context with the three clouds resident and what the kinds need besides: the depth plane, the kept-order chunk, the
    particle behaviours."""

    def __init__(self, plugin):
        self.p = plugin
        self.handles, self.depth_ptr, self.entries, self.behaviors = {}, 0, None, None
        self.binning = "scan"
        self.outputs = None
        try:
            for name in M.CLOUDS:
                self.handles[name] = M.upload(plugin, name)
            self.depth_ptr = plugin.upload_depth(M.depth_plane(next(k for k in M.KINDS if k.depth_buffer)))
            kept = next(k for k in M.KINDS if k.kept)
            self.entries = plugin.device_sorted_entries(1, self.handles[kept.cloud])
            plugin.sort(self.handles[kept.cloud], kept.view(M.KEPT_SORT_YAW), kept.settings(), download=False, into=self.entries.chunk(0))
            self.behaviors = plugin.upload_particle_behaviors(M.particle_step()[0])
            self.views = {}
            for k in M.KINDS:
                v = k.view()
                if k.depth_buffer:
                    v.depth_device_ptr = self.depth_ptr
                self.views[k.name] = (v, k.settings())
        except Exception:
            self.close()
            raise

    def close(self):
        p = self.p
        for h in self.handles.values():
            h.free()
        self.handles = {}
        if self.entries is not None:
            self.entries.free()
        if self.behaviors is not None:
            self.behaviors.free()
        if self.depth_ptr:
            p.device_free(self.depth_ptr)
        self.entries = self.behaviors = None
        self.depth_ptr = 0

    def set_binning(self, mode):
        """(bgs_set_binning completes the ring: the caller has popped what was in flight)"""
        if self.binning != mode:
            self.p.set_binning(mode)
            self.binning = mode

    def enqueue(self, k, flags=0):
        """The kind's frame: enqueued in an async context that bins by scan, drawn to completion otherwise."""
        p = self.p
        self.set_binning(k.binning)
        if self.outputs != k.outputs:
            p.set_output_srgb8(k.outputs == "srgb8")
            p.set_output_rgba16f(k.outputs == "f16_only")
            p.set_packed_only(k.outputs == "f16_only")
            self.outputs = k.outputs
        v, s = self.views[k.name]
        p.set_debug_flags(flags)
        p.render(self.handles[k.cloud], v, s, download=False, entries=self.entries.chunk(0) if k.kept else None)
        if flags:
            p.set_debug_flags(0)

    def images(self, k, ptrs=None):
        """{"f32": ..., "packed": ...} of a popped frame (`ptrs` of pipeline_pop) or of the context's most recent frame; an image
        the frame should have and does not hand out is None, and `stray` names one it hands out and should not have."""
        p = self.p
        out = {"f32": None, "packed": None, "stray": []}
        if k.outputs != "f16_only":
            ptr = ptrs[0] if ptrs else p.framebuffer_device_ptr()[0]
            out["f32"] = _read(ptr, k, "f32") if ptr else None
        elif ptrs and ptrs[0] is not None:
            out["stray"].append("a packed-only frame hands out an f32 target")
        if k.outputs != "f32":
            recent = p.framebuffer_srgb8_device_ptr if k.outputs == "srgb8" else p.framebuffer_rgba16f_device_ptr
            ptr = ptrs[1] if ptrs else recent()[0]
            out["packed"] = _read(ptr, k, k.outputs) if ptr else None
        elif ptrs and ptrs[1] is not None:
            out["stray"].append("a frame without a packed output hands one out")
        return out

    def step(self, dt):
        self.p.apply_particle_behaviors(self.handles[M.STEP_CLOUD], self.behaviors, dt)


def _same(a, b):
    return a is b or (a is not None and b is not None and a.tobytes() == b.tobytes())


# ---- 1. alone ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def alone():
    want = {}
    t0 = time.perf_counter()
    for k in M.KINDS:
        with GaussianSplattingPlugin(0) as p:
            sc = Scene(p)
            try:
                sc.enqueue(k)
                base = sc.images(k)
                st = p.stats()
                want[k.name] = {"base": base, "stats": {f: st[f] for f in ("draw_count", "visible_count", "instance_count")}}
                if k.outputs == "f16_only":   # (its f32 image, for the comparisons between kinds only)
                    p.set_packed_only(False)
                    sc.enqueue(k)
                    want[k.name]["f32_for_kinds"] = _read(p.framebuffer_device_ptr()[0], k, "f32")
                    sc.outputs = None
                if k.cloud == M.STEP_CLOUD:
                    sc.step(M.STEP_DT)
                    sc.enqueue(k)
                    want[k.name]["stepped"] = sc.images(k)
                    sc.step(-M.STEP_DT)
                    sc.enqueue(k)
                    back = sc.images(k)
                    assert _same(back["f32"], base["f32"]) and _same(back["packed"], base["packed"]), \
                        f"{k.name}: the inverse step does not give the first frame back"
            finally:
                sc.close()
    print(f"alone: {len(M.KINDS)} contexts in {time.perf_counter() - t0:.2f} s")
    for k in M.KINDS:
        w = want[k.name]
        print(f"alone {k.name}: {w['stats']}")
        assert w["stats"]["draw_count"] > 0 and w["stats"]["visible_count"] > 0 and w["stats"]["instance_count"] > 0, k.name
        f32 = w["base"]["f32"] if w["base"]["f32"] is not None else w["f32_for_kinds"]
        clear = np.asarray(k.view().clear_color, np.float32)
        touched = int((f32 != clear).any(axis=-1).sum())
        assert np.isfinite(f32).all() and touched > f32.shape[0] * f32.shape[1] // 50, f"{k.name}: {touched} pixels are not the clear colour"
        if w["base"]["packed"] is not None:
            assert len(np.unique(w["base"]["packed"].reshape(-1, 4), axis=0)) > 16, f"{k.name}: the packed image is all but constant"
        if "stepped" in w:
            for what in ("f32", "packed"):
                assert (w["base"][what] is None) or not _same(w["base"][what], w["stepped"][what]), f"{k.name}: the step does not show in {what}"
        w["f32_any"] = f32
    # a mix-up must show: no two kinds of one size draw the same image
    for i, a in enumerate(M.KINDS):
        for b in M.KINDS[i + 1:]:
            if a.size == b.size:
                assert not _same(want[a.name]["f32_any"], want[b.name]["f32_any"]), f"{a.name} and {b.name} draw the same image"
                pa, pb = want[a.name]["base"]["packed"], want[b.name]["base"]["packed"]
                if pa is not None and pb is not None and pa.dtype == pb.dtype:
                    assert not _same(pa, pb), f"{a.name} and {b.name} draw the same packed image"
    return want


# ---- 2. mixed ----------------------------------------------------------------------------------------------------------------
def _first_difference(got, want):
    g, w = got.reshape(got.shape[0], got.shape[1], -1), want.reshape(want.shape[0], want.shape[1], -1)
    bad = np.argwhere((g.view(np.uint8) != w.view(np.uint8)).any(axis=-1))
    y, x = (int(c) for c in bad[0])
    return f"{len(bad)} pixels, first ({x}, {y}) of tile ({x // 16}, {y // 16}): got {got[y, x].tolist()}, alone {want[y, x].tolist()}"


class Walk:
    def __init__(self, plugin, scene, alone, depth):
        self.p, self.sc, self.alone, self.depth = plugin, scene, alone, depth
        self.in_flight = deque()          # (Position, pass, was a replay), oldest first
        self.bad, self.compared = [], 0
        self.context = {}                 # (pass, frame index) -> Position

    def compare(self, pos, rep, replay, got, how):
        k = M.by_name(pos.kind)
        want = self.alone[pos.kind]["stepped" if (pos.stepped and k.cloud == M.STEP_CLOUD) else "base"]
        self.compared += 1
        for what in ("f32", "packed", "stray"):
            if what == "stray":
                wrong = "; ".join(got["stray"])
            elif want[what] is None or (got[what] is not None and got[what].tobytes() == want[what].tobytes()):
                wrong = ""
            else:
                wrong = f"{what} differs: " + ("no image" if got[what] is None else _first_difference(got[what], want[what]))
            if not wrong:
                continue
            before, after = self.context.get((rep, pos.index - 1)), self.context.get((rep, pos.index + 1))
            line = (f"pass {rep} frame {pos.index} ({how}) kind {pos.kind} lane {pos.lane}{' stepped' if pos.stepped else ''}: "
                    f"lane's previous frame {pos.lane_prev.kind if pos.lane_prev else None}, frame before {before.kind if before else None}, "
                    f"frame after {after.kind if after else None}, events before it {list(pos.events)}, last event {self.last_event(pos)}, "
                    f"re-run {pos.rerun}, replay {replay}; {wrong}")
            print(line)
            self.bad.append(line)

    def last_event(self, pos):
        for s in reversed(self.steps[:pos.step]):
            if s[0] != "frame":
                return s
        return None

    def pop_one(self):
        assert self.p.frames_in_flight() == len(self.in_flight), (self.p.frames_in_flight(), len(self.in_flight))
        ptrs = self.p.pipeline_pop()
        pos, rep, replay = self.in_flight.popleft()   # (first in, first out: a frame out of turn is another kind's image)
        self.compare(pos, rep, replay, self.sc.images(M.by_name(pos.kind), ptrs), "popped")

    def pop_down_to(self, keep):
        while len(self.in_flight) > keep:
            self.pop_one()

    def around_newest(self, call):
        """A call that completes the ring, with the newest frame still in flight: that frame is read as the most recent one."""
        self.pop_down_to(1)
        call()
        assert self.p.frames_in_flight() == 0
        if self.in_flight:
            pos, rep, replay = self.in_flight.popleft()
            self.compare(pos, rep, replay, self.sc.images(M.by_name(pos.kind)), "completed by the call behind it")

    def event(self, step):
        p, sc = self.p, self.sc
        if step[0] == "sort":
            self.pop_down_to(0)
            k = M.by_name(step[1])
            entries = p.sort(sc.handles[k.cloud], k.view(), k.settings())
            assert len(entries) == k.n
        elif step[0] == "radix_pairs":
            self.pop_down_to(0)
            keys = (np.arange(1000, dtype=np.uint32) * np.uint32(2654435761)) >> np.uint32(3)
            out = p.radix_sort_pairs(keys)
            assert (np.diff(out["key"].astype(np.int64)) >= 0).all()
        elif step[0] == "particle_step":
            sc.step(step[1])     # (completes the frames and leaves them in the ring)
            assert p.frames_in_flight() == len(self.in_flight)
        elif step[0] == "reupload":
            def call():
                sc.handles[step[1]].free()
                sc.handles[step[1]] = M.upload(p, step[1])
            self.around_newest(call)
        elif step[0] == "reset_learning":
            self.around_newest(p.reset_adaptive_state)
        else:
            assert step[0] == "rerun_next"   # (the next frame's flag: Position.rerun)

    def run(self, steps, rep, rule, lane_last):
        self.steps = steps
        frames = {f.step: f for f in M.walk(steps, self.depth, rule, lane_last)}
        for f in frames.values():
            self.context[(rep, f.index)] = f
        p, sc = self.p, self.sc
        for si, step in enumerate(steps):
            if step[0] != "frame":
                self.event(step)
                continue
            pos, k = frames[si], M.by_name(step[1])
            flags = M.RERUN_EVERY_FRAME if pos.rerun else 0
            if k.binning == "sort":
                self.pop_down_to(0)
                sc.enqueue(k, flags)
                assert p.frames_in_flight() == 0
                self.compare(pos, rep, False, sc.images(k), "blocking")
                continue
            if sc.binning != "scan":
                assert not self.in_flight
            replays = p.graph_counters()[1]
            sc.enqueue(k, flags)
            self.in_flight.append((pos, rep, p.graph_counters()[1] != replays))
            while p.frames_in_flight() >= self.depth:
                self.pop_one()
        self.pop_down_to(0)
        assert p.frames_in_flight() == 0


def _restore(p):
    p.set_async(False)
    p.set_graphs(False)
    p.set_pipeline_depth(1)
    p.set_pipeline_streams(DEFAULT_STREAMS)
    p.set_binning("scan")
    p.set_output_srgb8(False)
    p.set_output_rgba16f(False)
    p.set_packed_only(False)
    p.set_debug_flags(0)
    p.set_profiling(2)
    p.reset_adaptive_state()


def _parameters():
    """(depth, graphs, streams): 0 streams is a stream a lane (assign_streams, csrc/bgs_frame.hip), 1 is every lane on one, and
    at depth 8 also a new context's own 4 (bgs_ctx::num_streams), two lanes a stream."""
    out = []
    for depth in M.DEPTHS:
        for graphs in (False, True):
            seen = set()
            for streams in (0, 1, depth) + ((DEFAULT_STREAMS,) if depth > DEFAULT_STREAMS else ()):
                effective = depth if streams == 0 else min(streams, depth)
                if effective not in seen:
                    seen.add(effective)
                    out.append(pytest.param(depth, graphs, streams, id=f"depth{depth}-{'graphs' if graphs else 'direct'}-streams{streams}"))
    return out


LEVEL_2, MIDROUND_ALWAYS = 0x400000, 0x20000   # include/bgs_diag.h: neither changes a bit of a frame
LEARN_MAX = 3                                  # csrc/adaptive_state.h: frames of a kind completed early before it is settled on anyway


def _alone_again(p, sc, w, steps):
    """What the mix left, one lane, blocking. Every kind once: its images and the counts of its alone twin (the draw count
    and the visible count of every kind; the tile instances of a BINNING_SORT kind only: a BINNING_SCAN frame counts list
    entries, which follow the supertile level the context has learnt). Then the BINNING_SCAN kinds at supertile level 2 with
    the mid-round exit, the plan under which plan_frame lets a frame leave and read the heavy-tile lists, the two grids of
    240 tiles in turn: a list left by a frame of 20 x 12 tiles is what the next frame of 24 x 10 would find. Returns the
    tiles strip workgroups drew (0: the lists were of no consequence)."""
    p.set_async(False)
    p.set_pipeline_depth(1)
    for i, k in enumerate(M.KINDS):
        sc.enqueue(k)
        pos = M.Position(i, len(steps), k.name, 0, False, False, None, ())
        w.compare(pos, "after", False, sc.images(k), "blocking, after the drain")
        st, want = p.stats(), w.alone[k.name]["stats"]
        for f in ("draw_count", "visible_count") + (("instance_count",) if k.binning == "sort" else ()):
            if st[f] != want[f]:
                w.bad.append(f"after the drain, kind {k.name}: {f} {st[f]}, alone {want[f]}")
                print(w.bad[-1])
    scan = [k for k in M.KINDS if k.binning == "scan"]
    a = [k for k in scan if k.tiles == (20, 12)]
    b = [k for k in scan if k.tiles == (24, 10)]
    assert a and b
    order = [k for pair in zip(a * len(b), b * len(a)) for k in pair][:2 * max(len(a), len(b))] + [k for k in scan if k not in a + b]
    strips = 0
    for rnd in range(2):
        for i, k in enumerate(order):
            sc.enqueue(k, LEVEL_2 | MIDROUND_ALWAYS)
            pos = M.Position(i, len(steps), k.name, 0, False, False, None, ())
            w.compare(pos, f"dense {rnd}", False, sc.images(k), "blocking, supertile level 2 and the mid-round exit, after " +
                      (order[i - 1].name if i else "the round before"))
            strips += p.stats()["strip_tiles"]
    return strips


def _mix(p, alone, depth, graphs, streams):
    """The schedule on context p; (the Walk, what was counted)."""
    steps = M.schedule(depth, M.SEEDS[0])
    passes = 3 if graphs else 1
    t0 = time.perf_counter()
    sc = None
    try:
        _restore(p)
        sc = Scene(p)
        p.set_profiling(0)          # (timed frames are launched directly, never as a graph)
        p.set_pipeline_streams(streams)
        p.set_pipeline_depth(depth)
        p.set_async(True)
        p.set_graphs(graphs)
        captures0, replays0 = p.graph_counters()
        counters0, early0 = p.adaptive_counters(), p.learning_counters()["early_frames"]
        w = Walk(p, sc, alone, depth)
        rule, lane_last = M.LaneRule(depth), {}
        for rep in range(passes):
            w.run(steps, rep, rule, lane_last)
        mixed = w.compared
        captures, replays = (a - b for a, b in zip(p.graph_counters(), (captures0, replays0)))
        counters, early = p.adaptive_counters(), p.learning_counters()["early_frames"] - early0
        strips = _alone_again(p, sc, w, steps)
        wall = time.perf_counter() - t0
        frames = M.walk(steps, depth)
        print(f"depth {depth} graphs {graphs} streams {streams}: {len(steps)} steps, {len(frames)} frames a pass, {mixed} frames compared in the mix, "
              f"{captures} captures, {replays} replays, {early} frames completed early, {strips} tiles drawn by strips after the drain, "
              f"wall {wall:.2f} s, {len(w.bad)} differ")
        assert mixed == len(frames) * passes
        assert (replays > 0 and captures > 0) if graphs else (replays == 0 and captures == 0), (captures, replays)
        # Every frame and every bgs_sort that sorts by depth is counted when it is enqueued, a re-run again (commit_frame): the
        # frames under RERUN_EVERY_FRAME were run twice, or the sum is short.
        capacity = sum(counters[f] - counters0[f] for f in counters if f.startswith("reruns"))
        sorting = [f for f in frames if not M.by_name(f.kind).kept]
        forced = [f for f in sorting if f.rerun and not M.is_sort(f.kind)]
        sorts = sum(1 for s in steps if s[0] == "sort")
        enqueued = sum(counters[f] - counters0[f] for f in ("bucket_frames", "onesweep_frames"))
        print(f"{enqueued} depth sorts enqueued: {len(sorting)} frames and {sorts} sorts a pass, {len(forced)} of them re-run by the flag, {capacity} for a capacity")
        assert forced, "no frame that sorts is re-run by the flag"
        assert enqueued == passes * (len(sorting) + sorts + len(forced)) + capacity
        # Frames really wait in the ring: a kind's frames are completed inside their render call LEARN_MAX times at the most
        # before the context settles on it, from the start and again from every reset of what it learnt.
        scan = [f for f in frames if not M.is_sort(f.kind)]
        resets = sum(1 for s in steps if s[0] == "reset_learning")
        bound = len({f.kind for f in scan}) * LEARN_MAX * (1 + passes * resets)
        assert early <= bound and early < passes * len(scan), f"{early} of {passes * len(scan)} async frames were completed early (at most {bound})"
        return w
    finally:
        try:
            _restore(p)
        finally:
            if sc is not None:
                sc.close()


@pytest.mark.parametrize("depth,graphs,streams", _parameters())
def test_every_frame_of_a_mixed_schedule_is_its_alone_twin(plugin, alone, depth, graphs, streams):
    w = _mix(plugin, alone, depth, graphs, streams)
    assert not w.bad, f"{len(w.bad)} comparisons of {w.compared} frames differ from the frame drawn alone:\n" + "\n".join(w.bad[:12])


def test_a_frame_that_is_not_its_twin_is_named(plugin, alone):
    """The walk against a table in which two kinds of one size have changed places: every frame of the two, in the mix and after
    the drain, is reported with its lane and its first pixel, and no other frame is."""
    a, other = "cov_dense", "f16_16bit_srgb8"
    assert M.by_name(a).outputs == "f32" and M.by_name(a).binning == "scan" and M.by_name(other).size == M.by_name(a).size
    swapped = dict(alone)
    swapped[a] = dict(alone[a], base={"f32": alone[other]["base"]["f32"], "packed": None})   # (an image of the right size, of another kind)
    w = _mix(plugin, swapped, 2, False, 0)
    frames = [f for f in M.walk(M.schedule(2, M.SEEDS[0]), 2) if f.kind == a]
    named = [line for line in w.bad if f"kind {a} " in line]
    assert len(named) == len(w.bad), [line for line in w.bad if line not in named][:3]
    assert len(named) == len(frames) + 1 + 2, (len(named), len(frames))   # (the mix, once after the drain, twice at level 2)
    assert all(" lane " in line and "f32 differs" in line and "pixels, first (" in line and "of tile (" in line for line in named)
    f = frames[0]
    assert any(line.startswith(f"pass 0 frame {f.index} (popped) kind {a} lane {f.lane}") or
               line.startswith(f"pass 0 frame {f.index} (completed by the call behind it) kind {a} lane {f.lane}") for line in named)
