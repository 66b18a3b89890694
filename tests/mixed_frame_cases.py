"""Frames of different kinds in flight: the kinds and the schedule of tests/test_mixed_frames_host.py and
tests/test_mixed_frames_in_flight_gpu.py. No GPU here.

WHICH LANE DRAWS A FRAME (run() and enqueue_frame, csrc/bgs_frame.hip; bgs_set_pipeline_depth, csrc/bgs_api.hip):

  A frame is ASYNC when bgs_set_async(1) holds, it is a render, and the context bins by scan. It goes to lane `next`, the
  lane's previous frame is completed first, and next = (next + 1) % depth. bgs_set_pipeline_depth sets next = 0.
  Every other call that draws or sorts is BLOCKING: a render of a context that bins by sort, a bgs_sort, a
  bgs_radix_sort_pairs. It completes every frame in flight, runs on lane 0 and leaves `next` where it was. So a BINNING_SORT
  frame is never in flight beside another frame; what it shares with the other kinds is lane 0 and what they left there.
  A re-run (finish_lane) is enqueued on the lane of the frame it repeats.

`LaneRule` is that rule; the same-lane successors of the schedule are computed with it, never with i % depth.

CALLS THAT COMPLETE THE RING (include/bgs.h: "completes the frames in flight"): a blocking frame or sort, bgs_set_binning,
bgs_radix_sort_pairs, bgs_cloud_free, bgs_reset_adaptive_state, bgs_get_stats. A frame they complete can no longer be
popped; only the most recently enqueued one can still be read (bgs_framebuffer_*_device_ptr). The walk of the GPU test pops
what is in flight before such a call, all of it or (cloud free, reset) all but the newest frame. A particle step completes
the frames too, and leaves them in the ring.

A PAIR OF THE SCHEDULE COUNTS only when no event other than `rerun_next` lies between its two frames: a sort, a free or a
reset between them rewrites what the first frame left, and the pair would be covered in name only."""
import random
from dataclasses import dataclass

import numpy as np

from bevy_gaussian_splatting_amd import CloudSettings, RasterizeMode, View, random_gaussians_3d_seeded
from bevy_gaussian_splatting_amd.particles import PARTICLE_BEHAVIOR_DTYPE, ParticleBehaviors, step_reference
from bevy_gaussian_splatting_amd.settings import GaussianMode, RadixSortDepthBits, SortMode

RERUN_EVERY_FRAME = 0x8000000   # include/bgs_diag.h: every BINNING_SCAN frame is run twice, as if a capacity had been short

# ---- the clouds --------------------------------------------------------------------------------------------------------------
CLOUDS = {"f32": (3000, 71, "f32"), "f16": (9000, 72, "f16"), "cov": (30000, 73, "cov3d")}   # name: splats, seed, format
_clouds = {}


def cloud(name: str):
    """The f32 source of a resident cloud, made once and never modified."""
    if name not in _clouds:
        n, seed, _ = CLOUDS[name]
        c = random_gaussians_3d_seeded(n, seed)
        c.position_visibility.setflags(write=False)
        _clouds[name] = c
    return _clouds[name]


def upload(plugin, name: str, source=None):
    c = cloud(name) if source is None else source
    fmt = CLOUDS[name][2]
    return plugin.upload(c.to_f16()) if fmt == "f16" else plugin.upload(c, precompute_covariance_3d=(fmt == "cov3d"))


# ---- the kinds ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Kind:
    name: str
    cloud: str                  # key of CLOUDS
    size: tuple                 # target, pixels
    binning: str = "scan"
    samples: int = 4
    shape: str = "obb"          # obb / aabb3d / surfel
    sort_mode: SortMode = SortMode.Radix
    bits: int = 32
    outputs: str = "f32"        # f32 / srgb8 (f32 and Rgba8UnormSrgb) / f16_only (Rgba16Float, set_packed_only)
    mode: RasterizeMode = RasterizeMode.Color
    scale: float = 1.0
    depth_buffer: bool = False  # View.depth_device_ptr: a device depth plane (upload_depth)
    kept: bool = False          # drawn from a chunk of device entries that a sort from another camera filled
    yaw: float = 0.0

    @property
    def format(self) -> str:
        return CLOUDS[self.cloud][2]

    @property
    def n(self) -> int:
        return CLOUDS[self.cloud][0]

    @property
    def tiles(self) -> tuple:
        return (-(-self.size[0] // 16), -(-self.size[1] // 16))

    def settings(self) -> CloudSettings:
        extra = {"obb": {}, "aabb3d": {"aabb": True}, "surfel": {"aabb": True, "gaussian_mode": GaussianMode.Gaussian2d}}[self.shape]
        return CloudSettings(sort_mode=self.sort_mode, radix_sort_depth_bits=RadixSortDepthBits(self.bits), global_scale=self.scale,
                             rasterize_mode=self.mode, **extra)

    def view(self, yaw=None) -> View:
        return View.headless(self.size[0], self.size[1], yaw=self.yaw if yaw is None else yaw, msaa_samples=self.samples)


KEPT_SORT_YAW = 0.4   # the camera whose sort fills the kept-order kind's chunk (culled entries are skipped)

KINDS = (
    Kind("f32_obb_80", "f32", (80, 48)),
    Kind("f32_surfel_s4_srgb8", "f32", (250, 130), shape="surfel", outputs="srgb8", yaw=0.1),
    Kind("f32_sortbin_rayon", "f32", (320, 192), binning="sort", samples=1, shape="aabb3d", sort_mode=SortMode.Rayon),
    Kind("f16_kept", "f16", (320, 192), kept=True),
    Kind("f16_16bit_srgb8", "f16", (384, 160), samples=1, shape="aabb3d", bits=16, outputs="srgb8"),
    Kind("f16_sortbin_surfel_s4", "f16", (250, 130), binning="sort", shape="surfel", yaw=-0.1),
    Kind("f16_depth_buffer", "f16", (80, 48), sort_mode=SortMode.Rayon, depth_buffer=True, yaw=0.2),
    Kind("cov_dense", "cov", (384, 160)),
    Kind("cov_sparse_rayon_srgb8", "cov", (320, 192), samples=1, sort_mode=SortMode.Rayon, outputs="srgb8", scale=0.05),
    Kind("cov_f16_only", "cov", (250, 130), shape="aabb3d", outputs="f16_only", yaw=0.3),
    Kind("cov_depth_mode_16bit", "cov", (80, 48), samples=1, bits=16, mode=RasterizeMode.Depth, scale=0.05, yaw=-0.2),
    Kind("cov_sortbin_dense_16bit", "cov", (384, 160), binning="sort", samples=1, shape="aabb3d", sort_mode=SortMode.Rayon, bits=16),
)
KIND_NAMES = tuple(k.name for k in KINDS)
AXES = ("cloud", "size", "binning", "samples", "shape", "sort_mode", "bits", "outputs", "mode", "scale", "depth_buffer", "kept")


def by_name(name: str) -> Kind:
    return KINDS[KIND_NAMES.index(name)]


def is_sort(name: str) -> bool:
    return by_name(name).binning == "sort"


def graph_tuple(k: Kind) -> tuple:
    """What GraphKey (csrc/bgs_context.h) takes from the frame rather than from the lane: the cloud, n, the digit places, the
    sort mode, the packed output, the vertex stage's and the rasteriser's instantiation, the target, the graph's kind."""
    places = 0 if k.kept else k.bits // 8
    return (k.cloud, k.n, places, int(k.sort_mode), k.outputs, (k.format, k.shape), (k.samples, k.depth_buffer, int(k.mode)),
            k.size, k.kept, k.binning)


def depth_plane(k: Kind) -> np.ndarray:
    """The depth-buffer kind's plane, [height, width, samples] reverse-Z (helpers.random_depth_buffer, a fixed seed)."""
    import helpers as H
    return H.random_depth_buffer(cloud(k.cloud), k.view(), k.settings(), np.random.default_rng(74))


# ---- the particle step of the f32 cloud ----------------------------------------------------------------------------------
STEP_DT = 0.25          # a power of two: v * dt is exact, and v * (-dt) its negation
STEP_CLOUD = "f32"
_step = {}


def particle_step():
    """(records, stepped position_visibility): velocities only (no acceleration, no jerk, nothing on the visibility lane), and
    only for the splats whose position comes back bit for bit, fl(fl(p + d) - d) == p on all three axes: the step by -dt is
    then the inverse of the step by dt, and the records are left as they were (dv = da = 0)."""
    if not _step:
        pv = cloud(STEP_CLOUD).position_visibility
        n = pv.shape[0]
        rng = np.random.default_rng(75)
        v = np.zeros((n, 4), np.float32)
        v[:, :3] = rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
        d = v * np.float32(STEP_DT)
        back = (pv + d) - d
        exact = np.flatnonzero((back.view(np.uint32) == pv.view(np.uint32)).all(axis=1))
        rec = np.zeros(exact.size, PARTICLE_BEHAVIOR_DTYPE)
        rec["indicies"][:, 0] = exact.astype(np.uint32)
        rec["velocity"] = v[exact]
        stepped, rec_after = step_reference(pv, rec, STEP_DT)
        assert rec_after.tobytes() == rec.tobytes()
        _step["records"], _step["stepped"] = ParticleBehaviors(rec, n), stepped
    return _step["records"], _step["stepped"]


# ---- the lane rule ---------------------------------------------------------------------------------------------------------
class LaneRule:
    """The lane of every frame of a context from bgs_set_pipeline_depth(depth) on (the module docstring)."""

    def __init__(self, depth: int):
        self.depth, self.next = int(depth), 0

    def place(self, kind_name: str) -> int:
        if is_sort(kind_name):
            return 0
        lane, self.next = self.next, (self.next + 1) % self.depth
        return lane


# ---- the schedule ----------------------------------------------------------------------------------------------------------
EVENTS = ("rerun_next", "sort", "radix_pairs", "particle_step", "reupload", "reset_learning")
DEPTHS = (2, 3, 4, 8)
SEEDS = (2,)               # the seeds the GPU test walks
EVENT_EVERY = 9            # frames between two events
# pairs the schedule must hold because a frame once differed from its alone twin there (none so far)
REGRESSION_ADJACENT = ()
REGRESSION_SAME_LANE = ()


@dataclass(frozen=True)
class Position:
    """One frame of a walked schedule."""
    index: int            # among the frames
    step: int             # among the steps
    kind: str
    lane: int
    stepped: bool         # drawn between a particle step and its inverse (the reference of an f32 kind is the stepped cloud's)
    rerun: bool           # under RERUN_EVERY_FRAME
    lane_prev: object     # the Position of the lane's previous frame, or None
    events: tuple         # the events between the previous frame and this one


def walk(steps, depth: int, rule: LaneRule = None, lane_last: dict = None, stepped: bool = False, first_index: int = 0):
    """The frames of `steps` as Positions. `rule`, `lane_last` and `stepped` carry a context's state from one pass to the next."""
    rule = rule or LaneRule(depth)
    lane_last = {} if lane_last is None else lane_last
    out, events, rerun = [], [], False
    for si, step in enumerate(steps):
        if step[0] != "frame":
            events.append(step)
            if step[0] == "rerun_next":
                rerun = True
            if step[0] == "particle_step":
                stepped = step[1] > 0
            continue
        lane = rule.place(step[1])
        pos = Position(first_index + len(out), si, step[1], lane, stepped, rerun, lane_last.get(lane), tuple(events))
        lane_last[lane] = pos
        out.append(pos)
        events, rerun = [], False
    return out


def barrier(events) -> bool:
    return any(e[0] != "rerun_next" for e in events)


def coverage(steps, depth: int):
    """(adjacent pairs, same-lane pairs, event placements) a schedule holds, pairs counted by the module docstring's rule."""
    frames = walk(steps, depth)
    adjacent, same_lane, placed = set(), set(), set()
    last_barrier = -1
    for i, f in enumerate(frames):
        if barrier(f.events):
            last_barrier = i
        for e in f.events:
            placed.add((e[0], by_name(f.kind).binning))
        if i and not barrier(f.events):
            adjacent.add((frames[i - 1].kind, f.kind))
        if f.lane_prev is not None and f.lane_prev.index >= last_barrier:
            same_lane.add((f.lane_prev.kind, f.kind))
    return adjacent, same_lane, placed


def required(depth: int):
    adjacent = {(a, b) for a in KIND_NAMES for b in KIND_NAMES if a != b} | set(REGRESSION_ADJACENT)
    same_lane = {(a, b) for a in KIND_NAMES for b in KIND_NAMES} | set(REGRESSION_SAME_LANE)
    placed = {(e, b) for e in EVENTS for b in ("scan", "sort")}
    return adjacent, same_lane, placed


_schedules = {}


def schedule(depth: int, seed: int):
    """A list of steps, ("frame", kind name) or an event (EVENTS), that holds every required pair and event placement for
    `depth`: a greedy walk over the uncovered pairs, ties broken by the seed, an event before every EVENT_EVERY-th frame."""
    if (depth, seed) in _schedules:
        return _schedules[(depth, seed)]
    rng = random.Random(seed * 100 + depth)
    need_adj, need_lane, need_ev = required(depth)
    need_adj, need_lane = set(need_adj), set(need_lane)
    todo = sorted(need_ev)
    rng.shuffle(todo)
    # the two particle steps: dt first, its inverse second, whichever binning each is placed before
    steps, rule, lane_last, prev = [], LaneRule(depth), {}, None
    stepped, frames, reuploads, sorts = False, 0, 0, 0
    scan_names = [k for k in KIND_NAMES if not is_sort(k)]
    sort_names = [k for k in KIND_NAMES if is_sort(k)]

    def emit_event(name):
        nonlocal stepped, reuploads, sorts, prev
        if name == "rerun_next":
            steps.append(("rerun_next",))
            return
        if name == "sort":
            steps.append(("sort", KIND_NAMES[(sorts * 5) % len(KIND_NAMES)]))
            sorts += 1
        elif name == "radix_pairs":
            steps.append(("radix_pairs",))
        elif name == "particle_step":
            steps.append(("particle_step", -STEP_DT if stepped else STEP_DT))
            stepped = not stepped
        elif name == "reupload":
            names = [c for c in CLOUDS if not (stepped and c == STEP_CLOUD)]   # (a fresh upload would undo the step)
            steps.append(("reupload", names[reuploads % len(names)]))
            reuploads += 1
        elif name == "reset_learning":
            steps.append(("reset_learning",))
        prev = None
        lane_last.clear()

    while need_adj or need_lane or todo or stepped:
        if len(steps) > 6000:
            raise RuntimeError(f"schedule(depth={depth}, seed={seed}) does not converge: {len(need_adj)} adjacent, {len(need_lane)} same-lane pairs left")
        names = KIND_NAMES
        if frames and frames % EVENT_EVERY == 0 and (todo or stepped):
            name, binning = todo.pop() if todo else ("particle_step", "scan")
            emit_event(name)
            names = sort_names if binning == "sort" else scan_names
        best, best_score = None, -1.0
        for k in names:
            lane = 0 if is_sort(k) else rule.next
            before = lane_last.get(lane)
            score = 10.0 * ((prev, k) in need_adj) + 10.0 * (before is not None and (before, k) in need_lane)
            score += sum(1 for p in need_lane if p[0] == k) / 12.0 + sum(1 for p in need_adj if p[0] == k) / 12.0
            score += rng.random() * 0.5
            if score > best_score:
                best, best_score = k, score
        lane = rule.place(best)
        need_adj.discard((prev, best))
        if lane in lane_last:
            need_lane.discard((lane_last[lane], best))
        lane_last[lane] = prev = best
        steps.append(("frame", best))
        frames += 1
    _schedules[(depth, seed)] = tuple(steps)
    return _schedules[(depth, seed)]
