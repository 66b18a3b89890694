"""What the hooks of include/bgs_diag.h refuse in common, as a table: hook x state of the context -> (status, the exact text
of bgs_last_error). The states are the ones the read-backs of the last frame tell apart: no frame yet, a bgs_sort or a
bgs_radix_sort_pairs since, frames in flight, an async frame behind them, at pipeline depth 1 and 2. Where the three
read-backs differ (the depth bgs_debug_frame_records insists on, the async frame bgs_debug_frame_leftovers accepts at
depth 1) the table says so, and a synchronous frame that every hook answers stands next to the refusals.

Only arguments and states are refused here: no call of this file reaches a kernel launch that could fail."""
import ctypes

import numpy as np
import pytest

import helpers as H
from bevy_gaussian_splatting_amd import CloudSettings, GaussianSplattingPlugin, View, _native

pytestmark = pytest.mark.gpu

OK, EINVAL = _native.BGS_OK, _native.BGS_EINVAL
HOOKS = ("records", "lists", "leftovers", "grids")
PREFIX = {"records": "frame records: ", "lists": "frame lists: ", "leftovers": "frame leftovers: ", "grids": "frame grids: "}
ANSWERS = (OK, None)
NO_FRAME = "no frame has been rendered (or a bgs_sort / bgs_radix_sort_pairs ran since)"
IN_FLIGHT = "frames are in flight"
DEPTH_1 = "the pipeline depth must be 1"
ASYNC = "the last frame was an async frame"
ASYNC_RING = "the last frame was an async frame at a pipeline depth other than 1"


def refuses(*texts):
    """One text per hook, in HOOKS' order (None: the hook answers)."""
    return {hook: ANSWERS if text is None else (EINVAL, PREFIX[hook] + text) for hook, text in zip(HOOKS, texts)}


def call(p, hook, info=True):
    """The hook's sizes-only call (bgs_debug_frame_grids: the whole report). Returns (status, bgs_last_error)."""
    lib, ctx = p._lib, p._ctx
    if hook == "records":
        out = _native.BgsFrameRecordsInfo()
        rc = lib.bgs_debug_frame_records(ctx, None, 0, None, 0, ctypes.byref(out) if info else None)
    elif hook == "lists":
        out = _native.BgsFrameListsInfo()
        rc = lib.bgs_debug_frame_lists(ctx, None, 0, None, 0, None, 0, ctypes.byref(out) if info else None)
    elif hook == "leftovers":
        out, layout = _native.BgsFrameLeftoversInfo(), _native.BgsScratchLayout()
        rc = lib.bgs_debug_frame_leftovers(ctx, None, 0, None, 0, ctypes.byref(layout), ctypes.byref(out) if info else None)
    else:
        out = np.zeros(_native.FRAME_GRIDS_WORDS, np.uint32)
        rc = lib.bgs_debug_frame_grids(ctx, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if info else None, out.size)
    return rc, lib.bgs_last_error(ctx).decode()


@pytest.fixture(scope="module")
def scene():
    """A context of the file's own with the 300-splat cloud resident, and the 64 x 64 view."""
    p = GaussianSplattingPlugin(0)
    h = p.upload(H.scene_like(300, 11))
    yield p, h, View.headless(64, 64), CloudSettings()
    h.free()
    p.close()


def _restore(p):
    while p.frames_in_flight():
        p.pipeline_pop()
    p.set_async(False)
    p.set_pipeline_depth(1)
    p.set_profiling(2)


def _sync_frame(p, h, v, s):
    p.render(h, v, s)


def _enqueue_async(p, h, v, s, depth):
    """Async frames on a ring of `depth` lanes until one is left in flight: a context completes the first frames of a kind
    inside their render call (AdaptiveState::LEARN_MAX of them at the most), and those are popped."""
    p.set_profiling(0)
    p.set_pipeline_depth(depth)
    p.set_async(True)
    for _ in range(8):
        early = p.learning_counters()["early_frames"]
        p.render(h, v, s, download=False)
        if p.learning_counters()["early_frames"] == early:
            assert p.frames_in_flight() >= 1
            return
        p.pipeline_pop()
    raise AssertionError("every async frame was completed inside its render call")


def _complete_async(p, h, v, s, depth):
    _enqueue_async(p, h, v, s, depth)
    while p.frames_in_flight():
        p.pipeline_pop()


def _after_sort(p, h, v, s):
    p.render(h, v, s)
    p.sort(h, v, s)


def _after_radix_sort_pairs(p, h, v, s):
    p.render(h, v, s)
    p.radix_sort_pairs(np.arange(100, dtype=np.uint32))


def _sync_frame_then_depth_2(p, h, v, s):
    p.render(h, v, s)
    p.set_pipeline_depth(2)


# state -> (how the context gets there, hook -> (status, text)); `grids` answers after anything that launched kernels
STATES = {
    "a synchronous frame": (_sync_frame, refuses(None, None, None, None)),
    "a synchronous frame, then depth 2": (_sync_frame_then_depth_2, refuses(DEPTH_1, None, None, None)),
    "a bgs_sort since": (_after_sort, refuses(NO_FRAME, NO_FRAME, NO_FRAME, None)),
    "a bgs_radix_sort_pairs since": (_after_radix_sort_pairs, refuses(NO_FRAME, NO_FRAME, NO_FRAME, None)),
    "a frame in flight at depth 1": (lambda *a: _enqueue_async(*a, 1), refuses(IN_FLIGHT, IN_FLIGHT, IN_FLIGHT, IN_FLIGHT)),
    "a frame in flight at depth 2": (lambda *a: _enqueue_async(*a, 2), refuses(DEPTH_1, IN_FLIGHT, IN_FLIGHT, IN_FLIGHT)),
    "an async frame at depth 1": (lambda *a: _complete_async(*a, 1), refuses(ASYNC, ASYNC, None, None)),
    "an async frame at depth 2": (lambda *a: _complete_async(*a, 2), refuses(DEPTH_1, ASYNC, ASYNC_RING, None)),
}


@pytest.mark.parametrize("state", list(STATES))
def test_the_read_backs_refuse_by_the_state_of_the_context(scene, state):
    p, h, v, s = scene
    reach, want = STATES[state]
    _restore(p)
    try:
        reach(p, h, v, s)
        got = {hook: call(p, hook) for hook in HOOKS}
        for hook in HOOKS:
            status, text = want[hook]
            assert got[hook][0] == status, (state, hook, got[hook])
            if text is not None:
                assert got[hook][1] == text, (state, hook)
    finally:
        _restore(p)


def test_the_read_backs_refuse_a_context_without_a_frame():
    with GaussianSplattingPlugin(0) as p:
        for hook in ("records", "lists", "leftovers"):
            assert call(p, hook) == (EINVAL, PREFIX[hook] + NO_FRAME), hook
        assert call(p, "grids") == (EINVAL, "frame grids: no frame has been run")


def test_a_missing_output_is_refused_ahead_of_the_state(scene):
    """Argument validation comes first: with a frame in flight the hooks name the missing output, not the frame."""
    p, h, v, s = scene
    texts = {"records": "frame records: info_out is NULL", "lists": "frame lists: info_out is NULL",
             "leftovers": "frame leftovers: layout_out and info_out must be non-NULL", "grids": "frame grids: out is NULL"}
    _restore(p)
    try:
        _enqueue_async(p, h, v, s, 1)
        for hook in HOOKS:
            assert call(p, hook, info=False) == (EINVAL, texts[hook]), hook
        small = np.zeros(_native.FRAME_GRIDS_WORDS - 1, np.uint32)
        rc = p._lib.bgs_debug_frame_grids(p._ctx, small.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), small.size)
        assert (rc, p._lib.bgs_last_error(p._ctx)) == (EINVAL, b"frame grids: out holds 15 words, the report is 16") and not small.any()
        assert call(p, "grids") == (EINVAL, "frame grids: " + IN_FLIGHT)
    finally:
        _restore(p)


# every hook of include/bgs_diag.h that takes a context -> what it says to a NULL one (bgs_last_error(NULL))
NULL_CONTEXT = {name: "ctx is NULL" for name in (
    "bgs_set_debug_flags", "bgs_learning_counters", "bgs_radix_sort_pairs", "bgs_hbm_probe", "bgs_selftest_ln_f32", "bgs_set_tile_trace",
    "bgs_graph_counters", "bgs_tile_order_counters", "bgs_selftest_tile_order", "bgs_selftest_pack", "bgs_debug_frame_records",
    "bgs_selftest_bin", "bgs_debug_frame_lists", "bgs_selftest_bucket_sort", "bgs_selftest_keygen_buckets", "bgs_selftest_raster",
    "bgs_debug_frame_leftovers", "bgs_set_grid_cap", "bgs_debug_frame_grids")}
NULL_CONTEXT["bgs_adaptive_counters"] = "NULL argument"


def test_every_hook_refuses_a_null_context():
    lib = _native.load()
    first = _native.EXPORTED_SYMBOLS.index("bgs_set_debug_flags")
    diag = [(name, args) for name, _, args in _native.PROTOTYPES[first:] if args and args[0] is ctypes.c_void_p]
    assert sorted(name for name, _ in diag) == sorted(NULL_CONTEXT)
    for name, args in diag:
        zeros = [None if hasattr(t, "contents") or t is ctypes.c_void_p else 0 for t in args[1:]]
        assert getattr(lib, name)(None, *zeros) == EINVAL, name
        assert lib.bgs_last_error(None).decode() == NULL_CONTEXT[name], name
