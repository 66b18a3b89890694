"""What a frame leaves for the frame behind it (bgs_debug_frame_leftovers; tests/frame_leftover_cases.py): integer work, every
comparison is an equality or an order.

  The rasteriser's clean-up leaves the lane's scratch region zero outside the frame's own Control block, for every case.
  The case's twin under BGS_DEBUG_NO_RASTER_CLEANUP (memset before, nothing cleaned after) shows what the frame published:
  words in every region the case is named for, none at or past what the clean-up zeroes or what the tile geometry allows.
  Frames that differ, back to back on one context, each bit-equal to the same frame alone in a fresh context.
  The pinned host Control the clean-up writes is the device's block, and the twin's copy; the quantile keys of both producers
  are the quantiles of the frame's sorted list.
  The hook's refusals, and that a read-back which finds dirty words takes the lane's clean flag back."""
import numpy as np
import pytest

import frame_leftover_cases as L
import helpers as H
from bevy_gaussian_splatting_amd import GaussianSplattingPlugin, _native
from bevy_gaussian_splatting_amd.settings import SortMode

pytestmark = pytest.mark.gpu

PLAN_FIELDS = ("bucket", "kept", "places", "large", "wide", "wide_bin", "keygen_tile", "bucket_sub", "n", "ntiles", "binning", "culled_tail")
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ctx():
    """One context for the cases, with the clouds they share resident; the session's plugin is left alone."""
    p = GaussianSplattingPlugin(0)
    p.handles = {}
    yield p
    for h in p.handles.values():
        h.free()
    p.close()


def _handle(p, case):
    key = (case.n, case.drawable, case.budget)
    if key not in p.handles:
        p.handles[key] = p.upload(L.cloud_of(case))
    return p.handles[key]


def _restore(p):
    p.set_async(False)
    p.set_graphs(False)
    p.set_debug_flags(0)
    p.set_profiling(2)
    p.set_pipeline_depth(1)
    p.set_binning("scan")


def run_case(p, case, extra_flags=0, handle=None, reset=True):
    """The case's frames on context p; what the last one left. `draw_count` as the frame's kernels read it, `entries` the
    first draw_count sorted entries, `lists` the binning hook's output (None for an async frame: it refuses those)."""
    _restore(p)
    if reset:
        p.reset_adaptive_state()
    own = handle is None
    h = _handle(p, case) if own else handle
    v, s = case.view(), case.settings()
    dse = None
    try:
        p.set_pipeline_depth(case.depth)
        if case.kept:
            dse = p.device_sorted_entries(1, h)
            p.sort(h, case.view(0.4), s, download=False, into=dse.chunk(0))   # another camera's order: culled entries are skipped
        chunk = dse.chunk(0) if dse else None
        p.set_debug_flags(case.flags | extra_flags)
        before = p.adaptive_counters()
        ordered = p.tile_order_counters()[1]
        replays = p.graph_counters()[1]
        img = None
        if extra_flags & L.NO_RASTER_CLEANUP:
            # a frame behind one that cleaned up takes no memset, whatever its own flags: one frame ends the clean state, and
            # what it taught the context is forgotten, so that the frames below start where the clean-up run's did
            p.render(h, v, s, download=False, entries=chunk)
            p.reset_adaptive_state()
        for f in range(case.sort_frames):
            p.set_binning("sort")
            p.render(h, v, s, download=False, entries=chunk)
            p.set_binning("scan")
        for f in range(case.warm + 1):
            if case.graphs:
                p.set_profiling(0)
                p.set_async(True)
                p.set_graphs(True)
                p.render(h, v, s, download=False, entries=chunk)
                ptr, _ = p.pipeline_pop()
                img = p.download(ptr, np.empty((v.height, v.width, 4), np.float32))
            else:
                img = p.render(h, v, s, entries=chunk)
        out = p.debug_frame_leftovers()
        off = H.control_offsets()
        ctl = out["control"]
        d = 0 if ctl[off["sort_overflow"]] else int(ctl[off["draw_count"]])
        res = {"out": out, "img": img, "stats": p.stats(), "draw_count": d, "entries": p.draw_list()[:d].copy(),
               "lists": None if case.graphs else p.debug_frame_lists(), "replays": p.graph_counters()[1] - replays, "ordered": p.tile_order_counters()[1] - ordered,
               "counters": {k: p.adaptive_counters()[k] - before[k] for k in before if k.startswith("reruns")}}
    finally:
        _restore(p)
        if dse:
            dse.free()
    return res


def _regions(layout):
    """[(name, first word, words)] of the whole scratch region, in address order."""
    names = ["ctl0"] + [r[4:] for r in _native.BgsScratchLayout.REGIONS]
    offs = [0] + [int(getattr(layout, r)) for r in _native.BgsScratchLayout.REGIONS] + [int(layout.bytes)]
    return [(names[i], offs[i] // 4, (offs[i + 1] - offs[i]) // 4) for i in range(len(names))]


def _own_words(out):
    first = int(out["layout"].off_ctl1) // 4 if out["ctl_block"] else 0
    return first, first + H.control_offsets()["words"]


def assert_clean(what, out):
    """Nothing outside the frame's own Control block: region by region, the first offending word named."""
    scratch = out["scratch"].copy()
    a, b = _own_words(out)
    scratch[a:b] = 0
    for name, first, words in _regions(out["layout"]):
        bad = np.nonzero(scratch[first:first + words])[0]
        assert not len(bad), f"{what}: region {name} word {bad[0]} holds 0x{int(scratch[first + bad[0]]):08x} ({len(bad)} words of the region are not zero)"
    other = int(out["layout"].off_ctl1) // 4 if not out["ctl_block"] else 0
    assert not out["scratch"][other:other + (b - a)].any(), f"{what}: the lane's other Control block"
    assert out["dirty_words"] == 0 and out["scratch_clean"] == 1 and out["scratch_reset"] == 0 and out["raster_cleans"] == 1, \
        f"{what}: dirty_words {out['dirty_words']} scratch_clean {out['scratch_clean']} raster_cleans {out['raster_cleans']}"


_RUNS = {}


def both(ctx, name):
    """The case's clean-up frame and its BGS_DEBUG_NO_RASTER_CLEANUP twin, run once for the tests that share them."""
    if name not in _RUNS:
        case = L.by_name(name)
        _RUNS[name] = (run_case(ctx, case), run_case(ctx, case, L.NO_RASTER_CLEANUP))
    return _RUNS[name]


# ---- 1. the clean-up leaves the scratch clean ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_the_clean_up_leaves_the_scratch_clean(ctx, name):
    case = L.by_name(name)
    run, _ = both(ctx, name)
    out = run["out"]
    for k, want in case.expect.items():
        assert out[k] == want, f"{name}: the frame ran with {k} = {out[k]}, the case is written for {want}"
    if case.reruns:
        assert run["counters"][case.reruns] >= 1, f"{name}: {run['counters']}"
    if case.graphs:
        assert run["replays"] >= 1
    assert (run["ordered"] >= 1) == case.ordered, f"{name}: {run['ordered']} frames drawn in cost order"
    assert out["n"] == case.n and out["ntiles"] == -(-case.size[0] // 16) * -(-case.size[1] // 16)
    print(f"{name}: D {run['draw_count']}, ctl block {out['ctl_block']}, plan " + ", ".join(f"{k} {out[k]}" for k in PLAN_FIELDS))
    assert_clean(name, out)


# ---- 2. each case really uses the words it is named for ------------------------------------------------------------------------
@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_the_twin_s_footprint_lies_inside_both_bounds(ctx, name):
    case = L.by_name(name)
    run, twin = both(ctx, name)
    out, d = twin["out"], twin["draw_count"]
    assert out["raster_cleans"] == 0 and out["scratch_clean"] == 0 and out["scratch_reset"] == 0
    for k in ("bucket", "kept", "places", "large", "wide", "wide_bin", "keygen_tile", "n", "ntiles"):
        assert out[k] == run["out"][k], f"{name}: the twin ran with {k} = {out[k]}, the clean-up frame with {run['out'][k]}"
    assert d == run["draw_count"]
    used, zeroed = L.words_used(out, d), L.words_zeroed(out, d)
    scratch, lay = out["scratch"], out["layout"]
    chain = {}
    for region in L.CHAIN_REGIONS:
        for p in range(4 if region == "depth" else 1):
            first, words = L.region_words(lay, region, p)
            nz = np.nonzero(scratch[first:first + words])[0]
            top = int(nz[-1]) + 1 if len(nz) else 0
            live = region != "depth" or p < used["passes"]
            print(f"{name} {region}{p if region == 'depth' else ''}: {len(nz)} words, highest index + 1 = {top}, used {used[region] if live else 0}, "
                  f"zeroed {zeroed[region] if (region != 'depth' or p < zeroed['passes']) else 0}")
            assert top <= (zeroed[region] if (region != "depth" or p < zeroed["passes"]) else 0), \
                f"{name}: {region} pass {p}: word {top - 1} is published, the clean-up zeroes {zeroed[region]} words of {zeroed['passes']} passes"
            assert top <= (used[region] if live else 0), f"{name}: {region} pass {p}: word {top - 1} is published, the tile geometry allows {used[region]}"
            if live and region in case.regions:
                assert len(nz), f"{name}: the case is named for the {region} words (pass {p}) and its twin published none"
            chain[(region, p)] = (first, words)
    # nothing anywhere else: the other regions belong to the instance-sort pipeline, and the other Control block is the memset's
    rest = scratch.copy()
    a, b = _own_words(out)
    rest[a:b] = 0
    for first, words in chain.values():
        rest[first:first + words] = 0
    for rname, first, words in _regions(lay):
        bad = np.nonzero(rest[first:first + words])[0]
        assert not len(bad), f"{name}: region {rname} word {bad[0]} is written by a scan frame"
    assert out["dirty_words"] == int(np.count_nonzero(scratch)) - int(np.count_nonzero(scratch[a:b]))
    assert (out["dirty_words"] > 0) == bool(case.regions)


# ---- 3. the host's Control is the device's ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_the_pinned_control_is_the_device_block_and_the_twin_s(ctx, name):
    case = L.by_name(name)
    run, twin = both(ctx, name)
    off = H.control_offsets()
    out = run["out"]
    a, b = _own_words(out)
    dev, host, thost = out["scratch"][a:b], out["control"], twin["out"]["control"]
    hw, ct = off["header_words"], off["coarse_total"]
    assert hw == 12
    assert np.array_equal(host[:hw - 2], dev[:hw - 2]), f"{name}: header words host {host[:hw - 2].tolist()} device {dev[:hw - 2].tolist()}"
    assert np.array_equal(host[:hw - 2], thost[:hw - 2]), f"{name}: header words host {host[:hw - 2].tolist()} twin {thost[:hw - 2].tolist()}"
    assert host[off["error"]] == 0
    assert np.array_equal(host[ct:ct + 256], dev[ct:ct + 256]) and np.array_equal(host[ct:ct + 256], thost[ct:ct + 256]), f"{name}: coarse_total"
    if run["lists"] is not None:
        totals = np.zeros(256, np.uint32)
        totals[:len(run["lists"]["totals"])] = run["lists"]["totals"]
        if run["draw_count"]:   # (an empty draw list launches no bin_kernel; the hook reports no lists)
            assert np.array_equal(host[ct:ct + 256], totals), f"{name}: coarse_total is not the lists hook's totals"
        else:
            assert not host[ct:ct + 256].any()
    assert int(host[off["strip_tiles"]]) == run["stats"]["strip_tiles"]
    print(f"{name}: strip_tiles {int(host[off['strip_tiles']])}, saturated_tiles_prev 0x{int(host[off['saturated_tiles_prev']]):08x}")
    # strip workgroups draw tiles in the case that is named for them, and never without being appended to the grid (a 1080p
    # frame at pipeline depth 1 gets them by itself once the supertile level has risen)
    if case.expect.get("strips_appended"):
        assert host[off["strip_tiles"]] > 0, f"{name}: strips appended, and no tile drawn by them"
    if not out["strips_appended"]:
        assert host[off["strip_tiles"]] == 0, f"{name}: strip_tiles {host[off['strip_tiles']]} without strip workgroups"
    # the saturation share: of the cost plane behind the frame's tile order; exactly "none" for a frame without an order
    sat = int(host[off["saturated_tiles_prev"]])
    if case.ordered:
        assert sat != NONE and sat <= 0x7FFF, f"{name}: saturated_tiles_prev 0x{sat:08x}"
    else:
        assert sat == NONE, f"{name}: saturated_tiles_prev 0x{sat:08x} without an order"
    # (the twin's copy holds its device block's words there: nothing on the device writes them)
    assert thost[off["strip_tiles"]] == 0 and thost[off["saturated_tiles_prev"]] == 0


# ---- 4. splitters from both producers ------------------------------------------------------------------------------------------
def _key_xor(case):
    return NONE if (not case.kept and case.sort_mode in (int(SortMode.Rayon), int(SortMode.Std))) else 0


@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_both_producers_leave_the_quantiles_of_the_sorted_list(ctx, name):
    case = L.by_name(name)
    run, twin = both(ctx, name)
    off = H.control_offsets()
    sp, full = off["splitters"], off["bucket_max_keys"]
    out, d = run["out"], run["draw_count"]
    nbk = 256 * out["split_sub_out"]
    want = L.quantile_keys(run["entries"], d, nbk, _key_xor(case))
    got = out["control"][sp:sp + nbk]
    bad = np.nonzero(got != want)[0]
    assert not len(bad), f"{name}: clean-up key {bad[0]} of {nbk} is 0x{int(got[bad[0]]):08x}, the quantile of D = {d} is 0x{int(want[bad[0]]):08x} ({len(bad)} differ)"
    assert np.array_equal(run["entries"], twin["entries"]), f"{name}: the twin's sorted list is not the clean-up frame's"
    # splitter_kernel: launched behind frames of four digit places on a cloud that is not empty (enqueue_frame), a whole table
    tgot = twin["out"]["control"][sp:sp + full]
    tsub = twin["out"]["split_sub_out"]
    if twin["out"]["places"] == 4 and case.n > 0:
        twant = np.full(full, NONE, np.uint32)
        twant[:256 * tsub] = L.quantile_keys(twin["entries"], twin["draw_count"], 256 * tsub, _key_xor(case))
        bad = np.nonzero(tgot != twant)[0]
        assert not len(bad), f"{name}: splitter_kernel key {bad[0]} is 0x{int(tgot[bad[0]]):08x}, expected 0x{int(twant[bad[0]]):08x} ({len(bad)} differ)"
        if tsub == out["split_sub_out"]:
            assert np.array_equal(tgot[:nbk], got), f"{name}: the two producers disagree"
    else:
        assert not tgot.any(), f"{name}: a frame of {twin['out']['places']} places leaves no table behind the memset path"


@pytest.mark.parametrize("mode", [SortMode.Radix, SortMode.Rayon, SortMode.Std])
def test_quantiles_below_at_and_above_the_table_size(ctx, mode):
    """D below, at and above nbk, at sub 1 and at 3 and 5 (what a small cloud can be made to ask for: BGS_DEBUG_SPLIT_SUB_3 /
    _5; sub 2, which a hint past 524 k pairs asks for, is the cases split_sub_2_*), each sort mode; a BINNING_SORT frame's
    splitter_kernel the same way."""
    off = H.control_offsets()
    sp = off["splitters"]
    xor = 0 if mode == SortMode.Radix else NONE
    for n, flags, sub in ((200, 0, 1), (256, 0, 1), (255, 0, 1), (257, 0, 1), (3000, 0, 1), (700, L.SPLIT_SUB_3, 3), (768, L.SPLIT_SUB_3, 3),
                          (5000, L.SPLIT_SUB_3, 3), (1279, L.SPLIT_SUB_5, 5), (1280, L.SPLIT_SUB_5, 5), (6000, L.SPLIT_SUB_5, 5)):
        # Rayon / Std draw every splat: D = n exactly
        case = L.Case(f"q_{n}", n, flags=flags | L.NO_BUCKET_SORT, sort_mode=int(mode))
        h = ctx.upload(L.cloud_of(case))
        try:
            run = run_case(ctx, case, handle=h)
            twin = run_case(ctx, case, L.NO_RASTER_CLEANUP, handle=h)
            ctx.set_binning("sort")
            ctx.set_debug_flags(case.flags)
            ctx.render(h, case.view(), case.settings(), download=False)
            sort_out = ctx.debug_frame_leftovers()
            sort_entries = ctx.draw_list()
        finally:
            _restore(ctx)
            h.free()
        d = run["draw_count"]
        assert run["out"]["split_sub_out"] == sub and (mode == SortMode.Radix or d == n)
        print(f"{mode.name} n {n}: D {d}, nbk {256 * sub}")
        want = L.quantile_keys(run["entries"], d, 256 * sub, xor)
        assert (np.diff(want.astype(np.int64)) >= 0).all()
        assert np.array_equal(run["out"]["control"][sp:sp + 256 * sub], want), f"{mode.name} n {n}: the clean-up's keys"
        full = np.full(off["bucket_max_keys"], NONE, np.uint32)
        full[:256 * sub] = want
        assert np.array_equal(twin["out"]["control"][sp:sp + full.size], full), f"{mode.name} n {n}: splitter_kernel behind a scan frame"
        assert sort_out["binning"] == 1 and sort_out["raster_cleans"] == 0 and sort_out["scratch_clean"] == 0
        sd = int(sort_out["control"][off["draw_count"]])
        assert sd == d and np.array_equal(sort_entries[:sd], run["entries"])
        assert np.array_equal(sort_out["control"][sp:sp + full.size], full), f"{mode.name} n {n}: splitter_kernel behind a BINNING_SORT frame"


def test_a_frame_of_fewer_than_four_places_leaves_no_table_on_the_memset_path(ctx):
    """enqueue_frame launches splitter_kernel behind frames of four digit places only (store_splitters wants 4): a 16-bit
    BINNING_SORT frame's pinned Control holds the memset's zeros there — and the clean-up of a 16-bit scan frame writes its
    quantiles all the same (the host does not read them)."""
    off = H.control_offsets()
    case = L.Case("sort_16", 3000, bits=16)
    h = ctx.upload(L.cloud_of(case))
    try:
        _restore(ctx)
        ctx.set_binning("sort")
        ctx.render(h, case.view(), case.settings(), download=False)
        out = ctx.debug_frame_leftovers()
    finally:
        _restore(ctx)
        h.free()
    assert out["places"] == 2 and out["binning"] == 1
    assert not out["control"][off["splitters"]:off["splitters"] + off["bucket_max_keys"]].any()


# ---- 5. frames that differ, back to back ---------------------------------------------------------------------------------------
# (the big frame draws every splat: 15 depth tiles and 30 bin tiles, whose words the frames behind it start on)
BIG = L.Case("seq_big_32", 30000, flags=L.NO_BUCKET_SORT, sort_mode=int(SortMode.Rayon), expect={"bucket": 0, "places": 4})
SEQUENCE = (
    BIG,
    L.Case("seq_small_bucket", 3000, flags=L.GUESSED_SPLITTERS, expect={"bucket": 1}),
    L.Case("seq_kept", 9000, kept=True, expect={"kept": 1}),
    L.Case("seq_16", 20000, flags=L.NO_BUCKET_SORT, bits=16, size=(80, 48), expect={"bucket": 0, "places": 2}),
    L.Case("seq_voided", 5000, drawable=0, flags=L.NO_BUCKET_SORT),
    BIG,
)


@pytest.fixture(scope="module")
def alone():
    """Every frame of the sequence drawn alone in a fresh context: its image and its sorted list."""
    want = {}
    for case in SEQUENCE:
        if case.name not in want:
            with GaussianSplattingPlugin(0) as p:
                h = p.upload(L.cloud_of(case))
                run = run_case(p, case, handle=h)
                h.free()
            for k, v in case.expect.items():
                assert run["out"][k] == v, (case.name, k)
            assert_clean(case.name + " alone", run["out"])
            want[case.name] = (run["img"], run["entries"])
    return want


@pytest.mark.parametrize("graphs", [False, True])
def test_frames_that_differ_back_to_back(alone, graphs):
    """No reset between the frames: each starts on what the one before it left. With graphs on every frame is drawn three
    times in a row (a lane's graph of a kind and parity replays on the third), and replays are counted."""
    import dataclasses
    replays = flagged = 0
    with GaussianSplattingPlugin(0) as p:
        handles = {c.name: p.upload(L.cloud_of(c)) for c in SEQUENCE}
        for i, case in enumerate(SEQUENCE):
            for rep in range(3 if graphs else 1):
                run = run_case(p, dataclasses.replace(case, graphs=graphs), handle=handles[case.name], reset=False)
                what = f"frame {i} ({case.name}) graphs {graphs} repeat {rep}"
                for k, v in case.expect.items():
                    assert run["out"][k] == v, (what, k, run["out"][k])
                assert_clean(what, run["out"])
                img, entries = alone[case.name]
                assert run["img"].tobytes() == img.tobytes(), f"{what}: the image is not the frame's alone"
                assert np.array_equal(run["entries"], entries), f"{what}: the sorted list is not the frame's alone"
                replays += run["replays"]
                flagged += run["out"]["graph_replay"]
        for h in handles.values():
            h.free()
    print(f"graphs {graphs}: {replays} replays counted, {flagged} read-backs of a replayed frame")
    assert (replays > 0 and flagged > 0) if graphs else (replays == 0 and flagged == 0)


# ---- 6. refusals, and the flag a dirty read-back takes back ------------------------------------------------------------------
def test_the_hook_refuses_what_it_cannot_answer_and_takes_a_dirty_flag_back():
    import ctypes
    off = H.control_offsets()
    case = L.Case("refusals", 9000, flags=L.NO_BUCKET_SORT)
    v, s = case.view(), case.settings()
    with GaussianSplattingPlugin(0) as p:
        with pytest.raises(_native.BgsError, match="frame leftovers: no frame has been rendered"):
            p.debug_frame_leftovers()
        h = p.upload(L.cloud_of(case))
        p.set_debug_flags(case.flags)
        # a context's first frame: no order, no cost plane behind it
        want = p.render(h, v, s)
        out = p.debug_frame_leftovers()
        assert_clean("first frame", out)
        assert out["control"][off["saturated_tiles_prev"]] == NONE
        p.set_debug_flags(case.flags | L.NO_TILE_COST)
        p.render(h, v, s)
        assert p.debug_frame_leftovers()["control"][off["saturated_tiles_prev"]] == NONE
        p.set_debug_flags(case.flags)
        # capacities: nothing is written
        info, lay = _native.BgsFrameLeftoversInfo(), _native.BgsScratchLayout()
        scratch, ctl = np.full(len(out["scratch"]), 0xA5A5A5A5, np.uint32), np.full(len(out["control"]), 0xA5A5A5A5, np.uint32)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = p._lib.bgs_debug_frame_leftovers(p._ctx, vp(scratch), scratch.nbytes - 4, vp(ctl), ctl.nbytes, ctypes.byref(lay), ctypes.byref(info))
        assert rc == _native.BGS_EINVAL and b"host_scratch holds" in p._lib.bgs_last_error(p._ctx)
        rc = p._lib.bgs_debug_frame_leftovers(p._ctx, vp(scratch), scratch.nbytes, vp(ctl), ctl.nbytes - 4, ctypes.byref(lay), ctypes.byref(info))
        assert rc == _native.BGS_EINVAL and b"host_control holds" in p._lib.bgs_last_error(p._ctx)
        rc = p._lib.bgs_debug_frame_leftovers(p._ctx, vp(scratch), scratch.nbytes, None, 0, ctypes.byref(lay), ctypes.byref(info))
        assert rc == _native.BGS_EINVAL and b"host_control holds" in p._lib.bgs_last_error(p._ctx)
        assert (scratch == 0xA5A5A5A5).all() and (ctl == 0xA5A5A5A5).all()
        rc = p._lib.bgs_debug_frame_leftovers(p._ctx, None, 0, None, 0, None, ctypes.byref(info))
        assert rc == _native.BGS_EINVAL and b"layout_out and info_out" in p._lib.bgs_last_error(p._ctx)
        # a bgs_sort / bgs_radix_sort_pairs since the last frame
        p.sort(h, v, s)
        with pytest.raises(_native.BgsError, match="no frame has been rendered"):
            p.debug_frame_leftovers()
        p.render(h, v, s)
        p.radix_sort_pairs(np.arange(100, dtype=np.uint32))
        with pytest.raises(_native.BgsError, match="no frame has been rendered"):
            p.debug_frame_leftovers()
        # frames in flight, and an async frame on a ring of lanes
        p.set_profiling(0)
        p.set_pipeline_depth(2)
        p.set_async(True)
        for _ in range(8):   # (past the learning phase, which completes a frame inside its render call)
            p.render(h, v, s, download=False)
            if p.frames_in_flight() == 2:
                p.pipeline_pop()
        if p.frames_in_flight():
            with pytest.raises(_native.BgsError, match="frames are in flight"):
                p.debug_frame_leftovers()
        while p.frames_in_flight():
            p.pipeline_pop()
        with pytest.raises(_native.BgsError, match="async frame at a pipeline depth other than 1"):
            p.debug_frame_leftovers()
        p.set_async(False)
        p.set_pipeline_depth(1)
        p.set_profiling(2)
        # a frame that cleans nothing: the lane does not believe its scratch clean, and the frame behind it is right
        p.set_debug_flags(case.flags | L.NO_RASTER_CLEANUP)
        assert p.render(h, v, s).tobytes() == want.tobytes()
        out = p.debug_frame_leftovers()
        assert out["scratch_clean"] == 0 and out["dirty_words"] > 0 and out["scratch_reset"] == 0
        p.set_debug_flags(case.flags)
        assert p.render(h, v, s).tobytes() == want.tobytes()
        assert_clean("the frame behind a frame that cleaned nothing", p.debug_frame_leftovers())
        h.free()
