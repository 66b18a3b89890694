"""The second and later trips of the persistent kernels' tile loops. Every stage pin runs at a few thousand splats, where the
default grids (num_cus * 4 or * 3 workgroups, or what the draw hint asks for) cover every tile: each workgroup takes one
ticket and leaves through `single_shot`. Under bgs_set_grid_cap(1 .. 3) the same small shapes walk every loop several times
— keygen_kernel (ordered instantiations), onesweep_kernel, project_kernel, bin_kernel, project_emit_kernel, the kept-order
compaction — and are held against the exact references the stage pins own (numpy's stable argsort, oracle.sort,
bucket_stage_cases, helpers.twin_project, bin_stage_cases, the kept-order host reference). Integer work and bit patterns:
every comparison is equality.

Every test asserts, from bgs_debug_frame_grids (or the hook's own report), that the kernel it is about launched fewer
workgroups than it had tiles BEFORE it compares anything, and that Control::error — the look-back watchdog — is 0 after:
a capped frame that completes without BGS_EINTERNAL has not tripped it (finish_lane, check_watchdog).

The kept-order compaction's tail is read back from the lane (bgs_debug_frame_grids names its device address) and compared
with the host reference: the skipped entries in list order, their index parked as entries_math.h's entry_parked_index does.

Shapes and caps: tests/grid_cap_cases.py; measured grids and the mutation table: profiles/grid_cap.md."""
import numpy as np
import pytest

import bin_stage_cases as B
import bucket_stage_cases as C
import grid_cap_cases as G
import test_bin_stage_gpu as TBin
import test_bucket_stage_gpu as TBucket
import test_vertex_stage_gpu as TVertex
import vertex_stage_cases as VC
from bevy_gaussian_splatting_amd import (
    CloudSettings, GaussianSplattingPlugin, PlanarGaussian3d, RadixSortDepthBits, RasterizeMode, SortMode, View, _native,
    random_gaussians_3d_seeded)
from bevy_gaussian_splatting_amd.plugin import SORT_ENTRY_DTYPE

pytestmark = pytest.mark.gpu
CULLED = 0xFFFFFFFF


@pytest.fixture(autouse=True)
def _uncapped_after(plugin):
    """The session's plugin goes back to what the other modules expect, whatever a test here left."""
    plugin.set_grid_cap(0)
    yield
    plugin.set_grid_cap(0)
    plugin.set_debug_flags(0)
    plugin.set_async(False)
    plugin.set_graphs(False)
    plugin.set_profiling(2)
    plugin.set_pipeline_depth(1)
    plugin.set_binning("scan")


def _assert_looped(grids, kernel, what, cap):
    print(f"{what}: cap {cap} -> {kernel} {grids[kernel][0]} workgroups / {grids[kernel][1]} tiles   {grids}")
    assert grids["cap"] == cap, f"{what}: the launches ran under cap {grids['cap']}, not {cap}"
    if cap:
        assert G.looped(grids, kernel), f"{what}: {kernel} ran {grids[kernel][0]} workgroups for {grids[kernel][1]} tiles: no workgroup took a second tile"
        assert grids[kernel][0] == cap


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- digit passes alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", (1, 2, 3, 4))
@pytest.mark.parametrize("n", G.PAIR_SIZES)
def test_onesweep_tile_loop_sorts_as_numpy(plugin, n, passes):
    for family, keys in G.key_families(n, passes, n + passes).items():
        order = np.argsort(keys, kind="stable").astype(np.uint32)
        for cap in (0,) + G.CAPS:
            plugin.set_grid_cap(cap)
            out = plugin.radix_sort_pairs(keys, passes)          # (raises on Control::error)
            _assert_looped(plugin.debug_frame_grids(), "depth", f"n {n} passes {passes} {family}", cap)
            assert np.array_equal(out["index"], order), f"n {n} passes {passes} {family} cap {cap}: index"
            assert np.array_equal(out["key"], keys[order]), f"n {n} passes {passes} {family} cap {cap}: key"


def test_onesweep_large_tile_loop_on_keys_with_many_ties(plugin):
    n = G.LARGE_PAIRS
    keys = G.key_families(n, 4, 5)["random with ties"]
    order = np.argsort(keys, kind="stable").astype(np.uint32)
    plugin.set_grid_cap(3)
    out = plugin.radix_sort_pairs(keys, 4)
    grids = plugin.debug_frame_grids()
    _assert_looped(grids, "depth", f"n {n} large tiles", 3)
    assert grids["depth"][1] == -(-n // G.LARGE_TILE)
    assert np.array_equal(out["index"], order) and np.array_equal(out["key"], keys[order])


# ---- sort through keygen, onesweep path ------------------------------------------------------------------------------
def _half_outside(n, seed):
    """Splats spread over 1.55 x the view's NDC square: about half lie outside the frustum (SortMode::Radix culls them)."""
    v = View.headless(320, 180, yaw=0.35)
    return VC.screen_cloud(v, n, seed, spread=1.55), v


def _check_sorted(plugin, oracle, h, c, v, s, what, kernels):
    """Returns (oracle.sort's list, the caps that ran). The passes sort the DRAWABLE pairs only, so the caps are those below
    the tile count the uncapped run reports for every kernel named: no list is compared under a cap that makes no loop."""
    ref = oracle.sort(c, v, s)
    caps = G.CAPS
    for cap in (0,) + G.CAPS:
        if cap and cap not in caps:
            continue
        plugin.set_grid_cap(cap)
        got = plugin.sort(h, v, s)
        grids = plugin.debug_frame_grids()
        if cap == 0:
            caps = tuple(k for k in G.CAPS if all(k < grids[kernel][1] for kernel in kernels))
            assert caps[:2] == G.CAPS[:2], f"{what}: {grids}"        # caps 1 and 2 always loop
        for kernel in kernels:
            _assert_looped(grids, kernel, what, cap)
        assert plugin.stats()["sort_path"] == "onesweep", what
        assert np.array_equal(got["key"], ref["key"]), f"{what} cap {cap}: keys"
        assert np.array_equal(got["index"], ref["index"]), f"{what} cap {cap}: indices (the culled tail included)"
    return ref, caps


@pytest.mark.parametrize("mode,bits", [(SortMode.Radix, 16), (SortMode.Radix, 24), (SortMode.Radix, 32), (SortMode.Rayon, 32), (SortMode.Std, 24),
                                       (SortMode.NONE, 16)], ids=["radix16", "radix24", "radix32", "rayon32", "std24", "none16"])
@pytest.mark.parametrize("n", G.SORT_SIZES)
def test_keygen_and_passes_loop_to_the_oracles_list(plugin, oracle, n, mode, bits):
    c, v = _half_outside(n, 900 + n % 89)
    s = CloudSettings(sort_mode=mode, radix_sort_depth_bits=RadixSortDepthBits(bits))
    plugin.set_debug_flags(G.NO_BUCKET_SORT)
    h = plugin.upload(c)
    try:
        ref, caps = _check_sorted(plugin, oracle, h, c, v, s, f"n {n} {mode.name} {bits} bits",
                                  ("front",) if mode == SortMode.NONE else ("front", "depth"))     # (SortMode::None: index order, no digit pass)
        # every cap at every shape but one: SortMode::Radix culls half of 5 x 2048 + 1 splats, which leaves the passes 3 tiles
        assert caps == G.CAPS or (mode == SortMode.Radix and n == G.SORT_SIZES[0] and caps == G.CAPS[:2]), caps
        if mode == SortMode.Radix and bits == 32:
            drawn = int((ref["key"] != CULLED).sum())
            assert 0.35 * n < drawn < 0.65 * n, (drawn, n)
    finally:
        h.free()


def test_keygen_long_tiles_and_passes_loop_to_the_oracles_list(plugin, oracle):
    n = G.BIG_SORT
    c, v = _half_outside(n, 77)
    plugin.set_debug_flags(G.NO_BUCKET_SORT)
    h = plugin.upload(c)
    try:
        ref = oracle.sort(c, v, CloudSettings())
        plugin.set_grid_cap(3)
        got = plugin.sort(h, v, CloudSettings())
        grids = plugin.debug_frame_grids()
        _assert_looped(grids, "front", "n 2^19 + 4097", 3)
        _assert_looped(grids, "depth", "n 2^19 + 4097", 3)
        assert grids["front"][1] == -(-n // 4096)
        assert np.array_equal(got["key"], ref["key"]) and np.array_equal(got["index"], ref["index"])
    finally:
        h.free()


# ---- keygen's ordered bucket placement -------------------------------------------------------------------------------
def _placement(plugin, oracle, n, mode, alones):
    scene = TBucket._tables(oracle, n, mode)
    cloud, view, settings, entries, kk, drawable, d, kd, kd_other = scene
    threads_items = {alone: C.tile_shape(n, alone) for alone in alones}
    tables = (("quantiles", 1), ("runs", 5)) if n < (1 << 19) else (("quantiles", 3),)
    handle = plugin.upload(cloud)
    try:
        for alone in alones:
            tiles = -(-n // (threads_items[alone][0] * threads_items[alone][1]))
            assert tiles >= 5
            for cap in (0,) + G.CAPS:
                plugin.set_grid_cap(cap)
                # (the quantile table first: its placement feeds the sort below. One table at the 2^19 size: a run moves 50 MB)
                for t, (kind, sub) in enumerate(tables):
                    tab = C.table(kind, sub, kd, kd_other)
                    what = f"n {n} {mode} ordered alone {alone} cap {cap} table '{kind}' sub {sub}"
                    assert not cap or cap < tiles, what
                    out = TBucket._check_run(plugin, handle, scene, what, tab, sub, 0, 1, alone, blocks=cap or tiles)
                    print(f"{what}: {out['blocks']} workgroups / {tiles} tiles")
                    if t == 0:
                        placed = out
                # placement + sort = oracle.sort
                sub = tables[0][1]
                counts = placed["counts"]
                assert counts.max() <= C.cap_of(0)
                pairs = np.concatenate([placed["slots"][b, :c] for b, c in enumerate(counts)])
                out = plugin.selftest_bucket_sort(sub, 0, C.key_xor_of(settings), counts, pairs)
                assert (out["sort_overflow"], out["draw_count"]) == (0, d)
                want = np.stack([entries["key"][:d], entries["index"][:d]], axis=1)
                assert np.array_equal(out["out"], want), f"n {n} {mode} alone {alone} cap {cap}: placement + sort is not the oracle's list"
    finally:
        handle.free()


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("n", G.SORT_SIZES)
def test_ordered_bucket_keygen_loops_to_the_reference_placement(plugin, oracle, n, mode):
    """Rayon: the full tiles take the register-to-bucket `continue` path, the ragged last tile the compacting path behind
    it — in the same workgroup under a cap."""
    _placement(plugin, oracle, n, mode, (0,))


@pytest.mark.parametrize("mode", C.MODES)
def test_ordered_bucket_keygen_loops_over_the_long_tiles(plugin, oracle, mode):
    """4096-splat tiles as 256 x 16 and, alone on the chip, 1024 x 4."""
    _placement(plugin, oracle, G.BIG_SORT, mode, (0, 1))


# ---- vertex stage, both binning modes --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.VERTEX_CASE_NAMES)
def test_vertex_stage_loops_to_its_host_twin(plugin, name):
    case = G.vertex_case(name)
    d = VC.twin_of(case)
    assert int(d["drawn"].sum()) >= G.MIN_DRAWN and d["twin"]["count"] % 256 != 0
    for binning, scan in (("scan", True), ("sort", False)):
        for cap in (0,) + G.CAPS:
            plugin.set_grid_cap(cap)
            dev = TVertex._frame(plugin, case, d, binning)
            grids = plugin.debug_frame_grids()
            _assert_looped(grids, "project", f"{name} {binning}", cap)
            assert grids["project"][1] == -(-d["twin"]["count"] // 256) >= 6
            TVertex._check_frame(case, d, dev, f"{binning} cap {cap}", scan)


# ---- instances and lists ---------------------------------------------------------------------------------------------
def test_bin_and_tile_sort_loop_to_the_reference_lists(plugin):
    """12 000 ranks: 12 tiles of bin_kernel, 47 of the project kernels, and more tile instances than three 4096-pair tiles."""
    case = B.frame_case("bin_12000_250x130")
    d = VC.twin_of(case)
    tiles = (-(-int(d["view"].viewport[2]) // 16), -(-int(d["view"].viewport[3]) // 16))
    try:
        for cap in (0,) + G.CAPS:
            plugin.set_grid_cap(cap)
            for level in (0, 3):
                dev = TBin._frame(plugin, case, d, "scan", 1, TBin.LEVEL_FLAGS[level])
                grids = plugin.debug_frame_grids()
                _assert_looped(grids, "bin", f"scan level {level}", cap)
                _assert_looped(grids, "project", f"scan level {level}", cap)
                TBin._check_scan(f"cap {cap} level {level}", dev, d, tiles, level, 1)
            dev = TBin._frame(plugin, case, d, "sort", 1)
            grids = plugin.debug_frame_grids()
            _assert_looped(grids, "tile_sort", "sort", cap)
            _assert_looped(grids, "project", "sort", cap)
            TBin._check_sort(f"cap {cap} sort", dev, d)
    finally:
        plugin.reset_adaptive_state()


# ---- kept order ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", (False, True), ids=["no tail", "tail"])
def test_compaction_loops_to_the_host_reference(plugin, tail):
    n = 5 * G.ENTRIES_TILE + 1
    small = random_gaussians_3d_seeded(5000, 21)
    rep = lambda a: np.ascontiguousarray(np.tile(a, (3, 1))[:n])
    cloud = PlanarGaussian3d(rep(small.position_visibility), rep(small.spherical_harmonic), rep(small.rotation), rep(small.scale_opacity))
    v = View.headless(64, 64, msaa_samples=1)
    s = CloudSettings(rasterize_mode=RasterizeMode.Depth) if tail else CloudSettings()
    rng = np.random.default_rng(n)
    e = np.empty(n, SORT_ENTRY_DTYPE)
    e["key"], e["index"] = rng.integers(0, CULLED, n, dtype=np.uint32), rng.permutation(n).astype(np.uint32)
    e["key"][0::4] = CULLED                                   # entries that cannot be drawn, mixed in
    e["index"][2::4] = n + (e["index"][2::4] % 5)
    e["key"][-1], e["index"][-1] = 5, 7                       # the ragged tile's one entry is kept
    kept = (e["key"] != CULLED) & (e["index"] < n)
    want = e[kept]
    want_tail = e[~kept].copy()                               # the skipped entries in list order, their index made safe
    want_tail["index"] = np.where(want_tail["index"] < n, want_tail["index"], n - 1)
    assert len(want_tail) > 2 * G.ENTRIES_TILE and (e[~kept]["index"] >= n).any()
    plugin.reset_adaptive_state()
    h = plugin.upload(cloud)
    dse = plugin.device_sorted_entries(1, h)
    try:
        dse.upload(0, e)
        records = {}
        for cap in (0,) + G.CAPS:
            plugin.set_grid_cap(cap)
            plugin.render(h, v, s, download=False, entries=dse.chunk(0))
            grids = plugin.debug_frame_grids()
            _assert_looped(grids, "front", f"compaction tail {tail}", cap)
            assert grids["front"][1] == 6 and grids["depth"] == (0, 0)
            st = plugin.stats()
            assert st["sort_path"] == "kept" and st["draw_count"] == len(want) and st["splat_count"] == n
            assert same_bits(plugin.draw_list(), want), f"cap {cap} tail {tail}: the draw list"
            if tail:
                assert grids["tail_ptr"] and grids["tail_count"] == len(want_tail) == n - len(want)
                got_tail = plugin.download(grids["tail_ptr"], np.empty(grids["tail_count"], SORT_ENTRY_DTYPE))
                bad = np.nonzero(got_tail != want_tail)[0]
                assert not len(bad), f"cap {cap}: {len(bad)} tail entries differ, the first at {bad[0]}: device {got_tail[bad[0]]} reference {want_tail[bad[0]]}"
            else:
                assert (grids["tail_ptr"], grids["tail_count"]) == (0, 0)
            records[cap] = plugin.debug_frame_records()["records"]
            assert same_bits(records[cap], records[0]), f"cap {cap} tail {tail}: the records"
    finally:
        dse.free()
        h.free()


# ---- whole frames ----------------------------------------------------------------------------------------------------
def _frame_scene():
    """20 000 splats, about three quarters of them in the frustum: 10 keygen tiles, 8 depth tiles, ~60 project tiles, ~15 bin
    tiles, and tile instances for more than three 4096-pair tiles."""
    v = View.headless(256, 144, yaw=0.2)
    return VC.screen_cloud(v, 20_000, 31), v, CloudSettings()


def _images(plugin, h, v, s):
    """One synchronous frame: the f32 image and the sRGB8 image, as uint32."""
    img = plugin.render(h, v, s)
    ptr, nbytes = plugin.framebuffer_srgb8_device_ptr()
    packed = plugin.download(ptr, np.empty(nbytes // 4, np.uint32))
    return img.view(np.uint32).copy(), packed


@pytest.mark.parametrize("binning", ("scan", "sort"))
def test_capped_frames_draw_the_uncapped_image(plugin, binning):
    c, v, s = _frame_scene()
    plugin.set_binning(binning)
    plugin.set_output_srgb8(True)
    plugin.reset_adaptive_state()
    h = plugin.upload(c)
    try:
        for flags in (G.NO_BUCKET_SORT, G.NO_BUCKET_SORT | G.RERUN_EVERY_FRAME, G.NO_BUCKET_SORT | G.SMALL_LISTS):
            plugin.set_debug_flags(flags)
            plugin.reset_adaptive_state()
            want = None
            for cap in (0,) + G.CAPS:
                plugin.set_grid_cap(cap)
                plugin.reset_adaptive_state()        # (BGS_DEBUG_SMALL_LISTS: every frame starts from 64-entry lists and is re-run)
                got = _images(plugin, h, v, s)
                grids = plugin.debug_frame_grids()
                for kernel in ("front", "depth", "project") + (("bin",) if binning == "scan" else ("tile_sort",)):
                    _assert_looped(grids, kernel, f"{binning} flags 0x{flags:x}", cap)
                # the re-run kept the cap: grids["cap"] is the re-run's. Both flags are BINNING_SCAN's (check_capacities re-runs
                # `render && scan` frames, the lists are the supertile lists): a sort-binning frame re-runs only when its
                # instances outgrow 4 M, which these do not
                assert plugin.stats()["regrow_count"] == (1 if binning == "scan" and flags != G.NO_BUCKET_SORT else 0)
                want = want or got
                assert np.array_equal(got[0], want[0]), f"{binning} flags 0x{flags:x} cap {cap}: the f32 image"
                assert np.array_equal(got[1], want[1]), f"{binning} flags 0x{flags:x} cap {cap}: the sRGB8 image"
            assert want[0].view(np.float32)[..., :3].max() > 0.05
    finally:
        plugin.set_output_srgb8(False)
        h.free()


def test_capped_frames_in_flight_and_the_graphs_follow_the_cap(plugin):
    """Depth 3, async, graphs on: the images under a cap are the uncapped ones, and changing the cap between two otherwise
    equal graph frames captures anew (the grids are in GraphKey) instead of replaying a graph with the old grids."""
    c, v, s = _frame_scene()
    plugin.set_debug_flags(G.NO_BUCKET_SORT)
    plugin.reset_adaptive_state()
    h = plugin.upload(c)
    try:
        want = plugin.render(h, v, s).view(np.uint32).copy()
        plugin.set_grid_cap(2)
        plugin.render(h, v, s, download=False)
        grids = plugin.debug_frame_grids()
        for kernel in ("front", "depth", "project", "bin"):
            _assert_looped(grids, kernel, "the async frames' shape, synchronously", 2)
        plugin.set_grid_cap(0)
        plugin.set_pipeline_depth(3)
        plugin.set_profiling(0)
        plugin.set_async(True)
        plugin.set_graphs(True)

        def frames(count):
            c0, r0 = plugin.graph_counters()
            out = []
            for _ in range(count // 3):              # three in flight, one per lane, then popped oldest first
                for _ in range(3):
                    plugin.render(h, v, s, download=False)
                for _ in range(3):
                    ptr, _ = plugin.pipeline_pop()
                    out.append(plugin.download(ptr, np.empty((v.height, v.width, 4), np.float32)).view(np.uint32).copy())
            c1, r1 = plugin.graph_counters()
            return out, c1 - c0, r1 - r0

        frames(12)                                   # the lanes' first frames memset, then both parities capture
        imgs, caps0, reps0 = frames(6)
        assert caps0 == 0 and reps0 == 6, (caps0, reps0)
        assert all(np.array_equal(i, want) for i in imgs)
        for cap in G.CAPS:
            plugin.set_grid_cap(cap)
            imgs, captures, replays = frames(6)      # 3 lanes x 2 parities: every one captures anew under the new cap
            print(f"cap {cap}: captures +{captures}, replays +{replays}")
            assert captures == 6 and replays == 0, (cap, captures, replays)
            grids = plugin.debug_frame_grids()       # (of the batch's last frame, now popped)
            for kernel in ("front", "depth", "project", "bin"):
                _assert_looped(grids, kernel, "async, captured", cap)
            assert all(np.array_equal(i, want) for i in imgs), f"cap {cap}: an async graph frame differs from the uncapped image"
            imgs, captures, replays = frames(6)
            assert captures == 0 and replays == 6, (cap, captures, replays)
            grids = plugin.debug_frame_grids()
            for kernel in ("front", "depth", "project", "bin"):
                _assert_looped(grids, kernel, "async, replayed", cap)
            assert all(np.array_equal(i, want) for i in imgs)
        # Sort binning at the same depth with async on: bgs_render runs such a frame synchronously on lane 0 (only
        # BINNING_SCAN frames are enqueued and left in flight), so none is ever in flight next to another lane's
        plugin.set_graphs(False)
        plugin.set_binning("sort")
        for cap in (0,) + G.CAPS:
            plugin.set_grid_cap(cap)
            img = plugin.render(h, v, s).view(np.uint32)
            assert plugin.frames_in_flight() == 0
            grids = plugin.debug_frame_grids()
            for kernel in ("front", "depth", "project", "tile_sort"):
                _assert_looped(grids, kernel, "sort binning, depth 3, async on", cap)
            assert np.array_equal(img, want), f"cap {cap}: the sort-binning frame at depth 3 differs from the uncapped scan image"
    finally:
        plugin.set_async(False)
        plugin.synchronize()
        h.free()


# ---- a stale hint, with no hook at all -------------------------------------------------------------------------------
def test_a_stale_draw_hint_makes_the_project_kernel_loop_on_its_own():
    """One cloud, two views: the first draws a few hundred splats, the second over 20 000. The second frame's project grid is
    max(hint / 256 + 8, 32) workgroups for 80 tiles or more — production's own short grid. Its records and image equal those
    of a fresh context that never had a hint (BGS_DEBUG_NO_DRAW_HINT)."""
    wide, narrow = View.headless(256, 144), View.headless(256, 144, yaw=np.pi)    # back to back: neither sees the other's splats
    a, b = VC.screen_cloud(wide, 30_000, 57, spread=1.0), VC.screen_cloud(narrow, 400, 58, spread=0.9)
    c = PlanarGaussian3d(*(np.concatenate([getattr(a, f), getattr(b, f)]) for f in ("position_visibility", "spherical_harmonic", "rotation", "scale_opacity")))
    s = CloudSettings()
    out = {}
    for name, flags in (("stale hint", 0), ("no hint", G.NO_DRAW_HINT)):
        with GaussianSplattingPlugin(0) as p:
            p.set_debug_flags(flags)
            h = p.upload(c)
            if not flags:
                p.render(h, narrow, s, download=False)
                few = p.stats()["draw_count"]
                assert 0 < few < 1000, few
            img = p.render(h, wide, s)
            grids = p.debug_frame_grids()
            st = p.stats()
            print(f"{name}: draw_count {st['draw_count']}, grids {grids}")
            assert st["draw_count"] >= 20_000 and grids["cap"] == 0
            if not flags:
                hint = few + few // 8 + 1024                                       # AdaptiveState::learn_draw_count
                assert grids["project"][0] == max(hint // 256 + 8, 32) == 32 and grids["project"][1] >= 80
                assert G.looped(grids, "project"), grids
            out[name] = (img.view(np.uint32).copy(), p.debug_frame_records())
            h.free()
    a, b = out["stale hint"], out["no hint"]
    assert a[1]["draw_count"] == b[1]["draw_count"] and a[1]["visible_count"] == b[1]["visible_count"]
    assert a[1]["color_max_bits"] == b[1]["color_max_bits"]
    assert same_bits(a[1]["records"], b[1]["records"]) and same_bits(a[1]["rects"], b[1]["rects"])
    assert np.array_equal(a[0], b[0])


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_the_grid_cap_refuses_what_it_cannot_be_and_zero_restores_the_grids():
    lib = _native.load()
    assert lib.bgs_set_grid_cap(None, 1) == _native.BGS_EINVAL and b"ctx is NULL" in lib.bgs_last_error(None)
    with GaussianSplattingPlugin(0) as p:
        with pytest.raises(_native.BgsError, match="frame grids: no frame has been run"):
            p.debug_frame_grids()
        with pytest.raises(_native.BgsError, match=r"blocks must be 0 \(off\) or 1 \.\. 4096, got 4097"):
            p.set_grid_cap(_native.GRID_CAP_MAX + 1)
        p.set_grid_cap(_native.GRID_CAP_MAX)
        p.set_debug_flags(G.NO_BUCKET_SORT | G.NO_DRAW_HINT)
        c, v, s = _frame_scene()
        h = p.upload(c)
        p.set_grid_cap(0)
        p.render(h, v, s, download=False)
        default = p.debug_frame_grids()
        draw = p.stats()["draw_count"]
        # one workgroup per tile: what num_cus * 4 / * 3 (>= 256 CUs) give a frame of this size
        # (the grids of the kernels behind keygen are sized by n, their tiles by the frame's draw count)
        assert default == {"front": (10, 10), "depth": (10, -(-draw // 2048)), "project": (79, -(-draw // 256)), "bin": (20, -(-draw // 1024)),
                           "tile_sort": (0, 0), "cap": 0, "front_chainless": False, "tail_ptr": 0, "tail_count": 0}, default
        p.set_grid_cap(2)
        p.render(h, v, s, download=False)
        capped = p.debug_frame_grids()
        assert capped["cap"] == 2 and all(capped[k][0] == 2 and capped[k][1] == default[k][1] for k in ("front", "depth", "project", "bin"))
        p.set_grid_cap(0)
        p.render(h, v, s, download=False)
        assert p.debug_frame_grids() == default
        # the chainless keygen of a rendered bucket frame is not capped
        p.set_debug_flags(G.NO_DRAW_HINT)
        p.set_grid_cap(1)
        p.render(h, v, s, download=False)
        p.render(h, v, s, download=False)
        g = p.debug_frame_grids()
        assert p.stats()["sort_path"] == "bucket" and g["front_chainless"] and g["front"] == (10, 10) and g["depth"] == (0, 0), g
        import ctypes
        small = np.zeros(_native.FRAME_GRIDS_WORDS - 1, np.uint32)
        rc = p._lib.bgs_debug_frame_grids(p._ctx, small.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), small.size)
        assert rc == _native.BGS_EINVAL and b"out holds 15 words" in p._lib.bgs_last_error(p._ctx) and not small.any()
        h.free()
