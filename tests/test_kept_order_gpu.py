"""Drawing from sorted entries kept on the device (bgs_view.entries_device_ptr): bgs_sort writes the camera's chunk,
bgs_render draws a chunk as it is — the reference's frames between two sorts (update_sort_trigger, src/sort/mod.rs:153-194).

Everything a kept-order frame shares with a sorting frame is compared BITWISE (same draw list -> same frame); the one thing
that has no counterpart on the parent commit, a STALE order under a moved camera, is compared with the oracle under the
tolerances and the ambiguity accounting of test_gpu_parity.py (_assert_image, default slack)."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from bevy_gaussian_splatting_amd import (
    CloudSettings, DeviceSortedEntries, PlanarGaussian3d, RadixSortDepthBits, RasterizeMode, SortMode, View, _native,
    random_gaussians_3d_seeded, random_particle_behaviors, step_reference)
from bevy_gaussian_splatting_amd.plugin import SORT_ENTRY_DTYPE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 5000
W = HT = 128
CULLED = 0xFFFFFFFF
YAW_A, YAW_B = 0.0, 0.65   # the stale-order pair (test_stale_order_...)
_CLOUD = None
# entries_math.h: ENTRIES_GRID_MAX workgroups x ENTRIES_TILE slots = what one sweep of the compaction's grid covers
_MATH = open(os.path.join(ROOT, "bevy_gaussian_splatting_amd", "csrc", "entries_math.h")).read()


def _constant(name):
    import re
    return int(re.search(r"\b" + name + r"\s*=\s*(\d+)\s*;", _MATH).group(1))


SWEEP = _constant("ENTRIES_GRID_MAX") * 256 * 8
assert SWEEP == 524288 and "ENTRIES_TILE = ENTRIES_THREADS * ENTRIES_ITEMS" in _MATH and "ENTRIES_THREADS = 256" in _MATH and "ENTRIES_ITEMS = 8" in _MATH


def base_cloud() -> PlanarGaussian3d:
    global _CLOUD
    if _CLOUD is None:
        _CLOUD = random_gaussians_3d_seeded(N, 21)
        _CLOUD.position_visibility.setflags(write=False)
    return _CLOUD


def view(yaw=0.0, samples=4):
    return View.headless(W, HT, yaw=yaw, msaa_samples=samples)


def entries_of(key, index):
    e = np.empty(len(index), SORT_ENTRY_DTYPE)
    e["key"], e["index"] = key, index
    return e


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_image(ref, got, amb, what):
    """test_gpu_parity._assert_image with its default slack."""
    assert got.shape == ref.shape and np.isfinite(got).all()
    ok, err = H.tolerance_mask(ref, got, amb)
    assert ok.all(), f"{what}: {(~ok).sum()} values out of tolerance, max err {err.max():.3e}"
    rec = H.account(ref, got, amb, what)
    print(f"[{what}] beyond strict {rec['beyond_strict']} of {rec['values']}, max err {rec['max_err']:.2e}")
    assert rec["beyond_strict"] <= 0.002 * rec["values"], f"{what}: ambiguity slack used by too many pixels"


@pytest.fixture()
def scene(plugin):
    """The 5000-splat cloud resident, one chunk of device entries, blocking frames on one lane; everything released after."""
    plugin.set_async(False)
    plugin.set_pipeline_depth(1)
    plugin.set_binning("scan")
    plugin.reset_adaptive_state()
    h = plugin.upload(base_cloud())
    dse = plugin.device_sorted_entries(2, h)
    yield h, dse
    plugin.set_async(False)
    plugin.set_graphs(False)
    plugin.set_profiling(2)
    plugin.set_pipeline_depth(1)
    plugin.set_binning("scan")
    dse.free()
    h.free()


# ---- 1. bgs_sort's second output ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,bits", [(SortMode.Radix, 16), (SortMode.Radix, 24), (SortMode.Radix, 32), (SortMode.Rayon, 32),
                                       (SortMode.NONE, 32)], ids=["radix16", "radix24", "radix32", "rayon", "none"])
def test_sort_writes_the_chunk_it_returns(plugin, oracle, scene, mode, bits):
    h, dse = scene
    s = CloudSettings(sort_mode=mode, radix_sort_depth_bits=RadixSortDepthBits(bits))
    v = view(0.3)
    before = dse.download(0)
    assert np.array_equal(before["key"], np.ones(N, np.uint32)) and np.array_equal(before["index"], np.arange(N))   # the asset's initial content
    host = plugin.sort(h, v, s, into=dse.chunk(1))
    assert same_bits(dse.download(1), host)
    assert same_bits(dse.download(0), before)   # the neighbouring chunk is untouched
    ref = oracle.sort(base_cloud(), v, s)
    assert np.array_equal(host["key"], ref["key"]) and np.array_equal(host["index"], ref["index"])


# ---- 2. a fresh order draws today's frame ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32", "f16", "cov3d"])
@pytest.mark.parametrize("binning", ["scan", "sort"])
def test_fresh_order_is_the_sorting_frame_bit_for_bit(plugin, fmt, binning):
    plugin.set_async(False)
    plugin.set_pipeline_depth(1)
    plugin.set_binning(binning)
    plugin.reset_adaptive_state()
    cloud = base_cloud()
    h = plugin.upload(cloud.to_f16()) if fmt == "f16" else plugin.upload(cloud, precompute_covariance_3d=(fmt == "cov3d"))
    dse = plugin.device_sorted_entries(1, h)
    rng = np.random.default_rng(5)
    try:
        cases = [(1, False, CloudSettings()), (4, False, CloudSettings()), (4, True, CloudSettings()),
                 (4, False, CloudSettings(rasterize_mode=RasterizeMode.Depth)), (1, True, CloudSettings(rasterize_mode=RasterizeMode.Position))]
        for samples, with_depth, s in cases:
            v = view(0.2, samples)
            depth = None
            if with_depth:
                depth = plugin.upload_depth(H.random_depth_buffer(cloud, v, s, rng))
                v.depth_device_ptr = depth
            want = plugin.render(h, v, s)
            want_list = plugin.draw_list()
            plugin.sort(h, v, s, download=False, into=dse.chunk(0))
            got = plugin.render(h, v, s, entries=dse.chunk(0))
            st = plugin.stats()
            assert same_bits(got, want), (fmt, binning, samples, with_depth, s.rasterize_mode)
            assert same_bits(plugin.draw_list(), want_list)
            assert st["sort_path"] == "kept" and st["depth_passes"] == 0 and st["draw_count"] == len(want_list)
            assert st["stage_ms"]["depth_sort"] == 0.0
            if depth:
                plugin.device_free(depth)
            assert np.abs(got[..., :3]).max() > 0.05   # (not an empty frame)
    finally:
        plugin.set_binning("scan")
        dse.free()
        h.free()


# ---- 3. a stale order: the frame the parent commit cannot draw --------------------------------------------------------------
def test_stale_order_under_a_moved_camera_matches_the_oracle(plugin, oracle, scene):
    """Sort at camera A (yaw 0), draw at camera B (yaw 0.65) from A's chunk. Chosen on the CPU with the oracle alone
    (5000 splats, seed 21, 128 x 128, 4 samples): A keeps 349 splats, B 402, 84 of them in both; the oracle's stale and
    fresh images of B differ beyond 1e-3 + 1e-4 |ref| on 47776 of 65536 values (16364 of 16384 pixels); the stale
    reference's ambiguity map is non-zero on 27 pixels (<= 108 values, inside the 0.2 % = 131 values the accounting
    allows on its slack), its largest bound 5.9e-3."""
    h, dse = scene
    cloud, s = base_cloud(), CloudSettings()
    a, b = view(YAW_A), view(YAW_B)
    e_a = plugin.sort(h, a, s, into=dse.chunk(0))
    got = plugin.render(h, b, s, entries=dse.chunk(0))
    st = plugin.stats()
    fresh = plugin.render(h, b, s)
    ref, amb = oracle.render(cloud, e_a, b, s, with_ambiguity=True)
    assert_image(ref, got, amb, "stale order A -> B")
    ok, _ = H.tolerance_mask(fresh, got, None)
    differing = int((~ok).any(axis=2).sum())
    print(f"[stale vs fresh] {differing} of {W * HT} pixels differ beyond the tolerance")
    assert differing >= W * HT // 2
    # the stale cull flags: what A culled stays undrawn although B sees it
    assert st["draw_count"] == int((e_a["key"] != CULLED).sum()) and st["visible_count"] < st["draw_count"]


# ---- 4. hand-built lists ---------------------------------------------------------------------------------------------------
def test_hand_built_lists(plugin, oracle, scene):
    h, dse = scene
    cloud, v = base_cloud(), view(0.1)
    s = CloudSettings(sort_mode=SortMode.Rayon)
    rayon = plugin.sort(h, v, s)
    chunk = dse.chunk(0)

    def draw(e):
        dse.upload(0, e)
        img = plugin.render(h, v, s, entries=chunk)
        return img, plugin.stats(), plugin.draw_list()

    # (a) holes interleaved = the same drawable entries followed by all-ones padding
    keep = rayon[: N // 2]
    holes = entries_of(np.full(N - len(keep), CULLED, np.uint32), np.arange(N - len(keep), dtype=np.uint32))
    holes["key"][::3] = 7                       # a live key ...
    holes["index"][::3] = N + np.arange(len(holes["index"][::3]))   # ... on a splat that does not exist
    holes["index"][1::3] = 0xFFFFFFFF
    mixed = np.empty(N, SORT_ENTRY_DTYPE)
    mixed[0::2], mixed[1::2] = holes, keep
    padded = np.concatenate([keep, entries_of(np.full(N - len(keep), CULLED, np.uint32), np.zeros(N - len(keep), np.uint32))])
    img_mixed, st_mixed, list_mixed = draw(mixed)
    img_padded, st_padded, list_padded = draw(padded)
    assert same_bits(img_mixed, img_padded) and same_bits(list_mixed, keep) and same_bits(list_padded, keep)
    assert st_mixed["draw_count"] == st_padded["draw_count"] == len(keep)
    # (b) the reversed Rayon list, and (c) a list that names one splat twice, against the oracle
    rev = rayon[::-1].copy()
    img, _, _ = draw(rev)
    ref, amb = oracle.render(cloud, rev, v, s, with_ambiguity=True)
    assert_image(ref, img, amb, "reversed rayon list")
    assert not same_bits(img, plugin.render(h, v, s))
    twice = rayon.copy()
    twice[N // 2] = rayon[-1]                   # the splat drawn last (nearest) also in the middle of the list
    img, st, _ = draw(twice)
    ref, amb = oracle.render(cloud, twice, v, s, with_ambiguity=True)
    assert_image(ref, img, amb, "a splat named twice")
    assert st["draw_count"] == N
    # (d) nothing drawable: the clear colour
    v.clear_color = (0.25, 0.5, 0.75, 1.0)
    img, st, lst = draw(entries_of(np.full(N, CULLED, np.uint32), np.arange(N, dtype=np.uint32)))
    assert st["draw_count"] == 0 and len(lst) == 0 and st["sort_path"] == "kept"
    assert np.array_equal(img, np.broadcast_to(np.array(v.clear_color, np.float32), img.shape))


# ---- 5. sizes at which the compaction can go wrong -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097, SWEEP + 1])
def test_compaction_sizes(plugin, n):
    plugin.set_async(False)
    plugin.set_pipeline_depth(1)
    plugin.reset_adaptive_state()
    small = base_cloud()
    reps = -(-n // N)
    tile = lambda a: np.ascontiguousarray(np.tile(a, (reps, 1))[:n])
    cloud = PlanarGaussian3d(tile(small.position_visibility), tile(small.spherical_harmonic), tile(small.rotation), tile(small.scale_opacity))
    h = plugin.upload(cloud)
    dse = plugin.device_sorted_entries(1, h)
    v, s = View.headless(32, 32, msaa_samples=1), CloudSettings()
    rng = np.random.default_rng(n)
    try:
        for pattern in ("none culled", "every second culled", "only the last kept"):
            e = entries_of(rng.integers(0, CULLED, n, dtype=np.uint32), rng.permutation(n).astype(np.uint32))
            if pattern == "every second culled":
                e["key"][0::4] = CULLED
                e["index"][2::4] = n + (e["index"][2::4] % 5)
            elif pattern == "only the last kept":
                e["key"][:-1] = CULLED
            dse.upload(0, e)
            plugin.render(h, v, s, download=False, entries=dse.chunk(0))
            want = e[(e["key"] != CULLED) & (e["index"] < n)]
            st = plugin.stats()
            assert st["draw_count"] == len(want) and st["splat_count"] == n, (n, pattern, st["draw_count"], len(want))
            assert same_bits(plugin.draw_list(), want), (n, pattern)
    finally:
        dse.free()
        h.free()


# ---- 6. frames in flight -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphs", [False, True], ids=["direct", "graphs"])
def test_kept_order_frames_in_flight(plugin, scene, graphs):
    h, dse = scene
    s = CloudSettings()
    a, b = view(YAW_A), view(0.3)
    plugin.sort(h, a, s, download=False, into=dse.chunk(0))
    kept_a, kept_b = plugin.render(h, a, s, entries=dse.chunk(0)), plugin.render(h, b, s, entries=dse.chunk(0))
    sorted_b = plugin.render(h, b, s)
    assert not same_bits(kept_b, sorted_b)
    plugin.set_pipeline_depth(4)
    plugin.set_graphs(graphs)
    plugin.set_profiling(0 if graphs else 2)   # (frames whose stages are timed are always launched directly)
    plugin.set_async(True)
    got = []

    def pop():
        ptr, _ = plugin.pipeline_pop()
        got.append(plugin.download(ptr, np.empty((HT, W, 4), np.float32)))

    # 12 kept-order frames, two cameras in turn, four in flight
    want = []
    for f in range(12):
        if plugin.frames_in_flight() == 4:
            pop()
        plugin.render(h, (a, b)[f % 2], s, download=False, entries=dse.chunk(0))
        want.append((kept_a, kept_b)[f % 2])
    while plugin.frames_in_flight():
        pop()
    assert len(got) == 12 and all(same_bits(g, w) for g, w in zip(got, want))
    # kept-order and sorting frames in turn
    got, want = [], []
    for f in range(12):
        if plugin.frames_in_flight() == 4:
            pop()
        if f % 2:
            plugin.render(h, b, s, download=False)
        else:
            plugin.render(h, b, s, download=False, entries=dse.chunk(0))
        want.append(sorted_b if f % 2 else kept_b)
    while plugin.frames_in_flight():
        pop()
    assert len(got) == 12 and all(same_bits(g, w) for g, w in zip(got, want))
    if graphs:
        assert plugin.graph_counters()[0] >= 1   # the sorting frames did go through a graph


# ---- 7. a particle step between the sort and the frame -----------------------------------------------------------------------
def test_kept_order_after_a_particle_step(plugin, scene):
    h, dse = scene
    cloud, s, v = base_cloud(), CloudSettings(), view(0.0)
    rec = random_particle_behaviors(N, 3).records
    b = plugin.upload_particle_behaviors(rec)
    plugin.sort(h, v, s, download=False, into=dse.chunk(0))
    before = plugin.render(h, v, s, entries=dse.chunk(0))
    plugin.apply_particle_behaviors(h, b, 0.25)
    got = plugin.render(h, v, s, entries=dse.chunk(0))
    pv, _ = step_reference(cloud.position_visibility, rec, 0.25)
    h2 = plugin.upload(PlanarGaussian3d(pv, cloud.spherical_harmonic, cloud.rotation, cloud.scale_opacity))
    try:
        want = plugin.render(h2, v, s, entries=dse.chunk(0))
        assert same_bits(got, want) and not same_bits(got, before)
    finally:
        b.free()
        h2.free()


# ---- 8. errors and stats -----------------------------------------------------------------------------------------------------
def test_errors_name_the_field_and_stats_say_kept(plugin, scene):
    h, dse = scene
    s, v = CloudSettings(), view(0.0)
    chunk = dse.chunk(0)
    bad = [(type(chunk)(chunk.ptr + 4, N), "entries_device_ptr"), (type(chunk)(chunk.ptr, N - 1), "entry_count"),
           (type(chunk)(chunk.ptr, N + 1), "entry_count")]
    for c, field in bad:
        for call in (lambda: plugin.render(h, v, s, entries=c), lambda: plugin.sort(h, v, s, into=c)):
            with pytest.raises(_native.BgsError) as ei:
                call()
            assert ei.value.status == _native.BGS_EINVAL and field in str(ei.value), str(ei.value)
    nv = v.to_native()
    nv.entry_count = N   # a count without a pointer
    import ctypes
    sn = s.to_native()
    assert plugin._lib.bgs_render(plugin._ctx, h._ptr, ctypes.byref(nv), ctypes.byref(sn), None) == _native.BGS_EINVAL
    assert b"entry_count" in plugin._lib.bgs_last_error(plugin._ctx)
    # sort_mode / radix_depth_bits do not reach a kept-order frame
    plugin.sort(h, v, s, download=False, into=chunk)
    want = plugin.render(h, v, s, entries=chunk)
    got = plugin.render(h, v, CloudSettings(sort_mode=SortMode.Rayon, radix_sort_depth_bits=RadixSortDepthBits(16)), entries=chunk)
    st = plugin.stats()
    assert same_bits(got, want)
    none = plugin.render(h, v, CloudSettings(sort_mode=SortMode.NONE))
    st_none = plugin.stats()
    assert st["sort_path"] == "kept" and st["depth_passes"] == 0 and st["splat_count"] == N and 0 < st["visible_count"] <= st["draw_count"] < N
    assert st_none["sort_path"] == "onesweep" and st_none["draw_count"] == N and st_none["visible_count"] == st["visible_count"]
    assert none.shape == want.shape


# ---- 9. the example ------------------------------------------------------------------------------------------------------------
def test_headless_example_with_a_sort_period_matches_the_plugin(plugin, scene, tmp_path):
    """--sort-period-frames 3 --frames 5 with particles: sorts on frames 0 and 3, frames 1, 2 and 4 and the dumped frame
    draw the kept entries over splats that moved since. The Python plugin driven the same way gives the same frame."""
    exe = os.path.join(ROOT, "examples", "headless")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "headless"], check=True, capture_output=True)
    cloud = base_cloud()
    planes = tmp_path / "cloud.bin"
    with open(planes, "wb") as f:
        f.write(np.uint32(N).tobytes())
        for a in (cloud.position_visibility, cloud.spherical_harmonic, cloud.rotation, cloud.scale_opacity):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    dump, recs = tmp_path / "frame.f32", tmp_path / "particles.bin"
    dt = 0.25
    subprocess.run([exe, "--cloud", str(planes), "--width", str(W), "--height", str(HT), "--frames", "5", "--depth", "2",
                    "--sort-period-frames", "3", "--particle-count", "2000", "--particle-dt", str(dt), "--dump-particle-behaviors", str(recs),
                    "--dump-f32", str(dump), "--output-dir", str(tmp_path / "out")], check=True, capture_output=True, timeout=120)
    got = np.fromfile(dump, np.float32).reshape(HT, W, 4)
    from bevy_gaussian_splatting_amd import PARTICLE_BEHAVIOR_DTYPE
    rec = np.fromfile(recs, PARTICLE_BEHAVIOR_DTYPE)
    h, dse = scene
    v, s = View.headless(W, HT), CloudSettings()
    b = plugin.upload_particle_behaviors(rec)
    try:
        for f in range(5):
            plugin.apply_particle_behaviors(h, b, dt)
            if f % 3 == 0:
                plugin.sort(h, v, s, download=False, into=dse.chunk(0))
            plugin.render(h, v, s, download=False, entries=dse.chunk(0))
        want = plugin.render(h, v, s, entries=dse.chunk(0))
        assert same_bits(got, want)
        assert not same_bits(want, plugin.render(h, v, s))   # (the kept order is stale by then: a sorting frame differs)
    finally:
        b.free()
    help_text = subprocess.run([exe, "--help"], check=True, capture_output=True, text=True).stdout
    assert "--sort-period-frames" in help_text and "not a reference flag" in help_text
