"""Host-side mirror of the reference's data model / settings (no GPU, no oracle)."""
import numpy as np
import pytest

from bevy_gaussian_splatting_amd import (
    CloudSettings, GaussianMode, PlanarGaussian3d, PlanarGaussian3dF16, RadixSortDepthBits,
    ShaderDefines, SortedEntries, SortMode, View, random_gaussians_3d_seeded)
from bevy_gaussian_splatting_amd import gaussian as G
from bevy_gaussian_splatting_amd.multiview import assign_views, headless_view


def test_shader_defines_geometry():
    # src/render/mod.rs:715-758
    d = ShaderDefines.for_radix_depth_bits(RadixSortDepthBits.Bits32)
    assert (d.radix_base, d.radix_bits_per_digit, d.workgroup_entries_c) == (256, 8, 1024)
    assert d.workgroup_entries_a == 256 * 4 * 4
    assert d.sorting_buffer_size == 256 * 4 * 4 + (5 + 256) * 4
    assert d.max_tile_count(1_000_000) == 977
    with pytest.raises(ValueError):
        ShaderDefines.for_radix_depth_bits(12)


def test_cloud_settings_defaults_match_reference():
    s = CloudSettings()  # src/gaussian/settings.rs:110-131
    assert (s.aabb, s.global_opacity, s.global_scale, s.opacity_adaptive_radius) == (False, 1.0, 1.0, True)
    assert s.sort_mode == SortMode.Radix and s.radix_sort_depth_bits == RadixSortDepthBits.Bits32
    assert s.gaussian_mode == GaussianMode.Gaussian3d
    n = s.to_native()
    assert list(n.transform) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    t = np.eye(4, dtype=np.float32); t[:3, 3] = [1, 2, 3]
    n2 = CloudSettings(transform=t).to_native()
    assert list(n2.transform)[12:15] == [1, 2, 3]  # column-major: translation in column 3


def test_sorted_entries_initialisation():
    se = SortedEntries.new(3, 5)  # src/sort/mod.rs:347-354
    assert se.sorted.shape == (15,) and np.all(se.sorted["key"] == 1)
    assert se.chunk(2)["index"].tolist() == [0, 1, 2, 3, 4]
    # auto_insert_sorted_entries sizes the asset with the square-padded length (src/sort/mod.rs:259-262) but the
    # sort and the draw stride by the CLOUD length (src/sort/rayon.rs:82-84, src/render/mod.rs:1548-1554)
    se = SortedEntries.for_cloud(2, 10)
    assert se.entry_count == 16 and se.sorted.shape == (32,)
    se.chunk(1, 10)["index"][:] = 7
    assert np.all(se.sorted["index"][10:20] == 7) and se.sorted["index"][9] == 9 and se.sorted["index"][20] == 4
    with pytest.raises(IndexError):
        se.chunk(4, 10)
    assert se.resized(2) is se and se.resized(3).sorted.shape == (48,) and np.all(se.resized(3).sorted["key"] == 1)


def test_random_cloud_distributions_and_determinism():
    a = random_gaussians_3d_seeded(20000, 5)
    b = random_gaussians_3d_seeded(20000, 5)
    assert np.array_equal(a.position_visibility, b.position_visibility)
    assert len(a) == 20000 and a.nbytes() == 20000 * 240
    p = a.position_visibility
    assert p[:, :3].min() >= -20 and p[:, :3].max() < 20 and np.all(p[:, 3] == 1)
    assert a.scale_opacity[:, :3].min() >= 0 and a.scale_opacity[:, :3].max() < 1
    assert a.scale_opacity[:, 3].max() < 0.8
    assert a.rotation.min() >= -1 and a.rotation.max() < 1
    assert abs(np.linalg.norm(a.rotation, axis=1).mean() - 1.0) > 0.05  # NOT normalised
    assert abs(a.spherical_harmonic.mean()) < 0.01


def test_f16_layout():
    c = random_gaussians_3d_seeded(16, 2)
    h = c.to_f16()
    assert isinstance(h, PlanarGaussian3dF16) and h.nbytes() == 16 * 128
    # low half = even coefficient (src/render/planar.wgsl:117-130)
    lo = (h.spherical_harmonic[:, 0] & 0xFFFF).astype(np.uint16).view(np.float16)
    assert np.array_equal(lo, c.spherical_harmonic[:, 0].astype(np.float16))
    # first value in the high half (src/gaussian/f16.rs:244-252)
    hi = (h.rotation_scale_opacity[:, 0] >> 16).astype(np.uint16).view(np.float16)
    assert np.array_equal(hi, c.rotation[:, 0].astype(np.float16))
    op = (h.rotation_scale_opacity[:, 3] & 0xFFFF).astype(np.uint16).view(np.float16)
    assert np.array_equal(op, c.scale_opacity[:, 3].astype(np.float16))
    back = h.to_f32()
    assert np.allclose(back.scale_opacity, c.scale_opacity, atol=1e-3)


def test_test_model_geometry():
    m = G.test_model(0)  # src/gaussian/formats/planar_3d.rs:193-251
    assert len(m) == 9 and np.array_equal(m.position_visibility[8], m.position_visibility[0])
    assert set(np.abs(m.position_visibility[:, :3]).ravel().tolist()) == {0.5}


def test_headless_camera_matches_reference_example():
    v = View.headless()  # examples/headless.rs:177-184
    assert np.allclose(v.world_position, [0, 1.5, 5])
    f = 1 / np.tan(np.pi / 8)
    assert np.isclose(v.clip_from_view[1, 1], f) and np.isclose(v.clip_from_view[0, 0], f / (1920 / 1080))
    assert v.clip_from_view[3, 2] == -1 and np.isclose(v.clip_from_view[2, 3], 0.1)
    p = v.clip_from_world @ np.array([0, 1.5, 5 - 0.1, 1], np.float32)  # point on the near plane
    assert np.isclose(p[2] / p[3], 1.0, atol=1e-5)  # reverse-Z: near -> 1
    assert np.allclose(v.view_from_world @ v.world_from_view, np.eye(4), atol=1e-6)


def test_view_assignment():
    assert assign_views(8, 8) == [[g] for g in range(8)]
    assert assign_views(8, 2) == [[0, 2, 4, 6], [1, 3, 5, 7]]
    assert assign_views(3, 4) == [[0], [1], [2], []]
    v = headless_view(2, 64, 32)
    assert v.camera.order == 2 and np.allclose(v.world_position, [0, 1.5, 5])
    fwd = v.world_from_view[:3, :3] @ np.array([0, 0, -1], np.float32)
    assert np.allclose(fwd, [-1, 0, 0], atol=1e-6)  # yawed 90 degrees about +Y


def test_compute_covariance_3d_cpu_twin():
    """src/gaussian/covariance.rs:4-41 and Covariance3dOpacity::from (src/gaussian/f32.rs:238-251)."""
    from bevy_gaussian_splatting_amd import compute_covariance_3d, covariance_3d_opacity
    assert np.allclose(compute_covariance_3d([1, 0, 0, 0], [2, 3, 4]), [4, 0, 0, 9, 0, 16])
    # a rotation leaves the trace (sum of squared scales) alone; Sigma = R^T S^2 R with the reference's R
    q = np.array([0.5, 0.5, 0.5, 0.5], np.float32)
    cov = compute_covariance_3d(q, [1, 2, 3])
    assert np.isclose(cov[0] + cov[3] + cov[5], 14.0)
    c = random_gaussians_3d_seeded(500, 3)
    planes = compute_covariance_3d(c.rotation, c.scale_opacity[:, :3])
    for i in (0, 7, 499):
        r, x, y, z = c.rotation[i].astype(np.float64)
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y + r * z), 2 * (x * z - r * y)],
                      [2 * (x * y - r * z), 1 - 2 * (x * x + z * z), 2 * (y * z + r * x)],
                      [2 * (x * z + r * y), 2 * (y * z - r * x), 1 - 2 * (x * x + y * y)]])   # rows = from_cols columns^T
        M = np.diag(c.scale_opacity[i, :3].astype(np.float64)) @ R
        S = M.T @ M
        assert np.allclose(planes[i], [S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]], rtol=1e-5, atol=1e-6)
    co = covariance_3d_opacity(c)
    assert co.shape == (500, 8) and np.array_equal(co[:, 6], c.scale_opacity[:, 3]) and np.all(co[:, 7] == 0)


def test_supertile_level_rule_is_stable_and_direct():
    """frame_params.h next_supertile_level (what finish_lane applies to every completed frame): inside
    [1.6, 4] entries per visible splat the level stays; outside it jumps straight to the level the frame's
    geometry asks for; a step never lands on a level that would step back (no flip-flop)."""
    import ctypes
    import helpers as H
    sh = H.shim()
    edges = (ctypes.c_uint32 * 4)(6, 8, 16, 32)

    def nxt(ratio, lv):
        longer = ctypes.c_double(0.0)
        return sh.shim_next_supertile_level(ratio, lv, edges, ctypes.byref(longer)), longer.value

    def ratio_at(extent_tiles, lv):   # a splat of that extent overlaps (extent / edge + 1)^2 supertiles on average
        return (extent_tiles / edges[lv] + 1.0) ** 2

    for lv in range(4):
        for r in (1.6, 2.0, 3.99, 4.0):
            assert nxt(r, lv)[0] == lv
    assert nxt(14.8, 1) == (3, pytest.approx(((22.77 / 32 + 1) ** 2 / 14.8) * 16, rel=1e-2))   # the dense headline frame
    assert nxt(1.3, 1)[0] == 0 and nxt(1.3, 3)[0] == 0 and nxt(1.2, 0)[0] == 0                  # scene-like
    assert nxt(5.0, 3)[0] == 3 and nxt(100.0, 0)[0] == 3
    # from any level and any splat extent the rule settles within two completed frames and then stays
    for extent in np.geomspace(0.05, 400.0, 60):
        for start in range(4):
            lv = start
            seen = [lv]
            for _ in range(4):
                lv = nxt(ratio_at(extent, lv), lv)[0]
                seen.append(lv)
            assert seen[2] == seen[3] == seen[4], (extent, seen)
    assert sh.shim_pow2_ceil(0) == 1 and sh.shim_pow2_ceil(1) == 1 and sh.shim_pow2_ceil(5) == 8
    assert sh.shim_pow2_ceil(1 << 20) == 1 << 20 and sh.shim_pow2_ceil((1 << 40) + 1) == 1 << 31


def test_supertile_edges_and_canonical_levels():
    """frame_params.h supertile_edges / canonical_supertile_level (what plan_frame runs a frame at and finish_lane moves
    between): at 1920x1080 (120 x 68 tiles) the four levels' edges are 6, 8, 16, 32; levels whose edges coincide are one
    level, the lowest; every edge keeps the coarse bins within 256 and 32 per axis."""
    import ctypes
    import helpers as H
    sh = H.shim()

    def edges(tx, ty):
        e = (ctypes.c_uint32 * 4)()
        sh.shim_supertile_edges(tx, ty, e)
        return list(e)

    def canon(lv, e):
        return sh.shim_canonical_supertile_level(lv, (ctypes.c_uint32 * 4)(*e))

    assert edges(120, 68) == [6, 8, 16, 32]
    assert [canon(lv, [6, 8, 16, 32]) for lv in range(4)] == [0, 1, 2, 3]
    big = edges(256, 256)   # 4096 x 4096: level 1 is 16 tiles, levels 2 and 3 both clamp to 32
    assert big[1] == 16 and big[2] == big[3] == 32
    assert [canon(lv, big) for lv in range(4)] == [0, 1, 2, 2]
    assert canon(3, [8, 8, 32, 32]) == 2 and canon(1, [8, 8, 16, 32]) == 1   # level 1 never collapses to level 0
    for tx, ty in ((1, 1), (20, 12), (120, 68), (160, 90), (240, 135), (256, 256), (256, 1), (1, 256)):
        e = edges(tx, ty)
        assert e[0] <= e[1] <= e[2] <= e[3] <= 32
        for edge in e:
            bx, by = -(-tx // edge), -(-ty // edge)
            assert bx * by <= 256 and bx <= 32 and by <= 32, (tx, ty, e)


def test_rasteriser_instantiation_choice():
    """frame_params.h raster_scan_mode: the rasteriser instantiation a frame launches, which is also what it reports
    (bgs_stats.tile_saturation bit 31) and what a captured graph is keyed by. Surfels, Sample2 / Sample8 and the
    bounding-box overlay never get a mid-round-exit mode; AABB3D has one exit mode."""
    import helpers as H
    sh = H.shim()
    OBB, AABB3D, SURFEL = 0, 1, 2
    NO_MIDROUND, MIDROUND_ALWAYS = 0x1000000, 0x20000

    def mode(variant, samples=4, overlay=0, level=1, kind=0, depth=1, flags=0):
        return sh.shim_raster_scan_mode(variant, samples, overlay, level, kind, depth, flags)

    for level in range(4):
        for kind in (0, 1):
            for depth in (1, 4):
                for flags in (0, MIDROUND_ALWAYS):
                    for samples in (1, 2, 4, 8):
                        assert mode(SURFEL, samples, 0, level, kind, depth, flags) == 0
                        assert mode(OBB, samples, 1, level, kind, depth, flags) == 0
                        assert mode(AABB3D, samples, 1, level, kind, depth, flags) == 0
                    for samples in (2, 8):
                        assert mode(OBB, samples, 0, level, kind, depth, flags) == 0
                    for v in (OBB, AABB3D):
                        assert mode(v, 4, 0, level, kind, depth, flags | NO_MIDROUND) == 0
                        assert mode(AABB3D, 4, 0, level, kind, depth, flags) in (0, 1)
    assert mode(OBB, level=2) == 1 and mode(OBB, 1, level=3) == 1 and mode(AABB3D, level=2) == 1
    assert mode(OBB, level=1) == 0 and mode(OBB, level=0) == 0
    # a kind whose saturating tiles hold the work: the sparse frames' exit, with frames in flight only
    assert mode(OBB, level=1, kind=1, depth=4) == 2 and mode(OBB, level=1, kind=1, depth=1) == 0
    assert mode(AABB3D, level=1, kind=1, depth=4) == 1
    assert mode(OBB, level=0, flags=MIDROUND_ALWAYS) == 2 and mode(OBB, level=2, flags=MIDROUND_ALWAYS) == 1


def test_the_compiled_instantiations_are_what_exists_says():
    """frame_params.h RasterInst::exists / ProjectInst::exists, the set the launchers instantiate: 72 of raster_scan_kernel,
    of which the 60 untraced ones are raster_stage_cases.instantiations() and the other 12 the traced ones; 10 of the vertex
    stage, the inst_* cases of vertex_stage_cases. key() tells every one of them from the others."""
    import helpers as H
    import raster_stage_cases as C
    import vertex_stage_cases as VC
    sh = H.shim()
    exist = [(v, s, d, o, m, t) for v in (0, 1, 2) for s in (1, 2, 4, 8) for d in (0, 1) for o in (0, 1) for t in (0, 1) for m in (0, 1, 2)
             if sh.shim_raster_inst_exists(v, s, d, o, m, t)]
    assert len(exist) == 72
    untraced = {(v, s, bool(d), o, m) for v, s, d, o, m, t in exist if not t}
    assert len(untraced) == 60 and untraced == set(C.instantiations())
    traced = [(v, s, m) for v, s, d, o, m, t in exist if t]
    assert len(traced) == 12 and all(not d and not o for v, s, d, o, m, t in exist if t)
    assert sorted(traced) == sorted((v, s, m) for v, modes in ((0, (0, 1, 2)), (1, (0, 1)), (2, (0,))) for s in (1, 4) for m in modes)
    for bad in ((3, 4, 0, 0, 0, 0), (-1, 4, 0, 0, 0, 0), (0, 3, 0, 0, 0, 0), (0, 16, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0), (0, 4, 0, 0, 3, 0), (0, 4, 0, 0, -1, 0)):
        assert not sh.shim_raster_inst_exists(*bad), bad
    assert len({sh.shim_raster_inst_key(*i) for i in exist}) == 72
    project = {(f, surfel, any_mode) for f in (0, 1, 2) for surfel in (0, 1) for any_mode in (0, 1) if sh.shim_project_inst_exists(f, surfel, any_mode)}
    assert len(project) == 10 and not sh.shim_project_inst_exists(3, 0, 0)
    named = {(("f32", "f16", "cov3d").index(fmt), int(shape == "surfel"), int(mode == "any"))
             for fmt, shape, mode in (n[len("inst_"):].split("_") for n in VC.CASE_NAMES if n.startswith("inst_"))}
    assert named == project


def test_every_admitted_frame_gets_an_instantiation_that_exists():
    """raster_instantiation over every input validate (bgs_frame.hip) admits — the per-tile trace only without a depth
    buffer, without the overlay, at 1 or 4 samples — at every supertile level, either verdict of the kind, one frame or
    several in flight and the debug flags that force the choice: what it returns exists(), so the launchers' refusal of an
    instantiation that does not exist cannot be reached from a frame."""
    import ctypes
    import helpers as H
    sh = H.shim()
    NO_MIDROUND, MIDROUND_ALWAYS = 0x1000000, 0x20000
    out = (ctypes.c_int32 * 6)()
    seen = set()
    for variant, (aabb, gaussian_mode) in ((0, (0, 1)), (0, (0, 0)), (1, (1, 1)), (2, (1, 0))):
        for samples in (1, 2, 4, 8):
            for depth in (0, 1):
                for overlay in (0, 1):
                    for trace in ((0, 1) if not depth and not overlay and samples in (1, 4) else (0,)):
                        for level in range(4):
                            for kind in (0, 1):
                                for pipeline in (1, 4):
                                    for flags in (0, NO_MIDROUND, MIDROUND_ALWAYS):
                                        sh.shim_raster_instantiation(aabb, gaussian_mode, samples, depth, overlay, level, kind, pipeline, flags, trace, out)
                                        assert list(out)[:4] == [variant, samples, depth, overlay] and out[5] == trace
                                        assert out[4] == sh.shim_raster_scan_mode(variant, samples, overlay, level, kind, pipeline, flags)
                                        assert sh.shim_raster_inst_exists(*out), list(out)
                                        seen.add(tuple(out))
    assert len(seen) == 72   # and every instantiation that is compiled is one a frame can ask for


def test_rasteriser_waves_and_runs_per_instantiation():
    """RasterInst::waves_per_simd (raster_scan_kernel's __launch_bounds__, and what plan_frame compares a frame's tile waves
    with) and RasterInst::runs (the kernel's RUNS, and the share of an XCD launch_tile_order deals out), against the tables
    of the default build (BGS_MS_WAVES 6, BGS_DENSE_RUNS 1, BGS_DENSE_RUNS_MS 2). Neither depends on overlay or trace."""
    import helpers as H
    sh = H.shim()
    OBB, AABB3D, SURFEL = 0, 1, 2
    #        samples:  1       2       4       8        (without, with a depth buffer)
    waves = {OBB:    ((8, 7), (6, 5), (6, 5), (4, 3)),
             AABB3D: ((8, 7), (6, 5), (6, 5), (4, 3)),
             SURFEL: ((6, 5), (4, 3), (4, 3), (3, 2))}
    for v in (OBB, AABB3D, SURFEL):
        for si, s in enumerate((1, 2, 4, 8)):
            for d in (0, 1):
                assert {sh.shim_raster_inst_waves(v, s, d, o, 0, t) for o in (0, 1) for t in (0, 1)} == {waves[v][si][d]}, (v, s, d)
                if v != SURFEL and s in (1, 4):
                    assert sh.shim_raster_inst_waves(v, s, d, 0, 1, 0) == waves[v][si][d]
    #       (samples, exit):  (1, no) (1, exit) (4, no) (4, exit)
    runs = {OBB:    (1, 1, 1, 2),
            AABB3D: (1, 1, 1, 2),
            SURFEL: (4, 4, 4, 4)}
    for v in (OBB, AABB3D, SURFEL):
        got = tuple(sh.shim_raster_inst_runs(v, s, 0, 0, m, 0) for s in (1, 4) for m in (0, 1))
        assert got == runs[v], (v, got)
        for s in (1, 4):
            assert sh.shim_raster_inst_runs(v, s, 0, 0, 2, 0) == sh.shim_raster_inst_runs(v, s, 0, 0, 1, 0)   # either exit mode
            assert {sh.shim_raster_inst_runs(v, s, d, 0, 0, t) for d in (0, 1) for t in (0, 1)} == {runs[v][0 if s == 1 else 2]}


def test_splitter_tables_are_only_accepted_when_ascending():
    """bucket(key) = number of splitters <= key orders the buckets only for an ascending table."""
    import ctypes
    import helpers as H
    sh = H.shim()
    rng = np.random.default_rng(2)
    good = np.sort(rng.integers(0, 1 << 32, 255, dtype=np.uint64).astype(np.uint32))
    ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    assert sh.shim_splitters_ascending(ptr(good), 255) == 1
    assert sh.shim_splitters_ascending(ptr(np.full(255, 7, np.uint32)), 255) == 1   # all equal keys: still monotone
    bad = good.copy()
    bad[100], bad[101] = bad[101], bad[100]
    assert good[100] == good[101] or sh.shim_splitters_ascending(ptr(bad), 255) == 0
    # the search keygen runs (branchless count of entries <= key over 255 sorted values) is monotone in the key
    keys = np.sort(rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32))
    buckets = np.searchsorted(good, keys, side="right")
    assert np.all(np.diff(buckets) >= 0) and buckets.min() >= 0 and buckets.max() <= 255
