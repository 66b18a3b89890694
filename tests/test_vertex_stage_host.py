"""CPU side of the vertex-stage pin (tests/test_vertex_stage_gpu.py compares the device's records with the host build of
csrc/splat_math.h, record by record): the twin's helpers are right, and every case holds what it is named for, so that
the GPU comparison cannot pass vacuously. No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import helpers as H
import vertex_stage_cases as VC
from bevy_gaussian_splatting_amd import CloudSettings, GaussianMode, View, random_gaussians_3d_seeded

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "bevy_gaussian_splatting_amd", "csrc")
POPULATED = [c.name for c in VC.CASES if c.populated]


def test_rect_empty_and_the_packing_order_are_the_sources():
    """RECT_EMPTY, the rect word's packing and the float4 lanes of both records, read from csrc the way
    test_kept_order_host.py reads its constants."""
    dev = open(os.path.join(CSRC, "bgs_device.h")).read()
    assert int(re.search(r"RECT_EMPTY\s*=\s*(0x[0-9A-Fa-f]+)u", dev).group(1), 16) == H.RECT_EMPTY
    src = open(os.path.join(CSRC, "render_kernels.hip")).read()
    body = src[src.index("__device__ __forceinline__ uint32_t project_rank("):src.index("// BINNING_SORT: project + ordered instance emission")]
    assert re.search(r"pr\.tx0 \| \(\(uint32_t\)pr\.tx1 << 8\) \| \(\(uint32_t\)pr\.ty0 << 16\) \|\s*\(\(uint32_t\)pr\.ty1 << 24\)", body)
    assert "draw_list[count - 1u - j]" in src            # the rank reversal
    surfel, plain = body[body.index("if constexpr (SURFEL)"):body.index("} else {\n        float4* dst")], body[body.index("} else {\n        float4* dst"):]
    lanes = lambda text: [a.strip() for m in re.findall(r"make_float4\((.*?)\);", text, flags=re.S) for a in re.sub(r"\s+", " ", m).split(", ")]
    assert lanes(plain) == ["pr.quad.cx", "pr.quad.cy", "pr.p[0]", "pr.p[1]", "pr.p[2]", "pr.p[3]", "pr.p[4]", "pr.color[0]",
                            "pr.color[1]", "pr.color[2]", "pr.color[3]", "pr.ndc_z"]
    assert len(H.RECORD_FIELDS) == 12 and H.RECORD_FIELDS == ("cx", "cy", "p0", "p1", "p2", "p3", "p4", "r", "g", "b", "a", "z")
    sl = lanes(surfel)
    assert len(sl) == 24 == len(H.SURFEL_FIELDS)
    assert sl[:7] == ["pr.quad.cx", "pr.quad.cy", "pr.p[0]", "pr.p[1]", "pr.radius", "pr.surfel.mean_x", "pr.surfel.mean_y"]
    assert sl[7:16] == ["(float)(T1y * T2z - T1z * T2y)", "(float)(T1z * T2x - T1x * T2z)", "(float)(T1x * T2y - T1y * T2x)",
                        "(float)(T2y * T0z - T2z * T0y)", "(float)(T2z * T0x - T2x * T0z)", "(float)(T2x * T0y - T2y * T0x)",
                        "(float)(T0y * T1z - T0z * T1y)", "(float)(T0z * T1x - T0x * T1z)", "(float)(T0x * T1y - T0y * T1x)"]
    assert sl[16:] == ["pr.color[0]", "pr.color[1]", "pr.color[2]", "pr.color[3]", "pr.ndc_z", "0.0f", "0.0f", "0.0f"]
    assert H.SURFEL_FIELDS[16:21] == ("r", "g", "b", "a", "z")
    # and the struct sizes the strides come from
    assert "sizeof(Record) == 48" in dev and "sizeof(RecordSurfel) == 96" in dev


@pytest.mark.parametrize("name", ["inst_f32_obb_color", "inst_f16_surfel_any", "kept_order"])
def test_record_words_round_trip(name):
    """twin -> the device's bytes -> named fields: every lane comes back at its place, ranks reversed, rects packed."""
    d = VC.twin_of(VC.by_name(name))
    tw, rec, rects, drawn = d["twin"], d["records"], d["rects"], d["drawn"]
    count = tw["count"]
    assert rec.dtype == np.uint32 and rec.shape == (count, 24 if tw["surfel"] else 12) and rec.flags["C_CONTIGUOUS"]
    assert np.array_equal(drawn, tw["draw"][::-1]) and drawn.sum() >= 32
    f = H.record_fields(rec)
    bits = lambda a: np.atleast_1d(np.asarray(a, np.float32)).view(np.uint32).tolist()
    for j in np.nonzero(drawn)[0][::17]:
        e = count - 1 - j
        assert bits(f["cx"][j]) == bits(tw["cx"][e]) and bits(f["cy"][j]) == bits(tw["cy"][e])
        assert [bits(f[k][j]) for k in ("r", "g", "b", "a")] == [bits(x) for x in tw["color"][e]]
        assert bits(f["z"][j]) == bits(tw["z"][e])
        if tw["surfel"]:
            assert bits(f["m00"][j]) == bits(tw["p"][e][0]) and bits(f["m11"][j]) == bits(tw["p"][e][1])
            assert bits(f["radius"][j]) == bits(tw["radius"][e])
            assert [bits(f[f"T{i}"][j]) for i in range(9)] == [bits(x) for x in tw["cross"][e]]
            assert [bits(f[f"pad{i}"][j]) for i in range(3)] == [[0], [0], [0]]     # +0.0
        else:
            assert [bits(f[f"p{i}"][j]) for i in range(5)] == [bits(x) for x in tw["p"][e]]
        tx0, tx1, ty0, ty1 = (int(x) for x in tw["rect"][e])
        assert int(rects[j]) == tx0 | (tx1 << 8) | (ty0 << 16) | (ty1 << 24) and 0 <= tx0 <= tx1 <= 255 and 0 <= ty0 <= ty1 <= 255
    assert (rects[~drawn] == H.RECT_EMPTY).all() and (rec[~drawn] == 0).all() and (rects[drawn] != H.RECT_EMPTY).all()
    assert rec.tobytes() == np.ascontiguousarray(rec).view(np.uint8).tobytes() and len(rec.tobytes()) == count * rec.shape[1] * 4


def test_case_generators_are_deterministic():
    for name in ("inst_f16_obb_any", "edge_on_surfels_surfel", "edge_borders_250x130", "ranks_257", "srgb_magnitudes_obb"):
        case = VC.by_name(name)
        (a, va, sa), (b, vb, sb) = case.build(), case.build()
        for x, y in ((a.position_visibility, b.position_visibility), (a.spherical_harmonic, b.spherical_harmonic),
                     (a.rotation, b.rotation), (a.scale_opacity, b.scale_opacity)):
            assert x.tobytes() == y.tobytes()
        assert np.array_equal(np.asarray(va.clip_from_world), np.asarray(vb.clip_from_world))
        assert bytes(sa.to_native()) == bytes(sb.to_native())
    assert VC._kept_chunk(500).tobytes() == VC._kept_chunk(500).tobytes()
    assert len(set(VC.CASE_NAMES)) == len(VC.CASE_NAMES)


@pytest.mark.parametrize("name", POPULATED)
def test_every_case_holds_drawn_undrawn_and_culled_ranks(name):
    tw = VC.twin_of(VC.by_name(name))["twin"]
    assert tw["count"] <= 3000
    assert int(tw["draw"].sum()) >= 32
    assert int((tw["visible"] & ~tw["draw"]).sum()) >= 1
    assert int((~tw["visible"]).sum()) >= 1
    # (the inputs are finite; a drawn record need not be: a scale of 7e4 overflows the AABB conic of edge_scales_aabb)
    assert np.isfinite(tw["color"][tw["draw"]]).all() and np.isfinite(tw["cx"][tw["draw"]]).all()


def test_every_input_value_is_finite():
    for case in VC.CASES:
        c = VC.twin_of(case)["cloud"]
        for plane in (c.position_visibility, c.spherical_harmonic, c.rotation, c.scale_opacity):
            assert np.isfinite(plane).all(), case.name


def test_the_cases_cover_what_the_launchers_dispatch():
    names = set(VC.CASE_NAMES)
    for fmt in ("f32", "f16", "cov3d"):
        for shape in ("obb", "aabb", "obb2d", "surfel"):
            for any_mode in ("color", "any"):
                assert (f"inst_{fmt}_{shape}_{any_mode}" in names) == (not (fmt == "cov3d" and shape in ("obb2d", "surfel")))
    # validate refuses what is left out (bgs_frame.hip): a precomputed-covariance cloud is 3D gaussian mode only
    frame = open(os.path.join(CSRC, "bgs_frame.hip")).read()
    assert "cloud->ptrs.format == CLOUD_COV3D &&\n        (s->gaussian_mode != BGS_GAUSSIAN_3D" in frame
    counts = sorted(c.rank_count for c in VC.CASES if c.rank_count)
    assert counts == [1, 255, 256, 257, 3000]
    for c in VC.CASES:
        if c.rank_count:
            assert VC.twin_of(c)["twin"]["count"] == c.rank_count and len(VC.twin_of(c)["cloud"]) > c.rank_count
    sizes = {(VC.twin_of(c)["view"].width, VC.twin_of(c)["view"].height) for c in VC.CASES}
    assert {(37, 21), (250, 130), (4096, 64)} <= sizes
    assert max(int(VC.twin_of(VC.by_name(n))["twin"]["rect"][:, 1].max()) for n in ("target_4096x64", "target_4096x64_surfel")) == 255
    kept = VC.twin_of(VC.by_name("kept_order"))
    assert (kept["kept"]["key"] == 0xFFFFFFFF).sum() > 300 and kept["twin"]["count"] == (kept["kept"]["key"] != 0xFFFFFFFF).sum()


# ---- the edge classes contain the decision they are named for: a splat on each side of every threshold -----------------
def test_edge_frustum_boundary_sits_on_both_sides_of_in_frustum():
    d = VC.twin_of(VC.by_name("edge_frustum_boundary"))
    vis = d["twin"]["visible"]
    boundary = d["draw_list"]["index"] < 880          # the boundary cloud's splats (the rest is an ordinary screenful)
    assert 0.2 * 880 < (vis & boundary).sum() < 0.8 * 880
    keys, unsure = H.device_keys_two_step(d["cloud"], d["view"], CloudSettings())
    assert unsure > 100                                  # inside the guard bands of the division-free verdict, too


def test_edge_on_axis_splats_have_a_nan_quad_and_their_neighbours_do_not():
    d = VC.twin_of(VC.by_name("edge_on_axis_nan_obb"))
    by_splat = np.empty(160, int)
    by_splat[d["draw_list"]["index"]] = np.arange(160)
    vis, draw = d["twin"]["visible"][by_splat], d["twin"]["draw"][by_splat]
    assert vis[:40].all() and not draw[:40].any()        # on the axis: in the frustum, nothing to draw
    assert draw[40:120].all() and not vis[120:].any()


@pytest.mark.parametrize("name", ["edge_scales_obb", "edge_scales_aabb", "edge_scales_surfel"])
def test_edge_scales_hold_every_edge_value_in_the_frustum(name):
    d = VC.twin_of(VC.by_name(name))
    vis = np.zeros(len(d["cloud"]), bool)
    vis[d["draw_list"]["index"]] = d["twin"]["visible"]
    so = d["cloud"].scale_opacity
    for val in VC.SCALE_EDGES:
        for axes in (1, 2, 3):
            hit = vis & ((so[:, :3] == np.float32(val)).sum(axis=1) == axes)
            assert hit.sum() >= 3, (val, axes)
    assert (vis & ~(np.isin(so[:, :3], np.array(VC.SCALE_EDGES, np.float32))).any(axis=1)).sum() > 500


@pytest.mark.parametrize("name", ["edge_opacities_obb", "edge_opacities_surfel"])
def test_edge_opacities_sit_on_both_sides_of_the_cutoff_clamp(name):
    d = VC.twin_of(VC.by_name(name))
    vis = np.zeros(len(d["cloud"]), bool)
    vis[d["draw_list"]["index"]] = d["twin"]["visible"]
    op = np.ascontiguousarray(d["cloud"].scale_opacity[vis, 3])
    ln = np.empty_like(op)
    H.shim().shim_ln_f32(H._fp(op), op.size, H._fp(ln))
    arg = np.float32(9.0) + np.float32(2.0) * ln           # cutoff_radius: sqrtf(fmaxf(arg, 0.000001f))
    near = np.abs(op - VC.E45) < 1e-5
    assert (near & (arg < np.float32(1e-6))).any() and (near & (arg > np.float32(1e-6))).any()
    assert (near & (arg == 0)).any() and (near & (arg < 0)).any()
    for val in (1e-6, 1.0, 1.5):
        assert (op == np.float32(val)).any(), val
    ops = VC.opacity_edges()
    assert np.nextafter(VC.E45, np.float32(0)) in ops and np.nextafter(VC.E45, np.float32(1)) in ops   # +-1 ulp


@pytest.mark.parametrize("name", ["edge_on_surfels_obb2d", "edge_on_surfels_surfel"])
def test_edge_on_surfels_take_both_outcomes_of_both_degeneracy_tests(name):
    d = VC.twin_of(VC.by_name(name))
    cl = d["cloud"]
    fpc = H.frame_params(len(cl), d["view"], d["settings"])
    probe = np.zeros((len(cl), 3), np.float32)
    for i in range(len(cl)):
        H.shim().shim_surfel_probe(ctypes.byref(fpc), H._fp(cl.position_visibility[i]), H._fp(cl.rotation[i]),
                                   H._fp(cl.scale_opacity[i]), H._fp(probe[i]))
    vis = np.zeros(len(cl), bool)
    vis[d["draw_list"]["index"]] = d["twin"]["visible"]
    p = probe[vis]
    d_fired = p[:, 2] == 1
    small = ~d_fired & ((p[:, 0] < 1e-4) | (p[:, 1] < 1e-4))
    assert d_fired.sum() >= 20 and (~d_fired).sum() >= 20          # |d| < 1e-4 and not
    assert small.sum() >= 20 and (~d_fired & ~small).sum() >= 20   # extent < 1e-4 and not
    # nearly edge-on on both sides: the smallest tilt that is drawn and the largest that is not are neighbours in the list
    idx = np.arange(len(cl))
    tilt = np.array(VC.EDGE_ON_OFFSETS)[idx % len(VC.EDGE_ON_OFFSETS)]
    edge = vis & (idx < 800)
    ext_small = (probe[:, 2] == 0) & ((probe[:, 0] < 1e-4) | (probe[:, 1] < 1e-4))
    assert (edge & ext_small & (tilt == 0.0)).any() and (edge & ext_small & (tilt >= 1e-3)).any()
    assert (edge & ~ext_small & (tilt <= 1e-3)).any()


def test_edge_borders_straddle_each_border_and_fall_on_both_sides_of_the_guard_band():
    d = VC.twin_of(VC.by_name("edge_borders_250x130"))
    tw = d["twin"]
    w, h = d["view"].width, d["view"].height
    b, draw = tw["bounds"], tw["draw"]
    minx, maxx, miny, maxy = (b[:, i] for i in range(4))
    undrawn = int((tw["visible"] & ~draw).sum())
    assert undrawn >= 20                                   # beyond the guard band
    for straddle, beyond in (((minx < 0) & (maxx > 0), maxx < 0), ((minx < w) & (maxx > w), minx > w),
                             ((miny < 0) & (maxy > 0), maxy < 0), ((miny < h) & (maxy > h), miny > h)):
        assert (draw & straddle).sum() >= 3
        assert (draw & beyond).sum() >= 1                  # entirely off the target, inside the 1.5-pixel guard band: drawn


@pytest.mark.parametrize("name", [c.name for c in VC.CASES if c.srgb])
def test_srgb_cases_hold_colours_on_both_sides_of_the_knee(name):
    case = VC.by_name(name)
    d = VC.twin_of(case)                                    # LinRec709Display: the pre-transfer colour
    assert d["settings"].rasterize_mode.name == "Color" and d["settings"].draw_mode.name == "All"
    col = d["twin"]["color"][d["twin"]["draw"]][:, :3]
    assert (col <= np.float32(0.04045)).sum() >= 10 and (col > np.float32(0.04045)).sum() >= 10
    assert (np.abs(col) > 5).sum() >= 1
    if "srgb_magnitudes" in name:
        assert (np.abs(col) > 5).sum() >= 10 and ((col > 0.03) & (col < 0.05)).sum() >= 10


# ---- the twin itself --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"aabb": True}, {"sh_degree": 1, "opacity_adaptive_radius": False}])
def test_cov3d_path_of_the_shim_renders_like_the_oracle(oracle, kw):
    """project_splat's cov3d_pre argument (CLOUD_COV3D) in the host build, composited by the numpy emulation, against the
    oracle — the comparison test_device_math_host.py makes for the other formats, at its tolerance. The oracle has no
    precomputed-covariance variant: with an identity model transform and global_scale 1 (what compute_cov3d folds in and
    the plane cannot see) the variant draws what the rotation / scale path draws."""
    c = random_gaussians_3d_seeded(2500, 11)
    v = View.headless(160, 96)
    s = CloudSettings(**kw)
    e = oracle.sort(c, v, s)
    ref, amb = oracle.render(c, e, v, s, with_ambiguity=True)
    got = H.emulate_render(c, v, s, cov3d=True)
    ok, err = H.tolerance_mask(ref, got, amb)
    assert ok.all(), f"max err {err.max():.3e}"
    strict, _ = H.tolerance_mask(ref, got, None)
    assert (~strict).sum() <= 0.002 * strict.size
    assert not np.array_equal(got, H.emulate_render(c, v, CloudSettings(global_scale=0.5, **kw)))   # (the images are not blank)


@pytest.mark.parametrize("name", ["inst_f32_obb_color", "inst_f32_surfel_any", "mode_Depth_obb", "draw_Selected_aabb", "kept_order"])
def test_batched_shim_equals_the_per_splat_shim_bit_for_bit(name):
    d = VC.twin_of(VC.by_name(name))
    c, tw, draw = d["cloud"], d["twin"], d["draw_list"]
    fpc = H.frame_params(len(c), d["view"], d["settings"])
    one = H.ShimOut()
    size = ctypes.sizeof(H.ShimOut)
    for e in range(0, tw["count"], 3):
        si = int(draw[e]["index"])
        H.shim().shim_project(ctypes.byref(fpc), int(draw[e]["key"]), H._fp(c.position_visibility[si]), H._fp(c.rotation[si]),
                              H._fp(c.scale_opacity[si]), H._fp(c.spherical_harmonic[si]), H._fp(tw["depth_range"]), ctypes.byref(one))
        assert ctypes.string_at(ctypes.addressof(one), size) == ctypes.string_at(ctypes.addressof(tw["raw"][e]), size), e
    if name == "mode_Depth_obb":
        assert tw["depth_range"][1] > tw["depth_range"][0] > 0


def test_surfel_cross_products_equal_a_float64_transcription():
    d = VC.twin_of(VC.by_name("inst_f32_surfel_color"))
    tw = d["twin"]
    T = tw["T"].astype(np.float64)
    T0, T1, T2 = T[:, 0:3], T[:, 3:6], T[:, 6:9]
    cross = lambda a, b: np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                                   a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    want = np.concatenate([cross(T1, T2), cross(T2, T0), cross(T0, T1)], axis=1).astype(np.float32)
    drawn = tw["draw"]
    assert drawn.sum() > 500 and np.abs(want[drawn]).max() > 1
    assert np.array_equal(want[drawn].view(np.uint32), tw["cross"][drawn].view(np.uint32))
