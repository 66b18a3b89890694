"""The cases of tests/test_vertex_stage_gpu.py (device vertex stage against its host twin, record by record) and of
tests/test_vertex_stage_host.py, which shows on the CPU that every case holds what it is named for. Each case is a
small, deterministic (cloud, view, settings, cloud format) — a few thousand splats at most — built so that the draw
list holds drawn, visible-but-not-drawn and culled ranks. No input value is non-finite."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

import helpers as H
from bevy_gaussian_splatting_amd import (
    CloudSettings, DrawMode, GaussianColorSpace, GaussianMode, PlanarGaussian3d, RasterizeMode, SortMode, View,
    compute_aabb, random_gaussians_3d_seeded, rotation_y, transform_from)

LIN, SRGB = GaussianColorSpace.LinRec709Display, GaussianColorSpace.SrgbRec709Display
E45 = np.float32(math.exp(-4.5))   # the opacity at which 9 + 2 ln(opacity) crosses 0 (cutoff_radius)


@dataclass
class Case:
    name: str
    build: Callable[[], tuple]            # -> (cloud, view, settings)
    fmt: str = "f32"                      # "f32" / "f16" / "cov3d": the upload, and what the twin decodes
    kept: Optional[Callable] = None       # (n) -> the caller's chunk of a kept-order frame (structured key / index)
    srgb: bool = False                    # also a frame with SrgbRec709Display (the one tolerance)
    populated: bool = True                # >= 32 drawn, >= 1 visible-but-not-drawn, >= 1 culled rank (the host test asserts it)
    rank_count: Optional[int] = None      # the draw count the case is built for
    tags: tuple = field(default_factory=tuple)


def screen_cloud(view: View, n: int, seed: int, depth=(1.0, 60.0), spread=1.25, transform=None) -> PlanarGaussian3d:
    """The reference's random splats (rotation, scale, opacity, SH of random_gaussians_3d_seeded) placed by un-projecting
    uniformly random NDC positions in [-spread, spread]^2 at log-uniform view distances: most of the cloud is in the
    frustum whatever the target's shape, a margin is outside the target (|ndc| in (1, 1.1): visible, mostly not drawn)
    and a margin is culled (|ndc| > 1.1). The visibility lane cycles 0 .. 7 (classes, selection)."""
    c = random_gaussians_3d_seeded(n, seed)
    rng = np.random.default_rng(1_000_003 * seed + n)
    inv = np.linalg.inv(np.asarray(view.clip_from_world, np.float64))
    near = float(np.asarray(view.clip_from_view, np.float64)[2, 3])
    dist = np.exp(rng.uniform(math.log(depth[0]), math.log(depth[1]), n))
    ndc = rng.uniform(-spread, spread, (n, 2))
    clip = np.stack([ndc[:, 0] * dist, ndc[:, 1] * dist, np.full(n, near), dist], axis=1)
    w = clip @ inv.T
    pos = w[:, :3] / w[:, 3:4]
    if transform is not None:   # positions are given in the model's frame
        ti = np.linalg.inv(np.asarray(transform, np.float64))
        pos = (np.concatenate([pos, np.ones((n, 1))], axis=1) @ ti.T)[:, :3]
    c.position_visibility[:, :3] = pos.astype(np.float32)
    c.position_visibility[:, 3] = (np.arange(n) % 8).astype(np.float32)
    return c


def _view(w=250, h=130, yaw=0.0):
    v = View.headless(w, h, yaw=yaw)
    v.previous_clip_from_world = View.headless(w, h, yaw=yaw + 0.002).clip_from_world   # the camera turned a little
    v.delta_time = 1.0 / 144.0
    return v


def _shape(shape: str) -> dict:
    return {"obb": {}, "aabb": {"aabb": True}, "obb2d": {"gaussian_mode": GaussianMode.Gaussian2d},
            "surfel": {"gaussian_mode": GaussianMode.Gaussian2d, "aabb": True}}[shape]


def _basic(n, seed, view=None, fmt="f32", sh_gain=None, **kw):
    """`sh_gain`: every third splat's SH coefficients times this — colours of magnitude 5 and more, as the reference's
    tool scenes have (helpers.visibility_test_cloud: 6.0), and negative ones, below the sRGB knee."""
    def build():
        v = view() if view else _view()
        c = screen_cloud(v, n, seed, transform=kw.get("transform"))
        if sh_gain:
            c.spherical_harmonic[::3] *= np.float32(sh_gain)
        if fmt == "f16":   # binary16 holds the cloud's values (scale 7e4 would be inf: the formats' own test covers that)
            c = c.to_f16().to_f32()
        mn, mx = compute_aabb(c)
        base = dict(sort_mode=SortMode.Rayon, color_space=LIN, position_min=mn, position_max=mx, num_classes=5)
        base.update(kw)
        return c, v, CloudSettings(**base)
    return build


def _rank_count(k: int):
    """SortMode::Radix (keygen leaves the culled entries behind the draw list): exactly k splats in the frustum."""
    def build():
        v = _view()
        c = screen_cloud(v, 6000 if k > 1000 else 1200, 40 + k % 7)
        s = CloudSettings(color_space=LIN)
        keys = H.device_keys(c, v, s)
        inside, outside = np.nonzero(keys != 0xFFFFFFFF)[0], np.nonzero(keys == 0xFFFFFFFF)[0]
        assert len(inside) >= k and len(outside) >= 40
        pick = np.sort(np.concatenate([inside[:k], outside[:40]]))
        c = PlanarGaussian3d(c.position_visibility[pick], c.spherical_harmonic[pick], c.rotation[pick], c.scale_opacity[pick])
        return c, v, s
    return build


def _kept_chunk(n: int) -> np.ndarray:
    """A chunk as a sort of some earlier frame left it: a permutation of the splats, keys that have nothing to do with
    this frame's distances (stale), and every seventh entry dropped by a selection (key 0xFFFFFFFF)."""
    rng = np.random.default_rng(77)
    e = np.empty(n, dtype=[("key", np.uint32), ("index", np.uint32)])
    e["index"] = rng.permutation(n).astype(np.uint32)
    e["key"] = rng.integers(0, 0xFFFFFFF0, n, dtype=np.uint32)
    e["key"][::7] = 0xFFFFFFFF
    return e


def _srgb_cloud(shape):
    def build():
        c, v, s = _basic(2000, 61, **_shape(shape))()
        # SH colours of magnitude 5 to 15, as the reference's tool scenes have (helpers.visibility_test_cloud: 6.0), on a
        # third of the splats; a third near the 0.04045 knee (DC only just below / above 0.5 - 0.46 / 0.2821)
        sh = c.spherical_harmonic
        sh[0::3] *= np.float32(5.0)
        sh[1::3, 3:] *= np.float32(0.01)
        sh[1::3, :3] = (np.float32(-1.63) + np.float32(0.02) * np.random.default_rng(5).uniform(-1, 1, (len(sh[1::3]), 3))).astype(np.float32)
        return c, v, s
    return build


# ---- edge geometry, one class per cloud ------------------------------------------------------------------------------
def _frustum_boundary():
    v = _view()
    c = H.frustum_boundary_cloud(v, 40, 9)
    rng = np.random.default_rng(12)
    c.spherical_harmonic[:] = rng.uniform(-1, 1, c.spherical_harmonic.shape).astype(np.float32)
    # (the boundary cloud's splats are tiny: near |x/w| = 1.1 they are off the target; a screenful of ordinary ones beside them)
    d = screen_cloud(v, 200, 13)
    both = PlanarGaussian3d(np.concatenate([c.position_visibility, d.position_visibility]),
                            np.concatenate([c.spherical_harmonic, d.spherical_harmonic]),
                            np.concatenate([c.rotation, d.rotation]), np.concatenate([c.scale_opacity, d.scale_opacity]))
    return both, v, CloudSettings(sort_mode=SortMode.Rayon, color_space=LIN)


def _on_axis():
    """tests/test_oracle_golden.py's on-axis isotropic splat: the OBB's eigenvector is 0 / 0 exactly on the axis (every
    input finite, the quad NaN: visible, not drawn); off the axis the same splats are drawn; some lie behind the camera."""
    v = View.perspective(transform_from((0, 0, 0)), 128, 128)
    n = 160
    rng = np.random.default_rng(21)
    pv = np.zeros((n, 4), np.float32)
    pv[:, 2] = -rng.uniform(2.0, 30.0, n)
    pv[:, 3] = 1.0
    pv[40:120, :2] = rng.uniform(-1.0, 1.0, (80, 2))      # off the axis
    pv[120:, 2] *= -1.0                                    # behind the camera
    so = np.empty((n, 4), np.float32)
    so[:, :3] = rng.uniform(0.05, 0.4, n).astype(np.float32)[:, None]
    so[:, 3] = 0.6
    rot = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
    sh = rng.uniform(-1, 1, (n, 48)).astype(np.float32)
    return PlanarGaussian3d(pv, sh, rot, so), v, CloudSettings(sort_mode=SortMode.Rayon, color_space=LIN)


SCALE_EDGES = (1e-9, 6e-8, 7e4)


def _scales(shape):
    def build():
        c, v, s = _basic(1500, 31, **_shape(shape))()
        for k, val in enumerate(SCALE_EDGES):          # one axis, two axes, all three at the edge value
            c.scale_opacity[6 * k::60, 0] = val
            c.scale_opacity[6 * k + 1::60, :2] = val
            c.scale_opacity[6 * k + 2::60, :3] = val
        return c, v, s
    return build


def opacity_edges() -> np.ndarray:
    """1e-6, 1, 1.5 and e^-4.5 moved by up to 40 ulp either way: ln changes by an ulp every ~8 of them, and 9 + 2 ln
    steps through -2, -1, 0, 1, 2 ulp(9) = 9.5e-7 around the fmaxf(.., 1e-6) clamp of cutoff_radius."""
    near = [E45]
    lo = hi = E45
    for _ in range(40):
        lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(1))
        near += [lo, hi]
    return np.array([1e-6, 1.0, 1.5] + near, np.float32)


def _opacities(shape):
    def build():
        c, v, s = _basic(1500, 33, opacity_adaptive_radius=True, **_shape(shape))()
        ops = opacity_edges()
        c.scale_opacity[: 6 * len(ops), 3] = np.tile(ops, 6)
        return c, v, s
    return build


EDGE_ON_OFFSETS = (0.0, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 3e-3, 1e-2, 3e-2, 0.1, 0.3)
DEPTH_REACH_EPS = (0.0, 1e-7, -1e-7, 1e-6, -1e-6, 3e-6, -3e-6, 1e-5, -1e-5, 1e-4, -1e-4, 1e-3, -1e-3)


def _quat_to(normal):
    """Unit quaternions (w, x, y, z) whose rotation takes e_z to `normal`. The reference builds L = T R^T S with
    R = rotation_matrix(q) fed row-wise to a column-major constructor: a surfel's tangents are the rotation's images of
    e_x and e_y, its normal that of e_z."""
    ez = np.array([0.0, 0.0, 1.0])
    axis = np.cross(np.broadcast_to(ez, normal.shape), normal)
    s_, c_ = np.linalg.norm(axis, axis=1), normal @ ez
    ang = np.arctan2(s_, c_)
    axis = axis / np.maximum(s_, 1e-30)[:, None]
    return np.concatenate([np.cos(ang / 2)[:, None], np.sin(ang / 2)[:, None] * axis], axis=1)


def _edge_on(shape):
    """The two `< 1e-4` degeneracy tests of the 2DGS path, both outcomes of each. Two thirds of the cloud: surfels whose
    plane holds the camera's ray to them and the screen's x axis — edge-on, their projection a horizontal line, so the
    quad's y extent (bounding_box_cov2d: extent < 1e-4) vanishes — and the same tilted towards the camera by
    EDGE_ON_OFFSETS radians. The last third: surfels with one tangent along the view direction whose cutoff * scale
    reaches the camera plane to within DEPTH_REACH_EPS (cov2d_surfel: |d| < 1e-4, d = cutoff^2 (w_u^2 + w_v^2) - w^2)."""
    def build():
        v = View.perspective(transform_from((0, 0, 0)), 250, 130)
        c = screen_cloud(v, 1200, 35, depth=(3.0, 40.0), spread=0.9)
        n, m = len(c), 800
        pos = c.position_visibility[:, :3].astype(np.float64)
        ray = pos / np.linalg.norm(pos, axis=1, keepdims=True)           # camera at the origin, looking down -z
        n0 = np.cross(ray, np.array([1.0, 0.0, 0.0]))
        n0 /= np.linalg.norm(n0, axis=1, keepdims=True)                    # normal of the plane through the ray and the x axis
        off = np.array(EDGE_ON_OFFSETS)[np.arange(n) % len(EDGE_ON_OFFSETS)] * np.where(np.arange(n) % 2, 1.0, -1.0)
        normal = np.cos(off)[:, None] * n0 + np.sin(off)[:, None] * ray
        c.rotation[:] = _quat_to(normal).astype(np.float32)
        c.scale_opacity[:, :3] = np.stack([np.full(n, 0.6), np.full(n, 0.3), np.full(n, 0.01)], axis=1).astype(np.float32)
        c.scale_opacity[:, 3] = 0.5
        # the depth-reaching third: e_x goes to the view direction (0, 0, -1) (a quarter turn about y), e_y stays
        k = n - m
        rng = np.random.default_rng(36)
        w_p = rng.uniform(1.0, 6.0, k)
        c.position_visibility[m:, 0] = rng.uniform(-0.3, 0.3, k) * w_p
        c.position_visibility[m:, 1] = rng.uniform(-0.15, 0.15, k) * w_p
        c.position_visibility[m:, 2] = -w_p
        c.rotation[m:] = np.array([math.cos(math.pi / 4), 0.0, math.sin(math.pi / 4), 0.0], np.float32)
        eps = np.array(DEPTH_REACH_EPS)[np.arange(k) % len(DEPTH_REACH_EPS)]
        c.scale_opacity[m:, 0] = (w_p / 3.0 * (1.0 + eps)).astype(np.float32)
        c.scale_opacity[m:, 1] = 0.05
        c.position_visibility[::10, 2] *= -1.0      # a tenth of the splats behind the camera: culled
        return c, v, CloudSettings(sort_mode=SortMode.Rayon, color_space=LIN, opacity_adaptive_radius=False, **_shape(shape))
    return build


def _borders(w, h):
    """Small isotropic splats whose centres lie within +-8 px of each target border (in the frustum: |ndc| = 1.1 is 12 px
    beyond a 250-px border): quads that straddle the border, quads entirely beyond it by less than tile_rect's 1.5-px
    guard band (drawn), and quads beyond that (visible, not drawn)."""
    def build():
        v = _view(w, h)
        rng = np.random.default_rng(41)
        m = 150
        px, py = [], []
        for side in range(4):
            t = rng.uniform(-8.0, 8.0, m)
            along = rng.uniform(0.1, 0.9, m)
            px.append([t, w + t, along * w, along * w][side])
            py.append([along * h, along * h, t, h + t][side])
        px, py = np.concatenate(px), np.concatenate(py)
        n = len(px)
        inv = np.linalg.inv(np.asarray(v.clip_from_world, np.float64))
        near = float(np.asarray(v.clip_from_view, np.float64)[2, 3])
        dist = rng.uniform(8.0, 12.0, n)
        clip = np.stack([(2 * px / w - 1) * dist, (1 - 2 * py / h) * dist, np.full(n, near), dist], axis=1)
        wpos = clip @ inv.T
        c = random_gaussians_3d_seeded(n + 40, 43)
        c.position_visibility[:n, :3] = (wpos[:, :3] / wpos[:, 3:4]).astype(np.float32)
        c.position_visibility[n:, 2] = 50.0          # behind the camera: culled
        c.scale_opacity[:, :3] = rng.uniform(0.01, 0.06, n + 40).astype(np.float32)[:, None]
        c.scale_opacity[:, 3] = 0.7
        return c, v, CloudSettings(sort_mode=SortMode.Rayon, color_space=LIN, opacity_adaptive_radius=False)
    return build


def _scaled_transform():
    tr = transform_from((0.5, -0.25, 0.0), rotation_y(0.3))
    tr[:3, :3] *= np.float32(1.25)   # Transform::with_scale
    return tr


def all_cases() -> list:
    cases = []
    # rank counts around the 256-rank block of both project kernels (SortMode::Radix: the draw list is the frustum's prefix)
    for k in (1, 255, 256, 257, 3000):
        cases.append(Case(f"ranks_{k}", _rank_count(k), populated=False, rank_count=k, tags=("ranks",)))
    # every instantiation the launchers dispatch: format x ANY_MODE x quad shape (validate refuses cov3d x 2DGS)
    seed = 100
    for fmt in ("f32", "f16", "cov3d"):
        for shape in ("obb", "aabb", "obb2d", "surfel"):
            if fmt == "cov3d" and shape in ("obb2d", "surfel"):
                continue
            for any_mode in (False, True):
                seed += 1
                kw = dict(_shape(shape))
                if any_mode:
                    kw["rasterize_mode"] = RasterizeMode.Classification
                srgb = fmt != "cov3d" and shape in ("obb", "surfel") and not any_mode
                cases.append(Case(f"inst_{fmt}_{shape}_{'any' if any_mode else 'color'}", _basic(1200, seed, fmt=fmt, sh_gain=20.0 if srgb else None, **kw),
                                  fmt=fmt, srgb=srgb, tags=("instantiation",)))
    # settings
    cases.append(Case("adaptive_radius_off", _basic(1200, 201, opacity_adaptive_radius=False), tags=("settings",)))
    cases.append(Case("adaptive_radius_on_surfel", _basic(1200, 202, opacity_adaptive_radius=True, **_shape("surfel")), tags=("settings",)))
    cases.append(Case("global_scale_0p05", _basic(2000, 203, global_scale=0.05), tags=("settings",)))
    cases.append(Case("global_scale_0p05_aabb", _basic(2000, 204, global_scale=0.05, aabb=True), tags=("settings",)))
    for shape in ("obb", "surfel"):
        cases.append(Case(f"transform_scaled_{shape}", _basic(1500, 205, transform=_scaled_transform(), **_shape(shape)), tags=("settings",)))
    cases.append(Case("sh_degree_0", _basic(1200, 206, sh_degree=0, sh_gain=20.0), srgb=True, tags=("settings",)))
    cases.append(Case("sh_degree_3_aabb", _basic(1200, 207, sh_degree=3, aabb=True, sh_gain=20.0), srgb=True, tags=("settings",)))
    for mode in (RasterizeMode.Classification, RasterizeMode.Depth, RasterizeMode.Normal, RasterizeMode.Position, RasterizeMode.OpticalFlow):
        for shape in ("obb", "surfel"):
            cases.append(Case(f"mode_{mode.name}_{shape}", _basic(1200, 210 + int(mode), rasterize_mode=mode, transform=_scaled_transform(), **_shape(shape)),
                              tags=("mode",)))
    for dm in (DrawMode.Selected, DrawMode.HighlightSelected):
        for shape in ("obb", "aabb"):
            cases.append(Case(f"draw_{dm.name}_{shape}", _basic(1200, 220 + int(dm), draw_mode=dm, **_shape(shape)), tags=("settings",)))
    cases.append(Case("kept_order", _basic(2500, 230, sort_mode=SortMode.Radix), kept=_kept_chunk, tags=("settings",)))
    cases.append(Case("kept_order_surfel_f16", _basic(2500, 231, fmt="f16", sort_mode=SortMode.Radix, **_shape("surfel")), fmt="f16", kept=_kept_chunk,
                      tags=("settings",)))
    # targets: not multiples of 16; tile x up to 255 in the packed word
    # (37 x 21: |ndc| = 1.1 is less than two pixels beyond the border, inside tile_rect's guard band — no quad of a visible
    # splat misses the target; the 2D case's undrawn ranks are surfels smaller than the `extent < 1e-4` test lets through)
    cases.append(Case("target_37x21", _basic(1200, 240, view=lambda: _view(37, 21)), populated=False, tags=("target",)))
    cases.append(Case("target_37x21_obb2d", _basic(2500, 243, view=lambda: _view(37, 21), global_scale=0.005, **_shape("obb2d")), tags=("target",)))
    cases.append(Case("target_4096x64", _basic(3000, 241, view=lambda: _view(4096, 64)), tags=("target",)))
    cases.append(Case("target_4096x64_surfel", _basic(3000, 242, view=lambda: _view(4096, 64), **_shape("surfel")), tags=("target",)))
    # the one tolerance
    cases.append(Case("srgb_magnitudes_obb", _srgb_cloud("obb"), srgb=True, tags=("srgb",)))
    cases.append(Case("srgb_magnitudes_surfel", _srgb_cloud("surfel"), srgb=True, tags=("srgb",)))
    # edge geometry
    cases.append(Case("edge_frustum_boundary", _frustum_boundary, tags=("edge",)))
    cases.append(Case("edge_on_axis_nan_obb", _on_axis, tags=("edge",)))
    for shape in ("obb", "aabb", "surfel"):
        cases.append(Case(f"edge_scales_{shape}", _scales(shape), tags=("edge", "scales")))
    for shape in ("obb", "surfel"):
        cases.append(Case(f"edge_opacities_{shape}", _opacities(shape), tags=("edge", "opacities")))
    for shape in ("obb2d", "surfel"):
        cases.append(Case(f"edge_on_surfels_{shape}", _edge_on(shape), tags=("edge", "edge_on")))
    cases.append(Case("edge_borders_250x130", _borders(250, 130), tags=("edge", "borders")))
    return cases


CASES = all_cases()
CASE_NAMES = [c.name for c in CASES]


def by_name(name: str) -> Case:
    return CASES[CASE_NAMES.index(name)]


_twins: dict = {}


def twin_of(case: Case, color_space=None) -> dict:
    """The case built and projected by the host twin, once per (case, colour space): cloud, view, settings, the draw list
    and the full list, the twin's output (helpers.twin_project) and the record words made of it."""
    key = (case.name, color_space)
    if key not in _twins:
        cloud, view, settings = case.build()
        if color_space is not None:
            settings.color_space = color_space
        kept = case.kept(len(cloud)) if case.kept else None
        draw, full = H.twin_draw_list(cloud, view, settings, kept)
        twin = H.twin_project(cloud, view, settings, draw, case.fmt, full)
        records, rects, drawn = H.twin_record_words(twin)
        _twins[key] = dict(cloud=cloud, view=view, settings=settings, kept=kept, draw_list=draw, twin=twin, records=records,
                           rects=rects, drawn=drawn)
    return _twins[key]
