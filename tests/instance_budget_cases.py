"""BINNING_SORT's tile-instance budget: the cases and references of tests/test_instance_budget_host.py and
tests/test_instance_budget_gpu.py. Integer work throughout: every check made with these is an equality of counts or bytes.

What is pinned (csrc/render_kernels.hip project_emit_kernel, csrc/bgs_frame.hip check_capacities, csrc/adaptive_state.h
instance_capacity_for): the last block's verdict `total > capacity` on a 64-bit chained total, the host's answer (the next
power of two that holds 1.25 x the need, within [2^22, 2^30], one re-run on the lane) and the refusal past 2^30.

The clouds are the smallest that reach those edges. A COVER splat lies in the frustum and is so large that its packed tile
rectangle is the whole target: exactly tiles_x * tiles_y instances whatever the view, and an alpha of at least 0.9 at
every pixel, so that a pixel is saturated after a few records and the rasteriser's work stays small. A DOT is a tiny splat
in the middle of a tile, in front of the covers. The host twin (helpers.twin_project) decides every count: a case is
built, projected by the twin, and held to its total by tests/test_instance_budget_host.py.

Excess of `one_over`: the twin draws a dot of 0.002 world units at a tile centre into ONE tile, so the case's total is
2^22 + 1 — the smallest overflow there is."""
from dataclasses import dataclass

import numpy as np

import bin_stage_cases as B
import helpers as H
from bevy_gaussian_splatting_amd import CloudSettings, PlanarGaussian3d, View, random_gaussians_3d_seeded

MIN_CAPACITY, MAX_CAPACITY = 1 << 22, 1 << 30   # csrc/adaptive_state.h; tests/test_adaptive_state_host.py holds them to it
TILE_PX = 16
COVER_OPACITY = 0.95
ALPHA_FLOOR = 0.9
CAMERA = (0.0, 1.5, 5.0)      # View.headless: looks down -Z with a vertical field of view of pi / 4
DOT_Z = 1.0                   # the dots' plane: 4 units in front of the camera, nearer than every cover


@dataclass(frozen=True)
class Case:
    name: str
    size: tuple      # target, pixels
    covers: int
    dots: int        # one-tile dots in front of the covers
    total: int       # tile instances the twin must count

    @property
    def tiles(self) -> tuple:
        return -(-self.size[0] // TILE_PX), -(-self.size[1] // TILE_PX)


CASES = (
    Case("at_capacity", (256, 256), 16384, 0, 1 << 22),                 # == the minimum capacity: no overflow
    Case("one_over", (256, 256), 16384, 1, (1 << 22) + 1),              # the smallest overflow: one re-run, 2^23
    Case("second_growth", (256, 256), 36000, 0, 36000 * 256),           # in (2^23, 1.25 * 2^23]: the next re-run, 2^24
    Case("head_room", (256, 256), 27000, 0, 27000 * 256),               # in (2^23 / 1.25, 2^23]: fits 2^23, grows to 2^24 all the same
    Case("refused_2pow30", (4096, 4096), 16385, 0, (1 << 30) + 65536),  # tx1 = ty1 = 255, the packed word's maximum
    Case("carry_2pow32", (4096, 4096), 65537, 0, (1 << 32) + 65536),    # instance_total_hi = 1
)
CASE_NAMES = tuple(c.name for c in CASES)


def by_name(name: str) -> Case:
    return CASES[CASE_NAMES.index(name)]


def view_of(case: Case, yaw: float = 0.0) -> View:
    return View.headless(case.size[0], case.size[1], yaw=yaw, msaa_samples=4)


def settings_of(case: Case) -> CloudSettings:
    return CloudSettings()


def _cover_rows(n: int):
    """n cover splats: centres in a small box around the view axis (never on it: an isotropic splat on the axis has no
    major axis and is not drawn), scales of 80-110 world units, colours of their own."""
    rng = np.random.default_rng(2230)
    pos = np.stack([rng.uniform(0.05, 0.3, n) * rng.choice([-1.0, 1.0], n), 1.5 + rng.uniform(0.05, 0.3, n) * rng.choice([-1.0, 1.0], n),
                    rng.uniform(-1.0, 0.0, n)], axis=1)
    scale = np.array([100.0, 90.0, 80.0]) * (1.0 + 0.1 * rng.random((n, 1)))
    sh = np.zeros((n, 48), np.float32)
    sh[:, :3] = rng.uniform(-1.5, 1.5, (n, 3))
    return pos, scale, np.full(n, COVER_OPACITY), sh


def _dot_rows(case: Case, n: int):
    """n dots at the centres of tiles spread over the target, on the plane z = DOT_Z."""
    tx, ty = case.tiles
    half = (CAMERA[2] - DOT_Z) * np.tan(np.pi / 8.0)
    k = np.arange(n)
    px = TILE_PX * ((3 + 5 * k) % tx) + TILE_PX / 2
    py = TILE_PX * ((2 + 7 * k) % ty) + TILE_PX / 2
    pos = np.stack([(2.0 * px / case.size[0] - 1.0) * half * case.size[0] / case.size[1], CAMERA[1] + (1.0 - 2.0 * py / case.size[1]) * half,
                    np.full(n, DOT_Z)], axis=1)
    sh = np.zeros((n, 48), np.float32)
    sh[:, 0] = 3.0
    return pos, np.full((n, 3), 0.002) * np.array([1.0, 0.9, 0.8]), np.full(n, 1.0), sh


def cloud_of(case: Case) -> PlanarGaussian3d:
    """The case's cloud: its covers (splats 0 .. covers - 1), then its dots."""
    parts = [_cover_rows(case.covers)] + ([_dot_rows(case, case.dots)] if case.dots else [])
    pos, scale, opacity, sh = (np.concatenate([p[i] for p in parts]) for i in range(4))
    n = len(pos)
    pv = np.concatenate([pos, np.ones((n, 1))], axis=1).astype(np.float32)
    so = np.concatenate([scale, opacity[:, None]], axis=1).astype(np.float32)
    return PlanarGaussian3d(pv, sh.astype(np.float32), np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1)), so)


_BUILT = {}


def built(name: str, yaw: float = 0.0) -> dict:
    """The case's cloud, view, settings and what the twin makes of them: draw list, twin, packed rectangle per rank and the
    instance total. Built once per (case, yaw)."""
    key = (name, yaw)
    if key not in _BUILT:
        case = by_name(name)
        cloud, view, settings = cloud_of(case), view_of(case, yaw), settings_of(case)
        draw, full = H.twin_draw_list(cloud, view, settings)
        twin = H.twin_project(cloud, view, settings, draw, full_entries=full)
        _, rects, drawn = H.twin_record_words(twin)
        _BUILT[key] = {"case": case, "cloud": cloud, "view": view, "settings": settings, "draw": draw, "twin": twin, "rects": rects,
                       "drawn": drawn, "total": H.twin_instances(twin)}
    return _BUILT[key]


def cover_alpha_floor(d: dict) -> np.ndarray:
    """Per cover splat of the draw list, the smallest alpha it has at a pixel centre of the target: min(exp(-4.5 r^2) a,
    0.999) with r^2 = |M (pixel - centre)|^2 (helpers.emulate_render, the 3D OBB quad). r^2 is a convex function of the
    pixel, so over the rectangle of pixel centres it is largest at one of the four corner pixels."""
    twin, (w, h) = d["twin"], d["case"].size
    is_cover = d["draw"]["index"] < d["case"].covers
    p, cx, cy = twin["p"].astype(np.float64), twin["cx"].astype(np.float64), twin["cy"].astype(np.float64)
    r2 = np.zeros(len(cx))
    for x in (0.5, w - 0.5):
        for y in (0.5, h - 0.5):
            dx, dy = x - cx, y - cy
            r2 = np.maximum(r2, (p[:, 0] * dx + p[:, 1] * dy) ** 2 + (p[:, 2] * dx + p[:, 3] * dy) ** 2)
    return np.minimum(np.exp(-4.5 * r2) * twin["color"][:, 3].astype(np.float64), 0.999)[is_cover]


_REFS = {}


def reference(name: str):
    """bin_stage_cases.reference_instances of the case's rectangles: (sorted instances, ranges, present). Once per case."""
    if name not in _REFS:
        _REFS[name] = B.reference_instances(built(name)["rects"])
    return _REFS[name]


def capacity_for(need: int):
    """The growth rule in three lines (None: refused)."""
    if need > MAX_CAPACITY:
        return None
    return min(next(1 << k for k in range(22, 64) if (1 << k) >= need + need // 4), MAX_CAPACITY)


def ordinary_frame():
    """An everyday frame for 'the context still draws': 6000 seeded splats at 160 x 96."""
    return random_gaussians_3d_seeded(6000, 41), View.headless(160, 96, msaa_samples=4), CloudSettings()
