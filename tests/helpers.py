"""Shared test helpers: scene builders, the host shim of the device math header, and a numpy
emulation of the device pipeline's DATA FLOW (keys -> stable sort -> records -> front-to-back
tile blend) that lets the product's per-splat arithmetic be checked against the oracle on a
machine without a GPU. None of this is a product path."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

from bevy_gaussian_splatting_amd import (
    CloudSettings, GaussianMode, PlanarGaussian3d, SortMode, View, random_gaussians_3d_seeded)
from bevy_gaussian_splatting_amd.camera import BgsView
from bevy_gaussian_splatting_amd.gaussian import Gaussian3d, SphericalHarmonicCoefficients
from bevy_gaussian_splatting_amd.settings import BgsSettings

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_DIR = os.path.join(HERE, "host_shim")
SHIM_SRC = os.path.join(SHIM_DIR, "device_math_shim.cpp")
SHIM_LIB = os.path.join(SHIM_DIR, "libdevice_math_shim.so")
CSRC = os.path.join(HERE, "..", "bevy_gaussian_splatting_amd", "csrc")


class FrameParamsC(ctypes.Structure):
    """ctypes image of bgs::FrameParams (bevy_gaussian_splatting_amd/csrc/bgs_device.h)."""

    _fields_ = [
        ("transform", ctypes.c_float * 16),
        ("view_from_world", ctypes.c_float * 16),
        ("clip_from_world", ctypes.c_float * 16),
        ("cam", ctypes.c_float * 3),
        ("focal_x", ctypes.c_float), ("focal_y", ctypes.c_float),
        ("viewport_w", ctypes.c_float), ("viewport_h", ctypes.c_float),
        ("global_opacity", ctypes.c_float), ("global_scale", ctypes.c_float),
        ("n", ctypes.c_uint32), ("key_shift", ctypes.c_uint32),
        ("gaussian_mode", ctypes.c_uint32), ("aabb", ctypes.c_uint32),
        ("adaptive_radius", ctypes.c_uint32), ("color_space", ctypes.c_uint32),
        ("sh_degree", ctypes.c_uint32), ("sort_mode", ctypes.c_uint32),
        ("width", ctypes.c_int32), ("height", ctypes.c_int32),
        ("tiles_x", ctypes.c_int32), ("tiles_y", ctypes.c_int32),
        ("debug", ctypes.c_uint32),
        ("rasterize_mode", ctypes.c_uint32), ("num_classes", ctypes.c_uint32),
        ("pos_min", ctypes.c_float * 3), ("pos_max", ctypes.c_float * 3),
        ("draw_mode", ctypes.c_uint32),
        ("prev_clip_from_world", ctypes.c_float * 16), ("delta_time", ctypes.c_float),
        ("clear", ctypes.c_float * 4), ("srgb8_target", ctypes.c_uint64),
        ("sort_path", ctypes.c_uint32), ("sample_count", ctypes.c_uint32), ("depth_ptr", ctypes.c_uint64),
        ("basis", ctypes.c_float * 9), ("inv_viewport_w", ctypes.c_float), ("inv_viewport_h", ctypes.c_float),
        ("visualize_bbox", ctypes.c_uint32),
    ]


class ScratchLayoutC(ctypes.Structure):
    """ctypes image of bgs::ScratchLayout (bevy_gaussian_splatting_amd/csrc/frame_params.h)."""

    REGIONS = ("off_depth_status", "off_scan_status", "off_tile_status", "off_ranges", "off_bin_status", "off_part_status",
               "off_ctl1")   # in address order, behind the first Control block at 0
    _fields_ = ([("bytes", ctypes.c_uint64)] + [(r, ctypes.c_uint64) for r in REGIONS] +
                [("depth_tiles", ctypes.c_uint64), ("inst_tiles", ctypes.c_uint64), ("inst_cap", ctypes.c_uint64),
                 ("n", ctypes.c_uint32), ("pass_stride", ctypes.c_uint32)])


# what shim_control_offsets reports, in its order: everything in 32-bit words (bucket_max_keys: BUCKET_MAX, the length of
# Control::splitters and Control::bucket_count)
CONTROL_FIELDS = ("words", "header_words", "draw_count", "instance_count", "error", "visible_count", "splat_count", "sort_overflow",
                  "bucket_max", "strip_tiles", "saturated_tiles_prev", "ticket", "color_max_bits", "hist_depth", "coarse_total",
                  "splitters", "bucket_count", "bucket_max_keys")


def header_version() -> int:
    """(BGS_VERSION_MAJOR << 16) | BGS_VERSION_MINOR as include/bgs.h defines them: what bgs_version() returns."""
    import re
    header = open(os.path.join(HERE, "..", "include", "bgs.h")).read()
    major, minor = (int(re.search(rf"^#define\s+BGS_VERSION_{part}\s+(\d+)u?\b", header, re.M).group(1)) for part in ("MAJOR", "MINOR"))
    return (major << 16) | minor


def control_offsets() -> dict:
    """Word offsets of the fields of a Control block (csrc/bgs_device.h), from the host build of the header itself."""
    out = (ctypes.c_uint32 * 32)()
    got = shim().shim_control_offsets(out)
    assert got == len(CONTROL_FIELDS)
    return {name: int(out[i]) for i, name in enumerate(CONTROL_FIELDS)}


def scratch_layout(n: int, inst_cap: int) -> ScratchLayoutC:
    out = ScratchLayoutC()
    shim().shim_scratch_layout(n, inst_cap, ctypes.byref(out))
    return out


class ShimOut(ctypes.Structure):
    _fields_ = [
        ("visible", ctypes.c_int32), ("draw", ctypes.c_int32),
        ("color", ctypes.c_float * 4),
        ("cx", ctypes.c_float), ("cy", ctypes.c_float),
        ("p", ctypes.c_float * 5),
        ("radius", ctypes.c_float),
        ("tx0", ctypes.c_int32), ("ty0", ctypes.c_int32), ("tx1", ctypes.c_int32), ("ty1", ctypes.c_int32),
        ("mean", ctypes.c_float * 2),
        ("T", ctypes.c_float * 9),
        ("quad_m", ctypes.c_float * 4),
        ("bounds", ctypes.c_float * 4),
        ("ndc_z", ctypes.c_float),
    ]


# what shim_state_get reports of an AdaptiveState (csrc/adaptive_state.h), in its order; kinds / learning: their sizes
STATE_FIELDS = ("draw_hint", "draw_hint_valid", "draw_shrink_votes", "sup_level", "coarse_cap_hint", "list_shrink_votes", "split_epoch",
                "split_failed_epoch", "bucket_block", "bucket_fail_streak", "cur_kind", "kinds", "learning")

_shim = None


def shim() -> ctypes.CDLL:
    """Build (g++, -ffp-contract=off) and load the host shim of splat_math.h."""
    global _shim
    if _shim is not None:
        return _shim
    deps = [SHIM_SRC, os.path.join(CSRC, "..", "..", "include", "bgs_diag.h")] + [os.path.join(CSRC, f) for f in ("splat_math.h", "exact_log.h", "bgs_device.h", "frame_params.h", "adaptive_state.h", "device_buffer.h")]
    if not os.path.exists(SHIM_LIB) or any(os.path.getmtime(d) > os.path.getmtime(SHIM_LIB) for d in deps):
        subprocess.run(
            ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-shared", "-fPIC",
             "-Wno-unknown-pragmas", SHIM_SRC, "-o", SHIM_LIB], check=True, capture_output=True)
    l = ctypes.CDLL(SHIM_LIB)
    fp = ctypes.POINTER(ctypes.c_float)
    l.shim_fill_params.argtypes = [ctypes.c_uint32, ctypes.POINTER(BgsView), ctypes.POINTER(BgsSettings),
                                   ctypes.POINTER(FrameParamsC)]
    l.shim_fill_params.restype = None
    l.shim_ln_f32.argtypes = [fp, ctypes.c_uint32, fp]
    l.shim_ln_f32.restype = None
    l.shim_ln_f32_checksum.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    l.shim_ln_f32_checksum.restype = ctypes.c_uint64
    l.shim_xcd_runs_items.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    l.shim_xcd_runs_items.restype = None
    l.shim_supertile_div.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    l.shim_supertile_div.restype = ctypes.c_uint32
    l.shim_next_supertile_level.argtypes = [ctypes.c_double, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                            ctypes.POINTER(ctypes.c_double)]
    l.shim_next_supertile_level.restype = ctypes.c_uint32
    l.shim_pow2_ceil.argtypes = [ctypes.c_uint64]
    l.shim_pow2_ceil.restype = ctypes.c_uint32
    l.shim_splitters_ascending.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32]
    l.shim_splitters_ascending.restype = ctypes.c_int
    l.shim_frame_params_size.argtypes = []
    l.shim_frame_params_size.restype = ctypes.c_uint32
    l.shim_sort_keys.argtypes = [ctypes.POINTER(FrameParamsC), fp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    l.shim_sort_keys.restype = None
    l.shim_sort_keys_two_step.argtypes = [ctypes.POINTER(FrameParamsC), fp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                          ctypes.POINTER(ctypes.c_uint32)]
    l.shim_sort_keys_two_step.restype = None
    l.shim_project.argtypes = [ctypes.POINTER(FrameParamsC), ctypes.c_uint32, fp, fp, fp, fp, fp, ctypes.POINTER(ShimOut)]
    l.shim_project.restype = None
    l.shim_project_batch.argtypes = [ctypes.POINTER(FrameParamsC), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, fp, fp, fp, fp, fp, fp,
                                     ctypes.POINTER(ShimOut), fp]
    l.shim_project_batch.restype = None
    l.shim_surfel_probe.argtypes = [ctypes.POINTER(FrameParamsC), fp, fp, fp, fp]
    l.shim_surfel_probe.restype = None
    l.shim_distance_to_camera.argtypes = [ctypes.POINTER(FrameParamsC), fp]
    l.shim_distance_to_camera.restype = ctypes.c_float
    l.shim_scratch_layout.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(ScratchLayoutC)]
    l.shim_scratch_layout.restype = None
    l.shim_control_offsets.argtypes = [ctypes.POINTER(ctypes.c_uint32)]
    l.shim_control_offsets.restype = ctypes.c_uint32
    l.shim_scratch_layout_size.argtypes = []
    l.shim_scratch_layout_size.restype = ctypes.c_uint32
    i64p, u64p, vp = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p
    for name, args, res in (("shim_mem_reset", [ctypes.c_int64], None), ("shim_mem_counters", [i64p], None),
                            ("shim_buf_new", [], vp), ("shim_buf_delete", [vp], None),
                            ("shim_buf_reserve", [vp, ctypes.c_uint64, ctypes.c_int64], ctypes.c_int),
                            ("shim_buf_reset", [vp], None), ("shim_buf_state", [vp, u64p], None),
                            ("shim_buf_move_assign", [vp, vp], None), ("shim_buf_move_new", [vp], vp),
                            ("shim_buf_release_and_free", [vp], None),
                            ("shim_buf_reserve_group", [vp, vp, vp, ctypes.c_uint64], ctypes.c_int)):
        getattr(l, name).argtypes, getattr(l, name).restype = args, res
    # the learnt state and its rules (adaptive_state.h): st is shim_state_new's handle, a cloud is (identity, n)
    u32, u64, cint, u32p = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)
    viewp, setp = ctypes.POINTER(BgsView), ctypes.POINTER(BgsSettings)
    for name, args, res in (("shim_state_new", [], vp), ("shim_state_delete", [vp], None),
                            ("shim_frame_kind", [u32, u32, viewp, setp], u64),
                            ("shim_instance_capacity_for", [u64, u64p], u64),
                            ("shim_state_switch_kind", [vp, u64], None), ("shim_state_settle", [vp, u64, u32], None),
                            ("shim_state_completed_early", [vp, u64], None), ("shim_state_learn_saturation", [vp, u64, u32], None),
                            ("shim_state_learn_draw_count", [vp, u32], None),
                            ("shim_state_find_splitter_slot", [vp, vp, u32, viewp, setp], cint),
                            ("shim_state_store_splitters", [vp, u32p, u32, u32, u32, vp, u32, viewp, setp, u64], None),
                            ("shim_state_frame_enqueued", [vp, u32, cint, u64], None),
                            ("shim_state_learn_bucket_sort", [vp, u32, cint, u64], cint),
                            ("shim_state_list_capacity", [vp, u32, cint], u32),
                            ("shim_state_learn_list_capacity", [vp, u32, u32, u32], cint),
                            ("shim_state_learn_level", [vp, u64, u32, u32p, u64, u32, u32], cint),
                            ("shim_state_distrust", [vp], None), ("shim_state_forget_cloud", [vp, vp], None),
                            ("shim_state_reset", [vp], None), ("shim_state_get", [vp, u64p], None),
                            ("shim_state_slot", [vp, cint, u64p, fp, u32p, u32], None),
                            ("shim_state_kind", [vp, u64, u32p, ctypes.POINTER(cint)], cint)):
        getattr(l, name).argtypes, getattr(l, name).restype = args, res
    assert l.shim_frame_params_size() == ctypes.sizeof(FrameParamsC)
    assert l.shim_scratch_layout_size() == ctypes.sizeof(ScratchLayoutC)
    _shim = l
    return l


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def frame_params(n: int, view: View, settings: CloudSettings) -> FrameParamsC:
    fpc = FrameParamsC()
    v, s = view.to_native(), settings.to_native()
    shim().shim_fill_params(n, ctypes.byref(v), ctypes.byref(s), ctypes.byref(fpc))
    return fpc


def device_keys(cloud: PlanarGaussian3d, view: View, settings: CloudSettings) -> np.ndarray:
    """Keys exactly as keygen_kernel writes them (SORT_RAYON keys still inverted)."""
    fpc = frame_params(len(cloud), view, settings)
    keys = np.empty(len(cloud), np.uint32)
    shim().shim_sort_keys(ctypes.byref(fpc), _fp(cloud.position_visibility), len(cloud),
                          keys.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    return keys


def device_keys_two_step(cloud: PlanarGaussian3d, view: View, settings: CloudSettings):
    """The same keys computed the way the chainless keygen tiles do (straight-line frustum verdict, divisions only where
    it is unsure), and how many splats took the divisions."""
    fpc = frame_params(len(cloud), view, settings)
    keys = np.empty(len(cloud), np.uint32)
    unsure = ctypes.c_uint32(0)
    shim().shim_sort_keys_two_step(ctypes.byref(fpc), _fp(cloud.position_visibility), len(cloud),
                                   keys.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(unsure))
    return keys, int(unsure.value)


def device_sorted_entries(cloud, view, settings) -> np.ndarray:
    """What bgs_sort must return, derived from the product's key arithmetic + a stable sort."""
    keys = device_keys(cloud, view, settings)
    n = len(cloud)
    out = np.empty(n, dtype=[("key", np.uint32), ("index", np.uint32)])
    if settings.sort_mode == SortMode.NONE:
        out["key"], out["index"] = keys, np.arange(n, dtype=np.uint32)
        return out
    order = np.argsort(keys, kind="stable").astype(np.uint32)
    out["index"] = order
    out["key"] = keys[order]
    if settings.sort_mode in (SortMode.Rayon, SortMode.Std):
        out["key"] = ~out["key"]
    return out


def emulate_render(cloud: PlanarGaussian3d, view: View, settings: CloudSettings, entries=None, cov3d: bool = False) -> np.ndarray:
    """numpy emulation of project_emit + raster: records from the HOST BUILD of splat_math.h,
    composited front-to-back per pixel exactly as raster_kernel does (same record fields, same
    formulas), without tiling. Small scenes only. `cov3d`: the records of the cloud's precomputed-covariance form
    (project_splat's cov3d_pre argument, through shim_project_batch)."""
    if entries is None:
        entries = device_sorted_entries(cloud, view, settings)
    depth = getattr(view, "depth_host", None)   # [H, W, samples] scene depth (random_case), or None
    n = len(cloud)
    W, H = view.width, view.height
    fpc = frame_params(n, view, settings)
    sentinel = np.uint32(0xFFFFFFFF >> fpc.key_shift)
    if settings.sort_mode == SortMode.Radix:
        count = int((entries["key"] != sentinel).sum())
    else:
        count = n
    qx, qy = np.meshgrid(np.arange(W, dtype=np.float32) + np.float32(0.5),
                         np.arange(H, dtype=np.float32) + np.float32(0.5))
    # samples per pixel: offsets from the pixel centre (csrc/render_kernels.hip: MS_OX0 ... — the standard 4x pattern)
    S = int(view.msaa_samples)
    offs = {1: [(0.0, 0.0)], 2: [(0.25, 0.25), (-0.25, -0.25)],
            4: [(-0.125, -0.375), (0.375, -0.125), (-0.375, 0.125), (0.125, 0.375)],
            8: [(k / 16.0, l / 16.0) for k, l in ((1, -3), (-1, 3), (5, 1), (-3, -5), (-5, 5), (-7, -1), (3, 7), (7, -7))]}[S]
    T = np.ones((H, W, S), np.float32)   # per-sample transmittance
    C = np.zeros((H, W, 3), np.float32)
    out = ShimOut()
    surfel = settings.gaussian_mode == GaussianMode.Gaussian2d and settings.aabb
    eps = None   # frame_t_eps of csrc/render_kernels.hip, from the largest colour magnitude of the drawn records
    # Depth mode: range from sorted[count-1] and sorted[1] of the FULL entry list (gaussian.wgsl:331-340)
    depth_range = np.zeros(2, np.float32)
    if n > 0:
        i_first, i_last = int(entries[min(1, n - 1)]["index"]), int(entries[n - 1]["index"])
        depth_range[0] = shim().shim_distance_to_camera(ctypes.byref(fpc), _fp(cloud.position_visibility[i_last]))
        depth_range[1] = shim().shim_distance_to_camera(ctypes.byref(fpc), _fp(cloud.position_visibility[i_first]))
    outs = twin_project(cloud, view, settings, entries[:count], fmt="cov3d", full_entries=entries)["raw"] if cov3d else None

    def project(j):
        nonlocal out
        if outs is not None:
            out = outs[count - 1 - j]
            return bool(out.draw)
        e = entries[count - 1 - j]
        si = int(e["index"])
        shim().shim_project(ctypes.byref(fpc), int(e["key"]), _fp(cloud.position_visibility[si]),
                            _fp(cloud.rotation[si]), _fp(cloud.scale_opacity[si]),
                            _fp(cloud.spherical_harmonic[si]), _fp(depth_range), ctypes.byref(out))
        return bool(out.draw)
    cmax = np.float32(0.0)
    for j in range(count):
        if project(j):
            mags = [abs(np.float32(v)) for v in out.color[:3]]
            cmax = max([cmax] + [m for m in mags if not np.isnan(m)])   # fmaxf drops a NaN
    with np.errstate(all="ignore"):
        eps = np.minimum(np.float32(1.0 / 8192.0), np.float32(1.0 / 2048.0) / np.float32(cmax))
    for j in range(count):
        if not project(j):
            continue
        dx = qx - np.float32(out.cx)
        dy = qy - np.float32(out.cy)
        p = [np.float32(v) for v in out.p]
        col = [np.float32(v) for v in out.color]
        with np.errstate(all="ignore"):
            if not settings.aabb:
                u = p[0] * dx + p[1] * dy
                v = p[2] * dx + p[3] * dy
                cov = [(np.abs(u + (p[0] * np.float32(ox) + p[1] * np.float32(oy))) <= 1) &
                       (np.abs(v + (p[2] * np.float32(ox) + p[3] * np.float32(oy))) <= 1) for ox, oy in offs]
                # fs_main's OBB discard (gaussian.wgsl:481-483): only a fragment shaded at a centre outside a small quad gets there
                hit = ~((u * u + v * v) > np.float32(9.0))
                sigma = np.float32(1.0) / np.float32(3.0)
                power = (u * u + v * v) * (np.float32(-1.0) / (np.float32(2.0) * sigma * sigma))
            elif not surfel:
                u = p[0] * dx
                v = p[1] * dy
                cov = [(np.abs(u + p[0] * np.float32(ox)) <= 1) & (np.abs(v + p[1] * np.float32(oy)) <= 1) for ox, oy in offs]
                power = np.float32(-0.5) * (p[2] * u * u + p[4] * v * v) + p[3] * u * v
                hit = ~(power > 0)
            else:
                u = p[0] * dx
                v = p[1] * dy
                cov = [(np.abs(u + p[0] * np.float32(ox)) <= 1) & (np.abs(v + p[1] * np.float32(oy)) <= 1) for ox, oy in offs]
                hit = np.ones_like(u, bool)
                rad = np.float32(out.radius)
                mx, my = np.float32(out.mean[0]), np.float32(out.mean[1])
                pcx = u * rad + mx
                pcy = v * rad * (np.float32(W) / np.float32(H)) + my
                Tm = [np.float32(t) for t in out.T]
                hu = [pcx * Tm[6 + i] - Tm[i] for i in range(3)]
                hv = [pcy * Tm[6 + i] - Tm[3 + i] for i in range(3)]
                cpx = hu[1] * hv[2] - hv[1] * hu[2]
                cpy = hu[2] * hv[0] - hv[2] * hu[0]
                cpz = hu[0] * hv[1] - hv[0] * hu[1]
                us, vs = cpx / cpz, cpy / cpz
                s3 = us * us + vs * vs
                s2 = np.float32(2.0) * ((mx - pcx) ** 2 + (my - pcy) ** 2)
                power = np.float32(-0.5) * np.minimum(s3, s2)
                hit &= ~(power > 0)
            alpha = np.minimum(np.exp(power) * col[3], np.float32(0.999)).astype(np.float32)
            if settings.visualize_bounding_box:   # the quad's frame (csrc/render_kernels.hip: BBOX_EDGE), per pixel
                frame = np.maximum(np.abs(u), np.abs(v)) > np.float32(0.84)
                alpha = np.where(frame, np.float32(1.0), alpha).astype(np.float32)
                col = [np.where(frame, np.float32(c0), c1).astype(np.float32) for c0, c1 in zip((0.3, 1.0, 0.1), col[:3])] + [col[3]]
        # the fragment is shaded once (at the pixel centre); a pixel stops once its MEAN transmittance is below the cut-off
        hit &= ~(T.mean(axis=2) < eps)
        covered = np.stack(cov, axis=2) & hit[..., None]
        if depth is not None:   # per-sample depth test: GreaterEqual against the reverse-Z scene depth, no write
            covered &= np.float32(out.ndc_z) >= depth
        w = (np.where(covered, T, np.float32(0)).mean(axis=2) * alpha).astype(np.float32)
        C[..., 0] += w * col[0]
        C[..., 1] += w * col[1]
        C[..., 2] += w * col[2]
        T = np.where(covered, T * (np.float32(1) - alpha)[..., None], T).astype(np.float32)
    clear = np.asarray(view.clear_color, np.float32)
    img = np.empty((H, W, 4), np.float32)
    T = T.mean(axis=2).astype(np.float32)   # the resolve: mean of the samples
    img[..., :3] = C + T[..., None] * clear[:3]
    img[..., 3] = (np.float32(1) - T) + T * clear[3]
    return img


# ---- the host twin of the device's vertex stage, for whole draw lists (tests/test_vertex_stage_*.py) -----------------
RECT_EMPTY = 0x000000FF   # csrc/bgs_device.h; tests/test_vertex_stage_host.py holds it to the header
# the float4 lanes of a record in project_rank's order (csrc/render_kernels.hip): Record 3 x float4, RecordSurfel 6 x float4
RECORD_FIELDS = ("cx", "cy", "p0", "p1", "p2", "p3", "p4", "r", "g", "b", "a", "z")
SURFEL_FIELDS = ("cx", "cy", "m00", "m11", "radius", "mean_x", "mean_y") + tuple(f"T{i}" for i in range(9)) + \
                ("r", "g", "b", "a", "z", "pad0", "pad1", "pad2")
COLOR_FIELDS = ("r", "g", "b")


def twin_draw_list(cloud, view, settings, kept=None):
    """(draw list, full list) of a frame as the device forms them, from the host build of the key arithmetic: the
    drawable prefix of the sorted entries — SortMode::Radix leaves the culled keys behind it, the other modes keep every
    splat — or, for a kept order (`kept`: the caller's chunk), the entries entry_kept (csrc/entries_math.h) lets through,
    in chunk order; the full list is the draw list followed by the rest (RasterizeMode::Depth reads its ends)."""
    n = len(cloud)
    if kept is not None:
        keep = (kept["key"] != 0xFFFFFFFF) & (kept["index"] < n)
        tail = kept[~keep].copy()
        tail["index"] = np.where(tail["index"] < n, tail["index"], n - 1)
        return kept[keep].copy(), np.concatenate([kept[keep], tail])
    full = device_sorted_entries(cloud, view, settings)
    if settings.sort_mode == SortMode.Radix:
        sentinel = np.uint32(0xFFFFFFFF >> frame_params(n, view, settings).key_shift)
        return full[: int((full["key"] != sentinel).sum())].copy(), full
    return full.copy(), full


def twin_project(cloud: PlanarGaussian3d, view: View, settings: CloudSettings, entries, fmt: str = "f32", full_entries=None) -> dict:
    """project_splat's host build over a whole draw list, as project_rank calls it for the cloud format `fmt`: "f32",
    "f16" (the planes encoded and decoded: f16 -> f32 is exact, so the twin sees what the device's loads see) or "cov3d"
    (the Covariance3dOpacity plane, project_splat's cov3d_pre). Arrays in ENTRY order (the device's rank j is entry
    count - 1 - j); geometry and colour fields are meaningful where `draw` is set. `full_entries`: the frame's full list
    (RasterizeMode::Depth normalises by its entries 1 and n - 1; default: `entries`)."""
    n, count = len(cloud), len(entries)
    fpc = frame_params(n, view, settings)
    src = cloud.to_f16().to_f32() if fmt == "f16" else cloud
    pv = np.ascontiguousarray(cloud.position_visibility, np.float32)
    sh = np.ascontiguousarray(src.spherical_harmonic, np.float32)
    rot = so = cov = None
    if fmt == "cov3d":
        from bevy_gaussian_splatting_amd.gaussian import covariance_3d_opacity
        cov = np.ascontiguousarray(covariance_3d_opacity(cloud), np.float32)
    else:
        rot, so = np.ascontiguousarray(src.rotation, np.float32), np.ascontiguousarray(src.scale_opacity, np.float32)
    depth_range = np.zeros(2, np.float32)
    full = entries if full_entries is None else full_entries
    if n > 0 and len(full) == n:
        i_first, i_last = int(full[min(1, n - 1)]["index"]), int(full[n - 1]["index"])
        depth_range[0] = shim().shim_distance_to_camera(ctypes.byref(fpc), _fp(pv[i_last]))
        depth_range[1] = shim().shim_distance_to_camera(ctypes.byref(fpc), _fp(pv[i_first]))
    e32 = np.ascontiguousarray(np.stack([entries["key"], entries["index"]], axis=1), np.uint32) if count else np.zeros((0, 2), np.uint32)
    outs = (ShimOut * max(count, 1))()
    cross = np.zeros((max(count, 1), 9), np.float32)
    null = ctypes.POINTER(ctypes.c_float)()
    shim().shim_project_batch(ctypes.byref(fpc), e32.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), count, _fp(pv),
                              _fp(rot) if rot is not None else null, _fp(so) if so is not None else null, _fp(sh),
                              _fp(cov) if cov is not None else null, _fp(depth_range), outs, _fp(cross))
    a = np.frombuffer(outs, dtype=np.dtype(ShimOut))[:count]
    rect = np.stack([a["tx0"], a["tx1"], a["ty0"], a["ty1"]], axis=1).astype(np.int64)
    return {"raw": outs, "count": count, "visible": a["visible"] != 0, "draw": a["draw"] != 0, "color": a["color"].copy(),
            "cx": a["cx"].copy(), "cy": a["cy"].copy(), "p": a["p"].copy(), "radius": a["radius"].copy(), "mean": a["mean"].copy(),
            "T": a["T"].copy(), "cross": cross[:count], "bounds": a["bounds"].copy(), "z": a["ndc_z"].copy(), "rect": rect, "depth_range": depth_range,
            "surfel": bool(fpc.gaussian_mode == 0 and fpc.aabb != 0)}


def twin_rect_words(twin) -> np.ndarray:
    """The packed tile rectangle x0 | x1 << 8 | y0 << 16 | y1 << 24 per RANK (project_rank), RECT_EMPTY where the twin does
    not draw."""
    r = twin["rect"][::-1]
    words = (r[:, 0] | (r[:, 1] << 8) | (r[:, 2] << 16) | (r[:, 3] << 24)).astype(np.uint32)
    return np.where(twin["draw"][::-1], words, np.uint32(RECT_EMPTY)).astype(np.uint32)


def twin_instances(twin) -> int:
    """Sum of the drawn ranks' tile-rectangle areas: what project_emit_kernel's scan totals."""
    r = twin["rect"][twin["draw"]]
    return int(((r[:, 1] - r[:, 0] + 1) * (r[:, 3] - r[:, 2] + 1)).sum())


def twin_record_words(twin):
    """(records, rects, drawn): the device's record array for the twin's draw list as uint32 [count, 12] (Record) or
    [count, 24] (RecordSurfel) — the exact bytes project_rank writes, rank j = entry count - 1 - j —, the packed rect
    word per rank, and which ranks the twin draws. A rank it does not draw is all zero here (the device leaves whatever
    its buffer held) and RECT_EMPTY in rects."""
    count = twin["count"]
    f = lambda x: np.ascontiguousarray(x[::-1], np.float32)
    col, p = f(twin["color"]), f(twin["p"])
    if twin["surfel"]:
        mean, cross = f(twin["mean"]), f(twin["cross"])
        lanes = [f(twin["cx"]), f(twin["cy"]), p[:, 0], p[:, 1], f(twin["radius"]), mean[:, 0], mean[:, 1]] + \
                [cross[:, i] for i in range(9)] + [col[:, 0], col[:, 1], col[:, 2], col[:, 3], f(twin["z"])] + \
                [np.zeros(count, np.float32)] * 3
    else:
        lanes = [f(twin["cx"]), f(twin["cy"]), p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 4], col[:, 0], col[:, 1], col[:, 2], col[:, 3],
                 f(twin["z"])]
    rec = np.ascontiguousarray(np.stack(lanes, axis=1), np.float32).view(np.uint32) if count else np.zeros((0, len(lanes)), np.uint32)
    drawn = twin["draw"][::-1].copy()
    rec = np.where(drawn[:, None], rec, np.uint32(0)).astype(np.uint32)
    return rec, twin_rect_words(twin), drawn


def record_fields(records: np.ndarray) -> dict:
    """The named lanes of a record array (uint32 [count, 12 or 24], the device's or the twin's) as float32 columns."""
    names = {12: RECORD_FIELDS, 24: SURFEL_FIELDS}[records.shape[1]]
    fl = np.ascontiguousarray(records, np.uint32).view(np.float32)
    return {name: fl[:, i] for i, name in enumerate(names)}


# ---- scenes of the reference's own tests / tools ------------------------------------------

def visibility_test_cloud() -> PlanarGaussian3d:
    """tests/visibility_render.rs:199-222."""
    red = SphericalHarmonicCoefficients()
    red.set(0, 6.0)
    gs = []
    for x in (-0.35, 0.35):
        for y in (-0.35, 0.35):
            for z in (-0.35, 0.35):
                gs.append(Gaussian3d(np.array([x, y, z, 1.0], np.float32), red.coefficients.copy(),
                                     np.array([1.0, 0.0, 0.0, 0.0], np.float32),
                                     np.array([0.22, 0.22, 0.22, 0.85], np.float32)))
    gs.append(gs[0])
    return PlanarGaussian3d.from_interleaved(gs)


def surfel_plane_cloud(grid: int = 10, spacing: float = 5.0) -> PlanarGaussian3d:
    """tools/surfel_plane.rs:64-91 (2DGS grid: scale (2,1,0.01), opacity 0.5, rotation about z)."""
    red = SphericalHarmonicCoefficients()
    red.set(0, 5.0)
    gs = []
    for i in range(grid):
        for j in range(grid):
            x = i * spacing - (grid * spacing) / 2.0
            y = j * spacing - (grid * spacing) / 2.0
            angle = np.pi / 2.0 * (i + 1) / grid
            # Quat::from_rotation_z -> (x,y,z,w) = (0,0,sin,cos); reference stores [w,x,y,z]
            rot = np.array([np.cos(angle / 2), 0.0, 0.0, np.sin(angle / 2)], np.float32)
            gs.append(Gaussian3d(np.array([x, y, 0.0, 1.0], np.float32), red.coefficients.copy(), rot,
                                 np.array([2.0, 1.0, 0.01, 0.5], np.float32)))
    return PlanarGaussian3d.from_interleaved(gs)


def aabb_obb_pair_cloud() -> PlanarGaussian3d:
    """tools/compare_aabb_obb.rs:19-58."""
    blue = SphericalHarmonicCoefficients()
    blue.set(2, 5.0)
    g = Gaussian3d(np.array([0.0, 0.0, 0.0, 1.0], np.float32), blue.coefficients.copy(),
                   np.array([0.89, 0.0, -0.432, 0.144], np.float32),
                   np.array([10.0, 1.0, 1.0, 0.5], np.float32))
    return PlanarGaussian3d.from_interleaved([g, g])


def scene_like(n: int, seed: int):
    """the reference's random distribution, plus the 'scene-like' global_scale."""
    return random_gaussians_3d_seeded(n, seed)


def tolerance_mask(ref: np.ndarray, got: np.ndarray, amb: np.ndarray | None, atol=1e-3, rtol=1e-4):
    """Per-pixel pass mask for |got - ref| <= atol + rtol*|ref| (+ the oracle's ambiguity
    bound where a coverage decision sits within rounding distance of its threshold)."""
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    lim = atol + rtol * np.abs(ref.astype(np.float64))
    if amb is not None:
        lim = lim + amb.astype(np.float64)[..., None]
    return err <= lim, err


# Tolerance accounting (round 4's verdict: "the tolerance is builder-adjustable"): every oracle comparison of a run reports
# here how many values passed only through the oracle's ambiguity bound and by HOW MUCH they exceed the strict tolerance
# 1e-3 + 1e-4 |ref|; the run's last test asserts on the totals and conftest writes them next to the other evidence.
TOLERANCE = {"values": 0, "checked": 0, "max_excess": 0.0, "max_excess_randomized": 0.0, "max_excess_overlay": 0.0,
             "max_excess_overlay_rel": 0.0, "comparisons": []}


def account(ref, got, amb, what: str = "", overlay: bool = False) -> dict:
    """Record one oracle comparison: values beyond the strict tolerance and their largest excess over it. `overlay`: a
    frame with the bounding-box overlay — an ambiguous decision there swaps a splat's fragment for the OPAQUE frame colour
    (magnitude 1), which also hides (or, the other way round, reveals) everything behind it: what one sample's flip can
    change is bounded by max(1, the frame's largest value) — the synthetic clouds' SH colours reach magnitudes of 5 to 15 —,
    so its excess is reported apart from the splat images', absolute and relative to that bound."""
    strict, err = tolerance_mask(ref, got, None)
    lim = 1e-3 + 1e-4 * np.abs(ref.astype(np.float64))
    over = ~strict
    excess = float((err - lim)[over].max()) if over.any() else 0.0
    rec = {"what": what, "values": int(strict.size), "beyond_strict": int(over.sum()), "max_excess": excess,
           "max_err": float(err.max()) if err.size else 0.0}
    TOLERANCE["values"] += rec["beyond_strict"]
    TOLERANCE["checked"] += rec["values"]
    # three classes: frames with the overlay; the randomized sweeps (they draw Msaa::Off — a flip is a WHOLE fragment —,
    # global_opacity up to 2 and every raster mode: larger single flips than the fixed configurations can have); the rest
    randomized = what.startswith("seed ") or what.startswith("medium seed ")
    key = "max_excess_overlay" if overlay else ("max_excess_randomized" if randomized else "max_excess")
    TOLERANCE[key] = max(TOLERANCE[key], excess)
    rec["overlay"] = bool(overlay)
    rec["randomized"] = bool(randomized)
    rec["ref_absmax"] = float(np.abs(ref).max()) if ref.size else 0.0
    if overlay:
        TOLERANCE["max_excess_overlay_rel"] = max(TOLERANCE["max_excess_overlay_rel"], excess / max(1.0, rec["ref_absmax"]))
    if rec["beyond_strict"] or rec["values"] >= 1_000_000:
        TOLERANCE["comparisons"].append(rec)
    return rec


def random_case(seed: int, medium: bool = False):
    """One random (cloud, view, settings) configuration for the randomized parity sweeps: camera pose,
    field of view, near plane and aspect; model transform with rotation, non-uniform scale and
    translation; every CloudSettings switch the path honours; clear colour. `medium`: 40-250 k splats
    and viewports up to 1280x720 (many tiles and supertiles, ticket loops) instead of a few thousand
    splats in a thumbnail."""
    import math
    from bevy_gaussian_splatting_amd import (DrawMode, GaussianColorSpace, RadixSortDepthBits, RasterizeMode,
                                             compute_aabb, random_gaussians_3d_seeded, transform_from)
    rng = np.random.default_rng(seed)
    n = int(rng.integers(40_000, 250_000)) if medium else int(rng.integers(1500, 5000))
    c = random_gaussians_3d_seeded(n, 100 + seed)
    # (a fourth stream, round 6: a sixth of the seeds draw a cloud with trained-asset statistics instead — surfaces, flat
    # log-normal splats, bimodal opacity, colours in [0, 1]; every other seed keeps the configuration it always had)
    rng4 = np.random.default_rng(11_000_000 + seed)
    trained = rng4.random() < 1.0 / 6.0
    if trained:
        from bevy_gaussian_splatting_amd import trained_like_gaussians_3d_seeded
        c = trained_like_gaussians_3d_seeded(n, 100 + seed, patches=24 if not medium else 96)
    c.position_visibility[:, 3] = rng.integers(0, 7, n).astype(np.float32)
    if medium:
        w, h = int(rng.integers(300, 1281)), int(rng.integers(200, 721))
    else:
        w, h = int(rng.integers(40, 200)), int(rng.integers(40, 140))
    ang = rng.uniform(-math.pi, math.pi)
    axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
    q = (*(np.sin(ang / 2) * axis), math.cos(ang / 2))
    cam = transform_from(tuple(rng.uniform(-8, 8, 3)), q)
    clear = tuple(rng.uniform(0, 1, 4)) if rng.random() < 0.5 else (0.0, 0.0, 0.0, 1.0)
    v = View.perspective(cam, w, h, fov_y=float(rng.uniform(0.4, 1.6)), near=float(rng.uniform(0.05, 0.5)),
                         clear_color=clear)
    ang2 = rng.uniform(-math.pi, math.pi)
    ax2 = rng.normal(size=3); ax2 /= np.linalg.norm(ax2)
    tr = transform_from(tuple(rng.uniform(-3, 3, 3)), (*(np.sin(ang2 / 2) * ax2), math.cos(ang2 / 2)))
    tr[:3, :3] = tr[:3, :3] @ np.diag(rng.uniform(0.5, 1.8, 3).astype(np.float32))
    mn, mx = compute_aabb(c)
    mode = [RasterizeMode.Color] * 3 + [RasterizeMode.Depth, RasterizeMode.Normal, RasterizeMode.Position,
                                        RasterizeMode.Classification, RasterizeMode.OpticalFlow]
    if rng.random() < 0.7:   # the camera moved since the previous frame (OpticalFlow)
        prev = transform_from(tuple(np.asarray(cam[:3, 3]) + rng.uniform(-0.05, 0.05, 3)), q)
        v.previous_clip_from_world = View.perspective(prev, w, h, fov_y=0.9, near=0.1).clip_from_world
        v.delta_time = float(rng.uniform(0.004, 0.05))
    s = CloudSettings(
        aabb=bool(rng.random() < 0.4),
        gaussian_mode=GaussianMode.Gaussian2d if rng.random() < 0.3 else GaussianMode.Gaussian3d,
        global_opacity=float(rng.uniform(0.3, 2.0)), global_scale=float(rng.choice([0.05, 0.3, 1.0, 1.5])),
        opacity_adaptive_radius=bool(rng.random() < 0.7),
        color_space=GaussianColorSpace.LinRec709Display if rng.random() < 0.3 else GaussianColorSpace.SrgbRec709Display,
        radix_sort_depth_bits=RadixSortDepthBits(int(rng.choice([16, 24, 32]))),
        sh_degree=int(rng.integers(0, 4)), rasterize_mode=mode[int(rng.integers(0, len(mode)))],
        num_classes=int(rng.integers(1, 6)), position_min=mn, position_max=mx, transform=tr,
        draw_mode=DrawMode(int(rng.choice([0, 0, 0, 1, 2]))))
    if trained:   # its scales are world units already; small clouds are sparse on their patches: draw them larger
        s.global_scale = float(rng4.choice([1.0, 2.0, 4.0]))
    # (a second stream, so that the configurations of the earlier rounds' sweeps keep everything above)
    rng2 = np.random.default_rng(7_000_000 + seed)
    v.msaa_samples = int(rng2.choice([1, 4, 4]))      # Msaa::Off or Bevy's default Sample4
    # (a third stream, round 5: Msaa::Sample2 / Sample8 on a quarter of the seeds, the bounding-box overlay on an eighth)
    rng3 = np.random.default_rng(9_000_000 + seed)
    r3 = rng3.random()
    if r3 < 0.125:
        v.msaa_samples = 2
    elif r3 < 0.25:
        v.msaa_samples = 8
    s.visualize_bounding_box = bool(rng3.random() < 0.125)
    v.depth_host = None
    if rng2.random() < 0.35:                           # a scene depth buffer that cuts through the cloud
        v.depth_host = random_depth_buffer(c, v, s, rng2)
    return c, v, s


def random_depth_buffer(cloud, view, settings, rng) -> np.ndarray:
    """[height, width, samples] float32 reverse-Z depth: a tilted plane between the 30 % and 70 % quantiles of the
    visible splats' depths, every sample jittered on its own (so that pixels whose samples disagree exist), and a
    corner left at 0 (no occluder: everything passes there)."""
    w, h, S = view.width, view.height, int(view.msaa_samples)
    pw = (np.asarray(settings.transform, np.float64) @ np.concatenate([cloud.position_visibility[:, :3].astype(np.float64),
                                                                       np.ones((len(cloud), 1))], 1).T).T
    clip = (np.asarray(view.clip_from_world, np.float64) @ pw.T).T
    ok = clip[:, 3] > 1e-6
    z = clip[ok, 2] / clip[ok, 3]
    z = z[(z > 0) & (z < 1)]
    lo, hi = (np.quantile(z, 0.3), np.quantile(z, 0.7)) if z.size > 10 else (0.01, 0.1)
    yy, xx = np.mgrid[0:h, 0:w]
    plane = lo + (hi - lo) * (0.5 * xx / max(w - 1, 1) + 0.5 * yy / max(h - 1, 1))
    d = plane[..., None] + (hi - lo) * 0.08 * rng.uniform(-1, 1, (h, w, S))
    d[: h // 4, : w // 4] = 0.0
    return np.ascontiguousarray(np.clip(d, 0.0, 1.0), np.float32)


def frustum_boundary_cloud(view, n_per_case, seed):
    """Points whose clip coordinates sit within a few ulp of every threshold of in_frustum (|x/w|, |y/w| = 1.1;
    z/w = 1, the near plane; z/w -> 0 far away; w ~ 0) and of the guard bands of the device's division-free verdict
    (splat_math.h in_frustum_of_world: 1.1 (1 +- 2^-20), 2^-20, 1 +- 2^-20), built by un-projecting in float64."""
    rng = np.random.default_rng(seed)
    inv = np.linalg.inv(np.asarray(view.clip_from_world, np.float64))
    near = float(np.asarray(view.clip_from_view, np.float64)[2, 3])     # infinite reverse-z: clip.z = near, clip.w = distance
    parts = []

    def unproject(ndc_x, ndc_y, dist):
        clip = np.stack([ndc_x * dist, ndc_y * dist, np.full_like(dist, near), dist], axis=1)
        w = clip @ inv.T
        return (w[:, :3] / w[:, 3:4]).astype(np.float32)
    m = n_per_case
    for centre in (1.1, 1.1 * (1 - 2.0 ** -20), 1.1 * (1 + 2.0 ** -20)):
        for axis in (0, 1):
            for sign in (-1.0, 1.0):
                edge = sign * centre * (1.0 + rng.uniform(-3e-6, 3e-6, m))
                other = rng.uniform(-1.05, 1.05, m)
                dist = np.exp(rng.uniform(np.log(0.2), np.log(200.0), m))
                parts.append(unproject(edge if axis == 0 else other, other if axis == 0 else edge, dist))
    for centre in (1.0, 1.0 - 2.0 ** -20, 1.0 + 2.0 ** -20):               # z/w = near/dist around 1: the near plane
        dist = near / (centre * (1.0 + rng.uniform(-3e-6, 3e-6, 2 * m)))
        parts.append(unproject(rng.uniform(-1.0, 1.0, 2 * m), rng.uniform(-1.0, 1.0, 2 * m), dist))
    dist = near / (2.0 ** -20 * (1.0 + rng.uniform(-3e-6, 3e-6, 2 * m)))   # z/w around 2^-20: ~100 km away
    parts.append(unproject(rng.uniform(-1.0, 1.0, 2 * m), rng.uniform(-1.0, 1.0, 2 * m), dist))
    dist = rng.uniform(-1e-7, 1e-7, 2 * m)                                  # w within 1e-7 of 0, either side
    parts.append(unproject(rng.uniform(-1.0, 1.0, 2 * m), rng.uniform(-1.0, 1.0, 2 * m), np.where(dist == 0, 1e-9, dist)))
    pos = np.concatenate(parts)
    pv = np.concatenate([pos, np.ones((len(pos), 1), np.float32)], axis=1).astype(np.float32)
    n = len(pv)
    return PlanarGaussian3d(pv, np.zeros((n, 48), np.float32), np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1)),
                            np.tile(np.array([0.01, 0.01, 0.01, 0.5], np.float32), (n, 1)))
