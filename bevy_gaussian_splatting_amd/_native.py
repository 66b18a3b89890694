"""ctypes binding of libbgs.so (the C ABI in include/bgs.h and include/bgs_diag.h).

What is specific to this library: its status codes, structs, prototype table and ABI handshake. How the library on
disk is kept the one built from this tree's sources is `_loader` + `_build_id`, shared with the bindings of the small libraries.
`__graft_entry__.build()` (or `make -C bevy_gaussian_splatting_amd/csrc`) builds it in-tree. There is no CPU fallback:
if the library is missing, or no HIP device is usable, every entry point of the package raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int
from typing import Optional

from . import _build_id, _loader
from .camera import BgsView
from .settings import BgsSettings

SPEC = _build_id.LIBBGS
LIB_PATH = SPEC.path

BGS_OK = 0
BGS_EINVAL = -1
BGS_ENOMEM = -2
BGS_EHIP = -3
BGS_ECAPACITY = -4
BGS_EINTERNAL = -5

STAGE_NAMES = ("keygen", "depth_sort", "project", "tile_sort", "ranges", "raster")

COMM_ID_BYTES = 128
# what this binding was written against (include/bgs.h BGS_VERSION_*): load() hands it to bgs_abi_check together with
# the sizes of its ctypes structs
ABI_VERSION = (0 << 16) | 9


class BgsSortEntry(ctypes.Structure):
    _fields_ = [("key", ctypes.c_uint32), ("index", ctypes.c_uint32)]


class BgsStats(ctypes.Structure):
    _fields_ = [
        ("stage_ms", ctypes.c_float * 6),
        ("total_ms", ctypes.c_float),
        ("splat_count", ctypes.c_uint32),
        ("visible_count", ctypes.c_uint32),
        ("draw_count", ctypes.c_uint32),
        ("sort_path", ctypes.c_uint32),
        ("instance_count", ctypes.c_uint64),
        ("instance_capacity", ctypes.c_uint64),
        ("tiles_x", ctypes.c_uint32),
        ("tiles_y", ctypes.c_uint32),
        ("depth_passes", ctypes.c_uint32),
        ("tile_passes", ctypes.c_uint32),
        ("algorithmic_bytes", ctypes.c_uint64),
        ("regrow_count", ctypes.c_uint32),
        ("binning_mode", ctypes.c_uint32),
        ("frames_averaged", ctypes.c_uint32),
        ("list_capacity", ctypes.c_uint32),
        ("list_entries_allocated", ctypes.c_uint64),
        ("strip_tiles", ctypes.c_uint32),
        ("tile_saturation", ctypes.c_uint32),
    ]


class BgsFrameRecordsInfo(ctypes.Structure):
    """bgs_frame_records_info (include/bgs_diag.h)."""

    _fields_ = [("draw_count", ctypes.c_uint32), ("record_stride", ctypes.c_uint32), ("has_rects", ctypes.c_uint32),
                ("visible_count", ctypes.c_uint32), ("color_max_bits", ctypes.c_uint32)]


class BgsFrameListsInfo(ctypes.Structure):
    """bgs_frame_lists_info (include/bgs_diag.h)."""

    _fields_ = [("entry_count", ctypes.c_uint64), ("binning", ctypes.c_uint32), ("draw_count", ctypes.c_uint32),
                ("sup_edge", ctypes.c_uint32), ("sup_x", ctypes.c_uint32), ("sup_y", ctypes.c_uint32), ("level", ctypes.c_uint32),
                ("coarse_cap", ctypes.c_uint32), ("wide_bin", ctypes.c_uint32), ("instance_count", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class BgsScratchLayout(ctypes.Structure):
    """bgs_scratch_layout (include/bgs_diag.h): the lane's scratch region, [Control 0 | the REGIONS | Control 1]."""

    REGIONS = ("off_depth_status", "off_scan_status", "off_tile_status", "off_ranges", "off_bin_status", "off_part_status",
               "off_ctl1")   # in address order, behind the first Control block at 0
    _fields_ = [("bytes", ctypes.c_uint64)] + [(name, ctypes.c_uint64) for name in REGIONS] + \
               [("depth_tiles", ctypes.c_uint64), ("inst_tiles", ctypes.c_uint64), ("inst_cap", ctypes.c_uint64),
                ("n", ctypes.c_uint32), ("pass_stride", ctypes.c_uint32)]


class BgsFrameLeftoversInfo(ctypes.Structure):
    """bgs_frame_leftovers_info (include/bgs_diag.h)."""

    _fields_ = [("dirty_words", ctypes.c_uint64)] + \
               [(name, ctypes.c_uint32) for name in ("ctl_block", "scratch_clean", "scratch_reset", "raster_cleans", "bucket", "places",
                                                     "large", "wide", "wide_bin", "kept", "bucket_sub", "split_sub_out", "keygen_tile",
                                                     "n", "ntiles", "raster_mode", "strips_appended", "graph_replay", "binning",
                                                     "control_bytes", "culled_tail", "reserved")]


class BgsRasterSelftest(ctypes.Structure):
    """bgs_raster_selftest (include/bgs_diag.h)."""

    _fields_ = [(name, ctypes.c_uint32) for name in ("width", "height", "sample_count", "variant", "overlay", "mode", "sup_edge",
                                                     "coarse_cap", "color_max_bits", "record_count", "heavy_count", "reserved")] + \
               [("viewport_w", ctypes.c_float), ("viewport_h", ctypes.c_float), ("clear", ctypes.c_float * 4)] + \
               [(name, ctypes.c_void_p) for name in ("records", "lists", "totals", "depth", "heavy_tiles", "order")]


SELFTEST_BIN_GUARD = 64   # BGS_SELFTEST_BIN_GUARD (include/bgs_diag.h)
SELFTEST_RASTER_GUARD = 64   # BGS_SELFTEST_RASTER_GUARD (include/bgs_diag.h)
# the HeavyFeedback buffer bgs_selftest_raster returns (csrc/kernels.h): [count | list u16[HEAVY_CAP] | flag u8[tiles]]
HEAVY_CAP, HEAVY_LIST_OFFSET = 256, 128
HEAVY_FLAGS_OFFSET = HEAVY_LIST_OFFSET + 2 * HEAVY_CAP
SELFTEST_BUCKET_GUARD = 64   # BGS_SELFTEST_BUCKET_GUARD (include/bgs_diag.h)
GRID_CAP_MAX = 4096   # BGS_GRID_CAP_MAX
FRAME_GRIDS_WORDS = 16   # BGS_FRAME_GRIDS_WORDS
GRID_KERNELS = ("front", "depth", "project", "bin", "tile_sort")   # enum bgs_grid_kernel, in order


vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
fp, up, u64p, vpp = POINTER(c_float), POINTER(u32), POINTER(u64), POINTER(vp)
view_p, settings_p, entry_p = POINTER(BgsView), POINTER(BgsSettings), POINTER(BgsSortEntry)

# Every function the two headers declare, in their order: (name, restype, argtypes), to be held against the header line
# by line. tests/test_native_binding.py does so for the names, the parameter counts and the return types; the parameter
# TYPES are checked by nothing but the reader. Opaque handles and device pointers are void*.
PROTOTYPES = (
    # ---- include/bgs.h ----
    ("bgs_create", c_int, (c_int, vpp)),
    ("bgs_destroy", None, (vp,)),
    ("bgs_last_error", c_char_p, (vp,)),
    ("bgs_version", u32, ()),
    ("bgs_abi_check", c_int, (u32, u32, u32, u32)),
    ("bgs_build_id", c_char_p, ()),
    ("bgs_settings_default", None, (settings_p,)),
    ("bgs_view_perspective", None, (fp, c_float, c_float, u32, u32, view_p)),
    ("bgs_cloud_upload_f32", c_int, (vp, u32, fp, fp, fp, fp, vpp)),
    ("bgs_cloud_upload_f16", c_int, (vp, u32, fp, up, up, vpp)),
    ("bgs_cloud_upload_cov3d_f32", c_int, (vp, u32, fp, fp, fp, vpp)),
    ("bgs_cloud_free", None, (vp, vp)),
    ("bgs_cloud_len", u32, (vp,)),
    ("bgs_cloud_apply_particle_behaviors", c_int, (vp, vp, vp, u32, c_float)),
    ("bgs_sort", c_int, (vp, vp, view_p, settings_p, entry_p)),
    ("bgs_render", c_int, (vp, vp, view_p, settings_p, fp)),
    ("bgs_framebuffer_device_ptr", c_int, (vp, vpp, u64p)),
    ("bgs_set_output_srgb8", c_int, (vp, c_int)),
    ("bgs_framebuffer_srgb8_device_ptr", c_int, (vp, vpp, u64p)),
    ("bgs_set_output_rgba16f", c_int, (vp, c_int)),
    ("bgs_framebuffer_rgba16f_device_ptr", c_int, (vp, vpp, u64p)),
    ("bgs_set_packed_only", c_int, (vp, c_int)),
    ("bgs_set_srgb8_target", c_int, (vp, vp)),
    ("bgs_download", c_int, (vp, vp, vp, u64)),
    ("bgs_device_alloc", c_int, (vp, u64, vpp)),
    ("bgs_device_free", c_int, (vp, vp)),
    ("bgs_upload", c_int, (vp, vp, vp, u64)),
    ("bgs_set_pipeline_depth", c_int, (vp, u32)),
    ("bgs_pipeline_pop", c_int, (vp, vpp, vpp)),
    ("bgs_frames_in_flight", c_int, (vp, up)),
    ("bgs_sorted_entries_device_ptr", c_int, (vp, vpp, up)),
    ("bgs_synchronize", c_int, (vp,)),
    ("bgs_set_async", c_int, (vp, c_int)),
    ("bgs_stream", c_int, (vp, vpp)),
    ("bgs_set_binning", c_int, (vp, u32)),
    ("bgs_reset_adaptive_state", c_int, (vp,)),
    ("bgs_set_profiling", c_int, (vp, c_int)),
    ("bgs_set_profiling_stride", c_int, (vp, u32)),
    ("bgs_get_stats", c_int, (vp, POINTER(BgsStats))),
    ("bgs_set_pipeline_streams", c_int, (vp, u32)),
    ("bgs_set_graphs", c_int, (vp, c_int)),
    ("bgs_comm_unique_id", c_int, (c_char_p,)),
    ("bgs_comm_create", c_int, (vp, c_char_p, u32, u32, vpp)),
    ("bgs_comm_gather", c_int, (vp, vp, u32, vp, u64, vp, u64p)),
    ("bgs_comm_gather_after", c_int, (vp, vp, u32, vp, u64, vp, vp, u64p)),
    ("bgs_comm_wait", c_int, (vp, vp, u64)),
    ("bgs_comm_stream", c_int, (vp, vp, vpp)),
    ("bgs_comm_destroy", None, (vp, vp)),
    # ---- include/bgs_diag.h ----
    ("bgs_set_debug_flags", c_int, (vp, u32)),
    ("bgs_adaptive_counters", c_int, (vp, u64p)),
    ("bgs_learning_counters", c_int, (vp, u64p, u64p)),
    ("bgs_radix_sort_pairs", c_int, (vp, entry_p, u32, u32)),
    ("bgs_hbm_probe", c_int, (vp, u64, u32, fp, fp)),
    ("bgs_selftest_ln_f32", c_int, (vp, u32, u32, fp, u64p)),
    ("bgs_set_queue_holders", c_int, (c_int,)),
    ("bgs_set_tile_trace", c_int, (vp, vp)),
    ("bgs_graph_counters", c_int, (vp, u64p, u64p)),
    ("bgs_tile_order_counters", c_int, (vp, u64p, u64p, u64p)),
    ("bgs_selftest_tile_order", c_int, (vp, vp, u32, u32, vp, vp)),
    ("bgs_selftest_pack", c_int, (vp, u32, vp, u32, vp)),
    ("bgs_debug_frame_records", c_int, (vp, vp, u64, up, u32, POINTER(BgsFrameRecordsInfo))),
    ("bgs_selftest_bin", c_int, (vp, up, u32, u32, u32, u32, u32, u32, u32, up, u64, up, up)),
    ("bgs_debug_frame_lists", c_int, (vp, up, u32, up, u64, up, u32, POINTER(BgsFrameListsInfo))),
    ("bgs_selftest_bucket_sort", c_int, (vp, u32, u32, u32, up, up, u32, up, u64, up)),
    ("bgs_selftest_keygen_buckets", c_int, (vp, vp, view_p, settings_p, up, u32, u32, u32, u32, up, up, u64, up, u64, up)),
    ("bgs_selftest_raster", c_int, (vp, POINTER(BgsRasterSelftest), fp, fp, u64, vp, vp, u64, up)),
    ("bgs_debug_frame_leftovers", c_int, (vp, vp, u64, vp, u32, POINTER(BgsScratchLayout), POINTER(BgsFrameLeftoversInfo))),
    ("bgs_set_grid_cap", c_int, (vp, u32)),
    ("bgs_debug_frame_grids", c_int, (vp, up, u32)),
)
EXPORTED_SYMBOLS = tuple(name for name, _, _ in PROTOTYPES)


class BgsError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libbgs error {status}: {message}")
        self.status = status


_lib: Optional[ctypes.CDLL] = None


def ensure_current() -> str:
    """`_loader.ensure_current` for the library at LIB_PATH (as it is when this is called). Returns the id."""
    return _loader.ensure_current(SPEC, LIB_PATH)


def build_id() -> str:
    """`bgs_build_id()` of the loaded library (= the tree's kernel-source hash, load() checked it)."""
    return load().bgs_build_id().decode()


def load() -> ctypes.CDLL:
    """Load libbgs.so once and declare prototypes. Raises if it is not built from this tree's sources and cannot
    be rebuilt."""
    global _lib
    if _lib is not None:
        return _lib
    override = os.environ.get("BGS_LIB_OVERRIDE")
    if override:
        # EXPERIMENTS ONLY (scripts/ab_variants.sh: same-box A/B of library variants built from modified sources): the
        # named library is loaded as it is, whatever it was built from. Said loudly; bench.py and the tests refuse it.
        import sys
        print(f"bevy_gaussian_splatting_amd: BGS_LIB_OVERRIDE={override} — NOT the library of this tree "
              f"(build id {_build_id.library_build_id(override)})", file=sys.stderr)
        lib = ctypes.CDLL(override, mode=SPEC.dlopen_mode)
        _loader.declare(lib, PROTOTYPES)
    else:
        want = ensure_current()
        lib = ctypes.CDLL(LIB_PATH, mode=SPEC.dlopen_mode)
        _loader.declare(lib, PROTOTYPES)
        if lib.bgs_build_id().decode() != want:
            raise ImportError(f"{LIB_PATH}: bgs_build_id() disagrees with the id in the file's bytes")
    # the handshake a binding owes the library (a stale struct layout is refused here, not read past)
    rc = lib.bgs_abi_check(ABI_VERSION, ctypes.sizeof(BgsView), ctypes.sizeof(BgsSettings), ctypes.sizeof(BgsStats))
    if rc != BGS_OK:
        raise ImportError("libbgs.so refuses this binding: " + (lib.bgs_last_error(None) or b"").decode("utf-8", "replace"))
    _lib = lib
    return lib


def check(lib: ctypes.CDLL, ctx, status: int) -> None:
    if status != BGS_OK:
        msg = lib.bgs_last_error(ctx)
        raise BgsError(status, msg.decode("utf-8", "replace") if msg else "")
