"""What a frame leaves for the frame behind it: the references and the cases of tests/test_frame_leftovers_host.py and
tests/test_frame_leftovers_gpu.py. Integer work throughout: every check made with these is an equality or an order.

The references are written from the kernels' tile geometry, NOT from the clean-up's formulas (csrc/render_kernels.hip,
raster_scan_kernel, `if (cl.other_ctl && !strip_block)`):

  keygen (csrc/sort_kernels.hip) publishes one chain word per tile of 2048 / 4096 / 8192 splats (keygen_tile_splats), the
  kept-order compaction (csrc/entries_kernels.hip) one per 2048 entries; a bucket frame that writes no culled tail runs
  the chainless keygen and publishes none;
  an onesweep depth pass publishes 256 words per tile of 2048 pairs, 4096 when FramePlan::large — plan_frame sets it for
  clouds of MORE THAN 4 << 20 = 4 194 304 splats, whatever the draw count —, of the D drawable pairs;
  bin_kernel publishes 256 words per tile of 1024 ranks of D, in both its shapes (<16>: pipeline depth 1, <4>: any other).

`info` is the dict of GaussianSplattingPlugin.debug_frame_leftovers (bgs_frame_leftovers_info by field name)."""
from dataclasses import dataclass, field

import numpy as np

from bevy_gaussian_splatting_amd import CloudSettings, PlanarGaussian3d, View, random_gaussians_3d_seeded
from bevy_gaussian_splatting_amd.settings import GaussianMode, RadixSortDepthBits, SortMode

# debug flags (include/bgs_diag.h)
BUCKETS_NARROW, SPLIT_SUB_3, SPLIT_SUB_5, BUCKETS_WIDE = 0x100, 0x200, 0x400, 0x800
NO_RASTER_CLEANUP, LEVEL_2, MIDROUND_ALWAYS, NO_BUCKET_SORT = 0x1000, 0x400000, 0x20000, 0x80000
SMALL_LISTS, GUESSED_SPLITTERS, STRIPS_ANY_DEPTH, RERUN_EVERY_FRAME, NO_TILE_COST = 0x100000, 0x200000, 0x4000000, 0x8000000, 0x10000000

KEYGEN_TILES = (2048, 4096, 8192)
SORT_TILE = {0: 2048, 1: 4096}   # by FramePlan::large
BIN_TILE = 1024
RADIX = 256
LARGE_ABOVE = 4 << 20            # plan_frame: p.large = n > (4u << 20)
CHAIN_REGIONS = ("part", "depth", "bin")


def ceil_div(a: int, b: int) -> int:
    return -(-int(a) // int(b))


def words_used(info: dict, draw_count: int) -> dict:
    """Chain words a frame of this plan may publish: {"part": words, "depth": words per pass, "passes": passes, "bin": words}."""
    n, d = int(info["n"]), int(draw_count)
    assert info["keygen_tile"] in KEYGEN_TILES
    chainless = info["bucket"] and not info["culled_tail"]
    part = 0 if (n == 0 or chainless) else ceil_div(n, 2048 if info["kept"] else info["keygen_tile"])
    passes = 0 if (info["bucket"] or info["kept"] or n == 0) else int(info["places"])
    depth = ceil_div(d, SORT_TILE[int(info["large"])]) * RADIX if passes else 0
    return {"part": part, "depth": depth, "passes": passes, "bin": ceil_div(d, BIN_TILE) * RADIX if info["binning"] == 0 else 0}


def words_zeroed(info: dict, draw_count: int) -> dict:
    """What the clean-up's three formulas cover, as the kernel states them (FrameCleanup: places = 0 for a bucket frame,
    depth_tile = sort_tile_size(large), KEYGEN_TILE = 2048; draw_count read as 0 under sort_overflow by the caller)."""
    n, d = int(info["n"]), int(draw_count)
    passes = 0 if info["bucket"] else int(info["places"])
    return {"part": ceil_div(n, 2048), "depth": ceil_div(d, SORT_TILE[int(info["large"])]) * 64 * 4, "passes": passes,
            "bin": ceil_div(d, BIN_TILE) * 64 * 4}


def region_words(layout, region: str, pass_index: int = 0):
    """[first word, words) of a chain region inside the lane's scratch region (ScratchLayout: helpers.ScratchLayoutC or
    _native.BgsScratchLayout). The depth passes' arrays lie pass_stride words apart and end where the scan status starts."""
    if region == "part":
        return int(layout.off_part_status) // 4, (int(layout.off_ctl1) - int(layout.off_part_status)) // 4
    if region == "bin":
        return int(layout.off_bin_status) // 4, (int(layout.off_part_status) - int(layout.off_bin_status)) // 4
    assert region == "depth" and 0 <= pass_index < 4
    return int(layout.off_depth_status) // 4 + pass_index * int(layout.pass_stride), int(layout.pass_stride)


def quantile_keys(sorted_entries, draw_count: int, nbk: int, key_xor: int) -> np.ndarray:
    """The nbk - 1 quantile keys of a sorted list of D entries in keygen's key space, then the terminator: what a frame
    leaves in Control::splitters[0 .. nbk). An empty list leaves terminators only."""
    keys = np.asarray(sorted_entries["key"] if getattr(sorted_entries, "dtype", None) is not None and sorted_entries.dtype.names
                      else sorted_entries, dtype=np.uint32)
    d = int(draw_count)
    out = np.full(nbk, 0xFFFFFFFF, np.uint32)
    if d > 0:
        t = np.arange(nbk - 1, dtype=np.int64)
        out[:nbk - 1] = keys[((t + 1) * d) // nbk] ^ np.uint32(key_xor & 0xFFFFFFFF)
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    n: int                     # splats in the cloud
    drawable: int = -1         # the first `drawable` splats stay where the generator put them, the rest go behind the camera (-1: all stay)
    size: tuple = (64, 64)
    flags: int = 0
    warm: int = 0              # identical frames before the one read back (a bucket frame needs a completed frame's table)
    depth: int = 1             # pipeline depth
    bits: int = 32
    sort_mode: int = int(SortMode.Radix)
    shape: str = "obb"         # obb / aabb3d / surfel
    kept: bool = False         # drawn from a chunk of device entries sorted for another yaw, with skipped entries
    graphs: bool = False       # async frames at depth 1 with graphs on: the frame read back is a counted replay
    scale: float = 1.0
    opacity: float = 1.0       # CloudSettings.global_opacity
    ordered: bool = False      # the frame draws its raster workgroups in a completed frame's cost order (a target of more tile
                               # waves than the chip holds): the only frames that report a saturation share
    expect: dict = field(default_factory=dict)   # plan fields the frame must report, else the case tests another path
    regions: tuple = ("part", "depth", "bin")    # the chain regions its twin must find words in
    reruns: str = ""           # adaptive counter that must have risen
    budget: str = ""           # the cloud is this case's of tests/instance_budget_cases.py (n: its splats) instead of the seeded rows
    sort_frames: int = 0       # BINNING_SORT frames of the same cloud and view drawn first, on the same lane: the frame read back
                               # starts on what they left (a scratch region rebuilt for grown instance buffers, not cleaned)

    def settings(self) -> CloudSettings:
        extra = {"obb": {}, "aabb3d": {"aabb": True}, "surfel": {"aabb": True, "gaussian_mode": GaussianMode.Gaussian2d}}[self.shape]
        return CloudSettings(sort_mode=SortMode(self.sort_mode), radix_sort_depth_bits=RadixSortDepthBits(self.bits),
                             global_scale=self.scale, global_opacity=self.opacity, **extra)

    def view(self, yaw: float = 0.0) -> View:
        return View.headless(self.size[0], self.size[1], yaw=yaw, msaa_samples=4)


_BASE = {}


def cloud_of(case: Case) -> PlanarGaussian3d:
    """n splats: the rows of one 8192-splat seeded cloud repeated; all but the first `drawable` behind the camera."""
    if case.budget:
        import instance_budget_cases as I
        assert len(I.built(case.budget)["cloud"]) == case.n and I.by_name(case.budget).size == case.size
        return I.built(case.budget)["cloud"]
    if "base" not in _BASE:
        _BASE["base"] = random_gaussians_3d_seeded(8192, 77)
    b, n = _BASE["base"], case.n
    rows = np.arange(n) % 8192
    pv = b.position_visibility[rows].copy()
    if case.drawable >= 0:
        pv[case.drawable:, 2] = np.abs(pv[case.drawable:, 2]) + 10.0
    return PlanarGaussian3d(pv, b.spherical_harmonic[rows], b.rotation[rows], b.scale_opacity[rows])


ONESWEEP = {"bucket": 0, "kept": 0}
CASES = (
    # n around the keygen tile
    Case("n_0", 0, regions=()),
    Case("n_1", 1, flags=NO_BUCKET_SORT, expect=ONESWEEP, regions=("part",)),   # (the one splat is not drawn: D = 0)
    Case("n_2047", 2047, flags=NO_BUCKET_SORT, expect=ONESWEEP),
    Case("n_2048", 2048, flags=NO_BUCKET_SORT, expect=ONESWEEP),
    Case("n_2049", 2049, flags=NO_BUCKET_SORT, expect=ONESWEEP),
    Case("n_4097", 4097, flags=NO_BUCKET_SORT, expect=ONESWEEP),
    # 4096-splat keygen tiles from 2^19 splats
    Case("keygen_4096_tiles", (1 << 19) + 1, drawable=9000, flags=NO_BUCKET_SORT, expect=dict(ONESWEEP, keygen_tile=4096, large=0)),
    # onesweep at 2 / 3 / 4 passes, 2048-pair tiles ...
    Case("onesweep_16", 30000, flags=NO_BUCKET_SORT, bits=16, expect=dict(ONESWEEP, places=2, large=0)),
    Case("onesweep_24", 30000, flags=NO_BUCKET_SORT, bits=24, expect=dict(ONESWEEP, places=3, large=0)),
    Case("onesweep_32", 30000, flags=NO_BUCKET_SORT, bits=32, expect=dict(ONESWEEP, places=4, large=0)),
    # ... and 4096-pair tiles: FramePlan::large, n > 4 << 20 splats (plan_frame), most of them behind the camera
    Case("onesweep_16_large", LARGE_ABOVE + 1, drawable=70000, flags=NO_BUCKET_SORT, bits=16, expect=dict(ONESWEEP, places=2, large=1, keygen_tile=4096)),
    Case("onesweep_24_large", LARGE_ABOVE + 1, drawable=70000, flags=NO_BUCKET_SORT, bits=24, expect=dict(ONESWEEP, places=3, large=1)),
    Case("onesweep_32_large", LARGE_ABOVE + 1, drawable=70000, flags=NO_BUCKET_SORT, bits=32, expect=dict(ONESWEEP, places=4, large=1)),
    # bucket sort: narrow / wide, sub 1 / 3 (table in keygen's arguments) / 5 (device table); chainless keygen, no passes
    Case("bucket_narrow_sub1", 30000, warm=2, expect={"bucket": 1, "wide": 0, "bucket_sub": 1}, regions=("bin",)),
    Case("bucket_narrow_sub3", 30000, warm=2, flags=SPLIT_SUB_3, expect={"bucket": 1, "wide": 0, "bucket_sub": 3, "split_sub_out": 3}, regions=("bin",)),
    Case("bucket_wide_sub1", 30000, warm=2, flags=BUCKETS_WIDE, expect={"bucket": 1, "wide": 1, "bucket_sub": 1}, regions=("bin",)),
    Case("bucket_wide_sub5", 30000, warm=2, flags=BUCKETS_WIDE | SPLIT_SUB_5, expect={"bucket": 1, "wide": 1, "bucket_sub": 5, "split_sub_out": 5}, regions=("bin",)),
    # a bucket frame that cannot fit (256 equal steps over 32 bits: one bucket takes the list) and its onesweep re-run
    Case("bucket_overflow_rerun", 200000, flags=GUESSED_SPLITTERS, expect=ONESWEEP, reruns="reruns_sort"),
    Case("small_lists_rerun", 12000, size=(250, 130), flags=SMALL_LISTS | NO_BUCKET_SORT, expect=ONESWEEP, reruns="reruns_lists"),
    Case("rerun_every_frame", 12000, flags=RERUN_EVERY_FRAME | NO_BUCKET_SORT, expect=ONESWEEP),
    # behind a BINNING_SORT frame of 2^22 + 1 tile instances (instance_budget_cases' one_over) that overflowed, grew the lane's
    # instance buffers and its scratch region, and was re-run: the scan frame on that lane finds nothing clean and leaves it clean
    Case("instances_overflow_rerun", 16385, size=(256, 256), flags=NO_BUCKET_SORT, budget="one_over", sort_frames=2, expect=ONESWEEP,
         reruns="reruns_instances"),
    # kept order: the compaction's chain, no passes
    Case("kept_order", 9000, kept=True, expect={"kept": 1, "bucket": 0, "places": 0}, regions=("part", "bin")),
    # everything behind the camera: D = 0
    Case("voided", 5000, drawable=0, flags=NO_BUCKET_SORT, expect=ONESWEEP, regions=("part",)),
    # one raster workgroup (a 16 x 16 target is one tile) zeroes everything, under 100 000 drawable splats
    Case("one_workgroup", 100000, size=(16, 16), flags=NO_BUCKET_SORT, sort_mode=int(SortMode.Rayon), expect=ONESWEEP),
    # 5 x 3 tiles: 4 workgroups, no multiple of 8
    Case("grid_not_of_8", 30000, size=(80, 48), flags=NO_BUCKET_SORT, expect=ONESWEEP),
    # dense frame with the strip workgroups behind its grid: 4 regular workgroups + 256 strip workgroups. The clean-up's stride is
    # the regular grid's, 4 x 256 = 1024 threads, and its depth and bin loops count uint4: every splat is drawn (Rayon, D = 70 000),
    # so the loops run to 35 x 64 = 2240 and 69 x 64 = 4416 and use the stride. Nearly transparent splats: no tile saturates
    # inside its first staging round, so the frames before this one list every tile as heavy and strip workgroups draw them.
    Case("strips_appended", 70000, flags=NO_BUCKET_SORT | LEVEL_2 | MIDROUND_ALWAYS | STRIPS_ANY_DEPTH, warm=2, opacity=0.05,
         sort_mode=int(SortMode.Rayon), expect=dict(ONESWEEP, raster_mode=1, strips_appended=1)),
    # a 1080p target: 8160 tile waves, more than the chip holds at once, so the third frame is drawn in the order made of the
    # first one's costs and reports that plane's saturation share
    Case("ordered_1080p", 30000, size=(1920, 1080), flags=NO_BUCKET_SORT, warm=2, ordered=True, expect=ONESWEEP),
    # the table of sub 2 that a draw-count hint past 524 288 pairs asks for by itself (plan_frame: split_sub_out), no flag
    Case("split_sub_2_rayon", 600000, flags=NO_BUCKET_SORT, warm=1, sort_mode=int(SortMode.Rayon), expect=dict(ONESWEEP, split_sub_out=2)),
    Case("split_sub_2_std", 600000, flags=NO_BUCKET_SORT, warm=1, sort_mode=int(SortMode.Std), expect=dict(ONESWEEP, split_sub_out=2)),
    # both shapes of bin_kernel
    Case("depth_1_bin16", 30000, flags=NO_BUCKET_SORT, depth=1, expect=dict(ONESWEEP, wide_bin=1)),
    Case("depth_2_bin4", 30000, flags=NO_BUCKET_SORT, depth=2, expect=dict(ONESWEEP, wide_bin=0)),
    # a counted graph replay
    Case("graph_replay", 30000, flags=NO_BUCKET_SORT, graphs=True, warm=4, expect=dict(ONESWEEP, graph_replay=1)),
    # the other instantiations of the rasteriser
    Case("surfel", 20000, flags=NO_BUCKET_SORT, shape="surfel", expect=ONESWEEP),
    Case("aabb3d", 20000, flags=NO_BUCKET_SORT, shape="aabb3d", expect=ONESWEEP),
)
CASE_NAMES = tuple(c.name for c in CASES)
assert len(set(CASE_NAMES)) == len(CASES)


def by_name(name: str) -> Case:
    return CASES[CASE_NAMES.index(name)]


def planned_info(case: Case) -> dict:
    """The plan a case is written to get, for the host checks (the GPU tests read the real one from the hook): `expect`
    over the defaults of a synchronous onesweep frame of the case's cloud."""
    n = case.n
    info = {"n": n, "bucket": 0, "kept": 1 if case.kept else 0, "places": 0 if case.kept else case.bits // 8, "large": 1 if n > LARGE_ABOVE else 0,
            "keygen_tile": 8192 if n >= 1 << 31 else (4096 if n >= 1 << 19 else 2048), "binning": 0, "culled_tail": 0}
    info.update({k: v for k, v in case.expect.items() if k in info})
    return info


def draw_counts(case: Case) -> tuple:
    """Draw counts a frame of the case's cloud may reach, for the host checks: none, one, around every tile edge, all."""
    top = case.n if case.drawable < 0 else min(case.drawable, case.n)
    edges = [e + k for e in (1024, 2048, 4096, 8192) for k in (-1, 0, 1)]
    return tuple(sorted({d for d in [0, 1, top // 2, top] + edges if 0 <= d <= top}))
