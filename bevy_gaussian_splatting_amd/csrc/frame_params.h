// frame_params.h — bgs_view + bgs_settings -> FrameParams (host, plain C++).
// Shared by bgs_frame.hip and the CPU pre-flight shim (tests/host_shim) so both feed the
// per-splat arithmetic exactly the same constants.
#pragma once
#include <string.h>

#include "../../include/bgs.h"
#include "../../include/bgs_diag.h"
#include "bgs_device.h"

namespace bgs {

inline uint32_t depth_places(const bgs_settings* s) {
    if (s->sort_mode == BGS_SORT_NONE) return 0;
    if (s->sort_mode == BGS_SORT_RADIX) return s->radix_depth_bits / 8u;  // src/render/mod.rs:718
    return 4;  // SORT_RAYON / SORT_STD: full 32-bit f32 keys
}

inline void fill_frame_params(uint32_t n, const bgs_view* view, const bgs_settings* s, FrameParams& fp) {
    memcpy(fp.transform, s->transform, sizeof fp.transform);
    memcpy(fp.view_from_world, view->view_from_world, sizeof fp.view_from_world);
    memcpy(fp.clip_from_world, view->clip_from_world, sizeof fp.clip_from_world);
    fp.cam[0] = view->world_from_view[12];  // view.world_position
    fp.cam[1] = view->world_from_view[13];
    fp.cam[2] = view->world_from_view[14];
    fp.viewport_w = view->viewport[2];
    fp.viewport_h = view->viewport[3];
    fp.focal_x = view->clip_from_view[0] * view->viewport[2];  // src/render/helpers.wgsl:20-23
    fp.focal_y = view->clip_from_view[5] * view->viewport[3];
    fp.global_opacity = s->global_opacity;
    fp.global_scale = s->global_scale;
    fp.n = n;
    fp.key_shift = s->sort_mode == BGS_SORT_RADIX ? 32u - s->radix_depth_bits : 0u;  // mod.rs:719
    fp.gaussian_mode = s->gaussian_mode;
    fp.aabb = s->aabb ? 1u : 0u;
    fp.adaptive_radius = s->opacity_adaptive_radius ? 1u : 0u;
    fp.color_space = s->color_space;
    fp.sh_degree = s->sh_degree;
    fp.sort_mode = s->sort_mode;
    fp.width = (int32_t)view->viewport[2];
    fp.height = (int32_t)view->viewport[3];
    fp.tiles_x = (fp.width + TILE_PX - 1) / TILE_PX;
    fp.tiles_y = (fp.height + TILE_PX - 1) / TILE_PX;
    fp.debug = 0;
    fp.rasterize_mode = s->rasterize_mode;
    fp.num_classes = s->num_classes;
    fp.draw_mode = s->draw_mode;
    memcpy(fp.prev_clip_from_world, view->previous_clip_from_world, sizeof fp.prev_clip_from_world);
    fp.delta_time = view->delta_time;
    memcpy(fp.clear, view->clear_color, sizeof fp.clear);
    fp.srgb8_target = 0;
    fp.sort_path = 0;  // chosen per frame by the host (bgs_frame.hip)
    fp.sample_count = view->sample_count ? view->sample_count : 4u;   // 0 = not set = Msaa::default() = Sample4
    // (bit 0: the colour attachment lies behind the depth plane, bgs_device.h ATTACH_COLOR_TAG; check_inputs has seen to it
    // that the address of such a pair is set and 16-byte aligned)
    fp.depth_ptr = view->depth_device_ptr |
                   (view->depth_device_ptr != 0ull && view->reserved[0] == BGS_VIEW_ATTACH_COLOR ? ATTACH_COLOR_TAG : 0ull);
    // uniform parts of world_to_local_direction (gaussian.wgsl:166-176: normalize(basis[k]) = v / length(v),
    // length = sqrt(dot)) and of the bounding boxes (1.0 / viewport): IEEE binary32, the order of splat_math.h
    for (int k = 0; k < 3; ++k) {
        const float x = s->transform[4 * k], y = s->transform[4 * k + 1], z = s->transform[4 * k + 2];
        const float len = __builtin_sqrtf((x * x + y * y) + z * z);
        fp.basis[3 * k] = x / len;
        fp.basis[3 * k + 1] = y / len;
        fp.basis[3 * k + 2] = z / len;
    }
    fp.inv_viewport_w = 1.0f / view->viewport[2];
    fp.inv_viewport_h = 1.0f / view->viewport[3];
    fp.visualize_bbox = s->visualize_bounding_box ? 1u : 0u;
    for (int i = 0; i < 3; ++i) {
        fp.pos_min[i] = s->position_min[i];
        fp.pos_max[i] = s->position_max[i];
    }
}

// a frame's tile grid in one word (what tile feedback left by one frame is matched against the next frame by)
inline uint32_t tile_grid_word(const FrameParams& fp) { return (uint32_t)fp.tiles_x | ((uint32_t)fp.tiles_y << 16); }

// ---- adaptive policies of the host side (plain functions so that the CPU suite can test them) -----------

inline uint32_t pow2_ceil_u32(uint64_t v) {
    uint64_t p = 1;
    while (p < v) p <<= 1;
    return (uint32_t)(p < (1ull << 31) ? p : (1ull << 31));
}

// Supertile level of the next frames from a completed frame's statistics (bgs_frame.hip, finish_lane).
// `ratio` = list entries per visible splat of a frame that ran at level `lv`; `edges` = supertile edge in
// tiles of levels 0..3. Inside [1.6, 4] the level stays. Outside it moves straight to the level the frame's
// own geometry asks for: a splat of s supertile edges overlaps (s + 1)^2 supertiles on average, so
// sqrt(ratio) - 1 is the typical splat extent in edges of THIS frame's level, and the finest level whose
// edge is at least that extent keeps the ratio under 4 — but always at least one level in the direction the
// band was left. *longer_out (if the level gets coarser): by how much the longest list is expected to grow
// (entries scale with the ratio, lists with the supertile area).
inline uint32_t next_supertile_level(double ratio, uint32_t lv, const uint32_t edges[4], double* longer_out) {
    if (longer_out) *longer_out = 1.0;
    if (!(ratio > 4.0 && lv < 3) && !(ratio < 1.6 && lv > 0)) return lv;
    const double root = ratio > 0.0 ? __builtin_sqrt(ratio) : 0.0;
    const double extent_tiles = (root > 1.0 ? root - 1.0 : 0.0) * (double)edges[lv];
    uint32_t target = 3;
    for (uint32_t k = 0; k < 4; ++k)
        if ((double)edges[k] >= extent_tiles) { target = k; break; }
    if (ratio > 4.0) target = target > lv + 1 ? target : lv + 1;
    else target = target < lv - 1 ? target : lv - 1;
    if (target > lv && longer_out) {
        const double e0 = (double)edges[lv], e1 = (double)edges[target];
        const double r1 = (extent_tiles / e1 + 1.0) * (extent_tiles / e1 + 1.0);
        const double longer = (r1 / ratio) * (e1 / e0) * (e1 / e0);
        *longer_out = longer > 1.0 ? longer : 1.0;
    }
    return target;
}

// Supertile edges (in tiles) of levels 0..3 for a grid of tiles. Level 1 is the smallest power of two >= 8 that keeps the
// coarse bins <= 256 and <= 32 per axis (8 at 1080p: 135 bins); level 0 the smallest edge >= 3/4 of it that does (6 at
// 1080p: 240 bins; within 3/4 of level 1, so that the two rules cannot flip-flop); levels 2 and 3 are 2x and 4x level 1,
// at most 32 (16 and 32 at 1080p: 40 and 12 bins).
inline bool supertile_bins_fit(uint32_t tiles_x, uint32_t tiles_y, uint32_t edge) {
    const uint32_t bx = (tiles_x + edge - 1) / edge, by = (tiles_y + edge - 1) / edge;
    return bx * by <= MAX_SUPERTILES && bx <= MAX_SUPERTILES_PER_AXIS && by <= MAX_SUPERTILES_PER_AXIS;
}
inline void supertile_edges(uint32_t tiles_x, uint32_t tiles_y, uint32_t edges[4]) {
    uint32_t edge_c = 8;
    while (!supertile_bins_fit(tiles_x, tiles_y, edge_c)) edge_c *= 2;
    uint32_t edge_f = (3 * edge_c + 3) / 4;
    while (!supertile_bins_fit(tiles_x, tiles_y, edge_f)) ++edge_f;
    edges[0] = edge_f < edge_c ? edge_f : edge_c;
    for (uint32_t k = 1; k < 4; ++k) edges[k] = (edge_c << (k - 1u)) < 32u ? (edge_c << (k - 1u)) : 32u;
}
// Levels whose edges coincide (level 1 of 16 tiles and up, i.e. targets of ~2048 px: levels 2 and 3 both clamp to 32) are
// ONE level: a frame runs, and is accounted, at the lowest level with that edge.
inline uint32_t canonical_supertile_level(uint32_t level, const uint32_t edges[4]) {
    while (level > 1 && edges[level - 1] == edges[level]) --level;
    return level;
}

// The instantiation of raster_scan_kernel (render_kernels.hip) a BINNING_SCAN frame launches. mode: 0 the plain one;
// 1 mid-round exit for DENSE frames (supertile level >= 2); 2 mid-round exit with the sparse frames' machinery, for frames
// of a kind whose saturating tiles hold a good share of the work (KindState::midround) when several frames are in flight.
// Only the OBB and AABB3D variants at 1 or 4 samples without the bounding-box overlay have the exit, and AABB3D has one
// exit instantiation (1). Debug flags: BGS_DEBUG_NO_MIDROUND never, BGS_DEBUG_MIDROUND_ALWAYS at any level.
// trace: the per-tile trace (bgs_set_tile_trace), which exists without a depth buffer, without the overlay, at 1 or 4 samples.
// RasterInst is the ONE description of an instantiation: plan_frame chooses it (FramePlan::raster), graph_key stores key(),
// the launchers look it up, and the kernel takes its __launch_bounds__ and RUNS from it with its template arguments.
#ifndef BGS_MS_WAVES
// multisampled ellipse variants: 6 since round 6. Round 5's kernel (92-96 VGPRs) spilled 10-25 registers INTO the record loop at
// 80 and lost 10 %; with the tile id in scalar registers and the interior records in their own loop it is 83-86 and the 3-5
// registers that spill at 80 are tile set-up values outside the loops: dense 1 M even, scene-like +1.9 %, trained-like +4.5 %
// frames/s (profiles/r6_experiments/ms_waves_6_ab.txt)
#define BGS_MS_WAVES 6
#endif
#ifndef BGS_DENSE_RUNS_MS
#define BGS_DENSE_RUNS_MS 2u
#endif
#ifndef BGS_DENSE_RUNS
#define BGS_DENSE_RUNS 1u
#endif
struct RasterInst {
    int variant = RV_OBB;
    uint32_t samples = 4;
    bool depth = false, overlay = false;
    int mode = 0;
    bool trace = false;
    // The instantiations of raster_scan_kernel that are compiled (72), and the only statement of them: the launchers
    // (render_kernels.hip) instantiate what exists() admits and refuse everything else.
    constexpr bool exists() const {
        if (variant != RV_OBB && variant != RV_AABB3D && variant != RV_SURFEL) return false;
        if (samples != 1u && samples != 2u && samples != 4u && samples != 8u) return false;
        const bool plain = !overlay && (samples == 1u || samples == 4u);
        if (trace && (depth || !plain)) return false;
        return mode == 0 || (plain && ((mode == 1 && variant != RV_SURFEL) || (mode == 2 && variant == RV_OBB)));
    }
    // Runs per XCD of the rasteriser's work order (raster_scan_kernel: RUNS; tile_order_kernel deals out the same shares)
    constexpr uint32_t runs() const {
        return variant == RV_SURFEL ? 4u : (mode != 0 ? (samples == 4u ? BGS_DENSE_RUNS_MS : BGS_DENSE_RUNS) : 1u);
    }
    // Waves per SIMD (the kernel's __launch_bounds__): 8 for the single-sampled ellipse variants (<= 64 VGPRs), 6 for the surfel
    // variant; the multisampled instantiations carry six transmittance words per pixel instead of one (5 / 4 waves).
    constexpr int waves_per_simd() const {
        const bool surfel = variant == RV_SURFEL;
        return samples == 8u ? (surfel ? (depth ? 2 : 3) : (depth ? 3 : 4))   // ten transmittance words per pixel; 8 KB of depth samples per wave
             : samples >= 2u ? (surfel ? (depth ? 3 : 4) : (depth ? 5 : BGS_MS_WAVES)) : (surfel ? (depth ? 5 : 6) : (depth ? 7 : 8));
    }
    // one word per instantiation (GraphKey)
    constexpr uint32_t key() const {
        return samples | (depth ? 0x100u : 0u) | (overlay ? 0x200u : 0u) | ((uint32_t)mode << 10) | ((uint32_t)variant << 12) | (trace ? 0x4000u : 0u);
    }
};
inline int raster_variant(const FrameParams& fp) { return fp.aabb == 0u ? RV_OBB : (fp.gaussian_mode != 0u ? RV_AABB3D : RV_SURFEL); }
inline int raster_scan_mode(int variant, uint32_t samples, bool overlay, uint32_t level, bool kind_midround, int pipeline_depth,
                            uint32_t debug_flags) {
    if (variant == RV_SURFEL || (samples != 1u && samples != 4u) || overlay || (debug_flags & BGS_DEBUG_NO_MIDROUND)) return 0;
    if (level < 2u && !(kind_midround && pipeline_depth > 1) && !(debug_flags & BGS_DEBUG_MIDROUND_ALWAYS)) return 0;
    return (level >= 2u || variant == RV_AABB3D) ? 1 : 2;
}
// (trace: validate, bgs_frame.hip, refuses it for the frames that have no traced instantiation, so what comes back exists())
inline RasterInst raster_instantiation(const FrameParams& fp, uint32_t level, bool kind_midround, int pipeline_depth,
                                       uint32_t debug_flags, bool trace) {
    RasterInst r;
    r.variant = raster_variant(fp);
    r.samples = fp.sample_count;
    r.depth = fp.depth_ptr != 0ull;
    r.overlay = fp.visualize_bbox != 0u;
    r.mode = raster_scan_mode(r.variant, r.samples, r.overlay, level, kind_midround, pipeline_depth, debug_flags);
    r.trace = trace;
    return r;
}

// The instantiation of the vertex stage (project_kernel / project_emit_kernel, render_kernels.hip) a frame launches: the
// cloud's format x surfel records x ANY_MODE (another RasterizeMode than Color, or a draw mode). A precomputed-covariance
// cloud has no rotation and scale, hence no surfels (validate refuses the frame): 10 instantiations of each kernel.
struct ProjectInst {
    uint32_t format = CLOUD_F32;
    bool surfel = false, any_mode = false;
    constexpr bool exists() const { return format <= CLOUD_COV3D && !(format == CLOUD_COV3D && surfel); }
    constexpr uint32_t key() const { return format | (surfel ? 0x100u : 0u) | (any_mode ? 0x200u : 0u); }
};
inline ProjectInst project_instantiation(const FrameParams& fp, uint32_t cloud_format) {
    return {cloud_format, raster_variant(fp) == RV_SURFEL, fp.rasterize_mode != RASTERIZE_COLOR || fp.draw_mode != 0u};
}

// A lane's zeroed-every-frame scratch region for n splats and inst_cap tile instances, every part 256-byte aligned:
//   [Control | depth status | scan status | tile status | ranges | bin status | partition status | Control 1]
// (Control 1: the lane's second Control block, see FrameCleanup.) The look-back arrays have one spare tile each; the depth
// passes may use either tile size, so theirs are sized for the smaller one. The depth passes' four arrays lie pass_stride
// words apart, the tile passes' two inst_tiles * RADIX_BASE words. All fields are 8 bytes or pairs of 4: no padding, so
// that a GraphKey can carry a layout and be compared bytewise.
struct ScratchLayout {
    uint64_t bytes = 0;   // of the whole region
    uint64_t off_depth_status = 0, off_scan_status = 0, off_tile_status = 0, off_ranges = 0, off_bin_status = 0,
             off_part_status = 0, off_ctl1 = 0;
    uint64_t depth_tiles = 0, inst_tiles = 0;
    uint64_t inst_cap = 0;   // what it was made for
    uint32_t n = 0;
    uint32_t pass_stride = 0;
};
static_assert(sizeof(ScratchLayout) == 11 * 8 + 2 * 4, "ScratchLayout has no padding (GraphKey)");

inline ScratchLayout scratch_layout(uint32_t n, uint64_t inst_cap) {
    const auto align256 = [](uint64_t v) { return (v + 255u) / 256u * 256u; };
    ScratchLayout s;
    s.n = n;
    s.inst_cap = inst_cap;
    s.depth_tiles = ((uint64_t)n + sort_tile_size(false) - 1) / sort_tile_size(false) + 1;
    const uint64_t scan_tiles = ((uint64_t)n + 255) / 256 + 1;
    s.inst_tiles = (inst_cap + sort_tile_size(true) - 1) / sort_tile_size(true) + 1;
    s.pass_stride = (uint32_t)(s.depth_tiles * RADIX_BASE);
    uint64_t off = align256(sizeof(Control));
    s.off_depth_status = off;
    off += align256(4 * s.depth_tiles * RADIX_BASE * sizeof(uint32_t));
    s.off_scan_status = off;
    off += align256(scan_tiles * sizeof(unsigned long long));
    s.off_tile_status = off;
    off += align256(2 * s.inst_tiles * RADIX_BASE * sizeof(uint32_t));
    s.off_ranges = off;
    off += align256((uint64_t)RADIX_BASE * RADIX_BASE * 2 * sizeof(uint32_t));   // (uint2 per tile)
    s.off_bin_status = off;
    off += align256(scan_tiles * MAX_SUPERTILES * sizeof(uint32_t));
    s.off_part_status = off;
    off += align256((((uint64_t)n + KEYGEN_TILE - 1) / KEYGEN_TILE + 1) * sizeof(uint32_t));
    s.off_ctl1 = off;
    off += align256(sizeof(Control));
    s.bytes = off;
    return s;
}

// A splitter table is usable only if it is ascending: bucket(key) = number of splitters <= key is monotone in
// the key exactly then, and the bucket sort's ORDER (not just its balance) rests on that.
inline bool splitters_ascending(const uint32_t* key, uint32_t count) {
    for (uint32_t i = 1; i < count; ++i)
        if (key[i - 1] > key[i]) return false;
    return true;
}

}  // namespace bgs
