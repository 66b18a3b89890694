/*
 * bgs.h — C ABI of libbgs: the MI355X-native Gaussian-splat sort + rasterize path.
 *
 * This is the drop-in boundary for ONE hot path of mosure/bevy_gaussian_splatting
 * (citations are into the reference tree):
 *
 *   cloud upload   <- RenderAsset upload of the planar cloud
 *                     (src/lib.rs:65-68, src/render/mod.rs:279-313,
 *                      layout src/gaussian/formats/planar_3d.rs:28-54)
 *   bgs_sort       <- run_radix_sort   (src/sort/radix.rs:616-756, kernels src/sort/radix.wgsl)
 *                     rayon_sort       (src/sort/rayon.rs:27-130)   [SortMode::Rayon ordering]
 *   bgs_render     <- DrawGaussianInstanced::render (src/render/mod.rs:1513-1569),
 *                     vs_points / fs_main (src/render/gaussian.wgsl:184-505),
 *                     blend state (src/render/mod.rs:944-948)
 *
 * The reference has no FFI of its own (it is a Bevy plugin); these entry points are
 * what a `hip-sys`-style Rust binding would declare.
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary, the library never aborts;
 *   - every function returns BGS_OK (0) or a negative bgs_status; the message for the
 *     last failure on a context is available from bgs_last_error();
 *   - all matrices are column-major float[16] (glam / WGSL convention): m[4*c + r];
 *   - host pointers are borrowed for the duration of the call only;
 *   - device memory is owned by the library behind opaque handles;
 *   - a bgs_ctx binds one HIP device (and a few HIP streams of its own) and is NOT re-entrant
 *     (matches Bevy: one render thread); distinct contexts are independent.
 *   - there is NO CPU fallback: without a usable HIP device bgs_create fails with
 *     BGS_EHIP.
 *
 * This header is the seam and nothing else: context, cloud upload, sort, render, the frame's targets and
 * the frame pipeline. Diagnostics, test hooks and experiment switches (per-tile trace, counters of the
 * adaptive machinery, the HBM probe, the radix kernel on caller keys, the ln self-test, debug flags, the
 * queue-holder switch) are declared in bgs_diag.h; libbgs.so exports both sets.
 */
#ifndef BGS_H
#define BGS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BGS_VERSION_MAJOR 0
#define BGS_VERSION_MINOR 9 /* 0.9: the grid cap of the persistent kernels and the read-back of a frame's grids (bgs_diag.h: bgs_set_grid_cap,
                               bgs_debug_frame_grids); the seam of this header, bgs_view, bgs_settings and bgs_stats as in 0.4.
                               Still 0.9 with the view's colour attachment: bgs_view.reserved[0] got two named values
                               (BGS_VIEW_ATTACH_*; size, offsets and the field's name as they were); zero — what every earlier
                               binding passes and what bgs_view_perspective sets — is the behaviour of before, bit for bit.
                               Still 0.9 with the cloud's own bounds: bgs_settings.reserved[0] got two named values (BGS_BOUNDS_*;
                               size, offsets and the field's name as they were); zero — what every earlier binding passes and what
                               bgs_settings_default sets — is the behaviour of before, bit for bit.
                               0.8: the read-back of what a frame leaves for the next (bgs_diag.h: bgs_debug_frame_leftovers); the seam of this
                               header, bgs_view, bgs_settings and bgs_stats as in 0.4.
                               0.7: the tile rasterisers' test hook (bgs_diag.h: bgs_selftest_raster); the seam of this header, bgs_view,
                               bgs_settings and bgs_stats as in 0.4.
                               0.6: the bucket sort path's test hooks (bgs_diag.h: bgs_selftest_bucket_sort, bgs_selftest_keygen_buckets); the
                               seam of this header, bgs_view, bgs_settings and bgs_stats as in 0.4.
                               0.5: the binning stage's test hooks (bgs_diag.h: bgs_selftest_bin, bgs_debug_frame_lists); the seam of
                               this header, bgs_view, bgs_settings and bgs_stats as in 0.4.
                               0.4: bgs_abi_check, bgs_comm_* (the multi-GPU frame gather), sample_count 0 = default; struct layouts as 0.3
                               (0.3: bgs_view gained sample_count + depth_device_ptr, 16 bytes longer; bgs_stats 16 bytes longer than 0.2's).
                               Still 0.4 with the particle behaviours: purely additive (one function, one POD typedef; bgs_view,
                               bgs_settings and bgs_stats as they were), so a 0.4 binding keeps working unchanged.
                               Still 0.4 with the kept sort order: two RESERVED fields of bgs_view got names (entries_device_ptr,
                               entry_count; size and offsets as they were); zero in both — what a 0.4 binding passes and what
                               bgs_view_perspective sets — is the behaviour of before, bit for bit */

typedef enum bgs_status {
    BGS_OK = 0,
    BGS_EINVAL = -1,    /* bad argument / unsupported setting               */
    BGS_ENOMEM = -2,    /* host or device allocation failed                 */
    BGS_EHIP = -3,      /* HIP runtime error (no device, launch failure...) */
    BGS_ECAPACITY = -4, /* tile-instance buffer could not be grown enough   */
    BGS_EINTERNAL = -5  /* device-side watchdog tripped (bounded spin)      */
} bgs_status;

typedef struct bgs_ctx bgs_ctx;
typedef struct bgs_cloud bgs_cloud;

/* The fields of Bevy's `View` uniform that the reference shaders read
 * (src/render/helpers.wgsl:18-38, src/render/transform.wgsl:5-8,
 *  src/render/gaussian_2d.wgsl:104, src/sort/radix.wgsl:90) plus the clear colour
 * (examples/headless.rs:70). The caller supplies every matrix explicitly, exactly as
 * Bevy does on the CPU, so the library never re-derives one from another. */
typedef struct bgs_view {
    float world_from_view[16]; /* camera transform; world_position = column 3        */
    float view_from_world[16];
    float clip_from_view[16];
    float clip_from_world[16]; /* also used as unjittered_clip_from_world (no TAA)   */
    float viewport[4];         /* x, y, width, height in pixels (View.viewport)      */
    float clear_color[4];      /* linear RGBA the target is cleared to before draws  */
    /* RasterizeMode::OpticalFlow only (src/material/optical_flow.wgsl:16-53): the PREVIOUS frame's
     * clip_from_world (Bevy's previous_view_uniforms) and globals.delta_time in seconds */
    float previous_clip_from_world[16];
    float delta_time;
    /* The camera's `Msaa` component as the pipeline is specialised on it: CloudPipelineKey.sample_count =
     * msaa.samples() (src/render/mod.rs:357,412,422) -> MultisampleState.count (:975-979). 1 = Msaa::Off, 2 / 4 / 8 =
     * Msaa::Sample2 / Sample4 / Sample8; 4 is Bevy's default, i.e. what every camera of the reference's examples and
     * tests runs with (nothing in the reference sets Msaa; src/utils.rs:34 `msaa_samples` is never read). With N > 1
     * samples coverage (and the depth test) is decided per sample at the graphics APIs' standard sample positions, the
     * fragment stage runs once per pixel at the pixel centre, every covered sample blends the same source colour, and
     * the image handed back is the resolved one (mean of the samples). 0 (a zero-initialised bgs_view) means "not set"
     * and renders with Msaa::default() = 4; anything else is BGS_EINVAL. bgs_view_perspective sets 4. */
    uint32_t sample_count;
    uint32_t entry_count;      /* records behind entries_device_ptr: bgs_cloud_len(cloud) when that is set, else 0 */
    /* reserved[0]: WHAT depth_device_ptr NAMES, one of BGS_VIEW_ATTACH_* below. The word keeps the name bindings built against
     * 0.4 know it by (they zero it: BGS_VIEW_ATTACH_DEPTH_ONLY, the behaviour of before, bit for bit; bgs_view_perspective
     * sets 0 too); size and offsets are as they were.
     *   BGS_VIEW_ATTACH_DEPTH_ONLY (0): the depth plane described at depth_device_ptr, or nothing (pointer 0). The target
     *     starts from clear_color.
     *   BGS_VIEW_ATTACH_COLOR (1): the view's ATTACHMENT PAIR in ONE caller-owned allocation, what the engine's opaque passes
     *     left behind: the depth plane exactly as below (w * h * S floats, [y][x][sample], S = sample_count), and at byte offset
     *     round_up(w * h * S * 4, 16) the colour plane, w * h * S float4 laid out [y][x][sample]: linear, premultiplied,
     *     unclamped RGBA in f32. The splats are one Transparent3d draw into a target that already holds the scene: every
     *     sample blends as dst = src + dst (1 - src.a) (src/render/mod.rs:944-948), and the image handed back is the resolve.
     *     A host without geometry hands a depth plane of 0.0. clear_color is IGNORED for such a frame. A second cloud is
     *     drawn over a first one this way (S = 1: the first frame's f32 image IS a colour plane).
     *     Arithmetic, per pixel and channel c, with C and the per-sample transmittances T_s as the frame forms them
     *     (T_s = S r_s, the product of the pixel's common and per-sample factors, rounded once), d_s the plane's sample:
     *         acc   = T_0 * d_0.c
     *         acc   = fma(T_s, d_s.c, acc)            s = 1 .. S-1, in sample order
     *         out.c = fma(acc, 1/S, C.c)              alpha: C.a = 1 - mean_s(T_s) as in every frame
     *     every line rounded once (the products contract into the fused multiply-adds written here and nowhere else; 1/S is
     *     exact). A pixel no fragment reaches (C = 0, T_s = 1) is the left-to-right f32 sum of its samples times 1/S.
     *     The packed outputs (sRGB8, Rgba16Float, packed-only) are conversions of that pixel, as ever.
     *     Works wherever the depth attachment does (both binning modes, asynchronous lanes, kept-order frames, captured
     *     graphs: flag and address travel with the frame, no new capture) and is refused where that is (the tile trace).
     *     bgs_stats.algorithmic_bytes counts the w * h * S * 16 bytes read. The memory must stay valid and UNWRITTEN until
     *     the frame has completed (the depth attachment's rule).
     *   BGS_EINVAL, naming the field: reserved[0] > 1; BGS_VIEW_ATTACH_COLOR with depth_device_ptr == 0 or with a
     *     depth_device_ptr that is not 16-byte aligned. */
    uint32_t reserved[1];
#define BGS_VIEW_ATTACH_DEPTH_ONLY 0u
#define BGS_VIEW_ATTACH_COLOR 1u
    /* The view's depth attachment the draw is tested against (src/render/mod.rs:959-974: Depth32Float,
     * CompareFunction::GreaterEqual — reverse-Z —, depth_write_enabled false): a DEVICE pointer to
     * viewport.w * viewport.h * sample_count floats laid out [y][x][sample] (sample order: the standard pattern's) (what Bevy's opaque passes left), or
     * 0 = no scene depth (every fragment passes, as against a buffer cleared to 0.0). A quad's depth is its
     * splat's constant NDC z (src/render/gaussian.wgsl:429-433). The memory must stay valid and unchanged until
     * the frame has completed (bgs_device_alloc / bgs_upload below serve hosts without a HIP runtime). */
    uint64_t depth_device_ptr;
    /* The camera's chunk of `SortedEntries` KEPT ON THE DEVICE (src/sort/mod.rs:331-393; the draw binds it per camera,
     * src/render/mod.rs:1548-1554): a DEVICE pointer to entry_count bgs_sort_entry records in CALLER-OWNED memory, 8-byte
     * aligned (bgs_device_alloc / bgs_upload, or any device memory of the caller), or 0 = none: then bgs_sort and
     * bgs_render behave as they always have. The reference sorts only when its SortTrigger says so (update_sort_trigger,
     * src/sort/mod.rs:153-194) and draws every frame in between from the chunk as the last sort left it; with this field
     * a host does the same: bgs_sort with the chunk when `needs_sort`, bgs_render with the chunk every frame.
     *   entry_count must equal bgs_cloud_len(cloud) when the pointer is set, and be 0 when it is not.
     *   bgs_sort, pointer set: OUTPUT. After the sort its n entries are also copied to the chunk (device to device, on the
     *     stream, behind the sort), in the order contract of bgs_sort: Radix ascending key, ties by index, culled entries
     *     last with key all-ones; Rayon / Std their order; None (1, i). host_out works as before. The chunk is complete
     *     when the call returns.
     *   bgs_render, pointer set: INPUT. The frame computes no keys and runs no depth sort: it draws entries[0 .. n) in that
     *     order, entry 0 first (furthest back). Entries with key == 0xFFFFFFFF are skipped (vs_points,
     *     src/render/gaussian.wgsl:191-195), and so are entries with index >= n (the reference leaves those to WebGPU's
     *     robustness rules). Every other per-splat test stays in the vertex stage, at the CURRENT camera: the frustum,
     *     DrawMode, the depth attachment. A splat named twice is drawn twice. settings.sort_mode and radix_depth_bits do
     *     not influence such a frame. RasterizeMode::Depth normalises by entries 1 and n - 1 of the list read as [entries
     *     that are drawn, in order] ++ [skipped entries, in order] — for a chunk bgs_sort wrote that IS the list —, an
     *     index >= n among them read as n - 1.
     *     Works with both binning modes, every cloud format, sample count, raster / draw mode, the depth attachment, the
     *     packed outputs, particle steps, and asynchronous frames on every lane (no host round trip). Under
     *     bgs_set_graphs(1) such a frame is replayed from a captured graph of its own kind, which a lane keeps beside the
     *     one of its sorting frames: the compaction is the node that is updated, and its arguments carry the chunk, so
     *     the chunk address may change between replays (a host with several cameras) without a new capture.
     *     Stats: sort_path = 2, depth_passes = 0, stage_ms[BGS_STAGE_KEYGEN] = the compaction of the chunk into the draw
     *     list, stage_ms[BGS_STAGE_DEPTH_SORT] = 0, draw_count = entries that pass the key / index test, visible_count
     *     as in every rendered frame (drawn splats that pass the vertex stage's tests). bgs_sorted_entries_device_ptr
     *     after it: the drawable prefix, as after any render.
     *   The memory must stay valid and UNWRITTEN until the frame has completed (the rule of depth_device_ptr): a host
     *   that sorts into a chunk while frames that read it are in flight orders the two itself (bgs_sort completes the
     *   frames in flight before it runs).
     *   BGS_EINVAL, naming the field: a misaligned pointer, entry_count != n with the pointer set, entry_count != 0
     *   without it. */
    uint64_t entries_device_ptr;
} bgs_view;

/* gaussian_mode: src/gaussian/settings.rs:17-22 */
#define BGS_GAUSSIAN_2D 0u
#define BGS_GAUSSIAN_3D 1u
/* color_space: src/render/mod.rs:1066-1069 */
#define BGS_COLOR_SRGB 0u
#define BGS_COLOR_LINEAR 1u
/* sort_mode: src/sort/mod.rs:46-58 */
#define BGS_SORT_NONE 0u  /* draw in entry order (key=1,index=i  src/sort/mod.rs:347-354) */
#define BGS_SORT_RADIX 1u /* GPU radix semantics: cull + inverted key, stable            */
#define BGS_SORT_RAYON 2u /* CPU-sort semantics: key=bits(dist2), descending, no cull    */
#define BGS_SORT_STD 3u   /* same ordering contract as RAYON (src/sort/std_sort.rs)      */

/* rasterize_mode: discriminants of RasterizeMode (src/gaussian/settings.rs:38-47); selects the
 * colour the vertex stage gives a splat (src/render/gaussian.wgsl:312-417). OpticalFlow needs the
 * previous frame's clip_from_world + delta_time in bgs_view. Velocity needs a 4D cloud: BGS_EINVAL. */
#define BGS_RASTERIZE_CLASSIFICATION 0u
#define BGS_RASTERIZE_COLOR 1u /* default */
#define BGS_RASTERIZE_DEPTH 2u
#define BGS_RASTERIZE_NORMAL 3u
#define BGS_RASTERIZE_OPTICAL_FLOW 4u
#define BGS_RASTERIZE_POSITION 5u
#define BGS_RASTERIZE_VELOCITY 6u

/* draw_mode: src/gaussian/settings.rs:6-12 -> DRAW_SELECTED / HIGHLIGHT_SELECTED shader defs
 * (src/render/mod.rs:889-893; src/render/gaussian.wgsl:203-205, 423-427) */
#define BGS_DRAW_ALL 0u
#define BGS_DRAW_SELECTED 1u           /* splats with visibility < 0.5 are not drawn         */
#define BGS_DRAW_HIGHLIGHT_SELECTED 2u /* splats with visibility > 0.5 drawn (0.3, 1, 0.1, 1) */

/* CloudUniform (src/render/mod.rs:995-1009) + the CloudSettings fields that select the
 * pipeline specialisation (src/gaussian/settings.rs:87-132, src/render/mod.rs:770-896). */
typedef struct bgs_settings {
    float transform[16];              /* model matrix (GlobalTransform)                  */
    float global_opacity;             /* default 1                                       */
    float global_scale;               /* default 1                                       */
    uint32_t gaussian_mode;           /* BGS_GAUSSIAN_3D default                         */
    uint32_t aabb;                    /* 0 = OBB (default), 1 = AABB   settings.rs:113   */
    uint32_t opacity_adaptive_radius; /* default 1                     settings.rs:116   */
    uint32_t color_space;             /* BGS_COLOR_SRGB default                          */
    uint32_t radix_depth_bits;        /* 16 | 24 | 32 (default 32)     settings.rs:52-77 */
    uint32_t sh_degree;               /* 0..3; reference is compile-time sh3             */
    uint32_t sort_mode;               /* BGS_SORT_RADIX default                          */
    uint32_t rasterize_mode;          /* BGS_RASTERIZE_COLOR default   settings.rs:38-47 */
    uint32_t num_classes;             /* default 1 (Classification)    settings.rs:124   */
    uint32_t draw_mode;               /* BGS_DRAW_ALL default          settings.rs:6-12  */
    uint32_t visualize_bounding_box;  /* default 0: VISUALIZE_BOUNDING_BOX (settings.rs:95,117; key bit
                                         src/render/mod.rs:418,824; src/render/gaussian.wgsl:486-495): fragments in the
                                         outer 8 % of a quad's uv square are (0.3, 1, 0.1, 1) — the quads' frames  */
    /* reserved[0]: WHOSE CloudUniform.min / .max the frame gets, one of BGS_BOUNDS_* below. The word keeps the name bindings
     * built against 0.4 know it by (they zero it: BGS_BOUNDS_CALLER, the behaviour of before, bit for bit; bgs_settings_default
     * sets 0 too); size and offsets are as they were.
     *   BGS_BOUNDS_CALLER (0): position_min / position_max below, as given.
     *   BGS_BOUNDS_CLOUD (1): the box of the RESIDENT cloud, taken on the device: CommonCloud::compute_aabb
     *     (src/gaussian/interface.rs:22-63), which calculate_bounds (src/gaussian/cloud.rs:45-62) attaches to every cloud
     *     entity. For hosts that never hold the positions: a cloud morphed or time-sliced on the device and uploaded from
     *     device planes, a cloud moved by bgs_cloud_apply_particle_behaviors. position_min / position_max are IGNORED, by
     *     every rasterize mode; only RasterizeMode::Position reads bounds at all (src/render/gaussian.wgsl:377), and every
     *     other mode's frame is the bits of its BGS_BOUNDS_CALLER frame.
     *     Arithmetic, per axis, over the UNTRANSFORMED position_visibility[i].xyz of all n splats, in f32, rounded once:
     *         min = fold(+inf, f32::min) of (p - 0.1f)          max = fold(-inf, f32::max) of (p + 0.1f)
     *     f32::min / max ignore a NaN operand (a NaN coordinate contributes nothing to its axis), +-inf propagate, an axis
     *     with no contributor keeps +inf / -inf. The visibility lane is not read. The result does not depend on the order
     *     of the splats (csrc/bounds_math.h says why), so it is a contract: bit for bit what a host computes that way.
     *     The box is reduced LAZILY and kept in the bgs_cloud: uploads and particle steps leave it invalid, and the first
     *     bgs_sort / bgs_render that says BGS_BOUNDS_CLOUD on such a cloud completes the frames in flight (as a particle
     *     step does: they stay in the ring), runs one pass over the position plane (16 bytes a splat) and waits for 24
     *     bytes to come back. Every later call finds the box in the cloud. Hosts that never ask pay nothing.
     *     Works wherever the caller's bounds do: the box travels with the frame like position_min / position_max
     *     (both binning modes, asynchronous lanes, kept-order frames, captured graphs: no new capture).
     *     n == 0: the reference's compute_aabb is None; the caller's values are used and nothing is launched.
     *   BGS_EINVAL from bgs_sort and bgs_render, naming the field: reserved[0] > 1. */
    uint32_t reserved[1];
#define BGS_BOUNDS_CALLER 0u
#define BGS_BOUNDS_CLOUD 1u
    float position_min[4];            /* CloudUniform.min/max = the cloud entity's Aabb   */
    float position_max[4];            /* (src/render/mod.rs:1070-1071); Position mode     */
} bgs_settings;

/* src/sort/mod.rs:324-329 */
typedef struct bgs_sort_entry {
    uint32_t key;
    uint32_t index;
} bgs_sort_entry;

/* Per-stage wall time (HIP events on the context's stream) and counters of the most
 * recent bgs_sort/bgs_render call. Times in milliseconds. */
#define BGS_STAGE_KEYGEN 0   /* keygen + 4-place global digit histogram             */
#define BGS_STAGE_DEPTH_SORT 1 /* all onesweep passes over the depth keys            */
#define BGS_STAGE_PROJECT 2  /* per-splat projection + SH + tile-instance emission   */
#define BGS_STAGE_TILE_SORT 3 /* stable radix passes over tile ids                   */
#define BGS_STAGE_RANGES 4   /* per-tile [start,end)                                 */
#define BGS_STAGE_RASTER 5   /* per-16x16-tile front-to-back blend                   */
#define BGS_STAGE_COUNT 6

typedef struct bgs_stats {
    float stage_ms[BGS_STAGE_COUNT];
    float total_ms;              /* first to last event of the call                    */
    uint32_t splat_count;        /* N                                                  */
    uint32_t visible_count;      /* V: splats that pass the frustum test               */
    uint32_t draw_count;         /* D: entries that go through the radix passes / reach the
                                    vertex stage (key != culled sentinel)               */
    uint32_t sort_path;          /* depth sort of the call: 0 = onesweep digit passes, 1 = bucket sort
                                    (one launch; chosen per frame), 2 = kept: none, the frame drew the
                                    caller's entries (bgs_view.entries_device_ptr)        */
    uint64_t instance_count;     /* I: (tile, splat) instances emitted                 */
    uint64_t instance_capacity;  /* BGS_BINNING_SORT: tile instances the lane's buffers hold (0 until that mode ran) */
    uint32_t tiles_x, tiles_y;
    uint32_t depth_passes;       /* radix digit places used for the depth keys         */
    uint32_t tile_passes;        /* radix passes used for the tile ids                 */
    uint64_t algorithmic_bytes;  /* SURVEY 8(d) bytes_frame (or bytes_sort) of the call */
    uint32_t regrow_count;       /* times a frame was re-run because a data-dependent capacity was
                                    too small (tile instances, supertile lists, bucket sort) */
    uint32_t binning_mode;       /* BGS_BINNING_* used by the call                     */
    uint32_t frames_averaged;    /* stage_ms/total_ms = mean over this many frames (async: all
                                    frames since the last read-back, at most 64)        */
    uint32_t list_capacity;      /* BGS_BINNING_SCAN: entries each supertile list could hold  */
    uint64_t list_entries_allocated; /* BGS_BINNING_SCAN: 8-byte list entries allocated for the lane (all supertile
                                    lists together); instance_count is how many of them the frame filled */
    uint32_t strip_tiles;        /* tiles of the frame that were drawn by four strip waves instead of one wave (dense
                                    frames: the tiles a completed frame found heavy); 0 otherwise */
    uint32_t tile_saturation;    /* BGS_BINNING_SCAN frames drawn in cost order: bit 16 = known, bits 0-14 = share (x 0x7FFF) of
                                    the tile work of the completed frame the order was made of that was in tiles whose
                                    every pixel went opaque before their list ended — what selects the mid-round-exit
                                    rasteriser for a kind of frame; bit 31: this frame ran it. 0 otherwise */
} bgs_stats;

/* ---- lifecycle ------------------------------------------------------------------ */
int bgs_create(int hip_device, bgs_ctx** out);
void bgs_destroy(bgs_ctx* ctx);
const char* bgs_last_error(const bgs_ctx* ctx); /* ctx may be NULL: global message   */
uint32_t bgs_version(void);                     /* (major << 16) | minor             */
/* A binding's handshake, once at start-up: the version and the struct sizes IT was built with. BGS_EINVAL (message via
 * bgs_last_error(NULL)) unless they are this library's — the structs are passed by pointer, so a binding built
 * against another layout (0.2's bgs_view was 16 bytes shorter) would otherwise have the library read past its
 * struct. C callers: bgs_abi_check(BGS_ABI_VERSION, sizeof(bgs_view), sizeof(bgs_settings), sizeof(bgs_stats)). */
#define BGS_ABI_VERSION ((BGS_VERSION_MAJOR << 16) | BGS_VERSION_MINOR)
int bgs_abi_check(uint32_t version, uint32_t sizeof_view, uint32_t sizeof_settings, uint32_t sizeof_stats);
/* Identity of the kernel sources the library was compiled from: the SHA-256 (64 hex digits) over the HIP
 * sources and headers of libbgs (csrc/ .hip and .h files). The Python binding, the tests and bench.py refuse a library whose id is not the
 * tree's (and rebuild it); counter files under profiles/ carry the same stamp. */
const char* bgs_build_id(void);

/* Fill defaults equal to CloudSettings::default() (src/gaussian/settings.rs:110-131)
 * with an identity transform. */
void bgs_settings_default(bgs_settings* out);

/* Convenience: build a bgs_view the way Bevy builds its View uniform for
 * `Camera3d::default()` (infinite reverse-Z right-handed perspective) from a camera
 * world transform. Pure host arithmetic in f32. clear_color is set to opaque black, sample_count to 4
 * (Msaa::default() = Sample4), depth_device_ptr, entries_device_ptr and entry_count to 0. */
void bgs_view_perspective(const float world_from_view[16], float fov_y_radians,
                          float near_plane, uint32_t width, uint32_t height,
                          bgs_view* out);

/* ---- cloud upload (planar SoA, src/gaussian/formats/planar_3d.rs:45-54) ---------- */
/* DEVICE PLANES. Each plane pointer of the three uploads below is, plane by plane, either host memory or device memory
 * of the context's device; the planes of one call may be mixed. The library asks the runtime where each pointer lies:
 *   - host plane: pageable, pinned or managed memory, and any pointer the runtime does not know. It is copied to the
 *     device (blocking) and has no alignment rule.
 *   - device plane: device memory of the context's device (bgs_device_alloc, or the caller's own). It must be 16-byte
 *     aligned. No copy of it is made: the library packs the cloud's records straight from where the plane lies; only
 *     position_visibility, which the cloud keeps as a plane of its own, is copied device to device. The upload never
 *     writes a plane of the caller's.
 *   - BGS_EINVAL, naming the plane, before anything is allocated: device memory of another device, and a device plane
 *     that is not 16-byte aligned.
 * Ordering of a device plane: the work that writes it is either complete, or was enqueued on the stream bgs_stream(ctx)
 * names BEFORE the call: the upload orders itself behind what that stream holds at the call, on the device, with no
 * synchronisation by the caller in between. The upload returns once the cloud is complete (it synchronises its own
 * stream), so the caller may overwrite or free its planes as soon as it returns, e.g. with the next time's output of a
 * kernel that produces a cloud per frame; bgs_cloud_free the previous cloud once its frames are done.
 * n == 0 is BGS_OK and looks at no pointer. */
/* f32 planes: position_visibility[n][4], spherical_harmonic[n][48] (index 3*k+c),
 * rotation[n][4] as [w,x,y,z], scale_opacity[n][4] (sx,sy,sz,opacity). */
int bgs_cloud_upload_f32(bgs_ctx* ctx, uint32_t n, const float* position_visibility,
                         const float* spherical_harmonic, const float* rotation,
                         const float* scale_opacity, bgs_cloud** out);
/* f16 planes (src/render/bindings.wgsl:102-140, src/gaussian/f16.rs:29-55):
 * position_visibility stays f32; spherical_harmonic[n][24] u32 (low half = even
 * coefficient, src/render/planar.wgsl:117-130); rotation_scale_opacity[n][4] u32 =
 * [rot0|rot1], [rot2|rot3], [s0|s1], [s2|opacity] with the FIRST value in the high half. */
int bgs_cloud_upload_f16(bgs_ctx* ctx, uint32_t n, const float* position_visibility,
                         const uint32_t* spherical_harmonic_h2,
                         const uint32_t* rotation_scale_opacity, bgs_cloud** out);
/* The `precompute_covariance_3d` storage variant (src/gaussian/f32.rs:218-251 Covariance3dOpacity,
 * src/render/planar.wgsl:132-152, src/render/gaussian_3d.wgsl:77-88): instead of rotation and scale the
 * cloud carries covariance_3d_opacity[n][8] = cov3d[6] (xx, xy, xz, yy, yz, zz of M^T M, M = S R:
 * src/gaussian/covariance.rs:4-41), opacity, pad. The vertex stage then skips compute_cov3d — and with
 * it the model transform's linear part and global_scale, which the reference applies only there.
 * 3D gaussian mode only (BGS_EINVAL for 2DGS and for RasterizeMode::Normal: both need rotation / scale). */
int bgs_cloud_upload_cov3d_f32(bgs_ctx* ctx, uint32_t n, const float* position_visibility,
                               const float* spherical_harmonic, const float* covariance_3d_opacity,
                               bgs_cloud** out);
void bgs_cloud_free(bgs_ctx* ctx, bgs_cloud* cloud);
uint32_t bgs_cloud_len(const bgs_cloud* cloud);

/* ---- particle behaviours: move splats of a resident cloud on the device -------------- */
/* ParticleBehavior (src/morph/particle.rs:349-358, #[repr(C)] Pod: 64 bytes; src/morph/particle.wgsl:14-19) */
typedef struct bgs_particle_behavior {
    uint32_t indicies[4]; /* [0] = splat index, read as int32: negative = inactive (particle.wgsl:46); [1..3] unused.
                             The reference's spelling. */
    float velocity[4];
    float acceleration[4];
    float jerk[4];
} bgs_particle_behavior;
/* One run of apply_particle_behaviors (src/morph/particle.wgsl:23-53) with globals.delta_time = delta_time, the compute
 * pass the reference runs before the draw (run_particle_behaviors, src/morph/particle.rs): call it before the frame's
 * bgs_render. behaviors_device_ptr: `count` bgs_particle_behavior records in CALLER-OWNED device memory, 16-byte aligned
 * (bgs_device_alloc / bgs_upload / bgs_download serve hosts without a HIP runtime), as the reference binds a storage
 * buffer of behaviours to the pass. For every record b in [0, count), with i = (int32)indicies[0] and n = bgs_cloud_len:
 *   i < 0 or i >= n: the record is skipped entirely (no position write, velocity and acceleration untouched);
 *   otherwise, on all four lanes (x, y, z AND w: the visibility moves too), in f32, every operation rounded once, in this order:
 *     position[i]  += ((v*dt) + (((0.5*a)*dt)*dt)) + ((((c6*j)*dt)*dt)*dt)     c6 = (float)(1.0 / 6.0)
 *     velocity     += (a*dt) + (((0.5*j)*dt)*dt)
 *     acceleration += j*dt
 *   with v, a, j the record's values before the call. jerk and indicies are never written.
 * Exactly `count` records act (the reference dispatches whole 32 x 32 workgroups past its buffer's end), and an index >= n
 * skips the record (the reference leaves that to WebGPU's robustness rules).
 * PRECONDITION: the indices of the active records are distinct. Two records that name one splat race in the reference;
 * here the result for that splat is then unspecified (the C++ and Python layers check it on the host before upload).
 * Works on every cloud format (position_visibility is f32 in all of them). position_min / position_max of bgs_settings
 * stay the caller's under BGS_BOUNDS_CALLER: no AABB is refreshed (the reference's TODO, src/gaussian/cloud.rs:43). Under
 * BGS_BOUNDS_CLOUD (bgs_settings.reserved[0]) the step invalidates the cloud's box, and the next bgs_sort / bgs_render that
 * asks for it reduces the stepped positions.
 * ORDERING: the step is a pipeline barrier. Frames in flight are completed first (they — and a re-run of them — draw the
 * positions they were enqueued with; they stay in the ring for bgs_pipeline_pop); every bgs_sort / bgs_render after the
 * call sees the stepped cloud. The call only ENQUEUES the step and returns: the behaviours' memory must stay valid, and
 * must not be written or read back, until a frame enqueued after the call has completed or bgs_synchronize has returned.
 * BGS_EINVAL: ctx or cloud NULL, a NULL or misaligned pointer with count > 0, a delta_time that is not finite.
 * count == 0: BGS_OK, nothing happens. */
int bgs_cloud_apply_particle_behaviors(bgs_ctx* ctx, bgs_cloud* cloud, void* behaviors_device_ptr, uint32_t count,
                                       float delta_time);

/* ---- the hot path ----------------------------------------------------------------- */
/* Depth sort for one view. Result is kept on the device (until the next call; and, with
 * view->entries_device_ptr set, copied to that caller-owned chunk, see bgs_view) and, if host_out != NULL, copied to
 * host_out[n]. Order contract for BGS_SORT_RADIX: ascending key, ties by ascending
 * splat index, culled splats (key all-ones) last  (src/sort/radix.wgsl:109-279). */
int bgs_sort(bgs_ctx* ctx, const bgs_cloud* cloud, const bgs_view* view,
             const bgs_settings* settings, bgs_sort_entry* host_out);

/* Sort (re-done with every call unless view->entries_device_ptr hands the frame a kept order, see bgs_view; the
 * benchmark sorts every frame) + project + bin + rasterize one view. Output: viewport.w x viewport.h RGBA f32, premultiplied, linear,
 * unclamped, row 0 = top. rgba_host_out may be NULL (result stays on the device). */
int bgs_render(bgs_ctx* ctx, const bgs_cloud* cloud, const bgs_view* view,
               const bgs_settings* settings, float* rgba_host_out);

/* Device pointer + size in bytes of the framebuffer written by the last bgs_render
 * (for an RCCL gather or zero-copy interop). Valid until the next render/destroy. */
int bgs_framebuffer_device_ptr(bgs_ctx* ctx, void** dptr, uint64_t* bytes);
/* Also produce, with every bgs_render, the frame in the reference's colour-attachment format
 * TextureFormat::Rgba8UnormSrgb (src/render/mod.rs:917-921, examples/headless.rs:120-123): linear
 * RGB -> sRGB transfer -> unorm8, alpha linear, 4 bytes per pixel R,G,B,A. Default off.
 * Exact for every f32 value: colour = round to nearest of the exact sRGB OETF (255 oetf(x)), alpha = round to
 * nearest of 255 x; NaN and values <= 0 (-0 included) -> 0, values >= 1 (+inf included) -> 255. */
int bgs_set_output_srgb8(bgs_ctx* ctx, int enabled);
int bgs_framebuffer_srgb8_device_ptr(bgs_ctx* ctx, void** dptr, uint64_t* bytes);
/* The same for an hdr camera: the reference's colour attachment is then TextureFormat::Rgba16Float
 * (src/render/mod.rs:917-921). Every bgs_render also produces the frame as IEEE binary16 RGBA (8 bytes per
 * pixel, round to nearest even, subnormals kept, overflow to inf, NaN -> NaN), linear and unclamped. Exclusive with
 * the sRGB8 output
 * (enabling one disables the other); bgs_set_srgb8_target / bgs_pipeline_pop's second pointer then carry
 * this image. Like the 8-bit image it is ONE conversion of the f32 result, not a per-blend quantisation. */
int bgs_set_output_rgba16f(bgs_ctx* ctx, int enabled);
int bgs_framebuffer_rgba16f_device_ptr(bgs_ctx* ctx, void** dptr, uint64_t* bytes);
/* Frames that write a packed image (sRGB8 or Rgba16Float) skip the f32 target (33 MB of writes per 1080p
 * frame) — for consumers that only ship the packed frame (the multi-GPU gather). BGS_BINNING_SCAN only.
 * bgs_framebuffer_device_ptr / a host copy of such a frame is BGS_EINVAL; bgs_pipeline_pop gives NULL. */
int bgs_set_packed_only(bgs_ctx* ctx, int enabled);
/* The NEXT bgs_render writes its Rgba8UnormSrgb image (width * height * 4 bytes) to this caller-owned
 * device memory instead of the lane's own buffer (one-shot; NULL cancels). Lets a consumer that ships
 * frames in batches (the multi-GPU gather) have each frame land in its slot of the batch with no copy
 * and no extra synchronisation. Implies srgb8 output for that frame; bgs_pipeline_pop /
 * bgs_framebuffer_srgb8_device_ptr then return this pointer for it. */
int bgs_set_srgb8_target(bgs_ctx* ctx, void* device_ptr);
/* Copy `bytes` from device memory this library handed out (a framebuffer, an sRGB8 image, the sorted
 * entries) to host memory, for hosts that do not link the HIP runtime themselves. Blocking. The
 * memory must belong to a COMPLETED frame: after a blocking call, bgs_pipeline_pop or bgs_synchronize. */
int bgs_download(bgs_ctx* ctx, const void* device_ptr, void* host_out, uint64_t bytes);
/* Device memory for what the CALLER hands to the library by device pointer (bgs_view.depth_device_ptr,
 * bgs_set_srgb8_target), for hosts that do not link the HIP runtime themselves: allocate / free on the context's
 * device, and a blocking host-to-device copy. bgs_device_free completes the frames in flight first. */
int bgs_device_alloc(bgs_ctx* ctx, uint64_t bytes, void** device_ptr_out);
int bgs_device_free(bgs_ctx* ctx, void* device_ptr);
int bgs_upload(bgs_ctx* ctx, void* device_ptr, const void* host_in, uint64_t bytes);

/* Frame pipelining. A single stream of this path's kernels is latency bound at 1M splats, so the
 * context can keep up to 8 frames in flight ("lanes", each with its own per-frame buffers, run on a
 * few shared HIP streams, see bgs_set_pipeline_streams): with bgs_set_async(1), successive bgs_render(..., NULL) calls go round-robin
 * over the lanes and overlap on the GPU. A lane's previous frame is completed (stream wait +
 * watchdog check) when the lane is reused. bgs_pipeline_pop completes the OLDEST frame in flight
 * and returns its f32 / sRGB8 framebuffers (valid until that lane is reused, i.e. for depth-1 more
 * enqueues). bgs_framebuffer_device_ptr & co refer to the most recently enqueued frame. */
int bgs_set_pipeline_depth(bgs_ctx* ctx, uint32_t lanes /* 1..8, default 1 */);
int bgs_pipeline_pop(bgs_ctx* ctx, void** rgba_f32_dptr_or_null, void** rgba8_dptr_or_null);
int bgs_frames_in_flight(bgs_ctx* ctx, uint32_t* count);

/* Device pointer of the sorted entries of the last call: after bgs_sort all n entries (culled
 * ones last); after bgs_render only the drawable prefix (*n = entries that reach the vertex
 * stage), because the culled tail is never needed for drawing. */
int bgs_sorted_entries_device_ptr(bgs_ctx* ctx, void** dptr, uint32_t* n);

/* Block until all work queued on the context's stream has finished; in async mode this is also
 * where the last frame's device watchdog word is checked (BGS_EINTERNAL) and its stats collected. */
int bgs_synchronize(bgs_ctx* ctx);
/* Async frames (default off). When on, bgs_render(..., rgba_host_out = NULL) under
 * BGS_BINNING_SCAN only ENQUEUES the frame and returns: that pipeline needs no host round trip
 * (every data-dependent size stays on the device; a frame whose supertile lists or bucket sort outgrow
 * their capacity is re-run on its lane when it is completed, before anyone sees it), so successive
 * frames run back-to-back on the GPU. Any call that needs results (a host copy, bgs_get_stats,
 * bgs_framebuffer_device_ptr, bgs_synchronize, bgs_sort) completes the pending frame first. */
int bgs_set_async(bgs_ctx* ctx, int enabled);
/* The hipStream_t (as void*) the context launches on, so a caller can order its own
 * HIP work (e.g. torch / RCCL) against it. */
int bgs_stream(bgs_ctx* ctx, void** hip_stream);

/* How splats are binned to 16x16 tiles (results are bit-identical between the two):
 *   BGS_BINNING_SCAN (default): ordered coarse (supertile) lists built during projection, each
 *     tile's rasteriser scans its list lazily and stops at saturation; instance_count in the
 *     stats is then the number of coarse list entries.
 *   BGS_BINNING_SORT: materialise every (tile, splat) instance and stable-radix-sort them by
 *     tile id ("tile-major|depth keys"), then per-tile ranges; instance_count = instances. */
#define BGS_BINNING_SCAN 0u
#define BGS_BINNING_SORT 1u
int bgs_set_binning(bgs_ctx* ctx, uint32_t mode);

/* Forget what completed frames taught the context: draw-count hint (grid sizes), drawable key range and
 * the bucket-sort back-off, supertile rule, list-capacity hint. Buffers stay allocated. The next frames
 * behave like the first frames of a fresh context (onesweep passes, default capacities, re-run on
 * overflow). Completes the frames in flight. */
int bgs_reset_adaptive_state(bgs_ctx* ctx);
/* HIP-event timing level: 0 = none, 1 = frame start/end only (total_ms), 2 = every stage
 * (default). Each recorded event costs a few microseconds of GPU timeline. */
int bgs_set_profiling(bgs_ctx* ctx, int enabled);
/* Record the events only on every Nth frame (default 1 = every frame); stage_ms is then the mean
 * over the timed frames since the last read-back. */
int bgs_set_profiling_stride(bgs_ctx* ctx, uint32_t every_nth_frame);
/* Stats of the most recent bgs_sort / bgs_render. Synchronises the stream. */
int bgs_get_stats(bgs_ctx* ctx, bgs_stats* out);

/* Streams the lanes run on: lane i uses stream i % min(streams, depth); 0 = one stream per lane.
 * Default 4: the HIP runtime multiplexes a process's streams onto 4 hardware queues (per priority), and only
 * queues run concurrently, so 4 streams — each on its own queue, the library parks idle streams to get them
 * dealt out that way — is one frame per queue; with more lanes than streams (depth 8 on 4 streams) a stream
 * already holds the next frame of a sibling lane while one executes and never waits for the host.
 * Measured on the headline workload (round 2): 8 lanes on 4 streams 19.0 k frames/s, 4 on 4 18.9 k, 8 on 8
 * 19.0 k, 6 on 3 16.9 k, 6 on 6 17.6 k, and anything that spreads unevenly over the 4 queues loses (8 on 6 16.7 k,
 * 5 on 5 15.6 k). BGS_QUEUE_HOLDERS=0 in the environment keeps the library from parking its idle streams: for
 * processes whose other streams (RCCL's) already hold the queues. */
int bgs_set_pipeline_streams(bgs_ctx* ctx, uint32_t streams);
/* Frame graphs (opt-in, default off). An asynchronous BINNING_SCAN frame (bgs_set_async) in the
 * steady state is replayed from a hipGraph captured once per (lane, parity): the frame's first kernel
 * receives the new view/settings as its arguments (one graph-node update) and leaves them in device
 * memory for the kernels behind it. A kept-order frame (bgs_view.entries_device_ptr) has a graph of its
 * own per (lane, parity), whose first kernel also receives the chunk's address: a lane that draws
 * kept and sorting frames in turn replays both. A replay costs the host ~10 us instead of ~19 us for 7 direct
 * launches, but runs ~5 % slower on the GPU than the same launches issued directly (measured), so it
 * is meant for hosts short of CPU time. The graph is rebuilt when anything else a launch depends on
 * changes (cloud, buffers, viewport size, pipeline variant, grid sizes, debug flags); frames whose
 * stages are timed with events (bgs_set_profiling) are always launched directly. */
int bgs_set_graphs(bgs_ctx* ctx, int enabled);

/* ---- multi-GPU: the gather of finished frames ------------------------------------------------------------------
 * Views are independent units (the reference keys its sort state and entry offsets by camera: src/sort/mod.rs:143-150,
 * src/render/mod.rs:1548-1554): one process per GPU, camera g on rank g, a replica of the cloud on every GPU, no
 * exchange during sort / rasterise. The ONE collective is the gather of finished frames to a root rank: RCCL
 * ncclGather (grouped send / receive over xGMI, every non-root rank on its own link), enqueued on a stream the
 * communicator owns. librccl is opened when the first bgs_comm_* call needs it (hosts that never gather do not need
 * it installed).
 *   rank 0:      bgs_comm_unique_id(id)   -> ship the 128 bytes to every rank by the host's own means (a file, MPI,
 *                                            the launcher's rendezvous)
 *   every rank:  bgs_comm_create(ctx, id, world_size, rank, &comm)      (collective: returns once all ranks called it)
 *   per batch:   bgs_comm_gather(ctx, comm, root, send, bytes, recv, &ticket)   asynchronous; `send` (device memory
 *                holding COMPLETED frames: after bgs_pipeline_pop / bgs_synchronize — e.g. the batch buffer the frames
 *                were written to through bgs_set_srgb8_target) and `recv` (root only: world_size * bytes, rank r's
 *                block at r * bytes) must stay untouched until that gather has completed
 *                bgs_comm_wait(ctx, comm, ticket)  blocks until the gather with that ticket (and every earlier one) has
 *                completed on this rank; ticket 0 = every gather enqueued so far. Double buffering: gather batch k,
 *                render batch k + 1 into the other buffer, wait for ticket k - 1 before reusing its buffer.
 * A communicator belongs to the context's device and, like the context, is driven by one thread. */
#define BGS_COMM_ID_BYTES 128
typedef struct bgs_comm bgs_comm;
int bgs_comm_unique_id(uint8_t id_out[BGS_COMM_ID_BYTES]);
int bgs_comm_create(bgs_ctx* ctx, const uint8_t id[BGS_COMM_ID_BYTES], uint32_t world_size, uint32_t rank, bgs_comm** out);
int bgs_comm_gather(bgs_ctx* ctx, bgs_comm* comm, uint32_t root, const void* send_device_ptr, uint64_t bytes_per_rank,
                    void* recv_device_ptr_root_only, uint64_t* ticket_out_or_null);
/* The same gather ORDERED ON THE DEVICE behind work that is still running (round 6): the communicator's stream first
 * waits — a stream-to-stream dependency, no host round trip — for everything enqueued so far on `hip_stream`, or, with
 * hip_stream == NULL, for every frame this context has enqueued and not yet completed (all lanes). The host may then
 * enqueue the gather of a batch right behind the batch's last bgs_render instead of popping / synchronising its frames
 * first (bgs_comm_gather's contract, a host round trip per batch and rank). What it cannot know: a frame the library
 * re-runs later because a data-dependent capacity turned out too small (bgs_adaptive_counters: reruns_sort, reruns_lists)
 * has been sent in the state of its first attempt — a host that gathers this way checks those counters when it pops the
 * batch's frames (they do not move on a settled view) and gathers the batch again, or uses bgs_comm_gather. */
int bgs_comm_gather_after(bgs_ctx* ctx, bgs_comm* comm, uint32_t root, const void* send_device_ptr, uint64_t bytes_per_rank,
                          void* recv_device_ptr_root_only, void* hip_stream_or_null, uint64_t* ticket_out_or_null);
int bgs_comm_wait(bgs_ctx* ctx, bgs_comm* comm, uint64_t ticket);
int bgs_comm_stream(bgs_ctx* ctx, bgs_comm* comm, void** hip_stream); /* the stream the gathers run on */
void bgs_comm_destroy(bgs_ctx* ctx, bgs_comm* comm);
#ifdef __cplusplus
}
#endif
#endif /* BGS_H */
