/*
 * bgs_diag.h — diagnostics, test hooks and experiment switches of libbgs.
 *
 * NOT part of the drop-in seam (include/bgs.h: context, cloud upload, bgs_sort, bgs_render, targets, frame
 * pipeline). Nothing here is needed to replace the reference's sort + rasterize path; these entry points exist
 * for the parity tests, bench.py's roofline legs and the profiling scripts under scripts/. Same conventions as
 * bgs.h (plain C, negative bgs_status on failure, bgs_last_error).
 */
#ifndef BGS_DIAG_H
#define BGS_DIAG_H

#include "bgs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Debug flags (bgs_set_debug_flags): test hooks and experiment switches. Production code leaves them at 0.
 * Bits 1..64 are kernel-ablation switches for performance experiments (scripts/ablate.py): they switch parts of kernels
 * off and produce WRONG images, and exist only in libraries built with -DBGS_ABLATION=1 (scripts/build_variant.sh); the
 * production library ignores them. Every flag below keeps images correct and exists for A/B timing and tests. */
enum bgs_debug_flag {
    BGS_DEBUG_BUCKETS_NARROW = 0x100,           /* bucket sort with narrow (4096-pair) buckets whatever the list's length
                                                   (default: wide past 1.57 M drawable pairs) */
    BGS_DEBUG_SPLIT_SUB_3 = 0x200,              /* bucket sort with at least 768 buckets whatever the list's length: the finer
                                                   splitter tables, in keygen's arguments */
    BGS_DEBUG_SPLIT_SUB_5 = 0x400,              /* ... at least 1280 buckets: the tables in the lane's device table */
    BGS_DEBUG_BUCKETS_WIDE = 0x800,             /* bucket sort with wide (16 384-pair) buckets whatever the list's length */
    BGS_DEBUG_NO_RASTER_CLEANUP = 0x1000,       /* per-frame memset + Control copy instead of the rasteriser's in-kernel
                                                   clean-up */
    BGS_DEBUG_NO_DRAW_HINT = 0x2000,            /* no draw-count hint for the sort, project and bin grids */
    BGS_DEBUG_NO_GRAPHS = 0x4000,               /* no hipGraph replay even when bgs_set_graphs is on */
    BGS_DEBUG_LEVEL_1 = 0x8000,                 /* force supertile level 1 instead of choosing by the completed frames' list
                                                   statistics */
    BGS_DEBUG_LEVEL_0 = 0x10000,                /* ... level 0 */
    BGS_DEBUG_MIDROUND_ALWAYS = 0x20000,        /* always a mid-round-exit rasteriser, whatever the supertile level and the
                                                   kind's saturation share (the dense frames' at level >= 2, the sparse
                                                   frames' below) */
    BGS_DEBUG_SEPARATE_ENCODE = 0x40000,        /* sRGB8 image from the separate encode pass instead of the rasteriser's
                                                   fused output */
    BGS_DEBUG_NO_BUCKET_SORT = 0x80000,         /* depth sort always by the onesweep digit passes */
    BGS_DEBUG_SMALL_LISTS = 0x100000,           /* supertile lists start at 64 entries (exercises the overflow -> re-run
                                                   path) */
    BGS_DEBUG_GUESSED_SPLITTERS = 0x200000,     /* bucket sort even before a completed frame has told the key range: the
                                                   full 32-bit range guessed */
    BGS_DEBUG_LEVEL_2 = 0x400000,               /* force supertile level 2 */
    BGS_DEBUG_LEVEL_3 = 0x800000,               /* force supertile level 3 */
    BGS_DEBUG_NO_MIDROUND = 0x1000000,          /* never a mid-round-exit rasteriser */
    BGS_DEBUG_NO_STRIPS = 0x2000000,            /* never the heavy-tile strip workgroups (default: pipeline depth 1 only) */
    BGS_DEBUG_STRIPS_ANY_DEPTH = 0x4000000,     /* the heavy-tile strip workgroups at any pipeline depth */
    BGS_DEBUG_RERUN_EVERY_FRAME = 0x8000000,    /* every BINNING_SCAN frame is run twice, as if a data-dependent capacity
                                                   had been too small (exercises the re-run path) */
    BGS_DEBUG_NO_TILE_COST = 0x10000000,        /* no tile-cost feedback / cost-ordered raster workgroups */
    BGS_DEBUG_NO_TILE_COST_PIPELINED = 0x20000000,  /* ... none at pipeline depths > 1 */
    BGS_DEBUG_ORDER_EVERY_FRAME = 0x40000000    /* the cost order is made anew with every frame (default: every 8th) */
};
int bgs_set_debug_flags(bgs_ctx* ctx, uint32_t flags);

/* What the adaptive machinery has done since bgs_create: out[0] frames enqueued on the bucket sort path,
 * [1] on the onesweep passes (both counts include re-runs), [2] frames re-run because the bucket sort gave
 * up, [3] because a supertile list overflowed, [4] because the tile-instance buffer was too small,
 * [5] supertile level changes, [6] the current level, [7] the current list-capacity hint (entries). */
int bgs_adaptive_counters(bgs_ctx* ctx, uint64_t out[8]);

/* The learning phase (bgs.h "Async frames"): how many async frames were completed inside their bgs_render
 * call because the context had not settled on their kind of frame yet, and how many kinds it has settled on. A host
 * whose frames/s fall to the blocking rate sees it here: early_frames grows with every frame. */
int bgs_learning_counters(bgs_ctx* ctx, uint64_t* early_frames, uint64_t* kinds_settled);

/* Stable LSD radix sort of n (key,index) pairs on the device, `passes` 8-bit digit
 * places starting at bit 0 (the Onesweep kernel used for both the depth and the tile
 * sort). entries_inout is a HOST buffer; used by the parity tests to exercise the sort
 * kernel on arbitrary keys (ties, all-equal, ragged sizes). The passes run with the frames' default grid under the
 * context's grid cap (bgs_set_grid_cap); bgs_debug_frame_grids reports it as BGS_GRID_DEPTH, tiles of n. */
int bgs_radix_sort_pairs(bgs_ctx* ctx, bgs_sort_entry* entries_inout, uint32_t n,
                         uint32_t passes);

/* Measured HBM ceiling of this device, for the roofline ("state both" the nominal and
 * the measured peak): `bytes` per buffer (rounded down to 16), `iters` timed repetitions.
 * copy_gbs = hipMemcpyDtoD rate counting read + write; triad_gbs = a[i] = b[i] + s * c[i] with
 * float4 accesses, counting 2 reads + 1 write. Allocates 3 * bytes for the call. */
int bgs_hbm_probe(bgs_ctx* ctx, uint64_t bytes, uint32_t iters, float* copy_gbs, float* triad_gbs);

/* Device self-test of the correctly rounded natural logarithm behind the adaptive cutoff
 * (src/render/gaussian.wgsl:229-235; csrc/exact_log.h: the one transcendental that reaches a cull decision).
 * Evaluates it ON THE DEVICE for the `count` binary32 bit patterns first_bits, first_bits + 1, ...:
 * host_out (may be NULL) receives the results; checksum_out (may be NULL) the wrap-around sum over the inputs of
 * mix((in_bits << 32 | out_bits)) with mix(v) = (v * 0x9E3779B97F4A7C15, v ^= v >> 29, v * 0xBF58476D1CE4E5B9),
 * so that a caller can compare 2^31 results with its own without moving them. */
int bgs_selftest_ln_f32(bgs_ctx* ctx, uint32_t first_bits, uint32_t count, float* host_out, uint64_t* checksum_out);

/* The library parks three idle "queue holder" streams per DEVICE (process-global, created once, however many
 * contexts the process has) before a context creates its own streams, so that the HIP runtime deals those out one per
 * hardware queue (see above). 0 switches that off for contexts that have not created their streams yet — for a
 * process whose other streams already hold the queues (e.g. RCCL's after a process group was initialised); 1 forces
 * it on; -1 (default) follows the environment variable BGS_QUEUE_HOLDERS (unset or non-zero: on). Never fails. */
int bgs_set_queue_holders(int enabled);

/* Diagnostics: per-tile trace of the default (BGS_BINNING_SCAN) rasteriser. With a non-NULL device buffer of
 * tiles_x * tiles_y * 32 bytes, every following frame runs the rasteriser's instrumented instantiation, in which each
 * tile's wave writes 8 uint32: s_memtime at its start (lo, hi) and end (lo, hi), the HW_ID and XCC_ID registers (which
 * XCD / SE / CU / SIMD / wave slot it ran on), the list candidates it scanned, and records blended | staged << 16.
 * scripts/tile_trace.py turns that into the launch's per-SIMD occupancy picture (the "tail"). NULL switches it off.
 * Completes the frames in flight; the buffer stays the caller's. Costs ~10 % of the rasteriser's time while on.
 * There is no traced instantiation with a depth buffer: bgs_render with bgs_view.depth_device_ptr set while a trace
 * buffer is set fails with BGS_EINVAL (it used to run untraced and leave the buffer's old contents). */
int bgs_set_tile_trace(bgs_ctx* ctx, void* device_ptr);

/* How many frames were captured into a graph / replayed from one since bgs_create. */
int bgs_graph_counters(bgs_ctx* ctx, uint64_t* captures, uint64_t* replays);

/* How many frames (re-runs included) left per-tile costs for the frames behind them / drew their raster workgroups in the
 * order made of a completed frame's costs (frames with more tile waves than the chip holds at once) /
 * made that order anew (tile_order_kernel launches). */
int bgs_tile_order_counters(bgs_ctx* ctx, uint64_t* cost_frames, uint64_t* ordered_frames, uint64_t* refreshes);

/* tile_order_kernel on caller-supplied per-tile costs (host_cost[ntiles], u16: work in bits 0-14, bit 15 = the tile ended
 * saturated; 1 <= ntiles <= 65535; runs per XCD 1, 2 or 4): host_order[(ntiles + 3) / 4] receives the raster workgroups'
 * order — a permutation of 0 .. (ntiles + 3) / 4 - 1 whatever the costs hold, heaviest workgroup (its heaviest tile) first
 * inside every XCD's share — and host_sums[2] (may be NULL) the kernel's sums: the work of all tiles, the work of the tiles
 * that ended saturated. Test hook. */
int bgs_selftest_tile_order(bgs_ctx* ctx, const uint16_t* host_cost, uint32_t ntiles, uint32_t runs, uint16_t* host_order,
                            uint32_t* host_sums);

/* The packed outputs' conversion (the one the rasteriser's fused output and the separate encode pass share) on
 * caller-supplied pixels: encode_srgb8_kernel, launched as a frame launches it, reads `pixels` RGBA f32 pixels from
 * device_in_rgba_f32 (16-byte aligned) and writes `pixels` packed texels to device_out: 4 bytes each (BGS_PACK_SRGB8,
 * 4-byte aligned) or 8 (BGS_PACK_RGBA16F, 8-byte aligned). Both buffers are DEVICE memory and stay the caller's, whose
 * writes to the input must be complete; the call returns once the output is written. Test hook. */
enum bgs_pack_format { BGS_PACK_SRGB8 = 1, BGS_PACK_RGBA16F = 2 };
int bgs_selftest_pack(bgs_ctx* ctx, uint32_t format, const void* device_in_rgba_f32, uint32_t pixels, void* device_out);

/* What the vertex stage of lane 0's last completed, synchronous bgs_render left on the device, copied to host memory as
 * it is (tests/test_vertex_stage_gpu.py compares it, record by record, with the host build of csrc/splat_math.h):
 *   info_out       draw_count: the ranks the frame projected (0 after a voided draw list); record_stride: 48 (Record) or
 *                  96 bytes (RecordSurfel, csrc/bgs_device.h); has_rects: 1 for a BGS_BINNING_SCAN frame; visible_count and
 *                  color_max_bits (the bits of the largest |r|, |g|, |b| of the drawn records) as the frame's last run
 *                  left them — after a re-run, the re-run's;
 *   host_records   the first draw_count records, front-to-back rank order (rank j = draw list entry draw_count - 1 - j);
 *                  a rank that is not drawn keeps whatever the buffer held;
 *   host_rects     BGS_BINNING_SCAN frames: the packed tile rectangle x0 | x1 << 8 | y0 << 16 | y1 << 24 of every rank,
 *                  0x000000FF for a rank that is not drawn. Other frames have none and leave it untouched.
 * With host_records and host_rects both NULL only info_out is filled (a caller sizes its buffers with it). Launches no
 * kernel: copies on the lane's stream, then waits for them. BGS_EINVAL, with the reason in bgs_last_error, when no frame
 * has been rendered (or a bgs_sort / bgs_radix_sort_pairs ran since), when frames are in flight or the pipeline depth is
 * not 1, when the last frame was an async one, and when a capacity (bytes / words) is too small. Test hook. */
typedef struct bgs_frame_records_info {
    uint32_t draw_count, record_stride, has_rects, visible_count, color_max_bits;
} bgs_frame_records_info;
int bgs_debug_frame_records(bgs_ctx* ctx, void* host_records, uint64_t records_capacity_bytes, uint32_t* host_rects,
                            uint32_t rects_capacity_words, bgs_frame_records_info* info_out);

/* bin_kernel (the ordered coarse binning of BGS_BINNING_SCAN frames) alone, launched once on caller-supplied packed tile
 * rectangles host_rects[n] (x0 | x1 << 8 | y0 << 16 | y1 << 24, 0x000000FF = touches no tile) for a grid of tiles_x x
 * tiles_y tiles in supertiles of sup_edge x sup_edge: `wide` 0 is the 256-thread instantiation (pipelined frames), 1 the
 * 1024-thread one (pipeline depth 1); `blocks` workgroups (fewer than ceil(n / 1024): each takes several 1024-rank tiles
 * by ticket); lists of coarse_cap entries. Everything the kernel reads or writes is allocated for the call and zeroed —
 * a Control block with draw_count = n, the chain words — except the lists, which are filled with 0xFF bytes together with
 * BGS_SELFTEST_BIN_GUARD entries behind the last list. Returned as they are:
 *   host_lists     (supertiles * coarse_cap + BGS_SELFTEST_BIN_GUARD) entries of two words (rank, packed rectangle), list s
 *                  (supertile sy * sup_x + sx) at entry s * coarse_cap; lists_capacity_words: the words host_lists holds;
 *   host_totals    256 words: Control::coarse_total (entries per list, counted past coarse_cap);
 *   error_out      Control::error (the look-back watchdog; 0).
 * BGS_EINVAL, naming the argument, for what the kernel's own indexing does not allow: 1 <= n <= 2^24, 1 <= tiles_x,
 * tiles_y <= 256, 1 <= sup_edge <= 32 with at most 256 supertiles and 32 per axis, wide 0 / 1, 1 <= blocks <= 4096,
 * coarse_cap >= 1 with supertiles * coarse_cap <= 2^25, and a host_lists that is too small (nothing is written then).
 * Completes the frames in flight. Test hook (tests/test_bin_stage_gpu.py). */
#define BGS_SELFTEST_BIN_GUARD 64u
int bgs_selftest_bin(bgs_ctx* ctx, const uint32_t* host_rects, uint32_t n, uint32_t tiles_x, uint32_t tiles_y, uint32_t sup_edge,
                     uint32_t coarse_cap, uint32_t wide, uint32_t blocks, uint32_t* host_lists, uint64_t lists_capacity_words,
                     uint32_t* host_totals, uint32_t* error_out);

/* What the binning stage of the last completed, synchronous bgs_render left on the device, copied to host memory as it is
 * — at ANY pipeline depth: a synchronous frame runs on lane 0, with the 1024-thread bin_kernel at depth 1 and the
 * 256-thread one at any other. By the frame's binning mode (info_out->binning):
 *   BGS_BINNING_SCAN (0)  sup_edge, sup_x, sup_y, level (the supertile level the frame ran at), coarse_cap (entries per list
 *                  the frame's last run was given), wide_bin; host_totals[sup_x * sup_y]: entries bin_kernel counted per
 *                  supertile list (past coarse_cap where a list overflowed); host_entries: the first min(total, coarse_cap)
 *                  entries (rank, packed tile rectangle: two words) of list 0, then of list 1, ...: entry_count in all;
 *   BGS_BINNING_SORT (1)  instance_count; host_entries: the instance_count tile-sorted instances (tile id ty << 8 | tx, rank);
 *                  host_ranges: the 65 536 [start, end) pairs of the tile ranges, indexed by tile id (131 072 words).
 * draw_count: the ranks the frame projected. With the three host pointers NULL only info_out is filled (a caller sizes its
 * buffers with entry_count). Launches no kernel. BGS_EINVAL, with the reason in bgs_last_error, when no frame has been
 * rendered (or a bgs_sort / bgs_radix_sort_pairs ran since), when frames are in flight, when the last frame was an async
 * one, and when a capacity (words) is too small — nothing is written then. Test hook. */
typedef struct bgs_frame_lists_info {
    uint64_t entry_count;
    uint32_t binning, draw_count;
    uint32_t sup_edge, sup_x, sup_y, level, coarse_cap, wide_bin;
    uint32_t instance_count, reserved;
} bgs_frame_lists_info;
int bgs_debug_frame_lists(bgs_ctx* ctx, uint32_t* host_totals, uint32_t totals_capacity_words, uint32_t* host_entries,
                          uint64_t entries_capacity_words, uint32_t* host_ranges, uint32_t ranges_capacity_words,
                          bgs_frame_lists_info* info_out);

/* bucket_sort_kernel (the default depth sort behind keygen's bucket placement) alone, launched once through the frames' own
 * launcher on caller-supplied bucket contents: nb = 256 * sub buckets; `wide` 0 is the 256-thread instantiation on slot
 * regions of 4096 pairs, 1 the 1024-thread one on regions of 16 384; key_xor is XOR-ed into every key on output.
 *   host_counts    nb words: what Control::bucket_count holds. A count may exceed the region's capacity `cap`;
 *   host_pairs     the pairs (key, index: two words), bucket after bucket, min(count, cap) of each, in the arrival order the
 *                  caller wants; pair_count = their number n. The hook puts each bucket's pairs at the start of its slot
 *                  region and fills the rest of every region with 0xFF bytes.
 * Everything the kernel reads or writes is allocated for the call: a zeroed Control block with the counts, the regions,
 * and an output list of n + BGS_SELFTEST_BUCKET_GUARD entries filled with 0xFF bytes. Returned as they are:
 *   host_out       (n + BGS_SELFTEST_BUCKET_GUARD) entries of two words (key ^ key_xor, index); out_capacity_words: the
 *                  words host_out holds;
 *   info_out       3 words: Control::draw_count, Control::sort_overflow (bit 0: a count over the capacity, bit 1: more than
 *                  BUCKET_FINE_MAX = 1024 pairs in one fine range of a bucket), Control::bucket_max.
 * BGS_EINVAL, naming the argument, for what the kernel's own indexing does not allow: 1 <= sub <= 16, wide 0 / 1, the
 * pointers non-NULL, pair_count = the sum of min(count, cap), and a host_out that is too small (nothing is launched then).
 * Completes the frames in flight. Test hook (tests/test_bucket_stage_gpu.py). */
#define BGS_SELFTEST_BUCKET_GUARD 64u
int bgs_selftest_bucket_sort(bgs_ctx* ctx, uint32_t sub, uint32_t wide, uint32_t key_xor, const uint32_t* host_counts,
                             const uint32_t* host_pairs, uint32_t pair_count, uint32_t* host_out, uint64_t out_capacity_words,
                             uint32_t* info_out);

/* keygen's bucket placement alone: keygen_kernel, launched once through the frames' own KeygenLaunch on a resident cloud
 * with a caller-supplied splitter table host_splitters[256 * sub - 1] — keygen's key space, the one a completed frame's
 * quantile keys are in (sorted key ^ 0xFFFFFFFF for BGS_SORT_RAYON / BGS_SORT_STD), non-strictly ascending. As in a frame,
 * a table of sub <= 3 travels in the kernel arguments and a longer one is copied to a device table first.
 *   wide_buckets   slot regions of 16 384 pairs instead of 4096 (cap);
 *   ordered        0: the chainless instantiation of rendered frames; 1: bgs_sort's, with the tile chain and the culled tail;
 *   alone          KeygenLaunch::wide, what a frame at pipeline depth 1 sets: 4096-splat tiles (clouds of 2^19 splats or
 *                  more) run as 1024 threads x 4 instead of 256 x 16.
 * Everything the kernel writes is allocated for the call: a zeroed Control block, zeroed chain words, and the slot regions
 * and the culled list filled with 0xFF bytes. Returned as they are:
 *   host_counts    256 * sub words: Control::bucket_count (counted past cap where a bucket overflows);
 *   host_slots     256 * sub regions of cap entries of two words (key, index); slots_capacity_words: the words it holds;
 *   host_culled    ordered = 1 only (else it may be NULL): bgs_cloud_len entries of two words, the culled splats (key = the
 *                  culled sentinel) in index order, then the fill; culled_capacity_words: the words it holds;
 *   info_out       5 words: Control::draw_count, Control::splat_count and Control::error (the look-back watchdog) — the
 *                  words keygen publishes; the chainless instantiation leaves draw_count to bucket_sort_kernel and
 *                  publishes splat_count only —, then the launch's threads per workgroup and its workgroups (the frames' default grid under the
 *                  context's grid cap, bgs_set_grid_cap, with ordered = 1; one workgroup per tile with ordered = 0).
 * BGS_EINVAL, naming the argument: NULL pointers, an empty cloud, sub outside 1 .. 16, a flag that is not 0 / 1, settings
 * bgs_sort would refuse (sort_mode, radix_depth_bits), a table that descends somewhere, a capacity that is too small
 * (nothing is launched then). Completes the frames in flight. Test hook (tests/test_bucket_stage_gpu.py). */
int bgs_selftest_keygen_buckets(bgs_ctx* ctx, const bgs_cloud* cloud, const bgs_view* view, const bgs_settings* settings,
                                const uint32_t* host_splitters, uint32_t sub, uint32_t wide_buckets, uint32_t ordered,
                                uint32_t alone, uint32_t* host_counts, uint32_t* host_slots, uint64_t slots_capacity_words,
                                uint32_t* host_culled, uint64_t culled_capacity_words, uint32_t* info_out);

/* The two tile rasterisers alone, launched once each through the frames' own launchers (launch_raster_scan: raster_scan_kernel
 * / raster_tile; launch_raster: raster_kernel) on caller-supplied stage inputs — what the vertex and binning stages leave:
 *   width, height      the target, 1 .. 512 px each; tiles of 16 x 16 px, supertiles of sup_edge x sup_edge tiles (at most 256
 *                      of them, 32 per axis);
 *   sample_count       1, 2, 4 or 8; variant 0 OBB, 1 AABB3D, 2 surfel; overlay 0 / 1 (the bounding-box overlay);
 *   mode               raster_scan_kernel's MODE: 0 plain, 1 dense + mid-round exit, 2 sparse + mid-round exit. Refused when
 *                      no such instantiation is built for the variant, samples and overlay (RasterInst::exists, csrc/frame_params.h);
 *   viewport_w / _h    FrameParams::viewport_w / _h (the surfel variant's aspect); clear[4]; color_max_bits: what
 *                      Control::color_max_bits holds (the bits of the frame's largest colour magnitude: the cut-off);
 *   records            record_count records of 48 bytes (OBB, AABB3D: Record) or 96 (surfel: RecordSurfel), csrc/bgs_device.h;
 *   lists, totals      the supertile lists: supertiles x coarse_cap entries of two words (rank, packed rectangle x0 | x1 << 8 |
 *                      y0 << 16 | y1 << 24), list s at entry s * coarse_cap, and totals[supertiles] (Control::coarse_total; a
 *                      total may exceed coarse_cap: the kernel reads min(total, coarse_cap) entries);
 *   depth              NULL, or width * height * sample_count floats ([y][x][sample], reverse-Z; FrameParams::depth_ptr);
 *   heavy_tiles        NULL, or heavy_count (<= 256) distinct tile ids (ty * tiles_x + tx) the strip workgroups draw; modes 1 and
 *                      2 only. The hook builds the HeavyFeedback buffer (count, list, flag per tile) the launch reads;
 *   order              NULL, or the raster workgroups' order: a permutation of 0 .. (tiles + 3) / 4 - 1.
 * The instance-sort rasteriser's instances and tile ranges are derived on the host from the same lists: for each tile the
 * entries of its supertile's list, in list order, whose rectangle holds the tile. FrameCleanup is all-null, there is no
 * trace buffer, and only the f32 target is written. Everything the kernels read or write is allocated for the call.
 *   host_scan, host_sort   (width * height + BGS_SELFTEST_RASTER_GUARD) RGBA f32 pixels each: the image, then the guard;
 *                      both buffers are filled with 0xFF bytes before the launch; image_capacity_floats: what each holds;
 *   host_cost          tiles words (u16): the scan rasteriser's cost_out, filled with 0xFF bytes before the launch;
 *   host_heavy         128 + 512 + tiles bytes: the heavy_out buffer (zeroed before the launch; modes 1 and 2 write it);
 *   error_out          Control::error.
 * BGS_EINVAL, naming the argument, and nothing launched: a size, count or flag outside the above; a rank >= record_count in a
 * list position below min(total, coarse_cap); a tile id >= tiles or twice in heavy_tiles; an order that is no permutation;
 * more than 2^24 tile instances; a capacity that is too small. Nothing the caller passes can then index outside an
 * allocation. Completes the frames in flight. Test hook (tests/test_raster_stage_gpu.py). */
#define BGS_SELFTEST_RASTER_GUARD 64u
typedef struct bgs_raster_selftest {
    uint32_t width, height, sample_count, variant, overlay, mode;
    uint32_t sup_edge, coarse_cap, color_max_bits, record_count, heavy_count, reserved;
    float viewport_w, viewport_h, clear[4];
    const void* records;
    const uint32_t* lists;
    const uint32_t* totals;
    const float* depth;
    const uint16_t* heavy_tiles;
    const uint16_t* order;
} bgs_raster_selftest;
int bgs_selftest_raster(bgs_ctx* ctx, const bgs_raster_selftest* in, float* host_scan, float* host_sort,
                        uint64_t image_capacity_floats, uint16_t* host_cost, uint8_t* host_heavy, uint64_t heavy_capacity_bytes,
                        uint32_t* error_out);

/* What lane 0's last completed bgs_render left for the frame behind it, copied to host memory as it is — at ANY pipeline
 * depth (tests/test_frame_leftovers_gpu.py). A BGS_BINNING_SCAN frame whose plan has raster_cleans set takes neither a memset
 * of the lane's scratch region nor a copy of its Control block: its rasteriser zeroes the chain words the frame used and the
 * lane's OTHER Control block, and writes the pinned host Control; the lane's next frame is launched on the strength of
 * Lane::scratch_clean alone. Returned:
 *   host_scratch   the lane's whole scratch region (layout_out->bytes bytes): [Control 0 | depth status | scan status | tile
 *                  status | ranges | bin status | partition status | Control 1], the parts at layout_out's offsets;
 *   layout_out     the layout the region was made with (csrc/frame_params.h ScratchLayout, field by field);
 *   host_control   the lane's pinned host Control (info_out->control_bytes bytes) as the frame's completion left it: written by
 *                  the frame's rasteriser (raster_cleans) or by the copy behind the frame;
 *   info_out       ctl_block: which of the two Control blocks the frame used (0: at offset 0, 1: at layout_out->off_ctl1; the
 *                  lane's parity before the flip); scratch_clean as the lane held it when the hook was called; the plan's
 *                  raster_cleans, bucket, places, large (4096-pair onesweep tiles), wide, wide_bin, kept, bucket_sub and
 *                  split_sub_out; culled_tail (keygen or the compaction wrote the culled tail: a bucket frame's keygen has a chain only then);
 *                  keygen_tile: splats per tile of the frame's keygen (2048 for a kept order's compaction); n; ntiles and raster_mode (the
 *                  rasteriser's grid is ceil(ntiles / 4) workgroups, plus 256 strip workgroups when strips_appended);
 *                  graph_replay: 1 when the frame was a replay of a captured graph; binning (0 scan, 1 sort);
 *                  dirty_words: how many 32-bit words of the region OUTSIDE the frame's own Control block are not zero.
 * If dirty_words != 0 while the lane's scratch_clean is true, the hook sets scratch_clean to false before it returns (and
 * reports scratch_reset = 1): the lane's next frame then takes the memset path, so that words a clean-up missed never reach
 * the chained scans of a later frame — a failed check costs a test, not a machine. info_out->scratch_clean is the value
 * before that.
 * With host_scratch and host_control both NULL only layout_out and info_out are filled (a caller sizes its buffers with them).
 * Launches no kernel: copies on the lane's stream, then waits for them. BGS_EINVAL, with the reason in bgs_last_error, when
 * no frame has been rendered (or a bgs_sort / bgs_radix_sort_pairs ran since), when frames are in flight, when the last frame
 * was an async one at a pipeline depth other than 1 (at depth 1 a completed async frame — the only kind a captured graph
 * replays — ran on lane 0 and is read like a synchronous one), and when a capacity (bytes) is too small — nothing is written
 * to the host buffers then. Test hook. */
typedef struct bgs_scratch_layout {
    uint64_t bytes;
    uint64_t off_depth_status, off_scan_status, off_tile_status, off_ranges, off_bin_status, off_part_status, off_ctl1;
    uint64_t depth_tiles, inst_tiles, inst_cap;
    uint32_t n, pass_stride;
} bgs_scratch_layout;
typedef struct bgs_frame_leftovers_info {
    uint64_t dirty_words;
    uint32_t ctl_block, scratch_clean, scratch_reset, raster_cleans;
    uint32_t bucket, places, large, wide, wide_bin, kept, bucket_sub, split_sub_out;
    uint32_t keygen_tile, n, ntiles, raster_mode, strips_appended, graph_replay, binning, control_bytes;
    uint32_t culled_tail, reserved;
} bgs_frame_leftovers_info;
int bgs_debug_frame_leftovers(bgs_ctx* ctx, void* host_scratch, uint64_t scratch_capacity_bytes, void* host_control,
                              uint32_t control_capacity_bytes, bgs_scratch_layout* layout_out, bgs_frame_leftovers_info* info_out);

/* A cap on the grid of every PERSISTENT launch of the context: the kernels whose workgroups take tiles of work by ticket
 * (or by stride) until none is left. Their default grids (num_cus * 4 or * 3 workgroups, or what the draw-count hint asks
 * for) cover every tile of a frame of a few thousand splats, so that each workgroup takes exactly one tile and never goes
 * round its loop a second time; under a cap of a few workgroups the same small frame walks every loop several times
 * (tests/test_grid_cap_gpu.py). blocks: 0 = off, the default; 1 .. BGS_GRID_CAP_MAX = every persistent launch uses
 * min(its own grid, blocks) workgroups; anything else is BGS_EINVAL. Capped:
 *   keygen_kernel        the ordered instantiations (the onesweep path's, and the bucket path's with the culled tail:
 *                        bgs_sort). The CHAINLESS bucket keygen of rendered frames keeps one workgroup per tile: its tiles
 *                        depend on nobody, its grid is not capped by design and it has no ticket loop to walk;
 *   onesweep_kernel      the depth passes and BGS_BINNING_SORT's two tile-id passes;
 *   project_kernel, bin_kernel (BGS_BINNING_SCAN), project_emit_kernel (BGS_BINNING_SORT);
 *   the kept-order compaction (entries_compact_kernel);
 *   the hooks bgs_radix_sort_pairs and bgs_selftest_keygen_buckets, which launch with the frames' default grid.
 * Not capped: the kernels whose grid IS their data — bucket_sort_kernel (workgroup = bucket), the rasterisers (workgroup =
 * four tiles), tile_order_kernel, the pack and encode kernels, the small libraries.
 * Why a capped grid cannot deadlock the chained scans: a tile is handed out by an atomic ticket, in tile order, to a
 * workgroup that is already running; so when a workgroup waits for the chain word of a predecessor tile, that tile has
 * been taken before its own, by a workgroup that is running (or has finished) and that waits, in turn, only for tiles
 * taken earlier still. The tile with the lowest unfinished ticket waits for nobody. With a cap of 1 the one workgroup
 * walks the tiles in order and every predecessor is complete. (project_kernel strides and has no chain.)
 * The cap travels with the frame like the debug flags: it is snapshotted when the frame is enqueued, a re-run of the frame
 * uses the grids it was enqueued with, and since the grids are part of what a captured frame graph is keyed on, a frame
 * under another cap is captured anew, never replayed with the old grids. Test hook. */
#define BGS_GRID_CAP_MAX 4096u
int bgs_set_grid_cap(bgs_ctx* ctx, uint32_t blocks);

/* What the persistent kernels of the most recently enqueued frame (bgs_sort or bgs_render; of a re-run, the re-run) launched,
 * once the frame is complete — or of a bgs_radix_sort_pairs / bgs_selftest_keygen_buckets since (whichever launched last). out[2 k] = workgroups launched, out[2 k + 1] = tiles of
 * work, for kernel k (both 0 for a kernel the frame did not launch):
 *   BGS_GRID_FRONT      keygen_kernel or the kept-order compaction: tiles of bgs_cloud_len splats;
 *   BGS_GRID_DEPTH      the onesweep depth passes (each pass has this grid): tiles of the frame's draw_count;
 *   BGS_GRID_PROJECT    project_kernel / project_emit_kernel: 256-rank tiles of draw_count;
 *   BGS_GRID_BIN        bin_kernel: 1024-rank tiles of draw_count;
 *   BGS_GRID_TILE_SORT  BGS_BINNING_SORT's tile-id passes: tiles of instance_count.
 * The tiles are computed on the host from the kernel's tile size and from the count the kernel read: the cloud's length, or
 * the completed frame's Control copy for the counts only the device knew. out[10] = the grid cap the launches ran under,
 * out[11] = 1 when the front kernel was the chainless keygen (never capped); out[12], out[13] = the low and high word of the
 * DEVICE address of the list the front kernel left behind the draw list — keygen's culled entries in index order, the
 * compaction's skipped entries in list order with their parked index — and out[14] = its entries (bgs_cloud_len - draw_count),
 * all 0 for a frame that wrote none (a render outside BGS_RASTERIZE_DEPTH, a hook); out[15] = 0. The list is the lane's
 * and is valid until the context's next call that runs kernels (read it with bgs_download). capacity: the words out holds, at least
 * BGS_FRAME_GRIDS_WORDS. BGS_EINVAL when nothing has run or frames are in flight. Launches nothing. Test hook: a test of a
 * loop's second trip asserts blocks < tiles before it compares anything. */
enum bgs_grid_kernel { BGS_GRID_FRONT = 0, BGS_GRID_DEPTH = 1, BGS_GRID_PROJECT = 2, BGS_GRID_BIN = 3, BGS_GRID_TILE_SORT = 4 };
#define BGS_FRAME_GRIDS_WORDS 16u
int bgs_debug_frame_grids(bgs_ctx* ctx, uint32_t* out, uint32_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* BGS_DIAG_H */
