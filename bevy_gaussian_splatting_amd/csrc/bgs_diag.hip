// bgs_diag.hip — libbgs: the test hooks and probes of include/bgs_diag.h that touch the device. Those that launch kernels
// of their own (the digit passes on caller-supplied pairs, the HBM probe, the device self-tests) issue their commands
// through one checked stream (command_stream.h); the read-backs of the last frame (bgs_debug_frame_records / _lists /
// _leftovers / _grids) launch nothing and share one guard, last_frame below. Counters and switches stay with the context
// (bgs_api.hip / bgs_frame.hip).
#include "bgs_context.h"
#include "command_stream.h"

namespace {

int refuse_in_flight(bgs_ctx* ctx, const std::string& hook) {
    for (const Lane& lane : ctx->lanes)
        if (lane.pending) return fail(ctx, BGS_EINVAL, hook + ": frames are in flight");
    return BGS_OK;
}

// What the read-backs of the last frame refuse in common, under the hook's name, in this order: a pipeline depth other than
// 1 (LF_DEPTH_1), frames in flight, a lane (lane 0, or with LF_RECENT the one the last frame ran on) that holds no rendered
// frame — or no scratch region, LF_SCRATCH —, and an async frame: always (LF_NO_ASYNC), or at a depth other than 1
// (LF_NO_ASYNC_RING). Between the second and the third it sets the device and completes what finish_all completes.
enum : uint32_t { LF_RECENT = 1u, LF_DEPTH_1 = 2u, LF_NO_ASYNC = 4u, LF_NO_ASYNC_RING = 8u, LF_SCRATCH = 16u };
int last_frame(bgs_ctx* ctx, const std::string& hook, uint32_t flags, Lane** lane_out) {
    if ((flags & LF_DEPTH_1) && ctx->depth != 1) return fail(ctx, BGS_EINVAL, hook + ": the pipeline depth must be 1");
    int rc = refuse_in_flight(ctx, hook);
    if (rc != BGS_OK || (rc = enter_drained(ctx)) != BGS_OK) return rc;
    Lane& L = ctx->lanes[(flags & LF_RECENT) ? ctx->recent : 0];
    if (!L.has_result || !L.plan.render || !L.last_ctl || !L.stream || ((flags & LF_SCRATCH) && !L.scratch.ptr))
        return fail(ctx, BGS_EINVAL, hook + ": no frame has been rendered (or a bgs_sort / bgs_radix_sort_pairs ran since)");
    if (L.in.allow_graph && (flags & LF_NO_ASYNC)) return fail(ctx, BGS_EINVAL, hook + ": the last frame was an async frame");
    if (L.in.allow_graph && (flags & LF_NO_ASYNC_RING) && ctx->depth != 1)
        return fail(ctx, BGS_EINVAL, hook + ": the last frame was an async frame at a pipeline depth other than 1");
    *lane_out = &L;
    return BGS_OK;
}

}  // namespace

extern "C" {

int bgs_radix_sort_pairs(bgs_ctx* ctx, bgs_sort_entry* entries, uint32_t n, uint32_t passes) {
    if (!ctx) return fail(nullptr, BGS_EINVAL, "ctx is NULL");
    if (passes < 1 || passes > 4) return fail(ctx, BGS_EINVAL, "passes must be 1..4");
    if (n > MAX_SPLATS) return fail(ctx, BGS_EINVAL, "too many pairs");
    int rc = enter_drained(ctx);
    if (rc != BGS_OK) return rc;
    if (n == 0) return BGS_OK;
    if (!entries) return fail(ctx, BGS_EINVAL, "entries is NULL");
    Lane& L = ctx->lanes[0];
    L.last_ctl = nullptr;   // (the last frame's Control block and tile rectangles go: bgs_debug_frame_records)
    if ((rc = ensure_entries(ctx, L, n)) != BGS_OK) return rc;
    if ((rc = ensure_scratch(ctx, L, n, L.inst[0].capacity)) != BGS_OK) return rc;
    hipStream_t st = L.stream;
    Control* ctl = (Control*)L.scratch.ptr;
    uint32_t* depth_status = (uint32_t*)(L.scratch.ptr + L.layout.off_depth_status);
    HIP_TRY(ctx, hipMemsetAsync(L.scratch.ptr, 0, L.layout.bytes, st));
    L.scratch_clean = false;
    HIP_TRY(ctx, hipMemcpyAsync(L.entries[0].ptr, entries, (size_t)n * sizeof(uint2), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)&ctl->splat_count, (int)n, 1, st));
    launch_histogram(st, L.entries[0].ptr, n, &ctl->hist_depth[0][0], passes);
    OnesweepLaunch sort;
    sort.lists[0] = L.entries[0].ptr; sort.lists[1] = L.entries[1].ptr;
    sort.n_ptr = &ctl->splat_count; sort.max_n = n;
    sort.hist = ctl->hist_depth; sort.status = depth_status; sort.status_stride = L.layout.pass_stride;
    sort.ctl = ctl; sort.first_ticket = TICKET_DEPTH; sort.passes = passes; sort.large_tiles = n > (4u << 20);
    // the frames' default grid, under the context's grid cap (bgs_set_grid_cap); what was launched: bgs_debug_frame_grids
    sort.prepare(grid_under_cap(ctx->num_cus * 4, ctx->grid_cap));
    Lane::Grids& g = L.grids = Lane::Grids(++ctx->grid_stamps, n, ctx->grid_cap);
    g.launched(g.DEPTH, sort);
    g.count[g.DEPTH] = g.HOST_N;
    sort.launch(st);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(entries, L.entries[passes & 1u].ptr, (size_t)n * sizeof(uint2), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(L.h_ctl.ptr, ctl, sizeof(Control), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (L.h_ctl.ptr->error) return fail(ctx, BGS_EINTERNAL, "device watchdog tripped in radix sort");
    return BGS_OK;
}

int bgs_hbm_probe(bgs_ctx* ctx, uint64_t bytes, uint32_t iters, float* copy_gbs, float* triad_gbs) {
    if (!ctx) return fail(nullptr, BGS_EINVAL, "ctx is NULL");
    bytes &= ~(uint64_t)15;
    if (bytes < 4096 || iters == 0 || iters > 10000) return fail(ctx, BGS_EINVAL, "bytes >= 4096 and 1 <= iters <= 10000");
    if (int rc = enter_drained(ctx); rc != BGS_OK) return rc;
    DeviceBuffer<char> probe;
    if (!probe.reserve((size_t)bytes * 3)) return fail(ctx, BGS_ENOMEM, "hipMalloc(probe buffers) failed");
    char* const buf = probe.ptr;
    hipStream_t st = ctx->lanes[0].stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms_copy = 0.0f, ms_triad = 0.0f;
    float4 *a = (float4*)buf, *b = (float4*)(buf + bytes), *c = (float4*)(buf + 2 * bytes);
    const size_t n4 = (size_t)bytes / 16;
    const int blocks = ctx->num_cus * 16;
    CommandStream cs(st);   // the set-up only: the two timed sections are a measurement and issue their commands themselves
    cs.check(hipEventCreate(&e0));
    if (cs.ok) cs.check(hipEventCreate(&e1));
    bool ok = cs.zero(buf, (size_t)bytes * 3);
    if (ok) {  // warm-up, then `iters` back-to-back repetitions between two events
        ok = hipMemcpyAsync(a, b, bytes, hipMemcpyDeviceToDevice, st) == hipSuccess;
        ok = ok && hipEventRecord(e0, st) == hipSuccess;
        for (uint32_t i = 0; ok && i < iters; ++i)
            ok = hipMemcpyAsync(a, b, bytes, hipMemcpyDeviceToDevice, st) == hipSuccess;
        ok = ok && hipEventRecord(e1, st) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
             hipEventElapsedTime(&ms_copy, e0, e1) == hipSuccess;
    }
    if (ok) {
        launch_triad(st, a, b, c, 0.5f, n4, blocks);
        ok = hipEventRecord(e0, st) == hipSuccess;
        for (uint32_t i = 0; ok && i < iters; ++i) launch_triad(st, a, b, c, 0.5f, n4, blocks);
        ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(e1, st) == hipSuccess &&
             hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms_triad, e0, e1) == hipSuccess;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (!ok) { (void)hipGetLastError(); return fail(ctx, BGS_EHIP, "HBM probe failed"); }
    if (copy_gbs) *copy_gbs = ms_copy > 0.0f ? (float)(2.0 * (double)bytes * iters / (ms_copy * 1e6)) : 0.0f;
    if (triad_gbs) *triad_gbs = ms_triad > 0.0f ? (float)(3.0 * (double)bytes * iters / (ms_triad * 1e6)) : 0.0f;
    return BGS_OK;
}

int bgs_selftest_ln_f32(bgs_ctx* ctx, uint32_t first_bits, uint32_t count, float* host_out, uint64_t* checksum_out) {
    if (!ctx) return fail(nullptr, BGS_EINVAL, "ctx is NULL");
    if (count == 0 || (!host_out && !checksum_out)) return fail(ctx, BGS_EINVAL, "count >= 1 and one of host_out / checksum_out");
    if (int rc = enter_drained(ctx); rc != BGS_OK) return rc;
    DeviceBuffer<unsigned long long> sum_buf;
    DeviceBuffer<float> out_buf;
    if (!sum_buf.reserve(1)) return fail(ctx, BGS_ENOMEM, "hipMalloc(selftest) failed");
    if (host_out && !out_buf.reserve(count)) return fail(ctx, BGS_ENOMEM, "hipMalloc(selftest output) failed");
    unsigned long long* const d_sum = sum_buf.ptr;
    float* const d_out = out_buf.ptr;   // (null without host_out)
    hipStream_t st = ctx->lanes[0].stream;
    unsigned long long sum = 0;
    CommandStream cs(st);
    cs.zero(d_sum, sizeof sum);
    if (cs.ok) launch_selftest_ln(st, first_bits, count, d_out, d_sum, ctx->num_cus * 8);
    cs.launched();
    cs.down(&sum, d_sum, sizeof sum);
    if (host_out) cs.down(host_out, d_out, (size_t)count * sizeof(float));
    cs.sync();
    if (!cs.ok) return fail(ctx, BGS_EHIP, "ln self-test failed on the device");
    if (checksum_out) *checksum_out = (uint64_t)sum;
    return BGS_OK;
}

int bgs_selftest_pack(bgs_ctx* ctx, uint32_t format, const void* device_in_rgba_f32, uint32_t pixels, void* device_out) {
    if (!ctx) return fail(nullptr, BGS_EINVAL, "ctx is NULL");
    if (format != BGS_PACK_SRGB8 && format != BGS_PACK_RGBA16F)
        return fail(ctx, BGS_EINVAL, "pack self-test: format must be BGS_PACK_SRGB8 or BGS_PACK_RGBA16F");
    if (pixels == 0 || !device_in_rgba_f32 || !device_out)
        return fail(ctx, BGS_EINVAL, "pack self-test: pixels >= 1 and both device buffers");
    const size_t out_align = format == BGS_PACK_RGBA16F ? 8u : 4u;
    if ((reinterpret_cast<uintptr_t>(device_in_rgba_f32) & 15u) || (reinterpret_cast<uintptr_t>(device_out) & (out_align - 1u)))
        return fail(ctx, BGS_EINVAL, "pack self-test: the input must be 16-byte aligned, the output 4- (sRGB8) or 8-byte "
                                     "(Rgba16Float) aligned");
    if (int rc = enter_drained(ctx); rc != BGS_OK) return rc;
    // encode_srgb8_kernel takes its destination from FrameParams::srgb8_target: a zeroed one sends it to device_out
    DeviceBuffer<FrameParams> fp_buf;
    if (!fp_buf.reserve(1)) return fail(ctx, BGS_ENOMEM, "hipMalloc(pack self-test) failed");
    FrameParams* const d_fp = fp_buf.ptr;
    hipStream_t st = ctx->lanes[0].stream;
    CommandStream cs(st);
    cs.zero(d_fp, sizeof(FrameParams));
    if (cs.ok)
        launch_encode_srgb8(st, static_cast<const float4*>(device_in_rgba_f32), static_cast<uint32_t*>(device_out), pixels,
                            d_fp, format == BGS_PACK_RGBA16F ? OUT_RGBA16F : OUT_SRGB8);
    cs.launched();
    cs.sync();
    if (!cs.ok) return fail(ctx, BGS_EHIP, "pack self-test failed on the device");
    return BGS_OK;
}

int bgs_selftest_tile_order(bgs_ctx* ctx, const uint16_t* host_cost, uint32_t ntiles, uint32_t runs, uint16_t* host_order, uint32_t* host_sums) {
    if (!ctx) return fail(nullptr, BGS_EINVAL, "ctx is NULL");
    if (!host_cost || !host_order || ntiles == 0 || ntiles > 65535u || (runs != 1u && runs != 2u && runs != 4u))
        return fail(ctx, BGS_EINVAL, "tile-order self-test: 1 <= ntiles <= 65535, runs 1 / 2 / 4, both host buffers");
    if (int rc = enter_drained(ctx); rc != BGS_OK) return rc;
    const uint32_t nblocks = (ntiles + 3u) / 4u;
    DeviceBuffer<uint16_t> cost_buf, order_buf;
    cost_buf.reserve(tile_cost_bytes(ntiles) / 2u);
    order_buf.reserve(tile_order_bytes(ntiles) / 2u);
    uint16_t* const d_cost = cost_buf.ptr;
    uint16_t* const d_order = order_buf.ptr;
    uint32_t pairs[16];
    CommandStream cs(ctx->lanes[0].stream);
    cs.ok = d_cost && d_order;   // (no memory: the hook's one refusal)
    cs.fill(d_order, 0xFF, tile_order_bytes(ntiles));
    cs.up(d_cost, host_cost, (size_t)ntiles * 2u);
    if (cs.ok) launch_tile_order_runs(cs.st, d_cost, d_order, ntiles, runs);
    cs.launched();
    cs.down(host_order, d_order, (size_t)nblocks * 2u);
    cs.down(pairs, reinterpret_cast<const uint8_t*>(d_order) + tile_order_stats_offset(ntiles), sizeof pairs);
    cs.sync();
    if (!cs.ok) return fail(ctx, BGS_EHIP, "tile-order self-test failed on the device");
    if (host_sums) {
        host_sums[0] = host_sums[1] = 0u;
        for (uint32_t x = 0; x < 8u; ++x) { host_sums[0] += pairs[2u * x]; host_sums[1] += pairs[2u * x + 1u]; }
    }
    return BGS_OK;
}

// bin_kernel alone, on the caller's rectangles: a zeroed Control of its own (draw_count = n), zeroed chain words, and the
// lists plus BGS_SELFTEST_BIN_GUARD entries filled with 0xFF bytes, all of which go back to the caller. What is refused is
// what the kernel's own indexing rests on (render_kernels.hip: 32-entry mask rows, 256 chain threads, 8-bit tile
// coordinates); the rectangles themselves may hold anything: a coordinate past the grid matches no column / row mask.
int bgs_selftest_bin(bgs_ctx* ctx, const uint32_t* host_rects, uint32_t n, uint32_t tiles_x, uint32_t tiles_y, uint32_t sup_edge,
                     uint32_t coarse_cap, uint32_t wide, uint32_t blocks, uint32_t* host_lists, uint64_t lists_capacity_words,
                     uint32_t* host_totals, uint32_t* error_out) {
    if (!ctx) return fail(nullptr, BGS_EINVAL, "ctx is NULL");
    if (!host_rects || !host_lists || !host_totals || !error_out)
        return fail(ctx, BGS_EINVAL, "bin self-test: host_rects, host_lists, host_totals and error_out must be non-NULL");
    if (n < 1u || n > (1u << 24)) return fail(ctx, BGS_EINVAL, "bin self-test: n must be 1 .. 2^24, got " + std::to_string(n));
    if (tiles_x < 1u || tiles_x > 256u) return fail(ctx, BGS_EINVAL, "bin self-test: tiles_x must be 1 .. 256, got " + std::to_string(tiles_x));
    if (tiles_y < 1u || tiles_y > 256u) return fail(ctx, BGS_EINVAL, "bin self-test: tiles_y must be 1 .. 256, got " + std::to_string(tiles_y));
    if (sup_edge < 1u || sup_edge > 32u) return fail(ctx, BGS_EINVAL, "bin self-test: sup_edge must be 1 .. 32, got " + std::to_string(sup_edge));
    if (!supertile_bins_fit(tiles_x, tiles_y, sup_edge))
        return fail(ctx, BGS_EINVAL, "bin self-test: sup_edge " + std::to_string(sup_edge) + " gives more than " + std::to_string(MAX_SUPERTILES) +
                                         " supertiles, or more than " + std::to_string(MAX_SUPERTILES_PER_AXIS) + " on an axis");
    if (wide > 1u) return fail(ctx, BGS_EINVAL, "bin self-test: wide must be 0 or 1, got " + std::to_string(wide));
    if (blocks < 1u || blocks > 4096u) return fail(ctx, BGS_EINVAL, "bin self-test: blocks must be 1 .. 4096, got " + std::to_string(blocks));
    const uint32_t sup_x = (tiles_x + sup_edge - 1u) / sup_edge, sup_y = (tiles_y + sup_edge - 1u) / sup_edge, num_st = sup_x * sup_y;
    if (coarse_cap < 1u || (uint64_t)num_st * coarse_cap > (1ull << 25))
        return fail(ctx, BGS_EINVAL, "bin self-test: coarse_cap must be >= 1 and supertiles x coarse_cap <= 2^25, got " + std::to_string(coarse_cap));
    const uint64_t list_words = ((uint64_t)num_st * coarse_cap + BGS_SELFTEST_BIN_GUARD) * 2u;
    if (lists_capacity_words < list_words)
        return fail(ctx, BGS_EINVAL, "bin self-test: host_lists holds " + std::to_string(lists_capacity_words) + " words, the lists and their guard are " +
                                         std::to_string(list_words));
    if (int rc = enter_drained(ctx); rc != BGS_OK) return rc;
    const size_t status_words = ((size_t)(n + 255u) / 256u + 1u) * MAX_SUPERTILES;   // (as scratch_layout sizes the frames')
    DeviceBuffer<uint32_t> rects_buf, status_buf, lists_buf;
    DeviceBuffer<Control> ctl_buf;
    if (!rects_buf.reserve(n) || !status_buf.reserve(status_words) || !lists_buf.reserve((size_t)list_words) || !ctl_buf.reserve(1))
        return fail(ctx, BGS_ENOMEM, "hipMalloc(bin self-test) failed");
    Control* const ctl = ctl_buf.ptr;
    hipStream_t st = ctx->lanes[0].stream;
    CommandStream cs(st);
    cs.zero(ctl, sizeof(Control));
    cs.zero(status_buf.ptr, status_words * sizeof(uint32_t));
    cs.fill(lists_buf.ptr, 0xFF, (size_t)list_words * sizeof(uint32_t));
    cs.up(rects_buf.ptr, host_rects, (size_t)n * sizeof(uint32_t));
    cs.word(&ctl->draw_count, n);
    BinLaunch bin;
    bin.rects = rects_buf.ptr; bin.ctl = ctl; bin.bin_status = status_buf.ptr; bin.coarse = lists_buf.ptr;
    bin.coarse_cap = coarse_cap; bin.sup_edge = sup_edge; bin.tiles_x = tiles_x; bin.tiles_y = tiles_y;
    bin.wide = wide != 0u; bin.blocks = blocks;   // (the caller's grid)
    if (cs.ok) bin.launch(st);
    cs.launched();
    cs.down(host_lists, lists_buf.ptr, (size_t)list_words * sizeof(uint32_t));
    cs.down(host_totals, ctl->coarse_total, sizeof ctl->coarse_total);
    cs.down(error_out, &ctl->error, sizeof(uint32_t));
    cs.sync();
    if (!cs.ok) return fail(ctx, BGS_EHIP, "bin self-test failed on the device");
    return BGS_OK;
}

// The Control block of the lane's last frame (Lane::last_ctl) is one of the two in the lane's scratch region. Where each
// value the hook reads is final, from bgs_frame.hip (enqueue_frame, finish_lane) and render_kernels.hip:
//   records      written by project_rank only (project_kernel / project_emit_kernel); bin_kernel and the rasterisers read them.
//                A re-run projects the whole list again into the same buffer, so the buffer holds the last run's records.
//   rects        written by project_kernel only (rects[j] for every j < count), read by bin_kernel; BINNING_SCAN frames only.
//   draw_count   keygen / the compaction / the bucket sort; the project kernels read it as `sort_overflow ? 0 : draw_count`,
//                which is what is reported here.
//   visible_count, color_max_bits   accumulated by the project kernel of the run alone. A BINNING_SCAN frame's rasteriser
//                zeroes the OTHER Control block (the lane's next frame's) and copies the header words to the pinned host
//                copy, which does not carry color_max_bits: both words are read from the frame's own device block, which
//                nothing writes until the lane's next frame runs (its rasteriser zeroes it as ITS other block). A
//                BINNING_SORT frame copies its whole block to the host and leaves it in place until the next memset.
int bgs_debug_frame_records(bgs_ctx* ctx, void* host_records, uint64_t records_capacity_bytes, uint32_t* host_rects,
                            uint32_t rects_capacity_words, bgs_frame_records_info* info_out) {
    if (!ctx) return fail(nullptr, BGS_EINVAL, "ctx is NULL");
    if (!info_out) return fail(ctx, BGS_EINVAL, "frame records: info_out is NULL");
    Lane* lane = nullptr;
    if (int rc = last_frame(ctx, "frame records", LF_DEPTH_1 | LF_NO_ASYNC, &lane); rc != BGS_OK) return rc;
    Lane& L = *lane;
    hipStream_t st = L.stream;
    uint32_t head[CONTROL_HEADER_WORDS] = {};
    uint32_t cmax = 0u;
    HIP_TRY(ctx, hipMemcpyAsync(head, L.last_ctl, sizeof head, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(&cmax, &L.last_ctl->color_max_bits, sizeof cmax, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    struct { uint32_t draw_count, visible_count, sort_overflow; } h{head[offsetof(Control, draw_count) / 4u], head[offsetof(Control, visible_count) / 4u],
                                                                     head[offsetof(Control, sort_overflow) / 4u]};
    static_assert(offsetof(Control, sort_overflow) / 4u < CONTROL_HEADER_WORDS, "the three words are in the header");
    bgs_frame_records_info info{};
    info.draw_count = h.sort_overflow ? 0u : h.draw_count;
    info.record_stride = L.plan.rec_bytes;
    info.has_rects = L.plan.scan ? 1u : 0u;
    info.visible_count = h.visible_count;
    info.color_max_bits = cmax;
    *info_out = info;
    if (!host_records && !host_rects) return BGS_OK;   // the sizes only
    const uint64_t rec_bytes = (uint64_t)info.draw_count * info.record_stride;
    if (info.draw_count > L.plan.n || rec_bytes > (uint64_t)L.records.capacity ||
        (info.has_rects && info.draw_count > L.rects.capacity))
        return fail(ctx, BGS_EINTERNAL, "frame records: the frame's draw count exceeds the lane's buffers");
    if (!host_records || records_capacity_bytes < rec_bytes)
        return fail(ctx, BGS_EINVAL, "frame records: host_records holds " + std::to_string(records_capacity_bytes) + " bytes, the frame's records are " +
                                         std::to_string(rec_bytes));
    if (info.has_rects && (!host_rects || rects_capacity_words < info.draw_count))
        return fail(ctx, BGS_EINVAL, "frame records: host_rects holds " + std::to_string(rects_capacity_words) + " words, the frame has " +
                                         std::to_string(info.draw_count) + " ranks");
    if (rec_bytes) HIP_TRY(ctx, hipMemcpyAsync(host_records, L.records.ptr, rec_bytes, hipMemcpyDeviceToHost, st));
    if (info.has_rects && info.draw_count)
        HIP_TRY(ctx, hipMemcpyAsync(host_rects, L.rects.ptr, (size_t)info.draw_count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return BGS_OK;
}

// What the binning stage of the last frame left, from the lane the frame ran on (ctx->recent: lane 0 for every synchronous
// frame, at any pipeline depth). Where each value is final (bgs_frame.hip, render_kernels.hip):
//   BINNING_SCAN  coarse_total   written by bin_kernel into the frame's Control block; the frame's rasteriser (or, under
//                                BGS_DEBUG_NO_RASTER_CLEANUP, the copy behind it) copies all 256 words to the lane's pinned
//                                Control, which finish_lane reads and nothing writes until the lane's next frame: read there.
//                 lists          L.coarse, num_st lists coarse_cap (Lane::pending_coarse_cap) entries apart, written by
//                                bin_kernel only. A re-run writes them again with the re-run's capacity.
//   BINNING_SORT  instances      L.inst[0] after the two tile-id passes (inst[0] -> inst[1] -> inst[0]); instance_count in
//                                the pinned Control (the whole block is copied behind the frame).
//                 ranges         in the lane's scratch region, which a BINNING_SORT frame leaves as it is: whatever
//                                rewrites the region (the next frame's memset, bgs_radix_sort_pairs, a re-allocation)
//                                clears Lane::last_ctl with it.
int bgs_debug_frame_lists(bgs_ctx* ctx, uint32_t* host_totals, uint32_t totals_capacity_words, uint32_t* host_entries,
                          uint64_t entries_capacity_words, uint32_t* host_ranges, uint32_t ranges_capacity_words,
                          bgs_frame_lists_info* info_out) {
    if (!ctx) return fail(nullptr, BGS_EINVAL, "ctx is NULL");
    if (!info_out) return fail(ctx, BGS_EINVAL, "frame lists: info_out is NULL");
    Lane* lane = nullptr;
    if (int rc = last_frame(ctx, "frame lists", LF_RECENT | LF_NO_ASYNC, &lane); rc != BGS_OK) return rc;
    Lane& L = *lane;
    const FramePlan& p = L.plan;
    const Control& h = *L.h_ctl.ptr;
    hipStream_t st = L.stream;
    bgs_frame_lists_info info{};
    info.binning = p.scan ? BINNING_SCAN : BINNING_SORT;
    info.draw_count = h.sort_overflow ? 0u : h.draw_count;
    if (p.scan) {
        const uint32_t cap = L.pending_coarse_cap;
        info.sup_edge = p.sup_edge;
        info.sup_x = ((uint32_t)p.fp.tiles_x + p.sup_edge - 1u) / p.sup_edge;
        info.sup_y = ((uint32_t)p.fp.tiles_y + p.sup_edge - 1u) / p.sup_edge;
        info.level = p.level;
        info.coarse_cap = cap;
        info.wide_bin = p.wide_bin ? 1u : 0u;
        const uint32_t num_st = info.draw_count ? p.num_st : 0u;   // (an empty draw list launches no bin_kernel: no lists)
        if (num_st > MAX_SUPERTILES || info.sup_x * info.sup_y != p.num_st || (size_t)p.num_st * cap * 2u > L.coarse.capacity)
            return fail(ctx, BGS_EINTERNAL, "frame lists: the frame's supertile lists exceed the lane's buffer");
        for (uint32_t s = 0; s < num_st; ++s) info.entry_count += std::min(h.coarse_total[s], cap);
        *info_out = info;
        if (!host_totals && !host_entries && !host_ranges) return BGS_OK;   // the sizes only
        if (!host_totals || totals_capacity_words < p.num_st)
            return fail(ctx, BGS_EINVAL, "frame lists: host_totals holds " + std::to_string(totals_capacity_words) + " words, the frame has " +
                                             std::to_string(p.num_st) + " supertiles");
        if (info.entry_count && (!host_entries || entries_capacity_words < info.entry_count * 2u))
            return fail(ctx, BGS_EINVAL, "frame lists: host_entries holds " + std::to_string(entries_capacity_words) + " words, the frame's lists are " +
                                             std::to_string(info.entry_count * 2u));
        uint64_t at = 0;
        for (uint32_t s = 0; s < p.num_st; ++s) {
            host_totals[s] = num_st ? h.coarse_total[s] : 0u;
            const uint32_t len = num_st ? std::min(h.coarse_total[s], cap) : 0u;
            if (len) HIP_TRY(ctx, hipMemcpyAsync(host_entries + at, L.coarse.ptr + (size_t)s * cap * 2u, (size_t)len * 8u, hipMemcpyDeviceToHost, st));
            at += (uint64_t)len * 2u;
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));
        return BGS_OK;
    }
    constexpr uint32_t RANGE_WORDS = RADIX_BASE * RADIX_BASE * 2u;
    info.entry_count = info.instance_count = h.instance_count;
    *info_out = info;
    if (!host_totals && !host_entries && !host_ranges) return BGS_OK;   // the sizes only
    if (info.instance_count > L.inst[0].capacity || L.layout.off_ranges + RANGE_WORDS * 4ull > L.layout.bytes)
        return fail(ctx, BGS_EINTERNAL, "frame lists: the frame's instances exceed the lane's buffers");
    if (info.instance_count && (!host_entries || entries_capacity_words < (uint64_t)info.instance_count * 2u))
        return fail(ctx, BGS_EINVAL, "frame lists: host_entries holds " + std::to_string(entries_capacity_words) + " words, the frame's instances are " +
                                         std::to_string((uint64_t)info.instance_count * 2u));
    if (!host_ranges || ranges_capacity_words < RANGE_WORDS)
        return fail(ctx, BGS_EINVAL, "frame lists: host_ranges holds " + std::to_string(ranges_capacity_words) + " words, the table is " +
                                         std::to_string(RANGE_WORDS));
    if (info.instance_count)
        HIP_TRY(ctx, hipMemcpyAsync(host_entries, L.inst[0].ptr, (size_t)info.instance_count * sizeof(uint2), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(host_ranges, L.scratch.ptr + L.layout.off_ranges, (size_t)RANGE_WORDS * 4u, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return BGS_OK;
}

// What lane 0's last frame left for the one behind it: the lane's scratch region and its pinned Control, as they are. Where
// each is final (bgs_frame.hip, render_kernels.hip):
//   scratch        a raster_cleans frame's rasteriser zeroes, at its start, the chain words the frame used and the lane's
//                  OTHER Control block; nothing writes the region behind it until the lane's next frame. Any other frame
//                  leaves what its kernels wrote on top of the memset ahead of it.
//   pinned Control written by the last workgroup of that rasteriser, or by the copy enqueued behind the frame; finish_lane
//                  only reads it.
// A word that is not zero outside the frame's own Control block while the lane believes the region clean would be read as a
// published look-back word by the next frame's chained scans: the hook takes the lane's belief back, and that frame memsets.
int bgs_debug_frame_leftovers(bgs_ctx* ctx, void* host_scratch, uint64_t scratch_capacity_bytes, void* host_control,
                              uint32_t control_capacity_bytes, bgs_scratch_layout* layout_out, bgs_frame_leftovers_info* info_out) {
    static_assert(sizeof(bgs_scratch_layout) == sizeof(ScratchLayout) && offsetof(bgs_scratch_layout, off_ctl1) == offsetof(ScratchLayout, off_ctl1) &&
                      offsetof(bgs_scratch_layout, inst_cap) == offsetof(ScratchLayout, inst_cap) &&
                      offsetof(bgs_scratch_layout, pass_stride) == offsetof(ScratchLayout, pass_stride),
                  "bgs_scratch_layout is ScratchLayout, field by field");
    if (!ctx) return fail(nullptr, BGS_EINVAL, "ctx is NULL");
    if (!info_out || !layout_out) return fail(ctx, BGS_EINVAL, "frame leftovers: layout_out and info_out must be non-NULL");
    Lane* lane = nullptr;
    if (int rc = last_frame(ctx, "frame leftovers", LF_NO_ASYNC_RING | LF_SCRATCH, &lane); rc != BGS_OK) return rc;
    Lane& L = *lane;
    const FramePlan& p = L.plan;
    const ScratchLayout& lay = L.layout;
    const uint8_t* const own = reinterpret_cast<const uint8_t*>(L.last_ctl);
    if (lay.bytes % 4u != 0u || lay.bytes > L.scratch.capacity || lay.off_ctl1 + sizeof(Control) > lay.bytes ||
        (own != L.scratch.ptr && own != L.scratch.ptr + lay.off_ctl1))
        return fail(ctx, BGS_EINTERNAL, "frame leftovers: the lane's scratch layout does not fit its region");
    hipStream_t st = L.stream;
    std::vector<uint32_t> words((size_t)(lay.bytes / 4u));
    HIP_TRY(ctx, hipMemcpyAsync(words.data(), L.scratch.ptr, (size_t)lay.bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const size_t own_first = (size_t)(own - L.scratch.ptr) / 4u, own_end = own_first + sizeof(Control) / 4u;
    uint64_t dirty = 0;
    for (size_t i = 0; i < words.size(); ++i)
        if (words[i] != 0u && (i < own_first || i >= own_end)) dirty += 1u;
    bgs_frame_leftovers_info info{};
    info.dirty_words = dirty;
    info.ctl_block = own == L.scratch.ptr ? 0u : 1u;
    info.scratch_clean = L.scratch_clean ? 1u : 0u;
    if (dirty != 0u && L.scratch_clean) {   // the lane's next frame memsets (enqueue_frame: need_memset)
        L.scratch_clean = false;
        info.scratch_reset = 1u;
    }
    info.raster_cleans = p.raster_cleans ? 1u : 0u;
    info.bucket = p.bucket ? 1u : 0u;
    info.places = p.places;
    info.large = p.large ? 1u : 0u;
    info.wide = p.wide ? 1u : 0u;
    info.wide_bin = p.wide_bin ? 1u : 0u;
    info.kept = p.kept ? 1u : 0u;
    info.bucket_sub = p.bucket_sub;
    info.split_sub_out = p.split_sub_out;
    info.keygen_tile = p.kept ? KEYGEN_TILE : keygen_tile_splats(p.n);   // (the compaction's tile: entries_kernels.hip)
    info.n = p.n;
    info.ntiles = p.ntiles;
    info.raster_mode = (uint32_t)p.raster.mode;
    info.strips_appended = L.last_strips ? 1u : 0u;
    info.graph_replay = L.last_replay ? 1u : 0u;
    info.binning = p.scan ? BINNING_SCAN : BINNING_SORT;
    info.control_bytes = (uint32_t)sizeof(Control);
    info.culled_tail = p.culled_tail ? 1u : 0u;
    std::memcpy(layout_out, &lay, sizeof lay);
    *info_out = info;
    if (!host_scratch && !host_control) return BGS_OK;   // the sizes only
    if (!host_scratch || scratch_capacity_bytes < lay.bytes)
        return fail(ctx, BGS_EINVAL, "frame leftovers: host_scratch holds " + std::to_string(scratch_capacity_bytes) + " bytes, the lane's scratch region is " +
                                         std::to_string(lay.bytes));
    if (!host_control || control_capacity_bytes < sizeof(Control))
        return fail(ctx, BGS_EINVAL, "frame leftovers: host_control holds " + std::to_string(control_capacity_bytes) + " bytes, the Control block is " +
                                         std::to_string(sizeof(Control)));
    std::memcpy(host_scratch, words.data(), (size_t)lay.bytes);
    std::memcpy(host_control, L.h_ctl.ptr, sizeof(Control));
    return BGS_OK;
}

// What the last frame's persistent kernels launched (Lane::Grids, filled by enqueue_frame from the frame's launch structs) and
// the tiles of work they had: of n for the front kernel, of the completed frame's Control copy for the kernels whose count
// only the device knew (draw_count, voided by sort_overflow as the kernels read it; instance_count).
int bgs_debug_frame_grids(bgs_ctx* ctx, uint32_t* out, uint32_t capacity) {
    if (!ctx) return fail(nullptr, BGS_EINVAL, "ctx is NULL");
    if (!out) return fail(ctx, BGS_EINVAL, "frame grids: out is NULL");
    if (capacity < BGS_FRAME_GRIDS_WORDS)
        return fail(ctx, BGS_EINVAL, "frame grids: out holds " + std::to_string(capacity) + " words, the report is " + std::to_string(BGS_FRAME_GRIDS_WORDS));
    if (int rc = refuse_in_flight(ctx, "frame grids"); rc != BGS_OK) return rc;
    const Lane* newest = &ctx->lanes[0];
    for (const Lane& lane : ctx->lanes)
        if (lane.grids.stamp > newest->grids.stamp) newest = &lane;
    const Lane& L = *newest;
    const Lane::Grids& g = L.grids;
    if (!g.stamp || !L.h_ctl.ptr) return fail(ctx, BGS_EINVAL, "frame grids: no frame has been run");
    const Control& h = *L.h_ctl.ptr;
    const uint64_t draw = h.sort_overflow ? 0u : h.draw_count;
    const uint64_t items[3] = {g.n, draw, h.instance_count};   // (Lane::Grids::Count)
    for (int k = 0; k < Lane::Grids::KERNELS; ++k) {
        out[2 * k] = g.blocks[k];
        out[2 * k + 1] = g.per_tile[k] ? (uint32_t)((items[g.count[k]] + g.per_tile[k] - 1u) / g.per_tile[k]) : 0u;
    }
    out[10] = g.cap;
    out[11] = g.front_chainless ? 1u : 0u;
    // the tail behind the draw list, where the front kernel left it (index order after keygen, list order after the compaction)
    const uint64_t tail = (g.tail && L.culled.ptr && g.n >= h.draw_count) ? (uint64_t)(uintptr_t)L.culled.ptr : 0u;
    out[12] = (uint32_t)tail;
    out[13] = (uint32_t)(tail >> 32);
    out[14] = tail ? g.n - h.draw_count : 0u;
    out[15] = 0u;
    return BGS_OK;
}

// bucket_sort_kernel alone, on the caller's bucket contents: a zeroed Control with the caller's counts, slot regions that
// hold each bucket's pairs at their start and 0xFF bytes behind them, an output list of n + BGS_SELFTEST_BUCKET_GUARD entries
// of 0xFF bytes. What the kernel indexes (sort_kernels.hip): bucket_count[i < nb], a region's first min(count, cap) slots
// (a launch with some count over cap reads no slot at all), out[offset of the bucket + rank < n]: any counts are in bounds
// once pair_count is their clamped sum, so only the geometry is refused.
int bgs_selftest_bucket_sort(bgs_ctx* ctx, uint32_t sub, uint32_t wide, uint32_t key_xor, const uint32_t* host_counts,
                             const uint32_t* host_pairs, uint32_t pair_count, uint32_t* host_out, uint64_t out_capacity_words,
                             uint32_t* info_out) {
    if (!ctx) return fail(nullptr, BGS_EINVAL, "ctx is NULL");
    if (!host_counts || !host_out || !info_out || (!host_pairs && pair_count))
        return fail(ctx, BGS_EINVAL, "bucket self-test: host_counts, host_pairs, host_out and info_out must be non-NULL");
    if (sub < 1u || sub > BUCKET_SUB_MAX) return fail(ctx, BGS_EINVAL, "bucket self-test: sub must be 1 .. 16, got " + std::to_string(sub));
    if (wide > 1u) return fail(ctx, BGS_EINVAL, "bucket self-test: wide must be 0 or 1, got " + std::to_string(wide));
    const uint32_t nb = BUCKET_COUNT * sub, cap = wide ? BUCKET_CAP_WIDE : BUCKET_CAP;
    uint64_t n = 0;
    for (uint32_t b = 0; b < nb; ++b) n += std::min(host_counts[b], cap);
    if (n != pair_count)
        return fail(ctx, BGS_EINVAL, "bucket self-test: pair_count is " + std::to_string(pair_count) + ", host_counts asks for " + std::to_string(n) +
                                         " pairs (the sum of min(count, capacity))");
    const uint64_t out_words = (n + BGS_SELFTEST_BUCKET_GUARD) * 2u;
    if (out_capacity_words < out_words)
        return fail(ctx, BGS_EINVAL, "bucket self-test: host_out holds " + std::to_string(out_capacity_words) + " words, the list and its guard are " +
                                         std::to_string(out_words));
    if (int rc = enter_drained(ctx); rc != BGS_OK) return rc;
    DeviceBuffer<uint2> slots_buf, out_buf;
    DeviceBuffer<Control> ctl_buf;
    if (!slots_buf.reserve((size_t)nb * cap) || !out_buf.reserve((size_t)(n + BGS_SELFTEST_BUCKET_GUARD)) || !ctl_buf.reserve(1))
        return fail(ctx, BGS_ENOMEM, "hipMalloc(bucket self-test) failed");
    Control* const ctl = ctl_buf.ptr;
    hipStream_t st = ctx->lanes[0].stream;
    CommandStream cs(st);
    cs.zero(ctl, sizeof(Control));
    cs.fill(slots_buf.ptr, 0xFF, (size_t)nb * cap * sizeof(uint2));
    cs.fill(out_buf.ptr, 0xFF, (size_t)out_words * sizeof(uint32_t));
    cs.up(ctl->bucket_count, host_counts, (size_t)nb * sizeof(uint32_t));
    uint64_t at = 0;
    for (uint32_t b = 0; b < nb; ++b) {
        const uint32_t len = std::min(host_counts[b], cap);
        if (len) cs.up(slots_buf.ptr + (size_t)b * cap, host_pairs + at * 2u, (size_t)len * sizeof(uint2));
        at += len;
    }
    if (cs.ok) cs.launched(launch_bucket_sort(st, slots_buf.ptr, out_buf.ptr, ctl, key_xor, nb, wide != 0u));
    cs.down(host_out, out_buf.ptr, (size_t)out_words * sizeof(uint32_t));
    cs.down(&info_out[0], &ctl->draw_count, sizeof(uint32_t));
    cs.down(&info_out[1], &ctl->sort_overflow, sizeof(uint32_t));
    cs.down(&info_out[2], &ctl->bucket_max, sizeof(uint32_t));
    cs.sync();
    if (!cs.ok) return fail(ctx, BGS_EHIP, "bucket self-test failed on the device");
    return BGS_OK;
}

// keygen's bucket placement alone: the KeygenLaunch of a bucket frame (bgs_frame.hip, enqueue_frame) with buffers of the
// call's own. What keygen_kernel<.., BUCKET = true, ..> indexes (sort_kernels.hip): pos[i < n]; bucket_count[bucket < nb];
// bucket_slots[bucket * cap + slot < cap]; the table's first nb - 1 keys (kernel arguments or device_keys); with ORDERED
// the tile's chain word part_status[tile < ceil(n / 2048)], ticket[ticket_slot][0] and culled[i - drawable before i < n].
// entries, fp_out, zero_word and bucket_status stay null: a bucket keygen writes no index-ordered list, and the other three
// are optional (bucket_status is unused).
int bgs_selftest_keygen_buckets(bgs_ctx* ctx, const bgs_cloud* cloud, const bgs_view* view, const bgs_settings* settings,
                                const uint32_t* host_splitters, uint32_t sub, uint32_t wide_buckets, uint32_t ordered,
                                uint32_t alone, uint32_t* host_counts, uint32_t* host_slots, uint64_t slots_capacity_words,
                                uint32_t* host_culled, uint64_t culled_capacity_words, uint32_t* info_out) {
    if (!ctx) return fail(nullptr, BGS_EINVAL, "ctx is NULL");
    if (!cloud || !view || !settings || !host_splitters || !host_counts || !host_slots || !info_out)
        return fail(ctx, BGS_EINVAL, "keygen self-test: cloud, view, settings, host_splitters, host_counts, host_slots and info_out must be non-NULL");
    const uint32_t n = cloud->ptrs.n;
    if (n < 1u || n > MAX_SPLATS) return fail(ctx, BGS_EINVAL, "keygen self-test: the cloud must hold 1 .. 2^30 - 1 splats, got " + std::to_string(n));
    if (sub < 1u || sub > BUCKET_SUB_MAX) return fail(ctx, BGS_EINVAL, "keygen self-test: sub must be 1 .. 16, got " + std::to_string(sub));
    if (wide_buckets > 1u) return fail(ctx, BGS_EINVAL, "keygen self-test: wide_buckets must be 0 or 1, got " + std::to_string(wide_buckets));
    if (ordered > 1u) return fail(ctx, BGS_EINVAL, "keygen self-test: ordered must be 0 or 1, got " + std::to_string(ordered));
    if (alone > 1u) return fail(ctx, BGS_EINVAL, "keygen self-test: alone must be 0 or 1, got " + std::to_string(alone));
    if (settings->sort_mode > BGS_SORT_STD) return fail(ctx, BGS_EINVAL, "keygen self-test: unknown sort_mode");
    if (settings->radix_depth_bits != 16 && settings->radix_depth_bits != 24 && settings->radix_depth_bits != 32)
        return fail(ctx, BGS_EINVAL, "keygen self-test: radix_depth_bits must be 16, 24 or 32");
    const uint32_t nb = BUCKET_COUNT * sub, cap = wide_buckets ? BUCKET_CAP_WIDE : BUCKET_CAP, nkeys = nb - 1u;
    for (uint32_t t = 1; t < nkeys; ++t)
        if (host_splitters[t] < host_splitters[t - 1u])
            return fail(ctx, BGS_EINVAL, "keygen self-test: host_splitters must ascend, entry " + std::to_string(t) + " is below entry " + std::to_string(t - 1u));
    const uint64_t slot_words = (uint64_t)nb * cap * 2u;
    if (slots_capacity_words < slot_words)
        return fail(ctx, BGS_EINVAL, "keygen self-test: host_slots holds " + std::to_string(slots_capacity_words) + " words, the slot regions are " +
                                         std::to_string(slot_words));
    if (ordered && (!host_culled || culled_capacity_words < (uint64_t)n * 2u))
        return fail(ctx, BGS_EINVAL, "keygen self-test: host_culled must hold " + std::to_string((uint64_t)n * 2u) + " words with ordered = 1");
    if (int rc = enter_drained(ctx); rc != BGS_OK) return rc;
    const size_t status_words = (size_t)(n + KEYGEN_TILE - 1u) / KEYGEN_TILE + 1u;
    DeviceBuffer<uint2> slots_buf, culled_buf;
    DeviceBuffer<uint32_t> status_buf, keys_buf;
    DeviceBuffer<Control> ctl_buf;
    if (!slots_buf.reserve((size_t)nb * cap) || !status_buf.reserve(status_words) || !ctl_buf.reserve(1) ||
        (ordered && !culled_buf.reserve(n)) || (sub > BUCKET_SUB_KERNARG && !keys_buf.reserve(nkeys)))
        return fail(ctx, BGS_ENOMEM, "hipMalloc(keygen self-test) failed");
    Control* const ctl = ctl_buf.ptr;
    hipStream_t st = ctx->lanes[0].stream;
    KeygenLaunch kg{};
    fill_frame_params(n, view, settings, kg.fp);
    kg.fp.sort_path = 1u;
    kg.pos = cloud->ptrs.position_visibility;
    kg.culled = ordered ? culled_buf.ptr : nullptr;   // (null: the chainless instantiation, as in every rendered frame)
    kg.ctl = ctl;
    kg.part_status = status_buf.ptr;
    kg.places = 4u;
    kg.ticket_slot = TICKET_FRONT;
    kg.bucket_slots = slots_buf.ptr;
    if (sub <= BUCKET_SUB_KERNARG) std::memcpy(kg.split.key, host_splitters, (size_t)nkeys * sizeof(uint32_t));
    kg.split.device_keys = keys_buf.ptr;
    kg.split.sub = sub;
    kg.split.wide = wide_buckets;
    kg.wide = alone != 0u;
    if (!kg.prepare(grid_under_cap(ctx->num_cus * 4, ctx->grid_cap))) return fail(ctx, BGS_EINTERNAL, "keygen self-test: nothing to launch");
    Lane::Grids& g = ctx->lanes[0].grids = Lane::Grids(++ctx->grid_stamps, n, ctx->grid_cap);   // (the culled list is the call's own: no tail)
    g.launched(g.FRONT, kg);
    g.front_chainless = !ordered;
    CommandStream cs(st);
    cs.zero(ctl, sizeof(Control));
    cs.zero(status_buf.ptr, status_words * sizeof(uint32_t));
    cs.fill(slots_buf.ptr, 0xFF, (size_t)slot_words * sizeof(uint32_t));
    if (ordered) cs.fill(culled_buf.ptr, 0xFF, (size_t)n * sizeof(uint2));
    if (sub > BUCKET_SUB_KERNARG) cs.up(keys_buf.ptr, host_splitters, (size_t)nkeys * sizeof(uint32_t));
    if (cs.ok) cs.launched(kg.launch(st));
    cs.down(host_counts, ctl->bucket_count, (size_t)nb * sizeof(uint32_t));
    cs.down(host_slots, slots_buf.ptr, (size_t)slot_words * sizeof(uint32_t));
    if (ordered) cs.down(host_culled, culled_buf.ptr, (size_t)n * sizeof(uint2));
    cs.down(&info_out[0], &ctl->draw_count, sizeof(uint32_t));
    cs.down(&info_out[1], &ctl->splat_count, sizeof(uint32_t));
    cs.down(&info_out[2], &ctl->error, sizeof(uint32_t));
    cs.sync();
    if (!cs.ok) return fail(ctx, BGS_EHIP, "keygen self-test failed on the device");
    info_out[3] = kg.threads;
    info_out[4] = kg.blocks;
    return BGS_OK;
}

// The two rasterisers alone, on the caller's stage inputs. What the kernels index (render_kernels.hip), and what bounds it:
//   raster_scan_kernel   coarse_total[st < supertiles <= 256]; list[st * coarse_cap + i], i < min(total, coarse_cap);
//                        records[rank]: every rank in those positions is checked against record_count here; heavy_in's count
//                        (<= HEAVY_CAP), list[sb < count] (tile ids checked here) and flags[tile < tiles]; order[block <
//                        (tiles + 3) / 4] (a checked permutation, so every tile is drawn once); cost_out[tile], heavy_out's
//                        list[at < HEAVY_CAP] and flags[tile]; the depth plane and the target at pixels inside width x height.
//   raster_kernel        ranges[ty << 8 | tx] (65 536 entries), instances[range) and records[rank] of instances built here from
//                        the checked lists; the same pixels.
// The records' and rectangles' CONTENTS may be anything: no index is formed from them (a rectangle is only compared with the
// tile's coordinates, a record only feeds arithmetic).
int bgs_selftest_raster(bgs_ctx* ctx, const bgs_raster_selftest* in, float* host_scan, float* host_sort,
                        uint64_t image_capacity_floats, uint16_t* host_cost, uint8_t* host_heavy, uint64_t heavy_capacity_bytes,
                        uint32_t* error_out) {
    if (!ctx) return fail(nullptr, BGS_EINVAL, "ctx is NULL");
    if (!in || !host_scan || !host_sort || !host_cost || !host_heavy || !error_out)
        return fail(ctx, BGS_EINVAL, "raster self-test: in, host_scan, host_sort, host_cost, host_heavy and error_out must be non-NULL");
    const auto num = [](uint64_t v) { return std::to_string(v); };
    if (in->width < 1u || in->width > 512u) return fail(ctx, BGS_EINVAL, "raster self-test: width must be 1 .. 512, got " + num(in->width));
    if (in->height < 1u || in->height > 512u) return fail(ctx, BGS_EINVAL, "raster self-test: height must be 1 .. 512, got " + num(in->height));
    const uint32_t ms = in->sample_count;
    if (ms != 1u && ms != 2u && ms != 4u && ms != 8u) return fail(ctx, BGS_EINVAL, "raster self-test: sample_count must be 1, 2, 4 or 8, got " + num(ms));
    if (in->variant > 2u) return fail(ctx, BGS_EINVAL, "raster self-test: variant must be 0 (OBB), 1 (AABB3D) or 2 (surfel), got " + num(in->variant));
    if (in->overlay > 1u) return fail(ctx, BGS_EINVAL, "raster self-test: overlay must be 0 or 1, got " + num(in->overlay));
    if (in->mode > 2u) return fail(ctx, BGS_EINVAL, "raster self-test: mode must be 0, 1 or 2, got " + num(in->mode));
    const RasterInst inst{(int)in->variant, ms, in->depth != nullptr, in->overlay != 0u, (int)in->mode};
    if (!inst.exists())
        return fail(ctx, BGS_EINVAL, "raster self-test: mode " + num(in->mode) + " is not built for variant " + num(in->variant) + " at " + num(ms) +
                                         " samples" + (in->overlay ? " with the overlay" : "") + " (RasterInst::exists)");
    if (in->reserved != 0u) return fail(ctx, BGS_EINVAL, "raster self-test: reserved must be 0");
    if (!(in->viewport_w > 0.0f) || !(in->viewport_h > 0.0f)) return fail(ctx, BGS_EINVAL, "raster self-test: viewport_w and viewport_h must be > 0");
    const uint32_t tiles_x = (in->width + TILE_PX - 1u) / TILE_PX, tiles_y = (in->height + TILE_PX - 1u) / TILE_PX, ntiles = tiles_x * tiles_y;
    if (in->sup_edge < 1u || in->sup_edge > 32u) return fail(ctx, BGS_EINVAL, "raster self-test: sup_edge must be 1 .. 32, got " + num(in->sup_edge));
    if (!supertile_bins_fit(tiles_x, tiles_y, in->sup_edge))
        return fail(ctx, BGS_EINVAL, "raster self-test: sup_edge " + num(in->sup_edge) + " gives more than " + num(MAX_SUPERTILES) +
                                         " supertiles, or more than " + num(MAX_SUPERTILES_PER_AXIS) + " on an axis");
    const uint32_t sup_x = (tiles_x + in->sup_edge - 1u) / in->sup_edge, sup_y = (tiles_y + in->sup_edge - 1u) / in->sup_edge, num_st = sup_x * sup_y;
    const uint32_t cap = in->coarse_cap;
    if (cap < 1u || (uint64_t)num_st * cap > (1ull << 20))
        return fail(ctx, BGS_EINVAL, "raster self-test: coarse_cap must be >= 1 and supertiles x coarse_cap <= 2^20, got " + num(cap));
    if (in->record_count > (1u << 20)) return fail(ctx, BGS_EINVAL, "raster self-test: record_count must be <= 2^20, got " + num(in->record_count));
    if (!in->lists || !in->totals || (!in->records && in->record_count))
        return fail(ctx, BGS_EINVAL, "raster self-test: records, lists and totals must be non-NULL");
    for (uint32_t s = 0; s < num_st; ++s) {
        const uint32_t len = std::min(in->totals[s], cap);
        for (uint32_t i = 0; i < len; ++i) {
            const uint32_t rank = in->lists[((size_t)s * cap + i) * 2u];
            if (rank >= in->record_count)
                return fail(ctx, BGS_EINVAL, "raster self-test: lists: entry " + num(i) + " of list " + num(s) + " holds rank " + num(rank) +
                                                 ", record_count is " + num(in->record_count));
        }
    }
    if (in->heavy_tiles || in->heavy_count) {
        if (in->mode == 0u) return fail(ctx, BGS_EINVAL, "raster self-test: heavy_tiles needs mode 1 or 2 (the plain instantiation has no strip workgroups)");
        if (!in->heavy_tiles || in->heavy_count > HEAVY_CAP)
            return fail(ctx, BGS_EINVAL, "raster self-test: heavy_count must be <= " + num(HEAVY_CAP) + " with heavy_tiles non-NULL, got " + num(in->heavy_count));
    }
    std::vector<uint8_t> heavy_host(heavy_feedback_bytes(ntiles), 0u);
    for (uint32_t i = 0; i < in->heavy_count; ++i) {
        const uint32_t t = in->heavy_tiles[i];
        if (t >= ntiles) return fail(ctx, BGS_EINVAL, "raster self-test: heavy_tiles[" + num(i) + "] is " + num(t) + ", the target has " + num(ntiles) + " tiles");
        if (heavy_host[HEAVY_FLAGS_OFFSET + t]) return fail(ctx, BGS_EINVAL, "raster self-test: heavy_tiles names tile " + num(t) + " twice");
        heavy_host[HEAVY_FLAGS_OFFSET + t] = 1u;
        const uint16_t t16 = (uint16_t)t;
        memcpy(&heavy_host[HEAVY_LIST_OFFSET + 2u * i], &t16, 2u);
    }
    memcpy(&heavy_host[0], &in->heavy_count, 4u);
    const uint32_t nblocks = (ntiles + 3u) / 4u;
    if (in->order) {
        std::vector<uint8_t> seen(nblocks, 0u);
        for (uint32_t b = 0; b < nblocks; ++b) {
            const uint32_t g = in->order[b];
            if (g >= nblocks || seen[g])
                return fail(ctx, BGS_EINVAL, "raster self-test: order is not a permutation of 0 .. " + num(nblocks - 1u) + " (entry " + num(b) + " is " + num(g) + ")");
            seen[g] = 1u;
        }
    }
    const uint64_t pixels = (uint64_t)in->width * in->height, image_floats = (pixels + BGS_SELFTEST_RASTER_GUARD) * 4u;
    if (image_capacity_floats < image_floats)
        return fail(ctx, BGS_EINVAL, "raster self-test: host_scan / host_sort hold " + num(image_capacity_floats) + " floats, an image and its guard are " +
                                         num(image_floats));
    if (heavy_capacity_bytes < heavy_host.size())
        return fail(ctx, BGS_EINVAL, "raster self-test: host_heavy holds " + num(heavy_capacity_bytes) + " bytes, the buffer is " + num(heavy_host.size()));
    // the instance-sort rasteriser's inputs, from the same lists: per tile the entries of its supertile's list whose rectangle holds it
    std::vector<uint2> instances;
    std::vector<uint2> ranges((size_t)RADIX_BASE * RADIX_BASE, make_uint2(0u, 0u));
    for (uint32_t ty = 0; ty < tiles_y; ++ty)
        for (uint32_t tx = 0; tx < tiles_x; ++tx) {
            const uint32_t s = (ty / in->sup_edge) * sup_x + tx / in->sup_edge, len = std::min(in->totals[s], cap);
            const uint32_t start = (uint32_t)instances.size();
            for (uint32_t i = 0; i < len; ++i) {
                const uint32_t rank = in->lists[((size_t)s * cap + i) * 2u], rect = in->lists[((size_t)s * cap + i) * 2u + 1u];
                if (tx >= (rect & 255u) && tx <= ((rect >> 8) & 255u) && ty >= ((rect >> 16) & 255u) && ty <= (rect >> 24))
                    instances.push_back(make_uint2((ty << 8) | tx, rank));
            }
            if (instances.size() > (1u << 24)) return fail(ctx, BGS_EINVAL, "raster self-test: the lists hold more than 2^24 tile instances");
            ranges[(ty << 8) | tx] = make_uint2(start, (uint32_t)instances.size());
        }
    if (int rc = enter_drained(ctx); rc != BGS_OK) return rc;
    const size_t stride = in->variant == (uint32_t)RV_SURFEL ? sizeof(RecordSurfel) : sizeof(Record);
    const size_t list_words = (size_t)num_st * cap * 2u, depth_floats = (size_t)pixels * ms;
    DeviceBuffer<uint8_t> rec_buf, heavy_in_buf, heavy_out_buf;
    DeviceBuffer<uint32_t> lists_buf;
    DeviceBuffer<float> depth_buf, scan_buf, sort_buf;
    DeviceBuffer<uint2> inst_buf, ranges_buf;
    DeviceBuffer<uint16_t> order_buf, cost_buf;
    DeviceBuffer<Control> ctl_buf;
    DeviceBuffer<FrameParams> fp_buf;
    if (!rec_buf.reserve((size_t)in->record_count * stride) || !lists_buf.reserve(list_words) || !scan_buf.reserve((size_t)image_floats) ||
        !sort_buf.reserve((size_t)image_floats) || !inst_buf.reserve(instances.size()) || !ranges_buf.reserve(ranges.size()) ||
        !heavy_in_buf.reserve(heavy_host.size()) || !heavy_out_buf.reserve(heavy_host.size()) || !order_buf.reserve(nblocks) ||
        !cost_buf.reserve(tile_cost_bytes(ntiles) / 2u) || !ctl_buf.reserve(1) || !fp_buf.reserve(1) || (in->depth && !depth_buf.reserve(depth_floats)))
        return fail(ctx, BGS_ENOMEM, "hipMalloc(raster self-test) failed");
    FrameParams fp;
    memset(&fp, 0, sizeof fp);
    fp.viewport_w = in->viewport_w;
    fp.viewport_h = in->viewport_h;
    fp.inv_viewport_w = 1.0f / in->viewport_w;
    fp.inv_viewport_h = 1.0f / in->viewport_h;
    fp.width = (int32_t)in->width;
    fp.height = (int32_t)in->height;
    fp.tiles_x = (int32_t)tiles_x;
    fp.tiles_y = (int32_t)tiles_y;
    fp.aabb = in->variant == (uint32_t)RV_OBB ? 0u : 1u;
    fp.gaussian_mode = in->variant == (uint32_t)RV_SURFEL ? 0u : 1u;
    fp.visualize_bbox = in->overlay;
    fp.sample_count = ms;
    fp.depth_ptr = in->depth ? (uint64_t)reinterpret_cast<uintptr_t>(depth_buf.ptr) : 0ull;
    fp.n = in->record_count;
    memcpy(fp.clear, in->clear, sizeof fp.clear);
    Control* const ctl = ctl_buf.ptr;
    hipStream_t st = ctx->lanes[0].stream;
    CommandStream cs(st);
    cs.zero(ctl, sizeof(Control));
    cs.fill(scan_buf.ptr, 0xFF, (size_t)image_floats * sizeof(float));
    cs.fill(sort_buf.ptr, 0xFF, (size_t)image_floats * sizeof(float));
    cs.fill(cost_buf.ptr, 0xFF, tile_cost_bytes(ntiles));
    cs.zero(heavy_out_buf.ptr, heavy_host.size());
    cs.up(heavy_in_buf.ptr, heavy_host.data(), heavy_host.size());
    cs.up(fp_buf.ptr, &fp, sizeof fp);
    cs.up(lists_buf.ptr, in->lists, list_words * sizeof(uint32_t));
    cs.up(ranges_buf.ptr, ranges.data(), ranges.size() * sizeof(uint2));
    cs.up(ctl->coarse_total, in->totals, (size_t)num_st * sizeof(uint32_t));
    cs.up(&ctl->color_max_bits, &in->color_max_bits, sizeof(uint32_t));
    cs.up(&ctl->draw_count, &in->record_count, sizeof(uint32_t));
    if (in->record_count) cs.up(rec_buf.ptr, in->records, (size_t)in->record_count * stride);
    if (!instances.empty()) cs.up(inst_buf.ptr, instances.data(), instances.size() * sizeof(uint2));
    if (in->depth) cs.up(depth_buf.ptr, in->depth, depth_floats * sizeof(float));
    if (in->order) cs.up(order_buf.ptr, in->order, (size_t)nblocks * sizeof(uint16_t));
    const bool exits = in->mode != 0u;
    RasterScanLaunch scan;
    scan.inst = inst; scan.d_fp = fp_buf.ptr; scan.tiles_x = tiles_x; scan.tiles_y = tiles_y;
    scan.records = rec_buf.ptr; scan.coarse = lists_buf.ptr; scan.coarse_cap = cap; scan.sup_edge = in->sup_edge;
    scan.ctl = ctl; scan.framebuffer = reinterpret_cast<float4*>(scan_buf.ptr);
    scan.heavy_in = exits && in->heavy_count ? heavy_in_buf.ptr : nullptr;
    scan.heavy_out = exits ? heavy_out_buf.ptr : nullptr;
    scan.order = in->order ? order_buf.ptr : nullptr;
    scan.cost_out = cost_buf.ptr;
    RasterLaunch sort;
    sort.fp = &fp; sort.inst = inst; sort.records = rec_buf.ptr; sort.instances = inst_buf.ptr; sort.ranges = ranges_buf.ptr;
    sort.framebuffer = reinterpret_cast<float4*>(sort_buf.ptr); sort.clear_color = in->clear; sort.ctl = ctl;
    if (cs.ok && cs.check(scan.launch(st))) cs.check(sort.launch(st));
    cs.launched();
    cs.down(host_scan, scan_buf.ptr, (size_t)image_floats * sizeof(float));
    cs.down(host_sort, sort_buf.ptr, (size_t)image_floats * sizeof(float));
    cs.down(host_cost, cost_buf.ptr, (size_t)ntiles * sizeof(uint16_t));
    cs.down(host_heavy, heavy_out_buf.ptr, heavy_host.size());
    cs.down(error_out, &ctl->error, sizeof(uint32_t));
    cs.sync();
    if (!cs.ok) return fail(ctx, BGS_EHIP, "raster self-test failed on the device");
    return BGS_OK;
}

}  // extern "C"
