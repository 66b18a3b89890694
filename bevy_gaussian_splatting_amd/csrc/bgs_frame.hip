// bgs_frame.hip — libbgs host side: the frame engine. Lanes and their buffers, one frame's launches (directly or as a
// captured graph), completion with its capacity checks and re-runs. What completed frames leave for the next ones, and
// every rule that writes it, is AdaptiveState (adaptive_state.h): this file calls the rules and reads the state.
// (The comment at the top of bgs_api.hip is the overview.)
#include "bgs_context.h"
#include "bounds_math.h"

thread_local std::string bgs_host::g_error;

namespace bgs_host {


// Idle "queue holder" streams (see assign_streams): PROCESS-global, three per device, created once before the first
// context of that device creates its own streams and kept for the life of the process — a process with several
// contexts (multi-camera, multi-cloud) parks three streams in all, not three per context, so its streams keep
// being dealt out evenly over the runtime's four hardware queues. -1: follow BGS_QUEUE_HOLDERS (default on).
constexpr int MAX_DEVICES = 64;
hipStream_t g_queue_holders[MAX_DEVICES][3] = {};
int g_queue_holders_mode = -1;
std::mutex g_queue_holders_mutex;   // contexts of one process may be created from different threads

int fail(bgs_ctx* ctx, int status, const std::string& msg) {
    if (ctx) ctx->error = msg;
    g_error = msg;
    return status;
}

int enter(bgs_ctx* ctx) { return hipSetDevice(ctx->device) == hipSuccess ? BGS_OK : fail(ctx, BGS_EHIP, "hipSetDevice failed"); }

int enter_drained(bgs_ctx* ctx) {
    const int rc = enter(ctx);
    return rc != BGS_OK ? rc : finish_all(ctx);
}

// Lane i runs on stream i % S (S = bgs_set_pipeline_streams, default: the pipeline depth, i.e. a
// stream per lane). With S < depth a stream holds the NEXT frame of a sibling lane while one executes,
// so the stream never waits for the host between frames.
int assign_streams(bgs_ctx* ctx) {
    const int S = ctx->num_streams > 0 ? std::min(ctx->num_streams, ctx->depth) : ctx->depth;
    for (int i = 0; i < MAX_LANES; ++i) {
        Lane& L = ctx->lanes[i];
        if (!L.done) continue;
        const int si = i < ctx->depth ? i % S : i;
        if (!ctx->streams[si]) {
            // The HIP runtime multiplexes a process's streams onto at most 4 hardware queues per priority
            // (GPU_MAX_HW_QUEUES), and only queues are concurrent: two streams on one queue run one after the other.
            // It creates a NEW queue for every new stream until the 4 exist and only then spreads further streams
            // by reference count — and the process's null stream already holds one. Left alone, our streams 0, 1, 2
            // get a queue each and stream 3 joins stream 2's (seen in the runtime's log, AMD_LOG_LEVEL=3): four
            // frames on three queues, two of them serialised — 14.0 k frames/s with 8 lanes on 4 streams where a
            // process that had initialised RCCL (whose idle streams happen to hold the queues) ran 19.2 k. So the
            // context parks three idle streams on the queues FIRST; ours are then dealt out evenly over all four,
            // the null stream's included (8 lanes / 4 streams 18.2 k, 8 / 8 19.0 k; scripts/queues_probe.py).
            // Priorities other than the default do not help: their queue pools are separate but slower (high:
            // 13.7 k at 8 / 4, 14.4 k at 6 / 6).
            // bgs_set_queue_holders(0) or BGS_QUEUE_HOLDERS=0 in the environment switches this off: a process whose
            // other streams already hold the queues (RCCL's, after a process group was initialised: bench.py's gather
            // path does) is better off without three more co-tenants on them (that path: 18.0 k frames/s without,
            // 13.6 k with). The holders are process-global (one set per device, however many contexts exist).
            {
                std::lock_guard<std::mutex> lock(g_queue_holders_mutex);
                const char* qh_env = std::getenv("BGS_QUEUE_HOLDERS");
                const bool park = g_queue_holders_mode >= 0 ? g_queue_holders_mode != 0 : !(qh_env && qh_env[0] == '0');
                if (park && ctx->device >= 0 && ctx->device < MAX_DEVICES && !g_queue_holders[ctx->device][0])
                    for (auto& qh : g_queue_holders[ctx->device]) HIP_TRY(ctx, hipStreamCreateWithFlags(&qh, hipStreamNonBlocking));
            }
            HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->streams[si], hipStreamNonBlocking));
            // a particle step may still be running on an older stream: the new one starts behind it, like its siblings
            if (ctx->step_done) HIP_TRY(ctx, hipStreamWaitEvent(ctx->streams[si], ctx->step_done, 0));
        }
        L.stream = ctx->streams[si];
    }
    return BGS_OK;
}

int lane_create(bgs_ctx* ctx, Lane& L) {
    if (L.done) return L.stream ? BGS_OK : assign_streams(ctx);
    HIP_TRY(ctx, hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
    for (auto& slot : L.ev_ring)
        for (auto& ev : slot) HIP_TRY(ctx, hipEventCreate(&ev));
    if (!L.h_ctl.reserve(1))
        return fail(ctx, BGS_EHIP, std::string("hipHostMalloc(&h, sizeof(Control), hipHostMallocDefault): ") + hipGetErrorString(hipErrorOutOfMemory));
    std::memset(L.h_ctl.ptr, 0, sizeof(Control));
    void* hd = nullptr;
    HIP_TRY(ctx, hipHostGetDevicePointer(&hd, L.h_ctl.ptr, 0));
    L.h_ctl_dev = (Control*)hd;
    if (!L.d_fp.reserve(1)) return fail(ctx, BGS_ENOMEM, "hipMalloc(frame params) failed");
    return assign_streams(ctx);
}

void graph_destroy(FrameGraph& g) {
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (g.graph) (void)hipGraphDestroy(g.graph);
    g = FrameGraph();
}

void lane_destroy(Lane& L) {
    if (L.stream) (void)hipStreamSynchronize(L.stream);
    for (auto& kind : L.graph)
        for (auto& g : kind) graph_destroy(g);
    for (auto& slot : L.ev_ring)
        for (auto ev : slot) if (ev) (void)hipEventDestroy(ev);
    if (L.done) (void)hipEventDestroy(L.done);
    L = Lane();   // (every buffer frees itself)
}

// (Re)build the zeroed scratch region for n splats and inst_cap instances: both only ever grow.
int ensure_scratch(bgs_ctx* ctx, Lane& L, uint32_t n, uint64_t inst_cap) {
    if (L.scratch.ptr && n <= L.layout.n && inst_cap <= L.layout.inst_cap) return BGS_OK;
    L.layout = scratch_layout(std::max(n, L.layout.n), std::max(inst_cap, L.layout.inst_cap));
    L.scratch_clean = false;
    L.last_ctl = nullptr;   // (it pointed into the old region)
    if (!L.scratch.reserve(L.layout.bytes)) return fail(ctx, BGS_ENOMEM, "hipMalloc(scratch) failed");
    return BGS_OK;
}

// The sort's lists and, with them, the tile rectangles (ensure_rects sizes those by the lists, and GraphKey::bufs does not
// name them: they are released whenever the lists are reallocated).
int ensure_entries(bgs_ctx* ctx, Lane& L, uint32_t n) {
    if (L.entries[0].holds(n) && L.entries[1].holds(n) && L.culled.holds(n)) return BGS_OK;
    L.rects.reset();
    const int failed = reserve_group(n, L.entries[0], L.entries[1], L.culled);
    if (failed < 0) return BGS_OK;
    return fail(ctx, BGS_ENOMEM, failed < 2 ? "hipMalloc(sort entries) failed" : "hipMalloc(culled entries) failed");
}

// BINNING_SCAN renders only: the packed tile rectangle per rank (project_kernel -> bin_kernel)
int ensure_rects(bgs_ctx* ctx, Lane& L) {
    if (!L.rects.reserve(L.entries[0].capacity)) return fail(ctx, BGS_ENOMEM, "hipMalloc(tile rectangles) failed");
    return BGS_OK;
}

int ensure_instances(bgs_ctx* ctx, Lane& L, uint64_t cap) {
    if (reserve_group(cap, L.inst[0], L.inst[1]) >= 0) return fail(ctx, BGS_ENOMEM, "hipMalloc(tile instances) failed");
    return BGS_OK;
}

int ensure_records(bgs_ctx* ctx, Lane& L, size_t bytes) {
    if (!L.records.reserve(bytes, 256)) return fail(ctx, BGS_ENOMEM, "hipMalloc(records) failed");
    return BGS_OK;
}

// Supertile lists: `num_st` lists of `cap` (rank, tile rect) entries each. `cap` follows the longest list
// seen so far (AdaptiveState::list_capacity, never more than n: a list holds each rank at most once); a frame
// that overflows a list is detected when it completes (coarse_total > cap) and re-run with larger lists.
int ensure_coarse(bgs_ctx* ctx, Lane& L, uint32_t n, uint32_t num_st, uint32_t debug_flags, uint32_t* cap_out) {
    const uint32_t n1 = std::max<uint32_t>(n, 1);
    const uint32_t want = ctx->state.list_capacity(n, (debug_flags & BGS_DEBUG_SMALL_LISTS) != 0u);
    const size_t need = (size_t)num_st * want;   // 8-byte entries, all lists together
    // (grown when too small; a lane keeps what it has when the hint falls — a context that alternates between
    // views of different density would otherwise free and allocate every frame)
    if (!L.coarse.holds(2 * need)) {
        if (need * 8u > (64ull << 30))
            return fail(ctx, BGS_ECAPACITY, "coarse bin lists would exceed 64 GiB; use bgs_set_binning(ctx, 1)");
        if (!L.coarse.reserve(2 * need))
            return fail(ctx, BGS_ENOMEM, "hipMalloc(coarse lists) failed: " + std::to_string((need * 8u) >> 20) +
                                             " MiB per lane (8 B x supertiles x longest list); fewer lanes (bgs_set_pipeline_depth) need less");
    }
    // everything that is allocated is used (a lane that grew for an earlier frame keeps its longer lists;
    // not under BGS_DEBUG_SMALL_LISTS, which exists to exercise the overflow path)
    *cap_out = (debug_flags & BGS_DEBUG_SMALL_LISTS) ? want : (uint32_t)std::min<size_t>(L.coarse.capacity / 2 / num_st, n1);
    return BGS_OK;
}

int ensure_bucket_slots(bgs_ctx* ctx, Lane& L, uint32_t sub, bool wide) {
    const uint32_t units = sub * (wide ? BUCKET_CAP_WIDE / BUCKET_CAP : 1u);   // (in narrow subs: 256 * BUCKET_CAP pairs = 8 MB each)
    // (growing frees first, which waits for the device: no frame in flight still uses the old slots)
    if (!L.bucket_slots.reserve((size_t)BUCKET_COUNT * units * BUCKET_CAP)) return fail(ctx, BGS_ENOMEM, "hipMalloc(bucket sort slots) failed");
    return BGS_OK;
}

// The lane's device splitter table and its pinned staging: one without the other is of no use
int ensure_split_keys(bgs_ctx* ctx, Lane& L) {
    if (reserve_group(BUCKET_MAX, L.d_split_keys, L.h_split_keys) >= 0)
        return fail(ctx, BGS_ENOMEM, "hipMalloc / hipHostMalloc(splitter table) failed");
    return BGS_OK;
}

int ensure_heavy(bgs_ctx* ctx, Lane& L, uint32_t tiles) {
    const size_t bytes = heavy_feedback_bytes(tiles);
    TileFeedback& F = L.feedback;
    if (F.heavy[0].holds(bytes)) return BGS_OK;
    // (freeing waits for the device: no frame in flight still reads the old buffers)
    F.forget_heavy();
    if (reserve_group(bytes, F.heavy[0], F.heavy[1]) >= 0) return fail(ctx, BGS_ENOMEM, "hipMalloc(heavy-tile feedback) failed");
    return BGS_OK;
}

// whether the lane's cost planes (and the order made of them) serve a grid of `tiles` as they are
bool cost_holds(const Lane& L, uint32_t tiles) { return L.feedback.cost[0].holds(tile_cost_bytes(tiles) / 2u); }

int ensure_cost(bgs_ctx* ctx, Lane& L, uint32_t tiles) {
    if (cost_holds(L, tiles)) return BGS_OK;
    TileFeedback& F = L.feedback;
    F.forget_cost();
    F.order.reset();
    bool ok = reserve_group(tile_cost_bytes(tiles) / 2u, F.cost[0], F.cost[1]) < 0;
    for (auto& c : F.cost)   // new planes start zeroed
        if (ok && hipMemset(c.ptr, 0, tile_cost_bytes(tiles)) != hipSuccess) { (void)hipGetLastError(); ok = false; }
    if (!ok) {
        for (auto& c : F.cost) c.reset();
        return fail(ctx, BGS_ENOMEM, "hipMalloc(tile cost feedback) failed");
    }
    if (!F.order.reserve(tile_order_bytes(tiles) / 2u)) {
        for (auto& c : F.cost) c.reset();
        return fail(ctx, BGS_ENOMEM, "hipMalloc(tile order) failed");
    }
    return BGS_OK;
}

int ensure_framebuffer(bgs_ctx* ctx, Lane& L, uint32_t w, uint32_t h, bool want8) {
    const size_t px = (size_t)w * h;
    if (!L.fb.reserve(px)) return fail(ctx, BGS_ENOMEM, "hipMalloc(framebuffer) failed");
    if (want8 && !L.fb8.reserve(2 * px)) return fail(ctx, BGS_ENOMEM, "hipMalloc(srgb8 framebuffer) failed");   // room for either packed format (4 or 8 bytes per pixel)
    L.fb_w = w;
    L.fb_h = h;
    return BGS_OK;
}

int validate(bgs_ctx* ctx, const bgs_cloud* cloud, const bgs_view* view, const bgs_settings* s, bool render) {
    if (!ctx) return fail(nullptr, BGS_EINVAL, "ctx is NULL");
    if (!cloud || !view || !s) return fail(ctx, BGS_EINVAL, "cloud, view and settings must be non-NULL");
    if (s->radix_depth_bits != 16 && s->radix_depth_bits != 24 && s->radix_depth_bits != 32)
        return fail(ctx, BGS_EINVAL, "radix_depth_bits must be 16, 24 or 32");
    if (s->gaussian_mode > BGS_GAUSSIAN_3D) return fail(ctx, BGS_EINVAL, "gaussian_mode must be 2D or 3D");
    if (s->sh_degree > 3) return fail(ctx, BGS_EINVAL, "sh_degree must be 0..3");
    if (s->sort_mode > BGS_SORT_STD) return fail(ctx, BGS_EINVAL, "unknown sort_mode");
    if (s->color_space > BGS_COLOR_LINEAR) return fail(ctx, BGS_EINVAL, "unknown color_space");
    if (s->rasterize_mode == BGS_RASTERIZE_VELOCITY)
        return fail(ctx, BGS_EINVAL, "rasterize_mode Velocity is outside the path (4D clouds only)");
    if (s->rasterize_mode == BGS_RASTERIZE_OPTICAL_FLOW && !(view->delta_time > 0.0f))
        return fail(ctx, BGS_EINVAL, "rasterize_mode OpticalFlow needs bgs_view.delta_time > 0");
    if (s->rasterize_mode > BGS_RASTERIZE_VELOCITY) return fail(ctx, BGS_EINVAL, "unknown rasterize_mode");
    if (s->draw_mode > BGS_DRAW_HIGHLIGHT_SELECTED) return fail(ctx, BGS_EINVAL, "unknown draw_mode");
    if (s->rasterize_mode == BGS_RASTERIZE_CLASSIFICATION && s->num_classes == 0)
        return fail(ctx, BGS_EINVAL, "num_classes must be >= 1");
    // whose CloudUniform.min / .max the frame gets (bgs.h: BGS_BOUNDS_*): the caller's, or the cloud's own box
    if (s->reserved[0] > BGS_BOUNDS_CLOUD)
        return fail(ctx, BGS_EINVAL, "bgs_settings.reserved[0] must be BGS_BOUNDS_CALLER (0) or BGS_BOUNDS_CLOUD (1); got " +
                                         std::to_string(s->reserved[0]));
    // the camera's chunk of sorted entries on the device: bgs_sort's second output, bgs_render's draw order
    if (view->entries_device_ptr) {
        if (view->entries_device_ptr % sizeof(bgs_sort_entry) != 0u)
            return fail(ctx, BGS_EINVAL, "bgs_view.entries_device_ptr must be aligned to 8 bytes (one bgs_sort_entry)");
        if (view->entry_count != cloud->ptrs.n)
            return fail(ctx, BGS_EINVAL, "bgs_view.entry_count must equal bgs_cloud_len(cloud) when entries_device_ptr is set; got " +
                                             std::to_string(view->entry_count) + " for a cloud of " + std::to_string(cloud->ptrs.n));
    } else if (view->entry_count != 0u) {
        return fail(ctx, BGS_EINVAL, "bgs_view.entry_count is " + std::to_string(view->entry_count) + " but bgs_view.entries_device_ptr is 0");
    }
    if (render && cloud->ptrs.format == CLOUD_COV3D &&
        (s->gaussian_mode != BGS_GAUSSIAN_3D || s->rasterize_mode == BGS_RASTERIZE_NORMAL))
        return fail(ctx, BGS_EINVAL, "a precomputed-covariance cloud has no rotation / scale: 3D gaussian mode only, no Normal raster mode");
    if (render) {
        // MultisampleState.count = Msaa::samples() (src/render/mod.rs:357-424,975-979): Off and Sample4 are built
        // (0 = "not set": a zero-initialised bgs_view gets Msaa::default() = Sample4, fill_frame_params)
        const uint32_t samples = view->sample_count ? view->sample_count : 4u;
        if (samples != 1u && samples != 2u && samples != 4u && samples != 8u)
            return fail(ctx, BGS_EINVAL, "bgs_view.sample_count must be 1 (Msaa::Off), 2, 4 (Msaa::Sample4, Bevy's default), 8 or 0 (= 4); got " +
                                             std::to_string(view->sample_count));
        if (ctx->tile_trace && (view->depth_device_ptr || s->visualize_bounding_box || samples == 2u || samples == 8u))
            return fail(ctx, BGS_EINVAL, "the per-tile trace (bgs_set_tile_trace) has no instantiation with a depth buffer, the bounding-box "
                                         "overlay or 2 / 8 samples per pixel: a frame would leave the trace buffer untouched");
        if (view->depth_device_ptr % (4u * samples) != 0u)
            return fail(ctx, BGS_EINVAL, "bgs_view.depth_device_ptr must be aligned to one pixel's samples (4 * sample_count bytes)");
        // what depth_device_ptr names (bgs.h: BGS_VIEW_ATTACH_*): the depth plane alone, or the depth and colour planes
        if (view->reserved[0] > BGS_VIEW_ATTACH_COLOR)
            return fail(ctx, BGS_EINVAL, "bgs_view.reserved[0] must be BGS_VIEW_ATTACH_DEPTH_ONLY (0) or BGS_VIEW_ATTACH_COLOR (1); got " +
                                             std::to_string(view->reserved[0]));
        if (view->reserved[0] == BGS_VIEW_ATTACH_COLOR && view->depth_device_ptr == 0ull)
            return fail(ctx, BGS_EINVAL, "bgs_view.reserved[0] is BGS_VIEW_ATTACH_COLOR but bgs_view.depth_device_ptr is 0: the colour plane lies "
                                         "behind a depth plane (all 0.0 for a host without geometry)");
        if (view->reserved[0] == BGS_VIEW_ATTACH_COLOR && view->depth_device_ptr % 16u != 0u)
            return fail(ctx, BGS_EINVAL, "bgs_view.reserved[0] is BGS_VIEW_ATTACH_COLOR: bgs_view.depth_device_ptr must then be aligned to 16 bytes");
        const float w = view->viewport[2], h = view->viewport[3];
        if (!(w >= 1.0f) || !(h >= 1.0f) || w > 4096.0f || h > 4096.0f || w != std::floor(w) || h != std::floor(h))
            return fail(ctx, BGS_EINVAL, "viewport width/height must be integers in [1, 4096]");
    }
    return BGS_OK;
}

// What a completed frame's Control block says about the size of its work: tile instances (BINNING_SCAN: the
// supertile lists' entries) and the longest supertile list.
struct FrameTotals { uint64_t instances = 0; uint32_t longest = 0; };

FrameTotals frame_totals(const FramePlan& p, const Control& h) {
    FrameTotals t;
    t.instances = (uint64_t)h.instance_total_lo | ((uint64_t)h.instance_total_hi << 32);
    if (p.render && p.scan) {
        t.instances = 0;
        for (uint32_t i = 0; i < p.num_st; ++i) {
            t.instances += h.coarse_total[i];
            t.longest = std::max(t.longest, h.coarse_total[i]);
        }
    }
    return t;
}

// finish_lane, step 1: nothing a frame that tripped the device watchdog left behind is trusted: not its counters, not
// the scratch region
int check_watchdog(bgs_ctx* ctx, Lane& L) {
    const Control& h = *L.h_ctl.ptr;
    if (!h.error) return BGS_OK;
    L.scratch_clean = false;
    ctx->state.distrust();
    return fail(ctx, BGS_EINTERNAL, "device watchdog tripped (look-back spin bound), code " + std::to_string(h.error));
}

// finish_lane, step 2: the capacities that depend on the data (the verdicts: adaptive_state.h). *rerun: the frame must be
// run again.
int check_capacities(bgs_ctx* ctx, Lane& L, const FrameTotals& t, int attempt, bool* rerun) {
    const FramePlan& p = L.plan;
    const Control& h = *L.h_ctl.ptr;
    *rerun = false;
    if (p.bucket && ctx->state.learn_bucket_sort(h.sort_overflow, p.split_slot, p.split_epoch)) {
        ctx->reruns_sort += 1;
        L.in.force_passes = true;   // the re-run is on the digit passes, and so is every further attempt of this frame
        *rerun = true;
    }
    if (p.render && p.scan && ctx->state.learn_list_capacity(t.longest, p.level, L.pending_coarse_cap)) {
        ctx->reruns_lists += 1;
        *rerun = true;
    }
    if (p.render && !p.scan && h.overflow) {
        // BINNING_SORT overflow: grow to the next power of two with 25 % headroom (instance_capacity_for, adaptive_state.h)
        const InstanceVerdict grown = instance_capacity_for(t.instances);
        if (grown.refuse)
            return fail(ctx, BGS_ECAPACITY,
                        "frame needs " + std::to_string(t.instances) + " tile instances, above the 2^30 limit");
        int rc = ensure_instances(ctx, L, grown.capacity);
        if (rc != BGS_OK) return rc;
        ctx->reruns_instances += 1;
        *rerun = true;
    }
    // test hook: every BINNING_SCAN frame is run twice, as if a capacity had been too small — exercises the re-run path
    // (same lane, same inputs, the buffers of the first attempt) under any pipeline state
    if ((L.in.debug_flags & BGS_DEBUG_RERUN_EVERY_FRAME) && attempt == 0 && p.render && p.scan) *rerun = true;
    return BGS_OK;
}

// finish_lane, step 3: what the completed frame (its first attempt, if `clean`) teaches the next ones: adaptive_state.h
void learn_from_frame(bgs_ctx* ctx, Lane& L, const FrameTotals& t, bool clean) {
    const FramePlan& p = L.plan;
    const Control& h = *L.h_ctl.ptr;
    AdaptiveState& state = ctx->state;
    const bool scan_render = p.render && p.scan;
    if (scan_render) {
        L.feedback.completed(p, L.in.kind);
        state.learn_saturation(p.sat_kind, h.saturated_tiles_prev);
    }
    state.learn_draw_count(h.draw_count);
    state.store_splitters(h.splitters, p.split_sub_out, p.places, h.draw_count, {L.in.cloud, p.n, &L.in.view, &L.in.settings}, ctx->seq);
    AdaptiveState::LevelVerdict level{false, false};
    if (scan_render && h.visible_count > 0) level = state.learn_level(L.in.kind, p.level, p.edges, t.instances, h.visible_count, t.longest);
    if (level.changed) ctx->level_changes += 1;
    if (scan_render && clean && !level.moved && L.in.kind) state.settle(L.in.kind, p.level);
}

// finish_lane, step 4: the lane's counters of the completed frame
void fill_stats(const bgs_ctx* ctx, Lane& L, const FrameTotals& t) {
    const FramePlan& p = L.plan;
    const Control& h = *L.h_ctl.ptr;
    const bool render = p.render, scan = p.scan;
    bgs_stats& stt = L.result;
    std::memset(&stt, 0, sizeof stt);
    stt.regrow_count = ctx->regrow_count;
    stt.splat_count = p.n;
    stt.visible_count = render ? h.visible_count : h.draw_count;
    stt.draw_count = h.draw_count;
    stt.sort_path = p.kept ? 2u : (p.bucket ? 1u : 0u);
    stt.list_capacity = (render && scan) ? L.pending_coarse_cap : 0u;
    stt.instance_count = render ? t.instances : 0;
    stt.instance_capacity = L.inst[0].capacity;
    stt.list_entries_allocated = (render && scan) ? (uint64_t)(L.coarse.capacity / 2) : 0;
    stt.strip_tiles = (render && scan) ? h.strip_tiles : 0u;
    stt.tile_saturation = (render && scan && p.sat_kind && h.saturated_tiles_prev != 0xFFFFFFFFu)
                              ? (0x10000u | (h.saturated_tiles_prev & 0x7FFFu) | (p.raster.mode != 0 ? 0x80000000u : 0u)) : 0u;
    stt.tiles_x = render ? (uint32_t)p.fp.tiles_x : 0;
    stt.tiles_y = render ? (uint32_t)p.fp.tiles_y : 0;
    stt.depth_passes = p.places;
    stt.tile_passes = (render && !scan) ? 2 : 0;
    stt.binning_mode = scan ? BINNING_SCAN : BINNING_SORT;
    // SURVEY 8(d) algorithmic bytes. SURVEY's bytes_sort is N*16 + N*8 + k*N*16; the partition
    // in keygen means only the D drawable pairs go through the k passes, so that is counted
    // (the bucket sort moves each drawable pair twice: scatter + gather, sorted write: k = 1.5).
    const uint64_t N = p.n, k = p.places, D = h.draw_count;
    // (keygen reads N positions and writes the D drawable pairs; the N - D culled pairs only in frames that
    // have a reader for them)
    uint64_t bytes = N * 16 + D * 8 + (p.culled_tail ? (N - D) * 8 : 0) + (p.bucket ? D * 24 : k * D * 16);
    // a kept order: no positions read, no keys sorted — the N entries of the caller's chunk read, the D drawable ones written
    if (p.kept) bytes = N * 8 + D * 8 + (p.culled_tail ? (N - D) * 8 : 0);
    if (render) {
        const uint64_t B = p.cloud_format == CLOUD_F16 ? 128 : 240, R = p.rec_bytes, V = h.visible_count, I = t.instances;
        const uint64_t P = (uint64_t)(uint32_t)p.fp.width * (uint32_t)p.fp.height;
        if (scan)  // coarse entries (rank + tile rect, 8 B): written once, read by the tiles of their supertile
            bytes += V * (B - 16) + V * R + V * 8 + V * 8 + I * 8 + I * 8 + P * 16;   // (+ the 4-byte tile rect per rank, written by project_kernel and read by bin_kernel)
        else
            bytes += V * (B - 16) + V * R + I * 8 + 2 * I * 16 + I * (4 + R) + P * 16;
        if (attach_has_color(p.fp.depth_ptr)) bytes += P * p.fp.sample_count * 16;   // the colour attachment, read once by the epilogue
    }
    stt.algorithmic_bytes = bytes;
    L.has_result = true;
    L.result_kind = p.ev_kind();
}

// Complete the frame pending on a lane: wait for it, check the watchdog word of the Control copy that
// travelled with the frame, and RE-RUN the frame on its lane if a data-dependent capacity turned out too
// small (a supertile list, the bucket sort's geometry, the tile-instance buffer): nobody has seen the
// frame's output yet, so the caller just gets the correct frame a little later. Fills the lane's stats.
int finish_lane(bgs_ctx* ctx, Lane& L) {
    L.ready = false;
    for (int attempt = 0; L.pending; ++attempt) {
        HIP_TRY(ctx, hipEventSynchronize(L.done));  // not the stream: a sibling lane's frame may be queued behind
        L.pending = false;
        int rc = check_watchdog(ctx, L);
        if (rc != BGS_OK) return rc;
        const FramePlan& p = L.plan;
        const Control& h = *L.h_ctl.ptr;
        const FrameTotals t = frame_totals(p, h);
        bool rerun = false;
        if ((rc = check_capacities(ctx, L, t, attempt, &rerun)) != BGS_OK) return rc;
        if (rerun) {
            if (attempt >= 8) return fail(ctx, BGS_ECAPACITY, "frame kept overflowing its buffers");
            ctx->regrow_count += 1;
            if ((rc = enqueue_frame(ctx, L, L.in)) != BGS_OK) return rc;
            continue;
        }

        learn_from_frame(ctx, L, t, /*clean=*/attempt == 0);

        // after a render only the drawable prefix of the list is materialised (the culled tail stays
        // in its side buffer); bgs_sort appends it so that callers get the reference's full list
        L.last_sorted_n = p.render ? h.draw_count : p.n;
        const bool append_tail = !p.render && h.draw_count < p.n;
        // bgs_sort with the camera's chunk named (bgs_view.entries_device_ptr): the whole list goes there too, on the stream
        const bool to_chunk = !p.render && L.in.view.entries_device_ptr && p.n > 0;
        if (append_tail) {
            // bgs_sort contract: one contiguous list, culled entries last (ascending index)
            HIP_TRY(ctx, hipMemcpyAsync(const_cast<uint2*>(L.last_sorted) + h.draw_count, L.culled.ptr,
                                        (size_t)(p.n - h.draw_count) * sizeof(uint2), hipMemcpyDeviceToDevice, L.stream));
        }
        if (to_chunk)
            HIP_TRY(ctx, hipMemcpyAsync(reinterpret_cast<void*>((uintptr_t)L.in.view.entries_device_ptr), L.last_sorted,
                                        (size_t)p.n * sizeof(uint2), hipMemcpyDeviceToDevice, L.stream));
        // (the chunk is complete when bgs_sort returns: frames of any lane may read it next)
        if (append_tail || to_chunk) HIP_TRY(ctx, hipStreamSynchronize(L.stream));
        fill_stats(ctx, L, t);
    }
    return BGS_OK;
}

// The lane whose frame in flight was enqueued first, or -1. Completing lanes oldest first leaves the stats of the most
// recent frame behind.
int oldest_pending_lane(const bgs_ctx* ctx) {
    int best = -1;
    for (int i = 0; i < MAX_LANES; ++i)
        if (ctx->lanes[i].pending && (best < 0 || ctx->lanes[i].seq < ctx->lanes[best].seq)) best = i;
    return best;
}

int finish_all(bgs_ctx* ctx) {
    for (int i; (i = oldest_pending_lane(ctx)) >= 0;) {
        int rc = finish_lane(ctx, ctx->lanes[i]);
        if (rc != BGS_OK) return rc;
    }
    for (auto& L : ctx->lanes) L.ready = false;
    return BGS_OK;
}

// Build ctx->stats: counters of the most recent frame + per-stage times averaged over every timed
// frame (all lanes) of the same pipeline since the previous call. All lanes must be complete.
int collect_stats(bgs_ctx* ctx) {
    Lane& R = ctx->lanes[ctx->recent];
    if (!R.has_result) return fail(ctx, BGS_EINVAL, "no frame has been run yet");
    ctx->stats = R.result;
    bgs_stats& stt = ctx->stats;
    if (ctx->profiling >= 1) {
        const uint8_t kind = R.result_kind;
        const auto [render, scan, kept] = FramePlan::decode_ev_kind(kind);
        uint32_t used = 0;
        float acc[BGS_STAGE_COUNT] = {0, 0, 0, 0, 0, 0}, acc_total = 0.0f;
        for (auto& L : ctx->lanes) {
            const uint32_t frames = std::min<uint32_t>(L.frames_timed, EV_RING);
            for (uint32_t f = 0; f < frames; ++f) {
                const uint32_t slot = (L.ev_head + EV_RING - f) % EV_RING;
                if (L.ev_kind[slot] != kind) continue;
                hipEvent_t* const ev = L.ev_ring[slot];
                auto ms = [&](StageMark a, StageMark b) { float t = 0; (void)hipEventElapsedTime(&t, ev[a], ev[b]); return t; };
                if (ctx->profiling >= 2) {
                    // (a kept order: the compaction is the whole front end, there is no depth sort)
                    acc[BGS_STAGE_KEYGEN] += kept ? ms(MARK_BEGIN, MARK_SORT) : ms(MARK_BEGIN, MARK_FRONT);
                    acc[BGS_STAGE_DEPTH_SORT] += kept ? 0.0f : ms(MARK_FRONT, MARK_SORT);
                    if (render && scan) {
                        acc[BGS_STAGE_PROJECT] += ms(MARK_SORT, MARK_PROJECT);
                        acc[BGS_STAGE_RASTER] += ms(MARK_PROJECT, MARK_RASTER);
                    } else if (render) {
                        acc[BGS_STAGE_PROJECT] += ms(MARK_SORT, MARK_PROJECT);
                        acc[BGS_STAGE_TILE_SORT] += ms(MARK_PROJECT, MARK_TILE_SORT);
                        acc[BGS_STAGE_RANGES] += ms(MARK_TILE_SORT, MARK_RANGES);
                        acc[BGS_STAGE_RASTER] += ms(MARK_RANGES, MARK_RASTER);
                    }
                }
                acc_total += ms(MARK_BEGIN, last_mark(render));
                ++used;
            }
            L.frames_timed = 0;
        }
        if (used) {
            for (int i = 0; i < BGS_STAGE_COUNT; ++i) stt.stage_ms[i] = acc[i] / (float)used;
            stt.total_ms = acc_total / (float)used;
        }
        stt.frames_averaged = used;
    }
    ctx->have_stats = true;
    return BGS_OK;
}

// Every choice of one frame, from its inputs and the context's learnt state. Allocates nothing and changes no state.
FramePlan plan_frame(const bgs_ctx& ctx, const Lane& L, const FrameInputs& in) {
    FramePlan p;
    const AdaptiveState& state = ctx.state;
    const TileFeedback& F = L.feedback;
    const uint32_t flags = in.debug_flags;
    const bgs_settings* s = &in.settings;
    FrameParams& fp = p.fp;
    fill_frame_params(in.cloud->ptrs.n, &in.view, s, fp);
    if (in.cloud_bounds) {   // BGS_BOUNDS_CLOUD: the caller's position_min / _max are ignored
        std::memcpy(fp.pos_min, in.pos_min, sizeof fp.pos_min);
        std::memcpy(fp.pos_max, in.pos_max, sizeof fp.pos_max);
    }
    fp.debug = flags;
    fp.srgb8_target = (uint64_t)(uintptr_t)in.srgb8_target;
    const uint32_t n = p.n = fp.n;
    p.render = in.render;
    // A kept order (bgs_view.entries_device_ptr on a render): the caller's entries are the draw order. No keys, no digit
    // places, no bucket sort, no splitter table read or left (store_splitters wants 4 places): sort_mode and
    // radix_depth_bits do not reach such a frame.
    p.kept = in.render && in.view.entries_device_ptr != 0u && fp.n > 0u;
    p.places = p.kept ? 0u : depth_places(s);
    p.scan = ctx.binning == BINNING_SCAN;
    p.cloud_format = in.cloud->ptrs.format;
    p.project = project_instantiation(fp, p.cloud_format);
    p.surfel = in.render && p.project.surfel;
    p.rec_bytes = p.surfel ? sizeof(RecordSurfel) : sizeof(Record);
    // The culled tail (index order, 8 B per culled splat: 7 of the 24 MB keygen moves on the headline frame) has two
    // readers: bgs_sort's full list and RasterizeMode::Depth (sorted[N-1] of the full list, gaussian.wgsl:331-340).
    // Every other rendered frame skips the writes; bgs_sorted_entries_device_ptr after a render has always meant the
    // drawable prefix only.
    // (a kept order: the skipped entries, in list order, for the same reader)
    p.culled_tail = !in.render || s->rasterize_mode == BGS_RASTERIZE_DEPTH;

    // Depth-sort path. The bucket sort needs 32-bit keys (shorter keys are mostly ties, which it ranks
    // quadratically), a draw count that fits its geometry (a bucket holds <= BUCKET_CAP pairs) and the key
    // range of a recent frame; it is checked on the device and the frame re-run with the digit passes when
    // it does not work out (then bucket_block keeps the following frames on the passes for a while).
    const bool hint = state.draw_hint_valid;
    const int slot = (p.places == 4 && n > 0) ? state.find_splitter_slot({in.cloud, n, &in.view, s}) : -1;
    // Geometry: NARROW buckets (BUCKET_CAP pairs, 256-thread workgroups) while 256 * BUCKET_SUB_KERNARG of them at BUCKET_TARGET
    // pairs hold the list (1.57 M pairs: every frame of the headline's kind), WIDE ones (BUCKET_CAP_WIDE, 1024 threads, 128 KB
    // of LDS) past that: a 5 M-pair list is 768 wide buckets instead of 2816 narrow ones, which keygen's scatter reached with
    // 1.5 pairs per (tile, bucket).
    const uint32_t narrow_max = BUCKET_COUNT * BUCKET_SUB_KERNARG * BUCKET_TARGET;
    p.wide = (hint && state.draw_hint > narrow_max && !(flags & BGS_DEBUG_BUCKETS_NARROW)) || (flags & BGS_DEBUG_BUCKETS_WIDE);
    const uint32_t cap_out = p.wide ? BUCKET_CAP_WIDE : BUCKET_CAP, target_out = p.wide ? BUCKET_TARGET_WIDE : BUCKET_TARGET;
    p.bucket = p.places == 4 && n > 0 && !(flags & BGS_DEBUG_NO_BUCKET_SORT) && state.bucket_block == 0 && !in.force_passes &&
               ((slot >= 0 && hint) || (flags & BGS_DEBUG_GUESSED_SPLITTERS)) &&
               (!hint || state.draw_hint <= BUCKET_MAX * (cap_out / 4u) * 3u);
    // Buckets: 256 * sub, as many as keep a bucket near its target (narrow: sub = 1 up to 524 k drawable pairs — the
    // headline's 120 k —, 2 at 1 M, 3 at 1.5 M; wide: 1 up to 2.1 M, 3 at 5 M, 16 up to 50 M). A frame sorts with the table
    // its slot HOLDS (table.sub), in the geometry the hint asks for: a table that is too coarse for the list in that
    // geometry is not used, and every completed frame leaves a table of the sub the current hint asks for (split_sub_out).
    if (hint)
        p.split_sub_out = std::min<uint32_t>(std::max<uint32_t>((state.draw_hint + BUCKET_COUNT * target_out - 1u) / (BUCKET_COUNT * target_out), 1u), BUCKET_SUB_MAX);
    if (flags & BGS_DEBUG_SPLIT_SUB_3) p.split_sub_out = std::max<uint32_t>(p.split_sub_out, BUCKET_SUB_KERNARG);
    if (flags & BGS_DEBUG_SPLIT_SUB_5) p.split_sub_out = std::max<uint32_t>(p.split_sub_out, 5u);
    if (p.bucket && slot >= 0) {
        p.bucket_sub = std::min<uint32_t>(std::max<uint32_t>(state.split_slots[slot].table.sub, 1u), BUCKET_SUB_MAX);
        if (hint && state.draw_hint > BUCKET_COUNT * p.bucket_sub * (cap_out / 4u) * 3u) p.bucket = false;   // too coarse a table
    }
    if (p.bucket && slot >= 0) { p.split_slot = slot; p.split_epoch = state.split_slots[slot].epoch; }
    fp.sort_path = p.bucket ? 1u : 0u;
    if (p.kept) { fp.sort_mode = SORT_NONE; fp.key_shift = 0u; }   // (what the frame is to its kernels: a list drawn in entry order)

    // Supertile edge (in tiles): four levels (supertile_edges, frame_params.h). Every tile scans its supertile's whole
    // list, so small splats want short lists (level 0: scene-like frame 91.7 -> 87.9 us against level 1); a splat that
    // spans many supertiles costs one list entry, one append and a share of the ballots in each, while a tile that
    // saturates after ~60 hits does not mind scanning three times as many candidates (dense frame, 6 lanes on 3 streams:
    // 13.3 k frames/s at level 1, 14.6 k at level 2, 15.3 k at level 3). Images do not depend on the level; it follows
    // the entries-per-visible-splat ratio of the completed frames (finish_lane) unless a debug flag forces one.
    supertile_edges((uint32_t)fp.tiles_x, (uint32_t)fp.tiles_y, p.edges);
    uint32_t level = state.sup_level;
    if (flags & BGS_DEBUG_LEVEL_0) level = 0;
    else if (flags & BGS_DEBUG_LEVEL_1) level = 1;
    else if (flags & BGS_DEBUG_LEVEL_2) level = 2;
    else if (flags & BGS_DEBUG_LEVEL_3) level = 3;
    p.level = canonical_supertile_level(level, p.edges);
    // tile / edge by reciprocal multiply is exact for edges <= 32 (supertile_div)
    p.sup_edge = supertile_bins_fit((uint32_t)fp.tiles_x, (uint32_t)fp.tiles_y, p.edges[p.level]) ? p.edges[p.level] : p.edges[1];
    p.num_st = (((uint32_t)fp.tiles_x + p.sup_edge - 1) / p.sup_edge) * (((uint32_t)fp.tiles_y + p.sup_edge - 1) / p.sup_edge);

    // Grids: only the D drawable entries are sorted, and D is known on the device only; launching a block per N/tile
    // would start ~6x more blocks than tiles, each queueing for a ticket just to leave. Project grid: one block per 256
    // ranks of the D drawable entries when that fits the chip (two 170-190-VGPR blocks are resident per CU; the kernel
    // strides over the rest); bin grid: one block per 1024 ranks (every block then takes exactly one ticket).
    p.large = n > (4u << 20);
    p.wide_bin = ctx.depth == 1;
    p.sort_blocks = ctx.num_cus * 4;
    p.bin_blocks = ctx.num_cus * 3;
    p.binning_blocks = ctx.num_cus * 4;
    if (hint && !(flags & BGS_DEBUG_NO_DRAW_HINT)) {
        const uint64_t want = (uint64_t)state.draw_hint / sort_tile_size(p.large) + 8;
        p.sort_blocks = (int)std::min<uint64_t>((uint64_t)p.sort_blocks, std::max<uint64_t>(want, 32));
        p.bin_blocks = (int)std::min<uint64_t>((uint64_t)p.bin_blocks, std::max<uint64_t>((uint64_t)state.draw_hint / 256 + 8, 32));
        p.binning_blocks = (int)std::min<uint64_t>((uint64_t)p.binning_blocks, std::max<uint64_t>((uint64_t)state.draw_hint / 1024 + 4, 16));
    }
    p.front_blocks = ctx.num_cus * 4;
    p.emit_blocks = ctx.num_cus * 3;
    p.tile_sort_blocks = ctx.num_cus * 4;
    // bgs_set_grid_cap (test hook): every persistent launch with at most that many workgroups, so that they come back for
    // further tiles. The grids are in GraphKey: a frame under another cap is captured anew.
    for (int* blocks : {&p.sort_blocks, &p.bin_blocks, &p.binning_blocks, &p.front_blocks, &p.emit_blocks, &p.tile_sort_blocks})
        *blocks = grid_under_cap(*blocks, in.grid_cap);
    p.want_srgb8 = in.render && (in.output_srgb8 || in.output_rgba16f || in.srgb8_target);
    p.out_format = !p.want_srgb8 ? 0u : ((in.output_rgba16f ? OUT_RGBA16F : OUT_SRGB8) |
                                         ((in.packed_only && p.scan) ? OUT_SKIP_F32 : 0u));

    // Rasteriser (raster_instantiation, frame_params.h): the mid-round exit for dense frames (supertile level >= 2), and
    // for frames of a kind whose saturating tiles hold a good share of the work (KindState::midround, from the cost planes)
    // when several frames are in flight: the trained-like 1 M frame 5.75 -> 6.31 k frames/s with 8 lanes, but ALONE on the
    // chip its launch ends with its longest lists' serial chains, which do not saturate and only pay the checks (231 -> 272 us)
    p.raster_cleans = in.render && p.scan && fp.tiles_x > 0 && fp.tiles_y > 0 && !(flags & BGS_DEBUG_NO_RASTER_CLEANUP);
    const bool kind_midround = ctx.depth > 1 && state.midround(in.kind);
    p.raster = raster_instantiation(fp, p.level, kind_midround, ctx.depth, flags, ctx.tile_trace != nullptr);
    p.ntiles = (uint32_t)(fp.tiles_x * fp.tiles_y);
    // the feedback buffers alternate with every completed frame: not under frame graphs
    const bool feedback = p.raster_cleans && !(in.allow_graph && ctx.use_graphs) && p.ntiles <= 65535u;
    // Dense frames (the mid-round exit at supertile level >= 2) leave, and use, the heavy-tile feedback (kernels.h
    // HeavyFeedback) — when ONE frame is in flight (pipeline depth 1): the strip workgroups cut the launch's tail (dense
    // 1 M frame: raster 49.4 -> 45.3 us, the heaviest tiles' serial chains split four ways), but with several frames in
    // flight that tail is filled by the other lanes' kernels anyway and the extra workgroups and the flag load only cost
    // (20.6 -> 20.0 k frames/s with 8 lanes; profiles/r3_notes.md). Not with the tile trace.
    p.heavy = feedback && p.raster.mode == 1 && p.level >= 2u && !p.raster.trace &&
              (ctx.depth == 1 || (flags & BGS_DEBUG_STRIPS_ANY_DEPTH)) && !(flags & BGS_DEBUG_NO_STRIPS);
    // Tile costs (kernels.h TileCost): every BINNING_SCAN frame leaves them, and a frame with more tile waves than the
    // chip holds at once draws its raster workgroups in the order made of a completed frame's costs; the tile trace shows
    // it. Unlike the heavy-tile strips it pays with frames in flight too, if little (+0.6 % dense, +0.9 % surfel
    // frames/s; alone on the chip 6-21 % of the rasteriser's time).
    p.cost = feedback && (ctx.depth == 1 || !(flags & BGS_DEBUG_NO_TILE_COST_PIPELINED)) && !(flags & BGS_DEBUG_NO_TILE_COST);
    if (p.cost && p.ntiles > (uint32_t)(ctx.num_cus * 4 * p.raster.waves_per_simd())) {
        // F.order holds a permutation of this grid's workgroups from the moment it was first made for the grid
        // (order_grid); it is made again from the newest completed costs every TILE_ORDER_REFRESH-th frame. (ensure_cost
        // keeps the lane's buffers, and what they hold, unless the grid outgrew them.)
        const uint32_t grid = tile_grid_word(fp);
        const bool kept = cost_holds(L, p.ntiles);
        const bool have_costs = kept && F.cost_done && F.cost_done != F.cost[F.cost_parity].ptr && F.cost_done_grid == grid;
        const bool have_order = kept && F.order_grid == grid;
        p.refresh = have_costs && (!have_order || F.order_age + 1u >= TILE_ORDER_REFRESH || (flags & BGS_DEBUG_ORDER_EVERY_FRAME));
        p.ordered = p.refresh || have_order;
    }
    // (a frame that makes the order makes its saturation counts anew, ahead of its own kernels)
    p.sat_kind = !p.ordered ? 0 : (p.refresh ? F.cost_done_kind : F.order_kind);
    // ---- opt-in (bgs_set_graphs): a steady-state BINNING_SCAN frame as a hipGraph, captured once per
    // (lane, Control parity), then replayed with ONE node update — keygen's arguments carry the new
    // FrameParams, every other kernel reads them from the copy keygen leaves in device memory.
    // Measured: 7 launches cost 19 us of host time (30 us with stage events), a replay 10 us; on the
    // GPU a replayed frame is ~5 % SLOWER than the same launches issued directly (178 vs 171 us per
    // frame back to back on one stream), so it is for hosts that cannot spare the CPU time.
    // A kept-order frame is a graph of its own kind (Lane::graph): the compaction stands in keygen's place as the updated
    // node, and its arguments carry the caller's chunk as well. (It is never a bucket frame: p.bucket_sub stays 1.)
    p.graph_ok = in.allow_graph && ctx.use_graphs && p.raster_cleans && p.bucket_sub <= BUCKET_SUB_KERNARG &&
                 !(flags & BGS_DEBUG_NO_GRAPHS) && !p.raster.trace;
    return p;
}

// The buffers a planned frame needs (allocated or grown); *coarse_cap: the entries per supertile list it gets.
int ensure_frame_buffers(bgs_ctx* ctx, Lane& L, const FramePlan& p, const FrameInputs& in, uint32_t* coarse_cap) {
    int rc;
    if ((rc = lane_create(ctx, L)) != BGS_OK) return rc;
    if ((rc = ensure_entries(ctx, L, p.n)) != BGS_OK) return rc;
    if (p.bucket && p.bucket_sub > BUCKET_SUB_KERNARG && (rc = ensure_split_keys(ctx, L)) != BGS_OK) return rc;
    if (p.bucket && (rc = ensure_bucket_slots(ctx, L, p.bucket_sub, p.wide)) != BGS_OK) return rc;
    if (p.render) {
        if (p.scan) {
            if ((rc = ensure_coarse(ctx, L, p.n, p.num_st, in.debug_flags, coarse_cap)) != BGS_OK) return rc;
            if ((rc = ensure_rects(ctx, L)) != BGS_OK) return rc;
        } else {
            if ((rc = ensure_instances(ctx, L, std::max<uint64_t>(L.inst[0].capacity, MIN_INSTANCE_CAPACITY))) != BGS_OK) return rc;
        }
        if ((rc = ensure_records(ctx, L, (size_t)p.n * p.rec_bytes)) != BGS_OK) return rc;
        if ((rc = ensure_framebuffer(ctx, L, (uint32_t)p.fp.width, (uint32_t)p.fp.height, in.output_srgb8 || in.output_rgba16f)) != BGS_OK) return rc;
    }
    if ((rc = ensure_scratch(ctx, L, p.n, L.inst[0].capacity)) != BGS_OK) return rc;
    if (p.heavy && (rc = ensure_heavy(ctx, L, p.ntiles)) != BGS_OK) return rc;
    if (p.cost && (rc = ensure_cost(ctx, L, p.ntiles)) != BGS_OK) return rc;
    return BGS_OK;
}

// Step 3 of enqueue_frame: the frame's device memory (FrameBindings, bgs_context.h). The one place that does arithmetic on
// the lane's scratch region and that says which buffer is which argument of which stage. No HIP call, no change of state.
FrameBindings bind_frame(const Lane& L, const FramePlan& p, const FrameInputs& in, uint32_t coarse_cap, uint4* tile_trace) {
    FrameBindings b;
    const FrameParams& fp = p.fp;
    const ScratchLayout& lay = L.layout;
    uint8_t* const scratch = L.scratch.ptr;
    Control* const ctl = b.ctl = (Control*)(scratch + (L.ctl_parity ? lay.off_ctl1 : 0));
    b.part_status = (uint32_t*)(scratch + lay.off_part_status);
    b.depth_status = (uint32_t*)(scratch + lay.off_depth_status);
    b.ranges = (uint2*)(scratch + lay.off_ranges);
    b.draw_list = L.entries[p.places & 1u].ptr;
    b.final_xor = (fp.sort_mode == BGS_SORT_RAYON || fp.sort_mode == BGS_SORT_STD) ? 0xFFFFFFFFu : 0u;
    const TileFeedback& F = L.feedback;
    b.cost_in = p.refresh ? F.cost_done : nullptr;
    b.tile_order = p.ordered ? F.order.ptr : nullptr;
    b.bucket_slots = L.bucket_slots.ptr;
    b.split_keys = L.d_split_keys.ptr;
    b.split_keys_staging = L.h_split_keys.ptr;
    b.d_fp = L.d_fp.ptr;
    b.fb = L.fb.ptr;
    b.fb8 = L.fb8.ptr;
    if (!p.bucket && p.places > 0) {
        // only the V' drawable entries are sorted; the culled tail is already in its final order
        OnesweepLaunch& d = b.depth;
        d.lists[0] = L.entries[0].ptr; d.lists[1] = L.entries[1].ptr;
        d.n_ptr = &ctl->draw_count; d.max_n = p.n;
        d.hist = ctl->hist_depth; d.status = b.depth_status; d.status_stride = lay.pass_stride;
        d.ctl = ctl; d.first_ticket = TICKET_DEPTH; d.passes = p.places; d.final_xor = b.final_xor; d.large_tiles = p.large;
        d.prepare(p.sort_blocks);
    }
    if (p.render && p.scan) {
        ProjectLaunch& v = b.project;
        v.inst = p.project; v.d_fp = b.d_fp; v.cloud = in.cloud->ptrs; v.draw_list = b.draw_list; v.culled = L.culled.ptr;
        v.ctl = ctl; v.records = L.records.ptr; v.rects = L.rects.ptr;
        v.prepare(p.n, p.bin_blocks);
        BinLaunch& bin = b.bin;
        bin.rects = L.rects.ptr; bin.ctl = ctl; bin.bin_status = (uint32_t*)(scratch + lay.off_bin_status);
        bin.coarse = L.coarse.ptr; bin.coarse_cap = coarse_cap; bin.sup_edge = p.sup_edge;
        bin.tiles_x = (uint32_t)fp.tiles_x; bin.tiles_y = (uint32_t)fp.tiles_y; bin.wide = p.wide_bin;
        bin.prepare(p.n, p.binning_blocks);
        RasterScanLaunch& r = b.raster_scan;
        r.inst = p.raster; r.d_fp = b.d_fp; r.tiles_x = bin.tiles_x; r.tiles_y = bin.tiles_y;
        r.records = L.records.ptr; r.coarse = L.coarse.ptr; r.coarse_cap = coarse_cap; r.sup_edge = p.sup_edge;
        r.ctl = ctl; r.framebuffer = b.fb; r.srgb8_default = b.fb8;
        r.out_format = (in.debug_flags & BGS_DEBUG_SEPARATE_ENCODE) ? 0u : p.out_format;
        r.tile_trace = tile_trace;
        // (p.heavy, p.cost and p.ordered are of BINNING_SCAN renders only: plan_frame)
        r.heavy_out = p.heavy ? F.heavy[F.heavy_parity].ptr : nullptr;
        r.heavy_in = (p.heavy && F.heavy_done && F.heavy_done != r.heavy_out && F.heavy_done_grid == tile_grid_word(fp)) ? F.heavy_done : nullptr;
        r.cost_out = p.cost ? F.cost[F.cost_parity].ptr : nullptr;
        r.order = b.tile_order;
        if (p.raster_cleans) {
            FrameCleanup& cl = r.cleanup;
            cl.part_status = b.part_status;
            cl.depth_status = b.depth_status;
            cl.bin_status = bin.bin_status;
            cl.other_ctl = (Control*)(scratch + (L.ctl_parity ? 0 : lay.off_ctl1));
            cl.host_ctl = L.h_ctl_dev;
            cl.pass_stride = lay.pass_stride;
            cl.places = p.bucket ? 0u : p.places;
            cl.depth_tile = sort_tile_size(p.large);
            cl.sorted = b.draw_list;
            cl.key_xor = b.final_xor;
            cl.split_sub = p.split_sub_out;
            if (b.tile_order) cl.order_stats = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(b.tile_order) + tile_order_stats_offset(p.ntiles));
        }
    } else if (p.render) {
        const uint32_t capacity = (uint32_t)std::min<uint64_t>(L.inst[0].capacity, MAX_INSTANCE_CAPACITY);
        ProjectEmitLaunch& v = b.project_emit;
        v.fp = &fp; v.inst = p.project; v.cloud = in.cloud->ptrs; v.draw_list = b.draw_list; v.culled = L.culled.ptr;
        v.ctl = ctl; v.scan_status = (unsigned long long*)(scratch + lay.off_scan_status);
        v.records = L.records.ptr; v.instances = L.inst[0].ptr; v.capacity = capacity;
        v.prepare(p.emit_blocks);
        OnesweepLaunch& t = b.tile_sort;
        t.lists[0] = L.inst[0].ptr; t.lists[1] = L.inst[1].ptr;
        t.n_ptr = &ctl->instance_count; t.max_n = capacity;
        t.hist = ctl->hist_tile; t.status = (uint32_t*)(scratch + lay.off_tile_status); t.status_stride = (size_t)lay.inst_tiles * RADIX_BASE;
        t.ctl = ctl; t.first_ticket = TICKET_TILE; t.passes = 2u; t.large_tiles = true;
        t.prepare(p.tile_sort_blocks);
        RasterLaunch& r = b.raster;
        r.fp = &fp; r.inst = p.raster; r.records = L.records.ptr; r.instances = L.inst[0].ptr; r.ranges = b.ranges;
        r.framebuffer = b.fb; r.clear_color = in.view.clear_color; r.ctl = ctl;
    }
    return b;
}

// The front end of a sorting frame: keygen on the frame's bindings, with the splitter table of a bucket frame's slot (a long
// one goes through the lane's pinned staging: the lane's previous frame is complete, nobody reads it). false: nothing to launch.
bool prepare_keygen(const bgs_ctx& ctx, const FramePlan& p, const FrameInputs& in, const FrameBindings& b, uint2* entries, uint2* culled, KeygenLaunch& kg) {
    kg.fp = p.fp;
    kg.pos = in.cloud->ptrs.position_visibility;
    kg.entries = entries;
    kg.culled = p.culled_tail ? culled : nullptr;
    kg.ctl = b.ctl;
    kg.part_status = b.part_status;
    kg.places = p.places;
    kg.ticket_slot = TICKET_FRONT;
    kg.fp_out = b.d_fp;
    kg.zero_word = reinterpret_cast<uint32_t*>(b.raster_scan.heavy_out);   // keygen, the frame's first kernel, zeroes the heavy-tile list's count
    kg.bucket_slots = b.bucket_slots;
    kg.bucket_status = b.depth_status;  // the depth passes' look-back words are free in a bucket-sort frame
    if (p.bucket) {
        if (p.split_slot >= 0) {
            const SplitterKeys& tk = ctx.state.split_slots[p.split_slot].table;
            const uint32_t nkeys = BUCKET_COUNT * p.bucket_sub - 1u;
            std::memcpy(p.bucket_sub <= BUCKET_SUB_KERNARG ? kg.split.key : b.split_keys_staging, tk.key, nkeys * sizeof(uint32_t));
            kg.split.device_keys = b.split_keys;
        } else {  // BGS_DEBUG_GUESSED_SPLITTERS: equal steps over the 32-bit range (badly balanced)
            for (uint32_t i = 0; i < BUCKET_COUNT; ++i) kg.split.key[i] = (i + 1u) << 24;
        }
        kg.split.sub = p.bucket_sub;
        kg.split.wide = p.wide ? 1u : 0u;
    }
    kg.wide = p.wide_bin;
    return kg.prepare(p.front_blocks);
}

// The front end of a kept-order frame: the compaction in keygen's place, leaving what keygen leaves (entries_kernels.hip)
bool prepare_compact(const FramePlan& p, const FrameInputs& in, const FrameBindings& b, uint2* culled, EntriesLaunch& ek) {
    ek.fp = p.fp;
    ek.entries = reinterpret_cast<const uint2*>((uintptr_t)in.view.entries_device_ptr);
    ek.draw_list = b.draw_list;
    ek.tail = p.culled_tail ? culled : nullptr;
    ek.ctl = b.ctl;
    ek.part_status = b.part_status;
    ek.ticket_slot = TICKET_FRONT;
    ek.fp_out = b.d_fp;
    ek.zero_word = reinterpret_cast<uint32_t*>(b.raster_scan.heavy_out);
    return ek.prepare(in.grid_cap);
}

// The stage events of one frame on its stream: all of them, the first and the last only (profiling level 1), or none
struct StageMarks {
    hipEvent_t* ev; hipStream_t st; int prof; StageMark last;
    void operator()(StageMark m) const { if (prof >= 2 || (prof == 1 && (m == MARK_BEGIN || m == last))) (void)hipEventRecord(ev[m], st); }
};

// Step 4 of enqueue_frame: what enqueueing the frame changes in the context's and the lane's state, and the ring slot of
// a timed frame's events (untimed frames do not consume one).
StageMarks commit_frame(bgs_ctx* ctx, Lane& L, const FramePlan& p) {
    ctx->state.frame_enqueued(p.places, p.split_slot, ctx->seq + 1);   // (split_slot: of a bucket frame only)
    L.feedback.enqueued(p);
    if (p.bucket) ctx->bucket_frames += 1;
    else if (p.places > 0) ctx->onesweep_frames += 1;
    if (p.cost) ctx->cost_frames += 1;
    if (p.ordered) ctx->ordered_frames += 1;
    if (p.refresh) ctx->order_refreshes += 1;
    const bool timed_frame = (ctx->frame_counter++ % ctx->profiling_stride) == 0;
    const int prof = timed_frame ? ctx->profiling : 0;
    if (prof) {
        L.ev_head = (L.ev_head + 1) % EV_RING;
        L.ev_kind[L.ev_head] = p.ev_kind();
        L.frames_timed += 1;
    }
    return {L.ev_ring[L.ev_head], L.stream, prof, last_mark(p.render)};
}

// Step 5 of enqueue_frame: the launches of one frame, in stream order (issued directly, or once into a stream capture).
// front: the prepared keygen or compaction, null if there is nothing to launch (an empty cloud).
template <class Front>
hipError_t issue_frame(hipStream_t st, const FramePlan& p, const FrameBindings& b, Front* front, const StageMarks& mark) {
    mark(MARK_BEGIN);
    if (b.cost_in) launch_tile_order(st, b.cost_in, b.tile_order, p.ntiles, p.raster);   // (counted with the frame's first stage)
    if (front) {
        if (p.bucket && p.bucket_sub > BUCKET_SUB_KERNARG) {
            const hipError_t ce = hipMemcpyAsync(b.split_keys, b.split_keys_staging, (BUCKET_COUNT * p.bucket_sub - 1u) * sizeof(uint32_t),
                                                 hipMemcpyHostToDevice, st);
            if (ce != hipSuccess) return ce;
        }
        const hipError_t e = front->launch(st);
        if (e != hipSuccess) return e;
    }
    mark(MARK_FRONT);
    if (p.bucket) {
        const hipError_t e = launch_bucket_sort(st, b.bucket_slots, b.draw_list, b.ctl, b.final_xor, BUCKET_COUNT * p.bucket_sub, p.wide);
        if (e != hipSuccess) return e;
    }
    b.depth.launch(st);
    mark(MARK_SORT);
    if (p.render && p.scan) {
        hipError_t e = b.project.launch(st);
        if (e != hipSuccess) return e;
        b.bin.launch(st);
        mark(MARK_PROJECT);
        e = b.raster_scan.launch(st);
        if (e != hipSuccess) return e;
        mark(MARK_RASTER);
    } else if (p.render) {
        hipError_t e = b.project_emit.launch(st);
        if (e != hipSuccess) return e;
        mark(MARK_PROJECT);
        b.tile_sort.launch(st);
        mark(MARK_TILE_SORT);
        launch_tile_ranges(st, b.raster.instances, b.ctl, b.ranges);
        mark(MARK_RANGES);
        e = b.raster.launch(st);
        if (e != hipSuccess) return e;
        mark(MARK_RASTER);
    }
    // BINNING_SCAN frames get their sRGB8 image from the rasteriser itself (BGS_DEBUG_SEPARATE_ENCODE: from the
    // separate encode pass, for A/B runs)
    if (p.want_srgb8 && !(p.render && p.scan && !(p.fp.debug & BGS_DEBUG_SEPARATE_ENCODE)))
        launch_encode_srgb8(st, b.fb, b.fb8, (uint32_t)p.fp.width * (uint32_t)p.fp.height, b.d_fp, p.out_format);
    return hipGetLastError();
}

// What the launches of a captured frame depend on besides FrameParams: the plan's choices and the buffers they were
// bound to. Nothing that changes from frame to frame (the splitter slot, its epoch, a kept order's chunk: the front node's
// update carries them). `front`: the prepared KeygenLaunch or EntriesLaunch, whose kernel and grid the node keeps.
template <class Front>
GraphKey graph_key(const FramePlan& p, const FrameInputs& in, const Lane& L, const FrameBindings& b, const Front& front) {
    GraphKey key;
    std::memset(&key, 0, sizeof key);
    const FrameParams& fp = p.fp;
    const void* planes[6] = {in.cloud->ptrs.position_visibility, in.cloud->ptrs.packed, nullptr, nullptr, nullptr, nullptr};
    std::memcpy(key.cloud, planes, sizeof planes);
    const void* bufs[11] = {L.entries[0].ptr, L.entries[1].ptr, L.culled.ptr, L.records.ptr, L.coarse.ptr, L.fb.ptr, L.fb8.ptr,
                            L.scratch.ptr, L.d_fp.ptr, L.h_ctl_dev, L.bucket_slots.ptr};   // (L.rects lives and dies with L.entries: ensure_entries)
    std::memcpy(key.bufs, bufs, sizeof bufs);
    key.n = p.n; key.places = p.places; key.sort_mode = in.settings.sort_mode;
    key.project = p.project.key(); key.raster = p.raster.key(); key.srgb8 = p.out_format;
    key.debug_flags = in.debug_flags;
    key.width = fp.width; key.height = fp.height;
    key.sort_blocks = p.bucket ? 0 : p.sort_blocks;  // the bucket sort's grid is fixed
    key.bin_blocks = p.bin_blocks * 4096 + p.binning_blocks;   // (the bin kernel's shape follows the pipeline depth, as keygen's does: key.front_threads)
    key.front_blocks = (int32_t)front.blocks; key.front_func = front.func; key.front_threads = front.threads;   // (kept: entries_blocks(n) of the compaction)
    key.wide_bin = p.wide_bin ? 1u : 0u;
    key.split_sub = p.split_sub_out;   // (round 5's advisor: a replay across a 524 k-pair step of the hint left a table of the captured sub under the new sub's label)
    key.sup_edge = p.sup_edge;
    key.scratch = L.layout;
    key.coarse_cap = b.raster_scan.coarse_cap;
    key.sort_path = p.bucket ? (p.bucket_sub | (p.wide ? 0x100u : 0u)) : 0u;   // (the bucket sort's grid and instantiation and keygen's dynamic LDS follow it)
    return key;
}

// Replay the graph G of this key (its front node updated to this frame), or capture the frame's launches into a new one.
template <class Front>
int launch_graph(bgs_ctx* ctx, Lane& L, FrameGraph& G, const GraphKey& key, Front& front, const FramePlan& p, const FrameBindings& b, const StageMarks& mark) {
    if (G.exec && std::memcmp(&G.key, &key, sizeof key) == 0) {
        HIP_TRY(ctx, front.update_node(G.exec, G.front_node));
        ctx->graph_replays += 1;
    } else {
        graph_destroy(G);
        HIP_TRY(ctx, hipStreamBeginCapture(L.stream, hipStreamCaptureModeThreadLocal));
        const hipError_t ie = issue_frame(L.stream, p, b, &front, mark);
        const hipError_t ce = hipStreamEndCapture(L.stream, &G.graph);
        size_t roots = 1;
        if (ie != hipSuccess || ce != hipSuccess || !G.graph ||
            hipGraphInstantiate(&G.exec, G.graph, nullptr, nullptr, 0) != hipSuccess ||
            hipGraphGetRootNodes(G.graph, &G.front_node, &roots) != hipSuccess || roots != 1) {
            graph_destroy(G);
            (void)hipGetLastError();
            return fail(ctx, BGS_EHIP, "capturing the frame into a hipGraph failed");
        }
        G.key = key;
        ctx->graph_captures += 1;
    }
    HIP_TRY(ctx, hipGraphLaunch(G.exec, L.stream));
    return BGS_OK;
}

// The frame on its lane's stream: as the captured graph of its kind (0 sorting, 1 kept order) and Control parity, or issued
// directly behind the memset of a scratch region that is not known to be clean; then what follows every frame.
template <class Front>
int submit_frame(bgs_ctx* ctx, Lane& L, const FramePlan& p, const FrameInputs& in, const FrameBindings& b, Front* front, bool need_memset,
                 const StageMarks& mark) {
    hipStream_t st = L.stream;
    int rc;
    if (p.graph_ok && !need_memset && mark.prof == 0 && front) {
        if ((rc = launch_graph(ctx, L, L.graph[p.kept ? 1 : 0][L.ctl_parity], graph_key(p, in, L, b, *front), *front, p, b, mark)) != BGS_OK) return rc;
    } else {
        if (need_memset) HIP_TRY(ctx, hipMemsetAsync(L.scratch.ptr, 0, L.layout.bytes, st));
        // no keygen (empty cloud): the kernels behind it still read the frame's parameters
        if (!front && !p.kept) HIP_TRY(ctx, hipMemcpyAsync(b.d_fp, &p.fp, sizeof p.fp, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, issue_frame(st, p, b, front, mark));
    }
    // the Control block travels back with the frame; it is looked at when the lane is completed.
    // A BINNING_SCAN frame's rasteriser has already written the counters to L.h_ctl and left the
    // scratch region zeroed for the next frame.
    L.scratch_clean = p.raster_cleans;
    if (p.raster_cleans) {
        L.ctl_parity ^= 1u;
    } else {
        if (p.places == 4 && p.n > 0) launch_splitters(st, b.draw_list, b.ctl, b.final_xor, p.split_sub_out);
        HIP_TRY(ctx, hipMemcpyAsync(L.h_ctl.ptr, b.ctl, sizeof(Control), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx, hipEventRecord(L.done, st));
    return BGS_OK;
}

// Step 6 of enqueue_frame: the lane keeps the frame's inputs and plan, and what was launched (g: with the front kernel's grid)
void keep_frame(bgs_ctx* ctx, Lane& L, const FramePlan& p, const FrameInputs& in, const FrameBindings& b, Lane::Grids g, bool replayed) {
    L.last_sorted = b.draw_list;
    L.last_sorted_n = p.n;
    L.last_ctl = p.render ? b.ctl : nullptr;
    L.last_replay = replayed;
    L.last_strips = b.raster_scan.strips();
    g.launched(g.DEPTH, b.depth);
    g.launched(g.PROJECT, b.project);
    g.launched(g.PROJECT, b.project_emit);
    g.launched(g.BIN, b.bin);
    if (b.project_emit.blocks) g.launched(g.TILE_SORT, b.tile_sort);   // (an empty frame's tile passes find nothing: not reported)
    L.grids = g;
    L.fb_valid = !(p.out_format & OUT_SKIP_F32) || (in.debug_flags & BGS_DEBUG_SEPARATE_ENCODE);
    L.fb8_is_f16 = (p.out_format & OUT_RGBA16F) != 0u;
    L.fb8_valid = p.want_srgb8;
    if (p.want_srgb8) L.fb8_out = in.srgb8_target ? in.srgb8_target : L.fb8.ptr;
    L.pending = true;
    L.pending_coarse_cap = b.raster_scan.coarse_cap;   // (of a BINNING_SCAN render)
    L.in = in;
    L.plan = p;
    L.seq = ++ctx->seq;
}

// Enqueue one frame on lane L: plan it, allocate, bind, commit its context changes, issue it, and keep its inputs and
// plan in the lane. Returns without waiting; the caller decides when to finish the lane.
int enqueue_frame(bgs_ctx* ctx, Lane& L, const FrameInputs& in) {
    const FramePlan p = plan_frame(*ctx, L, in);                                     // 1. the frame's choices
    uint32_t coarse_cap = 1;  // entries per supertile list
    int rc = ensure_frame_buffers(ctx, L, p, in, &coarse_cap);                       // 2. buffers
    if (rc != BGS_OK) return rc;
    const bool need_memset = !L.scratch_clean;  // else the previous frame's rasteriser left it zeroed
    if (need_memset) L.ctl_parity = 0;
    const FrameBindings b = bind_frame(L, p, in, coarse_cap, ctx->tile_trace);       // 3. bindings, and the front launch on them
    KeygenLaunch kg{};
    EntriesLaunch ek;   // (filled for a kept order only: a sorting frame's enqueue does not touch it)
    const bool have_keygen = !p.kept && prepare_keygen(*ctx, p, in, b, L.entries[0].ptr, L.culled.ptr, kg);
    const bool have_compact = p.kept && prepare_compact(p, in, b, L.culled.ptr, ek);
    const StageMarks mark = commit_frame(ctx, L, p);                                 // 4. the context's and the lane's state
    const uint64_t replays_before = ctx->graph_replays;
    rc = p.kept ? submit_frame(ctx, L, p, in, b, have_compact ? &ek : nullptr, need_memset, mark)   // 5. the launches
                : submit_frame(ctx, L, p, in, b, have_keygen ? &kg : nullptr, need_memset, mark);
    if (rc != BGS_OK) return rc;
    Lane::Grids g(++ctx->grid_stamps, p.n, in.grid_cap);                             // 6. what the lane keeps
    g.tail = p.culled_tail && (have_keygen || have_compact);
    if (have_keygen) g.launched(g.FRONT, kg);
    else if (have_compact) g.launched(g.FRONT, ek);
    g.front_chainless = have_keygen && p.bucket && !p.culled_tail;
    keep_frame(ctx, L, p, in, b, g, ctx->graph_replays != replays_before);
    return BGS_OK;
}

int run(bgs_ctx* ctx, const bgs_cloud* cloud, const bgs_view* view, const bgs_settings* s, bool render) {
    int rc = validate(ctx, cloud, view, s, render);
    if (rc != BGS_OK) return rc;
    if ((rc = enter(ctx)) != BGS_OK) return rc;
    const bool async = ctx->async_frames && render && ctx->binning == BINNING_SCAN;
    // a blocking call: complete whatever is queued first (surfaces its watchdog state), use lane 0;
    // an async frame: the next lane of the ring, completing its previous occupant first
    Lane& L = ctx->lanes[async ? ctx->next : 0];
    if (!async && (rc = finish_all(ctx)) != BGS_OK) return rc;
    if (async && L.pending && (rc = finish_lane(ctx, L)) != BGS_OK) return rc;
    // BGS_BOUNDS_CLOUD: the cloud's box, reduced now if no call has asked since the positions last changed (an empty
    // cloud has none: the caller's values stay, nothing is launched)
    const bool own_bounds = s->reserved[0] == BGS_BOUNDS_CLOUD && cloud->ptrs.n > 0u;
    if (own_bounds && (rc = cloud_bounds(ctx, cloud)) != BGS_OK) return rc;
    FrameInputs in{cloud, *view, *s, render, /*allow_graph=*/async, render ? ctx->next_srgb8_target : nullptr,
                         ctx->output_srgb8, ctx->output_rgba16f, ctx->packed_only, ctx->debug_flags,
                         render ? frame_kind(cloud->ptrs.n, cloud->ptrs.format, view, s) : 0ull, /*force_passes=*/false, ctx->grid_cap};
    if (own_bounds) {
        in.cloud_bounds = true;
        std::memcpy(in.pos_min, cloud->bounds_min, sizeof in.pos_min);
        std::memcpy(in.pos_max, cloud->bounds_max, sizeof in.pos_max);
    }
    if (!async) {
        ctx->recent = 0;
        ctx->regrow_count = 0;
        if (render) ctx->state.switch_kind(in.kind);
        if ((rc = enqueue_frame(ctx, L, in)) != BGS_OK) return rc;
        ctx->next_srgb8_target = nullptr;   // (one-shot: it belonged to this frame)
        return finish_lane(ctx, L);  // re-runs the frame itself if a capacity was too small
    }
    L.ready = false;
    const bool learn = !ctx->state.settled(in.kind);
    ctx->state.switch_kind(in.kind);
    if ((rc = enqueue_frame(ctx, L, in)) != BGS_OK) return rc;
    ctx->next_srgb8_target = nullptr;
    ctx->recent = ctx->next;
    ctx->next = (ctx->next + 1) % ctx->depth;
    if (learn) {
        // complete it now (re-running it if a first guess was too small): the frames behind it start from what it learnt.
        // It stays in the ring for bgs_pipeline_pop like any other frame.
        if ((rc = finish_lane(ctx, L)) != BGS_OK) return rc;
        L.ready = true;
        ctx->early_frames += 1;
        ctx->state.completed_early(in.kind);   // (bounded: LEARN_MAX of them settle the kind whatever they ran like)
    }
    return BGS_OK;
}

// One step of particle behaviours on a resident cloud (bgs_cloud_apply_particle_behaviors; the arguments are checked there).
// The step WRITES what every frame reads, so it is a pipeline barrier like bgs_cloud_free:
//   1. Frames in flight are completed first. They were enqueued against the old positions, and a frame that finish_lane
//      re-runs because a capacity was short must be re-run against those. Completed frames stay in the ring
//      (bgs_pipeline_pop still hands them out, oldest first): unlike finish_all this only waits.
//   2. The kernel goes on lane 0's stream, an event behind it, and every stream of the context waits for that event on
//      the device. The host does not wait: the next bgs_sort / bgs_render on any lane runs behind the step, the call
//      returns while the kernel may still be running.
// What the context has learnt about the cloud stays as it is. Every item is a hint that the frame's own kernels check:
//   - splitter tables (split_slots, keyed on the cloud): quantile keys of an earlier sorted list. Moved splats make the
//     buckets uneven; a bucket that outgrows its slots sets sort_overflow and the frame is re-run on the digit passes, the
//     table dropped (check_capacities) — the path a camera cut takes. A re-run sees the same, stepped, positions.
//   - draw-count hint, list capacity, supertile level: grid sizes and capacities; kernels loop over tickets and count
//     true totals, a short capacity re-runs the frame.
//   - heavy-tile lists, tile costs and the raster order: balance only, every tile is drawn exactly once whatever they hold.
//   - captured frame graphs: their nodes hold the ADDRESSES of the two position copies (GraphKey::cloud), which a step
//     does not change; the positions are read when the graph runs, behind the event above.
// So staleness is slow at worst, never wrong, and a small step (the usual case) keeps every hint useful.
int apply_particle_step(bgs_ctx* ctx, bgs_cloud* cloud, void* behaviors, uint32_t count, float dt) {
    if (int rc = enter(ctx); rc != BGS_OK) return rc;
    for (int i; (i = oldest_pending_lane(ctx)) >= 0;) {
        int rc = finish_lane(ctx, ctx->lanes[i]);
        if (rc != BGS_OK) return rc;
        ctx->lanes[i].ready = true;
    }
    if (!ctx->step_done) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->step_done, hipEventDisableTiming));
    hipStream_t st = ctx->lanes[0].stream;
    cloud->bounds_valid = false;   // (BGS_BOUNDS_CLOUD: the next frame or sort that asks reduces the stepped positions)
    launch_particle_step(st, behaviors, count, cloud->ptrs, dt);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->step_done, st));
    for (hipStream_t other : ctx->streams)
        if (other && other != st) HIP_TRY(ctx, hipStreamWaitEvent(other, ctx->step_done, 0));
    return BGS_OK;
}

// The box of a resident cloud for BGS_BOUNDS_CLOUD frames (bounds_math.h), lazily: uploads and particle steps leave it
// invalid, and the first bgs_sort / bgs_render that asks
//   1. completes the frames in flight, as a particle step does (they stay in the ring for bgs_pipeline_pop);
//   2. enqueues the two presets and the reduction on lane 0's stream: behind a particle step, which ran there, and behind
//      nothing else that writes positions (an upload has synchronised before it returned);
//   3. reads the six words back, 24 bytes, and WAITS for them: the one blocking read-back per change of the cloud;
//   4. decodes them, applies the -+0.1f and keeps the result in the cloud.
// Every frame, that one included, then carries the box in its FrameInputs.
int cloud_bounds(bgs_ctx* ctx, const bgs_cloud* cloud) {
    if (cloud->bounds_valid || cloud->ptrs.n == 0u) return BGS_OK;
    for (int i; (i = oldest_pending_lane(ctx)) >= 0;) {
        int rc = finish_lane(ctx, ctx->lanes[i]);
        if (rc != BGS_OK) return rc;
        ctx->lanes[i].ready = true;
    }
    if (!cloud->bounds_words.reserve(BOUNDS_WORDS)) return fail(ctx, BGS_ENOMEM, "hipMalloc(cloud bounds) failed");
    hipStream_t st = ctx->lanes[0].stream;
    uint32_t words[BOUNDS_WORDS];
    HIP_TRY(ctx, launch_cloud_bounds(st, cloud->ptrs.position_visibility, cloud->ptrs.n, cloud->bounds_words.ptr, (uint32_t)ctx->num_cus, ctx->grid_cap));
    HIP_TRY(ctx, hipMemcpyAsync(words, cloud->bounds_words.ptr, sizeof words, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    bounds_decode(words, cloud->bounds_min, cloud->bounds_max);
    cloud->bounds_valid = true;
    return BGS_OK;
}

}  // namespace bgs_host
