// bgs_context.h — what the translation units of libbgs' host side share: the context, its frame lanes and captured frame
// graphs (bgs_frame.hip owns their logic), and the functions the C ABI (bgs_api.hip), the diagnostics (bgs_diag.hip)
// and the frame gather (bgs_comm.hip) call. Internal: nothing here is part of the C ABI (include/bgs.h).
#pragma once
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/bgs.h"
#include "../../include/bgs_diag.h"
#include "bgs_device.h"
#include "adaptive_state.h"
#include "device_buffer.h"
#include "entries_math.h"
#include "frame_params.h"
#include "kernels.h"

using namespace bgs;

namespace bgs_host {

// The two memory policies of Buffer (device_buffer.h). A failed allocation leaves HIP's sticky error set, and the next
// hipGetLastError() — the one a frame's launches end in — would report it as that frame's: it is cleared here, always.
struct DeviceMem {
    static void* alloc(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) == hipSuccess) return p;
        (void)hipGetLastError();
        return nullptr;
    }
    static void free(void* p) { (void)hipFree(p); }
};
struct PinnedMem {
    static void* alloc(size_t bytes) {
        void* p = nullptr;
        if (hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess) return p;
        (void)hipGetLastError();
        return nullptr;
    }
    static void free(void* p) { (void)hipHostFree(p); }
};
template <class T> using DeviceBuffer = Buffer<T, DeviceMem>;
template <class T> using PinnedBuffer = Buffer<T, PinnedMem>;

}  // namespace bgs_host

struct bgs_cloud {
    CloudPtrs ptrs{};
    bgs_host::DeviceBuffer<uint8_t> positions, packed;   // what ptrs.position_visibility and ptrs.packed point at
    uint64_t bytes = 0;
    // The cloud's own box (BGS_BOUNDS_CLOUD, bounds_math.h): the six device words the reduction merges into, and what the
    // host read back and decoded from them. A cache of what the positions say, hence mutable: uploads leave it invalid and
    // the first frame or sort that asks fills it (cloud_bounds, bgs_frame.hip); a particle step invalidates it again.
    mutable bgs_host::DeviceBuffer<uint32_t> bounds_words;
    mutable float bounds_min[3] = {0.0f, 0.0f, 0.0f}, bounds_max[3] = {0.0f, 0.0f, 0.0f};
    mutable bool bounds_valid = false;
};

namespace bgs_host {

extern thread_local std::string g_error;   // (bgs_frame.hip) the message of the calling thread's last failure: bgs_last_error(NULL)

// (MIN_INSTANCE_CAPACITY / MAX_INSTANCE_CAPACITY: adaptive_state.h, with the growth rule)
constexpr uint32_t MAX_SPLATS = (1u << 30) - 1u;
// The stage events of a timed frame, each recorded behind the stage it is named for (issue_frame marks, collect_stats
// reads): a sort-only frame ends at MARK_SORT, a BINNING_SCAN render has no MARK_TILE_SORT / MARK_RANGES.
enum StageMark : int { MARK_BEGIN, MARK_FRONT, MARK_SORT, MARK_PROJECT, MARK_TILE_SORT, MARK_RANGES, MARK_RASTER, EV_COUNT };
static_assert(EV_COUNT == BGS_STAGE_COUNT + 1, "one event per stage boundary");
inline StageMark last_mark(bool render) { return render ? MARK_RASTER : MARK_SORT; }
constexpr int EV_RING = 64;   // per-stage timings are averaged over up to this many frames per lane
constexpr int MAX_LANES = 8;

// What the launches of a captured frame depend on besides what its first node carries (FrameParams; a kept-order
// frame's chunk address too: KeygenLaunch, EntriesLaunch): compared bytewise, any difference rebuilds the graph.
struct GraphKey {
    const void* cloud[6];
    const void* bufs[11];
    uint32_t n, places, sort_mode, srgb8, debug_flags;
    uint32_t project, raster;   // the launched instantiations of the vertex stage and the rasteriser: ProjectInst::key(), RasterInst::key()
    int32_t width, height;
    int32_t sort_blocks, bin_blocks, front_blocks;
    uint32_t sup_edge;
    // the offsets baked into the nodes depend on the scratch layout and the list capacity, not only on
    // the base pointers (a re-allocation may return the same address)
    ScratchLayout scratch;
    uint32_t coarse_cap, sort_path;
    // The front node (FrameGraph::front_node): keygen, or a kept-order frame's compaction (EntriesLaunch). keygen has
    // several instantiations per size (with / without chains, 256- or 1024-thread tiles: KeygenLaunch), the compaction
    // two (with / without the skipped tail): a captured node is only ever UPDATED to the kernel, grid (front_blocks) and
    // block size it was captured with
    const void* front_func;
    uint32_t front_threads;
    uint32_t wide_bin;         // bin_kernel<16> (1024 threads) or <4>: follows the pipeline depth, not the grid sizes
    uint32_t split_sub;        // FrameCleanup::split_sub, a rasteriser argument: how many quantile keys the captured clean-up leaves
};
struct FrameGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipGraphNode_t front_node = nullptr;   // the graph's root, the one node a replay updates: keygen, or the kept-order compaction
    GraphKey key{};
};

// What one frame depends on apart from the context's learnt state. run() fills it once; a frame whose data-dependent
// capacities turn out too small (coarse lists, bucket sort, tile instances) is re-run from its lane's copy, so that it
// produces the SAME outputs even if a setter (bgs_set_output_srgb8 / _rgba16f / _packed_only / _debug_flags /
// _srgb8_target) was called while it was in flight.
struct FrameInputs {
    const bgs_cloud* cloud = nullptr;   // (cleared by bgs_cloud_free)
    bgs_view view{};
    bgs_settings settings{};
    bool render = false, allow_graph = false;
    uint32_t* srgb8_target = nullptr;   // bgs_set_srgb8_target: the frame's own packed-image destination (renders only)
    bool output_srgb8 = false, output_rgba16f = false, packed_only = false;
    uint32_t debug_flags = 0;
    uint64_t kind = 0;                  // frame_kind() (0: a bgs_sort)
    bool force_passes = false;          // the digit passes, not the bucket sort: a re-run of a frame whose bucket sort gave up
    uint32_t grid_cap = 0;              // bgs_set_grid_cap as it was when the frame was enqueued (0: off): a re-run keeps its grids
    // BGS_BOUNDS_CLOUD (bgs_settings.reserved[0]) on a cloud that has splats: the cloud's own box as it was when the frame
    // was enqueued, which plan_frame puts in the place of settings.position_min / _max (a re-run draws the same frame)
    bool cloud_bounds = false;
    float pos_min[3] = {0.0f, 0.0f, 0.0f}, pos_max[3] = {0.0f, 0.0f, 0.0f};
};

// Every choice of one frame (plan_frame, bgs_frame.hip): enqueue_frame allocates, binds (FrameBindings) and issues it,
// finish_lane reads it back when the frame is complete.
struct FramePlan {
    FrameParams fp{};               // what keygen hands the frame's kernels (debug flags, sRGB8 target, sort path included)
    bool render = false, scan = false, surfel = false, culled_tail = true;   // (culled_tail: keygen writes the culled tail)
    uint32_t n = 0, places = 0, rec_bytes = 0, cloud_format = 0;
    // depth sort: bucket or digit passes; 256 * bucket_sub buckets (the sub of the splitter slot's table); the quantile
    // table the frame LEAVES has 256 * split_sub_out - 1 keys; the slot (-1: none, or a guessed table) and its epoch
    // kept: no keys and no depth sort at all — the frame draws the caller's entries (bgs_view.entries_device_ptr) through
    // the compaction of entries_kernels.hip (places = 0, never bucket)
    bool bucket = false, wide = false, kept = false;
    uint32_t bucket_sub = 1, split_sub_out = 1;
    int split_slot = -1;
    uint64_t split_epoch = 0;
    uint32_t edges[4] = {6, 8, 16, 32}, level = 1, sup_edge = 8, num_st = 0;   // supertiles
    bool large = false, wide_bin = false, want_srgb8 = false;
    int sort_blocks = 0, bin_blocks = 0, binning_blocks = 0;
    // the grids plan_frame does not size by the draw hint: keygen's (ordered instantiations) and the compaction's, BINNING_SORT's
    // project_emit and its two tile-id passes. All six are what bgs_set_grid_cap caps (FrameInputs::grid_cap)
    int front_blocks = 0, emit_blocks = 0, tile_sort_blocks = 0;
    uint32_t out_format = 0, ntiles = 0;
    bool raster_cleans = false;     // the rasteriser zeroes the scratch region and reports the Control block (FrameCleanup)
    RasterInst raster{};            // the instantiation launch_raster_scan launches (launch_raster: its variant, samples, depth, overlay)
    ProjectInst project{};          // the instantiation of the vertex stage (ProjectLaunch / ProjectEmitLaunch)
    // heavy-tile strips; leaves tile costs / draws in cost order / makes that order anew; the kind of the cost plane
    // behind its order, whose saturation counts the frame reports (0: none); may replay a captured graph
    bool heavy = false, cost = false, ordered = false, refresh = false, graph_ok = false;
    uint64_t sat_kind = 0;
    // what the frame is to the stage timings (Lane::ev_kind, result_kind): 1 sort-only frame, 2 render/scan, 3 render/sort-binning,
    // 4 / 5: 2 / 3 drawn in a kept order (0: an unused ring slot)
    uint8_t ev_kind() const { return (uint8_t)(!render ? 1 : (scan ? 2 : 3) + (kept ? 2 : 0)); }
    struct EvKind { bool render, scan, kept; };
    static EvKind decode_ev_kind(uint8_t kind) { return {kind != 1, kind == 2 || kind == 4, kind >= 4}; }
};

// A frame's device memory: which pointer of the lane (and of its scratch region, ScratchLayout) each kernel argument is,
// and the frame's stage launches filled from them and prepared. bind_frame (bgs_frame.hip) makes it from the lane, the
// plan and the inputs, without a HIP call or a change of state; issue_frame launches from it, graph_key and the lane's
// bookkeeping read it. Of the stage launches only those of the frame's path are filled (the others launch nothing).
struct FrameBindings {
    Control* ctl = nullptr;          // this frame's Control block, by the lane's parity (the other one: raster_scan.cleanup)
    uint32_t* part_status = nullptr;   // the front kernel's chain
    uint32_t* depth_status = nullptr;  // the depth passes' look-back words
    uint2* ranges = nullptr;         // BINNING_SORT: [start, end) per tile
    uint2* draw_list = nullptr;      // the sorted draw list: entries[places & 1], the passes ping-pong from entries[0]
    uint32_t final_xor = 0;          // SortMode::Rayon / Std sort ascending on the inverted key; the last step of either path un-inverts it
    // the tile feedback (TileFeedback): the cost plane the frame makes its order of (only a frame that makes it anew) and the
    // order; what the rasteriser reads and leaves is in raster_scan (heavy_in: only a completed buffer of the same grid
    // that is not the one being written)
    const uint16_t* cost_in = nullptr;
    uint16_t* tile_order = nullptr;
    // the lane's buffers that the short launchers and the front launch take
    uint2* bucket_slots = nullptr;
    uint32_t* split_keys = nullptr;          // a long splitter table as keygen reads it, and the pinned staging it is copied from
    uint32_t* split_keys_staging = nullptr;
    FrameParams* d_fp = nullptr;
    float4* fb = nullptr;
    uint32_t* fb8 = nullptr;
    OnesweepLaunch depth, tile_sort;     // the digit passes of the depth keys; BINNING_SORT: of the tile ids
    ProjectLaunch project;               // BINNING_SCAN
    BinLaunch bin;
    RasterScanLaunch raster_scan;        // (its cleanup: the frame's FrameCleanup)
    ProjectEmitLaunch project_emit;      // BINNING_SORT
    RasterLaunch raster;
};

// The tile feedback a lane's BINNING_SCAN frames leave for its next ones: balance only, every tile is drawn exactly once
// whatever the buffers hold.
struct TileFeedback {
    // heavy-tile feedback of the rasteriser (kernels.h HeavyFeedback): two buffers per lane, written alternately, so that
    // frames of other lanes can still be reading the one this lane's previous frame completed
    DeviceBuffer<uint8_t> heavy[2];
    uint32_t heavy_parity = 0;  // heavy[heavy_parity] is what the lane's NEXT frame writes; flipped when a frame COMPLETES
    // The feedback the lane's next dense frame consumes: the buffer its most recently COMPLETED dense frame wrote (any
    // view: a stale list costs balance, never pixels — every tile is drawn exactly once, by its regular wave or by a
    // strip workgroup, whichever the list it reads says). Per LANE: a lane's frames run one after the other, so the
    // buffer a frame reads (heavy[parity ^ 1], complete) is never the one it — or a re-run of it — writes
    // (heavy[parity]), and no frame of another lane ever reads either.
    const uint8_t* heavy_done = nullptr;
    uint32_t heavy_done_grid = 0;   // tile_grid_word of that frame
    // per-tile cost feedback (kernels.h TileCost), the same life cycle as the heavy-tile lists: cost[cost_parity] is what
    // the lane's next frame writes, cost_done what its most recently completed frame wrote; `order` is made of
    // cost_done at the start of a frame and read by that frame's rasteriser only
    DeviceBuffer<uint16_t> cost[2], order;   // (cost planes: tile_cost_bytes / 2 elements)
    uint32_t cost_parity = 0;
    const uint16_t* cost_done = nullptr;
    uint32_t cost_done_grid = 0;
    uint64_t cost_done_kind = 0;    // kind of the frame that left cost_done
    uint32_t order_grid = 0xFFFFFFFFu, order_age = 0;   // the grid `order` is a permutation for; frames drawn with it since it was made
    uint64_t order_kind = 0;        // kind of the frame whose cost plane the lane's order (and its saturation counts) was made of

    // nothing a completed frame left is used again (the buffers stay)
    void forget_heavy() { heavy_done = nullptr; }
    void forget_cost() { cost_done = nullptr; order_grid = 0xFFFFFFFFu; }
    void forget() { forget_heavy(); forget_cost(); }
    // A frame is ENQUEUED: one that makes the order anew makes it of cost_done, for its grid
    void enqueued(const FramePlan& p) {
        if (p.refresh) { order_kind = cost_done_kind; order_grid = tile_grid_word(p.fp); order_age = 0; }
        else if (p.ordered) order_age += 1u;
    }
    // The frame is COMPLETE: what it wrote is what the lane's next dense frames read (null after a frame that left none).
    // Only now does the lane's next frame write the OTHER buffer: a re-run wrote the one its failed attempt wrote, never
    // the completed frame's list it was reading
    void completed(const FramePlan& p, uint64_t kind) {
        heavy_done = p.heavy ? heavy[heavy_parity].ptr : nullptr;
        heavy_done_grid = cost_done_grid = tile_grid_word(p.fp);
        if (p.heavy) heavy_parity ^= 1u;
        cost_done = p.cost ? cost[cost_parity].ptr : nullptr;
        cost_done_kind = kind;
        if (p.cost) cost_parity ^= 1u;
    }
};

// Everything one in-flight frame owns. The buffers free themselves (lane_destroy: L = Lane()); a buffer's capacity is in
// elements of its type.
struct Lane {
    hipStream_t stream = nullptr;  // owned by the context; lanes may share one (bgs_set_pipeline_streams)
    hipEvent_t done = nullptr;     // recorded behind the lane's frame: what completing the lane waits for
    DeviceBuffer<FrameParams> d_fp;  // the frame's FrameParams as the kernels behind keygen read them
    // the captured BINNING_SCAN frames, one per kind (0 sorting, 1 kept order) and Control parity: a lane that alternates
    // between the kinds replays both
    FrameGraph graph[2][2];

    // zeroed-every-frame scratch and where its parts lie (scratch_layout, frame_params.h; grown monotonically in the
    // splat and the instance capacity it is laid out for)
    DeviceBuffer<uint8_t> scratch;
    ScratchLayout layout;
    uint32_t ctl_parity = 0;  // which of the lane's two Control blocks the next frame uses
    // true while the scratch region is known to be all zero without a memset: the rasteriser of a
    // BINNING_SCAN frame zeroes what the frame used (FrameCleanup, kernels.h)
    bool scratch_clean = false;

    // the sort's ping-pong lists and the entries with the culled sentinel key (index order): one group, all of one
    // capacity or all empty (ensure_entries)
    DeviceBuffer<uint2> entries[2], culled;
    DeviceBuffer<uint8_t> records;
    DeviceBuffer<uint32_t> rects;   // BINNING_SCAN: packed tile rectangle per rank (project_kernel -> bin_kernel), as many words as entries; released with them
    DeviceBuffer<uint2> inst[2];    // BINNING_SORT only (one group)
    DeviceBuffer<uint32_t> coarse;  // BINNING_SCAN: [num_supertiles][coarse_cap] ordered (rank, tile rect) lists: two words per entry
    // bucket sort: BUCKET_COUNT * BUCKET_CAP pairs (8 MB) per narrow sub, four times that per wide one; allocated on first
    // use, grown with sub
    DeviceBuffer<uint2> bucket_slots;
    // a long splitter table (sub > BUCKET_SUB_KERNARG) as keygen reads it, BUCKET_MAX words, and the pinned staging it is
    // copied from, ahead of keygen, on the frame's stream (one group)
    DeviceBuffer<uint32_t> d_split_keys;
    PinnedBuffer<uint32_t> h_split_keys;
    TileFeedback feedback;
    bool ready = false;   // the lane's frame is complete but nobody has taken it yet (bgs_pipeline_pop): a frame finished early, see AdaptiveState::kinds
    DeviceBuffer<float4> fb;
    DeviceBuffer<uint32_t> fb8;  // the packed image (optional): two words per pixel, room for either format (4 or 8 bytes)
    uint32_t* fb8_out = nullptr; // where the last frame's packed image went (fb8 or a caller's target)
    uint32_t fb_w = 0, fb_h = 0;
    bool fb8_valid = false, fb8_is_f16 = false;
    bool fb_valid = true;  // false after a packed-only frame (the f32 target was not written)

    PinnedBuffer<Control> h_ctl;  // filled by a copy enqueued with the frame, or by the rasteriser
    Control* h_ctl_dev = nullptr;  // the same memory as the device sees it
    hipEvent_t ev_ring[EV_RING][EV_COUNT] = {};
    uint8_t ev_kind[EV_RING] = {};  // FramePlan::ev_kind() of the frame timed in the slot, 0 unused
    uint32_t ev_head = 0;
    uint32_t frames_timed = 0;  // timed frames since the last stats read-back

    bool pending = false;  // a frame is enqueued whose Control block has not been checked yet
    FrameInputs in;        // what the lane's frame was enqueued with (a re-run enqueues it again)
    FramePlan plan;        // ... and the choices it was enqueued with
    uint32_t pending_coarse_cap = 0;   // entries per supertile list the pending frame was given
    uint64_t seq = 0;  // enqueue sequence number (to find the oldest pending lane)

    const uint2* last_sorted = nullptr;
    uint32_t last_sorted_n = 0;
    // The Control block (in `scratch`) the lane's last ENQUEUED render used — a re-run's is the re-run's —, for
    // bgs_debug_frame_records: a frame's own block keeps what its project kernel left (visible_count, color_max_bits)
    // until the lane's next frame. Null after a bgs_sort and after anything else that rewrites the scratch region.
    const Control* last_ctl = nullptr;
    // ... and, for bgs_debug_frame_leftovers, whether that frame was a graph replay and whether its rasteriser's grid had
    // the strip workgroups behind it
    bool last_replay = false, last_strips = false;
    // What the lane's last enqueued frame — or a diag hook that launches persistent kernels of its own, on lane 0 —
    // launched, for bgs_debug_frame_grids: per persistent kernel the workgroups, the items of one tile (0: not launched) and
    // which count its tiles are made of when the report is read. The report is the lane's with the newest stamp.
    struct Grids {
        enum Kernel { FRONT, DEPTH, PROJECT, BIN, TILE_SORT, KERNELS };
        enum Count : uint8_t { HOST_N, DRAW_COUNT, INSTANCE_COUNT };   // n below, or the completed frame's Control copy
        uint32_t blocks[KERNELS] = {}, per_tile[KERNELS] = {};
        Count count[KERNELS] = {HOST_N, DRAW_COUNT, DRAW_COUNT, DRAW_COUNT, INSTANCE_COUNT};
        uint32_t n = 0;           // the items the host knows: the cloud's splats, a hook's pairs
        uint32_t cap = 0;         // the grid cap the kernels were launched under
        bool front_chainless = false;
        bool tail = false;        // the front kernel wrote the culled / skipped entries to the lane's `culled`, n - draw_count of them
        uint64_t stamp = 0;       // bgs_ctx::grid_stamps when it was written (0: never)
        Grids() = default;
        Grids(uint64_t stamp_, uint32_t n_, uint32_t cap_) : n(n_), cap(cap_), stamp(stamp_) {}   // a report of its own stamp: ++ctx->grid_stamps
        // what a prepared launch struct (kernels.h) launches, or would: a captured frame's replay runs what was prepared
        template <class Launch> void launched(Kernel k, const Launch& l) { if (l.blocks) { per_tile[k] = l.per_tile; blocks[k] = l.blocks; } }
    } grids;

    bgs_stats result{};      // counters of the last completed frame of this lane (no timings)
    bool has_result = false;
    uint8_t result_kind = 0; // ev_kind of that frame
};

}  // namespace bgs_host
using namespace bgs_host;

struct bgs_ctx {
    int device = 0;
    int num_cus = 256;
    std::string error;

    Lane lanes[MAX_LANES];
    hipStream_t streams[MAX_LANES] = {};
    int num_streams = 4;  // streams the lanes are multiplexed onto, 0 = one per lane (one per hardware queue: include/bgs.h)
    int depth = 1;    // lanes in use
    int next = 0;     // lane the next frame goes to
    int recent = 0;   // lane of the most recently enqueued frame
    uint64_t seq = 0;
    // recorded behind the last particle step (apply_particle_step): every stream of the context waits for it, one created
    // later included (assign_streams)
    hipEvent_t step_done = nullptr;

    uint32_t binning = BINNING_SCAN;
    uint32_t debug_flags = 0;
    uint32_t grid_cap = 0;          // bgs_set_grid_cap: 0 off, else the most workgroups of any persistent launch
    uint64_t grid_stamps = 0;       // Lane::Grids written so far
    int profiling = 2;              // 0 = no events, 1 = frame start/end only, 2 = every stage
    uint32_t profiling_stride = 1;  // record events only on every Nth frame
    uint32_t frame_counter = 0;
    bool async_frames = false;
    bool output_srgb8 = false;
    bool output_rgba16f = false;   // the packed image is Rgba16Float (8 B per pixel) instead of Rgba8UnormSrgb
    bool packed_only = false;      // frames with a packed image do not write the f32 target
    uint32_t* next_srgb8_target = nullptr;  // bgs_set_srgb8_target: one-shot destination of the next frame

    AdaptiveState state;   // everything completed frames leave for the next ones, and the rules that write it
    uint64_t bucket_frames = 0, onesweep_frames = 0;  // frames enqueued on either sort path (incl. re-runs)
    uint64_t reruns_sort = 0, reruns_lists = 0, reruns_instances = 0, level_changes = 0;
    uint64_t early_frames = 0;      // async frames completed inside their bgs_render call (bgs_learning_counters)
    uint4* tile_trace = nullptr;  // bgs_set_tile_trace: caller-owned device buffer the rasteriser's TRACE instantiation fills
    bool use_graphs = false;  // async BINNING_SCAN frames replay a captured hipGraph (bgs_set_graphs)
    uint64_t graph_captures = 0, graph_replays = 0;
    uint64_t cost_frames = 0, ordered_frames = 0, order_refreshes = 0;   // frames that left tile costs / drew their raster workgroups in cost order / made the order anew

    bool have_stats = false;
    bgs_stats stats{};
    uint32_t regrow_count = 0;
};

namespace bgs_host {
// (bgs_frame.hip)
int fail(bgs_ctx* ctx, int status, const std::string& msg);   // records the message, returns the status
int enter(bgs_ctx* ctx);                                       // what an entry point that talks to the device begins with: hipSetDevice
int enter_drained(bgs_ctx* ctx);                               // ... and finish_all: no frame is in flight behind it
int assign_streams(bgs_ctx* ctx);
int lane_create(bgs_ctx* ctx, Lane& L);
void lane_destroy(Lane& L);
int finish_lane(bgs_ctx* ctx, Lane& L);                        // completes the lane's frame in flight (re-runs it if a capacity was short)
int finish_all(bgs_ctx* ctx);                                  // ... every lane's
int collect_stats(bgs_ctx* ctx);
int ensure_scratch(bgs_ctx* ctx, Lane& L, uint32_t n, uint64_t inst_cap);
int enqueue_frame(bgs_ctx* ctx, Lane& L, const FrameInputs& in);
int ensure_entries(bgs_ctx* ctx, Lane& L, uint32_t n);
int run(bgs_ctx* ctx, const bgs_cloud* cloud, const bgs_view* view, const bgs_settings* s, bool render);   // bgs_sort / bgs_render
int apply_particle_step(bgs_ctx* ctx, bgs_cloud* cloud, void* behaviors, uint32_t count, float dt);        // bgs_cloud_apply_particle_behaviors
int cloud_bounds(bgs_ctx* ctx, const bgs_cloud* cloud);        // BGS_BOUNDS_CLOUD: the cloud's box is valid behind it (reduced on the device if it was not)
extern int g_queue_holders_mode;           // bgs_set_queue_holders
extern std::mutex g_queue_holders_mutex;
}  // namespace bgs_host

#define HIP_TRY(ctx, expr)                                                                  \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(ctx, BGS_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));  \
    } while (0)
