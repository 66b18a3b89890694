// device_math_shim.cpp — TEST-ONLY host build of the product's device math header.
//
// Compiles bevy_gaussian_splatting_amd/csrc/splat_math.h with g++ (BGS_HD expands to nothing)
// so tests/test_device_math_host.py can check the per-splat arithmetic the HIP kernels run
// against the oracle WITHOUT a GPU. This is a pre-flight check, not a product path: libbgs
// never runs these functions on the host and has no CPU fallback.
#include <stdlib.h>

#include "../../bevy_gaussian_splatting_amd/csrc/adaptive_state.h"
#include "../../bevy_gaussian_splatting_amd/csrc/device_buffer.h"
#include "../../bevy_gaussian_splatting_amd/csrc/frame_params.h"
#include "../../bevy_gaussian_splatting_amd/csrc/splat_math.h"

using namespace bgs;

struct ShimOut {
    int32_t visible, draw;
    float color[4];
    float cx, cy;
    float p[5];
    float radius;
    int32_t tx0, ty0, tx1, ty1;
    float mean[2];
    float T[9];
    float quad_m[4];
    float bounds[4];  // minx maxx miny maxy
    float ndc_z;      // the quad's depth (position.z / position.w)
};

struct ShFloat {
    const float* base;
    void load_all(float* c) const { memcpy(c, base, 48 * sizeof(float)); }
};

extern "C" {

void shim_fill_params(uint32_t n, const bgs_view* view, const bgs_settings* s, FrameParams* fp) {
    fill_frame_params(n, view, s, *fp);
}

// csrc/exact_log.h: the correctly rounded ln of the adaptive cutoff, host build (the device runs the same operations)
// the rasteriser's work order with S runs per XCD, for every workgroup of a grid of n
void shim_xcd_runs_items(uint32_t n, uint32_t S, uint32_t* out) {
    for (uint32_t b = 0; b < n; ++b) out[b] = xcd_runs_item(b, n, S);
}

void shim_ln_f32(const float* x, uint32_t n, float* out) {
    for (uint32_t i = 0; i < n; ++i) out[i] = ln_f32_cr(x[i]);
}

uint64_t shim_ln_f32_checksum(uint32_t first_bits, uint32_t count) {
    uint64_t sum = 0;
#pragma omp parallel for schedule(static) reduction(+ : sum)
    for (int64_t i = 0; i < (int64_t)count; ++i) {
        const uint32_t in_bits = first_bits + (uint32_t)i;
        float x; memcpy(&x, &in_bits, 4);
        sum += ln_selftest_mix(in_bits, f2u(ln_f32_cr(x)));
    }
    return sum;
}

uint32_t shim_frame_params_size(void) { return (uint32_t)sizeof(FrameParams); }

// supertile index of a tile for a supertile edge (bgs_device.h: reciprocal multiply)
uint32_t shim_supertile_div(uint32_t tile, uint32_t edge) { return supertile_div(tile, supertile_mul(edge)); }

// host-side adaptive policies (frame_params.h)
uint32_t shim_next_supertile_level(double ratio, uint32_t lv, const uint32_t* edges, double* longer_out) {
    return next_supertile_level(ratio, lv, edges, longer_out);
}
uint32_t shim_pow2_ceil(uint64_t v) { return pow2_ceil_u32(v); }
int shim_splitters_ascending(const uint32_t* key, uint32_t count) { return splitters_ascending(key, count) ? 1 : 0; }
void shim_supertile_edges(uint32_t tiles_x, uint32_t tiles_y, uint32_t* edges) { supertile_edges(tiles_x, tiles_y, edges); }
uint32_t shim_canonical_supertile_level(uint32_t level, const uint32_t* edges) { return canonical_supertile_level(level, edges); }
int shim_raster_scan_mode(int variant, uint32_t samples, int overlay, uint32_t level, int kind_midround, int pipeline_depth,
                          uint32_t debug_flags) {
    return raster_scan_mode(variant, samples, overlay != 0, level, kind_midround != 0, pipeline_depth, debug_flags);
}
// RasterInst / ProjectInst (frame_params.h): the instantiations that are compiled, and what the kernel takes from one
static RasterInst raster_inst(int variant, uint32_t samples, int depth, int overlay, int mode, int trace) {
    return RasterInst{variant, samples, depth != 0, overlay != 0, mode, trace != 0};
}
int shim_raster_inst_exists(int variant, uint32_t samples, int depth, int overlay, int mode, int trace) {
    return raster_inst(variant, samples, depth, overlay, mode, trace).exists() ? 1 : 0;
}
uint32_t shim_raster_inst_runs(int variant, uint32_t samples, int depth, int overlay, int mode, int trace) {
    return raster_inst(variant, samples, depth, overlay, mode, trace).runs();
}
int shim_raster_inst_waves(int variant, uint32_t samples, int depth, int overlay, int mode, int trace) {
    return raster_inst(variant, samples, depth, overlay, mode, trace).waves_per_simd();
}
uint32_t shim_raster_inst_key(int variant, uint32_t samples, int depth, int overlay, int mode, int trace) {
    return raster_inst(variant, samples, depth, overlay, mode, trace).key();
}
int shim_project_inst_exists(uint32_t format, int surfel, int any_mode) { return ProjectInst{format, surfel != 0, any_mode != 0}.exists() ? 1 : 0; }
// raster_instantiation for a frame of these settings: out = variant, samples, depth, overlay, mode, trace
void shim_raster_instantiation(uint32_t aabb, uint32_t gaussian_mode, uint32_t samples, int depth, int overlay, uint32_t level, int kind_midround,
                               int pipeline_depth, uint32_t debug_flags, int trace, int32_t out[6]) {
    FrameParams fp{};
    fp.aabb = aabb;
    fp.gaussian_mode = gaussian_mode;
    fp.sample_count = samples;
    fp.depth_ptr = depth ? 16ull : 0ull;
    fp.visualize_bbox = overlay ? 1u : 0u;
    const RasterInst r = raster_instantiation(fp, level, kind_midround != 0, pipeline_depth, debug_flags, trace != 0);
    const int32_t v[6] = {r.variant, (int32_t)r.samples, r.depth ? 1 : 0, r.overlay ? 1 : 0, r.mode, r.trace ? 1 : 0};
    memcpy(out, v, sizeof v);
}

// the scratch layout of a lane (frame_params.h), as 11 x u64 + 2 x u32
void shim_scratch_layout(uint32_t n, uint64_t inst_cap, ScratchLayout* out) { *out = scratch_layout(n, inst_cap); }
uint32_t shim_scratch_layout_size(void) { return (uint32_t)sizeof(ScratchLayout); }

// where the words of a Control block lie (bgs_device.h), in 32-bit words: sizeof(Control), CONTROL_HEADER_WORDS, then the
// offsets named in tests/helpers.py CONTROL_FIELDS, in that order; returns how many words `out` was given
uint32_t shim_control_offsets(uint32_t* out) {
    const uint32_t v[] = {(uint32_t)(sizeof(Control) / 4u), CONTROL_HEADER_WORDS,
                          (uint32_t)(offsetof(Control, draw_count) / 4u), (uint32_t)(offsetof(Control, instance_count) / 4u),
                          (uint32_t)(offsetof(Control, error) / 4u), (uint32_t)(offsetof(Control, visible_count) / 4u),
                          (uint32_t)(offsetof(Control, splat_count) / 4u), (uint32_t)(offsetof(Control, sort_overflow) / 4u),
                          (uint32_t)(offsetof(Control, bucket_max) / 4u), (uint32_t)(offsetof(Control, strip_tiles) / 4u),
                          (uint32_t)(offsetof(Control, saturated_tiles_prev) / 4u), (uint32_t)(offsetof(Control, ticket) / 4u),
                          (uint32_t)(offsetof(Control, color_max_bits) / 4u), (uint32_t)(offsetof(Control, hist_depth) / 4u),
                          (uint32_t)(offsetof(Control, coarse_total) / 4u), (uint32_t)(offsetof(Control, splitters) / 4u),
                          (uint32_t)(offsetof(Control, bucket_count) / 4u), BUCKET_MAX};
    for (uint32_t i = 0; i < sizeof v / sizeof v[0]; ++i) out[i] = v[i];
    return (uint32_t)(sizeof v / sizeof v[0]);
}

// ---- Buffer (device_buffer.h) over a memory policy that counts: live allocations and their peak, calls, the bytes of the
// last request; fail_at = k makes the k-th alloc() from now fail
struct CountingMem {
    static inline int64_t live = 0, peak = 0, allocs = 0, frees = 0, last_bytes = 0, fail_at = 0;
    static void* alloc(size_t bytes) {
        ++allocs;
        last_bytes = (int64_t)bytes;
        if (fail_at > 0 && --fail_at == 0) return nullptr;
        if (++live > peak) peak = live;
        return malloc(bytes ? bytes : 1);
    }
    static void free(void* p) { ++frees; --live; ::free(p); }
};
using TestBuffer = Buffer<uint64_t, CountingMem>;

void shim_mem_reset(int64_t fail_at) {
    CountingMem::peak = CountingMem::live;
    CountingMem::allocs = CountingMem::frees = CountingMem::last_bytes = 0;
    CountingMem::fail_at = fail_at;
}
void shim_mem_counters(int64_t out[5]) {
    out[0] = CountingMem::live; out[1] = CountingMem::peak; out[2] = CountingMem::allocs; out[3] = CountingMem::frees;
    out[4] = CountingMem::last_bytes;
}
void* shim_buf_new(void) { return new TestBuffer(); }
void shim_buf_delete(void* b) { delete (TestBuffer*)b; }
int shim_buf_reserve(void* b, uint64_t count, int64_t min_bytes) {
    TestBuffer& t = *(TestBuffer*)b;
    return (min_bytes < 0 ? t.reserve(count) : t.reserve(count, (size_t)min_bytes)) ? 1 : 0;
}
void shim_buf_reset(void* b) { ((TestBuffer*)b)->reset(); }
void shim_buf_state(const void* b, uint64_t out[2]) {
    out[0] = (uint64_t)(uintptr_t)((const TestBuffer*)b)->ptr;
    out[1] = ((const TestBuffer*)b)->capacity;
}
void shim_buf_move_assign(void* dst, void* src) { *(TestBuffer*)dst = static_cast<TestBuffer&&>(*(TestBuffer*)src); }
void* shim_buf_move_new(void* src) { return new TestBuffer(static_cast<TestBuffer&&>(*(TestBuffer*)src)); }
void shim_buf_release_and_free(void* b) { CountingMem::free(((TestBuffer*)b)->release()); }
int shim_buf_reserve_group(void* b0, void* b1, void* b2, uint64_t count) {
    return reserve_group(count, *(TestBuffer*)b0, *(TestBuffer*)b1, *(TestBuffer*)b2);
}

// ---- the context's learnt state and its rules (adaptive_state.h): an opaque handle, one export per rule, getters for what
// a rule leaves. A cloud is its identity (any pointer value) and its n.
void* shim_state_new(void) { return new AdaptiveState(); }
void shim_state_delete(void* st) { delete (AdaptiveState*)st; }
uint64_t shim_frame_kind(uint32_t n, uint32_t format, const bgs_view* view, const bgs_settings* s) { return frame_kind(n, format, view, s); }
void shim_state_switch_kind(void* st, uint64_t kind) { ((AdaptiveState*)st)->switch_kind(kind); }
void shim_state_settle(void* st, uint64_t kind, uint32_t level) { ((AdaptiveState*)st)->settle(kind, level); }
void shim_state_completed_early(void* st, uint64_t kind) { ((AdaptiveState*)st)->completed_early(kind); }
void shim_state_learn_saturation(void* st, uint64_t kind, uint32_t saturated) { ((AdaptiveState*)st)->learn_saturation(kind, saturated); }
void shim_state_learn_draw_count(void* st, uint32_t draw_count) { ((AdaptiveState*)st)->learn_draw_count(draw_count); }
int shim_state_find_splitter_slot(const void* st, const void* cloud, uint32_t n, const bgs_view* view, const bgs_settings* s) {
    return ((const AdaptiveState*)st)->find_splitter_slot({cloud, n, view, s});
}
void shim_state_store_splitters(void* st, const uint32_t* keys, uint32_t sub, uint32_t places, uint32_t draw_count, const void* cloud,
                                uint32_t n, const bgs_view* view, const bgs_settings* s, uint64_t seq) {
    ((AdaptiveState*)st)->store_splitters(keys, sub, places, draw_count, {cloud, n, view, s}, seq);
}
void shim_state_frame_enqueued(void* st, uint32_t places, int slot, uint64_t seq) { ((AdaptiveState*)st)->frame_enqueued(places, slot, seq); }
int shim_state_learn_bucket_sort(void* st, uint32_t sort_overflow, int slot, uint64_t epoch) {
    return ((AdaptiveState*)st)->learn_bucket_sort(sort_overflow, slot, epoch) ? 1 : 0;
}
uint32_t shim_state_list_capacity(void* st, uint32_t n, int small_lists) { return ((AdaptiveState*)st)->list_capacity(n, small_lists != 0); }
int shim_state_learn_list_capacity(void* st, uint32_t longest, uint32_t level, uint32_t capacity) {
    return ((AdaptiveState*)st)->learn_list_capacity(longest, level, capacity) ? 1 : 0;
}
// BINNING_SORT's growth rule: the capacity a frame that needs `need` tile instances is re-run with, 0: refused; limits[0..1]:
// MIN_INSTANCE_CAPACITY, MAX_INSTANCE_CAPACITY
uint64_t shim_instance_capacity_for(uint64_t need, uint64_t* limits) {
    if (limits) { limits[0] = MIN_INSTANCE_CAPACITY; limits[1] = MAX_INSTANCE_CAPACITY; }
    const InstanceVerdict v = instance_capacity_for(need);
    return v.refuse ? 0ull : v.capacity;
}
// returns moved | changed << 1
int shim_state_learn_level(void* st, uint64_t kind, uint32_t lv, const uint32_t* edges, uint64_t instances, uint32_t visible, uint32_t longest) {
    const AdaptiveState::LevelVerdict v = ((AdaptiveState*)st)->learn_level(kind, lv, edges, instances, visible, longest);
    return (v.moved ? 1 : 0) | (v.changed ? 2 : 0);
}
void shim_state_distrust(void* st) { ((AdaptiveState*)st)->distrust(); }
void shim_state_forget_cloud(void* st, const void* cloud) { ((AdaptiveState*)st)->forget_cloud(cloud); }
void shim_state_reset(void* st) { ((AdaptiveState*)st)->reset(); }
// the scalar members, in the order of tests/helpers.py STATE_FIELDS
void shim_state_get(const void* st, uint64_t out[13]) {
    const AdaptiveState& a = *(const AdaptiveState*)st;
    const uint64_t v[13] = {a.draw_hint, a.draw_hint_valid ? 1u : 0u, a.draw_shrink_votes, a.sup_level, a.coarse_cap_hint, a.list_shrink_votes,
                            a.split_epoch, a.split_failed_epoch, a.bucket_block, a.bucket_fail_streak, a.cur_kind, a.kinds.size(), a.learning.size()};
    memcpy(out, v, sizeof v);
}
// slot i: epoch, last_used, table.sub, n, the cloud's identity; *reach; the first `nkeys` keys of its table
void shim_state_slot(const void* st, int i, uint64_t out[5], float* reach, uint32_t* keys, uint32_t nkeys) {
    const AdaptiveState::SplitterSlot& sl = ((const AdaptiveState*)st)->split_slots[i];
    out[0] = sl.epoch; out[1] = sl.last_used; out[2] = sl.table.sub; out[3] = sl.n; out[4] = (uint64_t)(uintptr_t)sl.cloud;
    *reach = sl.reach;
    memcpy(keys, sl.table.key, (size_t)nkeys * sizeof(uint32_t));
}
// a kind: settled or not; its level and mid-round choice if it is
int shim_state_kind(const void* st, uint64_t kind, uint32_t* level, int* midround) {
    const AdaptiveState& a = *(const AdaptiveState*)st;
    const auto it = a.kinds.find(kind);
    if (it == a.kinds.end()) return 0;
    *level = it->second.sup_level;
    *midround = a.midround(kind) ? 1 : 0;
    return 1;
}
// keys exactly as keygen_kernel stores them (before any final-pass un-inversion)
void shim_sort_keys(const FrameParams* fp, const float* pos_vis, uint32_t n, uint32_t* keys_out) {
    for (uint32_t i = 0; i < n; ++i)
        keys_out[i] = sort_key(*fp, V3{pos_vis[4 * i], pos_vis[4 * i + 1], pos_vis[4 * i + 2]});
}

// the same keys the way the chainless keygen tiles compute them: the straight-line verdict first (sort_key_fast), the
// reference's divisions only for the splats it is unsure about. `unsure_out` counts those.
void shim_sort_keys_two_step(const FrameParams* fp, const float* pos_vis, uint32_t n, uint32_t* keys_out, uint32_t* unsure_out) {
    uint32_t unsure_count = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const V3 p{pos_vis[4 * i], pos_vis[4 * i + 1], pos_vis[4 * i + 2]};
        bool unsure = false;
        uint32_t k;
        if (fp->sort_mode == SORT_NONE) k = sort_key_fast<0>(*fp, p, unsure);
        else if (fp->sort_mode != SORT_RADIX) k = sort_key_fast<2>(*fp, p, unsure);
        else k = sort_key_fast<1>(*fp, p, unsure);
        if (unsure) { k = sort_key(*fp, p); ++unsure_count; }
        keys_out[i] = k;
    }
    *unsure_out = unsure_count;
}

// One draw-list entry through project_splat, the way project_rank (render_kernels.hip) calls it: the Color-only
// instantiation unless another mode is asked for (the launchers' dispatch); cov6 != nullptr is the CLOUD_COV3D call
// (rot and so[0..2] unused, the six covariance entries handed through).
static void project_one(const FrameParams* fp, uint32_t key, const float* pos, const float* rot, const float* so,
                        const float* sh48, const float* cov6, const float* depth_range, ShimOut* out) {
    Projected pr;
    memset(&pr, 0, sizeof pr);
    ColorInputs ci{pos[3], depth_range[0], depth_range[1]};
    if (fp->rasterize_mode == RASTERIZE_COLOR && fp->draw_mode == 0u)
        project_splat<false>(*fp, key, V3{pos[0], pos[1], pos[2]}, rot, so, ShFloat{sh48}, ci, pr, cov6);
    else
        project_splat<true>(*fp, key, V3{pos[0], pos[1], pos[2]}, rot, so, ShFloat{sh48}, ci, pr, cov6);
    memset(out, 0, sizeof *out);
    out->visible = pr.visible;
    out->draw = pr.draw;
    if (!pr.draw) return;
    memcpy(out->color, pr.color, sizeof out->color);
    out->cx = pr.quad.cx;
    out->cy = pr.quad.cy;
    memcpy(out->p, pr.p, sizeof out->p);
    out->radius = pr.radius;
    out->tx0 = pr.tx0; out->ty0 = pr.ty0; out->tx1 = pr.tx1; out->ty1 = pr.ty1;
    out->mean[0] = pr.surfel.mean_x;
    out->mean[1] = pr.surfel.mean_y;
    memcpy(out->T, pr.surfel.T, sizeof out->T);
    out->quad_m[0] = pr.quad.m00; out->quad_m[1] = pr.quad.m01;
    out->quad_m[2] = pr.quad.m10; out->quad_m[3] = pr.quad.m11;
    out->bounds[0] = pr.quad.minx; out->bounds[1] = pr.quad.maxx;
    out->bounds[2] = pr.quad.miny; out->bounds[3] = pr.quad.maxy;
    out->ndc_z = pr.ndc_z;
}

// pos = position_visibility row (4 floats); depth_range = {min_distance, max_distance}
void shim_project(const FrameParams* fp, uint32_t key, const float* pos, const float* rot,
                  const float* so, const float* sh48, const float* depth_range, ShimOut* out) {
    project_one(fp, key, pos, rot, so, sh48, nullptr, depth_range, out);
}

// A whole entry list: out[e] is entry e = (key, index) of `entries` (list order; the device's rank j is entry
// count - 1 - j). The planes are the cloud's, indexed by the entry's index: rot / scale_opacity [n][4], or — a
// precomputed-covariance cloud — cov3d_opacity [n][8] (cov3d[6], opacity, pad) with rot = scale_opacity = NULL, which
// takes project_rank's CLOUD_COV3D branch: rot = identity, so = (0, 0, 0, opacity), the six entries as cov3d_pre.
// cross (may be NULL): [count][9], the surfel record's cross products A = T1 x T2, B = T2 x T0, C = T0 x T1 of
// Surfel::T's columns, formed in double and rounded to float once each, the statements of project_rank.
void shim_project_batch(const FrameParams* fp, const uint32_t* entries, uint32_t count, const float* pos_vis, const float* rot,
                        const float* scale_opacity, const float* sh48, const float* cov3d_opacity, const float* depth_range,
                        ShimOut* out, float* cross) {
    for (uint32_t e = 0; e < count; ++e) {
        const uint32_t key = entries[2 * e], si = entries[2 * e + 1];
        if (cov3d_opacity) {
            const float* c = cov3d_opacity + 8 * (size_t)si;
            const float r1[4] = {1.0f, 0.0f, 0.0f, 0.0f}, so1[4] = {0.0f, 0.0f, 0.0f, c[6]};
            project_one(fp, key, pos_vis + 4 * (size_t)si, r1, so1, sh48 + 48 * (size_t)si, c, depth_range, out + e);
        } else {
            project_one(fp, key, pos_vis + 4 * (size_t)si, rot + 4 * (size_t)si, scale_opacity + 4 * (size_t)si,
                        sh48 + 48 * (size_t)si, nullptr, depth_range, out + e);
        }
        if (cross) {
            const float* T = out[e].T;
            float* x = cross + 9 * (size_t)e;
            const double T0x = T[0], T0y = T[1], T0z = T[2];
            const double T1x = T[3], T1y = T[4], T1z = T[5];
            const double T2x = T[6], T2y = T[7], T2z = T[8];
            x[0] = (float)(T1y * T2z - T1z * T2y); x[1] = (float)(T1z * T2x - T1x * T2z); x[2] = (float)(T1x * T2y - T1y * T2x);
            x[3] = (float)(T2y * T0z - T2z * T0y); x[4] = (float)(T2z * T0x - T2x * T0z); x[5] = (float)(T2x * T0y - T2y * T0x);
            x[6] = (float)(T0y * T1z - T0z * T1y); x[7] = (float)(T0z * T1x - T0x * T1z); x[8] = (float)(T0x * T1y - T0y * T1x);
        }
    }
}

// The two degeneracy decisions of the 2DGS path for one splat (cov2d_surfel, bounding_box_cov2d: `|d| < 1e-4` and
// `extent < 1e-4`), so that a test can show its edge-on clouds hold both outcomes of each: out = extent[0], extent[1],
// and 1 where cov2d_surfel returned at its d test (it then leaves T zero; otherwise T[8] is the centre's clip w, not 0 in the frustum).
void shim_surfel_probe(const FrameParams* fp, const float* pos, const float* rot, const float* so, float out[3]) {
    const V4 t4 = m4_mul_point(fp->transform, V3{pos[0], pos[1], pos[2]});
    Surfel sf;
    cov2d_surfel(*fp, V3{t4.x, t4.y, t4.z}, rot, so, cutoff_radius(*fp, so[3]), sf);
    bool zero = true;
    for (int i = 0; i < 9; ++i) zero = zero && sf.T[i] == 0.0f;
    out[0] = sf.extent[0]; out[1] = sf.extent[1]; out[2] = zero ? 1.0f : 0.0f;
}

float shim_distance_to_camera(const FrameParams* fp, const float* pos) {
    return distance_to_camera(*fp, V3{pos[0], pos[1], pos[2]});
}

}  // extern "C"
