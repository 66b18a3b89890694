// adaptive_state.h — what completed frames leave for the next ones (host, plain C++: no HIP type, no context, no lane).
// AdaptiveState owns every learnt member and every rule that writes one; bgs_frame.hip and bgs_api.hip call the rules with
// plain values and READ the members (plan_frame through a const reference). Counters stay in bgs_ctx: a rule that has
// something to count returns it. tests/test_adaptive_state_host.py drives the rules through the host shim, without a GPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <unordered_map>

#include "frame_params.h"

namespace bgs {

// camera pose of a view: world position and viewing direction (-Z of the view frame)
inline void view_pose(const bgs_view* v, float pos[3], float fwd[3]) {
    for (int k = 0; k < 3; ++k) { pos[k] = v->world_from_view[12 + k]; fwd[k] = -v->world_from_view[8 + k]; }
    const float len = std::sqrt(fwd[0] * fwd[0] + fwd[1] * fwd[1] + fwd[2] * fwd[2]);
    if (len > 0.0f) for (int k = 0; k < 3; ++k) fwd[k] /= len;
}

// What AdaptiveState::kinds is keyed by: a hash of the inputs the data-dependent capacities depend on (never 0). The cloud
// enters by its size and storage format, not by its address (a host that uploads a new cloud per frame — a stream of
// same-sized captures — stays pipelined; a different cloud of the same size is at worst a re-run, as for any stale
// hint), the global scale to half an octave (an animated scale crosses a step now and then, not with every frame).
inline uint64_t frame_kind(uint32_t n, uint32_t format, const bgs_view* view, const bgs_settings* s) {
    int32_t scale_step = INT32_MIN;
    if (s->global_scale > 0.0f && std::isfinite(s->global_scale)) scale_step = (int32_t)std::lround(2.0 * std::log2((double)s->global_scale));
    const uint64_t words[6] = {((uint64_t)n << 32) | format, ((uint64_t)s->gaussian_mode << 32) | s->aabb,
                               ((uint64_t)(uint32_t)scale_step << 32) | s->opacity_adaptive_radius,
                               ((uint64_t)(uint32_t)view->viewport[2] << 32) | (uint32_t)view->viewport[3],
                               ((uint64_t)(view->sample_count ? view->sample_count : 4u) << 32) | (view->depth_device_ptr ? 1u : 0u),
                               ((uint64_t)s->rasterize_mode << 32) | (s->draw_mode << 1) | (s->visualize_bounding_box ? 1u : 0u)};
    uint64_t hsh = 0xcbf29ce484222325ull;   // FNV-1a over the words
    for (uint64_t w : words)
        for (int b = 0; b < 8; ++b) { hsh ^= (w >> (8 * b)) & 0xFFu; hsh *= 0x100000001b3ull; }
    return hsh ? hsh : 1ull;
}

// ---- tile instances (BINNING_SORT) ---------------------------------------------------------------------------------------
constexpr uint64_t MIN_INSTANCE_CAPACITY = 1ull << 22;  // 4M instances (32 MB per buffer)
constexpr uint64_t MAX_INSTANCE_CAPACITY = 1ull << 30;  // look-back words carry 30-bit values
// The host's answer to a BINNING_SORT frame that needed `need` tile instances and overflowed its buffer: refused past the
// limit, else the next power of two that holds the need with 25 % head-room, within [MIN, MAX]. Not learnt state: each
// lane's buffers grow by it on their own (check_capacities), and nothing shrinks.
struct InstanceVerdict { bool refuse; uint64_t capacity; };
inline InstanceVerdict instance_capacity_for(uint64_t need) {
    if (need > MAX_INSTANCE_CAPACITY) return {true, 0};
    uint64_t cap = MIN_INSTANCE_CAPACITY;
    while (cap < need + need / 4) cap <<= 1;
    return {false, std::min(cap, MAX_INSTANCE_CAPACITY)};
}

// Whose sorted list a splitter table describes: the cloud (by identity and size), the camera and the settings.
struct SortedView {
    const void* cloud;
    uint32_t n;
    const bgs_view* view;
    const bgs_settings* settings;
};

struct AdaptiveState {
    // Sizes the grids of the next frames' sort and projection launches: the draw_count of a completed
    // frame plus head-room, raised at once and lowered only after 64 frames at under a quarter of it, so that a
    // captured frame graph (whose grids are frozen) survives a moving camera. A hint only — the
    // kernels read the real count on the device and loop over tickets if the grid is short.
    uint32_t draw_hint = 0;
    bool draw_hint_valid = false;
    uint32_t draw_shrink_votes = 0;
    uint32_t sup_level = 1;  // supertile edge level of the next frames (see plan_frame)
    // Bucket sort (one launch instead of four digit passes) is used while a completed frame's quantile keys
    // are known, the draw count fits the bucket geometry, and it has not just failed.
    // Splitter tables: the quantile keys of completed frames' sorted lists, kept per "view slot" — a context that
    // alternates between cameras (the reference's multi_camera example), clouds or model transforms would
    // otherwise hand every frame the table of the wrong view. A table is used for a frame of the same cloud and
    // transform whose camera is near the pose it was measured at; it is dropped when a frame it served overflows.
    struct SplitterSlot {
        SplitterKeys table{};
        const void* cloud = nullptr;
        uint32_t n = 0;
        uint32_t sort_mode = 0;   // Radix culls (a frustum's worth of keys), Rayon / Std keep every splat
        float transform[16] = {};
        float pos[3] = {}, fwd[3] = {};
        // SORT_RADIX keys only what the frustum keeps, so the key set also depends on the projection and viewport:
        // two cameras at one pose with different fov / zoom / target size must not share (and overwrite) a table
        float clip_from_view[16] = {};
        float viewport_wh[2] = {};
        float reach = 0.0f;       // median view distance of the list the table came from (scale of "near")
        uint64_t epoch = 0;       // 0 = empty
        uint64_t last_used = 0;
    };
    static constexpr int SPLITTER_SLOTS = 16;  // (16 KB each; the key includes the projection since round 3, so zooms / resizes take slots too)
    SplitterSlot split_slots[SPLITTER_SLOTS];
    uint64_t split_epoch = 0;         // epochs handed out so far
    uint64_t split_failed_epoch = 0;  // newest epoch whose table overflowed (escalation looks at newer ones only)
    uint32_t bucket_block = 0;        // frames to stay on the onesweep passes after a bucket-sort overflow
    uint32_t bucket_fail_streak = 0;  // tables in a row that overflowed on their first use
    uint32_t list_shrink_votes = 0;   // completed frames in a row whose lists would fit a much smaller capacity
    // entries per supertile list the next frames allocate (grown from the longest list seen; a frame whose
    // lists overflow is re-run): the worst case is n entries in each of up to 256 lists (1.9 GB per lane at
    // 1 M splats), the real lists of a frame hold ~1 % of that
    uint32_t coarse_cap_hint = 0;
    // KINDS OF FRAME. What a completed frame teaches (list capacity, supertile level) depends on the kind of frame it was:
    // (splat count and storage format of the cloud, mode, quad shape, global scale to half an octave, viewport size,
    // sample count, depth buffer or not) — frame_kind(); poses do not count, a moving camera stays pipelined. An async
    // frame of a kind the context has not settled on is completed at once (re-running it if a first guess was too
    // small) instead of sending pipeline-depth frames out on first guesses and re-running every one of them (round 3's
    // verdict: "reruns: 8" on every first use); the frames behind it start from what it learnt. A kind is settled once
    // a frame of it has run with everything it needed (no re-run, no change of supertile level) — or, at the latest,
    // after LEARN_MAX frames of it IN TOTAL were completed early (a frame that always re-runs, a level that oscillates:
    // bounded, not a phase the context can stay in — counted per kind since round 6: round 5 counted frames "in a row",
    // and a host that alternated two kinds that never ran clean reset the streak with every frame and stayed blocking). The set NEVER FORGETS (round 4 kept the last 16 kinds FIFO and
    // hashed the cloud's ADDRESS and the raw scale bits into the kind: a host with more than 16 clouds or settings, a new
    // cloud handle per frame or an animated global_scale lost its pipelining for good, silently), and every kind keeps
    // its own supertile level, so a context that alternates between kinds does not run each at the other's level.
    // midround: frames of the kind run the rasteriser's mid-round-exit instantiation whatever their supertile level — set
    // (with hysteresis) from the share of a completed frame's tiles that ended SATURATED rather than at the end of their
    // lists (round 6: a cloud of opaque surfaces saturates its tiles inside a staging round like a dense one does)
    struct KindState { uint32_t sup_level = 1; bool midround = false; };
    std::unordered_map<uint64_t, KindState> kinds;   // the kinds settled on (8 + 4 bytes each)
    static constexpr uint32_t LEARN_MAX = 3;
    // share of a frame's tile work in tiles that ended saturated at/above which frames of its kind run the mid-round-exit
    // rasteriser, and at/below which they stop (hysteresis; measured: profiles/r6_notes.md §9)
    static constexpr double MIDROUND_ON = 0.30, MIDROUND_OFF = 0.15;
    uint64_t cur_kind = 0;          // kind of the most recently enqueued frame (sup_level is that kind's level)
    std::unordered_map<uint64_t, uint32_t> learning;   // kinds being learnt: frames of each completed early so far

    // ---- kinds ---------------------------------------------------------------------------------------------------------
    bool settled(uint64_t kind) const { return kinds.find(kind) != kinds.end(); }
    // whether frames of the kind run the mid-round-exit rasteriser (false for a kind not settled on)
    bool midround(uint64_t kind) const {
        const auto it = kinds.find(kind);
        return it != kinds.end() && it->second.midround;
    }
    // The frame about to be enqueued is of `kind`: sup_level becomes that kind's level (if it has one).
    void switch_kind(uint64_t kind) {
        if (kind == cur_kind) return;
        const auto it = kinds.find(kind);
        if (it != kinds.end()) sup_level = it->second.sup_level;
        cur_kind = kind;
    }
    // the kind is settled: a frame of it ran at `level` with everything it needed
    void settle(uint64_t kind, uint32_t level) {
        if (kinds.size() >= (1u << 20)) kinds.clear();   // (12 MB of kinds: a host that hashes noise into its settings)
        kinds[kind].sup_level = level;
    }
    // A frame of a kind that was not settled when it was enqueued has been completed early. Bounded: a kind whose frames
    // never run clean (every frame re-run, a level that oscillates) is settled on anyway, at the level the context is on.
    void completed_early(uint64_t kind) {
        if (settled(kind)) {
            learning.erase(kind);   // (it ran clean: settle() was called)
        } else if (++learning[kind] >= LEARN_MAX) {
            kinds[kind].sup_level = sup_level;
            learning.erase(kind);
        }
        if (learning.size() >= (1u << 16)) learning.clear();   // (a host that hashes noise into its settings)
    }
    // What the cost plane of a frame of `kind` said: the share of its tile work that was in tiles which ended saturated
    // (tile_order_kernel sums, a later frame's clean-up block reports; x 0x7FFF, 0xFFFFFFFF: no report) moves the kind's
    // mid-round-exit choice
    void learn_saturation(uint64_t kind, uint32_t saturated_x7fff) {
        if (!kind || saturated_x7fff == 0xFFFFFFFFu) return;
        const auto kit = kinds.find(kind);
        if (kit == kinds.end()) return;
        const double share = (double)saturated_x7fff / (double)0x7FFF;
        if (share >= MIDROUND_ON) kit->second.midround = true;
        else if (share <= MIDROUND_OFF) kit->second.midround = false;
    }

    // ---- draw count ----------------------------------------------------------------------------------------------------
    // the draw-count hint (up at once; down only after 64 completed frames in a row at under a quarter of it: a context
    // that cycles through cameras seeing different shares of the cloud keeps one hint — and one captured graph per lane)
    void learn_draw_count(uint32_t draw_count) {
        if (!draw_hint_valid || draw_count > draw_hint) {
            draw_hint = (uint32_t)std::min<uint64_t>((uint64_t)draw_count + draw_count / 8 + 1024, 0xFFFFFFFFull);
            draw_hint_valid = true;
            draw_shrink_votes = 0;
        } else if ((uint64_t)draw_count * 4 < draw_hint) {
            if (++draw_shrink_votes >= 64u) {
                draw_hint = (uint32_t)std::min<uint64_t>((uint64_t)draw_count * 2 + 1024, 0xFFFFFFFFull);
                draw_shrink_votes = 0;
            }
        } else {
            draw_shrink_votes = 0;
        }
    }

    // ---- splitter tables -----------------------------------------------------------------------------------------------
    // The splitter slot that fits a frame (same cloud, sort mode and model transform, camera within 5 % of the
    // slot's reach and 10 degrees of its direction), or -1.
    int find_splitter_slot(const SortedView& f) const {
        const bgs_view* view = f.view;
        const bgs_settings* s = f.settings;
        float pos[3], fwd[3];
        view_pose(view, pos, fwd);
        int best = -1;
        float best_d = 0.0f;
        for (int i = 0; i < SPLITTER_SLOTS; ++i) {
            const auto& sl = split_slots[i];
            if (!sl.epoch || sl.cloud != f.cloud || sl.n != f.n || sl.sort_mode != s->sort_mode) continue;
            if (std::memcmp(sl.transform, s->transform, sizeof sl.transform) != 0) continue;
            if (s->sort_mode == BGS_SORT_RADIX &&
                (std::memcmp(sl.clip_from_view, view->clip_from_view, sizeof sl.clip_from_view) != 0 ||
                 sl.viewport_wh[0] != view->viewport[2] || sl.viewport_wh[1] != view->viewport[3]))
                continue;
            const float dx = pos[0] - sl.pos[0], dy = pos[1] - sl.pos[1], dz = pos[2] - sl.pos[2];
            const float d = std::sqrt(dx * dx + dy * dy + dz * dz);
            const float c = fwd[0] * sl.fwd[0] + fwd[1] * sl.fwd[1] + fwd[2] * sl.fwd[2];
            if (!(d <= 0.05f * sl.reach) || !(c >= 0.9848f)) continue;
            const float score = d / std::max(sl.reach, 1e-30f) + (1.0f - c);
            if (best < 0 || score < best_d) { best = i; best_d = score; }
        }
        return best;
    }
    // A completed frame's sorted list is good: its quantile keys (`keys`: 256 * sub - 1 of them, what the frame's clean-up
    // was asked for) balance the buckets of the next frames of its view. bucket() is only monotone for an ascending
    // table, so that is checked, not assumed. `seq`: the context's frame sequence number, the slots' clock.
    void store_splitters(const uint32_t* keys, uint32_t sub, uint32_t places, uint32_t draw_count, const SortedView& f, uint64_t seq) {
        const uint32_t nkeys = BUCKET_COUNT * sub - 1u;
        if (places != 4 || draw_count < BUCKET_COUNT || !splitters_ascending(keys, nkeys) || !f.cloud) return;
        int slot = find_splitter_slot(f);
        if (slot < 0) {  // a view not seen lately: take an empty slot, else the least recently used one
            slot = 0;
            for (int i = 0; i < SPLITTER_SLOTS; ++i) {
                if (!split_slots[i].epoch) { slot = i; break; }
                if (split_slots[i].last_used < split_slots[slot].last_used) slot = i;
            }
        }
        auto& sl = split_slots[slot];
        std::memcpy(sl.table.key, keys, nkeys * sizeof(uint32_t));
        sl.table.sub = sub;
        sl.cloud = f.cloud;
        sl.n = f.n;
        sl.sort_mode = f.settings->sort_mode;
        std::memcpy(sl.transform, f.settings->transform, sizeof sl.transform);
        view_pose(f.view, sl.pos, sl.fwd);
        std::memcpy(sl.clip_from_view, f.view->clip_from_view, sizeof sl.clip_from_view);
        sl.viewport_wh[0] = f.view->viewport[2];
        sl.viewport_wh[1] = f.view->viewport[3];
        // the median key is ~bits(dist^2) of the median drawable splat (keys are 0xFFFFFFFF - bits)
        const uint32_t mid_bits = 0xFFFFFFFFu - keys[BUCKET_COUNT * sub / 2 - 1];
        float d2;
        std::memcpy(&d2, &mid_bits, 4);
        sl.reach = (d2 > 0.0f && d2 < 3.0e38f) ? std::sqrt(d2) : 1.0f;
        sl.epoch = ++split_epoch;
        sl.last_used = seq;
    }
    void drop_tables() { for (auto& sl : split_slots) sl.epoch = 0; }

    // ---- bucket sort ---------------------------------------------------------------------------------------------------
    // A frame is enqueued: the block after an overflow counts down with every frame that could have taken the bucket sort
    // (4 digit places), and the table the frame sorts with (`slot`, -1: none) is the most recently used one.
    void frame_enqueued(uint32_t places, int slot, uint64_t seq) {
        if (bucket_block > 0 && places == 4) bucket_block -= 1;
        if (slot >= 0) split_slots[slot].last_used = seq;
    }
    // The verdict of a completed bucket-sort frame that sorted with the table of `slot` as it was at `epoch` (-1, 0: a
    // guessed table). Returns whether the frame must be run again on the digit passes.
    // A bucket over capacity (sort_overflow & 1): the view changed faster than the splitters follow; the table is dropped
    // and the re-run delivers a fresh one. Frames already in flight with the same stale table fail for the same reason,
    // so only a table NEWER than the last failed one counts towards the back-off (three such tables in a row: 7, 15, ...
    // 255 frames on the passes). One key value far too often (& 2): no table can split that; 256 frames on the passes.
    bool learn_bucket_sort(uint32_t sort_overflow, int slot, uint64_t epoch) {
        if (!sort_overflow) {
            bucket_fail_streak = 0;
            return false;
        }
        if (slot >= 0 && split_slots[slot].epoch == epoch) split_slots[slot].epoch = 0;  // drop the table
        if (sort_overflow & 2u) {
            bucket_block = 256u;
        } else if (epoch > split_failed_epoch) {
            bucket_fail_streak = std::min(bucket_fail_streak + 1u, 8u);
            if (bucket_fail_streak >= 3u) bucket_block = (1u << bucket_fail_streak) - 1u;
        }
        split_failed_epoch = std::max(split_failed_epoch, epoch);
        return true;
    }

    // ---- supertile lists -----------------------------------------------------------------------------------------------
    // entries per supertile list the next frame of a cloud of n splats asks for; a first guess if nothing is known yet (a
    // frame that outgrows it is re-run; small_lists: BGS_DEBUG_SMALL_LISTS, which exists to exercise that)
    uint32_t list_capacity(uint32_t n, bool small_lists) {
        const uint32_t n1 = std::max<uint32_t>(n, 1);
        if (coarse_cap_hint == 0) coarse_cap_hint = small_lists ? 64u : std::max<uint32_t>(pow2_ceil_u32(n1 / 64u), 4096u);
        return std::min<uint32_t>(n1, coarse_cap_hint);
    }
    // A completed BINNING_SCAN frame that ran at `level` with lists of `capacity` entries, the longest of which wanted
    // `longest`. The capacity the next allocations aim at follows the longest list SEEN (25 % head-room, power of two): up
    // at once, down only after 64 completed frames in a row that would fit an eighth of it. Returns whether this frame
    // dropped entries (it must be run again).
    bool learn_list_capacity(uint32_t longest, uint32_t level, uint32_t capacity) {
        const uint32_t want = std::max<uint32_t>(pow2_ceil_u32((uint64_t)longest + longest / 4), 4096u);
        if (level == sup_level) {
            if (want > coarse_cap_hint) {
                coarse_cap_hint = want;
                list_shrink_votes = 0;
            } else if ((uint64_t)want * 8u <= coarse_cap_hint) {
                if (++list_shrink_votes >= 64u) { coarse_cap_hint = want * 2u; list_shrink_votes = 0; }
            } else {
                list_shrink_votes = 0;
            }
        }
        if (longest <= capacity) return false;
        if (want > coarse_cap_hint) coarse_cap_hint = want;
        return true;
    }
    // List entries per visible splat (~1.2 when splats are smaller than a supertile, 15-20 when they span many) -> the
    // supertile level of the next frames (next_supertile_level, frame_params.h; relative to the level `lv` THIS frame ran
    // at, not to sup_level, which frames completed in the meantime may already have moved).
    // moved: the frame asks for another level than it ran at; changed: sup_level went there (the caller counts it).
    struct LevelVerdict { bool moved, changed; };
    LevelVerdict learn_level(uint64_t kind, uint32_t lv, const uint32_t edges[4], uint64_t instances, uint32_t visible, uint32_t longest) {
        double longer = 1.0;
        // (a level whose edge equals a lower level's is that lower level: moving between them is not a change — no new
        // capacity prediction, no vote reset, no level_changes)
        const uint32_t target = canonical_supertile_level(next_supertile_level((double)instances / (double)visible, lv, edges, &longer), edges);
        const auto kit = kinds.find(kind);
        // (a settled kind remembers its level for the next time the context comes back to it)
        if (kit != kinds.end()) kit->second.sup_level = target;
        // a frame of ANOTHER kind than the one the context is on by now (kinds alternate while frames are in flight): its
        // verdict belongs to its own kind, not to sup_level
        if (kind != cur_kind || target == lv) return {target != lv, false};
        if (sup_level == target) return {true, false};
        // lists of another level: predicted from THIS frame's longest list (coarser supertiles hold longer lists:
        // entries scale with the ratio, lists with the area), never from the old hint
        const double predicted = (double)longest * (target > lv ? longer : 1.0) * 1.25;
        coarse_cap_hint = std::max<uint32_t>(pow2_ceil_u32((uint64_t)std::min(predicted, 1.0e9)), 4096u);
        list_shrink_votes = 0;
        sup_level = target;
        return {true, true};
    }

    // ---- forgetting ----------------------------------------------------------------------------------------------------
    // Nothing a frame that tripped the device watchdog left behind is trusted: not its counters
    void distrust() {
        draw_hint_valid = false;
        drop_tables();
    }
    // a later cloud may get the same address
    void forget_cloud(const void* cloud) {
        for (auto& sl : split_slots)
            if (sl.cloud == cloud) sl.epoch = 0;
    }
    // The context learns everything anew (bgs_reset_adaptive_state). Member by member, against a new state:
    //   draw_hint, draw_shrink_votes: kept, and never read while draw_hint_valid is false — the first learn_draw_count
    //       then sets both.
    //   split_slots: emptied (epoch 0). What an empty slot holds besides is never read: find_splitter_slot skips it,
    //       store_splitters takes the FIRST empty slot before it compares any last_used, and writes every field.
    //   split_epoch: kept, so epochs stay monotonic — a table stored after the reset never carries the epoch of one
    //       handed out before it. split_failed_epoch = split_epoch: no table from before the reset is "newer than the
    //       last failed one", exactly as no table is in a new state (both 0); only the difference of the two is ever used.
    //   everything else: the value a new state starts with.
    void reset() {
        draw_hint_valid = false;
        drop_tables();
        split_failed_epoch = split_epoch;
        bucket_block = 0;
        bucket_fail_streak = 0;
        list_shrink_votes = 0;
        sup_level = 1;
        coarse_cap_hint = 0;
        kinds.clear();
        cur_kind = 0;
        learning.clear();
    }
};

}  // namespace bgs
