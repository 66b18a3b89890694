// bounds_math.h — the box of a resident cloud, CommonCloud::compute_aabb (src/gaussian/interface.rs:22-63), which the
// reference hands its shaders as CloudUniform.min / .max (src/render/mod.rs:1070-1071). Shared by the device kernel
// (bounds_kernels.hip), the host side that decodes its six words (bgs_frame.hip) and a g++ build
// (tests/host_shim/bounds_shim.cpp), like particle_math.h.
//
// CONTRACT (BGS_BOUNDS_CLOUD, include/bgs.h). Per axis a of x, y, z, over the UNTRANSFORMED position_visibility[i].xyz of
// the cloud's n > 0 splats, in f32, every operation rounded once:
//     min[a] = fold(+inf, f32::min) over fl(p_i[a] - 0.1f)          max[a] = fold(-inf, f32::max) over fl(p_i[a] + 0.1f)
// f32::min / f32::max ignore a NaN operand: a NaN lane contributes nothing to its axis. +-inf propagate. An axis with no
// contributor at all keeps +inf / -inf. The visibility lane (w) is NOT read: a splat that is not drawn still counts, as in
// the reference. The numpy twin is bevy_gaussian_splatting_amd/bounds.py bounds_reference, compared bit for bit.
//
// WHY THE KERNEL MAY REDUCE RAW COORDINATES and apply the offset once at the end: x -> fl(x - 0.1f) is monotone
// non-decreasing (rounding to nearest is monotone, and -inf, +inf map to themselves), so it commutes with min:
//     min_i fl(p_i - 0.1f) = fl((min_i p_i) - 0.1f)      bit for bit, and the same for max with fl(x + 0.1f).
// The one place where "min of the raw values" is not a single bit pattern is a zero: min(-0, +0) may be either. The sign
// of a zero never reaches the result, because a zero -+ 0.1f is never zero. So the result does not depend on the order the
// splats are visited in, nor on how partial results are combined: device, g++ build and twin agree bitwise on every input.
//
// THE ORDER-PRESERVING ENCODING. The device merges the workgroups' partial results with INTEGER atomicMin / atomicMax on
//     key(bits) = bits ^ (sign ? 0xFFFFFFFF : 0x80000000)
// under which unsigned order is the order of the floats: -inf < negative < -0 < +0 < positive < +inf (< the NaNs with a
// clear sign bit, which no workgroup ever merges: a lane's running values never become NaN). The min words start at all-ones
// and the max words at zero, which every merged value beats.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define BGS_BOUNDS_HD __host__ __device__ __forceinline__
#else
#define BGS_BOUNDS_HD static inline
#endif

namespace bgs {

constexpr float BOUNDS_MAX_SCALE = 0.1f;              // interface.rs:31 `max_scale`
constexpr uint32_t BOUNDS_WORDS = 6u;                 // min x, y, z then max x, y, z
constexpr uint32_t BOUNDS_MIN_PRESET = 0xFFFFFFFFu;   // what the three min words hold before the launch
constexpr uint32_t BOUNDS_MAX_PRESET = 0u;            // ... and the three max words
constexpr uint32_t BOUNDS_POS_INF_BITS = 0x7F800000u, BOUNDS_NEG_INF_BITS = 0xFF800000u;

// One fold step on raw coordinates: a NaN p compares false and is skipped; acc starts at +-inf and never becomes NaN.
BGS_BOUNDS_HD float bounds_fold_min(float acc, float p) { return p < acc ? p : acc; }
BGS_BOUNDS_HD float bounds_fold_max(float acc, float p) { return p > acc ? p : acc; }

// The offset, once, on a folded raw coordinate.
BGS_BOUNDS_HD float bounds_finish_min(float raw) { return raw - BOUNDS_MAX_SCALE; }
BGS_BOUNDS_HD float bounds_finish_max(float raw) { return raw + BOUNDS_MAX_SCALE; }

BGS_BOUNDS_HD uint32_t bounds_key(uint32_t bits) { return bits ^ ((bits & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u); }
BGS_BOUNDS_HD uint32_t bounds_key_bits(uint32_t key) { return key ^ ((key & 0x80000000u) ? 0x80000000u : 0xFFFFFFFFu); }

// (host) The six device words -> the box: a word still at its preset (nothing was merged) reads as +inf / -inf.
static inline void bounds_decode(const uint32_t words[BOUNDS_WORDS], float mn[3], float mx[3]) {
    for (int a = 0; a < 3; ++a) {
        const uint32_t lo = words[a] == BOUNDS_MIN_PRESET ? BOUNDS_POS_INF_BITS : bounds_key_bits(words[a]);
        const uint32_t hi = words[3 + a] == BOUNDS_MAX_PRESET ? BOUNDS_NEG_INF_BITS : bounds_key_bits(words[3 + a]);
        float raw_lo, raw_hi;
        memcpy(&raw_lo, &lo, 4);
        memcpy(&raw_hi, &hi, 4);
        mn[a] = bounds_finish_min(raw_lo);
        mx[a] = bounds_finish_max(raw_hi);
    }
}

// (host) The contract as the reference writes it: one splat after the other, the offset per splat.
static inline void bounds_fold_reference(const float* position_visibility, uint32_t n, float mn[3], float mx[3]) {
    uint32_t pinf = BOUNDS_POS_INF_BITS, ninf = BOUNDS_NEG_INF_BITS;
    for (int a = 0; a < 3; ++a) {
        memcpy(&mn[a], &pinf, 4);
        memcpy(&mx[a], &ninf, 4);
    }
    for (uint32_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            const float p = position_visibility[4u * (size_t)i + a];
            mn[a] = bounds_fold_min(mn[a], bounds_finish_min(p));
            mx[a] = bounds_fold_max(mx[a], bounds_finish_max(p));
        }
}

// (host) What the device does: fold raw coordinates in `parts` interleaved partial results (a stand-in for lanes and
// workgroups), merge them as keys with integer min / max onto the preset words, decode.
static inline void bounds_fold_device_order(const float* position_visibility, uint32_t n, uint32_t parts, float mn[3], float mx[3]) {
    uint32_t words[BOUNDS_WORDS] = {BOUNDS_MIN_PRESET, BOUNDS_MIN_PRESET, BOUNDS_MIN_PRESET, BOUNDS_MAX_PRESET, BOUNDS_MAX_PRESET, BOUNDS_MAX_PRESET};
    if (parts == 0u) parts = 1u;
    for (uint32_t part = 0; part < parts && part < n; ++part) {
        float lo[3], hi[3];
        uint32_t pinf = BOUNDS_POS_INF_BITS, ninf = BOUNDS_NEG_INF_BITS;
        for (int a = 0; a < 3; ++a) {
            memcpy(&lo[a], &pinf, 4);
            memcpy(&hi[a], &ninf, 4);
        }
        for (uint64_t i = part; i < n; i += parts)
            for (int a = 0; a < 3; ++a) {
                const float p = position_visibility[4u * (size_t)i + a];
                lo[a] = bounds_fold_min(lo[a], p);
                hi[a] = bounds_fold_max(hi[a], p);
            }
        for (int a = 0; a < 3; ++a) {
            uint32_t lo_bits, hi_bits;
            memcpy(&lo_bits, &lo[a], 4);
            memcpy(&hi_bits, &hi[a], 4);
            const uint32_t lo_key = bounds_key(lo_bits), hi_key = bounds_key(hi_bits);
            words[a] = lo_key < words[a] ? lo_key : words[a];
            words[3 + a] = hi_key > words[3 + a] ? hi_key : words[3 + a];
        }
    }
    bounds_decode(words, mn, mx);
}

// The grid of the reduction (bounds_kernels.hip): 256-thread workgroups, one per 256 splats, at most two per compute unit
// (a 5 M cloud: two workgroups on every CU, each lane striding over ~38 splats), fewer under a grid cap (bgs_set_grid_cap).
// Lane t of workgroup b visits splats b * 256 + t + k * (256 * grid): one sweep reaches 256 * grid splats.
constexpr uint32_t BOUNDS_THREADS = 256u;
static inline uint32_t bounds_grid(uint32_t n, uint32_t compute_units, uint32_t grid_cap) {
    uint64_t most = 2ull * (compute_units ? compute_units : 1u);
    if (grid_cap && grid_cap < most) most = grid_cap;
    const uint64_t tiles = ((uint64_t)n + BOUNDS_THREADS - 1u) / BOUNDS_THREADS;
    return (uint32_t)(tiles < most ? tiles : most);
}

}  // namespace bgs
