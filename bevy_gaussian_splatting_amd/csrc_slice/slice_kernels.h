// slice_kernels.h — the launcher of slice_kernels.hip, called by the C ABI (bgs_slice_api.hip). It only enqueues on the
// stream it is given and returns the first hipError_t that was not hipSuccess.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "slice_math.h"

namespace bgst {

constexpr uint32_t GEOMETRY_THREADS = 256;                    // one splat a lane
constexpr uint32_t FOLD_QUADS = SH_COEFFS / 4u;               // 12 float4 of folded coefficients a splat
constexpr uint32_t FOLD_SPLATS = 16;                          // splats a workgroup of the fold
constexpr uint32_t FOLD_THREADS = FOLD_SPLATS * FOLD_QUADS;   // 192 lanes, three waves: one float4 of output a lane

// The five planes of a 4D cloud in, the three planes of its slice out; n > 0 rows each, every pointer 16-byte aligned.
struct SlicePlanes {
    const float4* position_visibility;      // n
    const float4* spherindrical_harmonic;   // n x 36
    const float4* isotropic_rotations;      // n x 2
    const float4* scale_opacity;            // n
    const float4* timestamp_timescale;      // n
    float4* out_position_visibility;        // n
    float4* out_spherical_harmonic;         // n x 12
    float4* out_covariance_3d_opacity;      // n x 2
};

// duration = time_stop - time_start
hipError_t launch_slice(hipStream_t stream, const SlicePlanes& planes, uint32_t n, float global_scale, float time, float duration);

}  // namespace bgst
