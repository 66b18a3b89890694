// morph_kernels.h — the launcher of morph_kernels.hip, called by the C ABI (bgs_morph_api.hip). It only enqueues on the
// stream it is given and returns the first hipError_t that was not hipSuccess.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "morph_math.h"

namespace bgsm {

constexpr uint32_t GEOMETRY_THREADS = 256;              // one splat a lane
constexpr uint32_t COLOUR_THREADS = 256;                // one float4 of output a lane
constexpr uint32_t COLOUR_QUADS = SH_COEFFS / 4u;       // 12 float4 of coefficients a splat

// One side's planes, n > 0 rows each, every pointer 16-byte aligned. The f32 layout has rotation and scale_opacity and no
// covariance_3d_opacity; the precomputed-covariance layout the other way round. What a layout lacks is nullptr and unread.
struct MorphSide {
    const float4* position_visibility;      // n
    const float4* spherical_harmonic;       // n x 12
    const float4* rotation;                 // n          [w, x, y, z]
    const float4* scale_opacity;            // n
    const float4* covariance_3d_opacity;    // n x 2
};

struct MorphOut {
    float4* position_visibility;
    float4* spherical_harmonic;
    float4* rotation;
    float4* scale_opacity;
    float4* covariance_3d_opacity;
};

// t and u = 1 - t: interpolation_factor() of morph_math.h, taken on the host
hipError_t launch_morph(hipStream_t stream, bool covariance, const MorphSide& lhs, const MorphSide& rhs, const MorphOut& out, uint32_t n,
                        float t, float u);

}  // namespace bgsm
