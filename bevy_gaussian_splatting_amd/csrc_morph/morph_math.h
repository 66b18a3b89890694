// morph_math.h — the per-splat linear blend of two Gaussian clouds (src/morph/interpolate.wgsl interpolate_gaussians,
// the reference's GaussianInterpolate { lhs, rhs }): the output cloud at CloudSettings.time between time_start and
// time_stop. Shared by the device kernels (morph_kernels.hip) and a g++ build (tests/host_shim/morph_math_shim.cpp),
// like csrc_slice/slice_math.h. Written from the WGSL as new code.
//
// ARITHMETIC CONTRACT: f32 throughout, every operation rounded once (both builds use -ffp-contract=off), in this order.
//
//   FACTOR (interpolate.wgsl:51-57), computed ONCE, on the host, by interpolation_factor() below, and handed to the kernels:
//     duration = time_stop - time_start
//     |duration| < 1e-6 (the f32 nearest 1e-6):   t = (time >= time_stop) ? 1 : 0                    the shader's step
//     otherwise:                                  x = (time - time_start) / duration
//                                                 t = x > 0 ? x : 0;  t = t > 1 ? 1 : t              clamp(x, 0, 1)
//     u = 1 - t                                   rounded once, on the host as well
//   A reversed interval (time_stop < time_start) is legal and runs backwards. The quotient may overflow to +-inf; the
//   clamp takes it to 0 or 1. Written with comparisons, the clamp takes a quotient of -0 (time == time_start of a
//   reversed interval) to +0, and there is no NaN to decide: the three times are finite (the C ABI refuses others).
//
//   mix(a, b) = (a * u) + (b * t)                 two products and one sum: WGSL's stated linear blend
//                                                 e1 * (1 - e3) + e2 * e3. It is NOT a + t * (b - a).
//   It is exact at both ends for finite inputs: t = 0 gives a * 1 + b * 0 = a, t = 1 gives b; a -0 may come out +0
//   (-0 + +0). A non-finite lane on the side with weight 0 gives NaN (inf * 0), as it does in the shader. A NaN's sign
//   and payload are no part of the contract.
//
//   PLANES, the f32 planar layout (include/bgs.h, bgs_cloud_upload_f32):
//     position_visibility[n][4]    all four lanes mixed: the visibility is mixed too
//     spherical_harmonic[n][48]    every lane mixed
//     scale_opacity[n][4]          all four lanes mixed
//     rotation[n][4]               stored lane order [w, x, y, z]:
//        q    = mix, lane by lane
//        len2 = ((q0*q0 + q1*q1) + q2*q2) + q3*q3
//        len2 <= 0:   the four stored lanes become (0, 0, 0, 1)
//        otherwise:   q_i / sqrt(len2), the square root and each division correctly rounded
//        a NaN len2 fails <= and yields four NaNs.
//     THE FALLBACK IS NOT THE IDENTITY HERE. The shader's normalize_quaternion returns the literal vec4(0, 0, 0, 1), and
//     the reference hands it the STORED vector as it is. With this project's stored order [w, x, y, z] the literal reads
//     z = 1, w = 0: a half turn about z. It is kept as the reference has it; a pair of antipodal rotations at t = 0.5
//     is where it shows.
//
//   PRECOMPUTED-COVARIANCE LAYOUT (bgs_cloud_upload_cov3d_f32: xx, xy, xz, yy, yz, zz, opacity, pad):
//     covariance_3d_opacity[n][8]  lanes 0..6 mixed, lane 7 written +0 whatever the inputs hold there
//     position and colour as above; there is no rotation and no scale.
//   A STATED DEVIATION: the reference's f32 setter (planar.wgsl:416-429) writes (cov, 0, opacity) and it has no f32
//   getter for the plane at all, so its precomputed f32 morph does not assemble. The layout here is the one this
//   project's renderer reads.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BGSM_HD __host__ __device__ __forceinline__
#else
#define BGSM_HD static inline
#endif

namespace bgsm {

constexpr float STEP_BELOW = 1e-6f;      // |duration| under this: the factor is a step at time_stop
constexpr uint32_t SH_COEFFS = 48;

// t and u = 1 - t of the contract's FACTOR.
struct Factor {
    float t;
    float u;
};

// Host side: called once a morph, never in a kernel.
static inline Factor interpolation_factor(float time, float time_start, float time_stop) {
    const float duration = time_stop - time_start;
    float t;
    if (fabsf(duration) < STEP_BELOW) {
        t = time >= time_stop ? 1.0f : 0.0f;
    } else {
        const float x = (time - time_start) / duration;
        t = x > 0.0f ? x : 0.0f;
        t = t > 1.0f ? 1.0f : t;
    }
    Factor f;
    f.t = t;
    f.u = 1.0f - t;
    return f;
}

BGSM_HD float mix(float a, float b, float t, float u) { return (a * u) + (b * t); }

BGSM_HD void mix4(const float a[4], const float b[4], float t, float u, float out[4]) {
    for (int k = 0; k < 4; ++k) out[k] = mix(a[k], b[k], t, u);
}

// Stored lanes [w, x, y, z] in and out; the fallback is the shader's literal in STORED order (see the contract).
BGSM_HD void normalize_quaternion(const float q[4], float out[4]) {
    const float len2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
    if (len2 <= 0.0f) {
        out[0] = 0.0f;
        out[1] = 0.0f;
        out[2] = 0.0f;
        out[3] = 1.0f;
        return;
    }
    const float len = sqrtf(len2);
    for (int k = 0; k < 4; ++k) out[k] = q[k] / len;
}

BGSM_HD void mix_rotation(const float a[4], const float b[4], float t, float u, float out[4]) {
    float q[4];
    mix4(a, b, t, u, q);
    normalize_quaternion(q, out);
}

// One splat's covariance_3d_opacity record, eight lanes: 0..6 mixed, the pad +0.
BGSM_HD void mix_covariance(const float a[8], const float b[8], float t, float u, float out[8]) {
    for (int k = 0; k < 7; ++k) out[k] = mix(a[k], b[k], t, u);
    out[7] = 0.0f;
}

}  // namespace bgsm
