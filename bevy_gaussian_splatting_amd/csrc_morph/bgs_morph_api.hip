// bgs_morph_api.hip — the C ABI of libbgs_morph.so (include/bgs_morph.h) over the launcher of morph_kernels.hip.
#include <math.h>

#include "../../include/bgs_morph.h"
#include "build_id.inc"
#include "morph_kernels.h"
#include "../small_lib/api_support_hip.h"

// The SHA-256 of the sources this library was compiled from (../_build_id.py libbgs_morph), readable from the
// file's bytes: the loader rebuilds a library that carries another one.
extern "C" __attribute__((used, visibility("hidden"))) const char bgsm_build_id_marker[] = "BGSM_BUILD_ID=" BGSM_BUILD_ID;

static_assert(BGSM_EINVAL == API_EINVAL && BGSM_ENOMEM == API_ENOMEM && BGSM_EHIP == API_EHIP, "the shared support's status codes");

namespace {

// Both entry points: `planes` holds the lhs's planes, then the rhs's, then the output's, `per_side` each. Everything is
// validated before a device is touched.
int interpolate(const char* fn, bool covariance, int hip_device, void* hip_stream, uint32_t n, const Named* planes, int per_side, float time,
                float time_start, float time_stop) {
    g_error[0] = 0;
    const char* const names[3] = {"time", "time_start", "time_stop"};
    const float values[3] = {time, time_start, time_stop};
    for (int k = 0; k < 3; ++k)
        if (!isfinite(values[k])) return fail(BGSM_EINVAL, "%s: %s %g must be finite", fn, names[k], (double)values[k]);
    if (n == 0u) return BGSM_OK;
    const int inputs = 2 * per_side, count = 3 * per_side;
    if (const int refused = check_planes(fn, planes, inputs, count)) return refused;
    if (const int refused = check_device(fn, hip_device)) return refused;
    DeviceScope scope(hip_device);
    if (scope.status() != hipSuccess) return fail_hip("hipSetDevice", scope.status());
    bgsm::MorphSide side[2];
    for (int s = 0; s < 2; ++s) {
        const Named* p = planes + s * per_side;
        side[s] = {(const float4*)p[0].ptr, (const float4*)p[1].ptr, covariance ? nullptr : (const float4*)p[2].ptr,
                   covariance ? nullptr : (const float4*)p[3].ptr, covariance ? (const float4*)p[2].ptr : nullptr};
    }
    const Named* o = planes + inputs;
    const bgsm::MorphOut out = {(float4*)o[0].ptr, (float4*)o[1].ptr, covariance ? nullptr : (float4*)o[2].ptr,
                                covariance ? nullptr : (float4*)o[3].ptr, covariance ? (float4*)o[2].ptr : nullptr};
    const bgsm::Factor f = bgsm::interpolation_factor(time, time_start, time_stop);
    const hipError_t e = bgsm::launch_morph((hipStream_t)hip_stream, covariance, side[0], side[1], out, n, f.t, f.u);
    return e == hipSuccess ? BGSM_OK : fail_hip(fn, e);
}

}  // namespace

extern "C" {

uint32_t bgsm_version(void) { return ((uint32_t)BGSM_VERSION_MAJOR << 16) | (uint32_t)BGSM_VERSION_MINOR; }

const char* bgsm_last_error(void) { return g_error; }

int bgsm_interpolate_f32(int hip_device, void* hip_stream, uint32_t n, const void* lhs_position_visibility_device_ptr,
                         const void* lhs_spherical_harmonic_device_ptr, const void* lhs_rotation_device_ptr,
                         const void* lhs_scale_opacity_device_ptr, const void* rhs_position_visibility_device_ptr,
                         const void* rhs_spherical_harmonic_device_ptr, const void* rhs_rotation_device_ptr,
                         const void* rhs_scale_opacity_device_ptr, void* out_position_visibility_device_ptr,
                         void* out_spherical_harmonic_device_ptr, void* out_rotation_device_ptr, void* out_scale_opacity_device_ptr,
                         float time, float time_start, float time_stop) {
    const Named planes[12] = {{"lhs_position_visibility_device_ptr", lhs_position_visibility_device_ptr},
                              {"lhs_spherical_harmonic_device_ptr", lhs_spherical_harmonic_device_ptr},
                              {"lhs_rotation_device_ptr", lhs_rotation_device_ptr},
                              {"lhs_scale_opacity_device_ptr", lhs_scale_opacity_device_ptr},
                              {"rhs_position_visibility_device_ptr", rhs_position_visibility_device_ptr},
                              {"rhs_spherical_harmonic_device_ptr", rhs_spherical_harmonic_device_ptr},
                              {"rhs_rotation_device_ptr", rhs_rotation_device_ptr},
                              {"rhs_scale_opacity_device_ptr", rhs_scale_opacity_device_ptr},
                              {"out_position_visibility_device_ptr", out_position_visibility_device_ptr},
                              {"out_spherical_harmonic_device_ptr", out_spherical_harmonic_device_ptr},
                              {"out_rotation_device_ptr", out_rotation_device_ptr},
                              {"out_scale_opacity_device_ptr", out_scale_opacity_device_ptr}};
    return interpolate("bgsm_interpolate_f32", false, hip_device, hip_stream, n, planes, 4, time, time_start, time_stop);
}

int bgsm_interpolate_cov3d_f32(int hip_device, void* hip_stream, uint32_t n, const void* lhs_position_visibility_device_ptr,
                               const void* lhs_spherical_harmonic_device_ptr, const void* lhs_covariance_3d_opacity_device_ptr,
                               const void* rhs_position_visibility_device_ptr, const void* rhs_spherical_harmonic_device_ptr,
                               const void* rhs_covariance_3d_opacity_device_ptr, void* out_position_visibility_device_ptr,
                               void* out_spherical_harmonic_device_ptr, void* out_covariance_3d_opacity_device_ptr, float time,
                               float time_start, float time_stop) {
    const Named planes[9] = {{"lhs_position_visibility_device_ptr", lhs_position_visibility_device_ptr},
                             {"lhs_spherical_harmonic_device_ptr", lhs_spherical_harmonic_device_ptr},
                             {"lhs_covariance_3d_opacity_device_ptr", lhs_covariance_3d_opacity_device_ptr},
                             {"rhs_position_visibility_device_ptr", rhs_position_visibility_device_ptr},
                             {"rhs_spherical_harmonic_device_ptr", rhs_spherical_harmonic_device_ptr},
                             {"rhs_covariance_3d_opacity_device_ptr", rhs_covariance_3d_opacity_device_ptr},
                             {"out_position_visibility_device_ptr", out_position_visibility_device_ptr},
                             {"out_spherical_harmonic_device_ptr", out_spherical_harmonic_device_ptr},
                             {"out_covariance_3d_opacity_device_ptr", out_covariance_3d_opacity_device_ptr}};
    return interpolate("bgsm_interpolate_cov3d_f32", true, hip_device, hip_stream, n, planes, 3, time, time_start, time_stop);
}

}  // extern "C"
