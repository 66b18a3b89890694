// bgs_slice_api.hip — the C ABI of libbgs_slice.so (include/bgs_slice.h) over the launcher of slice_kernels.hip.
#include <math.h>

#include "../../include/bgs_slice.h"
#include "build_id.inc"
#include "slice_kernels.h"
#include "../small_lib/api_support_hip.h"

// The SHA-256 of the sources this library was compiled from (../_build_id.py libbgs_slice), readable from the
// file's bytes: the loader rebuilds a library that carries another one.
extern "C" __attribute__((used, visibility("hidden"))) const char bgst_build_id_marker[] = "BGST_BUILD_ID=" BGST_BUILD_ID;

static_assert(BGST_EINVAL == API_EINVAL && BGST_ENOMEM == API_ENOMEM && BGST_EHIP == API_EHIP, "the shared support's status codes");

extern "C" {

uint32_t bgst_version(void) { return ((uint32_t)BGST_VERSION_MAJOR << 16) | (uint32_t)BGST_VERSION_MINOR; }

const char* bgst_last_error(void) { return g_error; }

int bgst_slice(int hip_device, void* hip_stream, uint32_t n, const void* position_visibility_device_ptr,
               const void* spherindrical_harmonic_device_ptr, const void* isotropic_rotations_device_ptr,
               const void* scale_opacity_device_ptr, const void* timestamp_timescale_device_ptr,
               void* out_position_visibility_device_ptr, void* out_spherical_harmonic_device_ptr,
               void* out_covariance_3d_opacity_device_ptr, float global_scale, float time, float time_start, float time_stop) {
    g_error[0] = 0;
    const char* const names[4] = {"global_scale", "time", "time_start", "time_stop"};
    const float values[4] = {global_scale, time, time_start, time_stop};
    for (int k = 0; k < 4; ++k)
        if (!isfinite(values[k])) return fail(BGST_EINVAL, "bgst_slice: %s %g must be finite", names[k], (double)values[k]);
    if (time_stop == time_start) return fail(BGST_EINVAL, "bgst_slice: time_stop == time_start (%g): the duration is 0", (double)time_start);
    if (n == 0u) return BGST_OK;
    const Named planes[8] = {{"position_visibility_device_ptr", position_visibility_device_ptr},
                             {"spherindrical_harmonic_device_ptr", spherindrical_harmonic_device_ptr},
                             {"isotropic_rotations_device_ptr", isotropic_rotations_device_ptr},
                             {"scale_opacity_device_ptr", scale_opacity_device_ptr},
                             {"timestamp_timescale_device_ptr", timestamp_timescale_device_ptr},
                             {"out_position_visibility_device_ptr", out_position_visibility_device_ptr},
                             {"out_spherical_harmonic_device_ptr", out_spherical_harmonic_device_ptr},
                             {"out_covariance_3d_opacity_device_ptr", out_covariance_3d_opacity_device_ptr}};
    if (const int refused = check_planes("bgst_slice", planes, 5, 8)) return refused;
    if (const int refused = check_device("bgst_slice", hip_device)) return refused;
    DeviceScope scope(hip_device);
    if (scope.status() != hipSuccess) return fail_hip("hipSetDevice", scope.status());
    const bgst::SlicePlanes p = {(const float4*)position_visibility_device_ptr, (const float4*)spherindrical_harmonic_device_ptr,
                                 (const float4*)isotropic_rotations_device_ptr, (const float4*)scale_opacity_device_ptr,
                                 (const float4*)timestamp_timescale_device_ptr, (float4*)out_position_visibility_device_ptr,
                                 (float4*)out_spherical_harmonic_device_ptr, (float4*)out_covariance_3d_opacity_device_ptr};
    const hipError_t e = bgst::launch_slice((hipStream_t)hip_stream, p, n, global_scale, time, time_stop - time_start);
    return e == hipSuccess ? BGST_OK : fail_hip("bgst_slice", e);
}

}  // extern "C"
