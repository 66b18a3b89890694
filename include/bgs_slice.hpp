// bgs_slice.hpp — C++ host side above the C ABI of libbgs_slice.so (include/bgs_slice.h): the time slice of a 4D
// Gaussian cloud on the device, the reference's Gaussian4d at CloudSettings.time. Header-only, C++17, no HIP headers
// needed: link libbgs_slice.so. It does not need bgs.hpp; with it, a slice becomes a resident cloud through the host:
//
//   bgs::slice::TimeSettings at;  at.time = 0.4f;                    // global_scale, time_start, time_stop as CloudSettings
//   bgs::slice::slice(/*hip_device*/ 0, plugin.stream(), n, in, out, at);
//   plugin.synchronize();                                            // then bgs_download of the three planes of `out`
//   bgs_cloud_upload_cov3d_f32(ctx, n, position_visibility, spherical_harmonic, covariance_3d_opacity, &cloud);
//
// Every failure of the C ABI becomes a bgs::slice::Error carrying the status and bgst_last_error().
#ifndef BGS_SLICE_HPP
#define BGS_SLICE_HPP

#include <cstdint>
#include <stdexcept>
#include <string>

#include "bgs_slice.h"

namespace bgs {
namespace slice {

class Error : public std::runtime_error {
  public:
    Error(int status, const std::string& what) : std::runtime_error(what), status_(status) {}
    int status() const { return status_; }

  private:
    int status_;
};

inline void check(int status) {
    if (status != BGST_OK) throw Error(status, bgst_last_error());
}

// What a slice reads of the reference's CloudSettings, with its defaults.
struct TimeSettings {
    float global_scale = 1.0f;
    float time = 0.0f;
    float time_start = 0.0f;
    float time_stop = 1.0f;
};

// Device addresses of the five planes of a 4D cloud (PlanarGaussian4d), n rows each, 16-byte aligned.
struct Planes4d {
    const void* position_visibility = nullptr;      // n x 4 floats
    const void* spherindrical_harmonic = nullptr;   // n x 144
    const void* isotropic_rotations = nullptr;      // n x 8
    const void* scale_opacity = nullptr;            // n x 4
    const void* timestamp_timescale = nullptr;      // n x 4
};

// Device addresses of the three planes of the slice: what bgs_cloud_upload_cov3d_f32 takes once they are on the host.
struct Planes3d {
    void* position_visibility = nullptr;            // n x 4 floats
    void* spherical_harmonic = nullptr;             // n x 48
    void* covariance_3d_opacity = nullptr;          // n x 8
};

// Enqueues the slice on hip_stream (include/bgs_slice.h "ORDERING"); it never blocks.
inline void slice(int hip_device, void* hip_stream, uint32_t n, const Planes4d& in, const Planes3d& out, const TimeSettings& at) {
    check(bgst_slice(hip_device, hip_stream, n, in.position_visibility, in.spherindrical_harmonic, in.isotropic_rotations,
                     in.scale_opacity, in.timestamp_timescale, out.position_visibility, out.spherical_harmonic,
                     out.covariance_3d_opacity, at.global_scale, at.time, at.time_start, at.time_stop));
}

}  // namespace slice
}  // namespace bgs

#endif  // BGS_SLICE_HPP
