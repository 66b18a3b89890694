// bgs_morph.hpp — C++ host side above the C ABI of libbgs_morph.so (include/bgs_morph.h): the morph between two
// Gaussian clouds on the device, the reference's GaussianInterpolate { lhs, rhs } at CloudSettings.time. Header-only,
// C++17, no HIP headers needed: link libbgs_morph.so. It does not need bgs.hpp; with it, a morphed cloud becomes a
// resident cloud through the host:
//
//   bgs::morph::TimeSettings at;  at.time = 0.4f;                    // time_start, time_stop as CloudSettings
//   bgs::morph::interpolate(/*hip_device*/ 0, plugin.stream(), n, lhs, rhs, out, at);
//   plugin.synchronize();                                            // then bgs_download of the four planes of `out`
//   bgs_cloud_upload_f32(ctx, n, position_visibility, spherical_harmonic, rotation, scale_opacity, &cloud);
//
// Every failure of the C ABI becomes a bgs::morph::Error carrying the status and bgsm_last_error().
#ifndef BGS_MORPH_HPP
#define BGS_MORPH_HPP

#include <cstdint>
#include <stdexcept>
#include <string>

#include "bgs_morph.h"

namespace bgs {
namespace morph {

class Error : public std::runtime_error {
  public:
    Error(int status, const std::string& what) : std::runtime_error(what), status_(status) {}
    int status() const { return status_; }

  private:
    int status_;
};

inline void check(int status) {
    if (status != BGSM_OK) throw Error(status, bgsm_last_error());
}

// What a morph reads of the reference's CloudSettings, with its defaults.
struct TimeSettings {
    float time = 0.0f;
    float time_start = 0.0f;
    float time_stop = 1.0f;
};

// Device addresses of one cloud's planes in the f32 layout, n rows each, 16-byte aligned. Pointer is const void* for
// the lhs and the rhs, void* for the output.
template <typename Pointer>
struct PlanesF32 {
    Pointer position_visibility = nullptr;      // n x 4 floats
    Pointer spherical_harmonic = nullptr;       // n x 48
    Pointer rotation = nullptr;                 // n x 4, (w, x, y, z)
    Pointer scale_opacity = nullptr;            // n x 4
};

// The same in the precomputed-covariance layout.
template <typename Pointer>
struct PlanesCov3d {
    Pointer position_visibility = nullptr;      // n x 4 floats
    Pointer spherical_harmonic = nullptr;       // n x 48
    Pointer covariance_3d_opacity = nullptr;    // n x 8
};

// Enqueues the blend on hip_stream (include/bgs_morph.h "ORDERING"); it never blocks.
inline void interpolate(int hip_device, void* hip_stream, uint32_t n, const PlanesF32<const void*>& lhs, const PlanesF32<const void*>& rhs,
                        const PlanesF32<void*>& out, const TimeSettings& at) {
    check(bgsm_interpolate_f32(hip_device, hip_stream, n, lhs.position_visibility, lhs.spherical_harmonic, lhs.rotation, lhs.scale_opacity,
                               rhs.position_visibility, rhs.spherical_harmonic, rhs.rotation, rhs.scale_opacity, out.position_visibility,
                               out.spherical_harmonic, out.rotation, out.scale_opacity, at.time, at.time_start, at.time_stop));
}

inline void interpolate(int hip_device, void* hip_stream, uint32_t n, const PlanesCov3d<const void*>& lhs, const PlanesCov3d<const void*>& rhs,
                        const PlanesCov3d<void*>& out, const TimeSettings& at) {
    check(bgsm_interpolate_cov3d_f32(hip_device, hip_stream, n, lhs.position_visibility, lhs.spherical_harmonic, lhs.covariance_3d_opacity,
                                     rhs.position_visibility, rhs.spherical_harmonic, rhs.covariance_3d_opacity, out.position_visibility,
                                     out.spherical_harmonic, out.covariance_3d_opacity, at.time, at.time_start, at.time_stop));
}

}  // namespace morph
}  // namespace bgs

#endif  // BGS_MORPH_HPP
