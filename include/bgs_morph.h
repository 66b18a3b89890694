/* bgs_morph.h — the morph between two Gaussian clouds on the device: the C ABI of libbgs_morph.so.
 *
 * The reference's GaussianInterpolate { lhs, rhs } (src/morph/interpolate.rs, src/morph/interpolate.wgsl
 * interpolate_gaussians): the output cloud is the per-splat linear blend of two clouds of equal length at
 * CloudSettings.time between time_start and time_stop. Like the other small libraries it stands alone. It links the HIP
 * runtime only, not libbgs, and declares nothing of its header. It works on device memory the caller owns, every plane
 * 16-byte aligned, n rows each, the same planes on the lhs, on the rhs and in the output:
 *   f32 layout (what bgs_cloud_upload_f32 takes):
 *         position_visibility      n x 4  floats  (x, y, z, visibility)       all four lanes blended
 *         spherical_harmonic       n x 48 floats                              every lane blended
 *         rotation                 n x 4  floats  (w, x, y, z)                blended, then normalised
 *         scale_opacity            n x 4  floats  (sx, sy, sz, opacity)       all four lanes blended
 *   precomputed-covariance layout (what bgs_cloud_upload_cov3d_f32 takes):
 *         position_visibility, spherical_harmonic as above
 *         covariance_3d_opacity    n x 8  floats  (xx, xy, xz, yy, yz, zz, opacity, pad)   lanes 0..6 blended, the pad +0
 * The blend is a * (1 - t) + b * t with the factor t = clamp((time - time_start) / (time_stop - time_start), 0, 1), or
 * the step (time >= time_stop) where |time_stop - time_start| < 1e-6; a reversed interval runs backwards. A blended
 * rotation of length 0 becomes the stored lanes (0, 0, 0, 1). bgs_device_alloc / bgs_upload / bgs_download serve such
 * memory.
 *
 * The arithmetic contract — f32, every operation rounded once, in a stated order, the square root and the divisions
 * correctly rounded, so that the result is the same bits on the device, in a host build and in the numpy twin — with
 * its stated deviation from the reference is bevy_gaussian_splatting_amd/csrc_morph/morph_math.h.
 *
 * ORDERING. Both entry points only ENQUEUE on the stream they are given (two launches): they never block and touch no
 * other stream. What they read must be complete on that stream (or earlier); what they write is complete once the
 * stream reaches that point. They keep no state and need no scratch: there is nothing to create or free, and any
 * number of threads may call them. libbgs's uploads take a plane by device address (include/bgs.h, DEVICE PLANES), so
 * a morphed cloud reaches a resident cloud without leaving the device:
 *   1. bgsm_interpolate_f32(.., bgs_stream(ctx), ..) or bgsm_interpolate_cov3d_f32: no synchronisation after it
 *   2. bgs_cloud_upload_f32(ctx, n, position_visibility, spherical_harmonic, rotation, scale_opacity, &cloud), or
 *      bgs_cloud_upload_cov3d_f32(ctx, n, position_visibility, spherical_harmonic, covariance_3d_opacity, &cloud), with
 *      the OUTPUT's device addresses: it orders itself behind what bgs_stream(ctx) holds, packs the cloud from the
 *      output planes, and returns once the cloud is complete; the output planes are free for the next time's morph from
 *      then on
 *   3. bgs_sort / bgs_render of that cloud; bgs_cloud_free before the next time's morph replaces it.
 * A host that wants the planes on the host anyway takes the other order: bgs_synchronize(ctx) after step 1, bgs_download
 * of the output planes, and the same upload from the host copies.
 * The lhs and rhs planes stay where they are: a host that scrubs `time` uploads each side once.
 * Status codes mirror bgs_status. */
#ifndef BGS_MORPH_H
#define BGS_MORPH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BGSM_VERSION_MAJOR 0
#define BGSM_VERSION_MINOR 1

#define BGSM_OK 0
#define BGSM_EINVAL (-1) /* bad argument; bgsm_last_error() names it */
#define BGSM_ENOMEM (-2) /* (unused: nothing is allocated) */
#define BGSM_EHIP (-3)   /* a HIP call failed, or no usable device */

/* (major << 16) | minor */
uint32_t bgsm_version(void);
/* Message of the calling thread's last failed call; "" if none. Valid until that thread's next call. */
const char* bgsm_last_error(void);

/* The blend of the n splats of two clouds in the f32 layout at `time`, as above. hip_device is the device the memory
 * and the stream live on. BGSM_EINVAL names the offender: a time, time_start or time_stop that is not finite; with
 * n > 0 a NULL pointer, a pointer that is not 16-byte aligned, or an output that is also an input or another output
 * (the planes must not overlap; only equal addresses are detected). time_stop == time_start is no error: it is the
 * shader's step. An input may be given on both sides, for a cloud morphed with itself. n == 0 enqueues nothing and
 * looks at no pointer. */
int bgsm_interpolate_f32(int hip_device, void* hip_stream, uint32_t n, const void* lhs_position_visibility_device_ptr,
                         const void* lhs_spherical_harmonic_device_ptr, const void* lhs_rotation_device_ptr,
                         const void* lhs_scale_opacity_device_ptr, const void* rhs_position_visibility_device_ptr,
                         const void* rhs_spherical_harmonic_device_ptr, const void* rhs_rotation_device_ptr,
                         const void* rhs_scale_opacity_device_ptr, void* out_position_visibility_device_ptr,
                         void* out_spherical_harmonic_device_ptr, void* out_rotation_device_ptr, void* out_scale_opacity_device_ptr,
                         float time, float time_start, float time_stop);

/* The same for two clouds in the precomputed-covariance layout: three planes a side. */
int bgsm_interpolate_cov3d_f32(int hip_device, void* hip_stream, uint32_t n, const void* lhs_position_visibility_device_ptr,
                               const void* lhs_spherical_harmonic_device_ptr, const void* lhs_covariance_3d_opacity_device_ptr,
                               const void* rhs_position_visibility_device_ptr, const void* rhs_spherical_harmonic_device_ptr,
                               const void* rhs_covariance_3d_opacity_device_ptr, void* out_position_visibility_device_ptr,
                               void* out_spherical_harmonic_device_ptr, void* out_covariance_3d_opacity_device_ptr, float time,
                               float time_start, float time_stop);

#ifdef __cplusplus
}
#endif

#endif /* BGS_MORPH_H */
