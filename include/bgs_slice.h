/* bgs_slice.h — the time slice of a 4D Gaussian cloud on the device: the C ABI of libbgs_slice.so.
 *
 * The reference's second kind of cloud, Gaussian4d (src/gaussian/formats/planar_4d.rs, src/render/gaussian_4d.wgsl,
 * src/material/spherindrical_harmonics.wgsl): at CloudSettings.time a 4D cloud IS a 3D cloud in the precomputed-
 * covariance layout, and this library computes that cloud. Like libbgs_query and libbgs_sparse it is a separate small
 * library. It links the HIP runtime only, not libbgs, and declares nothing of its header. It works on device memory the
 * caller owns, every plane 16-byte aligned, n rows each:
 *   in:   position_visibility      n x 4  floats  (x, y, z, visibility)
 *         spherindrical_harmonic   n x 144 floats (three groups of 48: static, cos(2 pi theta), cos(4 pi theta))
 *         isotropic_rotations      n x 8  floats  (w, x, y, z, wr, xr, yr, zr)
 *         scale_opacity            n x 4  floats  (sx, sy, sz, opacity)
 *         timestamp_timescale      n x 4  floats  (timestamp, time_scale; two lanes unread)
 *   out:  position_visibility      n x 4  floats  (p + delta_mean, visibility)
 *         spherical_harmonic       n x 48 floats  (sh[k] + t1 sh[48 + k]) + t2 sh[96 + k]
 *         covariance_3d_opacity    n x 8  floats  (xx, xy, xz, yy, yz, zz, opacity * marginal, 0)
 * The three outputs are the three planes bgs_cloud_upload_cov3d_f32 takes. A splat whose temporal marginal is not above
 * 0.05 (the shader's mask; a NaN fails it) keeps its position and visibility and gets eight +0: it blends alpha 0.
 * bgs_device_alloc / bgs_upload / bgs_download serve such memory.
 *
 * The arithmetic contract — f32, every operation rounded once, in a stated order; exp and cos through the device's
 * math library — with its two stated deviations from the reference is
 * bevy_gaussian_splatting_amd/csrc_slice/slice_math.h.
 *
 * ORDERING. bgst_slice only ENQUEUES on the stream it is given (two launches): it never blocks and touches no other
 * stream. What it reads must be complete on that stream (or earlier); what it writes is complete once the stream
 * reaches that point. It keeps no state and needs no scratch: there is nothing to create or free, and any number of
 * threads may call it. libbgs's uploads take a plane by device address (include/bgs.h, DEVICE PLANES), so a slice
 * reaches a resident cloud without leaving the device:
 *   1. bgst_slice(.., bgs_stream(ctx), ..): no synchronisation after it
 *   2. bgs_cloud_upload_cov3d_f32(ctx, n, out_position_visibility_device_ptr, out_spherical_harmonic_device_ptr,
 *      out_covariance_3d_opacity_device_ptr, &cloud): it orders itself behind what bgs_stream(ctx) holds, packs the
 *      cloud from the three output planes, and returns once the cloud is complete; the output planes are free for the
 *      next time's slice from then on
 *   3. bgs_sort / bgs_render of that cloud; bgs_cloud_free before the next time's slice replaces it.
 * A host that wants the planes on the host anyway takes the other order: bgs_synchronize(ctx) after step 1, bgs_download
 * of the three output planes, and the same upload from the host copies.
 * Status codes mirror bgs_status. */
#ifndef BGS_SLICE_H
#define BGS_SLICE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BGST_VERSION_MAJOR 0
#define BGST_VERSION_MINOR 1

#define BGST_OK 0
#define BGST_EINVAL (-1) /* bad argument; bgst_last_error() names it */
#define BGST_ENOMEM (-2) /* (unused: nothing is allocated) */
#define BGST_EHIP (-3)   /* a HIP call failed, or no usable device */

/* (major << 16) | minor */
uint32_t bgst_version(void);
/* Message of the calling thread's last failed call; "" if none. Valid until that thread's next call. */
const char* bgst_last_error(void);

/* The slice of the n splats at `time`, as above. hip_device is the device the memory and the stream live on.
 * BGST_EINVAL names the offender: a global_scale, time, time_start or time_stop that is not finite; time_stop ==
 * time_start; with n > 0 a NULL pointer, a pointer that is not 16-byte aligned, or an output that is also an input or
 * another output (the planes must not overlap; only equal addresses are detected). n == 0 enqueues nothing and looks
 * at no pointer. */
int bgst_slice(int hip_device, void* hip_stream, uint32_t n, const void* position_visibility_device_ptr,
               const void* spherindrical_harmonic_device_ptr, const void* isotropic_rotations_device_ptr,
               const void* scale_opacity_device_ptr, const void* timestamp_timescale_device_ptr,
               void* out_position_visibility_device_ptr, void* out_spherical_harmonic_device_ptr,
               void* out_covariance_3d_opacity_device_ptr, float global_scale, float time, float time_start, float time_stop);

#ifdef __cplusplus
}
#endif

#endif /* BGS_SLICE_H */
