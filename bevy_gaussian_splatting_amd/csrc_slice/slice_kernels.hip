// slice_kernels.hip — the time slice of a 4D Gaussian cloud on the device, by the arithmetic of slice_math.h. gfx950, wave64.
//
// The stage moves bytes: 656 read and 240 written a splat, 576 + 192 of them spherindrical coefficients. Two launches on
// one stream, neither waiting for the other or for another workgroup:
//   1. geometry: one splat a lane. Five 16-byte loads (position, the rotation pair, scale, timestamp), the conditional
//      covariance, one exp, three 16-byte stores.
//   2. fold:     one float4 of OUTPUT a lane over n x 12. A workgroup of 192 lanes takes 16 splats: its stores are 3 KiB in
//      a row, 16 bytes a lane, and its three loads a lane cover 9 KiB in a row between them, every 128-byte line of it used
//      whole by the wave that touches it. The twelve lanes of a splat each read its timestamp (one line, from the cache)
//      and take the two cosines themselves: there is no scratch to pass them through, and the arithmetic hides under
//      the loads.
// Two launches and not one because the two shapes share nothing but the timestamp: one splat a lane against twelve
// lanes a splat. Folded into one grid, either eleven of twelve lanes idle through the geometry or a workgroup's role
// depends on its number; what is saved is one launch (DESIGN.md section 8 has the measured time of both).
#include "slice_kernels.h"

namespace bgst {

__global__ __launch_bounds__(GEOMETRY_THREADS) void slice_geometry_kernel(SlicePlanes p, uint32_t n, float global_scale, float time) {
    const uint64_t i = (uint64_t)blockIdx.x * GEOMETRY_THREADS + threadIdx.x;
    if (i >= n) return;
    const float4 pv = p.position_visibility[i];
    const float4 q = p.isotropic_rotations[2u * i], qr = p.isotropic_rotations[2u * i + 1u];
    const float4 so = p.scale_opacity[i];
    const float4 tt = p.timestamp_timescale[i];
    const float rot[4] = {q.x, q.y, q.z, q.w}, rot_r[4] = {qr.x, qr.y, qr.z, qr.w}, scale[3] = {so.x, so.y, so.z};
    const Conditioned g = condition(rot, rot_r, scale, tt.x, tt.y, global_scale, time);
    const float in[4] = {pv.x, pv.y, pv.z, pv.w};
    float out[4], cov[8];
    slice_geometry(in, g, marginal_of(g.exponent), so.w, out, cov);
    p.out_position_visibility[i] = make_float4(out[0], out[1], out[2], out[3]);
    p.out_covariance_3d_opacity[2u * i] = make_float4(cov[0], cov[1], cov[2], cov[3]);
    p.out_covariance_3d_opacity[2u * i + 1u] = make_float4(cov[4], cov[5], cov[6], cov[7]);
}

// Lane (s, k) of a workgroup: splat blockIdx.x * 16 + s, float4 k of its 12. The output index is blockIdx.x * 192 +
// threadIdx.x: consecutive lanes, consecutive 16 bytes.
__global__ __launch_bounds__(FOLD_THREADS) void slice_fold_kernel(const float4* __restrict__ sh, const float4* __restrict__ timestamp_timescale,
                                                                   uint32_t n, float time, float duration, float4* __restrict__ out) {
    const uint32_t s = threadIdx.x / FOLD_QUADS, k = threadIdx.x - s * FOLD_QUADS;
    const uint64_t i = (uint64_t)blockIdx.x * FOLD_SPLATS + s;
    if (i >= n) return;
    const float4* row = sh + i * (3u * FOLD_QUADS) + k;
    const float4 a = row[0], b = row[FOLD_QUADS], c = row[2u * FOLD_QUADS];
    float t1, t2;
    time_cosines(time - timestamp_timescale[i].x, duration, &t1, &t2);
    out[i * FOLD_QUADS + k] = make_float4(fold(a.x, b.x, c.x, t1, t2), fold(a.y, b.y, c.y, t1, t2), fold(a.z, b.z, c.z, t1, t2),
                                          fold(a.w, b.w, c.w, t1, t2));
}

hipError_t launch_slice(hipStream_t stream, const SlicePlanes& planes, uint32_t n, float global_scale, float time, float duration) {
    if (n == 0u) return hipSuccess;
    const uint32_t geometry_blocks = (uint32_t)(((uint64_t)n + GEOMETRY_THREADS - 1u) / GEOMETRY_THREADS);
    const uint32_t fold_blocks = (uint32_t)(((uint64_t)n + FOLD_SPLATS - 1u) / FOLD_SPLATS);
    hipLaunchKernelGGL(slice_geometry_kernel, dim3(geometry_blocks), dim3(GEOMETRY_THREADS), 0, stream, planes, n, global_scale, time);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(slice_fold_kernel, dim3(fold_blocks), dim3(FOLD_THREADS), 0, stream, planes.spherindrical_harmonic,
                       planes.timestamp_timescale, n, time, duration, planes.out_spherical_harmonic);
    return hipGetLastError();
}

}  // namespace bgst
