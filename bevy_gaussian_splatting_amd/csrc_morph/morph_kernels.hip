// morph_kernels.hip — the linear blend of two Gaussian clouds on the device, by the arithmetic of morph_math.h. gfx950, wave64.
//
// The stage moves bytes: 480 read and 240 written a splat in either layout, 384 + 192 of them coefficients, against two
// products and a sum a float. Every access is a 16-byte load or store; nothing uses LDS, scratch, atomics or waits for
// another workgroup. Two launches on one stream, neither waiting for the other:
//   1. geometry: one splat a lane. f32 layout: three 16-byte loads a side (position, rotation, scale/opacity), the mix,
//      the rotation's normalisation (one sqrt, four divisions), three stores. Covariance layout: position and the two
//      float4 of the covariance plane a side, the mix with the pad lane forced to +0, three stores. The variant is a
//      template parameter.
//   2. colour:   one float4 of OUTPUT a lane over the n x 12 rows of the colour plane: two loads, four mix, one store.
//      Consecutive lanes take consecutive rows, so a wave reads 1 KiB in a row from each side and writes 1 KiB in a row.
//      Row indices are 64 bit: the byte offsets pass 2^32 at 22 M splats.
// Two launches and not one for the time slice's reason: the two shapes share nothing but the factor, one splat a lane
// against twelve lanes a splat. Folded into one grid, either eleven of twelve lanes idle through the geometry or a
// workgroup's role depends on its number; what is saved is one launch (DESIGN.md section 8 has the measured time of both).
#include "morph_kernels.h"

namespace bgsm {

__device__ __forceinline__ float4 mix_quad(const float4 a, const float4 b, float t, float u) {
    return make_float4(mix(a.x, b.x, t, u), mix(a.y, b.y, t, u), mix(a.z, b.z, t, u), mix(a.w, b.w, t, u));
}

template <bool COVARIANCE>
__global__ __launch_bounds__(GEOMETRY_THREADS) void morph_geometry_kernel(MorphSide lhs, MorphSide rhs, MorphOut out, uint32_t n, float t, float u) {
    const uint64_t i = (uint64_t)blockIdx.x * GEOMETRY_THREADS + threadIdx.x;
    if (i >= n) return;
    const float4 pa = lhs.position_visibility[i], pb = rhs.position_visibility[i];
    if (COVARIANCE) {
        const float4 a0 = lhs.covariance_3d_opacity[2u * i], a1 = lhs.covariance_3d_opacity[2u * i + 1u];
        const float4 b0 = rhs.covariance_3d_opacity[2u * i], b1 = rhs.covariance_3d_opacity[2u * i + 1u];
        const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w}, b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
        float cov[8];
        mix_covariance(a, b, t, u, cov);
        out.position_visibility[i] = mix_quad(pa, pb, t, u);
        out.covariance_3d_opacity[2u * i] = make_float4(cov[0], cov[1], cov[2], cov[3]);
        out.covariance_3d_opacity[2u * i + 1u] = make_float4(cov[4], cov[5], cov[6], cov[7]);
    } else {
        const float4 ra = lhs.rotation[i], rb = rhs.rotation[i];
        const float4 sa = lhs.scale_opacity[i], sb = rhs.scale_opacity[i];
        const float a[4] = {ra.x, ra.y, ra.z, ra.w}, b[4] = {rb.x, rb.y, rb.z, rb.w};
        float q[4];
        mix_rotation(a, b, t, u, q);
        out.position_visibility[i] = mix_quad(pa, pb, t, u);
        out.rotation[i] = make_float4(q[0], q[1], q[2], q[3]);
        out.scale_opacity[i] = mix_quad(sa, sb, t, u);
    }
}

// rows = n x 12. The planes never alias an output (the C ABI refuses it), hence __restrict__; lhs may be rhs.
__global__ __launch_bounds__(COLOUR_THREADS) void morph_colour_kernel(const float4* lhs, const float4* rhs, float4* __restrict__ out, uint64_t rows,
                                                                       float t, float u) {
    const uint64_t row = (uint64_t)blockIdx.x * COLOUR_THREADS + threadIdx.x;
    if (row >= rows) return;
    out[row] = mix_quad(lhs[row], rhs[row], t, u);
}

hipError_t launch_morph(hipStream_t stream, bool covariance, const MorphSide& lhs, const MorphSide& rhs, const MorphOut& out, uint32_t n,
                        float t, float u) {
    if (n == 0u) return hipSuccess;
    const uint32_t geometry_blocks = (uint32_t)(((uint64_t)n + GEOMETRY_THREADS - 1u) / GEOMETRY_THREADS);
    const uint64_t rows = (uint64_t)n * COLOUR_QUADS;
    const uint32_t colour_blocks = (uint32_t)((rows + COLOUR_THREADS - 1u) / COLOUR_THREADS);      // under 2^28 for every uint32_t n
    if (covariance)
        hipLaunchKernelGGL(morph_geometry_kernel<true>, dim3(geometry_blocks), dim3(GEOMETRY_THREADS), 0, stream, lhs, rhs, out, n, t, u);
    else
        hipLaunchKernelGGL(morph_geometry_kernel<false>, dim3(geometry_blocks), dim3(GEOMETRY_THREADS), 0, stream, lhs, rhs, out, n, t, u);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(morph_colour_kernel, dim3(colour_blocks), dim3(COLOUR_THREADS), 0, stream, lhs.spherical_harmonic, rhs.spherical_harmonic,
                       out.spherical_harmonic, rows, t, u);
    return hipGetLastError();
}

}  // namespace bgsm
