// bounds_kernels.hip — the box of a resident cloud taken on the device (BGS_BOUNDS_CLOUD, include/bgs.h): one pass over
// the position plane the cloud keeps (f32 in every cloud format), CommonCloud::compute_aabb's fold. The arithmetic, and why
// raw coordinates may be reduced with the offset applied once by the host, is bounds_math.h.
#include "kernels.h"
#include "bounds_math.h"

namespace bgs {

// 256-thread workgroups, grid-stride over the splats (bounds_grid: at most two workgroups per CU), one 16-byte load per
// splat and lane, BOUNDS_UNROLL of them in flight per lane. A lane keeps six running values, NaN coordinates skipped
// (bounds_fold_*); the w lane is loaded with the rest and not looked at. Then the wave's 64 lanes fold across lanes, the
// four waves through 96 bytes of LDS, and ONE lane of the workgroup merges into the six device words with integer
// atomicMin / atomicMax on the order-preserving key. The words were preset on the stream ahead of the launch
// (launch_cloud_bounds). No workgroup waits on another, no float atomics, no scratch; every index is < n.
constexpr uint32_t BOUNDS_UNROLL = 8u;

__device__ __forceinline__ void bounds_fold_splat(float (&lo)[3], float (&hi)[3], const float4& p) {
    asm volatile("" ::"v"(p.w));   // keeps the splat's load one whole 16-byte global_load_dwordx4 (else the compiler trims it to 12)
    lo[0] = bounds_fold_min(lo[0], p.x); hi[0] = bounds_fold_max(hi[0], p.x);
    lo[1] = bounds_fold_min(lo[1], p.y); hi[1] = bounds_fold_max(hi[1], p.y);
    lo[2] = bounds_fold_min(lo[2], p.z); hi[2] = bounds_fold_max(hi[2], p.z);
}

__global__ __launch_bounds__(BOUNDS_THREADS) void cloud_bounds_kernel(const float4* __restrict__ position_visibility, uint32_t n,
                                                                      uint32_t* __restrict__ words) {
    __shared__ float part[BOUNDS_THREADS / 64u][BOUNDS_WORDS];   // 96 bytes
    const float inf = __builtin_inff();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    const uint64_t stride = (uint64_t)gridDim.x * BOUNDS_THREADS;
    uint64_t i = (uint64_t)blockIdx.x * BOUNDS_THREADS + threadIdx.x;
    for (; i + (BOUNDS_UNROLL - 1u) * stride < n; i += BOUNDS_UNROLL * stride) {
        float4 p[BOUNDS_UNROLL];
#pragma unroll
        for (uint32_t k = 0; k < BOUNDS_UNROLL; ++k) p[k] = position_visibility[i + k * stride];
#pragma unroll
        for (uint32_t k = 0; k < BOUNDS_UNROLL; ++k) bounds_fold_splat(lo, hi, p[k]);
    }
    for (; i < n; i += stride) bounds_fold_splat(lo, hi, position_visibility[i]);

    // the wave: every lane ends with the fold of all 64 (the operands are never NaN)
#pragma unroll
    for (int a = 0; a < 3; ++a)
        for (int off = 32; off > 0; off >>= 1) {
            lo[a] = bounds_fold_min(lo[a], __shfl_xor(lo[a], off, 64));
            hi[a] = bounds_fold_max(hi[a], __shfl_xor(hi[a], off, 64));
        }
    const uint32_t wave = threadIdx.x / 64u;
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            part[wave][a] = lo[a];
            part[wave][3 + a] = hi[a];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float l = part[0][a], h = part[0][3 + a];
            for (uint32_t w = 1; w < BOUNDS_THREADS / 64u; ++w) {
                l = bounds_fold_min(l, part[w][a]);
                h = bounds_fold_max(h, part[w][3 + a]);
            }
            atomicMin(&words[a], bounds_key(__float_as_uint(l)));
            atomicMax(&words[3 + a], bounds_key(__float_as_uint(h)));
        }
    }
}

hipError_t launch_cloud_bounds(hipStream_t stream, const float4* position_visibility, uint32_t n, uint32_t* words,
                               uint32_t compute_units, uint32_t grid_cap) {
    if (n == 0u) return hipSuccess;
    hipError_t e = hipMemsetAsync(words, 0xFF, 3u * sizeof(uint32_t), stream);                 // BOUNDS_MIN_PRESET
    if (e == hipSuccess) e = hipMemsetAsync(words + 3, 0, 3u * sizeof(uint32_t), stream);      // BOUNDS_MAX_PRESET
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cloud_bounds_kernel, dim3(bounds_grid(n, compute_units, grid_cap)), dim3(BOUNDS_THREADS), 0, stream,
                       position_visibility, n, words);
    return hipGetLastError();
}

}  // namespace bgs
