// particle_kernels.hip — particle behaviours (src/morph/particle.rs, src/morph/particle.wgsl): one step of per-splat
// velocity / acceleration / jerk integrated into the positions of a resident cloud.
#include "kernels.h"
#include "particle_math.h"

namespace bgs {

// One thread per behaviour record (64 bytes: indicies | velocity | acceleration | jerk). The position of a splat lives
// twice on the device (CloudPtrs): in the position_visibility plane keygen streams and in word 0 of the splat's packed
// record the vertex stage gathers. Both are written from the same registers, so the sort and the projection of every
// later frame agree. A record whose index is negative (as i32) or >= n returns before any store: its velocity and
// acceleration stay as they are. Indices of active records are distinct (bgs.h), so no two threads touch one splat.
// Plain 16-byte vector loads and stores only; nothing waits on anything.
__global__ __launch_bounds__(256) void particle_step_kernel(float4* behaviors, uint32_t count, float4* position_visibility,
                                                             float4* packed, uint32_t packed_v4, uint32_t n, float dt) {
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= count) return;
    float4* rec = behaviors + b * 4u;
    const int4 indicies = *reinterpret_cast<const int4*>(rec);
    float4 v = rec[1], a = rec[2];
    const float4 j = rec[3];
    const int32_t i = indicies.x;
    if (i < 0 || (uint32_t)i >= n) return;
    float4 p = position_visibility[i];
    particle_step_lane(p.x, v.x, a.x, j.x, dt);
    particle_step_lane(p.y, v.y, a.y, j.y, dt);
    particle_step_lane(p.z, v.z, a.z, j.z, dt);
    particle_step_lane(p.w, v.w, a.w, j.w, dt);   // visibility moves too, as in the reference
    position_visibility[i] = p;
    packed[(size_t)i * packed_v4] = p;
    rec[1] = v;
    rec[2] = a;
}

void launch_particle_step(hipStream_t stream, void* behaviors, uint32_t count, const CloudPtrs& cloud, float dt) {
    if (count == 0 || cloud.n == 0) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)count + 255u) / 256u);
    hipLaunchKernelGGL(particle_step_kernel, dim3(blocks), dim3(256), 0, stream, (float4*)behaviors, count,
                       const_cast<float4*>(cloud.position_visibility),
                       reinterpret_cast<float4*>(const_cast<uint4*>(cloud.packed)), cloud.packed_v4, cloud.n, dt);
}

}  // namespace bgs
