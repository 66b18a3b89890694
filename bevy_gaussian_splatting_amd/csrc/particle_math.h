// particle_math.h — one step of a particle behaviour (src/morph/particle.wgsl:36-42), shared by the device kernel
// (particle_kernels.hip) and a g++ build (tests/host_shim/particle_math_shim.cpp), like splat_math.h.
//
// ARITHMETIC CONTRACT: f32, every operation rounded once (the library and the shim build with -ffp-contract=off), in the
// shader's written left-to-right order:
//   dp = ((v*dt) + (((0.5*a)*dt)*dt)) + ((((c6*j)*dt)*dt)*dt)      c6 = (float)(1.0 / 6.0) = 0x3E2AAAAB
//   dv = (a*dt) + (((0.5*j)*dt)*dt)
//   da = j*dt
// No dt*dt or 0.5*dt*dt is formed first: that rounds differently, and the numpy twin
// (bevy_gaussian_splatting_amd/particles.py step_reference) is compared bit for bit.
#pragma once

#if defined(__HIPCC__)
#define BGS_PARTICLE_HD __host__ __device__ __forceinline__
#else
#define BGS_PARTICLE_HD static inline
#endif

namespace bgs {

constexpr float PARTICLE_C6 = (float)(1.0 / 6.0);

BGS_PARTICLE_HD float particle_delta_position(float v, float a, float j, float dt) {
    return ((v * dt) + (((0.5f * a) * dt) * dt)) + ((((PARTICLE_C6 * j) * dt) * dt) * dt);
}
BGS_PARTICLE_HD float particle_delta_velocity(float a, float j, float dt) { return (a * dt) + (((0.5f * j) * dt) * dt); }
BGS_PARTICLE_HD float particle_delta_acceleration(float j, float dt) { return j * dt; }

// One lane of one record: p, v, a in place.
BGS_PARTICLE_HD void particle_step_lane(float& p, float& v, float& a, float j, float dt) {
    const float dp = particle_delta_position(v, a, j, dt);
    const float dv = particle_delta_velocity(a, j, dt);
    const float da = particle_delta_acceleration(j, dt);
    p = p + dp;
    v = v + dv;
    a = a + da;
}

}  // namespace bgs
