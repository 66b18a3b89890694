// particle_math_shim.cpp — TEST-ONLY host build of the product's particle step arithmetic.
//
// Compiles bevy_gaussian_splatting_amd/csrc/particle_math.h with g++ (same flags as device_math_shim.cpp) so that
// tests/test_particles_host.py can compare the operations the HIP kernel runs with the numpy twin (particles.py
// step_reference) WITHOUT a GPU. The loop around them mirrors particle_step_kernel record for record. Not a product path:
// libbgs never steps a cloud on the host.
#include <stdint.h>
#include <string.h>

#include "../../bevy_gaussian_splatting_amd/csrc/particle_math.h"

extern "C" {

// position_visibility: n x 4 floats; records: count x 64 bytes (indicies | velocity | acceleration | jerk), both in place
void shim_particle_step(float* position_visibility, uint32_t n, uint8_t* records, uint32_t count, float dt) {
    for (uint32_t b = 0; b < count; ++b) {
        uint8_t* rec = records + (size_t)b * 64u;
        int32_t i;
        float v[4], a[4], j[4];
        memcpy(&i, rec, 4);
        memcpy(v, rec + 16, 16);
        memcpy(a, rec + 32, 16);
        memcpy(j, rec + 48, 16);
        if (i < 0 || (uint32_t)i >= n) continue;
        float* p = position_visibility + (size_t)i * 4u;
        for (int k = 0; k < 4; ++k) bgs::particle_step_lane(p[k], v[k], a[k], j[k], dt);
        memcpy(rec + 16, v, 16);
        memcpy(rec + 32, a, 16);
    }
}

uint32_t shim_particle_c6_bits(void) {
    const float c = bgs::PARTICLE_C6;
    uint32_t u;
    memcpy(&u, &c, 4);
    return u;
}

}  // extern "C"
