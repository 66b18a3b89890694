// morph_math_shim.cpp — TEST-ONLY host build of the product's morph arithmetic.
//
// Compiles bevy_gaussian_splatting_amd/csrc_morph/morph_math.h with g++ (same flags as slice_math_shim.cpp) so that
// tests/test_interpolate_host.py can compare the operations the HIP kernels run with the numpy twin (interpolate.py
// interpolate_reference) WITHOUT a GPU. The two functions walk the planes as the two kernels of morph_kernels.hip do, one
// splat after the other, with the factor taken once by the header's own function, as the C ABI takes it. Not a product
// path: libbgs_morph never blends on the host. tests/cpp/morph_math_tool.cpp includes this file under a main of its own.
#include <stddef.h>
#include <stdint.h>

#include "../../bevy_gaussian_splatting_amd/csrc_morph/morph_math.h"

extern "C" {

void shim_factor(float time, float time_start, float time_stop, float* t, float* u) {
    const bgsm::Factor f = bgsm::interpolation_factor(time, time_start, time_stop);
    *t = f.t;
    *u = f.u;
}

static void shim_mix_plane(size_t floats, const float* a, const float* b, bgsm::Factor f, float* out) {
    for (size_t k = 0; k < floats; ++k) out[k] = bgsm::mix(a[k], b[k], f.t, f.u);
}

// planes as include/bgs_morph.h lays them out: pv n x 4, sh n x 48, rot n x 4, so n x 4
void shim_interpolate_f32(uint32_t n, const float* l_pv, const float* l_sh, const float* l_rot, const float* l_so, const float* r_pv,
                          const float* r_sh, const float* r_rot, const float* r_so, float time, float time_start, float time_stop,
                          float* o_pv, float* o_sh, float* o_rot, float* o_so) {
    const bgsm::Factor f = bgsm::interpolation_factor(time, time_start, time_stop);
    shim_mix_plane((size_t)n * 4, l_pv, r_pv, f, o_pv);
    shim_mix_plane((size_t)n * 4, l_so, r_so, f, o_so);
    shim_mix_plane((size_t)n * bgsm::SH_COEFFS, l_sh, r_sh, f, o_sh);
    for (size_t i = 0; i < n; ++i) bgsm::mix_rotation(l_rot + 4 * i, r_rot + 4 * i, f.t, f.u, o_rot + 4 * i);
}

// pv n x 4, sh n x 48, cov n x 8
void shim_interpolate_cov3d_f32(uint32_t n, const float* l_pv, const float* l_sh, const float* l_cov, const float* r_pv, const float* r_sh,
                                const float* r_cov, float time, float time_start, float time_stop, float* o_pv, float* o_sh, float* o_cov) {
    const bgsm::Factor f = bgsm::interpolation_factor(time, time_start, time_stop);
    shim_mix_plane((size_t)n * 4, l_pv, r_pv, f, o_pv);
    shim_mix_plane((size_t)n * bgsm::SH_COEFFS, l_sh, r_sh, f, o_sh);
    for (size_t i = 0; i < n; ++i) bgsm::mix_covariance(l_cov + 8 * i, r_cov + 8 * i, f.t, f.u, o_cov + 8 * i);
}

}  // extern "C"
