// slice_math_shim.cpp — TEST-ONLY host build of the product's time-slice arithmetic.
//
// Compiles bevy_gaussian_splatting_amd/csrc_slice/slice_math.h with g++ (same flags as sparse_math_shim.cpp) so that
// tests/test_time_slice_host.py can compare the operations the HIP kernels run with the numpy twin (time_slice.py
// slice_reference) WITHOUT a GPU. shim_slice walks the planes as the two kernels of slice_kernels.hip do, one splat after
// the other, with this host's expf and cosf; shim_expf and shim_cosf hand those two to the twin, so that the comparison
// is bit for bit on every lane. Not a product path: libbgs_slice never slices on the host.
#include <stddef.h>
#include <stdint.h>

#include "../../bevy_gaussian_splatting_amd/csrc_slice/slice_math.h"

extern "C" {

void shim_expf(const float* in, uint32_t n, float* out) {
    for (uint32_t i = 0; i < n; ++i) out[i] = bgst::marginal_of(in[i]);
}

void shim_cosf(const float* in, uint32_t n, float* out) {
    for (uint32_t i = 0; i < n; ++i) out[i] = cosf(in[i]);
}

// planes as include/bgs_slice.h lays them out; exponent: n, cosine_arguments: n x 2 (what exp and cos were called with)
void shim_slice(uint32_t n, const float* pv, const float* sh, const float* rot, const float* so, const float* tt, float global_scale,
                float time, float time_start, float time_stop, float* out_pv, float* out_sh, float* out_cov, float* exponent,
                float* cosine_arguments) {
    const float duration = time_stop - time_start;
    for (size_t i = 0; i < n; ++i) {
        const bgst::Conditioned g = bgst::condition(rot + 8 * i, rot + 8 * i + 4, so + 4 * i, tt[4 * i], tt[4 * i + 1], global_scale, time);
        bgst::slice_geometry(pv + 4 * i, g, bgst::marginal_of(g.exponent), so[4 * i + 3], out_pv + 4 * i, out_cov + 8 * i);
        exponent[i] = g.exponent;
        float t1, t2;
        bgst::time_cosines(time - tt[4 * i], duration, &t1, &t2);
        const float theta = (time - tt[4 * i]) / duration;
        cosine_arguments[2 * i] = bgst::TWO_PI * theta;
        cosine_arguments[2 * i + 1] = bgst::FOUR_PI * theta;
        for (uint32_t k = 0; k < bgst::SH_COEFFS; ++k)
            out_sh[48 * i + k] = bgst::fold(sh[144 * i + k], sh[144 * i + 48 + k], sh[144 * i + 96 + k], t1, t2);
    }
}

}  // extern "C"
