// slice_math.h — the time slice of a 4D Gaussian cloud (src/render/gaussian_4d.wgsl conditional_cov3d,
// src/render/gaussian.wgsl:261-290, src/material/spherindrical_harmonics.wgsl:74-122): at time t a Gaussian4d is a
// Gaussian3d in the precomputed-covariance layout. Shared by the device kernels (slice_kernels.hip) and a g++ build
// (tests/host_shim/slice_math_shim.cpp), like csrc_sparse/sparse_math.h. Written from the WGSL as new code.
//
// ARITHMETIC CONTRACT: f32 throughout, every operation rounded once (both builds use -ffp-contract=off), in this order.
// For a splat with position p, rotations q = (w, x, y, z) and q_r = (wr, xr, yr, zr), scale (sx, sy, sz), opacity,
// timestamp and time_scale, and the settings global_scale g, time t, time_start, time_stop:
//
//   dt       = t - timestamp
//   S        = (g*sx, g*sy, g*sz, time_scale)
//   M_l, M_r = the WGSL's mat4x4 constructors, which take COLUMNS: as matrices (row, column)
//                M_l = [ w  x  y  z ;  -x  w  z -y ;  -y -z  w  x ;  -z  y -x  w ]
//                M_r = [ wr xr yr zr; -xr wr -zr yr; -yr zr wr -xr; -zr -yr xr wr ]
//   R(r, c)  = ((M_r(r,0)*M_l(0,c) + M_r(r,1)*M_l(1,c)) + M_r(r,2)*M_l(2,c)) + M_r(r,3)*M_l(3,c)        R = M_r * M_l
//   M(r, c)  = R(r, c) * S[c]                                                                            M = R * S
//   Sg(i, j) = ((M(0,i)*M(0,j) + M(1,i)*M(1,j)) + M(2,i)*M(2,j)) + M(3,i)*M(3,j)                         Sigma = M^T * M
//   cov_t    = Sg(3, 3),   cov12 = (Sg(0,3), Sg(1,3), Sg(2,3))
//   exponent = ((-0.5*dt)*dt) / cov_t
//   marginal = exp(exponent)                              (the one lane of the geometry that goes through a math library)
//   mask     = marginal > 0.05                            (a NaN fails)
//   unmasked:  cov3d  = (Sg(0,0) - (c0*c0)/cov_t, Sg(0,1) - (c0*c1)/cov_t, Sg(0,2) - (c0*c2)/cov_t,
//                        Sg(1,1) - (c1*c1)/cov_t, Sg(1,2) - (c1*c2)/cov_t, Sg(2,2) - (c2*c2)/cov_t)      c = cov12
//              delta  = (c / cov_t) * dt
//              position_visibility      = (p + delta, visibility)
//              covariance_3d_opacity    = (cov3d, opacity * marginal, 0)
//   masked:    position_visibility      = (p, visibility), copied
//              covariance_3d_opacity    = eight +0: such a splat blends alpha 0 wherever it lands
//
//   colour, for k in [0, 48):   out[k] = (sh[k] + t1*sh[48 + k]) + t2*sh[96 + k]
//              theta = dt / (time_stop - time_start)      (the difference rounded once, by the caller)
//              t1 = cos(TWO_PI * theta),  t2 = cos(FOUR_PI * theta)     TWO_PI = 2 * f32(pi), FOUR_PI = 4 * f32(pi), both exact
//   dir_t of spherindrical_harmonics_lookup IS this dt (gaussian.wgsl:322 passes gaussian_4d.dir_t): t1 and t2 are per
//   splat. They and `marginal` are cosf / expf of the build's math library: the device's and a host's may differ by
//   their documented error, every other lane is the same bits everywhere. Masked splats' coefficients are folded too.
//
// TWO STATED DEVIATIONS from the reference:
//   1. The fold reorders the colour sum. The reference adds t1 * (sum over the 16 basis terms) to the colour; here the
//      coefficient that multiplies each basis term is summed first. The colour is linear in the coefficients, so the two
//      agree in exact arithmetic; tests/test_time_slice_host.py bounds the difference by the image tolerance.
//   2. A slice is depth-sorted by the conditioned mean p + delta. The reference's keygen reads the unconditioned p.
//
// WHAT THE REFERENCE'S FORMULA IS. Sigma = M^T * M with M = R * S is S * (R^T * R) * S, and R^T * R = |q|^2 |q_r|^2 * I
// for every pair: both factors are scaled orthogonal matrices. In exact arithmetic Sigma is therefore the DIAGONAL
// |q|^2 |q_r|^2 * S^2 whatever the pair is, cov12 = 0 and delta = 0; what f32 leaves of them is rounding residue, which
// this contract reproduces bit for bit like everything else. The rotation pair scales a 4D splat and does not turn it.
//
// Non-finite input goes where the arithmetic takes it: a NaN marginal is masked; time_scale = 0 gives cov_t = 0, an
// exponent of -inf (masked) or, with dt = 0, NaN (masked). A NaN's sign and payload are no part of the contract.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BGST_HD __host__ __device__ __forceinline__
#else
#define BGST_HD static inline
#endif

namespace bgst {

constexpr float TWO_PI = 6.2831854820251465f;     // 2 * f32(pi)
constexpr float FOUR_PI = 12.566370964050293f;    // 4 * f32(pi)
constexpr float MASK_THRESHOLD = 0.05f;
constexpr uint32_t SH_COEFFS = 48;                // of the slice; a 4D splat has three such groups

// Everything of a splat's geometry up to the one call of exp.
struct Conditioned {
    float dt;
    float cov_t;
    float exponent;
    float cov3d[6];   // xx, xy, xz, yy, yz, zz of cov11 - (cov12 (x) cov12) / cov_t
    float delta[3];   // (cov12 / cov_t) * dt
};

BGST_HD float dot4(float a0, float b0, float a1, float b1, float a2, float b2, float a3, float b3) {
    return ((a0 * b0 + a1 * b1) + a2 * b2) + a3 * b3;
}

// rot: (w, x, y, z), rot_r: (wr, xr, yr, zr), scale: (sx, sy, sz)
BGST_HD Conditioned condition(const float rot[4], const float rot_r[4], const float scale[3], float timestamp, float time_scale,
                              float global_scale, float time) {
    const float w = rot[0], x = rot[1], y = rot[2], z = rot[3];
    const float wr = rot_r[0], xr = rot_r[1], yr = rot_r[2], zr = rot_r[3];
    const float ml[4][4] = {{w, x, y, z}, {-x, w, z, -y}, {-y, -z, w, x}, {-z, y, -x, w}};
    const float mr[4][4] = {{wr, xr, yr, zr}, {-xr, wr, -zr, yr}, {-yr, zr, wr, -xr}, {-zr, -yr, xr, wr}};
    const float s[4] = {global_scale * scale[0], global_scale * scale[1], global_scale * scale[2], time_scale};
    float m[4][4];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            m[r][c] = dot4(mr[r][0], ml[0][c], mr[r][1], ml[1][c], mr[r][2], ml[2][c], mr[r][3], ml[3][c]) * s[c];
#define BGST_SIGMA(i, j) dot4(m[0][i], m[0][j], m[1][i], m[1][j], m[2][i], m[2][j], m[3][i], m[3][j])
    Conditioned out;
    out.dt = time - timestamp;
    out.cov_t = BGST_SIGMA(3, 3);
    out.exponent = ((-0.5f * out.dt) * out.dt) / out.cov_t;
    const float c0 = BGST_SIGMA(0, 3), c1 = BGST_SIGMA(1, 3), c2 = BGST_SIGMA(2, 3);
    out.cov3d[0] = BGST_SIGMA(0, 0) - (c0 * c0) / out.cov_t;
    out.cov3d[1] = BGST_SIGMA(0, 1) - (c0 * c1) / out.cov_t;
    out.cov3d[2] = BGST_SIGMA(0, 2) - (c0 * c2) / out.cov_t;
    out.cov3d[3] = BGST_SIGMA(1, 1) - (c1 * c1) / out.cov_t;
    out.cov3d[4] = BGST_SIGMA(1, 2) - (c1 * c2) / out.cov_t;
    out.cov3d[5] = BGST_SIGMA(2, 2) - (c2 * c2) / out.cov_t;
#undef BGST_SIGMA
    out.delta[0] = (c0 / out.cov_t) * out.dt;
    out.delta[1] = (c1 / out.cov_t) * out.dt;
    out.delta[2] = (c2 / out.cov_t) * out.dt;
    return out;
}

// The stated functions of the three lanes that pass through a math library.
BGST_HD float marginal_of(float exponent) { return expf(exponent); }

BGST_HD bool unmasked(float marginal) { return marginal > MASK_THRESHOLD; }

// duration = time_stop - time_start, rounded once by the caller
BGST_HD void time_cosines(float dt, float duration, float* t1, float* t2) {
    const float theta = dt / duration;
    *t1 = cosf(TWO_PI * theta);
    *t2 = cosf(FOUR_PI * theta);
}

// One splat's two output records. pv: (x, y, z, visibility) in; pv_out and cov_out[8] out.
BGST_HD void slice_geometry(const float pv[4], const Conditioned& g, float marginal, float opacity, float pv_out[4], float cov_out[8]) {
    const bool keep = unmasked(marginal);
    pv_out[0] = keep ? pv[0] + g.delta[0] : pv[0];
    pv_out[1] = keep ? pv[1] + g.delta[1] : pv[1];
    pv_out[2] = keep ? pv[2] + g.delta[2] : pv[2];
    pv_out[3] = pv[3];
    for (int k = 0; k < 6; ++k) cov_out[k] = keep ? g.cov3d[k] : 0.0f;
    cov_out[6] = keep ? opacity * marginal : 0.0f;
    cov_out[7] = 0.0f;
}

BGST_HD float fold(float sh0, float sh1, float sh2, float t1, float t2) { return (sh0 + t1 * sh1) + t2 * sh2; }

}  // namespace bgst
