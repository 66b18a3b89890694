// mesh_query_math.h — point-in-mesh by ray parity (src/query/raycast.rs:31-124), shared by the device kernels
// (mesh_query_kernels.hip) and a g++ build (tests/host_shim/mesh_query_math_shim.cpp), like csrc/particle_math.h.
//
// ARITHMETIC CONTRACT: f32 throughout, every operation rounded once (both builds use -ffp-contract=off), the one division
// correctly rounded, in the scalar Vec3 order the reference's code implies (glam's scalar Mat4::transform_point3,
// Vec3::dot = (x*x' + y*y') + z*z', Vec3::cross):
//
//   local p (M = mesh_from_points, column-major):  r = col0*px;  r = col1*py + r;  r = col2*pz + r;  r = col3 + r   (xyz)
//   per triangle (v0, v1, v2):  e1 = v1 - v0;  e2 = v2 - v0;  h = (0, -e2.z, e2.y);  a = e1.y*h.y + e1.z*h.z
//                               a > -1e-6f && a < 1e-6f -> the triangle never hits;  f = 1.0f / a
//   per pair:  s = p - v0;  u = f * (s.y*h.y + s.z*h.z);  !(u >= 0 && u <= 1) -> miss
//              q = (s.y*e1.z - e1.y*s.z,  s.z*e1.x - e1.z*s.x,  s.x*e1.y - e1.x*s.y)
//              v = f * q.x;  v < 0 || (u + v) > 1 -> miss
//              t = f * ((e2.x*q.x + e2.y*q.y) + e2.z*q.z);  hit iff t > 1e-6f
//   crossings(p) = number of hits over all triangles;  inside(p) = crossings & 1
//
// The ray is +x. The reference forms cross((1,0,0), e2) and dot((1,0,0), q) in full, and its dot products with h carry the
// term x*h.x with h.x = 0*e2.z - 0*e2.y. Here the products with those literal zeros are dropped: h.y = -(e2.z) is the
// exact value of 0*e2.x - 1*e2.z, h.z = e2.y that of 1*e2.y - 0*e2.x, and adding a zero product to a sum can change only
// the sign of a zero result. No comparison above tells +0 from -0, so for finite operands (no difference or product that
// overflowed to infinity, where 0*inf would have made a NaN) every decision is the reference's.
//
// STATED DEVIATION: a point whose LOCAL position has a non-finite lane has 0 crossings. The reference's outcome there is
// an accident of NaN propagation through the comparisons.
//
// There is no bounding-box or grid culling: a point just outside a triangle's projection can still pass the ROUNDED u, v
// tests, so culling that is not proven exact breaks bit parity. All pairs are tested, as in the reference. The numpy twin
// is bevy_gaussian_splatting_amd/mesh_query.py crossings_reference.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define BGSQ_HD __host__ __device__ __forceinline__
#else
#define BGSQ_HD static inline
#endif

namespace bgsq {

constexpr float RAY_EPSILON = 1e-6f;   // `let epsilon = 0.000_001;` (raycast.rs:93)

// What the pair test needs of one triangle: 48 bytes, so that a wave reads it with three 16-byte scalar loads.
struct TriangleRecord {
    float v0[3];
    float e1[3];
    float e2[3];
    float f;        // 1 / a, or NaN for a triangle the `a` test rejects: u = NaN * .. then fails u >= 0 for every point
    float pad[2];
};
static_assert(sizeof(TriangleRecord) == 48, "the kernels index records of 48 bytes");

BGSQ_HD bool finite_f32(float x) {
    uint32_t b;
    __builtin_memcpy(&b, &x, 4);
    return (b & 0x7F800000u) != 0x7F800000u;
}

// xyz of M * (x, y, z, 1), M column-major (glam Mat4::transform_point3, scalar path)
BGSQ_HD void local_point(const float* m, float x, float y, float z, float& px, float& py, float& pz) {
    float r0 = m[0] * x, r1 = m[1] * x, r2 = m[2] * x;
    r0 = m[4] * y + r0;  r1 = m[5] * y + r1;  r2 = m[6] * y + r2;
    r0 = m[8] * z + r0;  r1 = m[9] * z + r1;  r2 = m[10] * z + r2;
    px = m[12] + r0;  py = m[13] + r1;  pz = m[14] + r2;
}

BGSQ_HD TriangleRecord triangle_prepare(const float* v0, const float* v1, const float* v2) {
    TriangleRecord r;
    for (int k = 0; k < 3; ++k) {
        r.v0[k] = v0[k];
        r.e1[k] = v1[k] - v0[k];
        r.e2[k] = v2[k] - v0[k];
    }
    const float hy = -r.e2[2], hz = r.e2[1];
    const float a = r.e1[1] * hy + r.e1[2] * hz;
    const bool rejected = a > -RAY_EPSILON && a < RAY_EPSILON;
    r.f = rejected ? __builtin_nanf("") : 1.0f / a;
    r.pad[0] = r.pad[1] = 0.0f;
    return r;
}

// Does the +x ray from the local point (px, py, pz) cross the triangle?
BGSQ_HD bool ray_crosses(const TriangleRecord& r, float px, float py, float pz) {
    const float hy = -r.e2[2], hz = r.e2[1];
    const float sx = px - r.v0[0], sy = py - r.v0[1], sz = pz - r.v0[2];
    const float u = r.f * (sy * hy + sz * hz);
    const float qx = sy * r.e1[2] - r.e1[1] * sz;
    const float qy = sz * r.e1[0] - r.e1[2] * sx;
    const float qz = sx * r.e1[1] - r.e1[0] * sy;
    const float v = r.f * qx;
    const float t = r.f * ((r.e2[0] * qx + r.e2[1] * qy) + r.e2[2] * qz);
    // written so that a NaN behaves as in the reference: `!(0..=1).contains(&u)` misses on NaN, `v < 0 || u + v > 1` does not
    return u >= 0.0f && u <= 1.0f && !(v < 0.0f) && !((u + v) > 1.0f) && t > RAY_EPSILON;
}

}  // namespace bgsq
