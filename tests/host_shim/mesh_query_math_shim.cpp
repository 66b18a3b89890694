// mesh_query_math_shim.cpp — TEST-ONLY host build of the product's point-in-mesh arithmetic.
//
// Compiles bevy_gaussian_splatting_amd/csrc_query/mesh_query_math.h with g++ (same flags as particle_math_shim.cpp) so that
// tests/test_mesh_query_host.py can compare the operations the HIP kernels run with the numpy twin (mesh_query.py
// crossings_reference) WITHOUT a GPU. The loops around them mirror triangle_prep_kernel and crossings_kernel pair for pair.
// Not a product path: libbgs_query never counts crossings on the host.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../bevy_gaussian_splatting_amd/csrc_query/mesh_query_math.h"

extern "C" {

// points: n x stride floats (xyz read); vertices: V x 3; indices: T x 3 (validated by the caller); m: column-major 4x4
void shim_crossings(const float* points, uint32_t n, uint32_t stride, const float* vertices, const uint32_t* indices, uint32_t triangles,
                    const float* m, uint32_t* crossings) {
    std::vector<bgsq::TriangleRecord> records(triangles);
    for (uint32_t t = 0; t < triangles; ++t)
        records[t] = bgsq::triangle_prepare(vertices + 3u * (size_t)indices[3u * (size_t)t], vertices + 3u * (size_t)indices[3u * (size_t)t + 1u],
                                            vertices + 3u * (size_t)indices[3u * (size_t)t + 2u]);
#pragma omp parallel for
    for (int64_t i = 0; i < (int64_t)n; ++i) {
        const float* w = points + (size_t)i * stride;
        float px, py, pz;
        bgsq::local_point(m, w[0], w[1], w[2], px, py, pz);
        uint32_t count = 0;
        for (uint32_t t = 0; t < triangles; ++t) count += bgsq::ray_crosses(records[t], px, py, pz) ? 1u : 0u;
        crossings[i] = (bgsq::finite_f32(px) && bgsq::finite_f32(py) && bgsq::finite_f32(pz)) ? count : 0u;
    }
}

// the 48-byte records as triangle_prep_kernel writes them
void shim_triangle_records(const float* vertices, const uint32_t* indices, uint32_t triangles, void* records_out) {
    for (uint32_t t = 0; t < triangles; ++t) {
        const bgsq::TriangleRecord r = bgsq::triangle_prepare(vertices + 3u * (size_t)indices[3u * (size_t)t],
                                                              vertices + 3u * (size_t)indices[3u * (size_t)t + 1u],
                                                              vertices + 3u * (size_t)indices[3u * (size_t)t + 2u]);
        memcpy((uint8_t*)records_out + (size_t)t * sizeof r, &r, sizeof r);
    }
}

uint32_t shim_record_bytes(void) { return (uint32_t)sizeof(bgsq::TriangleRecord); }

}  // extern "C"
