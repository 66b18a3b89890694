// mesh_query_kernels.h — launchers of mesh_query_kernels.hip, called by the C ABI (bgs_query_api.hip). Every launcher only
// enqueues on the stream it is given and returns the launch's hipError_t.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_query_math.h"

namespace bgsq {

constexpr uint32_t CROSSINGS_THREADS = 256;       // lanes per workgroup of crossings_kernel
constexpr uint32_t CROSSINGS_POINTS = 4;          // points a lane keeps in registers (P)
constexpr uint32_t CROSSINGS_BLOCK_POINTS = CROSSINGS_THREADS * CROSSINGS_POINTS;
constexpr uint32_t CROSSINGS_MAX_SLICES = 1024;   // grid.y; far below the launch limit of 65535
constexpr uint32_t CROSSINGS_MIN_SLICE = 64;      // the automatic choice gives a slice at least this many triangles

struct Mat4 {
    float m[16];   // column-major
};

// vertices: vertex_count x 3 floats, indices: triangle_count x 3, both on the device; records: triangle_count x 48 bytes out
hipError_t launch_triangle_prep(hipStream_t stream, const float* vertices, const uint32_t* indices, uint32_t triangle_count,
                                TriangleRecord* records);

// crossings[i] = number of triangles the +x ray from M * points[i].xyz crosses. slices >= 1; with more than one the plane
// is zeroed on the stream first and the slices add into it.
hipError_t launch_crossings(hipStream_t stream, const float4* points, uint32_t n, const Mat4& mesh_from_points,
                            const TriangleRecord* records, uint32_t triangle_count, uint32_t slices, uint32_t* crossings);

// entries: entry_count x (key, index); flags bit 0: keep the outside
hipError_t launch_entries_keep(hipStream_t stream, uint32_t* entries, uint32_t entry_count, const uint32_t* crossings, uint32_t n,
                               uint32_t flags);

}  // namespace bgsq
