// mesh_query_kernels.hip — point-in-mesh selection on the device (the reference's query_raycast, src/query/raycast.rs):
// brute force over every (point, triangle) pair, the arithmetic of mesh_query_math.h. gfx950, wave64.
#include "mesh_query_kernels.h"

namespace bgsq {

// One thread per triangle: gather the three vertices, write the 48-byte record the pair test reads.
__global__ __launch_bounds__(256) void triangle_prep_kernel(const float* __restrict__ vertices, const uint32_t* __restrict__ indices,
                                                            uint32_t triangle_count, TriangleRecord* __restrict__ records) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= triangle_count) return;
    const uint32_t i0 = indices[3u * (size_t)t], i1 = indices[3u * (size_t)t + 1u], i2 = indices[3u * (size_t)t + 2u];
    float v[3][3];
    for (int k = 0; k < 3; ++k) {
        v[0][k] = vertices[3u * (size_t)i0 + k];
        v[1][k] = vertices[3u * (size_t)i1 + k];
        v[2][k] = vertices[3u * (size_t)i2 + k];
    }
    records[t] = triangle_prepare(v[0], v[1], v[2]);
}

// The hot loop. grid = (point blocks, triangle slices). A lane keeps CROSSINGS_POINTS local points in registers; the
// triangle index is a uniform loop counter and the records come through a const __restrict__ pointer, so a record is
// fetched once per wave by scalar loads into SGPRs and used for 64 x CROSSINGS_POINTS pairs. No LDS, no scratch.
// A lane's points are CROSSINGS_THREADS apart, so each of its loads and stores is coalesced across the wave.
__global__ __launch_bounds__(CROSSINGS_THREADS) void crossings_kernel(const float4* __restrict__ points, uint32_t n, Mat4 mesh_from_points,
                                                                      const TriangleRecord* __restrict__ records, uint32_t triangle_count,
                                                                      uint32_t slice_triangles, uint32_t* __restrict__ crossings,
                                                                      uint32_t merge) {
    constexpr uint32_t P = CROSSINGS_POINTS;
    const uint64_t base = (uint64_t)blockIdx.x * CROSSINGS_BLOCK_POINTS + threadIdx.x;
    float px[P], py[P], pz[P];
    uint32_t count[P];
    bool counted[P];   // in range and finite: everything else reports 0 crossings
#pragma unroll
    for (uint32_t k = 0; k < P; ++k) {
        const uint64_t i = base + (uint64_t)k * CROSSINGS_THREADS;
        count[k] = 0u;
        px[k] = py[k] = pz[k] = 0.0f;
        counted[k] = false;
        if (i < n) {
            const float4 w = points[i];
            local_point(mesh_from_points.m, w.x, w.y, w.z, px[k], py[k], pz[k]);
            counted[k] = finite_f32(px[k]) && finite_f32(py[k]) && finite_f32(pz[k]);
        }
    }
    // slice_triangles * gridDim.y >= triangle_count, both below 2^32: the products below stay in 64 bits, the bounds in 32
    const uint64_t first = (uint64_t)blockIdx.y * slice_triangles;
    const uint32_t t0 = first < triangle_count ? (uint32_t)first : triangle_count;
    const uint32_t t1 = first + slice_triangles < triangle_count ? (uint32_t)(first + slice_triangles) : triangle_count;
    for (uint32_t t = t0; t < t1; ++t) {
        const TriangleRecord r = records[t];
#pragma unroll
        for (uint32_t k = 0; k < P; ++k) count[k] += ray_crosses(r, px[k], py[k], pz[k]) ? 1u : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < P; ++k) {
        const uint64_t i = base + (uint64_t)k * CROSSINGS_THREADS;
        if (i >= n) continue;
        const uint32_t c = counted[k] ? count[k] : 0u;
        if (!merge)
            crossings[i] = c;
        else if (c)
            atomicAdd(&crossings[i], c);   // an integer sum: the slices' order does not show
    }
}

// One thread per entry: an entry that names a point of the plane and whose point fails the predicate loses its key.
// Entries with index >= n and entries already at 0xFFFFFFFF stay as they are; index is never written.
__global__ __launch_bounds__(256) void entries_keep_kernel(uint32_t* __restrict__ entries, uint32_t entry_count,
                                                           const uint32_t* __restrict__ crossings, uint32_t n, uint32_t keep_outside) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= entry_count) return;
    const uint2 entry = reinterpret_cast<const uint2*>(entries)[e];
    if (entry.x == 0xFFFFFFFFu || entry.y >= n) return;
    const uint32_t inside = crossings[entry.y] & 1u;
    if (inside == keep_outside) entries[2u * e] = 0xFFFFFFFFu;
}

hipError_t launch_triangle_prep(hipStream_t stream, const float* vertices, const uint32_t* indices, uint32_t triangle_count,
                                TriangleRecord* records) {
    if (triangle_count == 0u) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((uint64_t)triangle_count + 255u) / 256u);
    hipLaunchKernelGGL(triangle_prep_kernel, dim3(blocks), dim3(256), 0, stream, vertices, indices, triangle_count, records);
    return hipGetLastError();
}

hipError_t launch_crossings(hipStream_t stream, const float4* points, uint32_t n, const Mat4& mesh_from_points,
                            const TriangleRecord* records, uint32_t triangle_count, uint32_t slices, uint32_t* crossings) {
    if (n == 0u) return hipSuccess;
    if (slices < 1u) slices = 1u;
    if (slices > CROSSINGS_MAX_SLICES) slices = CROSSINGS_MAX_SLICES;
    if (slices > triangle_count) slices = triangle_count ? triangle_count : 1u;
    const uint32_t slice_triangles = (uint32_t)(((uint64_t)triangle_count + slices - 1u) / slices);
    const uint32_t blocks = (uint32_t)(((uint64_t)n + CROSSINGS_BLOCK_POINTS - 1u) / CROSSINGS_BLOCK_POINTS);
    const uint32_t merge = slices > 1u ? 1u : 0u;
    if (merge) {
        const hipError_t e = hipMemsetAsync(crossings, 0, (size_t)n * sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(crossings_kernel, dim3(blocks, slices), dim3(CROSSINGS_THREADS), 0, stream, points, n, mesh_from_points, records,
                       triangle_count, slice_triangles, crossings, merge);
    return hipGetLastError();
}

hipError_t launch_entries_keep(hipStream_t stream, uint32_t* entries, uint32_t entry_count, const uint32_t* crossings, uint32_t n,
                               uint32_t flags) {
    if (entry_count == 0u) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((uint64_t)entry_count + 255u) / 256u);
    hipLaunchKernelGGL(entries_keep_kernel, dim3(blocks), dim3(256), 0, stream, entries, entry_count, crossings, n, flags & 1u);
    return hipGetLastError();
}

}  // namespace bgsq
