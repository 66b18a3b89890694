// sparse_math.h — sparse-splat selection (src/query/sparse.rs:41-53): how many splats lie within `radius` of a splat.
// Shared by the device kernels (sparse_kernels.hip) and a g++ build (tests/host_shim/sparse_math_shim.cpp), like
// csrc_query/mesh_query_math.h.
//
// ARITHMETIC CONTRACT: f32 throughout, every operation rounded once (both builds use -ffp-contract=off):
//
//   d2(i, j)    = ((0 + dx*dx) + dy*dy) + dz*dz      with dx = x_j - x_i, dy, dz likewise
//   near(i, j)  = d2(i, j) < radius*radius           (strict; the product rounded once)
//   count(i)    = #{ j in [0, n) : near(i, j) }      (j = i included: a finite point counts itself)
//   reported(i) = cap == 0 ? count(i) : min(count(i), cap)
//   sparse(i)   = count(i) < neighbor_threshold
//
// This is what SparseSelect::select does through kd_tree::KdTree::within_radius. UNPINNED: the kd-tree crate's source
// (0.6.2) was not at hand when this was written; the strict `<`, the squared distance summed axis by axis from zero and
// the self-count are that crate's as remembered, not as read. STATED DEVIATION: the crate's per-axis box prefilter
// [q - r, q + r] is not reproduced; it can differ only where a rounded q +- r excludes a point the distance test accepts.
//
// A NaN or infinite difference makes d2 NaN or +inf and `near` false: a point with a non-finite lane has count 0 and is
// counted by nobody. The fourth lane of a point (visibility) is never read. near(i, j) == near(j, i): negating dx leaves
// dx*dx as it is. Every result is an integer that does not depend on the order in which pairs were visited.
//
// THE GRID IS AN ACCELERATOR ONLY. cell_of() is not part of the contract: the counts equal the all-pairs count for every
// input. What the kernels rely on (DESIGN.md section 8 has the argument): with the cell scale of cell_scale(), two points
// with near(i, j) lie in cells that differ by at most 1 along every axis.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define BGSS_HD __host__ __device__ __forceinline__
#else
#define BGSS_HD static inline
#endif

namespace bgss {

BGSS_HD float distance_squared(float xi, float yi, float zi, float xj, float yj, float zj) {
    const float dx = xj - xi, dy = yj - yi, dz = zj - zi;
    return ((0.0f + dx * dx) + dy * dy) + dz * dz;
}

// radius_squared = radius * radius, rounded once by the caller
BGSS_HD bool near(float xi, float yi, float zi, float xj, float yj, float zj, float radius_squared) {
    return distance_squared(xi, yi, zi, xj, yj, zj) < radius_squared;
}

BGSS_HD uint32_t reported(uint32_t count, uint32_t cap) { return cap != 0u && count > cap ? cap : count; }

// ---- the grid -----------------------------------------------------------------------------------------------------------------
// Cells are cubes of edge radius * (1 + 2^-10), numbered per axis from 0 to 2 * CELL_LIMIT after clamping. The one
// multiplication is done in f64: its error at a cell number below 2^22 is under 2^-30, far inside the margin 2^-10.
constexpr int32_t CELL_LIMIT = 1 << 20;

BGSS_HD double cell_scale(float radius) { return 1.0 / ((double)radius * (1.0 + 1.0 / 1024.0)); }

// Monotone in x, and safe for every f32: the value is clamped as a double BEFORE it becomes an integer (a NaN goes to cell
// 0: such a point is near nobody, wherever it is filed).
BGSS_HD uint32_t cell_of(float x, double scale) {
    double u = (double)x * scale;
    if (!(u >= -(double)CELL_LIMIT)) u = -(double)CELL_LIMIT;
    if (!(u <= (double)CELL_LIMIT)) u = (double)CELL_LIMIT;
    return (uint32_t)((int32_t)__builtin_floor(u) + CELL_LIMIT);
}

// Ten low bits of each cell number. Two cells of one 3 x 3 x 3 block differ by at most 2 along an axis, so their tags
// differ; the block may hang over the clamped range, where the numbers wrap as uint32 and the rule still holds.
BGSS_HD uint32_t cell_tag(uint32_t cx, uint32_t cy, uint32_t cz) { return (cx & 1023u) | ((cy & 1023u) << 10) | ((cz & 1023u) << 20); }

// The slot of cell (cx, cy, cz) is (row_hash(cy, cz) + cx) & mask: the three x-neighbours of a cell are three
// consecutive slots, one cache line as a rule.
BGSS_HD uint32_t row_hash(uint32_t cy, uint32_t cz) {
    uint32_t h = cy * 0x9E3779B1u + cz * 0x85EBCA77u;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    return h;
}

}  // namespace bgss
