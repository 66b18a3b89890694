// sparse_math_shim.cpp — TEST-ONLY host build of the product's sparse-selection arithmetic.
//
// Compiles bevy_gaussian_splatting_amd/csrc_sparse/sparse_math.h with g++ (same flags as mesh_query_math_shim.cpp) so that
// tests/test_sparse_select_host.py can compare the operations the HIP kernels run with the numpy twin (sparse_select.py
// neighbor_counts_reference) WITHOUT a GPU. shim_counts tests all pairs. shim_grid_counts walks the grid as the four
// kernels of sparse_kernels.hip do (cells, slots, ranges, scatter with tags, the 27-cell walk), one point after the other:
// it shows that the grid's rules lose and double no pair, not that the kernels are right.
// Not a product path: libbgs_sparse never counts on the host.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../bevy_gaussian_splatting_amd/csrc_sparse/sparse_math.h"

extern "C" {

// points: n x stride floats (xyz read)
void shim_counts(const float* points, uint32_t n, uint32_t stride, float radius, uint32_t cap, uint32_t* counts) {
    const float r2 = radius * radius;
#pragma omp parallel for
    for (int64_t i = 0; i < (int64_t)n; ++i) {
        const float* a = points + (size_t)i * stride;
        uint32_t count = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const float* b = points + (size_t)j * stride;
            count += bgss::near(a[0], a[1], a[2], b[0], b[1], b[2], r2) ? 1u : 0u;
        }
        counts[i] = bgss::reported(count, cap);
    }
}

// the clamped cell numbers of every point, n x 3
void shim_cells(const float* points, uint32_t n, uint32_t stride, float radius, uint32_t* cells) {
    const double scale = bgss::cell_scale(radius);
    for (uint32_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) cells[3u * (size_t)i + k] = bgss::cell_of(points[(size_t)i * stride + k], scale);
}

void shim_grid_counts(const float* points, uint32_t n, uint32_t stride, float radius, uint32_t cap, uint32_t table_bits, uint32_t* counts) {
    const double scale = bgss::cell_scale(radius);
    const float r2 = radius * radius;
    const uint32_t slots = 1u << table_bits, mask = slots - 1u;
    struct Slot { uint32_t count, cursor; };
    struct Point { float x, y, z; uint32_t tag; };
    std::vector<Slot> table(slots, Slot{0u, 0u});
    std::vector<Point> scattered(n);
    std::vector<uint32_t> order(n);
    auto slot_of = [&](const float* p, uint32_t* tag) {
        const uint32_t cx = bgss::cell_of(p[0], scale), cy = bgss::cell_of(p[1], scale), cz = bgss::cell_of(p[2], scale);
        if (tag) *tag = bgss::cell_tag(cx, cy, cz);
        return (bgss::row_hash(cy, cz) + cx) & mask;
    };
    for (uint32_t i = 0; i < n; ++i) table[slot_of(points + (size_t)i * stride, nullptr)].count += 1u;
    uint32_t cursor = 0;
    for (uint32_t s = 0; s < slots; ++s)
        if (table[s].count) {
            table[s].cursor = cursor;
            cursor += table[s].count;
        }
    for (uint32_t i = 0; i < n; ++i) {
        const float* p = points + (size_t)i * stride;
        uint32_t tag;
        const uint32_t at = table[slot_of(p, &tag)].cursor++;
        scattered[at] = Point{p[0], p[1], p[2], tag};
        order[at] = i;
    }
    const uint32_t last = 2u * (uint32_t)bgss::CELL_LIMIT;
    for (uint32_t k = 0; k < n; ++k) {
        const Point me = scattered[k];
        const uint32_t cx = bgss::cell_of(me.x, scale), cy = bgss::cell_of(me.y, scale), cz = bgss::cell_of(me.z, scale);
        uint32_t count = 0;
        bool full = false;
        for (uint32_t dz = 0; dz < 3 && !full; ++dz)
            for (uint32_t dy = 0; dy < 3 && !full; ++dy)
                for (uint32_t dx = 0; dx < 3 && !full; ++dx) {
                    const uint32_t nx = cx + dx - 1u, ny = cy + dy - 1u, nz = cz + dz - 1u;
                    if (nx > last || ny > last || nz > last) continue;
                    const Slot s = table[(bgss::row_hash(ny, nz) + nx) & mask];
                    const uint32_t tag = bgss::cell_tag(nx, ny, nz);
                    for (uint32_t j = s.cursor - s.count; j < s.cursor; ++j) {
                        const Point q = scattered[j];
                        if (q.tag == tag && bgss::near(me.x, me.y, me.z, q.x, q.y, q.z, r2)) {
                            ++count;
                            if (cap != 0u && count >= cap) {
                                full = true;
                                break;
                            }
                        }
                    }
                }
        counts[order[k]] = bgss::reported(count, cap);
    }
}

}  // extern "C"
