// bgs_sparse.hpp — C++ host side above the C ABI of libbgs_sparse.so (include/bgs_sparse.h): sparse-splat selection on
// the device, the reference's SparseSelect (src/query/sparse.rs). Header-only, C++17, no HIP headers needed: link
// libbgs_sparse.so. It does not need bgs.hpp; with it, a selection reaches the draw through a kept chunk:
//
//   bgs::sparse::Grid grid(/*hip_device*/ 0, /*max_points*/ n);
//   const bgs::sparse::SparseSelect floaters;                        // radius 0.05, neighbor_threshold 3
//   plugin.sort(cloud, view, settings, chunk);                       // bgs_sort into the chunk (blocking)
//   grid.neighbor_counts(plugin.stream(), points_ptr, n, floaters.radius, floaters.neighbor_threshold, counts_ptr);
//   grid.entries_keep(plugin.stream(), chunk_ptr, n, counts_ptr, n, floaters.neighbor_threshold, /*dense*/ true);
//   plugin.synchronize();                                            // then bgs_render with the chunk
//
// Every failure of the C ABI becomes a bgs::sparse::Error carrying the status and bgss_last_error().
#ifndef BGS_SPARSE_HPP
#define BGS_SPARSE_HPP

#include <cstdint>
#include <stdexcept>
#include <string>

#include "bgs_sparse.h"

namespace bgs {
namespace sparse {

class Error : public std::runtime_error {
  public:
    Error(int status, const std::string& what) : std::runtime_error(what), status_(status) {}
    int status() const { return status_; }

  private:
    int status_;
};

inline void check(int status) {
    if (status != BGSS_OK) throw Error(status, bgss_last_error());
}

// The reference's component with its defaults: a splat is selected when fewer than neighbor_threshold splats, itself
// included, lie within radius of it.
struct SparseSelect {
    float radius = 0.05f;
    uint32_t neighbor_threshold = 3;
};

// The device scratch of the counting stages (bgss_grid) for clouds of up to max_points, held until destruction.
// neighbor_counts() and entries_keep() only enqueue on the stream they are given (include/bgs_sparse.h "ORDERING").
class Grid {
  public:
    Grid(int hip_device, uint32_t max_points) : device_(hip_device) { check(bgss_grid_create(hip_device, max_points, &grid_)); }
    ~Grid() { bgss_grid_free(grid_); }
    Grid(const Grid&) = delete;
    Grid& operator=(const Grid&) = delete;
    Grid(Grid&& o) noexcept : grid_(o.grid_), device_(o.device_) { o.grid_ = nullptr; }
    Grid& operator=(Grid&& o) noexcept {
        if (this != &o) {
            bgss_grid_free(grid_);
            grid_ = o.grid_;
            device_ = o.device_;
            o.grid_ = nullptr;
        }
        return *this;
    }

    uint32_t capacity() const { return bgss_grid_capacity(grid_); }
    int device() const { return device_; }

    // counts[i] = points within radius of point i, itself included, clamped to cap when cap != 0; points: n x float4
    void neighbor_counts(void* hip_stream, const void* points_device_ptr, uint32_t n, float radius, uint32_t cap, void* counts_device_ptr) {
        check(bgss_neighbor_counts(grid_, hip_stream, points_device_ptr, n, radius, cap, counts_device_ptr));
    }
    // entries that name a point with counts >= neighbor_threshold (with dense: below it) get key 0xFFFFFFFF
    void entries_keep(void* hip_stream, void* entries_device_ptr, uint32_t entry_count, const void* counts_device_ptr, uint32_t n,
                      uint32_t neighbor_threshold, bool dense = false) {
        check(bgss_entries_keep(device_, hip_stream, entries_device_ptr, entry_count, counts_device_ptr, n, neighbor_threshold,
                                dense ? BGSS_KEEP_DENSE : BGSS_KEEP_SPARSE));
    }
    void debug_set_table_bits(uint32_t bits) { check(bgss_debug_set_table_bits(grid_, bits)); }

  private:
    bgss_grid* grid_ = nullptr;
    int device_ = 0;
};

}  // namespace sparse
}  // namespace bgs

#endif  // BGS_SPARSE_HPP
