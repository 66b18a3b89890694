// sparse_kernels.h — launchers of sparse_kernels.hip, called by the C ABI (bgs_sparse_api.hip). Every launcher only
// enqueues on the stream it is given and returns the first hipError_t that was not hipSuccess.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sparse_math.h"

namespace bgss {

constexpr uint32_t THREADS = 256;   // lanes per workgroup of every kernel here

// What the four stages work in; all of it is the grid's, sized for its max_points.
struct GridScratch {
    uint2* table;        // 2^bits slots of (count, cursor); after the scatter a slot's points are [cursor - count, cursor)
    uint32_t* cursor;    // one word: where the next non-empty slot's range starts
    float4* scattered;   // n x (x, y, z, bitcast cell tag), slot by slot
    uint32_t* order;     // n: the original index of each scattered point
};

// counts[i] = reported(count(i)) for i < n (sparse_math.h). table_bits in [1, 31]: the table has 2^table_bits slots.
hipError_t launch_neighbor_counts(hipStream_t stream, const GridScratch& g, uint32_t table_bits, const float4* points, uint32_t n,
                                  float radius, uint32_t cap, uint32_t* counts);

// entries: entry_count x (key, index); dense = 0 keeps the sparse points' entries, 1 the others'
hipError_t launch_entries_keep(hipStream_t stream, uint32_t* entries, uint32_t entry_count, const uint32_t* counts, uint32_t n,
                               uint32_t neighbor_threshold, uint32_t dense);

}  // namespace bgss
