// sparse_kernels.hip — sparse-splat selection on the device (the reference's SparseSelect, src/query/sparse.rs): for
// every point, how many points lie within `radius` of it, by the arithmetic of sparse_math.h. A uniform grid with a hashed
// table of cells finds the candidates; the counts are those of all pairs. gfx950, wave64.
//
// Four launches on one stream, after the table and the cursor were zeroed on it. No kernel waits for another workgroup:
// there is no spin, no flag and no look-back, and every loop runs over a range that is at most n long.
//   1. cell_keys:  one thread per point adds 1 to its cell's slot (integer atomic)
//   2. ranges:     one thread per slot; a wave sums its slots' counts and takes its stretch of [0, n) with one atomicAdd
//   3. scatter:    one thread per point writes (x, y, z, cell tag) and its index at its slot's cursor (integer atomic)
//   4. count:      one lane per scattered point walks the slots of the 27 cells around it
// The order of points inside a slot and of the slots' ranges depends on the atomics' arrival; the counts do not: they are
// sums of ones over sets that do not.
#include "sparse_kernels.h"

namespace bgss {

namespace {

struct Cell {
    uint32_t x, y, z;
};

__device__ __forceinline__ Cell cell_of_point(float x, float y, float z, double scale) {
    return Cell{cell_of(x, scale), cell_of(y, scale), cell_of(z, scale)};
}

__device__ __forceinline__ uint32_t slot_of(const Cell& c, uint32_t mask) { return (row_hash(c.y, c.z) + c.x) & mask; }

}  // namespace

__global__ __launch_bounds__(THREADS) void cell_keys_kernel(const float4* __restrict__ points, uint32_t n, double scale, uint2* table,
                                                            uint32_t mask) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const float4 p = points[i];
    atomicAdd(&table[slot_of(cell_of_point(p.x, p.y, p.z, scale), mask)].x, 1u);
}

// A wave's 64 slots take one stretch of [0, n), in slot order inside it. Every lane runs the shuffles; slots past the
// table count as empty. The counts sum to n, so the cursor ends at n and no stretch passes it.
__global__ __launch_bounds__(THREADS) void ranges_kernel(uint2* table, uint32_t slots, uint32_t* cursor) {
    const uint64_t s = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t count = s < slots ? table[s].x : 0u;
    uint32_t inclusive = count;
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const uint32_t below = __shfl_up(inclusive, d, 64);
        if (lane >= d) inclusive += below;
    }
    uint32_t base = 0u;
    if (lane == 63u && inclusive != 0u) base = atomicAdd(cursor, inclusive);
    base = __shfl(base, 63, 64);
    if (count != 0u) table[s].y = base + (inclusive - count);
}

// After this launch a slot's cursor is the END of its range. A position is checked against n before it is written: it
// cannot pass n while the points are what stage 1 read, and a caller who rewrites them in between breaks only the counts.
__global__ __launch_bounds__(THREADS) void scatter_kernel(const float4* __restrict__ points, uint32_t n, double scale, uint2* table,
                                                          uint32_t mask, float4* __restrict__ scattered, uint32_t* __restrict__ order) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const float4 p = points[i];
    const Cell c = cell_of_point(p.x, p.y, p.z, scale);
    const uint32_t at = atomicAdd(&table[slot_of(c, mask)].y, 1u);
    if (at >= n) return;
    scattered[at] = make_float4(p.x, p.y, p.z, __uint_as_float(cell_tag(c.x, c.y, c.z)));   // the tag's bits are only ever copied
    order[at] = (uint32_t)i;
}

// The hot loop. Lanes in scattered order: a wave's points share their cells as a rule, so its table and candidate loads
// fall on the same lines. A slot may hold points of other cells (collisions), and two of the 27 cells may share a slot:
// a candidate is tested only while the lane walks the cell whose tag the candidate carries, and the 27 tags of a block
// differ, so a candidate is tested at most once — and exactly once when its cell is one of the 27, which it is whenever
// it is near.
__global__ __launch_bounds__(THREADS) void count_kernel(const float4* __restrict__ scattered, const uint32_t* __restrict__ order,
                                                        uint32_t n, double scale, const uint2* __restrict__ table, uint32_t mask,
                                                        float radius_squared, uint32_t cap, uint32_t* __restrict__ counts) {
    const uint64_t k = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (k >= n) return;
    const float4 me = scattered[k];
    const Cell c = cell_of_point(me.x, me.y, me.z, scale);
    constexpr uint32_t LAST_CELL = 2u * (uint32_t)CELL_LIMIT;
    uint32_t count = 0u;
    bool full = false;
    for (uint32_t dz = 0u; dz < 3u && !full; ++dz) {
        const uint32_t nz = c.z + dz - 1u;   // wraps below cell 0: no point is filed there
        if (nz > LAST_CELL) continue;
        for (uint32_t dy = 0u; dy < 3u && !full; ++dy) {
            const uint32_t ny = c.y + dy - 1u;
            if (ny > LAST_CELL) continue;
            const uint32_t row = row_hash(ny, nz);
            for (uint32_t dx = 0u; dx < 3u && !full; ++dx) {
                const uint32_t nx = c.x + dx - 1u;
                if (nx > LAST_CELL) continue;
                const uint2 slot = table[(row + nx) & mask];
                const uint32_t end = slot.y < n ? slot.y : n;
                const uint32_t length = slot.x < end ? slot.x : end;
                const uint32_t tag = cell_tag(nx, ny, nz);
                for (uint32_t j = end - length; j < end; ++j) {
                    const float4 q = scattered[j];
                    if (__float_as_uint(q.w) == tag && near(me.x, me.y, me.z, q.x, q.y, q.z, radius_squared)) {
                        ++count;
                        if (cap != 0u && count >= cap) {
                            full = true;
                            break;
                        }
                    }
                }
            }
        }
    }
    const uint32_t i = order[k];
    if (i < n) counts[i] = reported(count, cap);   // (always, unless the caller rewrote the points between the stages)
}

// One thread per entry, the twin of libbgs_query's entries_keep_kernel: an entry that names a point of the plane and whose
// point fails the predicate loses its key. Entries with index >= n and entries already at 0xFFFFFFFF stay as they are;
// index is never written.
__global__ __launch_bounds__(THREADS) void entries_keep_kernel(uint32_t* __restrict__ entries, uint32_t entry_count,
                                                               const uint32_t* __restrict__ counts, uint32_t n,
                                                               uint32_t neighbor_threshold, uint32_t dense) {
    const uint64_t e = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (e >= entry_count) return;
    const uint2 entry = reinterpret_cast<const uint2*>(entries)[e];
    if (entry.x == 0xFFFFFFFFu || entry.y >= n) return;
    const uint32_t sparse = counts[entry.y] < neighbor_threshold ? 1u : 0u;
    if (sparse == dense) entries[2u * e] = 0xFFFFFFFFu;
}

hipError_t launch_neighbor_counts(hipStream_t stream, const GridScratch& g, uint32_t table_bits, const float4* points, uint32_t n,
                                  float radius, uint32_t cap, uint32_t* counts) {
    if (n == 0u) return hipSuccess;
    const uint32_t slots = 1u << table_bits, mask = slots - 1u;
    const double scale = cell_scale(radius);
    const float radius_squared = radius * radius;
    const uint32_t point_blocks = (uint32_t)(((uint64_t)n + THREADS - 1u) / THREADS);
    const uint32_t slot_blocks = (uint32_t)(((uint64_t)slots + THREADS - 1u) / THREADS);
    hipError_t e = hipMemsetAsync(g.table, 0, (size_t)slots * sizeof(uint2), stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(g.cursor, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cell_keys_kernel, dim3(point_blocks), dim3(THREADS), 0, stream, points, n, scale, g.table, mask);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(ranges_kernel, dim3(slot_blocks), dim3(THREADS), 0, stream, g.table, slots, g.cursor);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(scatter_kernel, dim3(point_blocks), dim3(THREADS), 0, stream, points, n, scale, g.table, mask, g.scattered, g.order);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(count_kernel, dim3(point_blocks), dim3(THREADS), 0, stream, (const float4*)g.scattered, (const uint32_t*)g.order, n,
                       scale, (const uint2*)g.table, mask, radius_squared, cap, counts);
    return hipGetLastError();
}

hipError_t launch_entries_keep(hipStream_t stream, uint32_t* entries, uint32_t entry_count, const uint32_t* counts, uint32_t n,
                               uint32_t neighbor_threshold, uint32_t dense) {
    if (entry_count == 0u) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((uint64_t)entry_count + THREADS - 1u) / THREADS);
    hipLaunchKernelGGL(entries_keep_kernel, dim3(blocks), dim3(THREADS), 0, stream, entries, entry_count, counts, n, neighbor_threshold,
                       dense & 1u);
    return hipGetLastError();
}

}  // namespace bgss
