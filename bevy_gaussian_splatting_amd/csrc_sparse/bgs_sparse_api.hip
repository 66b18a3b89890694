// bgs_sparse_api.hip — the C ABI of libbgs_sparse.so (include/bgs_sparse.h) over the launchers of sparse_kernels.hip.
#include <math.h>

#include <new>

#include "../../include/bgs_sparse.h"
#include "build_id.inc"
#include "sparse_kernels.h"
#include "../small_lib/api_support_hip.h"

// The SHA-256 of the sources this library was compiled from (../_build_id.py libbgs_sparse), readable from the
// file's bytes: the loader rebuilds a library that carries another one.
extern "C" __attribute__((used, visibility("hidden"))) const char bgss_build_id_marker[] = "BGSS_BUILD_ID=" BGSS_BUILD_ID;

static_assert(BGSS_EINVAL == API_EINVAL && BGSS_ENOMEM == API_ENOMEM && BGSS_EHIP == API_EHIP, "the shared support's status codes");

struct bgss_grid {
    int device = 0;
    uint32_t max_points = 0;
    uint32_t allocated_bits = 0;   // the table holds 2^allocated_bits slots
    uint32_t forced_bits = 0;      // 0 = automatic
    bgss::GridScratch scratch = {nullptr, nullptr, nullptr, nullptr};
};

namespace {

constexpr uint32_t MIN_TABLE_BITS = 6, MAX_TABLE_BITS = 26;

// The smallest table with at least two slots a point: half of them stay empty, so a cell seldom shares its slot.
uint32_t automatic_bits(uint32_t n) {
    uint32_t bits = MIN_TABLE_BITS;
    while (bits < MAX_TABLE_BITS && (1ull << bits) < 2ull * n) ++bits;
    return bits;
}

void release(bgss_grid* g) {
    if (g->scratch.table) (void)hipFree(g->scratch.table);   // hipFree waits for the launches that still use it
    if (g->scratch.cursor) (void)hipFree(g->scratch.cursor);
    if (g->scratch.scattered) (void)hipFree(g->scratch.scattered);
    if (g->scratch.order) (void)hipFree(g->scratch.order);
    delete g;
}

}  // namespace

extern "C" {

uint32_t bgss_version(void) { return ((uint32_t)BGSS_VERSION_MAJOR << 16) | (uint32_t)BGSS_VERSION_MINOR; }

const char* bgss_last_error(void) { return g_error; }

int bgss_grid_create(int hip_device, uint32_t max_points, bgss_grid** out) {
    g_error[0] = 0;
    if (!out) return fail(BGSS_EINVAL, "bgss_grid_create: out is NULL");
    *out = nullptr;
    if (const int refused = check_device("bgss_grid_create", hip_device)) return refused;
    DeviceScope scope(hip_device);
    if (scope.status() != hipSuccess) return fail_hip("hipSetDevice", scope.status());

    bgss_grid* g = new (std::nothrow) bgss_grid;
    if (!g) return fail(BGSS_ENOMEM, "bgss_grid_create: out of host memory");
    g->device = hip_device;
    g->max_points = max_points;
    g->allocated_bits = automatic_bits(max_points);
    const size_t points = max_points ? max_points : 1u;
    hipError_t e = hipMalloc((void**)&g->scratch.table, ((size_t)1u << g->allocated_bits) * sizeof(uint2));
    if (e == hipSuccess) e = hipMalloc((void**)&g->scratch.cursor, sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&g->scratch.scattered, points * sizeof(float4));
    if (e == hipSuccess) e = hipMalloc((void**)&g->scratch.order, points * sizeof(uint32_t));
    if (e != hipSuccess) {
        release(g);
        return e == hipErrorOutOfMemory ? fail(BGSS_ENOMEM, "bgss_grid_create: out of device memory (%u points)", max_points)
                                        : fail_hip("hipMalloc", e);
    }
    *out = g;
    return BGSS_OK;
}

void bgss_grid_free(bgss_grid* grid) {
    if (!grid) return;
    DeviceScope scope(grid->device);
    release(grid);
}

uint32_t bgss_grid_capacity(const bgss_grid* grid) { return grid ? grid->max_points : 0u; }

int bgss_neighbor_counts(bgss_grid* grid, void* hip_stream, const void* points_device_ptr, uint32_t n, float radius, uint32_t cap,
                         void* counts_device_ptr) {
    g_error[0] = 0;
    const float radius_squared = radius * radius;
    if (!isfinite(radius) || !(radius > 0.0f)) return fail(BGSS_EINVAL, "bgss_neighbor_counts: radius %g must be finite and positive", (double)radius);
    if (!(radius_squared > 0.0f) || !isfinite(radius_squared))
        return fail(BGSS_EINVAL, "bgss_neighbor_counts: radius %g has the square %g in f32", (double)radius, (double)radius_squared);
    if (n != 0u && (!points_device_ptr || ((uintptr_t)points_device_ptr & 15u)))
        return fail(BGSS_EINVAL, "bgss_neighbor_counts: points_device_ptr must be a 16-byte aligned device address");
    if (n != 0u && (!counts_device_ptr || ((uintptr_t)counts_device_ptr & 3u)))
        return fail(BGSS_EINVAL, "bgss_neighbor_counts: counts_device_ptr must be a 4-byte aligned device address");
    if (!grid) return fail(BGSS_EINVAL, "bgss_neighbor_counts: grid is NULL");
    if (n > grid->max_points) return fail(BGSS_EINVAL, "bgss_neighbor_counts: n %u is above the grid's capacity %u", n, grid->max_points);
    if (n == 0u) return BGSS_OK;
    DeviceScope scope(grid->device);
    if (scope.status() != hipSuccess) return fail_hip("hipSetDevice", scope.status());
    uint32_t bits = grid->forced_bits ? grid->forced_bits : automatic_bits(n);
    if (bits > grid->allocated_bits) bits = grid->allocated_bits;
    const hipError_t e = bgss::launch_neighbor_counts((hipStream_t)hip_stream, grid->scratch, bits, (const float4*)points_device_ptr, n,
                                                      radius, cap, (uint32_t*)counts_device_ptr);
    return e == hipSuccess ? BGSS_OK : fail_hip("bgss_neighbor_counts", e);
}

int bgss_entries_keep(int hip_device, void* hip_stream, void* entries_device_ptr, uint32_t entry_count, const void* counts_device_ptr,
                      uint32_t n, uint32_t neighbor_threshold, uint32_t flags) {
    g_error[0] = 0;
    if (flags > BGSS_KEEP_DENSE) return fail(BGSS_EINVAL, "bgss_entries_keep: flags %u (BGSS_KEEP_SPARSE or BGSS_KEEP_DENSE)", flags);
    if (entry_count == 0u) return BGSS_OK;
    if (!entries_device_ptr || ((uintptr_t)entries_device_ptr & 7u))
        return fail(BGSS_EINVAL, "bgss_entries_keep: entries_device_ptr must be an 8-byte aligned device address");
    if (n && (!counts_device_ptr || ((uintptr_t)counts_device_ptr & 3u)))
        return fail(BGSS_EINVAL, "bgss_entries_keep: counts_device_ptr must be a 4-byte aligned device address");
    if (n == 0u) return BGSS_OK;   // no entry names a point: nothing changes
    if (hip_device < 0) return fail(BGSS_EINVAL, "bgss_entries_keep: hip_device %d", hip_device);
    DeviceScope scope(hip_device);
    if (scope.status() != hipSuccess) return fail_hip("hipSetDevice", scope.status());
    const hipError_t e = bgss::launch_entries_keep((hipStream_t)hip_stream, (uint32_t*)entries_device_ptr, entry_count,
                                                   (const uint32_t*)counts_device_ptr, n, neighbor_threshold, flags);
    return e == hipSuccess ? BGSS_OK : fail_hip("bgss_entries_keep", e);
}

int bgss_debug_set_table_bits(bgss_grid* grid, uint32_t bits) {
    g_error[0] = 0;
    if (!grid) return fail(BGSS_EINVAL, "bgss_debug_set_table_bits: grid is NULL");
    grid->forced_bits = bits > grid->allocated_bits ? grid->allocated_bits : bits;   // 0 stays 0: automatic
    return BGSS_OK;
}

}  // extern "C"
