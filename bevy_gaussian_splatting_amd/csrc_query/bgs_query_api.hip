// bgs_query_api.hip — the C ABI of libbgs_query.so (include/bgs_query.h) over the launchers of mesh_query_kernels.hip.
#include <math.h>

#include <new>

#include "../../include/bgs_query.h"
#include "build_id.inc"
#include "mesh_query_kernels.h"
#include "../small_lib/api_support_hip.h"

// The SHA-256 of the sources this library was compiled from (../_build_id.py libbgs_query), readable from the
// file's bytes: the loader rebuilds a library that carries another one.
extern "C" __attribute__((used, visibility("hidden"))) const char bgsq_build_id_marker[] = "BGSQ_BUILD_ID=" BGSQ_BUILD_ID;

static_assert(BGSQ_EINVAL == API_EINVAL && BGSQ_ENOMEM == API_ENOMEM && BGSQ_EHIP == API_EHIP, "the shared support's status codes");

struct bgsq_mesh {
    int device = 0;
    uint32_t triangle_count = 0;
    uint32_t slices = 0;             // 0 = automatic
    uint32_t compute_units = 0;
    bgsq::TriangleRecord* records = nullptr;   // device
};

namespace {

// Enough workgroups to give every compute unit two: below that, the triangle list is cut into slices.
uint32_t automatic_slices(const bgsq_mesh& m, uint32_t n) {
    const uint64_t point_blocks = ((uint64_t)n + bgsq::CROSSINGS_BLOCK_POINTS - 1u) / bgsq::CROSSINGS_BLOCK_POINTS;
    const uint64_t wanted = 2ull * (m.compute_units ? m.compute_units : 256u);
    if (point_blocks >= wanted) return 1u;
    uint64_t s = (wanted + point_blocks - 1u) / point_blocks;
    const uint64_t most = m.triangle_count / bgsq::CROSSINGS_MIN_SLICE;
    if (s > most) s = most;
    if (s > bgsq::CROSSINGS_MAX_SLICES) s = bgsq::CROSSINGS_MAX_SLICES;
    return s < 1u ? 1u : (uint32_t)s;
}

}  // namespace

extern "C" {

uint32_t bgsq_version(void) { return ((uint32_t)BGSQ_VERSION_MAJOR << 16) | (uint32_t)BGSQ_VERSION_MINOR; }

const char* bgsq_last_error(void) { return g_error; }

int bgsq_mesh_create(int hip_device, const float* vertices_xyz, uint32_t vertex_count, const uint32_t* indices,
                     uint32_t triangle_count, bgsq_mesh** out) {
    g_error[0] = 0;
    if (!out) return fail(BGSQ_EINVAL, "bgsq_mesh_create: out is NULL");
    *out = nullptr;
    if (vertex_count && !vertices_xyz) return fail(BGSQ_EINVAL, "bgsq_mesh_create: vertices_xyz is NULL with vertex_count %u", vertex_count);
    if (triangle_count && !indices) return fail(BGSQ_EINVAL, "bgsq_mesh_create: indices is NULL with triangle_count %u", triangle_count);
    for (uint64_t k = 0; k < 3ull * vertex_count; ++k)
        if (!bgsq::finite_f32(vertices_xyz[k]))
            return fail(BGSQ_EINVAL, "bgsq_mesh_create: vertex %llu has a non-finite %c", (unsigned long long)(k / 3u), "xyz"[k % 3u]);
    for (uint64_t k = 0; k < 3ull * triangle_count; ++k)
        if (indices[k] >= vertex_count)
            return fail(BGSQ_EINVAL, "bgsq_mesh_create: triangle %llu names vertex %u, the mesh has %u", (unsigned long long)(k / 3u),
                        indices[k], vertex_count);
    if (const int refused = check_device("bgsq_mesh_create", hip_device)) return refused;
    DeviceScope scope(hip_device);
    if (scope.status() != hipSuccess) return fail_hip("hipSetDevice", scope.status());

    bgsq_mesh* m = new (std::nothrow) bgsq_mesh;
    if (!m) return fail(BGSQ_ENOMEM, "bgsq_mesh_create: out of host memory");
    m->device = hip_device;
    m->triangle_count = triangle_count;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, hip_device) == hipSuccess && cus > 0) m->compute_units = (uint32_t)cus;
    if (triangle_count == 0u) {
        *out = m;
        return BGSQ_OK;
    }
    // The records are prepared on the device, on a stream of the mesh's own that nothing else ever sees.
    float* d_vertices = nullptr;
    uint32_t* d_indices = nullptr;
    hipStream_t stream = nullptr;
    const size_t vertex_bytes = (size_t)vertex_count * 3u * sizeof(float), index_bytes = (size_t)triangle_count * 3u * sizeof(uint32_t);
    int status = BGSQ_OK;
    hipError_t e = hipMalloc((void**)&m->records, (size_t)triangle_count * sizeof(bgsq::TriangleRecord));
    if (e == hipSuccess) e = hipMalloc((void**)&d_vertices, vertex_bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&d_indices, index_bytes);
    if (e != hipSuccess) {
        status = e == hipErrorOutOfMemory ? fail(BGSQ_ENOMEM, "bgsq_mesh_create: out of device memory (%u triangles)", triangle_count)
                                          : fail_hip("hipMalloc", e);
    } else {
        e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipMemcpyAsync(d_vertices, vertices_xyz, vertex_bytes, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_indices, indices, index_bytes, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = bgsq::launch_triangle_prep(stream, d_vertices, d_indices, triangle_count, m->records);
        if (stream) {
            const hipError_t s = hipStreamSynchronize(stream);   // the host arrays are borrowed for the call only
            if (e == hipSuccess) e = s;
            (void)hipStreamDestroy(stream);
        }
        if (e != hipSuccess) status = fail_hip("bgsq_mesh_create: preparing the triangle records", e);
    }
    if (d_vertices) (void)hipFree(d_vertices);
    if (d_indices) (void)hipFree(d_indices);
    if (status != BGSQ_OK) {
        if (m->records) (void)hipFree(m->records);
        delete m;
        return status;
    }
    *out = m;
    return BGSQ_OK;
}

void bgsq_mesh_free(bgsq_mesh* mesh) {
    if (!mesh) return;
    if (mesh->records) {
        DeviceScope scope(mesh->device);
        (void)hipFree(mesh->records);   // waits for the launches that still read the records
    }
    delete mesh;
}

uint32_t bgsq_mesh_triangles(const bgsq_mesh* mesh) { return mesh ? mesh->triangle_count : 0u; }

int bgsq_crossings(bgsq_mesh* mesh, void* hip_stream, const void* points_device_ptr, uint32_t n, const float mesh_from_points[16],
                   void* crossings_device_ptr) {
    g_error[0] = 0;
    if (!mesh) return fail(BGSQ_EINVAL, "bgsq_crossings: mesh is NULL");
    if (!mesh_from_points) return fail(BGSQ_EINVAL, "bgsq_crossings: mesh_from_points is NULL");
    if (n == 0u) return BGSQ_OK;
    if (!points_device_ptr || ((uintptr_t)points_device_ptr & 15u))
        return fail(BGSQ_EINVAL, "bgsq_crossings: points_device_ptr must be a 16-byte aligned device address");
    if (!crossings_device_ptr || ((uintptr_t)crossings_device_ptr & 3u))
        return fail(BGSQ_EINVAL, "bgsq_crossings: crossings_device_ptr must be a 4-byte aligned device address");
    DeviceScope scope(mesh->device);
    if (scope.status() != hipSuccess) return fail_hip("hipSetDevice", scope.status());
    bgsq::Mat4 m;
    for (int k = 0; k < 16; ++k) m.m[k] = mesh_from_points[k];
    const uint32_t slices = mesh->slices ? mesh->slices : automatic_slices(*mesh, n);
    const hipError_t e = bgsq::launch_crossings((hipStream_t)hip_stream, (const float4*)points_device_ptr, n, m, mesh->records,
                                                mesh->triangle_count, slices, (uint32_t*)crossings_device_ptr);
    return e == hipSuccess ? BGSQ_OK : fail_hip("bgsq_crossings", e);
}

int bgsq_entries_keep(int hip_device, void* hip_stream, void* entries_device_ptr, uint32_t entry_count,
                      const void* crossings_device_ptr, uint32_t n, uint32_t flags) {
    g_error[0] = 0;
    if (flags > BGSQ_KEEP_OUTSIDE) return fail(BGSQ_EINVAL, "bgsq_entries_keep: flags %u (BGSQ_KEEP_INSIDE or BGSQ_KEEP_OUTSIDE)", flags);
    if (entry_count == 0u) return BGSQ_OK;
    if (!entries_device_ptr || ((uintptr_t)entries_device_ptr & 7u))
        return fail(BGSQ_EINVAL, "bgsq_entries_keep: entries_device_ptr must be an 8-byte aligned device address");
    if (n && (!crossings_device_ptr || ((uintptr_t)crossings_device_ptr & 3u)))
        return fail(BGSQ_EINVAL, "bgsq_entries_keep: crossings_device_ptr must be a 4-byte aligned device address");
    if (n == 0u) return BGSQ_OK;   // no entry names a point: nothing changes
    if (hip_device < 0) return fail(BGSQ_EINVAL, "bgsq_entries_keep: hip_device %d", hip_device);
    DeviceScope scope(hip_device);
    if (scope.status() != hipSuccess) return fail_hip("hipSetDevice", scope.status());
    const hipError_t e = bgsq::launch_entries_keep((hipStream_t)hip_stream, (uint32_t*)entries_device_ptr, entry_count,
                                                   (const uint32_t*)crossings_device_ptr, n, flags);
    return e == hipSuccess ? BGSQ_OK : fail_hip("bgsq_entries_keep", e);
}

int bgsq_debug_set_slices(bgsq_mesh* mesh, uint32_t slices) {
    g_error[0] = 0;
    if (!mesh) return fail(BGSQ_EINVAL, "bgsq_debug_set_slices: mesh is NULL");
    mesh->slices = slices;   // launch_crossings clamps it to [1, min(triangle count, CROSSINGS_MAX_SLICES)]
    return BGSQ_OK;
}

}  // extern "C"
