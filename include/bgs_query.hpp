// bgs_query.hpp — C++ host side above the C ABI of libbgs_query.so (include/bgs_query.h): point-in-mesh selection on the
// device, the reference's query_raycast (src/query/raycast.rs). Header-only, C++17, no HIP headers needed: link
// libbgs_query.so. It does not need bgs.hpp; with it, a selection reaches the draw through a kept chunk:
//
//   bgs::query::MeshQuery hull(bgs::query::icosphere_mesh(3), /*hip_device*/ 0);
//   plugin.sort(cloud, view, settings, chunk);                       // bgs_sort into the chunk (blocking)
//   hull.crossings(plugin.stream(), points_ptr, n, mesh_from_points, crossings_ptr);
//   hull.entries_keep(plugin.stream(), chunk_ptr, n, crossings_ptr, n);
//   plugin.synchronize();                                            // then bgs_render with the chunk
//
// Every failure of the C ABI becomes a bgs::query::Error carrying the status and bgsq_last_error().
#ifndef BGS_QUERY_HPP
#define BGS_QUERY_HPP

#include <array>
#include <cmath>
#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "bgs_query.h"

namespace bgs {
namespace query {

class Error : public std::runtime_error {
  public:
    Error(int status, const std::string& what) : std::runtime_error(what), status_(status) {}
    int status() const { return status_; }

  private:
    int status_;
};

inline void check(int status) {
    if (status != BGSQ_OK) throw Error(status, bgsq_last_error());
}

using Mat4 = std::array<float, 16>;  // column-major, m[4 * c + r] (glam)

// A triangle list as the reference reads one: ATTRIBUTE_POSITION as float3, Indices::U32, TriangleList.
struct TriangleMesh {
    std::vector<std::array<float, 3>> vertices;
    std::vector<std::array<uint32_t, 3>> indices;
    size_t triangle_count() const { return indices.size(); }
};

// The axis-aligned cube [-h, h]^3 as 12 triangles, outward winding; vertex index = 4 ix + 2 iy + iz.
inline TriangleMesh cube_mesh(float half_extent = 0.5f) {
    TriangleMesh m;
    const float h = half_extent;
    for (float x : {-h, h})
        for (float y : {-h, h})
            for (float z : {-h, h}) m.vertices.push_back({x, y, z});
    const uint32_t quads[6][4] = {{0, 1, 3, 2}, {4, 6, 7, 5}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 2, 6, 4}, {1, 5, 7, 3}};
    for (const auto& q : quads) {
        m.indices.push_back({q[0], q[1], q[2]});
        m.indices.push_back({q[0], q[2], q[3]});
    }
    return m;
}

// An icosahedron, each triangle split in four `subdivisions` times, every vertex on the sphere of `radius`:
// 20 * 4^subdivisions triangles, closed, outward winding. Built in double, rounded once.
inline TriangleMesh icosphere_mesh(unsigned subdivisions = 0, double radius = 1.0) {
    using V = std::array<double, 3>;
    auto unit = [](V v) {
        const double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        return V{v[0] / n, v[1] / n, v[2] / n};
    };
    const double t = (1.0 + std::sqrt(5.0)) / 2.0;
    std::vector<V> verts = {{-1, t, 0}, {1, t, 0}, {-1, -t, 0}, {1, -t, 0}, {0, -1, t}, {0, 1, t},
                            {0, -1, -t}, {0, 1, -t}, {t, 0, -1}, {t, 0, 1}, {-t, 0, -1}, {-t, 0, 1}};
    for (auto& v : verts) v = unit(v);
    std::vector<std::array<uint32_t, 3>> faces = {{0, 11, 5}, {0, 5, 1}, {0, 1, 7}, {0, 7, 10}, {0, 10, 11}, {1, 5, 9}, {5, 11, 4},
                                                  {11, 10, 2}, {10, 7, 6}, {7, 1, 8}, {3, 9, 4}, {3, 4, 2}, {3, 2, 6}, {3, 6, 8},
                                                  {3, 8, 9}, {4, 9, 5}, {2, 4, 11}, {6, 2, 10}, {8, 6, 7}, {9, 8, 1}};
    for (unsigned level = 0; level < subdivisions; ++level) {
        std::map<std::pair<uint32_t, uint32_t>, uint32_t> middle;
        auto mid = [&](uint32_t a, uint32_t b) {
            const auto key = std::make_pair(a < b ? a : b, a < b ? b : a);
            const auto it = middle.find(key);
            if (it != middle.end()) return it->second;
            verts.push_back(unit(V{verts[a][0] + verts[b][0], verts[a][1] + verts[b][1], verts[a][2] + verts[b][2]}));
            return middle[key] = (uint32_t)verts.size() - 1u;
        };
        std::vector<std::array<uint32_t, 3>> split;
        for (const auto& f : faces) {
            const uint32_t ab = mid(f[0], f[1]), bc = mid(f[1], f[2]), ca = mid(f[2], f[0]);
            split.push_back({f[0], ab, ca});
            split.push_back({f[1], bc, ab});
            split.push_back({f[2], ca, bc});
            split.push_back({ab, bc, ca});
        }
        faces.swap(split);
    }
    TriangleMesh m;
    for (const auto& v : verts) m.vertices.push_back({(float)(v[0] * radius), (float)(v[1] * radius), (float)(v[2] * radius)});
    m.indices = std::move(faces);
    return m;
}

// inverse(mesh GlobalTransform) * cloud GlobalTransform (raycast.rs:43-46 with the cloud's own transform in front),
// composed in double and rounded once. Both are affine (last row 0 0 0 1), as a GlobalTransform is.
inline Mat4 mesh_from_points(const Mat4& mesh_transform, const Mat4& cloud_transform = Mat4{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}) {
    double a[3][3], tr[3];
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) a[r][c] = mesh_transform[4 * c + r];
    for (int r = 0; r < 3; ++r) tr[r] = mesh_transform[12 + r];
    const double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                       a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    if (!(std::fabs(det) > 0.0)) throw Error(BGSQ_EINVAL, "mesh_from_points: the mesh transform is singular");
    double inv[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
            inv[r][c] = (a[r1][c1] * a[r2][c2] - a[r1][c2] * a[r2][c1]) / det;
        }
    double it[3];
    for (int r = 0; r < 3; ++r) it[r] = -(inv[r][0] * tr[0] + inv[r][1] * tr[1] + inv[r][2] * tr[2]);
    Mat4 out{};
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 3; ++r) {
            double s = c == 3 ? it[r] : 0.0;
            for (int k = 0; k < 3; ++k) s += inv[r][k] * (double)cloud_transform[4 * c + k];
            out[4 * c + r] = (float)s;
        }
    out[15] = 1.0f;
    return out;
}

// A TriangleMesh prepared on one HIP device (bgsq_mesh): its triangle records live in device memory until destruction.
// crossings() and entries_keep() only enqueue on the stream they are given (include/bgs_query.h "ORDERING").
class MeshQuery {
  public:
    MeshQuery(const TriangleMesh& mesh, int hip_device) : device_(hip_device) {
        check(bgsq_mesh_create(hip_device, mesh.vertices.empty() ? nullptr : mesh.vertices[0].data(), (uint32_t)mesh.vertices.size(),
                               mesh.indices.empty() ? nullptr : mesh.indices[0].data(), (uint32_t)mesh.indices.size(), &mesh_));
    }
    ~MeshQuery() { bgsq_mesh_free(mesh_); }
    MeshQuery(const MeshQuery&) = delete;
    MeshQuery& operator=(const MeshQuery&) = delete;
    MeshQuery(MeshQuery&& o) noexcept : mesh_(o.mesh_), device_(o.device_) { o.mesh_ = nullptr; }
    MeshQuery& operator=(MeshQuery&& o) noexcept {
        if (this != &o) {
            bgsq_mesh_free(mesh_);
            mesh_ = o.mesh_;
            device_ = o.device_;
            o.mesh_ = nullptr;
        }
        return *this;
    }

    uint32_t triangles() const { return bgsq_mesh_triangles(mesh_); }
    int device() const { return device_; }

    // crossings[i] = triangles the +x ray from mesh_from_points * points[i].xyz crosses; points: n x float4 on the device
    void crossings(void* hip_stream, const void* points_device_ptr, uint32_t n, const Mat4& mesh_from_points_matrix,
                   void* crossings_device_ptr) {
        check(bgsq_crossings(mesh_, hip_stream, points_device_ptr, n, mesh_from_points_matrix.data(), crossings_device_ptr));
    }
    // entries that name a point outside (with keep_outside: inside) get key 0xFFFFFFFF
    void entries_keep(void* hip_stream, void* entries_device_ptr, uint32_t entry_count, const void* crossings_device_ptr, uint32_t n,
                      bool keep_outside = false) {
        check(bgsq_entries_keep(device_, hip_stream, entries_device_ptr, entry_count, crossings_device_ptr, n,
                                keep_outside ? BGSQ_KEEP_OUTSIDE : BGSQ_KEEP_INSIDE));
    }
    void debug_set_slices(uint32_t slices) { check(bgsq_debug_set_slices(mesh_, slices)); }

  private:
    bgsq_mesh* mesh_ = nullptr;
    int device_ = 0;
};

}  // namespace query
}  // namespace bgs

#endif  // BGS_QUERY_HPP
