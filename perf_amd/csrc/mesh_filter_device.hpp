// The compaction of a mesh by a kept predicate, shared by the component filter (meshcc.hip) and the visibility cull (meshvis.hip): the
// kept vertices' new indices, the kept vertices, the kept faces.  A unit states which vertices and faces it keeps as two small functors:
//   VertexKept: int64_t n_vertices; bool operator()(int64_t v) const    whether v is a vertex of the mesh that stays
//   FaceKept:   bool operator()(int64_t f, int32_t abc[3]) const        whether f is a face of the mesh that stays; then abc = its indices
// The kernels have internal linkage, as mesh_scan_device.hpp's.
#pragma once
#include "mesh_scan_device.hpp"

namespace perf {

namespace {

// prefix holds the exclusive prefixes of the groups' kept counts: the new index of every vertex, or -1.  new_index may be the array the
// predicate reads (a thread reads and writes its own word).
template <class VertexKept>
__global__ void __launch_bounds__(kScanGroup) filter_new_index_kernel(VertexKept vertex_kept, const uint64_t* __restrict__ prefix, int32_t* new_index) {
    const int64_t v = (int64_t)blockIdx.x * kScanGroup + threadIdx.x;
    const bool kept = vertex_kept(v);
    const int32_t r = group_rank(kept, nullptr);
    if (v < vertex_kept.n_vertices) new_index[v] = kept ? (int32_t)prefix[blockIdx.x] + r : -1;
}

__global__ void __launch_bounds__(kScanGroup) filter_write_vertices_kernel(const int32_t* __restrict__ new_index, int64_t n_vertices, const float* __restrict__ vertices,
                                                                           float* __restrict__ vertices_out, int32_t* __restrict__ kept_vertex_index,
                                                                           int64_t vertex_capacity) {
    const int64_t v = (int64_t)blockIdx.x * kScanGroup + threadIdx.x;
    if (v >= n_vertices) return;
    const int64_t n = new_index[v];
    if (n < 0 || n >= vertex_capacity) return;
    kept_vertex_index[n] = (int32_t)v;
    if (vertices) {
        vertices_out[3 * n] = vertices[3 * v];
        vertices_out[3 * n + 1] = vertices[3 * v + 1];
        vertices_out[3 * n + 2] = vertices[3 * v + 2];
    }
}

template <class FaceKept>
__global__ void __launch_bounds__(kScanGroup) filter_write_faces_kernel(FaceKept face_kept, const uint64_t* __restrict__ prefix, const int32_t* __restrict__ new_index,
                                                                        int32_t* __restrict__ faces_out, int64_t face_capacity) {
    const int64_t f = (int64_t)blockIdx.x * kScanGroup + threadIdx.x;
    int32_t abc[3];
    const bool kept = face_kept(f, abc);
    const int64_t n = (int64_t)prefix[blockIdx.x] + group_rank(kept, nullptr);
    if (!kept || n >= face_capacity) return;
    faces_out[3 * n] = new_index[abc[0]];
    faces_out[3 * n + 1] = new_index[abc[1]];
    faces_out[3 * n + 2] = new_index[abc[2]];
}

}  // namespace

}  // namespace perf
