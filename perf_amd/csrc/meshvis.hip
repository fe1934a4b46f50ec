// Cull the faces of a mesh no registered panorama saw (include/perf_hip_meshvis.h): vertex bits (one launch for all views) -> face rule ->
// compaction by the face mask (mark -> rank -> scan -> write).  The look-up of stage 1 is pano_lookup_device.hpp's, the one
// pano_reproject_kernel (visibility.hip) runs; the scan and the group rank are mesh_scan_device.hpp's, the compaction mesh_filter_device.hpp's.
#include "common.hpp"
#include "mesh_filter_device.hpp"
#include "pano_lookup_device.hpp"
#include "../../include/perf_hip_meshvis.h"

namespace perf {

constexpr int kVisGroup = kScanGroup;        // items of one workgroup: one per thread (group_rank's workgroup)
constexpr int kVisViewWords = sizeof(perf_meshvis_view) / 4;
static_assert(sizeof(perf_meshvis_view) == 64 && alignof(perf_meshvis_view) == 8, "the view descriptor is 64 bytes");

// ---- stage 1 ----------------------------------------------------------------------------------------------------------------------------
// dist and proj of one point in one view
__device__ __forceinline__ void vis_lookup(float x, float y, float z, const perf_meshvis_view& pf, float& dist_out, float& proj_out) {
    const int32_t h = pf.height, w = pf.width;
    const PanoPixel p = pano_pixel(x, y, z, pf.rt, pf.t, h, w);
    dist_out = p.dist;
    proj_out = pano_tap(pf.distance_map, h, w, p);
}

// A workgroup stages its 256 vertices (768 consecutive floats, loaded in three coalesced passes) and the views' descriptors in LDS; a
// thread then loops over the views, every read of a descriptor the same LDS word for the whole wave.  All 256 threads arrive at the barrier.
__global__ void __launch_bounds__(kVisGroup) meshvis_vertex_bits_kernel(const float* __restrict__ vertices, int64_t n_vertices,
                                                                        const perf_meshvis_view* __restrict__ views, int32_t n_views, float tol, float neg_free_tol,
                                                                        unsigned long long* __restrict__ visible_bits, unsigned long long* __restrict__ free_bits) {
    __shared__ perf_meshvis_view view[PERF_MESHVIS_MAX_VIEWS];
    __shared__ float xyz[3 * kVisGroup];
    const int64_t first = (int64_t)blockIdx.x * kVisGroup;
    const uint32_t* __restrict__ words = reinterpret_cast<const uint32_t*>(views);
    uint32_t* staged = reinterpret_cast<uint32_t*>(view);
    for (int k = threadIdx.x; k < n_views * kVisViewWords; k += kVisGroup) staged[k] = words[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t at = 3 * first + k * kVisGroup + threadIdx.x;
        xyz[k * kVisGroup + threadIdx.x] = at < 3 * n_vertices ? vertices[at] : 0.0f;
    }
    __syncthreads();
    const int64_t i = first + threadIdx.x;
    if (i >= n_vertices) return;
    const float x = xyz[3 * threadIdx.x], y = xyz[3 * threadIdx.x + 1], z = xyz[3 * threadIdx.x + 2];
    unsigned long long visible = 0, free_space = 0;
    for (int k = 0; k < n_views; ++k) {
        float dist, proj;
        vis_lookup(x, y, z, view[k], dist, proj);
        if (dist < add_rn(proj, tol)) visible |= 1ull << k;
        if (dist < add_rn(proj, neg_free_tol)) free_space |= 1ull << k;
    }
    visible_bits[i] = visible;
    free_bits[i] = free_space;
}

// ---- stage 2 ----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kVisGroup) meshvis_face_keep_kernel(const int32_t* __restrict__ faces, int64_t n_faces, const float* __restrict__ vertices,
                                                                      int64_t n_vertices, const unsigned long long* __restrict__ visible_bits,
                                                                      const unsigned long long* __restrict__ free_bits, const float* __restrict__ centres,
                                                                      int32_t n_views, int32_t facing, int32_t min_views, int32_t carve,
                                                                      uint8_t* __restrict__ face_keep, unsigned long long* __restrict__ first_bad) {
#pragma clang fp contract(off)
    __shared__ float centre[3 * PERF_MESHVIS_MAX_VIEWS];
    if (facing)
        for (int k = threadIdx.x; k < 3 * n_views; k += kVisGroup) centre[k] = centres[k];
    __syncthreads();
    const int64_t f = (int64_t)blockIdx.x * kVisGroup + threadIdx.x;
    if (f >= n_faces) return;
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (!(a >= 0 && a < n_vertices && b >= 0 && b < n_vertices && c >= 0 && c < n_vertices)) {
        atomicMin(first_bad, (unsigned long long)f);
        face_keep[f] = 0;
        return;
    }
    const unsigned long long low = n_views >= 64 ? ~0ull : (1ull << n_views) - 1ull;
    unsigned long long bits = visible_bits[a] & visible_bits[b] & visible_bits[c] & low;
    if (facing && bits) {
        const double ax = vertices[3 * (int64_t)a], ay = vertices[3 * (int64_t)a + 1], az = vertices[3 * (int64_t)a + 2];
        const double e1x = (double)vertices[3 * (int64_t)b] - ax, e1y = (double)vertices[3 * (int64_t)b + 1] - ay, e1z = (double)vertices[3 * (int64_t)b + 2] - az;
        const double e2x = (double)vertices[3 * (int64_t)c] - ax, e2y = (double)vertices[3 * (int64_t)c + 1] - ay, e2z = (double)vertices[3 * (int64_t)c + 2] - az;
        const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        unsigned long long todo = bits;
        while (todo) {
            const int k = __ffsll(todo) - 1;
            todo &= todo - 1;
            const double gx = (double)centre[3 * k] - ax, gy = (double)centre[3 * k + 1] - ay, gz = (double)centre[3 * k + 2] - az;
            const double s = (nx * gx + ny * gy) + nz * gz;
            if (!(s > 0.0)) bits &= ~(1ull << k);
        }
    }
    bool keep = __popcll(bits) >= min_views;
    if (carve && keep) keep = ((free_bits[a] | free_bits[b] | free_bits[c]) & low) == 0;
    face_keep[f] = keep ? 1 : 0;
}

// ---- stage 3: the compaction (mesh_filter_device.hpp) by the face mask ---------------------------------------------------------------------
struct VisLayout {
    int32_t* a;              // [V] 1 where a kept face names the vertex; then the kept vertices' new indices (-1: dropped)
    uint64_t* vsums;         // S(V)
    uint64_t* fsums;         // S(F)
    int64_t* totals;         // [4] (V', F', 0, 0)
};

static inline VisLayout vis_layout(void* workspace, int64_t n_vertices, int64_t n_faces) {
    VisLayout l;
    l.a = (int32_t*)workspace;
    l.vsums = (uint64_t*)workspace + (n_vertices + 1) / 2;
    l.fsums = l.vsums + group_words(n_vertices);
    l.totals = (int64_t*)(l.fsums + group_words(n_faces));
    return l;
}

// a face is kept iff the mask says so and its three indices are vertices
__device__ __forceinline__ bool vis_face_kept(const int32_t* __restrict__ faces, const uint8_t* __restrict__ face_keep, int64_t n_faces, int64_t n_vertices, int64_t f,
                                              int32_t abc[3]) {
    if (f >= n_faces || face_keep[f] == 0) return false;
    abc[0] = faces[3 * f]; abc[1] = faces[3 * f + 1]; abc[2] = faces[3 * f + 2];
    return abc[0] >= 0 && abc[0] < n_vertices && abc[1] >= 0 && abc[1] < n_vertices && abc[2] >= 0 && abc[2] < n_vertices;
}

struct VisFaceKept {
    const int32_t* faces;
    const uint8_t* face_keep;
    int64_t n_faces, n_vertices;
    __device__ __forceinline__ bool operator()(int64_t f, int32_t abc[3]) const { return vis_face_kept(faces, face_keep, n_faces, n_vertices, f, abc); }
};

// a vertex is kept iff a kept face marked it
struct VisVertexKept {
    const int32_t* marks;
    int64_t n_vertices;
    __device__ __forceinline__ bool operator()(int64_t v) const { return v < n_vertices && marks[v] != 0; }
};

// marks [V] are 0 before the launch: a kept face stores 1 on its three vertices (every store to a word stores the same value); the
// group's count of kept faces to sums
__global__ void __launch_bounds__(kVisGroup) meshvis_mark_kernel(const int32_t* __restrict__ faces, const uint8_t* __restrict__ face_keep, int64_t n_faces,
                                                                 int64_t n_vertices, int32_t* marks, uint64_t* __restrict__ sums) {
    const int64_t f = (int64_t)blockIdx.x * kVisGroup + threadIdx.x;
    int32_t abc[3];
    const bool kept = vis_face_kept(faces, face_keep, n_faces, n_vertices, f, abc);
    if (kept) { marks[abc[0]] = 1; marks[abc[1]] = 1; marks[abc[2]] = 1; }
    group_rank(kept, sums);
}

__global__ void __launch_bounds__(kVisGroup) meshvis_count_vertices_kernel(const int32_t* __restrict__ marks, int64_t n_vertices, uint64_t* __restrict__ sums) {
    const int64_t v = (int64_t)blockIdx.x * kVisGroup + threadIdx.x;
    group_rank(v < n_vertices && marks[v] != 0, sums);
}

__global__ void meshvis_totals_kernel(const uint64_t* __restrict__ first, const uint64_t* __restrict__ second, int64_t* __restrict__ totals,
                                      int64_t* __restrict__ counts_dev) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t a = first ? (int64_t)first[0] : 0, b = second ? (int64_t)second[0] : 0;
    totals[0] = a; totals[1] = b; totals[2] = 0; totals[3] = 0;
    counts_dev[0] = a; counts_dev[1] = b;
}

// ---- the checks of the entry points -------------------------------------------------------------------------------------------------------
static int vis_counts_check(const char* who, int64_t n_vertices, int64_t n_faces) {
    return mesh_counts_check(who, n_vertices, n_faces, PERF_MESHVIS_MAX_VERTICES, PERF_MESHVIS_MAX_FACES, "2^38");
}

static int vis_views_check(const char* who, int32_t n_views) {
    PERF_REQUIRE(n_views >= 0, "%s: a negative number of views (%d)", who, n_views);
    PERF_REQUIRE(n_views <= PERF_MESHVIS_MAX_VIEWS, "%s: %d views are more than 64 (a vertex has one bit per view in a 64-bit word)", who, n_views);
    return PERF_OK;
}

static int vis_workspace_check(const char* who, int64_t n_vertices, int64_t n_faces, const void* workspace, int64_t workspace_bytes) {
    return workspace_check(who, perf_meshvis_workspace_bytes(n_vertices, n_faces), workspace, workspace_bytes);
}

static int vis_filter_check(const char* who, const int32_t* faces, int64_t n_faces, int64_t n_vertices, const uint8_t* face_keep, const void* workspace,
                            int64_t workspace_bytes) {
    if (int rc = vis_counts_check(who, n_vertices, n_faces)) return rc;
    PERF_REQUIRE(faces || n_faces == 0, "%s: NULL input (faces) with faces to filter", who);
    PERF_REQUIRE(face_keep || n_faces == 0, "%s: NULL input (face_keep) with faces to filter", who);
    return vis_workspace_check(who, n_vertices, n_faces, workspace, workspace_bytes);
}

}  // namespace perf

using namespace perf;

extern "C" int perf_meshvis_version(void) { return PERF_MESHVIS_ABI_VERSION; }

extern "C" int64_t perf_meshvis_sizeof_view(void) { return (int64_t)sizeof(perf_meshvis_view); }

extern "C" int64_t perf_meshvis_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
    if (vis_counts_check("perf_meshvis_workspace_bytes", n_vertices, n_faces) != PERF_OK) return -1;
    const int64_t words = (n_vertices + 1) / 2 + group_words(n_vertices) + group_words(n_faces) + 4;
    return ((words + 1) & ~(int64_t)1) * (int64_t)sizeof(uint64_t);      // (a multiple of 16)
}

extern "C" int perf_meshvis_vertex_bits(const float* vertices, int64_t n_vertices, const perf_meshvis_view* views_dev, const int32_t* view_sizes,
                                        int32_t n_views, float tol, float free_tol, int64_t* visible_bits, int64_t* free_bits, void* stream) {
    if (int rc = vis_counts_check("perf_meshvis_vertex_bits", n_vertices, 0)) return rc;
    if (int rc = vis_views_check("perf_meshvis_vertex_bits", n_views)) return rc;
    PERF_REQUIRE(tol >= 0.0f && tol <= 3.0e38f, "perf_meshvis_vertex_bits: tol %g is negative or not finite", (double)tol);
    PERF_REQUIRE(free_tol >= 0.0f && free_tol <= 3.0e38f, "perf_meshvis_vertex_bits: free_tol %g is negative or not finite", (double)free_tol);
    PERF_REQUIRE(vertices || n_vertices == 0, "perf_meshvis_vertex_bits: NULL input (vertices) with vertices to test");
    PERF_REQUIRE((views_dev && view_sizes) || n_views == 0, "perf_meshvis_vertex_bits: NULL input (views_dev or view_sizes) with views to test against");
    PERF_REQUIRE((reinterpret_cast<uintptr_t>(views_dev) & 7) == 0, "perf_meshvis_vertex_bits: views_dev must be 8-byte aligned");
    PERF_REQUIRE((visible_bits && free_bits) || n_vertices == 0, "perf_meshvis_vertex_bits: NULL output (visible_bits or free_bits) with vertices to test");
    for (int k = 0; k < n_views; ++k)
        PERF_REQUIRE(view_sizes[2 * k] >= 1 && view_sizes[2 * k + 1] >= 1, "perf_meshvis_vertex_bits: view %d has a map of %d x %d: a map dimension below 1", k,
                     view_sizes[2 * k], view_sizes[2 * k + 1]);
    if (n_vertices == 0) return PERF_OK;
    hipLaunchKernelGGL(meshvis_vertex_bits_kernel, dim3(scan_groups(n_vertices)), dim3(kVisGroup), 0, as_stream(stream), vertices, n_vertices, views_dev, n_views, tol,
                       -free_tol, (unsigned long long*)visible_bits, (unsigned long long*)free_bits);
    PERF_LAUNCH_CHECK("perf_meshvis_vertex_bits");
    return PERF_OK;
}

extern "C" int perf_meshvis_face_keep(const int32_t* faces, int64_t n_faces, const float* vertices, int64_t n_vertices, const int64_t* visible_bits,
                                      const int64_t* free_bits, const float* centres, int32_t n_views, int32_t facing, int32_t min_views, int32_t carve,
                                      uint8_t* face_keep, int64_t* bad_face_dev, void* stream) {
    if (int rc = vis_counts_check("perf_meshvis_face_keep", n_vertices, n_faces)) return rc;
    if (int rc = vis_views_check("perf_meshvis_face_keep", n_views)) return rc;
    PERF_REQUIRE((facing == 0 || facing == 1) && (carve == 0 || carve == 1), "perf_meshvis_face_keep: facing (%d) and carve (%d) are 0 or 1", facing, carve);
    PERF_REQUIRE(min_views >= 1, "perf_meshvis_face_keep: min_views %d is below 1", min_views);
    PERF_REQUIRE(faces || n_faces == 0, "perf_meshvis_face_keep: NULL input (faces) with faces to test");
    PERF_REQUIRE(visible_bits || n_vertices == 0 || n_faces == 0, "perf_meshvis_face_keep: NULL input (visible_bits) with faces to test");
    PERF_REQUIRE(free_bits || !carve || n_vertices == 0 || n_faces == 0, "perf_meshvis_face_keep: NULL input (free_bits) with carve");
    PERF_REQUIRE((vertices && centres) || !facing || n_vertices == 0 || n_faces == 0 || n_views == 0,
                 "perf_meshvis_face_keep: NULL input (vertices or centres) with facing");
    PERF_REQUIRE(face_keep || n_faces == 0, "perf_meshvis_face_keep: NULL output (face_keep) with faces to test");
    PERF_REQUIRE(bad_face_dev, "perf_meshvis_face_keep: NULL output (bad_face_dev)");
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(bad_face_dev, 0xff, sizeof(int64_t), st) != hipSuccess) {          // the flag: no bad face (-1, the largest unsigned)
        (void)hipGetLastError();
        set_error("perf_meshvis_face_keep: clearing the flag failed");
        return PERF_E_LAUNCH;
    }
    if (n_faces > 0)
        hipLaunchKernelGGL(meshvis_face_keep_kernel, dim3(scan_groups(n_faces)), dim3(kVisGroup), 0, st, faces, n_faces, vertices, n_vertices,
                           (const unsigned long long*)visible_bits, (const unsigned long long*)free_bits, centres, n_views, facing, min_views, carve, face_keep,
                           (unsigned long long*)bad_face_dev);
    PERF_LAUNCH_CHECK("perf_meshvis_face_keep");
    return PERF_OK;
}

extern "C" int perf_meshvis_filter_count(const int32_t* faces, int64_t n_faces, int64_t n_vertices, const uint8_t* face_keep, void* workspace,
                                         int64_t workspace_bytes, int64_t* counts_dev, void* stream) {
    if (int rc = vis_filter_check("perf_meshvis_filter_count", faces, n_faces, n_vertices, face_keep, workspace, workspace_bytes)) return rc;
    PERF_REQUIRE(counts_dev, "perf_meshvis_filter_count: NULL output (counts_dev)");
    const VisLayout l = vis_layout(workspace, n_vertices, n_faces);
    hipStream_t st = as_stream(stream);
    const uint64_t *v_total = nullptr, *f_total = nullptr;
    if (n_vertices > 0 && hipMemsetAsync(l.a, 0, n_vertices * sizeof(int32_t), st) != hipSuccess) {
        (void)hipGetLastError();
        set_error("perf_meshvis_filter_count: clearing the marks failed");
        return PERF_E_LAUNCH;
    }
    if (n_faces > 0) {
        const unsigned groups = scan_groups(n_faces);
        hipLaunchKernelGGL(meshvis_mark_kernel, dim3(groups), dim3(kVisGroup), 0, st, faces, face_keep, n_faces, n_vertices, l.a, l.fsums);
        f_total = scan_u64(l.fsums, groups, l.fsums + groups, st);
    }
    if (n_vertices > 0) {
        const unsigned groups = scan_groups(n_vertices);
        hipLaunchKernelGGL(meshvis_count_vertices_kernel, dim3(groups), dim3(kVisGroup), 0, st, (const int32_t*)l.a, n_vertices, l.vsums);
        v_total = scan_u64(l.vsums, groups, l.vsums + groups, st);
        hipLaunchKernelGGL(filter_new_index_kernel<VisVertexKept>, dim3(groups), dim3(kVisGroup), 0, st, VisVertexKept{l.a, n_vertices}, (const uint64_t*)l.vsums, l.a);
    }
    hipLaunchKernelGGL(meshvis_totals_kernel, dim3(1), dim3(64), 0, st, v_total, f_total, l.totals, counts_dev);
    PERF_LAUNCH_CHECK("perf_meshvis_filter_count");
    return PERF_OK;
}

extern "C" int perf_meshvis_filter_write(const int32_t* faces, int64_t n_faces, int64_t n_vertices, const uint8_t* face_keep, const float* vertices,
                                         const void* workspace, int64_t workspace_bytes, float* vertices_out, int32_t* kept_vertex_index,
                                         int64_t vertex_capacity, int32_t* faces_out, int64_t face_capacity, void* stream) {
    if (int rc = vis_filter_check("perf_meshvis_filter_write", faces, n_faces, n_vertices, face_keep, workspace, workspace_bytes)) return rc;
    PERF_REQUIRE(vertex_capacity >= 0 && face_capacity >= 0, "perf_meshvis_filter_write: negative capacity");
    PERF_REQUIRE((kept_vertex_index || vertex_capacity == 0) && (faces_out || face_capacity == 0) && (vertices_out || !vertices || vertex_capacity == 0),
                 "perf_meshvis_filter_write: NULL output with a capacity above 0");
    const VisLayout l = vis_layout(const_cast<void*>(workspace), n_vertices, n_faces);
    hipStream_t st = as_stream(stream);
    int64_t totals[4] = {0, 0, 0, 0};
    if (hipMemcpyAsync(totals, l.totals, sizeof(totals), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        (void)hipGetLastError();
        set_error("perf_meshvis_filter_write: reading the counted totals back failed");
        return PERF_E_LAUNCH;
    }
    PERF_REQUIRE(vertex_capacity >= totals[0], "perf_meshvis_filter_write: room for %lld vertices, %lld were counted", (long long)vertex_capacity, (long long)totals[0]);
    PERF_REQUIRE(face_capacity >= totals[1], "perf_meshvis_filter_write: room for %lld faces, %lld were counted", (long long)face_capacity, (long long)totals[1]);
    if (totals[0] == 0) return PERF_OK;                     // (no kept vertex: no kept face either)
    hipLaunchKernelGGL(filter_write_vertices_kernel, dim3(scan_groups(n_vertices)), dim3(kVisGroup), 0, st, (const int32_t*)l.a, n_vertices, vertices, vertices_out,
                       kept_vertex_index, vertex_capacity);
    if (totals[1] > 0)
        hipLaunchKernelGGL(filter_write_faces_kernel<VisFaceKept>, dim3(scan_groups(n_faces)), dim3(kVisGroup), 0, st, VisFaceKept{faces, face_keep, n_faces, n_vertices},
                           (const uint64_t*)l.fsums, (const int32_t*)l.a, faces_out, face_capacity);
    PERF_LAUNCH_CHECK("perf_meshvis_filter_write");
    return PERF_OK;
}
