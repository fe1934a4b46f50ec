// The texture atlas of a mesh without the panoramas (include/perf_hip_meshtex.h): the corner UVs and the materialised texel -> point map.
// The rule is meshtex_device.hpp's; the fused bake, which needs the blend, lives in meshcolor.hip.
#include "common.hpp"
#include "meshtex_device.hpp"

namespace perf {

// one thread per corner: face f, corner k of (a, b, c)
__global__ void __launch_bounds__(kTexGroup) meshtex_uv_kernel(int64_t n_faces, int32_t size, int32_t tile, float* __restrict__ uv) {
#pragma clang fp contract(off)
    const int64_t at = (int64_t)blockIdx.x * kTexGroup + threadIdx.x;
    if (at >= 3 * n_faces) return;
    const int64_t f = at / 3, t = f >> 1;
    const int32_t k = (int32_t)(at - 3 * f), h = (int32_t)(f & 1), n = size / tile, m = tile - 3;
    const int32_t x0 = (int32_t)(t % n) * tile, y0 = (int32_t)(t / n) * tile;
    const int32_t di = k == 1 ? m : 0, dj = k == 2 ? m : 0;          // a (0, 0), b (m, 0), c (0, m); half 1 mirrored
    const int32_t i = x0 + (h ? tile - 1 - di : di), j = y0 + (h ? tile - 1 - dj : dj);
    uv[2 * at] = __fdiv_rn(add_rn((float)i, 0.5f), (float)size);          // (the sum is exact: i < 2^14)
    uv[2 * at + 1] = __fdiv_rn(add_rn((float)j, 0.5f), (float)size);
}

// one thread per texel; nothing waits on another thread
__global__ void __launch_bounds__(kTexGroup) meshtex_points_kernel(const float* __restrict__ vertices, int64_t n_vertices, const float* __restrict__ normals,
                                                                   const int32_t* __restrict__ faces, int64_t n_faces, int32_t size, int32_t tile,
                                                                   float* __restrict__ points, float* __restrict__ point_normals, int32_t* __restrict__ face_of,
                                                                   uint8_t* __restrict__ coverage, unsigned long long* __restrict__ first_bad) {
#pragma clang fp contract(off)
    int32_t col, row;
    tex_thread_texel(col, row);
    if (col >= size || row >= size) return;
    TexOwner o = tex_owner(col, row, size, tile, n_faces);
    float p[3] = {0.0f, 0.0f, 0.0f}, nrm[3] = {0.0f, 0.0f, 0.0f};
    if (o.face >= 0) {
        int64_t abc[3];
        if (tex_face(faces, o.face, n_vertices, abc)) {
            const TexBary w = tex_bary(o, tile);
            tex_point(vertices, abc, w, p);
            tex_normal(vertices, normals, abc, w, nrm);
        } else {
            if (o.li == 0 && o.lj == 0) atomicMin(first_bad, (unsigned long long)o.face);          // (corner a: one texel per face)
            o.face = -1;
            o.code = PERF_MESHTEX_COVER_NONE;
        }
    }
    const int64_t at = (int64_t)row * size + col;
    points[3 * at] = p[0]; points[3 * at + 1] = p[1]; points[3 * at + 2] = p[2];
    point_normals[3 * at] = nrm[0]; point_normals[3 * at + 1] = nrm[1]; point_normals[3 * at + 2] = nrm[2];
    face_of[at] = (int32_t)o.face;
    coverage[at] = (uint8_t)o.code;
}

}  // namespace perf

using namespace perf;

extern "C" int perf_meshtex_version(void) { return PERF_MESHTEX_ABI_VERSION; }

extern "C" int perf_meshtex_uv(int64_t n_faces, int32_t size, int32_t tile, float* uv, void* stream) {
    const char* who = "perf_meshtex_uv";
    if (int rc = tex_layout_check(who, n_faces, size, tile)) return rc;
    PERF_REQUIRE(uv || n_faces == 0, "%s: NULL output (uv) with faces to place", who);
    if (n_faces == 0) return PERF_OK;
    hipLaunchKernelGGL(meshtex_uv_kernel, dim3((unsigned)div_up(3 * n_faces, kTexGroup)), dim3(kTexGroup), 0, as_stream(stream), n_faces, size, tile, uv);
    PERF_LAUNCH_CHECK(who);
    return PERF_OK;
}

extern "C" int perf_meshtex_points(const float* vertices, int64_t n_vertices, const float* normals, const int32_t* faces, int64_t n_faces, int32_t size,
                                   int32_t tile, float* points, float* point_normals, int32_t* face_of, uint8_t* coverage, int64_t* bad_face_dev,
                                   void* stream) {
    const char* who = "perf_meshtex_points";
    if (int rc = tex_layout_check(who, n_faces, size, tile)) return rc;
    PERF_REQUIRE(n_vertices >= 0, "%s: a negative number of vertices (%lld)", who, (long long)n_vertices);
    PERF_REQUIRE(n_vertices <= PERF_MESHTEX_MAX_VERTICES, "%s: %lld vertices are more than 2^30 (vertex indices are int32)", who, (long long)n_vertices);
    PERF_REQUIRE(vertices || n_vertices == 0, "%s: NULL input (vertices) with vertices", who);
    PERF_REQUIRE(faces || n_faces == 0, "%s: NULL input (faces) with faces to place", who);
    PERF_REQUIRE(points && point_normals && face_of && coverage, "%s: NULL output (points, point_normals, face_of or coverage)", who);
    PERF_REQUIRE(bad_face_dev, "%s: NULL output (bad_face_dev)", who);
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(bad_face_dev, 0xff, sizeof(int64_t), st) != hipSuccess) {          // the flag: no bad face (-1, the largest unsigned)
        (void)hipGetLastError();
        set_error("%s: clearing the flag failed", who);
        return PERF_E_LAUNCH;
    }
    hipLaunchKernelGGL(meshtex_points_kernel, tex_grid(size), dim3(kTexGroup), 0, st, vertices, n_vertices, normals, faces, n_faces, size, tile, points, point_normals,
                       face_of, coverage, (unsigned long long*)bad_face_dev);
    PERF_LAUNCH_CHECK(who);
    return PERF_OK;
}
