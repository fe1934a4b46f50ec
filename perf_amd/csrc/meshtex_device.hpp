// The texture atlas of include/perf_hip_meshtex.h stated once: texel -> (face, li, lj) -> (beta, gamma) -> point / normal / fallback, and
// the layout's host check.  meshtex.hip stores what this header forms; the bake of meshcolor.hip takes the same values through the blend.
// It names no view and no panorama: neither perf_hip_meshvis.h nor perf_hip_meshcolor.h is included here.
#pragma once
#include "common.hpp"
#include "../../include/perf_hip_meshtex.h"

namespace perf {

constexpr int kTexEdge = 16;                 // a workgroup covers 16 x 16 texels: four waves, an 8 x 8 block each
constexpr int kTexGroup = kTexEdge * kTexEdge;
static_assert(kTexGroup == 4 * kWave, "one 8 x 8 block of texels per wave");

// the texel of a thread: lane l of wave w sits at (l & 7, l >> 3) of the wave's block, the four blocks tile the workgroup's 16 x 16
__device__ __forceinline__ void tex_thread_texel(int32_t& col, int32_t& row) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    col = (int32_t)blockIdx.x * kTexEdge + (wave & 1) * 8 + (lane & 7);
    row = (int32_t)blockIdx.y * kTexEdge + (wave >> 1) * 8 + (lane >> 3);
}

struct TexOwner {
    int64_t face;          // -1: the texel belongs to no face of the mesh
    int32_t li, lj;        // the local index, mirrored for half 1
    int32_t code;          // PERF_MESHTEX_COVER_*
};

// which face owns texel (col, row) of an atlas of edge size cut into tiles of edge tile, by the layout alone (the face's indices are not read)
__device__ __forceinline__ TexOwner tex_owner(int32_t col, int32_t row, int32_t size, int32_t tile, int64_t n_faces) {
    TexOwner o{-1, 0, 0, PERF_MESHTEX_COVER_NONE};
    const int32_t n = size / tile;
    const int32_t tx = col / tile, ty = row / tile;
    if (tx >= n || ty >= n) return o;          // the margin
    const int32_t i = col - tx * tile, j = row - ty * tile;
    const int32_t h = (i + j >= tile) ? 1 : 0;
    const int64_t f = 2 * ((int64_t)ty * n + tx) + h;
    if (f >= n_faces) return o;
    o.face = f;
    o.li = h ? tile - 1 - i : i;
    o.lj = h ? tile - 1 - j : j;
    o.code = (o.li + o.lj <= tile - 3) ? PERF_MESHTEX_COVER_INSIDE : PERF_MESHTEX_COVER_GUTTER;
    return o;
}

// the three indices of a face, and whether all lie in [0, V)
__device__ __forceinline__ bool tex_face(const int32_t* __restrict__ faces, int64_t f, int64_t n_vertices, int64_t abc[3]) {
    abc[0] = faces[3 * f]; abc[1] = faces[3 * f + 1]; abc[2] = faces[3 * f + 2];
    return abc[0] >= 0 && abc[0] < n_vertices && abc[1] >= 0 && abc[1] < n_vertices && abc[2] >= 0 && abc[2] < n_vertices;
}

struct TexBary {
    double alpha, beta, gamma;
};

__device__ __forceinline__ TexBary tex_bary(const TexOwner& o, int32_t tile) {
#pragma clang fp contract(off)
    const double m = (double)(tile - 3);
    TexBary b;
    b.beta = (double)o.li / m;
    b.gamma = (double)o.lj / m;
    b.alpha = (1.0 - b.beta) - b.gamma;
    return b;
}

// P = (a + beta (b - a)) + gamma (c - a) per component in double, rounded to fp32 once
__device__ __forceinline__ void tex_point(const float* __restrict__ vertices, const int64_t abc[3], const TexBary& w, float p[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double a = vertices[3 * abc[0] + k], b = vertices[3 * abc[1] + k], c = vertices[3 * abc[2] + k];
        p[k] = (float)((a + w.beta * (b - a)) + w.gamma * (c - a));
    }
}

// (alpha Ra + beta Rb) + gamma Rc per component in double over per-vertex rows fp32 [V, 3], rounded once: the normals and the fallback
__device__ __forceinline__ void tex_rows(const float* __restrict__ rows, const int64_t abc[3], const TexBary& w, float r[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double a = rows[3 * abc[0] + k], b = rows[3 * abc[1] + k], c = rows[3 * abc[2] + k];
        r[k] = (float)((w.alpha * a + w.beta * b) + w.gamma * c);
    }
}

// the face's own unit normal: e1 x e2 in double, divided by its length, exactly 0 where the length is 0
__device__ __forceinline__ void tex_flat_normal(const float* __restrict__ vertices, const int64_t abc[3], float n[3]) {
#pragma clang fp contract(off)
    const double ax = vertices[3 * abc[0]], ay = vertices[3 * abc[0] + 1], az = vertices[3 * abc[0] + 2];
    const double e1x = (double)vertices[3 * abc[1]] - ax, e1y = (double)vertices[3 * abc[1] + 1] - ay, e1z = (double)vertices[3 * abc[1] + 2] - az;
    const double e2x = (double)vertices[3 * abc[2]] - ax, e2y = (double)vertices[3 * abc[2] + 1] - ay, e2z = (double)vertices[3 * abc[2] + 2] - az;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    const bool none = len == 0.0;
    n[0] = none ? 0.0f : (float)(nx / len);
    n[1] = none ? 0.0f : (float)(ny / len);
    n[2] = none ? 0.0f : (float)(nz / len);
}

// the texel's normal: interpolated from per-vertex normals when they are given, the face's own otherwise
__device__ __forceinline__ void tex_normal(const float* __restrict__ vertices, const float* __restrict__ normals, const int64_t abc[3], const TexBary& w, float n[3]) {
    if (normals) tex_rows(normals, abc, w, n);
    else tex_flat_normal(vertices, abc, n);
}

// ---- the layout's host check: every entry point of the atlas begins with it ----------------------------------------------------------------
static int tex_layout_check(const char* who, int64_t n_faces, int32_t size, int32_t tile) {
    PERF_REQUIRE(n_faces >= 0, "%s: a negative number of faces (%lld)", who, (long long)n_faces);
    PERF_REQUIRE(size >= PERF_MESHTEX_MIN_SIZE && size <= PERF_MESHTEX_MAX_SIZE, "%s: an atlas size of %d is outside 64 .. 16384", who, size);
    PERF_REQUIRE(tile >= PERF_MESHTEX_MIN_TILE, "%s: a tile of %d texels is below 4", who, tile);
    PERF_REQUIRE(tile <= size, "%s: a tile of %d texels is larger than the atlas (%d)", who, tile, size);
    const int64_t n = size / tile;
    PERF_REQUIRE(n_faces <= 2 * n * n, "%s: %lld faces are more than the %lld an atlas of %d with tiles of %d holds (2 n^2, n = %lld)", who, (long long)n_faces,
                 (long long)(2 * n * n), size, tile, (long long)n);
    return PERF_OK;
}

static inline dim3 tex_grid(int32_t size) { return dim3((unsigned)div_up(size, kTexEdge), (unsigned)div_up(size, kTexEdge)); }

}  // namespace perf
