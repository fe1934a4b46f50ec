// Colour a mesh's vertices from the registered panoramas and build vertex normals from its faces (include/perf_hip_meshcolor.h):
// normal sums (int64 atomics) -> unit normals; the blend (one launch for all views).  The pixel of the blend's look-up is
// pano_lookup_device.hpp's, the one the cull (meshvis.hip) runs; this unit keeps the taps and the weights the cull throws away.  The fused
// texture bake of include/perf_hip_meshtex.h lives here too: it runs the blend's per-point function on the texels of meshtex_device.hpp.
#include "common.hpp"
#include "mesh_check_host.hpp"
#include "pano_lookup_device.hpp"
#include "meshtex_device.hpp"
#include "../../include/perf_hip_meshcolor.h"
#include "../../include/perf_hip_meshtex.h"

namespace perf {

constexpr int kColGroup = 256;               // items of one workgroup: one per thread
constexpr int kColViewWords = sizeof(perf_meshvis_view) / 4;
static_assert(sizeof(perf_meshvis_view) == 64 && alignof(perf_meshvis_view) == 8, "the view descriptor is 64 bytes");
static_assert(PERF_MESHCOLOR_MAX_VIEWS == PERF_MESHVIS_MAX_VIEWS, "a vertex has one bit per view in a 64-bit word");

// ---- stage A ----------------------------------------------------------------------------------------------------------------------------
// scale = 2^s, exact; a face whose scaled normal is not finite or reaches 2^62 contributes nothing
__global__ void __launch_bounds__(kColGroup) meshcolor_normal_sums_kernel(const float* __restrict__ vertices, int64_t n_vertices, const int32_t* __restrict__ faces,
                                                                          int64_t n_faces, double scale, unsigned long long* __restrict__ acc,
                                                                          unsigned long long* __restrict__ first_bad) {
#pragma clang fp contract(off)
    const int64_t f = (int64_t)blockIdx.x * kColGroup + threadIdx.x;
    if (f >= n_faces) return;
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (!(a >= 0 && a < n_vertices && b >= 0 && b < n_vertices && c >= 0 && c < n_vertices)) {
        atomicMin(first_bad, (unsigned long long)f);
        return;
    }
    const double ax = vertices[3 * (int64_t)a], ay = vertices[3 * (int64_t)a + 1], az = vertices[3 * (int64_t)a + 2];
    const double e1x = (double)vertices[3 * (int64_t)b] - ax, e1y = (double)vertices[3 * (int64_t)b + 1] - ay, e1z = (double)vertices[3 * (int64_t)b + 2] - az;
    const double e2x = (double)vertices[3 * (int64_t)c] - ax, e2y = (double)vertices[3 * (int64_t)c + 1] - ay, e2z = (double)vertices[3 * (int64_t)c + 2] - az;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double sx = nx * scale, sy = ny * scale, sz = nz * scale;
    const double kTop = 4611686018427387904.0;          // 2^62
    if (!(fabs(sx) < kTop && fabs(sy) < kTop && fabs(sz) < kTop)) return;          // (a NaN fails every comparison)
    const long long q[3] = {llrint(sx), llrint(sy), llrint(sz)};
    const int32_t abc[3] = {a, b, c};
#pragma unroll
    for (int v = 0; v < 3; ++v)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (q[k] != 0) atomicAdd(acc + 3 * (int64_t)abc[v] + k, (unsigned long long)q[k]);          // (two's complement: the signed sum)
}

__global__ void __launch_bounds__(kColGroup) meshcolor_normals_kernel(const long long* __restrict__ acc, int64_t n_vertices, float* __restrict__ normals) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kColGroup + threadIdx.x;
    if (i >= n_vertices) return;
    const double ax = (double)acc[3 * i], ay = (double)acc[3 * i + 1], az = (double)acc[3 * i + 2];
    const double len = sqrt((ax * ax + ay * ay) + az * az);
    const bool none = len == 0.0;
    normals[3 * i] = none ? 0.0f : (float)(ax / len);
    normals[3 * i + 1] = none ? 0.0f : (float)(ay / len);
    normals[3 * i + 2] = none ? 0.0f : (float)(az / len);
}

// ---- stage B ----------------------------------------------------------------------------------------------------------------------------
// what the look-up of one point in one view leaves: the four taps (element offsets y * w + x, -1 where the index test fails) and their weights
struct ColTaps {
    int64_t at[4];          // nw, ne, sw, se
    float w[4];
};

// dist and proj of one point in one view: the pixel is pano_lookup_device.hpp's; the taps of pano_tap are kept for the colour maps
__device__ __forceinline__ void col_lookup(float x, float y, float z, const perf_meshvis_view& pf, float& dist_out, float& proj_out, ColTaps& taps) {
    const int32_t h = pf.height, w = pf.width;
    const PanoPixel p = pano_pixel(x, y, z, pf.rt, pf.t, h, w);
    const float dist = p.dist;
    const float* __restrict__ dmap = pf.distance_map;
    auto where = [&](int yy, int xx) { return (yy >= 0 && yy < h && xx >= 0 && xx < w) ? (int64_t)yy * w + xx : (int64_t)-1; };
    taps.at[0] = where(p.y0, p.x0); taps.at[1] = where(p.y0, p.x1); taps.at[2] = where(p.y1, p.x0); taps.at[3] = where(p.y1, p.x1);
    taps.w[0] = mul_rn(p.wx0, p.wy0); taps.w[1] = mul_rn(p.wx1, p.wy0); taps.w[2] = mul_rn(p.wx0, p.wy1); taps.w[3] = mul_rn(p.wx1, p.wy1);
    auto at = [&](int t) { return taps.at[t] >= 0 ? dmap[taps.at[t]] : 0.0f; };
    float proj = mul_rn(at(0), taps.w[0]);
    proj = add_rn(proj, mul_rn(at(1), taps.w[1]));
    proj = add_rn(proj, mul_rn(at(2), taps.w[2]));
    proj = add_rn(proj, mul_rn(at(3), taps.w[3]));
    dist_out = dist;
    proj_out = proj;
}

// the same four-tap accumulation over one channel of a colour map [H, W, 3]
__device__ __forceinline__ float col_sample(const float* __restrict__ cmap, const ColTaps& taps, int channel) {
    auto at = [&](int t) { return taps.at[t] >= 0 ? cmap[3 * taps.at[t] + channel] : 0.0f; };
    float c = mul_rn(at(0), taps.w[0]);
    c = add_rn(c, mul_rn(at(1), taps.w[1]));
    c = add_rn(c, mul_rn(at(2), taps.w[2]));
    c = add_rn(c, mul_rn(at(3), taps.w[3]));
    return c;
}

// Stage B for one point, from the loop over the views to the four outputs: the point (x, y, z), its normal (read only with facing), the views
// and the colour maps (staged in LDS by the caller) -> the colour, the weight, the bits and the best view.  none(k) is channel k of the
// colour where no view passes; it is evaluated only then.  Both kernels of this unit run it: a vertex of the blend and a texel of the bake
// with the same fp32 point and normal get the same bits.
template <class None>
__device__ __forceinline__ void col_blend_point(float x, float y, float z, float nx, float ny, float nz, const perf_meshvis_view* view, const float* const* cmap,
                                                int32_t n_views, float tol, int32_t facing, int32_t power, int32_t select, None&& none, float out[3], float& wt,
                                                unsigned long long& used_out, int& best_out) {
#pragma clang fp contract(off)
    const double Nx = nx, Ny = ny, Nz = nz;
    const double nlen = sqrt((Nx * Nx + Ny * Ny) + Nz * Nz);
    unsigned long long used = 0;
    double num[3] = {0.0, 0.0, 0.0}, den = 0.0, best_w = 0.0;
    float best_c[3] = {0.0f, 0.0f, 0.0f};
    int best_k = -1;
    for (int k = 0; k < n_views; ++k) {
        float dist, proj;
        ColTaps taps;
        col_lookup(x, y, z, view[k], dist, proj, taps);
        if (!(dist < add_rn(proj, tol))) continue;
        if (!(dist > 0.0f && dist <= 3.4028234663852886e38f)) continue;
        const double d2 = (double)dist * (double)dist;
        double w = 1.0 / d2;
        if (facing) {
            const double gx = (double)view[k].t[0] - (double)x, gy = (double)view[k].t[1] - (double)y, gz = (double)view[k].t[2] - (double)z;
            const double s = (Nx * gx + Ny * gy) + Nz * gz;
            if (!(s > 0.0)) continue;
            const double c = s / (nlen * sqrt((gx * gx + gy * gy) + gz * gz));
            double cp = c;
            for (int e = 1; e < power; ++e) cp = cp * c;
            w = cp / d2;
        }
        if (!(w > 0.0)) continue;
        used |= 1ull << k;
        const float* __restrict__ m = cmap[k];
        const float c0 = col_sample(m, taps, 0), c1 = col_sample(m, taps, 1), c2 = col_sample(m, taps, 2);
        if (select == PERF_MESHCOLOR_SELECT_BEST) {
            if (best_k < 0 || w > best_w) { best_k = k; best_w = w; best_c[0] = c0; best_c[1] = c1; best_c[2] = c2; }
        } else {
            num[0] = num[0] + w * (double)c0; num[1] = num[1] + w * (double)c1; num[2] = num[2] + w * (double)c2;
            den = den + w;
        }
    }
    wt = 0.0f;
    if (used == 0) {
        out[0] = none(0); out[1] = none(1); out[2] = none(2);
    } else if (select == PERF_MESHCOLOR_SELECT_BEST) {
        out[0] = best_c[0]; out[1] = best_c[1]; out[2] = best_c[2];
        wt = (float)best_w;
    } else {
        out[0] = (float)(num[0] / den); out[1] = (float)(num[1] / den); out[2] = (float)(num[2] / den);
        wt = (float)den;
    }
    used_out = used;
    best_out = best_k;
}

// A workgroup stages its 256 vertices (and, with facing, their normals), the views' descriptors and the colour maps' pointers in LDS; a
// thread then loops over the views.  All 256 threads arrive at the barrier.  (The bound of seven waves per SIMD keeps the 72
// VGPRs the kernel had with its per-point body written in place; without it the inlined function takes 74 and one wave less.)
__global__ void __launch_bounds__(kColGroup, 7) meshcolor_blend_kernel(const float* __restrict__ vertices, const float* __restrict__ normals, int64_t n_vertices,
                                                                    const perf_meshvis_view* __restrict__ views, const float* const* __restrict__ color_maps,
                                                                    int32_t n_views, float tol, int32_t facing, int32_t power, int32_t select,
                                                                    const float* __restrict__ fallback, float fill_r, float fill_g, float fill_b,
                                                                    float* __restrict__ colors, float* __restrict__ weight, unsigned long long* __restrict__ used_bits,
                                                                    int8_t* __restrict__ best_view) {
#pragma clang fp contract(off)
    __shared__ perf_meshvis_view view[PERF_MESHCOLOR_MAX_VIEWS];
    __shared__ const float* cmap[PERF_MESHCOLOR_MAX_VIEWS];
    __shared__ float xyz[3 * kColGroup];
    __shared__ float nrm[3 * kColGroup];
    const int64_t first = (int64_t)blockIdx.x * kColGroup;
    const uint32_t* __restrict__ words = reinterpret_cast<const uint32_t*>(views);
    uint32_t* staged = reinterpret_cast<uint32_t*>(view);
    for (int k = threadIdx.x; k < n_views * kColViewWords; k += kColGroup) staged[k] = words[k];
    for (int k = threadIdx.x; k < n_views; k += kColGroup) cmap[k] = color_maps[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t at = 3 * first + k * kColGroup + threadIdx.x;
        xyz[k * kColGroup + threadIdx.x] = at < 3 * n_vertices ? vertices[at] : 0.0f;
        nrm[k * kColGroup + threadIdx.x] = facing && at < 3 * n_vertices ? normals[at] : 0.0f;
    }
    __syncthreads();
    const int64_t i = first + threadIdx.x;
    if (i >= n_vertices) return;
    const float x = xyz[3 * threadIdx.x], y = xyz[3 * threadIdx.x + 1], z = xyz[3 * threadIdx.x + 2];
    float out[3], wt;
    unsigned long long used;
    int best_k;
    col_blend_point(x, y, z, nrm[3 * threadIdx.x], nrm[3 * threadIdx.x + 1], nrm[3 * threadIdx.x + 2], view, cmap, n_views, tol, facing, power, select,
                    [&](int k) { return fallback ? fallback[3 * i + k] : k == 0 ? fill_r : k == 1 ? fill_g : fill_b; }, out, wt, used, best_k);
    colors[3 * i] = out[0]; colors[3 * i + 1] = out[1]; colors[3 * i + 2] = out[2];
    weight[i] = wt;
    used_bits[i] = used;
    best_view[i] = (int8_t)best_k;
}

// ---- the fused bake of include/perf_hip_meshtex.h ------------------------------------------------------------------------------------------
// One thread per texel, an 8 x 8 block of texels per wave (at T = 8 a wave reads two faces).  The texel's point and normal are
// meshtex_device.hpp's, rounded to fp32 as perf_meshtex_points stores them, and go through col_blend_point as a vertex of the blend does.
// All 256 threads arrive at the barrier; nothing else waits on another thread.
__global__ void __launch_bounds__(kTexGroup) meshtex_bake_kernel(const float* __restrict__ vertices, int64_t n_vertices, const float* __restrict__ normals,
                                                                 const int32_t* __restrict__ faces, int64_t n_faces, int32_t size, int32_t tile,
                                                                 const perf_meshvis_view* __restrict__ views, const float* const* __restrict__ color_maps,
                                                                 int32_t n_views, float tol, int32_t facing, int32_t power, int32_t select,
                                                                 const float* __restrict__ fallback, float fill_r, float fill_g, float fill_b,
                                                                 float* __restrict__ image, float* __restrict__ weight, unsigned long long* __restrict__ used_bits,
                                                                 uint8_t* __restrict__ coverage, unsigned long long* __restrict__ first_bad) {
#pragma clang fp contract(off)
    __shared__ perf_meshvis_view view[PERF_MESHCOLOR_MAX_VIEWS];
    __shared__ const float* cmap[PERF_MESHCOLOR_MAX_VIEWS];
    const uint32_t* __restrict__ words = reinterpret_cast<const uint32_t*>(views);
    uint32_t* staged = reinterpret_cast<uint32_t*>(view);
    for (int k = threadIdx.x; k < n_views * kColViewWords; k += kTexGroup) staged[k] = words[k];
    for (int k = threadIdx.x; k < n_views; k += kTexGroup) cmap[k] = color_maps[k];
    __syncthreads();
    int32_t col, row;
    tex_thread_texel(col, row);
    if (col >= size || row >= size) return;
    const int64_t at = (int64_t)row * size + col;
    TexOwner o = tex_owner(col, row, size, tile, n_faces);
    int64_t abc[3];
    if (o.face >= 0 && !tex_face(faces, o.face, n_vertices, abc)) {
        if (o.li == 0 && o.lj == 0) atomicMin(first_bad, (unsigned long long)o.face);          // (corner a: one texel per face)
        o.face = -1;
    }
    if (o.face < 0) {
        image[3 * at] = fill_r; image[3 * at + 1] = fill_g; image[3 * at + 2] = fill_b;
        weight[at] = 0.0f;
        used_bits[at] = 0;
        coverage[at] = PERF_MESHTEX_COVER_NONE;
        return;
    }
    const TexBary w = tex_bary(o, tile);
    float p[3], nrm[3] = {0.0f, 0.0f, 0.0f};
    tex_point(vertices, abc, w, p);
    if (facing) tex_normal(vertices, normals, abc, w, nrm);
    float out[3], wt;
    unsigned long long used;
    int best_k;
    col_blend_point(p[0], p[1], p[2], nrm[0], nrm[1], nrm[2], view, cmap, n_views, tol, facing, power, select,
                    [&](int k) {
                        if (!fallback) return k == 0 ? fill_r : k == 1 ? fill_g : fill_b;
                        float rows[3];
                        tex_rows(fallback, abc, w, rows);
                        return rows[k];
                    },
                    out, wt, used, best_k);
    image[3 * at] = out[0]; image[3 * at + 1] = out[1]; image[3 * at + 2] = out[2];
    weight[at] = wt;
    used_bits[at] = used;
    coverage[at] = (uint8_t)o.code;
}

// ---- the checks of the entry points -------------------------------------------------------------------------------------------------------
static int col_counts_check(const char* who, int64_t n_vertices, int64_t n_faces) {
    return mesh_counts_check(who, n_vertices, n_faces, PERF_MESHCOLOR_MAX_VERTICES, PERF_MESHCOLOR_MAX_FACES, "2^31 - 1");
}

static inline unsigned col_groups(int64_t n) { return (unsigned)div_up(n, kColGroup); }

}  // namespace perf

using namespace perf;

extern "C" int perf_meshcolor_version(void) { return PERF_MESHCOLOR_ABI_VERSION; }

extern "C" int perf_meshcolor_normal_sums(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t scale_log2,
                                          int64_t* acc, int64_t* bad_face_dev, void* stream) {
    if (int rc = col_counts_check("perf_meshcolor_normal_sums", n_vertices, n_faces)) return rc;
    PERF_REQUIRE(scale_log2 >= -200 && scale_log2 <= 200, "perf_meshcolor_normal_sums: scale_log2 %d is outside -200 .. 200", scale_log2);
    PERF_REQUIRE(vertices || n_vertices == 0, "perf_meshcolor_normal_sums: NULL input (vertices) with vertices to sum at");
    PERF_REQUIRE(faces || n_faces == 0, "perf_meshcolor_normal_sums: NULL input (faces) with faces to sum");
    PERF_REQUIRE(acc || n_vertices == 0, "perf_meshcolor_normal_sums: NULL output (acc) with vertices to sum at");
    PERF_REQUIRE(bad_face_dev, "perf_meshcolor_normal_sums: NULL output (bad_face_dev)");
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(bad_face_dev, 0xff, sizeof(int64_t), st) != hipSuccess ||          // the flag: no bad face (-1, the largest unsigned)
        (n_vertices > 0 && hipMemsetAsync(acc, 0, (size_t)n_vertices * 3 * sizeof(int64_t), st) != hipSuccess)) {
        (void)hipGetLastError();
        set_error("perf_meshcolor_normal_sums: clearing the sums and the flag failed");
        return PERF_E_LAUNCH;
    }
    if (n_faces > 0)
        hipLaunchKernelGGL(meshcolor_normal_sums_kernel, dim3(col_groups(n_faces)), dim3(kColGroup), 0, st, vertices, n_vertices, faces, n_faces, ldexp(1.0, scale_log2),
                           (unsigned long long*)acc, (unsigned long long*)bad_face_dev);
    PERF_LAUNCH_CHECK("perf_meshcolor_normal_sums");
    return PERF_OK;
}

extern "C" int perf_meshcolor_normals(const int64_t* acc, int64_t n_vertices, float* normals, void* stream) {
    if (int rc = col_counts_check("perf_meshcolor_normals", n_vertices, 0)) return rc;
    PERF_REQUIRE(acc || n_vertices == 0, "perf_meshcolor_normals: NULL input (acc) with vertices");
    PERF_REQUIRE(normals || n_vertices == 0, "perf_meshcolor_normals: NULL output (normals) with vertices");
    if (n_vertices == 0) return PERF_OK;
    hipLaunchKernelGGL(meshcolor_normals_kernel, dim3(col_groups(n_vertices)), dim3(kColGroup), 0, as_stream(stream), (const long long*)acc, n_vertices, normals);
    PERF_LAUNCH_CHECK("perf_meshcolor_normals");
    return PERF_OK;
}

extern "C" int perf_meshcolor_blend(const float* vertices, const float* normals, int64_t n_vertices, const perf_meshvis_view* views_dev,
                                    const float* const* color_maps_dev, const int32_t* view_sizes, int32_t n_views, float tol, int32_t facing,
                                    int32_t power, int32_t select, const float* fallback, const float* fill, float* colors, float* weight,
                                    int64_t* used_bits, int8_t* best_view, void* stream) {
    const char* who = "perf_meshcolor_blend";
    if (int rc = col_counts_check(who, n_vertices, 0)) return rc;
    PERF_REQUIRE(n_views >= 0, "%s: a negative number of views (%d)", who, n_views);
    PERF_REQUIRE(n_views <= PERF_MESHCOLOR_MAX_VIEWS, "%s: %d views are more than 64 (a vertex has one bit per view in a 64-bit word)", who, n_views);
    PERF_REQUIRE(tol >= 0.0f && tol <= 3.0e38f, "%s: tol %g is negative or not finite", who, (double)tol);
    PERF_REQUIRE(facing == 0 || facing == 1, "%s: facing (%d) is 0 or 1", who, facing);
    PERF_REQUIRE(!facing || (power >= 1 && power <= PERF_MESHCOLOR_MAX_POWER), "%s: power %d is outside 1 .. 8", who, power);
    PERF_REQUIRE(select == PERF_MESHCOLOR_SELECT_BLEND || select == PERF_MESHCOLOR_SELECT_BEST, "%s: select %d is neither blend (0) nor best (1)", who, select);
    PERF_REQUIRE(vertices || n_vertices == 0, "%s: NULL input (vertices) with vertices to colour", who);
    PERF_REQUIRE(normals || !facing || n_vertices == 0, "%s: NULL input (normals) with facing", who);
    PERF_REQUIRE((views_dev && color_maps_dev && view_sizes) || n_views == 0, "%s: NULL input (views_dev, color_maps_dev or view_sizes) with views to colour from", who);
    PERF_REQUIRE((reinterpret_cast<uintptr_t>(views_dev) & 7) == 0 && (reinterpret_cast<uintptr_t>(color_maps_dev) & 7) == 0,
                 "%s: views_dev and color_maps_dev must be 8-byte aligned", who);
    PERF_REQUIRE(fill, "%s: NULL input (fill)", who);
    PERF_REQUIRE((colors && weight && used_bits && best_view) || n_vertices == 0, "%s: NULL output (colors, weight, used_bits or best_view) with vertices to colour", who);
    for (int k = 0; k < n_views; ++k)
        PERF_REQUIRE(view_sizes[2 * k] >= 1 && view_sizes[2 * k + 1] >= 1, "%s: view %d has a map of %d x %d: a map dimension below 1", who, k, view_sizes[2 * k],
                     view_sizes[2 * k + 1]);
    if (n_vertices == 0) return PERF_OK;
    hipLaunchKernelGGL(meshcolor_blend_kernel, dim3(col_groups(n_vertices)), dim3(kColGroup), 0, as_stream(stream), vertices, normals, n_vertices, views_dev,
                       color_maps_dev, n_views, tol, facing, power, select, fallback, fill[0], fill[1], fill[2], colors, weight, (unsigned long long*)used_bits,
                       best_view);
    PERF_LAUNCH_CHECK(who);
    return PERF_OK;
}

static_assert(PERF_MESHTEX_MAX_VIEWS == PERF_MESHCOLOR_MAX_VIEWS && PERF_MESHTEX_MAX_POWER == PERF_MESHCOLOR_MAX_POWER, "the bake is the blend on texels");

extern "C" int perf_meshtex_bake(const float* vertices, int64_t n_vertices, const float* normals, const int32_t* faces, int64_t n_faces, int32_t size,
                                 int32_t tile, const void* views_dev, const float* const* color_maps_dev, const int32_t* view_sizes, int32_t n_views,
                                 float tol, int32_t facing, int32_t power, int32_t select, const float* fallback, const float* fill, float* image,
                                 float* weight, int64_t* used_bits, uint8_t* coverage, int64_t* bad_face_dev, void* stream) {
    const char* who = "perf_meshtex_bake";
    if (int rc = tex_layout_check(who, n_faces, size, tile)) return rc;
    if (int rc = col_counts_check(who, n_vertices, 0)) return rc;
    PERF_REQUIRE(n_views >= 0, "%s: a negative number of views (%d)", who, n_views);
    PERF_REQUIRE(n_views <= PERF_MESHTEX_MAX_VIEWS, "%s: %d views are more than 64 (a texel has one bit per view in a 64-bit word)", who, n_views);
    PERF_REQUIRE(tol >= 0.0f && tol <= 3.0e38f, "%s: tol %g is negative or not finite", who, (double)tol);
    PERF_REQUIRE(facing == 0 || facing == 1, "%s: facing (%d) is 0 or 1", who, facing);
    PERF_REQUIRE(!facing || (power >= 1 && power <= PERF_MESHTEX_MAX_POWER), "%s: power %d is outside 1 .. 8", who, power);
    PERF_REQUIRE(select == PERF_MESHCOLOR_SELECT_BLEND || select == PERF_MESHCOLOR_SELECT_BEST, "%s: select %d is neither blend (0) nor best (1)", who, select);
    PERF_REQUIRE(vertices || n_vertices == 0, "%s: NULL input (vertices) with vertices", who);
    PERF_REQUIRE(faces || n_faces == 0, "%s: NULL input (faces) with faces to bake", who);
    PERF_REQUIRE((views_dev && color_maps_dev && view_sizes) || n_views == 0, "%s: NULL input (views_dev, color_maps_dev or view_sizes) with views to bake from", who);
    PERF_REQUIRE((reinterpret_cast<uintptr_t>(views_dev) & 7) == 0 && (reinterpret_cast<uintptr_t>(color_maps_dev) & 7) == 0,
                 "%s: views_dev and color_maps_dev must be 8-byte aligned", who);
    PERF_REQUIRE(fill, "%s: NULL input (fill)", who);
    PERF_REQUIRE(image && weight && used_bits && coverage, "%s: NULL output (image, weight, used_bits or coverage)", who);
    PERF_REQUIRE(bad_face_dev, "%s: NULL output (bad_face_dev)", who);
    for (int k = 0; k < n_views; ++k)
        PERF_REQUIRE(view_sizes[2 * k] >= 1 && view_sizes[2 * k + 1] >= 1, "%s: view %d has a map of %d x %d: a map dimension below 1", who, k, view_sizes[2 * k],
                     view_sizes[2 * k + 1]);
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(bad_face_dev, 0xff, sizeof(int64_t), st) != hipSuccess) {          // the flag: no bad face (-1, the largest unsigned)
        (void)hipGetLastError();
        set_error("%s: clearing the flag failed", who);
        return PERF_E_LAUNCH;
    }
    hipLaunchKernelGGL(meshtex_bake_kernel, tex_grid(size), dim3(kTexGroup), 0, st, vertices, n_vertices, normals, faces, n_faces, size, tile,
                       static_cast<const perf_meshvis_view*>(views_dev), color_maps_dev, n_views, tol, facing, power, select, fallback, fill[0], fill[1], fill[2], image,
                       weight, (unsigned long long*)used_bits, coverage, (unsigned long long*)bad_face_dev);
    PERF_LAUNCH_CHECK(who);
    return PERF_OK;
}
