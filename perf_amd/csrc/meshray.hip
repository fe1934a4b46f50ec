// Rays against a triangle mesh on a uniform grid (include/perf_hip_meshray.h): the grid by count -> scan -> write (integer atomics only),
// the closest hit and the any hit of a batch of rays, the occlusion of the segments from the vertices to the views' centres.  The rule of
// one face is the header's, line for line, in double; the grid only decides which faces are tested.
#include "common.hpp"
#include "mesh_check_host.hpp"
#include "../../include/perf_hip_meshray.h"
#include <math.h>

namespace perf {

constexpr int kRayGroup = 256;               // items of one workgroup: one per thread
constexpr float kRayFltMax = 3.4028234663852886e38f;

struct RayGrid {                             // the caller's box, widened to double on the host
    double origin[3];
    double cell, margin;                     // margin = cell / 8, exact
    int32_t dims[3];
    int64_t n_cells;
};

__device__ __forceinline__ bool ray_finite(float x) { return fabsf(x) <= kRayFltMax; }          // (false on a NaN)

// ---- the grid ---------------------------------------------------------------------------------------------------------------------------
// The clamped cell range of face f -> true when it is listed somewhere.  bad: an index outside [0, V) or a vertex that is not finite.
__device__ __forceinline__ bool ray_face_range(const RayGrid& g, const float* __restrict__ vertices, int64_t n_vertices, const int32_t* __restrict__ faces, int64_t f,
                                               int lo[3], int hi[3], bool& bad) {
#pragma clang fp contract(off)
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    bad = !(a >= 0 && a < n_vertices && b >= 0 && b < n_vertices && c >= 0 && c < n_vertices);
    if (bad) return false;
    bool listed = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float xa = vertices[3 * (int64_t)a + k], xb = vertices[3 * (int64_t)b + k], xc = vertices[3 * (int64_t)c + k];
        if (!(ray_finite(xa) && ray_finite(xb) && ray_finite(xc))) bad = true;
        const double mn = fmin(fmin((double)xa, (double)xb), (double)xc), mx = fmax(fmax((double)xa, (double)xb), (double)xc);
        const double first = floor(((mn - g.margin) - g.origin[k]) / g.cell), last = floor(((mx + g.margin) - g.origin[k]) / g.cell);
        const double top = (double)(g.dims[k] - 1);
        if (!(last >= 0.0 && first <= top)) listed = false;          // (wholly outside the box; a NaN fails both)
        lo[k] = (int)fmin(fmax(first, 0.0), top);                    // (both ends clamped in double before the conversion; fmax / fmin drop a NaN)
        hi[k] = (int)fmin(fmax(last, 0.0), top);
    }
    return listed && !bad;
}

__global__ void __launch_bounds__(kRayGroup) meshray_grid_count_kernel(RayGrid g, const float* __restrict__ vertices, int64_t n_vertices, const int32_t* __restrict__ faces,
                                                                       int64_t n_faces, int32_t* __restrict__ counts, unsigned long long* __restrict__ first_bad) {
    const int64_t f = (int64_t)blockIdx.x * kRayGroup + threadIdx.x;
    if (f >= n_faces) return;
    int lo[3], hi[3];
    bool bad;
    const bool listed = ray_face_range(g, vertices, n_vertices, faces, f, lo, hi, bad);
    if (bad) atomicMin(first_bad, (unsigned long long)f);
    if (!listed) return;
    // lo and hi are clamped to [0, dims - 1]: every cell index below is inside the counts.  One thread walks all cells of its face: a face
    // as large as the box costs one lane as many atomics as the grid has cells (2^24 at the most) -- bounded, and slow only for such a face
    for (int i = lo[0]; i <= hi[0]; ++i)
        for (int j = lo[1]; j <= hi[1]; ++j)
            for (int k = lo[2]; k <= hi[2]; ++k) atomicAdd(counts + ((int64_t)i * g.dims[1] + j) * g.dims[2] + k, 1);
}

// The counts are the cursors: a reference takes the slot offsets[c] + (the count before the decrement) - 1 and leaves the count one lower.
__global__ void __launch_bounds__(kRayGroup) meshray_grid_write_kernel(RayGrid g, const float* __restrict__ vertices, int64_t n_vertices, const int32_t* __restrict__ faces,
                                                                       int64_t n_faces, int32_t* __restrict__ counts, const int32_t* __restrict__ offsets,
                                                                       int32_t* __restrict__ refs, int64_t ref_capacity) {
    const int64_t f = (int64_t)blockIdx.x * kRayGroup + threadIdx.x;
    if (f >= n_faces) return;
    int lo[3], hi[3];
    bool bad;
    if (!ray_face_range(g, vertices, n_vertices, faces, f, lo, hi, bad)) return;
    for (int i = lo[0]; i <= hi[0]; ++i)
        for (int j = lo[1]; j <= hi[1]; ++j)
            for (int k = lo[2]; k <= hi[2]; ++k) {
                const int64_t c = ((int64_t)i * g.dims[1] + j) * g.dims[2] + k;
                const int32_t rank = atomicSub(counts + c, 1) - 1;
                const int64_t slot = (int64_t)offsets[c] + rank;
                if (rank >= 0 && slot >= 0 && slot < ref_capacity) refs[slot] = (int32_t)f;          // (never outside refs, whatever counts and offsets hold)
            }
}

// ---- the rule ---------------------------------------------------------------------------------------------------------------------------
struct RayHit {
    double t, u, v;
    int32_t face;                            // -1: none
};

// the header's lines in its order; kStrict: t_lo < t < t_hi (the segment test), else t_lo <= t <= t_hi
template <bool kStrict>
__device__ __forceinline__ bool ray_rule(const double o[3], const double d[3], const float* __restrict__ vertices, int32_t ia, int32_t ib, int32_t ic, double t_lo,
                                         double t_hi, double& t, double& u, double& v) {
#pragma clang fp contract(off)
    const float* __restrict__ pa = vertices + 3 * (int64_t)ia;
    const float* __restrict__ pb = vertices + 3 * (int64_t)ib;
    const float* __restrict__ pc = vertices + 3 * (int64_t)ic;
    const double ax = pa[0], ay = pa[1], az = pa[2];
    const double e1x = (double)pb[0] - ax, e1y = (double)pb[1] - ay, e1z = (double)pb[2] - az;
    const double e2x = (double)pc[0] - ax, e2y = (double)pc[1] - ay, e2z = (double)pc[2] - az;
    const double px = d[1] * e2z - d[2] * e2y, py = d[2] * e2x - d[0] * e2z, pz = d[0] * e2y - d[1] * e2x;
    const double det = (e1x * px + e1y * py) + e1z * pz;
    if (!(det != 0.0) || det != det) return false;          // det == 0 or NaN
    const double sx = o[0] - ax, sy = o[1] - ay, sz = o[2] - az;
    u = ((sx * px + sy * py) + sz * pz) / det;
    const double qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
    v = ((d[0] * qx + d[1] * qy) + d[2] * qz) / det;
    t = ((e2x * qx + e2y * qy) + e2z * qz) / det;
    if (!(u >= 0.0 && v >= 0.0 && (u + v) <= 1.0)) return false;
    return kStrict ? (t > t_lo && t < t_hi) : (t >= t_lo && t <= t_hi);
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------------------
// kAny: return at the first hit.  skip: a vertex index whose faces are not tested (-1: none).  Returns whether something was hit; best
// holds the closest hit when !kAny.
template <bool kAny, bool kStrict>
__device__ __forceinline__ bool ray_walk(const RayGrid& g, const float* __restrict__ vertices, int64_t n_vertices, const int32_t* __restrict__ faces, int64_t n_faces,
                                         const int32_t* __restrict__ offsets, const int32_t* __restrict__ refs, int64_t n_refs, const double o[3], const double d[3],
                                         double t_lo, double t_hi, int32_t skip, RayHit& best) {
#pragma clang fp contract(off)
    best.t = HUGE_VAL; best.u = 0.0; best.v = 0.0; best.face = -1;
    // a NaN or an infinite ray and d = 0 end here, before anything is read (the rule gives them no hit: det is 0, NaN or infinite)
    const double kTop = 1.0e300;
    if (!(fabs(o[0]) < kTop && fabs(o[1]) < kTop && fabs(o[2]) < kTop && fabs(d[0]) < kTop && fabs(d[1]) < kTop && fabs(d[2]) < kTop)) return false;
    if (d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0) return false;
    // clip to the box widened by the margin.  A zero component of d forms no product (no inf * 0): the origin is inside that slab or the
    // ray misses the box.
    double t0 = t_lo, t1 = t_hi, inv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double lo = g.origin[k] - g.margin, hi = (g.origin[k] + (double)g.dims[k] * g.cell) + g.margin;
        if (d[k] == 0.0) {
            inv[k] = 0.0;
            if (!(o[k] >= lo && o[k] <= hi)) return false;
        } else {
            inv[k] = 1.0 / d[k];
            const double ta = (lo - o[k]) * inv[k], tb = (hi - o[k]) * inv[k];
            t0 = fmax(t0, fmin(ta, tb));
            t1 = fmin(t1, fmax(ta, tb));
        }
    }
    if (!(t0 <= t1)) return false;          // the ray misses the box (or the interval is empty, or a bound is NaN)
    // the cell of the entry point, clamped into the grid (the entry point may lie in the margin)
    int idx[3], step[3];
    double t_next[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double at = o[k] + d[k] * t0;          // (t0 is finite here: some component of d is not 0, and its slab bounded it)
        idx[k] = (int)fmin(fmax(floor((at - g.origin[k]) / g.cell), 0.0), (double)(g.dims[k] - 1));
        step[k] = d[k] > 0.0 ? 1 : d[k] < 0.0 ? -1 : 0;
        t_next[k] = step[k] == 0 ? HUGE_VAL : ((g.origin[k] + (double)(idx[k] + (step[k] > 0 ? 1 : 0)) * g.cell) - o[k]) * inv[k];
    }
    // At most nx + ny + nz + 2 steps: every step moves one index by one in a fixed direction and leaves the loop when the index leaves
    // the grid.  Nothing here waits on another thread.
    const int max_steps = g.dims[0] + g.dims[1] + g.dims[2] + 2;
    for (int it = 0; it < max_steps; ++it) {
        const int64_t c = ((int64_t)idx[0] * g.dims[1] + idx[1]) * g.dims[2] + idx[2];          // idx is inside the grid: clamped at entry, tested at each step
        int64_t begin = offsets[c], end = c + 1 < g.n_cells ? (int64_t)offsets[c + 1] : n_refs;
        begin = begin < 0 ? 0 : begin;
        end = end > n_refs ? n_refs : end;
        // bounded by the cell's count; every face index in refs and every vertex index of a listed face was validated when the grid was
        // built (a face that fails the test is listed nowhere), and is tested again against the counts given here
        for (int64_t j = begin; j < end; ++j) {
            const int32_t f = refs[j];
            if (!(f >= 0 && f < n_faces)) continue;
            const int32_t ia = faces[3 * (int64_t)f], ib = faces[3 * (int64_t)f + 1], ic = faces[3 * (int64_t)f + 2];
            if (!(ia >= 0 && ia < n_vertices && ib >= 0 && ib < n_vertices && ic >= 0 && ic < n_vertices)) continue;
            if (ia == skip || ib == skip || ic == skip) continue;
            double t, u, v;
            if (!ray_rule<kStrict>(o, d, vertices, ia, ib, ic, t_lo, t_hi, t, u, v)) continue;
            if (kAny) return true;
            if (best.face < 0 || t < best.t || (t == best.t && f < best.face)) { best.t = t; best.u = u; best.v = v; best.face = f; }
        }
        const int axis = t_next[0] <= t_next[1] ? (t_next[0] <= t_next[2] ? 0 : 2) : (t_next[1] <= t_next[2] ? 1 : 2);
        const double tn = t_next[axis];
        if (!kAny && best.face >= 0 && tn > best.t) break;          // the next cell begins behind the best hit
        if (!(tn <= t1)) break;                                     // the ray leaves the widened box (or its interval ends)
        idx[axis] += step[axis];
        if (idx[axis] < 0 || idx[axis] >= g.dims[axis]) break;
        t_next[axis] = ((g.origin[axis] + (double)(idx[axis] + (step[axis] > 0 ? 1 : 0)) * g.cell) - o[axis]) * inv[axis];
    }
    return best.face >= 0;
}

template <bool kAny>
__global__ void __launch_bounds__(kRayGroup) meshray_cast_kernel(RayGrid g, const float* __restrict__ vertices, int64_t n_vertices, const int32_t* __restrict__ faces,
                                                                 int64_t n_faces, const int32_t* __restrict__ offsets, const int32_t* __restrict__ refs, int64_t n_refs,
                                                                 const float* __restrict__ rays_o, const float* __restrict__ rays_d, int64_t n_rays, double t_min,
                                                                 double t_max, float* __restrict__ t_out, int32_t* __restrict__ face_out, float* __restrict__ u_out,
                                                                 float* __restrict__ v_out, uint8_t* __restrict__ hit_out) {
    const int64_t r = (int64_t)blockIdx.x * kRayGroup + threadIdx.x;
    if (r >= n_rays) return;
    const double o[3] = {(double)rays_o[3 * r], (double)rays_o[3 * r + 1], (double)rays_o[3 * r + 2]};
    const double d[3] = {(double)rays_d[3 * r], (double)rays_d[3 * r + 1], (double)rays_d[3 * r + 2]};
    RayHit best;
    const bool hit = ray_walk<kAny, false>(g, vertices, n_vertices, faces, n_faces, offsets, refs, n_refs, o, d, t_min, t_max, -1, best);
    if (kAny) {
        hit_out[r] = hit ? 1 : 0;
        return;
    }
    t_out[r] = hit ? (float)best.t : __builtin_inff();
    face_out[r] = best.face;
    if (u_out) u_out[r] = (float)best.u;
    if (v_out) v_out[r] = (float)best.v;
}

// One thread per vertex, looping over the set bits of its mask: the lanes of a wave share the view and have neighbouring origins.  The
// centres are staged in LDS; all 256 threads arrive at the barrier.
__global__ void __launch_bounds__(kRayGroup) meshray_occluded_kernel(RayGrid g, const float* __restrict__ vertices, int64_t n_vertices, const int32_t* __restrict__ faces,
                                                                     int64_t n_faces, const int32_t* __restrict__ offsets, const int32_t* __restrict__ refs, int64_t n_refs,
                                                                     const float* __restrict__ centres, int32_t n_views, const unsigned long long* __restrict__ mask_bits,
                                                                     unsigned long long* __restrict__ occluded_bits) {
#pragma clang fp contract(off)
    __shared__ float centre[3 * PERF_MESHRAY_MAX_VIEWS];
    for (int k = threadIdx.x; k < 3 * n_views; k += kRayGroup) centre[k] = centres[k];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kRayGroup + threadIdx.x;
    if (i >= n_vertices) return;
    const unsigned long long low = n_views >= 64 ? ~0ull : (1ull << n_views) - 1ull;
    unsigned long long todo = mask_bits[i] & low, occluded = 0;
    const double o[3] = {(double)vertices[3 * i], (double)vertices[3 * i + 1], (double)vertices[3 * i + 2]};
    while (todo) {          // at most n_views rounds: one bit leaves per round
        const int k = __ffsll(todo) - 1;
        todo &= todo - 1;
        const double d[3] = {(double)centre[3 * k] - o[0], (double)centre[3 * k + 1] - o[1], (double)centre[3 * k + 2] - o[2]};
        RayHit best;
        if (ray_walk<true, true>(g, vertices, n_vertices, faces, n_faces, offsets, refs, n_refs, o, d, 0.0, 1.0, (int32_t)i, best)) occluded |= 1ull << k;
    }
    occluded_bits[i] = occluded;
}

// ---- the checks of the entry points -------------------------------------------------------------------------------------------------------
static int ray_mesh_check(const char* who, const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces) {
    if (int rc = mesh_counts_check(who, n_vertices, n_faces, PERF_MESHRAY_MAX_VERTICES, PERF_MESHRAY_MAX_FACES, "2^31 - 1")) return rc;
    PERF_REQUIRE(vertices || n_vertices == 0, "%s: NULL input (vertices) with vertices", who);
    PERF_REQUIRE(faces || n_faces == 0, "%s: NULL input (faces) with faces", who);
    return PERF_OK;
}

static int ray_grid_check(const char* who, const float* origin, float cell, const int32_t* dims, RayGrid& g) {
    PERF_REQUIRE(origin && dims, "%s: NULL input (origin or dims)", who);
    PERF_REQUIRE(cell > 0.0f && cell <= kRayFltMax, "%s: the cell edge %g is not positive or not finite", who, (double)cell);
    int64_t cells = 1;
    for (int k = 0; k < 3; ++k) {
        PERF_REQUIRE(fabsf(origin[k]) <= kRayFltMax, "%s: origin[%d] = %g is not finite", who, k, (double)origin[k]);
        PERF_REQUIRE(dims[k] >= 1, "%s: dims[%d] = %d is below 1", who, k, dims[k]);
        cells *= dims[k];
        PERF_REQUIRE(cells <= PERF_MESHRAY_MAX_CELLS, "%s: a grid of %d x %d x %d cells has more than 2^24 cells: choose a larger cell", who, dims[0], dims[1], dims[2]);
        g.origin[k] = origin[k];
        g.dims[k] = dims[k];
    }
    g.cell = cell;
    g.margin = (double)cell / 8.0;
    g.n_cells = cells;
    return PERF_OK;
}

static int ray_refs_check(const char* who, const int32_t* offsets, const int32_t* refs, int64_t n_refs) {
    PERF_REQUIRE(n_refs >= 0, "%s: a negative number of references (%lld)", who, (long long)n_refs);
    PERF_REQUIRE(n_refs < ((int64_t)1 << 31), "%s: %lld references are 2^31 or more (the offsets are int32)", who, (long long)n_refs);
    PERF_REQUIRE(offsets, "%s: NULL input (cell_offsets)", who);
    PERF_REQUIRE(refs || n_refs == 0, "%s: NULL input (refs) with references", who);
    return PERF_OK;
}

static inline unsigned ray_groups(int64_t n) { return (unsigned)div_up(n, kRayGroup); }

}  // namespace perf

using namespace perf;

extern "C" int perf_meshray_version(void) { return PERF_MESHRAY_ABI_VERSION; }

extern "C" int perf_meshray_grid_count(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float* origin, float cell,
                                       const int32_t* dims, int32_t* cell_counts, int64_t* bad_face_dev, void* stream) {
    const char* who = "perf_meshray_grid_count";
    RayGrid g;
    if (int rc = ray_mesh_check(who, vertices, n_vertices, faces, n_faces)) return rc;
    if (int rc = ray_grid_check(who, origin, cell, dims, g)) return rc;
    PERF_REQUIRE(cell_counts, "%s: NULL output (cell_counts)", who);
    PERF_REQUIRE(bad_face_dev, "%s: NULL output (bad_face_dev)", who);
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(bad_face_dev, 0xff, sizeof(int64_t), st) != hipSuccess ||          // the flag: no bad face (-1, the largest unsigned)
        hipMemsetAsync(cell_counts, 0, (size_t)g.n_cells * sizeof(int32_t), st) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: clearing the counts and the flag failed", who);
        return PERF_E_LAUNCH;
    }
    if (n_faces > 0)
        hipLaunchKernelGGL(meshray_grid_count_kernel, dim3(ray_groups(n_faces)), dim3(kRayGroup), 0, st, g, vertices, n_vertices, faces, n_faces, cell_counts,
                           (unsigned long long*)bad_face_dev);
    PERF_LAUNCH_CHECK(who);
    return PERF_OK;
}

extern "C" int perf_meshray_grid_write(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float* origin, float cell,
                                       const int32_t* dims, int32_t* cell_counts, const int32_t* cell_offsets, int64_t n_refs_counted, int32_t* refs,
                                       int64_t ref_capacity, void* stream) {
    const char* who = "perf_meshray_grid_write";
    RayGrid g;
    if (int rc = ray_mesh_check(who, vertices, n_vertices, faces, n_faces)) return rc;
    if (int rc = ray_grid_check(who, origin, cell, dims, g)) return rc;
    PERF_REQUIRE(cell_counts, "%s: NULL input (cell_counts)", who);
    PERF_REQUIRE(n_refs_counted >= 0, "%s: a negative number of counted references (%lld)", who, (long long)n_refs_counted);
    PERF_REQUIRE(n_refs_counted < ((int64_t)1 << 31), "%s: %lld references are 2^31 or more (the offsets are int32): choose a larger cell", who,
                 (long long)n_refs_counted);
    PERF_REQUIRE(ref_capacity >= n_refs_counted, "%s: room for %lld references, %lld were counted", who, (long long)ref_capacity, (long long)n_refs_counted);
    PERF_REQUIRE(cell_offsets, "%s: NULL input (cell_offsets)", who);
    PERF_REQUIRE(refs || n_refs_counted == 0, "%s: NULL output (refs) with references to write", who);
    if (n_faces == 0 || n_refs_counted == 0) return PERF_OK;
    hipLaunchKernelGGL(meshray_grid_write_kernel, dim3(ray_groups(n_faces)), dim3(kRayGroup), 0, as_stream(stream), g, vertices, n_vertices, faces, n_faces, cell_counts,
                       cell_offsets, refs, ref_capacity);
    PERF_LAUNCH_CHECK(who);
    return PERF_OK;
}

extern "C" int perf_meshray_cast(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float* origin, float cell, const int32_t* dims,
                                 const int32_t* cell_offsets, const int32_t* refs, int64_t n_refs, const float* rays_o, const float* rays_d, int64_t n_rays, float t_min,
                                 float t_max, int32_t any_hit, float* t_out, int32_t* face_out, float* u_out, float* v_out, uint8_t* hit_out, void* stream) {
    const char* who = "perf_meshray_cast";
    RayGrid g;
    if (int rc = ray_mesh_check(who, vertices, n_vertices, faces, n_faces)) return rc;
    if (int rc = ray_grid_check(who, origin, cell, dims, g)) return rc;
    if (int rc = ray_refs_check(who, cell_offsets, refs, n_refs)) return rc;
    PERF_REQUIRE(n_rays >= 0, "%s: a negative number of rays (%lld)", who, (long long)n_rays);
    PERF_REQUIRE(n_rays <= ((int64_t)1 << 38), "%s: %lld rays are more than 2^38", who, (long long)n_rays);
    PERF_REQUIRE(t_min == t_min && t_max == t_max, "%s: t_min (%g) or t_max (%g) is NaN", who, (double)t_min, (double)t_max);
    PERF_REQUIRE(any_hit == 0 || any_hit == 1, "%s: any_hit (%d) is 0 or 1", who, any_hit);
    PERF_REQUIRE((rays_o && rays_d) || n_rays == 0, "%s: NULL input (rays_o or rays_d) with rays to cast", who);
    if (any_hit)
        PERF_REQUIRE(hit_out || n_rays == 0, "%s: NULL output (hit_out) with rays to cast", who);
    else
        PERF_REQUIRE((t_out && face_out) || n_rays == 0, "%s: NULL output (t_out or face_out) with rays to cast", who);
    if (n_rays == 0) return PERF_OK;
    hipStream_t st = as_stream(stream);
    if (any_hit)
        hipLaunchKernelGGL(meshray_cast_kernel<true>, dim3(ray_groups(n_rays)), dim3(kRayGroup), 0, st, g, vertices, n_vertices, faces, n_faces, cell_offsets, refs, n_refs,
                           rays_o, rays_d, n_rays, (double)t_min, (double)t_max, t_out, face_out, u_out, v_out, hit_out);
    else
        hipLaunchKernelGGL(meshray_cast_kernel<false>, dim3(ray_groups(n_rays)), dim3(kRayGroup), 0, st, g, vertices, n_vertices, faces, n_faces, cell_offsets, refs, n_refs,
                           rays_o, rays_d, n_rays, (double)t_min, (double)t_max, t_out, face_out, u_out, v_out, hit_out);
    PERF_LAUNCH_CHECK(who);
    return PERF_OK;
}

extern "C" int perf_meshray_occluded(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float* origin, float cell,
                                     const int32_t* dims, const int32_t* cell_offsets, const int32_t* refs, int64_t n_refs, const float* centres, int32_t n_views,
                                     const int64_t* mask_bits, int64_t* occluded_bits, void* stream) {
    const char* who = "perf_meshray_occluded";
    RayGrid g;
    if (int rc = ray_mesh_check(who, vertices, n_vertices, faces, n_faces)) return rc;
    if (int rc = ray_grid_check(who, origin, cell, dims, g)) return rc;
    if (int rc = ray_refs_check(who, cell_offsets, refs, n_refs)) return rc;
    PERF_REQUIRE(n_views >= 0, "%s: a negative number of views (%d)", who, n_views);
    PERF_REQUIRE(n_views <= PERF_MESHRAY_MAX_VIEWS, "%s: %d views are more than 64 (a vertex has one bit per view in a 64-bit word)", who, n_views);
    PERF_REQUIRE(centres || n_views == 0, "%s: NULL input (centres) with views", who);
    PERF_REQUIRE(mask_bits || n_vertices == 0, "%s: NULL input (mask_bits) with vertices", who);
    PERF_REQUIRE(occluded_bits || n_vertices == 0, "%s: NULL output (occluded_bits) with vertices", who);
    if (n_vertices == 0) return PERF_OK;
    hipLaunchKernelGGL(meshray_occluded_kernel, dim3(ray_groups(n_vertices)), dim3(kRayGroup), 0, as_stream(stream), g, vertices, n_vertices, faces, n_faces, cell_offsets,
                       refs, n_refs, centres, n_views, (const unsigned long long*)mask_bits, (unsigned long long*)occluded_bits);
    PERF_LAUNCH_CHECK(who);
    return PERF_OK;
}
