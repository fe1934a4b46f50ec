// The closest point of a triangle mesh to each query point (include/staged/perf_hip_meshnear.h), on the uniform grid meshray.hip builds:
// one thread per point, shells of cells of growing Chebyshev radius around the point's cell, the rule of one face the header's, line for
// line, in double; the grid only decides which faces are tested.  No atomics.  This unit includes no public header but its own: what it
// reads of the grid (the box, the cell of a point, a cell's slice of refs) is restated here and held to meshray.hip's by a GPU test.
#include "common.hpp"
#include "mesh_check_host.hpp"
#include "../../include/staged/perf_hip_meshnear.h"
#include <math.h>

#pragma clang fp contract(off)

namespace perf {

constexpr int kNearGroup = 256;              // points of one workgroup: one per thread
constexpr float kNearFltMax = 3.4028234663852886e38f;

struct NearGrid {                            // the caller's box, widened to double on the host (meshray.hip's RayGrid, restated)
    double origin[3];
    double cell;
    int32_t dims[3];
    int64_t n_cells;
};

__device__ __forceinline__ bool near_finite(float x) { return fabsf(x) <= kNearFltMax; }          // (false on a NaN)

// ---- the rule ---------------------------------------------------------------------------------------------------------------------------
struct NearBest {
    double dist2, u, v;
    int32_t face;                            // -1: none
};

__device__ __forceinline__ double near_dot(double xx, double xy, double xz, double yx, double yy, double yz) {
#pragma clang fp contract(off)
    return (xx * yx + xy * yy) + xz * yz;
}

// the header's lines in its order -> false for a face with a vertex that is not finite (never the answer)
__device__ __forceinline__ bool near_rule(const double p[3], const float* __restrict__ vertices, int32_t ia, int32_t ib, int32_t ic, double& dist2, double& u, double& v) {
#pragma clang fp contract(off)
    const float* __restrict__ pa = vertices + 3 * (int64_t)ia;
    const float* __restrict__ pb = vertices + 3 * (int64_t)ib;
    const float* __restrict__ pc = vertices + 3 * (int64_t)ic;
    const float fax = pa[0], fay = pa[1], faz = pa[2], fbx = pb[0], fby = pb[1], fbz = pb[2], fcx = pc[0], fcy = pc[1], fcz = pc[2];
    if (!(near_finite(fax) && near_finite(fay) && near_finite(faz) && near_finite(fbx) && near_finite(fby) && near_finite(fbz) && near_finite(fcx) && near_finite(fcy) &&
          near_finite(fcz)))
        return false;
    const double ax = fax, ay = fay, az = faz;
    const double abx = (double)fbx - ax, aby = (double)fby - ay, abz = (double)fbz - az;
    const double acx = (double)fcx - ax, acy = (double)fcy - ay, acz = (double)fcz - az;
    const double apx = p[0] - ax, apy = p[1] - ay, apz = p[2] - az;
    const double bpx = p[0] - (double)fbx, bpy = p[1] - (double)fby, bpz = p[2] - (double)fbz;
    const double cpx = p[0] - (double)fcx, cpy = p[1] - (double)fcy, cpz = p[2] - (double)fcz;
    const double d1 = near_dot(abx, aby, abz, apx, apy, apz), d2 = near_dot(acx, acy, acz, apx, apy, apz);
    const double d3 = near_dot(abx, aby, abz, bpx, bpy, bpz), d4 = near_dot(acx, acy, acz, bpx, bpy, bpz);
    const double d5 = near_dot(abx, aby, abz, cpx, cpy, cpz), d6 = near_dot(acx, acy, acz, cpx, cpy, cpz);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4, e = d4 - d3, g = d5 - d6;
    const bool at_a = apx == 0.0 && apy == 0.0 && apz == 0.0, at_b = bpx == 0.0 && bpy == 0.0 && bpz == 0.0, at_c = cpx == 0.0 && cpy == 0.0 && cpz == 0.0;
    int corner = -1;                         // 0, 1, 2: the region of the vertex a, b, c
    if (at_a) corner = 0;                                                   // 0
    else if (at_b) corner = 1;
    else if (at_c) corner = 2;
    else if (d1 <= 0.0 && d2 <= 0.0) corner = 0;                             // 1
    else if (d3 >= 0.0 && d4 <= d3) corner = 1;                              // 2
    else if (d6 >= 0.0 && d5 <= d6) corner = 2;                              // 3
    else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0 && (d1 - d3) > 0.0) { u = d1 / (d1 - d3); v = 0.0; }          // 4 (every denominator is tested first)
    else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0 && (d2 - d6) > 0.0) { u = 0.0; v = d2 / (d2 - d6); }          // 5
    else if (va <= 0.0 && e >= 0.0 && g >= 0.0 && (e + g) > 0.0) { v = e / (e + g); u = 1.0 - v; }             // 6
    else if (va > 0.0 && vb > 0.0 && vc > 0.0) { const double den = (va + vb) + vc; u = vb / den; v = vc / den; }          // 7 (den > 0: a sum of three positive terms)
    else {                                                                   // 8
        const double ra = near_dot(apx, apy, apz, apx, apy, apz), rb = near_dot(bpx, bpy, bpz, bpx, bpy, bpz), rc = near_dot(cpx, cpy, cpz, cpx, cpy, cpz);
        corner = 0;
        double least = ra;
        if (rb < least) { corner = 1; least = rb; }
        if (rc < least) corner = 2;
    }
    double rx, ry, rz;
    if (corner == 0) { u = 0.0; v = 0.0; rx = apx; ry = apy; rz = apz; }
    else if (corner == 1) { u = 1.0; v = 0.0; rx = bpx; ry = bpy; rz = bpz; }
    else if (corner == 2) { u = 0.0; v = 1.0; rx = cpx; ry = cpy; rz = cpz; }
    else {
        rx = p[0] - ((ax + u * abx) + v * acx);
        ry = p[1] - ((ay + u * aby) + v * acy);
        rz = p[2] - ((az + u * abz) + v * acz);
    }
    dist2 = near_dot(rx, ry, rz, rx, ry, rz);
    return true;
}

// ---- the search -------------------------------------------------------------------------------------------------------------------------
// every listed face of cell (i, j, k), which is inside the grid.  Bounded by the cell's count; every face index in refs and every vertex
// index of a listed face was validated when the grid was built, and is tested again against the counts given here
__device__ __forceinline__ void near_cell(const NearGrid& g, const float* __restrict__ vertices, int64_t n_vertices, const int32_t* __restrict__ faces, int64_t n_faces,
                                          const int32_t* __restrict__ offsets, const int32_t* __restrict__ refs, int64_t n_refs, const double p[3], int i, int j, int k,
                                          NearBest& best) {
    const int64_t c = ((int64_t)i * g.dims[1] + j) * g.dims[2] + k;
    int64_t begin = offsets[c], end = c + 1 < g.n_cells ? (int64_t)offsets[c + 1] : n_refs;
    begin = begin < 0 ? 0 : begin;
    end = end > n_refs ? n_refs : end;
    for (int64_t s = begin; s < end; ++s) {
        const int32_t f = refs[s];
        if (!(f >= 0 && f < n_faces)) continue;
        const int32_t ia = faces[3 * (int64_t)f], ib = faces[3 * (int64_t)f + 1], ic = faces[3 * (int64_t)f + 2];
        if (!(ia >= 0 && ia < n_vertices && ib >= 0 && ib < n_vertices && ic >= 0 && ic < n_vertices)) continue;
        double dist2, u, v;
        if (!near_rule(p, vertices, ia, ib, ic, dist2, u, v)) continue;
        if (best.face < 0 || dist2 < best.dist2 || (dist2 == best.dist2 && f < best.face)) { best.dist2 = dist2; best.u = u; best.v = v; best.face = f; }
    }
}

__global__ void __launch_bounds__(kNearGroup) meshnear_query_kernel(NearGrid g, const float* __restrict__ vertices, int64_t n_vertices, const int32_t* __restrict__ faces,
                                                                    int64_t n_faces, const int32_t* __restrict__ offsets, const int32_t* __restrict__ refs, int64_t n_refs,
                                                                    const float* __restrict__ points, int64_t n_points, double max_distance, double* __restrict__ dist2_out,
                                                                    int32_t* __restrict__ face_out, float* __restrict__ u_out, float* __restrict__ v_out) {
#pragma clang fp contract(off)
    const int64_t n = (int64_t)blockIdx.x * kNearGroup + threadIdx.x;
    if (n >= n_points) return;
    const float fx = points[3 * n], fy = points[3 * n + 1], fz = points[3 * n + 2];
    NearBest best;
    best.dist2 = HUGE_VAL; best.u = 0.0; best.v = 0.0; best.face = -1;
    // a NaN or an infinite point ends here, before anything is read
    if (near_finite(fx) && near_finite(fy) && near_finite(fz)) {
        const double p[3] = {(double)fx, (double)fy, (double)fz};
        int c0[3];
#pragma unroll
        for (int a = 0; a < 3; ++a)          // the cell of the point, as meshray.hip forms the cell of a ray's entry point: in double, clamped into the grid
            c0[a] = (int)fmin(fmax(floor((p[a] - g.origin[a]) / g.cell), 0.0), (double)(g.dims[a] - 1));
        // At most max(nx, ny, nz) shells: at r = max(nx, ny, nz) - 1 the block is the whole grid.  Every loop below runs over cell indices
        // clamped into the grid, each cell's loop is bounded by its count.  Nothing here waits on another thread.
        const int shells = max(g.dims[0], max(g.dims[1], g.dims[2]));
        for (int r = 0; r < shells; ++r) {
            int lo[3], hi[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = max(c0[a] - r, 0);
                hi[a] = min(c0[a] + r, g.dims[a] - 1);
            }
            // the new cells of shell r: those of the block at Chebyshev distance exactly r from c0
            for (int i = lo[0]; i <= hi[0]; ++i) {
                const bool rim_i = i - c0[0] == r || c0[0] - i == r;
                for (int j = lo[1]; j <= hi[1]; ++j) {
                    // on the rim of i or j the whole column lo[2] .. hi[2]; inside it (r >= 1 there) the two caps c0[2] - r and c0[2] + r, a
                    // stride of 2 r apart, where they are inside the grid (neither: the loop is empty)
                    const bool rim = rim_i || j - c0[1] == r || c0[1] - j == r;
                    const bool below = c0[2] - r >= 0, above = c0[2] + r < g.dims[2];
                    const int k_first = rim ? lo[2] : below ? c0[2] - r : c0[2] + r;
                    const int k_last = rim ? hi[2] : above ? c0[2] + r : c0[2] - r;
                    const int k_step = rim ? 1 : 2 * r;
                    for (int k = k_first; k <= k_last; k += k_step) near_cell(g, vertices, n_vertices, faces, n_faces, offsets, refs, n_refs, p, i, j, k, best);
                }
            }
            // D: the smallest distance, along its own axis, from the point to a side of the block that is not the grid's own boundary.
            // The guard: a face not yet visited lies at least D + m away (m = cell / 8), its computed dist2 exceeds D * D.
            double D = HUGE_VAL;
            bool whole = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (lo[a] > 0) { whole = false; D = fmin(D, p[a] - (g.origin[a] + (double)lo[a] * g.cell)); }
                if (hi[a] < g.dims[a] - 1) { whole = false; D = fmin(D, (g.origin[a] + (double)(hi[a] + 1) * g.cell) - p[a]); }
            }
            if (whole) break;
            D = fmax(D, 0.0);
            if ((best.face >= 0 && best.dist2 <= D * D) || D > max_distance) break;
        }
        if (!(best.face >= 0 && best.dist2 <= max_distance * max_distance)) { best.dist2 = HUGE_VAL; best.u = 0.0; best.v = 0.0; best.face = -1; }
    }
    dist2_out[n] = best.dist2;
    face_out[n] = best.face;
    if (u_out) u_out[n] = (float)best.u;
    if (v_out) v_out[n] = (float)best.v;
}

// ---- the checks of the entry point: meshray.hip's, with its messages -----------------------------------------------------------------------
static int near_grid_check(const char* who, const float* origin, float cell, const int32_t* dims, NearGrid& g) {
    PERF_REQUIRE(origin && dims, "%s: NULL input (origin or dims)", who);
    PERF_REQUIRE(cell > 0.0f && cell <= kNearFltMax, "%s: the cell edge %g is not positive or not finite", who, (double)cell);
    int64_t cells = 1;
    for (int k = 0; k < 3; ++k) {
        PERF_REQUIRE(fabsf(origin[k]) <= kNearFltMax, "%s: origin[%d] = %g is not finite", who, k, (double)origin[k]);
        PERF_REQUIRE(dims[k] >= 1, "%s: dims[%d] = %d is below 1", who, k, dims[k]);
        cells *= dims[k];
        PERF_REQUIRE(cells <= PERF_MESHNEAR_MAX_CELLS, "%s: a grid of %d x %d x %d cells has more than 2^24 cells: choose a larger cell", who, dims[0], dims[1], dims[2]);
        g.origin[k] = origin[k];
        g.dims[k] = dims[k];
    }
    g.cell = cell;
    g.n_cells = cells;
    return PERF_OK;
}

}  // namespace perf

using namespace perf;

extern "C" int perf_meshnear_version(void) { return PERF_MESHNEAR_ABI_VERSION; }

extern "C" int perf_meshnear_query(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float* origin, float cell, const int32_t* dims,
                                   const int32_t* cell_offsets, const int32_t* refs, int64_t n_refs, const float* points, int64_t n_points, float max_distance,
                                   double* dist2_out, int32_t* face_out, float* u_out, float* v_out, void* stream) {
    const char* who = "perf_meshnear_query";
    NearGrid g;
    if (int rc = mesh_counts_check(who, n_vertices, n_faces, PERF_MESHNEAR_MAX_VERTICES, PERF_MESHNEAR_MAX_FACES, "2^31 - 1")) return rc;
    PERF_REQUIRE(vertices || n_vertices == 0, "%s: NULL input (vertices) with vertices", who);
    PERF_REQUIRE(faces || n_faces == 0, "%s: NULL input (faces) with faces", who);
    if (int rc = near_grid_check(who, origin, cell, dims, g)) return rc;
    PERF_REQUIRE(n_refs >= 0, "%s: a negative number of references (%lld)", who, (long long)n_refs);
    PERF_REQUIRE(n_refs < ((int64_t)1 << 31), "%s: %lld references are 2^31 or more (the offsets are int32)", who, (long long)n_refs);
    PERF_REQUIRE(cell_offsets, "%s: NULL input (cell_offsets)", who);
    PERF_REQUIRE(refs || n_refs == 0, "%s: NULL input (refs) with references", who);
    PERF_REQUIRE(n_points >= 0, "%s: a negative number of points (%lld)", who, (long long)n_points);
    PERF_REQUIRE(n_points <= ((int64_t)1 << 38), "%s: %lld points are more than 2^38", who, (long long)n_points);
    PERF_REQUIRE(max_distance >= 0.0f, "%s: max_distance (%g) is NaN or negative", who, (double)max_distance);
    PERF_REQUIRE(points || n_points == 0, "%s: NULL input (points) with points to query", who);
    PERF_REQUIRE((dist2_out && face_out) || n_points == 0, "%s: NULL output (dist2_out or face_out) with points to query", who);
    if (n_points == 0) return PERF_OK;
    hipLaunchKernelGGL(meshnear_query_kernel, dim3((unsigned)div_up(n_points, kNearGroup)), dim3(kNearGroup), 0, as_stream(stream), g, vertices, n_vertices, faces,
                       n_faces, cell_offsets, refs, n_refs, points, n_points, (double)max_distance, dist2_out, face_out, u_out, v_out);
    PERF_LAUNCH_CHECK(who);
    return PERF_OK;
}
