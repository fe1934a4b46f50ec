// Quadric error placement of the clusters' vertices (include/perf_hip_meshquadric.h): sums (one thread per face, int64 fixed point,
// return-less integer atomics) -> place (one thread per cluster, a 3 x 3 solve by cofactors).  The header states the rule line for line;
// the kernels follow it in its order.
#include "common.hpp"
#include "mesh_check_host.hpp"
#include "../../include/perf_hip_meshquadric.h"

namespace perf {

constexpr int kQdGroup = 256;
constexpr int kQdTerms = PERF_MESHQUADRIC_TERMS;
constexpr double kQdScale = 1099511627776.0;                 // 2^40
constexpr double kQdInvScale = 1.0 / 1099511627776.0;        // 2^-40 (exact)
constexpr double kQdSkip = 1152921504606846976.0;            // 2^60
constexpr double kQdRegulariser = 1.0 / 1024.0;              // 2^-10

struct QdGrid {
    double lo[3];
    double h;
    int32_t n[3];
};

// The cell rule, one axis of a FINITE coordinate: i the cell, f the fraction in it.
__device__ __forceinline__ void qd_cell(float x, const QdGrid& g, int a, int64_t& i, double& f) {
#pragma clang fp contract(off)
    const double n = (double)g.n[a];
    double t = ((double)x - g.lo[a]) / g.h;
    t = t > 0.0 ? t : 0.0;
    t = t < n ? t : n;
    i = (int64_t)floor(t);
    if (i > g.n[a] - 1) i = g.n[a] - 1;
    f = t - (double)i;
}

// kSkipZeros: a term that is zero is not sent (adding zero changes no sum: a face in an axis plane has two terms of nine).
template <bool kSkipZeros>
__device__ __forceinline__ void qd_add_row(unsigned long long* __restrict__ acc, int32_t c, const int64_t q[kQdTerms]) {
    unsigned long long* row = acc + (int64_t)kQdTerms * c;
    for (int k = 0; k < kQdTerms; ++k)
        if (!kSkipZeros || q[k] != 0) atomicAdd(row + k, (unsigned long long)q[k]);          // (the result is not used: return-less)
}

// Stage A for one face, steps 1 to 5 of the header: -> whether the face contributes; cl [3] its corners' clusters, q [3][9] the corners' integers.
__device__ __forceinline__ bool qd_face(const float* __restrict__ vertices, int64_t n_vertices, const int32_t* __restrict__ faces, int64_t face, const QdGrid& g,
                                        const int32_t* __restrict__ vertex_cluster, int64_t n_clusters, unsigned long long* __restrict__ first_bad,
                                        unsigned long long* __restrict__ first_skipped, int32_t cl[3], int64_t q[3][kQdTerms]) {
#pragma clang fp contract(off)
    int64_t abc[3];
    for (int k = 0; k < 3; ++k) abc[k] = faces[3 * face + k];
    if (abc[0] < 0 || abc[0] >= n_vertices || abc[1] < 0 || abc[1] >= n_vertices || abc[2] < 0 || abc[2] >= n_vertices) {
        atomicMin(first_bad, (unsigned long long)face);
        return false;
    }
    for (int k = 0; k < 3; ++k) cl[k] = vertex_cluster[abc[k]];
    if (cl[0] < 0 || cl[0] >= n_clusters || cl[1] < 0 || cl[1] >= n_clusters || cl[2] < 0 || cl[2] >= n_clusters) return false;
    float p[3][3];
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) p[k][a] = vertices[3 * abc[k] + a];
    double e1[3], e2[3];
    for (int a = 0; a < 3; ++a) {
        e1[a] = ((double)p[1][a] - (double)p[0][a]) / g.h;
        e2[a] = ((double)p[2][a] - (double)p[0][a]) / g.h;
    }
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double scaled[6] = {(n[0] * n[0]) * kQdScale, (n[0] * n[1]) * kQdScale, (n[0] * n[2]) * kQdScale,
                              (n[1] * n[1]) * kQdScale, (n[1] * n[2]) * kQdScale, (n[2] * n[2]) * kQdScale};
    bool fits = true;
    for (int k = 0; k < 6; ++k) fits = fits && fabs(scaled[k]) < kQdSkip;          // (false for a NaN and for an infinity)
    if (!fits) {
        atomicMin(first_skipped, (unsigned long long)face);
        return false;
    }
    for (int k = 0; k < 3; ++k) {
        double r[3];
        for (int a = 0; a < 3; ++a) {
            int64_t i;
            double f;
            qd_cell(p[k][a], g, a, i, f);          // (finite: the vertex has a cluster)
            r[a] = f - 0.5;
        }
        const double d = (n[0] * r[0] + n[1] * r[1]) + n[2] * r[2];
        for (int j = 0; j < 6; ++j) q[k][j] = (int64_t)llrint(scaled[j]);
        for (int a = 0; a < 3; ++a) q[k][6 + a] = (int64_t)llrint((n[a] * d) * kQdScale);          // (|n_a d| * 2^40 < 1.5 * 2^60)
    }
    return true;
}

// Stage A.  One thread per face; nothing waits on another thread and there is no loop but the fixed ones over three axes, nine terms and
// the six steps of the wave's scan.
__global__ void __launch_bounds__(kQdGroup) meshquadric_sums_kernel(const float* __restrict__ vertices, int64_t n_vertices, const int32_t* __restrict__ faces,
                                                                    int64_t n_faces, QdGrid g, const int32_t* __restrict__ vertex_cluster, int64_t n_clusters,
                                                                    unsigned long long* __restrict__ acc, unsigned long long* __restrict__ first_bad,
                                                                    unsigned long long* __restrict__ first_skipped) {
    const int64_t face = (int64_t)blockIdx.x * kQdGroup + threadIdx.x;
    int32_t cl[3] = {-1, -1, -1};
    int64_t q[3][kQdTerms];
#ifdef PERF_MESHQUADRIC_PLAIN_SUMS
    // The plain form, kept to be measured against (profiles/meshquadric.json has both): every face goes to memory on its own.
    if (face >= n_faces || !qd_face(vertices, n_vertices, faces, face, g, vertex_cluster, n_clusters, first_bad, first_skipped, cl, q)) return;
    if (cl[0] == cl[1] && cl[1] == cl[2]) {          // the common case at a cell of two spacings or more: 9 atomics, not 27
        for (int j = 0; j < kQdTerms; ++j) q[0][j] = (int64_t)((uint64_t)q[0][j] + (uint64_t)q[1][j] + (uint64_t)q[2][j]);
        qd_add_row<false>(acc, cl[0], q[0]);
    } else {
        for (int k = 0; k < 3; ++k) qd_add_row<false>(acc, cl[k], q[k]);
    }
#else
    // The faces of a wave that follow one another wholly inside one cluster are summed along the wave (a segmented scan of six steps:
    // integers, exact in any grouping) and the run's last lane sends the run's nine sums.  Every lane arrives at the shuffles.
    const bool live = face < n_faces && qd_face(vertices, n_vertices, faces, face, g, vertex_cluster, n_clusters, first_bad, first_skipped, cl, q);
    const bool whole = live && cl[0] == cl[1] && cl[1] == cl[2];
    const int32_t id = whole ? cl[0] : -1 - (int32_t)(threadIdx.x & 63);          // (a lane that joins no run: an id no neighbour has)
    uint64_t s[kQdTerms];
    for (int j = 0; j < kQdTerms; ++j) s[j] = whole ? (uint64_t)q[0][j] + (uint64_t)q[1][j] + (uint64_t)q[2][j] : 0;
    const int lane = threadIdx.x & 63;
    const int32_t before = __shfl_up(id, 1), after = __shfl_down(id, 1);
    const uint64_t heads = __ballot(lane == 0 || before != id);
    const int head = 63 - __clzll((long long)(heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1))));
    const bool tail = lane == 63 || after != id;
    for (int step = 1; step < 64; step <<= 1)
        for (int j = 0; j < kQdTerms; ++j) {
            const uint64_t other = (uint64_t)__shfl_up((long long)s[j], step);
            if (lane - step >= head) s[j] += other;
        }
    if (whole && tail) {
        int64_t sum[kQdTerms];
        for (int j = 0; j < kQdTerms; ++j) sum[j] = (int64_t)s[j];
        qd_add_row<true>(acc, cl[0], sum);
    }
    if (live && !whole) {          // two or three clusters: the two corners that share one go together, 18 atomics at the most, not 27
        const bool ab = cl[0] == cl[1], ac = cl[0] == cl[2], bc = cl[1] == cl[2];          // (at most one of them: the face is not whole)
        for (int j = 0; j < kQdTerms; ++j) {          // (static indices only: the arrays stay in registers)
            if (ab) q[0][j] = (int64_t)((uint64_t)q[0][j] + (uint64_t)q[1][j]);
            if (ac) q[0][j] = (int64_t)((uint64_t)q[0][j] + (uint64_t)q[2][j]);
            if (bc) q[1][j] = (int64_t)((uint64_t)q[1][j] + (uint64_t)q[2][j]);
        }
        qd_add_row<true>(acc, cl[0], q[0]);
        if (!ab) qd_add_row<true>(acc, cl[1], q[1]);
        if (!ac && !bc) qd_add_row<true>(acc, cl[2], q[2]);
    }
#endif
}

// Stage B.  One thread per cluster.
__global__ void __launch_bounds__(kQdGroup) meshquadric_place_kernel(const float* __restrict__ vertices, int64_t n_vertices, QdGrid g, const float* anchor,
                                                                     const int32_t* __restrict__ representative, const int64_t* __restrict__ acc,
                                                                     int64_t n_clusters, float* cluster_vertices) {
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * kQdGroup + threadIdx.x;
    if (c >= n_clusters) return;
    const float a0 = anchor[3 * c], a1 = anchor[3 * c + 1], a2 = anchor[3 * c + 2];          // (read before the row is written: anchor may be the output)
    float out[3] = {a0, a1, a2};
    double t[kQdTerms];
    for (int k = 0; k < kQdTerms; ++k) t[k] = (double)acc[kQdTerms * c + k] * kQdInvScale;
    const double Axx = t[0], Axy = t[1], Axz = t[2], Ayy = t[3], Ayz = t[4], Azz = t[5];
    const double tr = (Axx + Ayy) + Azz;
    const int64_t rep = representative[c];
    bool ok = tr > 0.0 && rep >= 0 && rep < n_vertices;
    float v[3] = {0.0f, 0.0f, 0.0f};
    if (ok)
        for (int a = 0; a < 3; ++a) {
            v[a] = vertices[3 * rep + a];
            ok = ok && __builtin_isfinite(v[a]);
        }
    if (ok) {
        double cell[3], m[3];
        for (int a = 0; a < 3; ++a) {
            int64_t i;
            double f;
            qd_cell(v[a], g, a, i, f);
            cell[a] = (double)i + 0.5;
            m[a] = ((double)out[a] - g.lo[a]) / g.h - cell[a];
        }
        const double lambda = tr * kQdRegulariser;
        const double Mxx = Axx + lambda, Myy = Ayy + lambda, Mzz = Azz + lambda, Mxy = Axy, Mxz = Axz, Myz = Ayz;
        const double gx = t[6] + lambda * m[0], gy = t[7] + lambda * m[1], gz = t[8] + lambda * m[2];
        const double c00 = Myy * Mzz - Myz * Myz;
        const double c01 = Mxz * Myz - Mxy * Mzz;
        const double c02 = Mxy * Myz - Mxz * Myy;
        const double c11 = Mxx * Mzz - Mxz * Mxz;
        const double c12 = Mxy * Mxz - Mxx * Myz;
        const double c22 = Mxx * Myy - Mxy * Mxy;
        const double det = (Mxx * c00 + Mxy * c01) + Mxz * c02;
        if (det > 0.0 && __builtin_isfinite(det)) {
            double x[3] = {((c00 * gx + c01 * gy) + c02 * gz) / det, ((c01 * gx + c11 * gy) + c12 * gz) / det, ((c02 * gx + c12 * gy) + c22 * gz) / det};
            if (__builtin_isfinite(x[0]) && __builtin_isfinite(x[1]) && __builtin_isfinite(x[2]))
                for (int a = 0; a < 3; ++a) {
                    x[a] = x[a] > -0.5 ? x[a] : -0.5;
                    x[a] = x[a] < 0.5 ? x[a] : 0.5;
                    out[a] = (float)(g.lo[a] + (cell[a] + x[a]) * g.h);
                }
        }
    }
    cluster_vertices[3 * c] = out[0];
    cluster_vertices[3 * c + 1] = out[1];
    cluster_vertices[3 * c + 2] = out[2];
}

static int qd_grid_check(const char* who, const float* lo, float h, int32_t nx, int32_t ny, int32_t nz, QdGrid* grid) {
    PERF_REQUIRE(lo, "%s: NULL input (lo)", who);
    PERF_REQUIRE(std::isfinite(lo[0]) && std::isfinite(lo[1]) && std::isfinite(lo[2]), "%s: the grid's origin lo is not finite", who);
    PERF_REQUIRE(std::isfinite(h) && h > 0.0f, "%s: the cell edge h (%g) is not positive or not finite", who, (double)h);
    const int32_t n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        PERF_REQUIRE(n[a] >= 1 && n[a] <= PERF_MESHQUADRIC_MAX_CELLS, "%s: %d cells along axis %d are outside 1 .. 2^21", who, (int)n[a], a);
        grid->lo[a] = (double)lo[a];
        grid->n[a] = n[a];
    }
    grid->h = (double)h;
    return PERF_OK;
}

static int qd_clusters_check(const char* who, int64_t n_clusters, int64_t n_vertices) {
    PERF_REQUIRE(n_clusters >= 0, "%s: a negative number of clusters (%lld)", who, (long long)n_clusters);
    PERF_REQUIRE(n_clusters <= n_vertices, "%s: %lld clusters, the mesh has %lld vertices", who, (long long)n_clusters, (long long)n_vertices);
    return PERF_OK;
}

}  // namespace perf

using namespace perf;

extern "C" int perf_meshquadric_version(void) { return PERF_MESHQUADRIC_ABI_VERSION; }

extern "C" int perf_meshquadric_sums(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float* lo, float h, int32_t nx,
                                     int32_t ny, int32_t nz, const int32_t* vertex_cluster, int64_t n_clusters, int64_t* acc, int64_t* bad_face_dev,
                                     int64_t* skipped_face_dev, void* stream) {
    const char* who = "perf_meshquadric_sums";
    QdGrid grid;
    if (int rc = mesh_counts_check(who, n_vertices, n_faces, PERF_MESHQUADRIC_MAX_VERTICES, PERF_MESHQUADRIC_MAX_FACES, "2^31 - 1")) return rc;
    if (int rc = qd_clusters_check(who, n_clusters, n_vertices)) return rc;
    if (int rc = qd_grid_check(who, lo, h, nx, ny, nz, &grid)) return rc;
    PERF_REQUIRE((vertices && vertex_cluster) || n_vertices == 0, "%s: NULL input (vertices or vertex_cluster) with vertices", who);
    PERF_REQUIRE(faces || n_faces == 0, "%s: NULL input (faces) with faces to sum", who);
    PERF_REQUIRE(acc || n_clusters == 0, "%s: NULL output (acc) with clusters to sum into", who);
    PERF_REQUIRE(bad_face_dev && skipped_face_dev, "%s: NULL output (bad_face_dev or skipped_face_dev)", who);
    hipStream_t st = as_stream(stream);
    // the flags: no such face (-1, the largest unsigned); the sums: zero
    if (hipMemsetAsync(bad_face_dev, 0xff, sizeof(int64_t), st) != hipSuccess || hipMemsetAsync(skipped_face_dev, 0xff, sizeof(int64_t), st) != hipSuccess ||
        (n_clusters > 0 && hipMemsetAsync(acc, 0, sizeof(int64_t) * kQdTerms * (size_t)n_clusters, st) != hipSuccess)) {
        (void)hipGetLastError();
        set_error("%s: clearing the flags and the sums failed", who);
        return PERF_E_LAUNCH;
    }
    if (n_faces == 0) return PERF_OK;
    hipLaunchKernelGGL(meshquadric_sums_kernel, dim3((unsigned)div_up(n_faces, kQdGroup)), dim3(kQdGroup), 0, st, vertices, n_vertices, faces, n_faces, grid,
                       vertex_cluster, n_clusters, (unsigned long long*)acc, (unsigned long long*)bad_face_dev, (unsigned long long*)skipped_face_dev);
    PERF_LAUNCH_CHECK(who);
    return PERF_OK;
}

extern "C" int perf_meshquadric_place(const float* vertices, int64_t n_vertices, const float* lo, float h, int32_t nx, int32_t ny, int32_t nz, const float* anchor,
                                      const int32_t* representative, const int64_t* acc, int64_t n_clusters, float* cluster_vertices, void* stream) {
    const char* who = "perf_meshquadric_place";
    QdGrid grid;
    if (int rc = mesh_counts_check(who, n_vertices, 0, PERF_MESHQUADRIC_MAX_VERTICES, PERF_MESHQUADRIC_MAX_FACES, "2^31 - 1")) return rc;
    if (int rc = qd_clusters_check(who, n_clusters, n_vertices)) return rc;
    if (int rc = qd_grid_check(who, lo, h, nx, ny, nz, &grid)) return rc;
    PERF_REQUIRE(vertices || n_vertices == 0, "%s: NULL input (vertices) with vertices", who);
    PERF_REQUIRE((anchor && representative && acc) || n_clusters == 0, "%s: NULL input (anchor, representative or acc) with clusters to place", who);
    PERF_REQUIRE(cluster_vertices || n_clusters == 0, "%s: NULL output (cluster_vertices) with clusters to place", who);
    if (n_clusters == 0) return PERF_OK;
    hipLaunchKernelGGL(meshquadric_place_kernel, dim3((unsigned)div_up(n_clusters, kQdGroup)), dim3(kQdGroup), 0, as_stream(stream), vertices, n_vertices, grid,
                       anchor, representative, acc, n_clusters, cluster_vertices);
    PERF_LAUNCH_CHECK(who);
    return PERF_OK;
}
